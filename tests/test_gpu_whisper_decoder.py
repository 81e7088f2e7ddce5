"""GPU: the Whisper text decoder -- ssak_dec_embed, ssak_dec_attention_fwd, ssak_token_logprobs (ssak_amd/csrc/whisper_decoder.hip)
and their composition ssak_amd/whisper_seq2seq.py -- against the float64 restatement tests/whisper_decoder_ref.py (itself held to
transformers in float64 by tests/test_whisper_decoder_ref.py) and the fixture tests/golden/whisper_dec_tiny.npz.  Every case
prints its distances before it asserts.

Bars.  u8 = 2^-8 (one bf16 rounding moves a value by at most 2^-8 of itself), u = 2^-24 (fp32).  References run on the kernels'
own bf16 inputs.

* ssak_dec_attention_fwd, per element of ctx.  ctx_mag = sum_j P_j |v_j|.  P is rounded to bf16 into the second MFMA (u8 ctx_mag)
  and ctx is stored as bf16 (u8 |ctx| <= u8 ctx_mag).  Exponent errors, relative to each probability: the 64-term MFMA score sum
  (two roundings against amax = max_j sum_d |q k| / 8), the multiplication by log2 e, the subtraction of the running maximum and
  v_exp_f32 give <= 4 u (amax log2 e + 1) ~ u (6 amax + 4); the maximum is subtracted once in a wave's tile and once where the four
  waves' partials meet, each a rounding of a value up to |smax| log2 e (smax = the row's largest |score|): 2 u smax more.  A tile
  whose maximum does not move is rescaled by exp2(0) = 1 exactly.  eta = u (6 amax + 2 smax + 4) enters numerator and row sum.
  The fp32 accumulations (one per 32-key tile and wave, four at the merge, in O and in the row sum) add (ceil(Lk / 32) + 8) u each.
      bar = ctx_mag (2 u8 + 2 eta + 2 (ceil(Lk / 32) + 8) u)
  The integer-exact case (every product and sum exact, every probability exactly 1) must equal bf16(fl(sum v) / fl(count)) to
  within the division: one bf16 ulp.
* ssak_dec_embed: bf16(fp32(e) + fp32(p)), one rounding, defined bit for bit -- exact.
* ssak_token_logprobs.  D = max_c |x_c - max x|; each exp costs its argument's rounding (D u) and expf's ulp (2 u); the sum of the
  n terms runs as per-thread partials (ceil(n / 256) terms), a 6-step wave tree and 4 waves: K = ceil(n / 256) + 10 additions on
  any path, K u of sum|terms| = K u s as all terms are positive.  rel = (4 D + K + 6) u bounds the relative error of the row sum
  and of each probability (numerator and denominator, one division):
      bar_p = rel p;   bar_lse = rel + 2 u (|log s| + |m| + |lse|);   bar_logprob = bar_lse + 2 u (|x_t| + |logprob|)
  arg-max is a selection: exact, the lowest id on a tie.
* The golden through WhisperSeq2Seq.  Logits: the project's bf16 bar, 2e-2 relative L2 per utterance.  Token log-probs, losses and
  language probabilities: measured on the CPU as the restatement evaluated with the device's storage roundings (bf16 weights --
  exact here --, activations, residual stream, P and ctx) minus the restatement in float64, the largest distance over the tensor;
  the test allows 4 x that (the bf16 GEMM's summation order differs from NumPy's, LayerNorm statistics and GELU are fp32 on the
  device).  The measured distances and the bars are printed by the test and recorded in DESIGN.md ("Whisper decoder").
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_decoder_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8, U = 2.0 ** -8, 2.0 ** -24
NH, D = 2, 128
B = 3


@pytest.fixture(scope="module")
def hip():
    import ssak_amd.hip as hip
    return hip


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


def dev_bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(DEV)


# ------------------------------------------------------------------------------------------------------------ 1. attention
def attn_inputs(Lq, Lk, klens, seed, poison=True):
    """float64 q [B, Lq, D], k / v [B, Lk, D] holding bf16 values; K / V rows at keys >= klens[b] poisoned (K aligned with a query,
    V = +-1000): a leaked key is a gross error, not a 1 / klen one."""
    rng = np.random.default_rng(seed)
    q, k, v = (WR.bf16_round(rng.standard_normal((B, n, D)) * s) for n, s in ((Lq, 0.8), (Lk, 0.8), (Lk, 1.0)))
    if poison and klens is not None:
        for b, kl in enumerate(klens):
            if kl < Lk:
                k[b, kl:] = WR.bf16_round(2 * q[b, 0])
                v[b, kl:] = 1000.0 * (rng.integers(0, 2, (Lk - kl, D)) * 2 - 1)
    return q, k, v


def run_attention(hip, q, k, v, klens, causal, q_offset, packed):
    """The kernel on strided views.  ``packed``: q | k | v as column blocks of one [B * L, 3 D] buffer (self-attention); otherwise q
    in a [B * Lq, D + 8] buffer and k, v in one [B * Lk, 2 D + 24] buffer at columns 8 and D + 24, the gaps NaN: row strides
    wider than D, separate pointers."""
    Lq, Lk = q.shape[1], k.shape[1]
    if packed:
        buf = dev_bf16(np.concatenate([q, k, v], -1).reshape(B * Lq, 3 * D))
        qd, kd, vd = buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:]
    else:
        qb = torch.full((B * Lq, D + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
        kvb = torch.full((B * Lk, 2 * D + 24), float("nan"), dtype=torch.bfloat16, device=DEV)
        qd, kd, vd = qb[:, :D], kvb[:, 8:8 + D], kvb[:, D + 24:]
        qd.copy_(dev_bf16(q.reshape(B * Lq, D)))
        kd.copy_(dev_bf16(k.reshape(B * Lk, D)))
        vd.copy_(dev_bf16(v.reshape(B * Lk, D)))
    ctx = torch.full((B * Lq, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.dec_attention_fwd(qd, kd, vd, B, Lq, Lk, NH, klens=klens, causal=causal, q_offset=q_offset, ctx=ctx)
    torch.cuda.synchronize()
    return ctx.double().cpu().numpy().reshape(B, Lq, D)


def check_attention(hip, name, Lq, Lk, klens, causal, q_offset, packed, seed):
    q, k, v = attn_inputs(Lq, Lk, klens, seed, poison=not causal)
    got = run_attention(hip, q, k, v, klens, causal, q_offset, packed)
    ref, st = WR.attention(q, k, v, NH, klens, causal, q_offset, stats=True)
    rows = lambda x: np.repeat(x.transpose(0, 2, 1), WR.HEAD_DIM, axis=-1)  # [B, nh, Lq] -> [B, Lq, D]
    eta = U * (6 * rows(st["amax"]) + 2 * rows(st["smax"]) + 4)
    bar = st["ctx_mag"] * (2 * U8 + 2 * eta + 2 * (math.ceil(Lk / 32) + 8) * U)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bar, 1e-300)).max())
    print(f"attention {name}: Lq={Lq} Lk={Lk} klens={klens} causal={causal} q_offset={q_offset}: max err {err.max():.3e}, worst err/bar {worst:.3f}")
    assert np.isfinite(got).all(), name
    assert (err <= bar).all(), (name, worst)


@pytest.mark.parametrize("Lq", [1, 5, 16, 17])
@pytest.mark.parametrize("Lk", [1, 50, 131])
def test_cross_attention_against_float64(hip, Lq, Lk):
    """One, partial and several 32-key tiles against one, partial and two 16-query tiles; per-utterance key counts (Lk, 1,
    Lk // 2 + 1) with the keys past them poisoned; separate k / v pointers, row strides wider than D."""
    check_attention(hip, "cross", Lq, Lk, (Lk, 1, Lk // 2 + 1), False, 0, False, seed=100 * Lq + Lk)


@pytest.mark.parametrize("Lq,Lk,q_offset", [(37, 37, 0), (5, 12, 7), (1, 8, 7)], ids=["whole", "offset", "cached-step"])
def test_causal_attention_against_float64(hip, Lq, Lk, q_offset):
    """The diagonal inside a tile, a partial last query tile and a partial key tile (37); queries that start at key 7; the
    incremental step of a cached decode (one query at position 7 of 8 keys).  q, k, v are column blocks of one packed buffer."""
    if Lq == Lk:
        check_attention(hip, "causal", Lq, Lk, None, True, q_offset, True, seed=Lq)
    else:
        check_attention(hip, "causal", Lq, Lk, None, True, q_offset, False, seed=Lq + 50)
    # and with key lengths on top of the causal mask (the host refuses none of them: every query still sees key 0)
    check_attention(hip, "causal+klens", Lq, Lk, (Lk, 1, Lk // 2 + 1), True, q_offset, False, seed=Lq + 99)


def test_attention_integer_exact(hip):
    """Small-integer q, k, v: every product and sum is exact in bf16 / fp32.  All keys of an (utterance, head) are one row, so all
    visible scores of a query are equal and every probability is exactly 1: ctx = bf16(fl(sum v) / fl(count)), exact up to the
    division.  Causal Lq = Lk = 37 (counts 1 .. 37, several tiles and waves) and cross Lk = 131 with klens."""
    rng = np.random.default_rng(7)
    for causal, Lq, Lk, klens in ((True, 37, 37, None), (False, 17, 131, (131, 1, 66))):
        q = rng.integers(-2, 3, (B, Lq, D)).astype(np.float64)
        k = np.repeat(rng.integers(-2, 3, (B, 1, D)), Lk, axis=1).astype(np.float64)
        v = rng.integers(-4, 5, (B, Lk, D)).astype(np.float64)
        got = run_attention(hip, q, k, v, klens, causal, 0, causal)
        want = np.zeros_like(got)
        for b in range(B):
            for i in range(Lq):
                n = min(Lk if klens is None else klens[b], i + 1 if causal else Lk)
                s = torch.from_numpy(v[b, :n].sum(0)).float()
                want[b, i] = (s / torch.tensor(float(n))).to(torch.bfloat16).double().numpy()
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -126))) - 7)
        err = np.abs(got - want)
        print(f"attention integer-exact causal={causal}: {int((err > 0).sum())} of {err.size} elements differ from the correctly rounded "
              f"quotient, max {float((err / ulp).max()):.2f} ulp")
        assert (err <= ulp).all()


def test_attention_refusals(hip):
    q, k, v = (dev_bf16(np.zeros((B * 4, D))) for _ in range(3))
    with pytest.raises(ValueError, match="64"):
        hip.dec_attention_fwd(q, k, v, B, 4, 4, 4, head_dim=32)
    with pytest.raises(ValueError, match="klens"):
        hip.dec_attention_fwd(q, k, v, B, 4, 4, NH, klens=(4, 0, 2))
    with pytest.raises(ValueError, match="klens"):
        hip.dec_attention_fwd(q, k, v, B, 4, 4, NH, klens=(4, 5, 2))


# ------------------------------------------------------------------------------------------------------------ 2. embedding
@pytest.mark.parametrize("pos_offset", [0, 5])
def test_embed_is_exact(hip, pos_offset):
    g = torch.Generator().manual_seed(3)
    V, P, L = 50, 32, 7
    E = torch.randn(V, D, generator=g).to(torch.bfloat16)
    Pz = torch.randn(P, D, generator=g).to(torch.bfloat16)
    ids = torch.randint(0, V, (2, L), generator=g)
    ids[0, 0], ids[1, -1] = 0, V - 1
    got = hip.dec_embed(E.to(DEV), Pz.to(DEV), ids, pos_offset).cpu()
    want = (E[ids].float() + Pz[pos_offset:pos_offset + L].float()[None]).to(torch.bfloat16).reshape(2 * L, D)
    print(f"embed pos_offset={pos_offset}: {int((got.view(torch.int16) != want.view(torch.int16)).sum())} elements differ")
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_embed_refuses_bad_ids_and_position_overrun(hip):
    V, P, L = 50, 32, 7
    E, Pz = dev_bf16(np.ones((V, D))), dev_bf16(np.ones((P, D)))
    out = torch.full((2 * L, D), 7.0, dtype=torch.bfloat16, device=DEV)
    for bad in (V, -1):
        ids = np.zeros((2, L), dtype=np.int64)
        ids[1, 3] = bad
        with pytest.raises(ValueError, match="id"):
            hip.dec_embed(E, Pz, ids, 0, out=out)
    with pytest.raises(ValueError, match="overrun"):
        hip.dec_embed(E, Pz, np.zeros((2, L), dtype=np.int64), P - L + 1, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call launched"
    hip.dec_embed(E, Pz, np.zeros((2, L), dtype=np.int64), P - L, out=out)  # the last positions of the table are fine
    assert bool((out == 2.0).all())


# ------------------------------------------------------------------------------------------------------------ 3. token log-probs
def check_logprobs(hip, name, x64, V, targets, allowed, logits_dev):
    lse, lp, am, probs = hip.token_logprobs(logits_dev, V, targets, allowed)
    torch.cuda.synchronize()
    r = WR.token_logprobs(x64, targets, allowed)
    cols = np.arange(V) if allowed is None else np.asarray(allowed)
    xs = x64[:, cols]
    m = xs.max(-1)
    Dm = np.abs(xs - m[:, None]).max(-1)
    s = np.exp(xs - m[:, None]).sum(-1)
    K = math.ceil(len(cols) / 256) + 10
    rel = (4 * Dm + K + 6) * U
    bar_lse = rel + 2 * U * (np.abs(np.log(s)) + np.abs(m) + np.abs(r["lse"]))
    e_lse = np.abs(lse.double().cpu().numpy() - r["lse"])
    print(f"token_logprobs {name}: lse err {e_lse.max():.3e} (bar >= {bar_lse.min():.3e})", end="")
    assert (e_lse <= bar_lse).all(), name
    assert np.array_equal(am.cpu().numpy(), r["argmax"]), name
    if targets is not None:
        t = np.asarray(targets)
        xt = np.where(t >= 0, x64[np.arange(len(t)), np.maximum(t, 0)], 0.0)
        bar_lp = np.where(t >= 0, bar_lse + 2 * U * (np.abs(xt) + np.abs(r["logprob"])), 0.0)
        e_lp = np.abs(lp.double().cpu().numpy() - r["logprob"])
        print(f", logprob err {e_lp.max():.3e} (bar >= {bar_lp[t >= 0].min():.3e})", end="")
        assert (e_lp <= bar_lp).all(), name
        assert bool((lp.cpu()[torch.from_numpy(t < 0)] == 0).all()), "an unscored row must be written as 0"
    if allowed is not None:
        e_p = np.abs(probs.double().cpu().numpy() - r["probs"])
        bar_p = rel[:, None] * r["probs"]
        print(f", probs err {e_p.max():.3e}, worst err/bar {float((e_p / bar_p).max()):.3f}", end="")
        assert (e_p <= bar_p).all(), name
    else:
        assert probs is None
    print()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_token_logprobs_against_float64(hip, dtype):
    """R = 5 rows of V = 203 valid columns in a [5, 208] buffer whose pad columns hold +1e30 (read, they would be the maximum); a
    target of -100; a planted tie for the arg-max; with and without an allowed list of 7 ids."""
    R, V, ldv = 5, 203, 208
    g = torch.Generator().manual_seed(11)
    x = (3 * torch.randn(R, ldv, generator=g)).to(dtype)
    x[:, V:] = 1e30
    x[3, 17] = x[3, 90] = x[3, :V].max() + 1  # the tie: id 17 wins
    x[1, V - 1] = x[1, :V].max() + 2          # the last valid column can win
    x64 = x[:, :V].double().numpy()
    targets = [3, -100, 202, 90, 0]
    allowed = [5, 17, 40, 90, 150, 201, 202]
    xd = x.to(DEV)
    check_logprobs(hip, f"{dtype} all columns", x64, V, targets, None, xd)
    check_logprobs(hip, f"{dtype} allowed", x64, V, [5, -100, 202, 90, 17], allowed, xd)
    check_logprobs(hip, f"{dtype} no targets", x64, V, None, allowed, xd)
    with pytest.raises(ValueError, match="target"):
        hip.token_logprobs(xd, V, [3, 0, V, 0, 0])
    with pytest.raises(ValueError, match="allowed"):
        hip.token_logprobs(xd, V, None, [5, V])


def test_token_logprobs_whisper_vocabulary_row(hip):
    """One row at V = 51 865 (the multilingual vocabulary; ldv = 51 872): crosses the vector main loop many times and leaves a
    one-column tail; also from an unaligned row start (ldv odd), which takes the scalar path."""
    V = 51865
    g = torch.Generator().manual_seed(12)
    for ldv in (51872, 51867):
        x = 3 * torch.randn(2, ldv, generator=g)
        x[:, V:] = 1e30
        x[1, V - 1] = 40.0
        check_logprobs(hip, f"V={V} ldv={ldv}", x[:, :V].double().numpy(), V, [V - 1, 12345], None, x.to(DEV))


# ------------------------------------------------------------------------------------------------------------ 4. the golden
@pytest.fixture(scope="module")
def model(golden):
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    cfg = json_config(golden)
    m = WhisperSeq2Seq(WhisperSeq2SeqConfig.from_hf_dict(cfg, lang_to_id={str(c): int(i) for c, i in zip(golden["lang_codes"], golden["lang_ids"])}))
    m.load_decoder_state_dict({k[2:]: torch.from_numpy(WR.bf16_from_bits(golden[k]).astype(np.float32)) for k in golden.files if k.startswith("w/")})
    return m


def json_config(golden):
    import json
    return json.loads(str(golden["config_json"]))


@pytest.fixture(scope="module")
def cpu_bars(golden):
    """The restatement in float64 and with the device's storage roundings: their distance is what the bars are measured from."""
    w = {k[2:]: WR.bf16_from_bits(golden[k]) for k in golden.files if k.startswith("w/")}
    enc, tokens = WR.bf16_from_bits(golden["enc"]), golden["tokens"]
    lens, enc_lens = [int(v) for v in golden["lens"]], [int(v) for v in golden["enc_lens"]]
    lang_ids = [int(i) for i in golden["lang_ids"]]
    out = {}
    for key, rnd in (("f64", WR.identity), ("dev", WR.bf16_round)):
        logits = WR.decoder_logits(w, G.NH, G.LAYERS, enc, tokens, enc_lens, rnd=rnd)
        sot = WR.decoder_logits(w, G.NH, G.LAYERS, enc, tokens[:, :1], enc_lens, rnd=rnd)
        out[key] = dict(scores=WR.scores(logits, tokens, lens), lang=WR.language_probs(sot[:, 0], lang_ids), logits=logits)
    a, b = out["f64"], out["dev"]
    out["d_logprob"] = float(np.abs(a["scores"]["logprobs"] - b["scores"]["logprobs"]).max())
    out["d_loss"] = float(max(np.abs(a["scores"]["loss"] - b["scores"]["loss"]).max(), abs(a["scores"]["batch_loss"] - b["scores"]["batch_loss"])))
    out["d_sum"] = float(np.abs(a["scores"]["sum_logprob"] - b["scores"]["sum_logprob"]).max())
    out["d_lang"] = float(np.abs(a["lang"][1] - b["lang"][1]).max())
    return out


def test_golden_logits(model, golden):
    enc = torch.from_numpy(WR.bf16_from_bits(golden["enc"]).astype(np.float32)).to(torch.bfloat16)
    logits = model.decode_logits(enc, golden["tokens"], golden["enc_lens"]).double().cpu().numpy()
    ref = golden["hf_logits"]
    for b, n in enumerate(golden["lens"]):
        rl = float(np.linalg.norm(logits[b, :n] - ref[b, :n]) / np.linalg.norm(ref[b, :n]))
        print(f"golden logits utterance {b} (len {int(n)}, enc_len {int(golden['enc_lens'][b])}): relative L2 {rl:.3e} (bar 2e-2)")
        assert rl < 2e-2, (b, rl)


def test_golden_scores(model, golden, cpu_bars):
    enc = torch.from_numpy(WR.bf16_from_bits(golden["enc"]).astype(np.float32)).to(torch.bfloat16)
    tokens, lens, enc_lens = golden["tokens"], golden["lens"], golden["enc_lens"]
    ref = cpu_bars["f64"]["scores"]
    assert np.abs(ref["loss"] - golden["hf_loss"]).max() < 1e-10  # the float64 value is transformers'
    lp = model.decode_logprobs(enc, tokens, lens, enc_lens)
    assert lp.shape == (B, tokens.shape[1] - 1) and lp.dtype == torch.float32
    sc = model.score(enc, tokens, lens, enc_lens)
    assert np.array_equal(sc.logprobs, lp.double().cpu().numpy()) and list(sc.n_scored) == [11, 1, 6]
    bar_lp, bar_loss, bar_sum = 4 * cpu_bars["d_logprob"], 4 * cpu_bars["d_loss"], 4 * cpu_bars["d_sum"]
    for b in range(B):
        e_lp = float(np.abs(sc.logprobs[b] - ref["logprobs"][b]).max())
        e_loss, e_sum = abs(sc.loss[b] - ref["loss"][b]), abs(sc.sum_logprob[b] - ref["sum_logprob"][b])
        print(f"golden scores utterance {b}: logprob err {e_lp:.3e} (CPU-measured {cpu_bars['d_logprob']:.3e}, bar {bar_lp:.3e}), sum err "
              f"{e_sum:.3e} (measured {cpu_bars['d_sum']:.3e}, bar {bar_sum:.3e}), loss err {e_loss:.3e} (measured {cpu_bars['d_loss']:.3e}, "
              f"bar {bar_loss:.3e})")
        assert e_lp <= bar_lp and e_loss <= bar_loss and e_sum <= bar_sum, b
        assert np.all(sc.logprobs[b, lens[b] - 1:] == 0), "positions past lens are 0"
        assert sc.avg_logprob[b] == sc.sum_logprob[b] / (lens[b] - 1 + 1)
    e_batch = abs(sc.batch_loss - float(golden["hf_batch_loss"]))
    print(f"golden batch loss {sc.batch_loss:.6f} vs transformers {float(golden['hf_batch_loss']):.6f}: err {e_batch:.3e} (bar {bar_loss:.3e})")
    assert e_batch <= bar_loss


def test_golden_language(model, golden, cpu_bars):
    enc = torch.from_numpy(WR.bf16_from_bits(golden["enc"]).astype(np.float32)).to(torch.bfloat16)
    codes, probs = model.detect_language(enc, golden["enc_lens"])
    want = golden["lang_probs"]
    want_codes = [str(golden["lang_codes"][i]) for i in want.argmax(-1)]
    bar = 4 * cpu_bars["d_lang"]
    err = np.abs(probs.double().cpu().numpy() - want)
    for b in range(B):
        print(f"golden language utterance {b}: {codes[b]} (want {want_codes[b]}), probs err {err[b].max():.3e} (CPU-measured "
              f"{cpu_bars['d_lang']:.3e}, bar {bar:.3e})")
    assert codes == want_codes  # all three: the fixture's margins are >= 0.2
    assert (err <= bar).all()


# ------------------------------------------------------------------------------------------------------------ 5. plumbing
@pytest.fixture(scope="module")
def folder(golden, tmp_path_factory):
    return G.write_folder(golden, str(tmp_path_factory.mktemp("whisper_tiny")), max_source_positions=1500, encoder_layers=1)


def test_folder_audio_and_row_chunks(folder, golden, model):
    from ssak_amd.data import load_audio
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    m = WhisperSeq2Seq.from_pretrained(folder)
    assert m.lang_codes == list(G.LANGS) and m.config.decoder_start_token_id == G.SOT
    assert torch.equal(m.dec_shadow, model.dec_shadow), "the folder's decoder is the fixture's"
    wav = load_audio(os.path.join(HERE, "golden", "bonjour.wav"))
    audio = torch.from_numpy(np.stack([wav, 0.5 * wav[::-1]]).astype(np.float32))
    tokens, lens = golden["tokens"][:2], golden["lens"][:2]
    enc = m.encode(m.features(audio))
    assert enc.shape == (2, 1500, D) and enc.dtype == torch.bfloat16 and bool(torch.isfinite(enc.float()).all())
    a, b = m.score(audio, tokens, lens), m.score(enc, tokens, lens)
    assert np.array_equal(a.logprobs, b.logprobs) and np.array_equal(a.loss, b.loss) and a.batch_loss == b.batch_loss
    assert np.isfinite(a.logprobs).all() and (a.sum_logprob < 0).all()
    # the row-chunked vocabulary projection: chunk sizes 1, 3 and "all" give the same log-probabilities
    ref = m.decode_logprobs(enc, tokens, lens)
    for chunk in (1, 3, 10 ** 6):
        m.row_chunk = chunk
        m._logits_ws = None
        got = m.decode_logprobs(enc, tokens, lens)
        diff = float((got - ref).abs().max())
        print(f"row chunk {chunk}: max |difference| to the default chunk {diff:.3e}")
        assert torch.equal(got, ref), chunk


def test_command_line(folder, capsys):
    from ssak_amd import whisper_lang
    wav = os.path.join(HERE, "golden", "bonjour.wav")
    whisper_lang.main([wav, "--model", folder])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1, lines
    path, code, prob = lines[0].split("\t")
    assert path == wav and code in G.LANGS and 0.0 < float(prob) <= 1.0


def test_refusals(golden, tmp_path):
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    heads = G.write_folder(golden, str(tmp_path / "heads"), config_overrides={"decoder_attention_heads": 4, "encoder_attention_heads": 4})
    with pytest.raises(ValueError, match="head dimension 32.*64"):
        WhisperSeq2Seq.from_pretrained(heads)
    untied = G.write_folder(golden, str(tmp_path / "untied"), extra_tensors={"proj_out.weight": torch.ones(G.V, G.D)})
    with pytest.raises(ValueError, match="untied proj_out"):
        WhisperSeq2Seq.from_pretrained(untied)
    flag = G.write_folder(golden, str(tmp_path / "flag"), config_overrides={"tie_word_embeddings": False})
    with pytest.raises(ValueError, match="untied proj_out"):
        WhisperSeq2Seq.from_pretrained(flag)
    scaled = G.write_folder(golden, str(tmp_path / "scaled"), config_overrides={"scale_embedding": True})
    with pytest.raises(ValueError, match="scale_embedding"):
        WhisperSeq2Seq.from_pretrained(scaled)
