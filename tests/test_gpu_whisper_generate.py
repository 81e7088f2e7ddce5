"""GPU: Whisper generation -- ssak_dec_attention_step, ssak_dec_greedy_step (ssak_amd/csrc/whisper_generate.hip), the stepping
primitives and ``WhisperSeq2Seq.generate`` (ssak_amd/whisper_seq2seq.py), ``python -m ssak_amd.whisper_infer`` -- against the
float64 restatements tests/whisper_decoder_ref.py / tests/whisper_generate_ref.py (held to transformers in float64 by the CPU
tests) and the fixture tests/golden/whisper_dec_tiny.npz.  Every case prints its distances before it asserts.

Bars.  u8 = 2^-8 (one bf16 rounding moves a value by at most 2^-8 of itself), u = 2^-24 (fp32).  References run on the kernels'
own bf16 inputs.

* ssak_dec_attention_step, per element of ctx: the formula of tests/test_gpu_whisper_decoder.py restated for this kernel's order.
  ctx_mag = sum_j P_j |v_j|.  P stays in fp32 into the second product, so the only bf16 rounding is the stored ctx (u8 |ctx| <=
  u8 ctx_mag; the MFMA kernel's second u8, for P, is absent).  Exponent errors, relative to each probability: the score is an
  8-term FMA chain per lane and three adds across the key's 8 lanes, 11 roundings against amax = max_j sum_d |q k| / 8; the
  multiplication by log2 e (one rounding of a value up to smax log2 e, smax = the row's largest |score|), the subtraction of the
  running maximum (one rounding of a value up to 2 smax log2 e) and v_exp_f32 (2 u):  u (11 amax + 3 smax + 2).  Every later
  rescale of a partial -- a tile that moves its lane group's maximum, the meeting of the workgroup's 32 partials, the combine of
  the splits: T + 2 stages with T = ceil(ceil(n_keys / n_split) / 128) tiles per wave -- subtracts two maxima (2 u smax), takes
  exp2 (2 u) and multiplies (u):
      eta = u (11 amax + 3 smax + 2 + (T + 2) (2 smax + 3))
  enters numerator and row sum.  Summation depth: 4 FMAs per tile into a lane group's O and row sum (4 T), 32 at the workgroup's
  meeting, n_split at the combine, one division: K = 4 T + 32 + n_split + 1, K u each for numerator and row sum.
      bar = ctx_mag (u8 + 2 eta + 2 K u)
  The integer-exact case (q = 0: every probability exactly 1, every sum exact, the fp32 division correctly rounded) must equal
  bf16(fl(sum v) / fl(count)) in every element.  The empty-split case (klens = 1, n_split = 5) must equal v[b, 0] bit for bit.
* ssak_dec_greedy_step.  Tokens, finished flags, n_unfinished: selections and counts, exact.  Log-probabilities: ssak_token_logprobs'
  bar over the columns that are not suppressed, rel = (4 D + K + 6) u with D = max_c |x_c - max x|, K = ceil(n / 256) + 10,
  bar = rel + 2 u (|log s| + |m| + |lse|) + 2 u (|x_t| + |logprob|).  h_next: bf16(fp32(e) + fp32(p)), one rounding -- exact.
* The cache against transformers (the fixture's own bars): every step's logits row 2e-2 relative L2, token log-probabilities
  7.76e-2 (DESIGN.md "Whisper decoder": 4 x the CPU-measured distance of the bf16 storage roundings).
* Free-running generate against the project's own teacher-forced pass: each path is within 7.76e-2 of float64, hence 2 x 7.76e-2
  between them; no arg-max margin is assumed.
"""
import json
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
import whisper_generate_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8, U = 2.0 ** -8, 2.0 ** -24
NH, D = 2, 128
B = 3
LP_BAR = 7.76e-2
SUPPRESS = list(range(G.EOT, G.NO_TIMESTAMPS + 1))  # every special token (eos among them): the text ids remain
N_NEW = 10


@pytest.fixture(scope="module")
def hip():
    import ssak_amd.hip as hip
    return hip


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


def dev_bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(DEV)


# ------------------------------------------------------------------------------------------------------------ 1. attention step
def run_step(hip, q, k, v, n_keys, klens, n_split, spare=5):
    """The kernel on a cache of n_keys + ``spare`` rows per utterance: k and v are column slices (at 8 and D + 24) of one buffer
    whose rows are 2 D + 24 wide, utterances cap * ld + 8 apart (not a whole number of rows); the gaps, the rows past n_keys and the
    rows past klens[b] hold NaN bit patterns.  q sits in a [B, D + 8] buffer."""
    cap, ld = n_keys + spare, 2 * D + 24
    bs = cap * ld + 8
    buf = torch.full((B * bs,), float("nan"), dtype=torch.bfloat16, device=DEV)
    kd = torch.as_strided(buf, (B, cap, D), (bs, ld, 1), 8)
    vd = torch.as_strided(buf, (B, cap, D), (bs, ld, 1), D + 24)
    for b in range(B):
        n = n_keys if klens is None else min(klens[b], n_keys)
        kd[b, :n].copy_(dev_bf16(k[b, :n]))
        vd[b, :n].copy_(dev_bf16(v[b, :n]))
    qb = torch.full((B, D + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    qb[:, :D].copy_(dev_bf16(q))
    kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device=DEV)
    ctx = torch.full((B, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.dec_attention_step(qb[:, :D], kd, vd, n_keys, NH, klens=kl, n_split=n_split, ctx=ctx)
    torch.cuda.synchronize()
    return ctx.double().cpu().numpy()


def step_bar(st, n_keys, n_split):
    rows = lambda x: np.repeat(x[:, :, 0], WR.HEAD_DIM, axis=-1)  # [B, nh, 1] -> [B, D]
    T = math.ceil(math.ceil(n_keys / n_split) / 128)
    eta = U * (11 * rows(st["amax"]) + 3 * rows(st["smax"]) + 2 + (T + 2) * (2 * rows(st["smax"]) + 3))
    K = 4 * T + 32 + n_split + 1
    return st["ctx_mag"][:, 0] * (U8 + 2 * eta + 2 * K * U)


@pytest.mark.parametrize("n_split", [1, 2, 5])
@pytest.mark.parametrize("n_keys", [1, 33, 131])
def test_attention_step_against_float64(hip, n_keys, n_split):
    """One key, a partial second tile, several tiles and waves; one piece, two, five with a ragged last one; with and without
    per-utterance key counts (n_keys, 1, n_keys // 2 + 1).  klens = 1 with n_split = 5 leaves four pieces empty: ctx = v[b, 0]."""
    rng = np.random.default_rng(1000 * n_keys + n_split)
    q = WR.bf16_round(rng.standard_normal((B, D)) * 0.8)
    k = WR.bf16_round(rng.standard_normal((B, n_keys, D)) * 0.8)
    v = WR.bf16_round(rng.standard_normal((B, n_keys, D)))
    for klens in ((n_keys, 1, n_keys // 2 + 1), None):
        got = run_step(hip, q, k, v, n_keys, klens, n_split)
        ref, st = WR.attention(q[:, None], k, v, NH, klens, stats=True)
        bar = step_bar(st, n_keys, n_split)
        err = np.abs(got - ref[:, 0])
        worst = float((err / np.maximum(bar, 1e-300)).max())
        print(f"attention step n_keys={n_keys} n_split={n_split} klens={klens}: max err {err.max():.3e}, worst err/bar {worst:.3f}")
        assert np.isfinite(got).all()
        assert (err <= bar).all(), worst
        if klens is not None:
            assert np.array_equal(got[1], v[1, 0]), "one visible key (and, at n_split = 5, four empty pieces): ctx is its value row exactly"


@pytest.mark.parametrize("n_split", [1, 3])
def test_attention_step_integer_exact(hip, n_split):
    """q = 0: every score is 0 and every probability exactly 1; integer v: every sum exact.  ctx = bf16(fl(sum v) / fl(count))."""
    rng = np.random.default_rng(5)
    n_keys, klens = 131, (131, 1, 66)
    q = np.zeros((B, D))
    k = WR.bf16_round(rng.standard_normal((B, n_keys, D)))
    v = rng.integers(-4, 5, (B, n_keys, D)).astype(np.float64)
    got = run_step(hip, q, k, v, n_keys, klens, n_split)
    want = np.stack([(torch.from_numpy(v[b, :n].sum(0)).float() / torch.tensor(float(n))).to(torch.bfloat16).double().numpy()
                     for b, n in enumerate(klens)])
    differ = int((got != want).sum())
    print(f"attention step integer-exact n_split={n_split}: {differ} of {got.size} elements differ from bf16(fl(sum v) / fl(count))")
    assert np.array_equal(got, want)


def test_attention_step_is_reproducible_and_library_split(hip):
    """n_split = 0 (the library's choice) at a shape where it splits (B * nh = 6, 1500 keys), twice: the same bits, within the bar."""
    rng = np.random.default_rng(9)
    n_keys = 1500
    q = WR.bf16_round(rng.standard_normal((B, D)) * 0.8)
    k = WR.bf16_round(rng.standard_normal((B, n_keys, D)) * 0.8)
    v = WR.bf16_round(rng.standard_normal((B, n_keys, D)))
    klens = (1500, 700, 129)
    a = run_step(hip, q, k, v, n_keys, klens, 0)
    b = run_step(hip, q, k, v, n_keys, klens, 0)
    ref, st = WR.attention(q[:, None], k, v, NH, klens, stats=True)
    bar = step_bar(st, n_keys, 10)  # (the library's split here: 10 pieces of 160 keys, T = 2 either way)
    err = np.abs(a - ref[:, 0])
    print(f"attention step n_keys=1500 library split: max err {err.max():.3e}, worst err/bar {float((err / bar).max()):.3f}")
    assert np.array_equal(a, b) and (err <= bar).all()


def test_attention_step_refusals(hip):
    cap = 8
    kv = dev_bf16(np.zeros((B, cap, 2 * D)))
    q = dev_bf16(np.zeros((B, D)))
    ctx = torch.full((B, D), 7.0, dtype=torch.bfloat16, device=DEV)
    k, v = kv[:, :, :D], kv[:, :, D:]
    with pytest.raises(ValueError, match="64"):
        hip.dec_attention_step(q, k, v, 4, 4, head_dim=32, ctx=ctx)
    with pytest.raises(ValueError, match="n_keys"):
        hip.dec_attention_step(q, k, v, 0, NH, ctx=ctx)
    narrow = dev_bf16(np.zeros((B, cap, 64)))
    with pytest.raises(ValueError, match="strides"):  # a row stride of 64 < nh * 64
        hip.dec_attention_step(q, narrow, narrow, 4, NH, ctx=ctx)
    odd = torch.as_strided(kv, (B, cap, D), (cap * 2 * D + 4, 2 * D, 1))  # a batch stride that is not a multiple of 8
    with pytest.raises(ValueError, match="strides"):
        hip.dec_attention_step(q, odd, odd, 4, NH, ctx=ctx)
    with pytest.raises(ValueError, match="workspace"):
        hip.dec_attention_step(q, k, v, 8, NH, n_split=4, workspace=torch.empty(16, dtype=torch.float32, device=DEV), ctx=ctx)
    torch.cuda.synchronize()
    assert bool((ctx == 7.0).all()), "a refused call launched"


# ------------------------------------------------------------------------------------------------------------ 2. greedy step
def test_greedy_step_planted_rows(hip):
    """R = 6 rows of V = 203 valid columns in a [6, 208] buffer whose pad columns hold +1e30.  Row 0: the maximum sits in a
    suppressed column; 1: its maximum is suppressed only at the first step; 2: an exact tie (ids 17 and 90); 3: emits eos; 4: was
    already finished; 5: plain, its maximum in the last valid column."""
    R, V, ldv, De, MAXP, EOS, PAD = 6, 203, 208, 136, 16, 7, 11
    g = torch.Generator().manual_seed(21)
    x = 3 * torch.randn(R, ldv, generator=g)
    x[:, V:] = 1e30
    top = x[:, :V].max()
    x[0, 50] = top + 5
    x[1, 60] = top + 3
    x[2, 17] = x[2, 90] = top + 1
    x[3, EOS] = top + 2
    x[4, 33] = top + 4
    x[5, V - 1] = top + 2
    sup_ids, begin_ids = [50, 120], [60, 3]
    sup, bsup = np.zeros(V, np.uint8), np.zeros(V, np.uint8)
    sup[sup_ids], bsup[begin_ids] = 1, 1
    E = torch.randn(V, De, generator=g).to(torch.bfloat16)
    Pz = torch.randn(MAXP, De, generator=g).to(torch.bfloat16)
    xd, Ed, Pd = x.to(DEV), E.to(DEV), Pz.to(DEV)
    x64 = x[:, :V].double().numpy()
    was = np.array([0, 0, 0, 0, 1, 0], dtype=bool)
    for first, t, next_pos in ((True, 0, 4), (False, 2, MAXP - 1)):
        tokens = torch.full((R, 3), -5, dtype=torch.int32, device=DEV)
        lps = torch.full((R, 3), 9.0, dtype=torch.float32, device=DEV)
        fin = torch.from_numpy(was.astype(np.uint8)).to(DEV)
        n_unf = torch.full((1,), 77, dtype=torch.int32, device=DEV)
        h_next = torch.full((R, De), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.dec_greedy_step(xd, V, finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=t, eos_id=EOS, pad_id=PAD,
                            suppress=torch.from_numpy(sup).to(DEV), begin_suppress=torch.from_numpy(bsup).to(DEV), first=first, embed_tokens=Ed,
                            embed_positions=Pd, next_pos=next_pos, h_next=h_next)
        torch.cuda.synchronize()
        want_tok, want_lp, want_fin = GR.greedy_step(x64, was, EOS, PAD, sup_ids, begin_ids, first)
        got_tok, got_lp = tokens[:, t].cpu().numpy(), lps[:, t].double().cpu().numpy()
        assert want_tok[0] != 50 and (want_tok[1] == 60) == (not first) and want_tok[2] == 17 and want_tok[3] == EOS and want_tok[4] == PAD \
            and want_tok[5] == V - 1, "the planted rows"
        assert np.array_equal(got_tok, want_tok), (got_tok, want_tok)
        assert np.array_equal(fin.cpu().numpy().astype(bool), want_fin) and want_fin.tolist() == [False, False, False, True, True, False]
        assert int(n_unf.item()) == int((~want_fin).sum()) == 4
        other = [c for c in range(3) if c != t]
        assert bool((tokens[:, other] == -5).all()) and bool((lps[:, other] == 9.0).all()), "only column t is written"
        xs = GR.process(x64, sup_ids, begin_ids, first)
        m = xs.max(-1)
        keep = np.isfinite(xs)
        Dm = np.where(keep, np.abs(xs - m[:, None]), 0).max(-1)
        s = np.exp(xs - m[:, None]).sum(-1)
        rel = (4 * Dm + math.ceil(V / 256) + 10 + 6) * U
        bar = rel + 2 * U * (np.abs(np.log(s)) + np.abs(m) + np.abs(m + np.log(s))) + 2 * U * (np.abs(m) + np.abs(want_lp))  # (x_t = m)
        err = np.abs(got_lp - want_lp)
        print(f"greedy step first={first}: tokens {got_tok.tolist()}, log-prob err {err.max():.3e}, worst err/bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all() and got_lp[4] == 0.0
        want_h = (E[torch.from_numpy(want_tok)].float() + Pz[next_pos].float()[None]).to(torch.bfloat16)
        assert torch.equal(h_next.cpu().view(torch.int16), want_h.view(torch.int16)), "h_next is defined bit for bit"
    # refusals: nothing is launched
    tokens = torch.full((R, 3), -5, dtype=torch.int32, device=DEV)
    lps = torch.zeros((R, 3), dtype=torch.float32, device=DEV)
    fin = torch.zeros(R, dtype=torch.uint8, device=DEV)
    n_unf = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    h_next = torch.full((R, De), 7.0, dtype=torch.bfloat16, device=DEV)
    kw = dict(finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, embed_tokens=Ed, embed_positions=Pd, h_next=h_next)
    with pytest.raises(ValueError, match="overruns"):
        hip.dec_greedy_step(xd, V, t=0, eos_id=EOS, pad_id=PAD, next_pos=MAXP, **kw)
    with pytest.raises(ValueError, match="eos_id"):
        hip.dec_greedy_step(xd, V, t=0, eos_id=V, pad_id=PAD, next_pos=0, **kw)
    with pytest.raises(ValueError, match="pad_id"):
        hip.dec_greedy_step(xd, V, t=0, eos_id=EOS, pad_id=-1, next_pos=0, **kw)
    with pytest.raises(ValueError, match="step t"):
        hip.dec_greedy_step(xd, V, t=3, eos_id=EOS, pad_id=PAD, next_pos=0, **kw)
    torch.cuda.synchronize()
    assert bool((tokens == -5).all()) and int(n_unf.item()) == 77 and bool((h_next == 7.0).all()), "a refused call launched"


def test_greedy_step_all_suppressed_row_and_vocabulary_width(hip):
    """A row whose columns are all suppressed (the caller's error) emits pad; V = 51 865 in a 51 872-column buffer crosses the
    vector loop many times and leaves a one-column tail, which holds the maximum of row 1."""
    V, ldv = 51865, 51872
    g = torch.Generator().manual_seed(22)
    x = 3 * torch.randn(2, ldv, generator=g)
    x[:, V:] = 1e30
    x[1, V - 1] = 40.0
    tokens = torch.zeros((2, 1), dtype=torch.int32, device=DEV)
    lps = torch.zeros((2, 1), dtype=torch.float32, device=DEV)
    fin, n_unf = torch.zeros(2, dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    hip.dec_greedy_step(x.to(DEV), V, finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=0, eos_id=1, pad_id=2)
    want_tok, want_lp, _ = GR.greedy_step(x[:, :V].double().numpy(), [False, False], 1, 2)
    err = np.abs(lps[:, 0].double().cpu().numpy() - want_lp)
    print(f"greedy step V={V}: tokens {tokens[:, 0].tolist()}, log-prob err {err.max():.3e}")
    assert tokens[:, 0].tolist() == want_tok.tolist() and want_tok[1] == V - 1 and err.max() < 1e-4
    every = torch.ones(V, dtype=torch.uint8, device=DEV)
    hip.dec_greedy_step(x.to(DEV), V, finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=0, eos_id=1, pad_id=2, suppress=every)
    assert tokens[:, 0].tolist() == [2, 2] and lps[:, 0].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------------------ 3. the golden
@pytest.fixture(scope="module")
def model(golden):
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    gen = json.loads(str(golden["generation_config_json"]))
    cfg = WhisperSeq2SeqConfig.from_hf_dict(json.loads(str(golden["config_json"])),
                                            lang_to_id={str(c): int(i) for c, i in zip(golden["lang_codes"], golden["lang_ids"])},
                                            task_to_id=gen["task_to_id"], no_timestamps_token_id=gen["no_timestamps_token_id"])
    m = WhisperSeq2Seq(cfg)
    m.load_decoder_state_dict({k[2:]: torch.from_numpy(WR.bf16_from_bits(golden[k]).astype(np.float32)) for k in golden.files if k.startswith("w/")})
    return m


@pytest.fixture(scope="module")
def enc(golden):
    return torch.from_numpy(WR.bf16_from_bits(golden["enc"]).astype(np.float32)).to(torch.bfloat16)


@pytest.mark.parametrize("attention", ["step", "fwd"])
@pytest.mark.parametrize("P", [1, 4])
def test_cache_against_transformers(hip, model, golden, enc, P, attention):
    """Prefill the first P tokens of the fixture's sequences, then step through the rest with the fixture's own tokens forced
    (the stepping primitives generate() is built from; the forced row is ssak_dec_embed at the step's position).  Every step's
    logits row against transformers'; a stale cache row, a wrong position or an off-by-one n_keys fails here.  ``attention``:
    the step kernel, and the older entry at Lq = 1 on the same cache (the path generate() keeps where the step kernel does not
    pay)."""
    tokens, lens, enc_lens = golden["tokens"].astype(np.int64), golden["lens"], golden["enc_lens"]
    L, V = tokens.shape[1], G.V
    step = attention == "step"  # (generate() itself keeps the older entry for a cache of up to 64 keys: here the step kernel runs from key 1)
    st = model._gen_begin(enc.to(DEV), enc_lens, cap=L, step_cross=step, step_self_min_keys=1 if step else None)
    rows = {P - 1: model._gen_prefill(st, tokens[:, :P])[:, :V].double().cpu().numpy()}
    E, Pz = model._w("embed_tokens.weight"), model._w("embed_positions.weight")
    for t in range(P, L):
        assert st.t == t
        rows[t] = model._gen_step(st, hip.dec_embed(E, Pz, tokens[:, t:t + 1], t))[:, :V].double().cpu().numpy()
    ref = golden["hf_logits"]
    worst_l2 = worst_lp = 0.0
    for b in range(B):
        for t in range(P - 1, int(lens[b])):
            rl = float(np.linalg.norm(rows[t][b] - ref[b, t]) / np.linalg.norm(ref[b, t]))
            worst_l2 = max(worst_l2, rl)
            assert rl < 2e-2, (b, t, rl)
            if t + 1 < lens[b]:
                tg = int(tokens[b, t + 1])
                d = abs(GR.log_softmax(rows[t][b][None])[0, tg] - GR.log_softmax(ref[b, t][None])[0, tg])
                worst_lp = max(worst_lp, d)
                assert d <= LP_BAR, (b, t, d)
    print(f"cache vs transformers P={P} attention={attention}: worst logits row relative L2 {worst_l2:.3e} (bar 2e-2), worst token log-prob "
          f"distance {worst_lp:.3e} (bar {LP_BAR:.2e})")


@pytest.fixture(scope="module")
def free_run(model, enc, golden):
    return model.generate(enc, max_new_tokens=N_NEW, enc_lens=golden["enc_lens"], suppress_tokens=SUPPRESS)


def test_generate_is_consistent_with_teacher_forcing(model, enc, golden, free_run):
    """Default prompt (the detected language per utterance), 10 tokens, eos suppressed.  lp_tf = the processed log-softmax of the
    project's own teacher-forced decode_logits on prompt + output: every returned log-probability within 2 x 7.76e-2 of lp_tf at
    the chosen token, every chosen token within 2 x 7.76e-2 of lp_tf's maximum."""
    r = free_run
    assert r.steps == N_NEW and r.lens.tolist() == [N_NEW] * B and r.token_array.shape == (B, N_NEW) and r.logprobs.shape == (B, N_NEW)
    assert not np.isin(r.token_array, SUPPRESS).any()
    codes, _ = model.detect_language(enc, golden["enc_lens"])
    prompt = model.default_prompt(B, codes)
    assert prompt.shape == (B, 4) and prompt[0].tolist() == [G.SOT, G.LANG0 + G.LANGS.index(codes[0]), G.TRANSCRIBE, G.NO_TIMESTAMPS]
    full = np.concatenate([prompt, r.token_array], 1)
    logits = model.decode_logits(enc, full, golden["enc_lens"]).double().cpu().numpy()
    P = prompt.shape[1]
    worst_lp = worst_top = 0.0
    for i in range(N_NEW):
        lsm = GR.log_softmax(GR.process(logits[:, P - 1 + i], SUPPRESS))
        at = lsm[np.arange(B), r.token_array[:, i]]
        worst_lp = max(worst_lp, float(np.abs(r.logprobs[:, i] - at).max()))
        worst_top = max(worst_top, float((lsm.max(-1) - at).max()))
    print(f"generate: tokens {r.tokens}; max |log-prob - teacher-forced| {worst_lp:.3e}, max (teacher-forced maximum - chosen) {worst_top:.3e} "
          f"(bar {2 * LP_BAR:.3e})")
    assert worst_lp <= 2 * LP_BAR and worst_top <= 2 * LP_BAR
    assert np.array_equal(r.sum_logprob, r.logprobs.sum(-1)) and np.array_equal(r.avg_logprob, r.sum_logprob / (r.lens + 1))


@pytest.mark.parametrize("poll_every", [0, 1, 8])
def test_generate_poll_every_changes_nothing(model, enc, golden, free_run, poll_every):
    r = model.generate(enc, max_new_tokens=N_NEW, enc_lens=golden["enc_lens"], suppress_tokens=SUPPRESS, poll_every=poll_every)
    assert r.tokens == free_run.tokens and np.array_equal(r.logprobs, free_run.logprobs) and r.steps == N_NEW


def test_generate_eos(model, enc, golden, free_run):
    """eos = the token utterance 0 produced at step 3 of the free run: utterance 0 stops there (lens 4, pads after), the others
    are unchanged up to their own first occurrence of that id.  Then that id as every utterance's step-0 token (everything else
    suppressed at the start), poll_every = 1: the call ends after one step."""
    eos = int(free_run.token_array[0, 3])
    sup = [s for s in SUPPRESS if s != eos]
    pad = model.config.pad_token_id
    r = model.generate(enc, max_new_tokens=N_NEW, enc_lens=golden["enc_lens"], suppress_tokens=sup, eos_token_id=eos, poll_every=0)
    print(f"generate with eos = {eos}: lens {r.lens.tolist()}, tokens {r.tokens}")
    for b in range(B):
        was = free_run.token_array[b].tolist()
        n = was.index(eos) + 1 if eos in was else N_NEW
        assert r.lens[b] == n and r.tokens[b] == was[:n], b
        assert (r.token_array[b, n:] == pad).all() and (r.logprobs[b, n:] == 0).all()
        assert np.array_equal(r.logprobs[b, :n], free_run.logprobs[b, :n]), "the same arithmetic up to the stop"
    assert r.lens[0] == 4 and r.tokens[0][-1] == eos
    begin = [t for t in range(G.V) if t != eos]
    r1 = model.generate(enc, max_new_tokens=N_NEW, enc_lens=golden["enc_lens"], suppress_tokens=sup, begin_suppress_tokens=begin, eos_token_id=eos,
                        poll_every=1)
    assert r1.lens.tolist() == [1] * B and r1.tokens == [[eos]] * B and r1.steps == 1
    r8 = model.generate(enc, max_new_tokens=N_NEW, enc_lens=golden["enc_lens"], suppress_tokens=sup, begin_suppress_tokens=begin, eos_token_id=eos,
                        poll_every=8)
    assert r8.lens.tolist() == [1] * B and r8.steps == 8 and np.array_equal(r8.logprobs, r1.logprobs)


def test_generate_refusals(model, enc):
    maxp = model.config.max_target_positions
    with pytest.raises(ValueError, match="max_target_positions"):
        model.generate(enc, language="en", max_new_tokens=maxp - 3)
    with pytest.raises(ValueError, match="max_target_positions"):
        model.generate(enc, prompt=np.full((B, maxp), G.SOT))
    with pytest.raises(ValueError, match="language"):
        model.generate(enc, language="xx", max_new_tokens=2)
    with pytest.raises(ValueError, match="enc_lens"):
        model.generate(enc, language="en", max_new_tokens=2, enc_lens=(50, 0, 23))
    r = model.generate(enc, language="en", max_new_tokens=maxp - 4, suppress_tokens=SUPPRESS, poll_every=0)  # what fits, to the last position
    assert r.steps == maxp - 4


# ------------------------------------------------------------------------------------------------------------ 4. plumbing
@pytest.fixture(scope="module")
def folder(golden, tmp_path_factory):
    return G.write_folder(golden, str(tmp_path_factory.mktemp("whisper_tiny_gen")), max_source_positions=1500, encoder_layers=1)


def test_folder_and_audio(folder, golden):
    from ssak_amd.data import load_audio
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    m = WhisperSeq2Seq.from_pretrained(folder)
    c = m.config
    assert (c.eos_token_id, c.pad_token_id, c.no_timestamps_token_id) == (G.EOT, G.EOT, G.NO_TIMESTAMPS)
    assert c.task_to_id == {"translate": G.TRANSLATE, "transcribe": G.TRANSCRIBE}
    wav = load_audio(os.path.join(HERE, "golden", "bonjour.wav"))
    audio = torch.from_numpy(np.stack([wav, 0.5 * wav[::-1]]).astype(np.float32))
    a = m.generate(audio, max_new_tokens=6, suppress_tokens=SUPPRESS)
    b = m.generate(m.encode(m.features(audio)), max_new_tokens=6, suppress_tokens=SUPPRESS)
    assert a.tokens == b.tokens and np.array_equal(a.logprobs, b.logprobs) and a.lens.tolist() == [6, 6]
    assert np.isfinite(a.logprobs).all() and (a.sum_logprob < 0).all()


def test_command_line(folder, capsys):
    from ssak_amd import whisper_infer
    wav = os.path.join(HERE, "golden", "bonjour.wav")
    whisper_infer.main([wav, "--model", folder, "--language", "fr", "--max_new_tokens", "5"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1, lines
    path, ids = lines[0].split("\t")[:2]
    ids = [int(t) for t in ids.split()]
    assert path == wav and 1 <= len(ids) <= 5 and all(0 <= t < G.V for t in ids)
