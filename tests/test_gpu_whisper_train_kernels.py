"""GPU: the Whisper decoder's backward kernels (ABI 650, ssak_amd/csrc/whisper_train.hip) -- ssak_dec_attention_fwd_lse,
ssak_dec_attention_bwd, ssak_dec_ce_bwd, ssak_dec_embed_bwd, ssak_layernorm_fwd_stats / ssak_layernorm_bwd -- per kernel against the
float64 references of tests/whisper_train_ref.py.  References run on the kernels' own bf16 inputs (the backward's on the ctx and lse
the device's forward wrote); outputs are prefilled with NaN and stride gaps are checked untouched.  Every case prints its worst
error / bar before it asserts.

Bars.  u8 = 2^-8 (one bf16 rounding), u = 2^-24 (fp32).  T(n) = ceil(n / 32).

* lse of ssak_dec_attention_fwd_lse.  lse = (M + log2 L) ln 2 where L 2^M is the forward's row sum, whose relative error the
  forward's bar already bounds: eta = u (6 amax + 2 smax + 4) from the exponents and (T(Lk) + 8) u from the fp32 sums (header of
  tests/test_gpu_whisper_decoder.py).  A relative error of the sum is an absolute error of its logarithm.  On top: log2f (u |log2 L|
  + u, |log2 L| <= log2 Lk + 1), the addition (u (|M| + |log2 L|), |M| <= 1.45 smax), the multiplication by a rounded ln 2 (2 u |lse|):
      bar_lse = eta + (T(Lk) + 8) u + u (4 |lse| + 3 smax + 2 log2(Lk) + 4)
* ssak_dec_attention_bwd.  delta: 64 exact products, 8 added in order and 3 exchanges per lane: 12 u sum_d |dO O|.
  A recomputed probability exp2(fl(s log2 e) - fl(lse log2 e)): the 64-term MFMA score sum (two roundings against amag = sum_d |q k|
  / 8), the two multiplications by log2 e (u |s|, 1.5 u |lse|), the subtraction (u max of the two) and v_exp_f32:
      epsP = u (2 amag + 2 |s| + 3 |lse| + 4)      relative to P
  dP = dO v^T is a 64-term MFMA sum: 2 u dpmag, dpmag = sum_d |dO v|.  dS = P (dP - delta) then costs
      E_dS = P ((epsP + 3 u) |dP - delta| + 2 u dpmag + bar_delta + u (|dP| + |delta|)) + u8 |dS|
  the last term being its rounding to bf16 into the second product; P enters dv's product with E_P = P (epsP + u8).  The second
  products accumulate in fp32, one MFMA per 32-row tile and wave and four partials at the merge: (T + 8) u of the sum of the
  magnitudes, T over the reduced dimension.  The outputs are stored as bf16 (u8 of themselves):
      bar_dq = (E_dS |k| + (T(Lk) + 8) u |dS| |k|) / 8 + u8 |dq|
      bar_dk = E_dS^T |q| / 8 + (T(Lq) + 8) u |dS|^T |q| / 8 + u8 |dk|
      bar_dv = E_P^T |dO| + (T(Lq) + 8) u P^T |dO| + u8 |dv|
  The integer-exact cases (lse = 0 and all scores 0, so P = 1 exactly; small-integer operands) must reproduce the correctly
  rounded result bit for bit.
* ssak_dec_ce_bwd.  ssak_token_logprobs' terms (header of tests/test_gpu_whisper_decoder.py): rel = (4 D + K + 6) u, K = ceil(V /
  256) + 10, bar_lse = rel + 2 u (|log s| + |m| + |lse|), bar_logprob = bar_lse + 2 u (|x_t| + |logprob|).  p = expf(x - lse)
  carries lse's error, its argument's rounding and expf's two ulp; the subtraction of the one-hot and the scaling one rounding
  each; the store one bf16 rounding (and fp32's underflow, 2^-126):
      bar_d = |scale| (p (bar_lse + u |x - lse| + 3 u) + 2 u |p - onehot| + 2^-126) + u8 |d|
  loss_sum: the sum of the rows' bar_logprob plus (ceil(R / 256) + 11) u sum |row_loss| for the fixed-order sum and the `+=`.
* ssak_dec_embed_bwd: n fp32 additions (the rows of a token, or the batch, and the `+=`): n u sum |terms|.
* ssak_layernorm_fwd_stats / ssak_layernorm_bwd: the same templates as the ssak_debug_layernorm_* entries -- bit for bit.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import whisper_decoder_ref as WR  # noqa: E402
import whisper_train_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8, U = 2.0 ** -8, 2.0 ** -24
NH, D = 2, 128
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    import ssak_amd.hip as hip
    return hip


def dev_bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int16)


def f64(t):
    return t.double().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ 1. attention
def attn_inputs(B, Lq, Lk, klens, seed):
    """float64 q / dctx [B, Lq, D], k / v [B, Lk, D] holding bf16 values; K / V rows at keys >= klens[b] poisoned (K aligned with a
    query, V = +-1000): a leaked key is a gross error."""
    rng = np.random.default_rng(seed)
    q, k, v, do = (WR.bf16_round(rng.standard_normal((B, n, D)) * s) for n, s in ((Lq, 0.8), (Lk, 0.8), (Lk, 1.0), (Lq, 1.0)))
    if klens is not None:
        for b, kl in enumerate(klens):
            if kl < Lk:
                k[b, kl:] = WR.bf16_round(2 * q[b, 0])
                v[b, kl:] = 1000.0 * (rng.integers(0, 2, (Lk - kl, D)) * 2 - 1)
    return q, k, v, do


class Buffers:
    """The kernels' strided views.  ``packed``: q | k | v (and dq | dk | dv) as column blocks of one [B * L, 3 D] buffer
    (self-attention); otherwise q in a [B * Lq, D + 8] buffer and k, v in one [B * Lk, 2 D + 24] buffer at columns 8 and D + 24
    (and dq, dk | dv likewise), the gaps NaN: separate pointers, row strides wider than D."""

    def __init__(self, q, k, v, packed):
        B, Lq, _ = q.shape
        Lk = k.shape[1]
        if packed:
            self.buf = dev_bf16(np.concatenate([q, k, v], -1).reshape(B * Lq, 3 * D))
            self.q, self.k, self.v = self.buf[:, :D], self.buf[:, D:2 * D], self.buf[:, 2 * D:]
            self.dbuf = torch.full((B * Lq, 3 * D), NAN, dtype=torch.bfloat16, device=DEV)
            self.dq, self.dk, self.dv = self.dbuf[:, :D], self.dbuf[:, D:2 * D], self.dbuf[:, 2 * D:]
            self.gaps = []
        else:
            qb = torch.full((B * Lq, D + 8), NAN, dtype=torch.bfloat16, device=DEV)
            kvb = torch.full((B * Lk, 2 * D + 24), NAN, dtype=torch.bfloat16, device=DEV)
            self.q, self.k, self.v = qb[:, :D], kvb[:, 8:8 + D], kvb[:, D + 24:]
            self.q.copy_(dev_bf16(q.reshape(B * Lq, D)))
            self.k.copy_(dev_bf16(k.reshape(B * Lk, D)))
            self.v.copy_(dev_bf16(v.reshape(B * Lk, D)))
            dqb = torch.full((B * Lq, D + 8), NAN, dtype=torch.bfloat16, device=DEV)
            dkvb = torch.full((B * Lk, 2 * D + 24), NAN, dtype=torch.bfloat16, device=DEV)
            self.dq, self.dk, self.dv = dqb[:, :D], dkvb[:, 8:8 + D], dkvb[:, D + 24:]
            self.gaps = [dqb[:, D:], dkvb[:, :8], dkvb[:, 8 + D:D + 24]]


def run_attention_bwd(hip, q, k, v, do, klens, causal, q_offset, packed, ctx_lse=None):
    """Forward (with and without lse) and backward on the device -> dict of float64 arrays + the forward's lse and ctx."""
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    bufs = Buffers(q, k, v, packed)
    kw = dict(klens=klens, causal=causal, q_offset=q_offset)
    if ctx_lse is None:
        ctx = torch.full((B * Lq, D), NAN, dtype=torch.bfloat16, device=DEV)
        lse = torch.full((B, NH, Lq), NAN, dtype=torch.float32, device=DEV)
        hip.dec_attention_fwd_lse(bufs.q, bufs.k, bufs.v, B, Lq, Lk, NH, ctx=ctx, lse=lse, **kw)
        ctx0 = hip.dec_attention_fwd(bufs.q, bufs.k, bufs.v, B, Lq, Lk, NH, **kw)
        assert torch.equal(bits(ctx), bits(ctx0)), "ssak_dec_attention_fwd_lse's ctx differs from ssak_dec_attention_fwd's"
    else:
        ctx, lse = dev_bf16(ctx_lse[0].reshape(B * Lq, D)), torch.from_numpy(np.asarray(ctx_lse[1], dtype=np.float32)).to(DEV)
    delta = torch.full((B, NH, Lq), NAN, dtype=torch.float32, device=DEV)
    hip.dec_attention_bwd(bufs.q, bufs.k, bufs.v, ctx, lse, dev_bf16(do.reshape(B * Lq, D)), bufs.dq, bufs.dk, bufs.dv, B, Lq, Lk, NH,
                          delta=delta, **kw)
    torch.cuda.synchronize()
    for gap in bufs.gaps:
        assert bool(torch.isnan(gap).all()), "a stride gap was written"
    return dict(dq=f64(bufs.dq).reshape(B, Lq, D), dk=f64(bufs.dk).reshape(B, Lk, D), dv=f64(bufs.dv).reshape(B, Lk, D), delta=f64(delta),
                lse=f64(lse), ctx=f64(ctx).reshape(B, Lq, D), raw=(bits(bufs.dq).clone(), bits(bufs.dk).clone(), bits(bufs.dv).clone(), delta.clone()))


def check_attention_bwd(hip, name, Lq, Lk, klens, causal, q_offset, packed, seed, B=3):
    q, k, v, do = attn_inputs(B, Lq, Lk, klens, seed)
    got = run_attention_bwd(hip, q, k, v, do, klens, causal, q_offset, packed)
    for key in ("dq", "dk", "dv", "delta", "lse"):
        assert np.isfinite(got[key]).all(), (name, key)
    # ---- the forward's lse
    _, st = WR.attention(q, k, v, NH, klens, causal, q_offset, stats=True)
    lse_ref = TR.attention_lse(q, k, NH, klens, causal, q_offset)
    eta = U * (6 * st["amax"] + 2 * st["smax"] + 4)
    bar_lse = eta + (math.ceil(Lk / 32) + 8) * U + U * (4 * np.abs(lse_ref) + 3 * st["smax"] + 2 * math.log2(Lk) + 4)
    worst = {"lse": float((np.abs(got["lse"] - lse_ref) / bar_lse).max())}
    # ---- the backward, on the ctx and lse it was given
    ref, bar = TR.attention_bwd(q, k, v, got["ctx"], got["lse"], do, NH, klens, causal, q_offset)
    for key in ("dq", "dk", "dv", "delta"):
        worst[key] = float((np.abs(got[key] - ref[key]) / np.maximum(bar[key], 1e-300)).max())
    print(f"attention_bwd {name}: B={B} Lq={Lq} Lk={Lk} klens={klens} causal={causal} q_offset={q_offset}: worst err/bar "
          + ", ".join(f"{k_} {w:.3f}" for k_, w in worst.items()))
    for key, w in worst.items():
        assert w <= 1.0, (name, key, w)
    if klens is not None:
        for b, kl in enumerate(klens):
            assert (got["dk"][b, kl:] == 0).all() and (got["dv"][b, kl:] == 0).all(), "dk / dv rows past klens must be written as zeros"
    return got


@pytest.mark.parametrize("Lq", [1, 5, 16, 17, 33])
@pytest.mark.parametrize("Lk", [1, 50, 131])
def test_cross_attention_bwd_against_float64(hip, Lq, Lk):
    """One, partial and several 32-key tiles and 16-key blocks against one, partial and several 16-query blocks and 32-query tiles;
    key counts (Lk, 1, Lk // 2 + 1) with the K / V rows past them poisoned; separate pointers, wide strides."""
    check_attention_bwd(hip, "cross", Lq, Lk, (Lk, 1, Lk // 2 + 1), False, 0, False, seed=100 * Lq + Lk)


def test_cross_attention_bwd_long_keys(hip):
    """The encoder's 1500 frames: 47 key tiles over four waves, 94 key blocks."""
    check_attention_bwd(hip, "cross-1500", 33, 1500, (1500, 1, 751), False, 0, False, seed=5)


@pytest.mark.parametrize("L", [37, 64, 65])
def test_causal_attention_bwd_against_float64(hip, L):
    """The diagonal inside a tile, at a tile's edge and one past it; q, k, v and dq, dk, dv column blocks of packed buffers."""
    check_attention_bwd(hip, "causal", L, L, None, True, 0, True, seed=L)


def test_causal_attention_bwd_longest(hip):
    """The decoder's longest sequence: 14 query tiles, 28 blocks."""
    check_attention_bwd(hip, "causal-448", 448, 448, None, True, 0, True, seed=448, B=1)


def test_causal_attention_bwd_offset_and_klens(hip):
    """Queries that start at key 7 of 12; causal with key counts on top."""
    check_attention_bwd(hip, "offset", 5, 12, None, True, 7, False, seed=55)
    check_attention_bwd(hip, "causal+klens", 37, 37, (37, 1, 19), True, 0, False, seed=136)
    check_attention_bwd(hip, "offset+klens", 5, 12, (12, 1, 7), True, 7, False, seed=104)


@pytest.mark.parametrize("Lq,Lk,causal", [(32, 129, False), (129, 15, False), (31, 128, False), (128, 128, True), (129, 129, True)],
                         ids=["32x129", "129x15", "31x128", "causal128", "causal129"])
def test_attention_bwd_tile_edges(hip, Lq, Lk, causal):
    """The kernels' own edges: 16-row blocks, 32-row reduction tiles, one full round of the four waves (128) and one tile more."""
    check_attention_bwd(hip, "edge", Lq, Lk, None if causal else (Lk, 1, Lk // 2 + 1), causal, 0, causal, seed=Lq * 7 + Lk)


def test_attention_bwd_integer_exact(hip):
    """lse = 0 with all scores 0 (q = 0, or k = 0): every P is exp2(0) = 1 exactly; small-integer v, dctx, ctx make dP, delta and
    dS = dP - delta integers below 2^8 (exact as bf16 operands) and every sum exact in fp32.  dq, dk, dv must be the correctly
    rounded bf16 of the exact results, delta exact."""
    rng = np.random.default_rng(11)
    B = 3
    for causal, Lq, Lk, klens in ((True, 37, 37, None), (False, 17, 131, (131, 1, 66))):
        for zero in ("q", "k"):
            q = rng.integers(-2, 3, (B, Lq, D)).astype(np.float64) * (zero != "q")
            k = rng.integers(-2, 3, (B, Lk, D)).astype(np.float64) * (zero != "k")
            v = rng.integers(-1, 2, (B, Lk, D)).astype(np.float64)
            do = rng.integers(-1, 2, (B, Lq, D)).astype(np.float64)
            ctx = rng.integers(-1, 2, (B, Lq, D)).astype(np.float64)
            lse = np.zeros((B, NH, Lq))
            got = run_attention_bwd(hip, q, k, v, do, klens, causal, 0, causal, ctx_lse=(ctx, lse))
            ref, _ = TR.attention_bwd(q, k, v, ctx, lse, do, NH, klens, causal, 0)
            diffs = {key: int((got[key] != (ref[key] if key == "delta" else WR.bf16_round(ref[key]))).sum()) for key in ("dq", "dk", "dv", "delta")}
            print(f"attention_bwd integer-exact causal={causal} zero={zero}: elements that differ {diffs}")
            assert not any(diffs.values()), diffs


def test_attention_bwd_independence_and_determinism(hip):
    """Another utterance's or another head's inputs do not move an (utterance, head)'s outputs by a bit; two runs agree bit for bit."""
    B, Lq, Lk, klens = 3, 33, 50, (50, 7, 26)
    q, k, v, do = attn_inputs(B, Lq, Lk, klens, 77)
    a = run_attention_bwd(hip, q, k, v, do, klens, False, 0, False)["raw"]
    a2 = run_attention_bwd(hip, q, k, v, do, klens, False, 0, False)["raw"]
    for x, y in zip(a, a2):
        assert torch.equal(x, y), "two runs differ"
    rng = np.random.default_rng(78)
    q2, k2, v2, do2 = (x.copy() for x in (q, k, v, do))
    for x in (q2, k2, v2, do2):
        x[1] = WR.bf16_round(rng.standard_normal(x[1].shape))  # utterance 1, both heads
        x[:, :, 64:] = WR.bf16_round(rng.standard_normal(x[:, :, 64:].shape))  # head 1 of every utterance
    b = run_attention_bwd(hip, q2, k2, v2, do2, klens, False, 0, False)["raw"]
    for name, x, y, n in zip(("dq", "dk", "dv"), a, b, (Lq, Lk, Lk)):
        x, y = x.reshape(B, n, D), y.reshape(B, n, D)
        for u in (0, 2):
            assert torch.equal(x[u, :, :64], y[u, :, :64]), f"{name}: utterance {u} head 0 moved"
    assert torch.equal(a[3][0, 0], b[3][0, 0]) and torch.equal(a[3][2, 0], b[3][2, 0]), "delta moved"


def test_attention_bwd_refusals(hip):
    B, L = 3, 4
    q, k, v, ctx, do = (dev_bf16(np.zeros((B * L, D))) for _ in range(5))
    dq, dk, dv = (torch.full((B * L, D), 7.0, dtype=torch.bfloat16, device=DEV) for _ in range(3))
    lse = torch.zeros((B, NH, L), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="64"):
        hip.dec_attention_bwd(q, k, v, ctx, torch.zeros((B, 4, L), dtype=torch.float32, device=DEV), do, dq, dk, dv, B, L, L, 4, head_dim=32)
    for bad in ((4, 0, 2), (4, 5, 2)):
        with pytest.raises(ValueError, match="klens"):
            hip.dec_attention_bwd(q, k, v, ctx, lse, do, dq, dk, dv, B, L, L, NH, klens=bad)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (dq, dk, dv)), "a refused call launched"


# ------------------------------------------------------------------------------------------------------------ 2. cross-entropy
def check_ce(hip, name, x64, V, ldv, ldd, targets, scale):
    R = x64.shape[0]
    logits = torch.full((R, ldv), 1e30, dtype=torch.float32, device=DEV)  # the pads would swamp any sum that read them
    logits[:, :V] = torch.from_numpy(x64.astype(np.float32)).to(DEV)
    x = f64(logits[:, :V])
    dl = torch.full((R, ldd), NAN, dtype=torch.bfloat16, device=DEV)
    loss_sum = torch.full((1,), 2.5, dtype=torch.float32, device=DEV)
    _, row_loss, _ = hip.dec_ce_bwd(logits, V, targets, scale, dlogits=dl, loss_sum=loss_sum)
    torch.cuda.synchronize()
    t = np.asarray(targets)
    sc = t >= 0
    r = TR.ce_bwd(x, t, scale)
    m = x.max(-1)
    Dm = np.abs(x - m[:, None]).max(-1)
    s = np.exp(x - m[:, None]).sum(-1)
    rel = (4 * Dm + math.ceil(V / 256) + 10 + 6) * U
    bar_lse = rel + 2 * U * (np.abs(np.log(s)) + np.abs(m) + np.abs(r["lse"]))
    onehot = np.zeros_like(x)
    onehot[np.nonzero(sc)[0], t[sc]] = 1.0
    bar_d = abs(scale) * (r["p"] * (bar_lse[:, None] + U * np.abs(x - r["lse"][:, None]) + 3 * U) + 2 * U * np.abs(r["p"] - onehot) + 2.0 ** -126) \
        + U8 * np.abs(r["dlogits"])
    got = f64(dl)
    e_d = np.abs(got[:, :V] - r["dlogits"])
    xt = np.where(sc, x[np.arange(R), np.maximum(t, 0)], 0.0)
    bar_lp = np.where(sc, bar_lse + 2 * U * (np.abs(xt) + np.abs(r["row_loss"])), 0.0)
    e_lp = np.abs(f64(row_loss) - r["row_loss"])
    bar_sum = bar_lp.sum() + (math.ceil(R / 256) + 11) * U * (np.abs(r["row_loss"]).sum() + 2.5)
    e_sum = abs(float(loss_sum.item()) - 2.5 - r["loss_sum"])
    print(f"ce_bwd {name}: R={R} V={V} ldv={ldv} ldd={ldd} scale={scale}: dlogits worst err/bar {float((e_d[sc] / bar_d[sc]).max()):.3f}, row_loss "
          f"{float((e_lp[sc] / bar_lp[sc]).max()):.3f}, loss_sum err {e_sum:.3e} bar {bar_sum:.3e}")
    assert np.isfinite(got).all(), name
    assert (e_d[sc] <= bar_d[sc]).all(), name
    assert (got[~sc] == 0).all(), "an ignored row must be written as zeros"
    assert (got[:, V:] == 0).all(), "the pad columns must be written as zeros"
    assert (e_lp <= bar_lp).all() and (f64(row_loss)[~sc] == 0).all(), name
    assert e_sum <= bar_sum, name
    # a target's gradient is negative, every other positive: the one-hot sits in the right column
    assert (got[np.nonzero(sc)[0], t[sc]] * scale <= 0).all()


@pytest.mark.parametrize("ldv,ldd", [(128, 128), (127, 136), (132, 127)], ids=["vector", "odd-ldv", "odd-ldd"])
def test_ce_bwd_small_vocabulary(hip, ldv, ldd):
    """V = 127 with ignored rows, through the vector path and both scalar ones."""
    rng = np.random.default_rng(ldv + ldd)
    x = rng.standard_normal((9, 127)) * 4.0
    targets = [3, -100, 126, 0, -100, 77, 5, -100, 126]
    check_ce(hip, "V127", x, 127, ldv, ldd, targets, 1.0 / 6)


def test_ce_bwd_whisper_vocabulary(hip):
    """Three rows of the multilingual vocabulary (203 columns per thread); a peaked row, a flat one and an ignored one."""
    rng = np.random.default_rng(51865)
    x = rng.standard_normal((3, 51865)) * np.array([[6.0], [0.1], [3.0]])
    x[0, 50257] += 40.0
    check_ce(hip, "V51865", x, 51865, 51872, 51872, [50257, 51864, -100], 3.0)


def test_ce_bwd_refusals(hip):
    logits = torch.zeros((4, 128), dtype=torch.float32, device=DEV)
    dl = torch.full((4, 128), 7.0, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="target"):
        hip.dec_ce_bwd(logits, 127, [0, 127, 1, 2], dlogits=dl)
    with pytest.raises(ValueError, match="shape"):
        hip.dec_ce_bwd(logits, 129, [0, 1, 1, 2], dlogits=dl)
    torch.cuda.synchronize()
    assert bool((dl == 7.0).all()), "a refused call launched"


# ------------------------------------------------------------------------------------------------------------ 3. embedding
def run_embed_bwd(hip, dh, ids, Vp, max_pos, pos_offset, base_t, base_p):
    B, L, Dm = dh.shape
    dt, dp = torch.from_numpy(base_t.astype(np.float32)).to(DEV), torch.from_numpy(base_p.astype(np.float32)).to(DEV)
    hip.dec_embed_bwd(dev_bf16(dh.reshape(B * L, Dm)), ids, dt, dp, pos_offset)
    torch.cuda.synchronize()
    return dt, dp


@pytest.mark.parametrize("case", ["one-token", "mixed"])
def test_embed_bwd_against_float64(hip, case):
    """One token at every position of every utterance (B L rows into one table row); a mix with an id used once and a padded
    vocabulary tail that is never touched.  D = 320: more columns than threads.  `+=` onto a non-zero table; two runs bit-identical."""
    rng = np.random.default_rng(9)
    B, L, Dm, Vp, max_pos, pos_offset = 4, 6, 320, 64, 16, 3
    ids = np.full((B, L), 5) if case == "one-token" else rng.integers(0, 12, (B, L))
    if case == "mixed":
        ids[ids == 39] = 0
        ids[2, 4] = 39  # used once
    dh = WR.bf16_round(rng.standard_normal((B, L, Dm)))
    base_t, base_p = rng.standard_normal((Vp, Dm)).astype(np.float32).astype(np.float64), rng.standard_normal((max_pos, Dm)).astype(np.float32).astype(np.float64)
    dt, dp = run_embed_bwd(hip, dh, ids, Vp, max_pos, pos_offset, base_t, base_p)
    dt2, dp2 = run_embed_bwd(hip, dh, ids, Vp, max_pos, pos_offset, base_t, base_p)
    assert torch.equal(dt.view(torch.int32), dt2.view(torch.int32)) and torch.equal(dp.view(torch.int32), dp2.view(torch.int32)), "two runs differ"
    rt, rp, at, ap = TR.embed_bwd(dh, ids, Vp, max_pos, pos_offset)
    counts = np.bincount(ids.reshape(-1), minlength=Vp)[:, None]
    bar_t = (counts + 1) * U * (at + np.abs(base_t))
    bar_p = (B + 1) * U * (ap + np.abs(base_p))
    e_t, e_p = np.abs(f64(dt) - (base_t + rt)), np.abs(f64(dp) - (base_p + rp))
    used = counts[:, 0] > 0
    print(f"embed_bwd {case}: tokens worst err/bar {float((e_t[used] / bar_t[used]).max()):.3f}, positions "
          f"{float((e_p[pos_offset:pos_offset + L] / bar_p[pos_offset:pos_offset + L]).max()):.3f}; {int(used.sum())} unique ids")
    assert (e_t <= bar_t).all() and (e_p <= bar_p).all()
    assert (f64(dt)[~used] == base_t[~used]).all(), "a table row of an unused id was touched"
    untouched = np.ones(max_pos, bool)
    untouched[pos_offset:pos_offset + L] = False
    assert (f64(dp)[untouched] == base_p[untouched]).all(), "a position outside the sequence was touched"


def test_embed_bwd_refusals(hip):
    B, L, Dm, Vp, max_pos = 2, 3, 64, 16, 8
    dh = dev_bf16(np.ones((B * L, Dm)))
    dt, dp = torch.zeros((Vp, Dm), device=DEV), torch.zeros((max_pos, Dm), device=DEV)
    for bad in (Vp, -1):
        ids = np.zeros((B, L), dtype=np.int64)
        ids[1, 1] = bad
        with pytest.raises(ValueError, match="uniq"):
            hip.dec_embed_bwd(dh, ids, dt, dp)
    with pytest.raises(ValueError, match="overrun"):
        hip.dec_embed_bwd(dh, np.zeros((B, L), dtype=np.int64), dt, dp, pos_offset=max_pos - L + 1)
    torch.cuda.synchronize()
    assert bool((dt == 0).all()) and bool((dp == 0).all()), "a refused call launched"


# ------------------------------------------------------------------------------------------------------------ 4. LayerNorm
@pytest.mark.parametrize("C", [128, 768, 1280])
def test_layernorm_product_entries_equal_the_debug_entries(hip, C):
    """ssak_layernorm_fwd_stats / ssak_layernorm_bwd call the templates the debug entries call: every output bit for bit."""
    g = torch.Generator().manual_seed(C)
    M = 37
    rnd = lambda *s: torch.randn(*s, generator=g)
    y, res, g1, g2, g_res = (rnd(M, C).to(torch.bfloat16).to(DEV) for _ in range(5))
    gamma, beta = (1 + 0.1 * rnd(C)).to(DEV), (0.1 * rnd(C)).to(DEV)
    outs = []
    for fwd, bwd in ((hip.layernorm_fwd_stats, hip.layernorm_bwd), (None, None)):
        r, out = (torch.full((M, C), NAN, dtype=torch.bfloat16, device=DEV) for _ in range(2))
        mean, rstd = (torch.full((M,), NAN, device=DEV) for _ in range(2))
        dr = torch.full((M, C), NAN, dtype=torch.bfloat16, device=DEV)
        dgamma, dbeta = torch.full((C,), 0.5, device=DEV), torch.full((C,), -0.25, device=DEV)
        if fwd is not None:
            fwd(y, res, gamma, beta, out, mean, rstd, r_out=r)
            bwd(g1, g2, r, mean, rstd, gamma, g_res, dr, dgamma, dbeta)
        else:
            hip.debug_layernorm_fwd(y, res, gamma, beta, r, out, mean, rstd)
            hip.debug_layernorm_bwd(g1, g2, r, mean, rstd, gamma, g_res, dr, None, dgamma, dbeta)
        torch.cuda.synchronize()
        outs.append((bits(r), bits(out), mean.view(torch.int32), rstd.view(torch.int32), bits(dr), dgamma.view(torch.int32), dbeta.view(torch.int32)))
        assert all(bool(torch.isfinite(t).all()) for t in (r, out, mean, rstd, dr, dgamma, dbeta))
    for name, a, b in zip(("r", "out", "mean", "rstd", "dr", "dgamma", "dbeta"), *outs):
        assert torch.equal(a, b), f"C={C}: {name} differs from the debug entry's"
    assert hip.lib.ssak_layernorm_bwd_workspace_bytes(C) == hip.lib.ssak_debug_layernorm_bwd_workspace_bytes(C)
