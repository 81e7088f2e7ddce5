"""GPU: the fused attention of ssak_amd/csrc/attention.hip (attn_fwd_kernel<DROP, 2>, attn_bwd_dq_kernel<DROP, 2>,
attn_bwd_dkv_kernel<DROP, 2, MASK>) through ssak_attention_fwd / _bwd / _bwd_bias, against the float64 restatement
tests/attention_ref.py (itself pinned to torch float64 autograd by tests/test_attention_ref.py).

Cases (head_dim 64 throughout): F in {1, 2, 63, 64, 65, 127, 128, 129, 255, 257, 499, 1500} (one, two, partial and whole 64-key
tiles and 128-query blocks), each with the key lengths {0, 1, 63, 64, 65, 127, 128, 129, F - 1, F, F + 5, -3} mixed in one batch;
the engine's shapes (wav2vec2-base B = 32, F = 499, nh = 12 with dropout 0.1; XLSR-large nh = 16, F = 749 ragged; Whisper-small
nh = 12 and Whisper-tiny nh = 6 at F = 1500 without a mask).  Score regimes: "mild" (std ~0.6: near-uniform softmax), "peaked"
(std ~5, the row maximum planted in the first key tile for some 16-query groups and in the last valid tile for others, so the
running maximum moves early and late), "large" (scaled scores in the thousands: an unshifted exp overflows fp32; q and k are
multiples of 4 up to 16, so the 64-term score sums are exact in fp32 and the exponent path alone is tested); and an exact
rescale case where the maximum moves by 0.0098, 1.25 or 0.0098 per tile with probabilities that are exactly 1.  Dropout
p in {0, 0.1, 0.5} with the oracle mask, including utterances with klen = 0.  K and V rows at keys >= klen are poisoned
(K = 2 Q of the same row, V = +-1000): a leaked key is a gross error, not a 1 / klen one.

Bars.  u8 = 2^-8 (a bf16 rounding, round to nearest, moves a value by at most 2^-8 of itself), u = 2^-24 (fp32).  The reference
runs on the kernels' bf16 inputs; the backward gets the kernels' own ctx and lse, so forward errors enter through delta and lse.

* Exponent errors (relative error of each probability).  Forward: the 64-term MFMA score sum (2 roundings against
  amax = scale max_k sum|q k|), the fma s c2 - mc (c2 = scale log2 e) and v_exp_f32 give <= 4 u (amax log2 e + 1) ~ 6 u amax + 4 u;
  the rescale factor alpha = exp2(fma(m, c2, -fl(m c2))) of a tile whose maximum did not move is not exactly 1 once |m c2| is
  large, and tile j's terms keep alpha^(nkt - 1 - j): <= (nkt - 1) u |m c2| ln 2 = (nkt - 1) u |smax| more.  eta_f = u (6 amax +
  nkt |smax| + 4).  Backward: P = exp2(s c2 - lse2), lse2 = fl(lse log2 e - log2(scale / (1 - p))): the stored lse's error
  (below) plus u (6 amax + 6 |lse| + 6) = eta_b.
* lse (absolute): eta_f (the row sum) + 4 u (|smax| + 24) (m scale in fp32 and __logf of the row sum, which is < 2^12 F: the
  exponent offset may sit up to 12 / c2 below the maximum, attention.hip softmax_offset): k u (|m scale| + 1) form.
* ctx:  2 u8 ctx_mag (P rounded to bf16 into the MFMA, the store) + 2 eta_f ctx_mag (numerator and row sum),  ctx_mag = Pd |v|.
* delta: sum_d |dO_d| bar(ctx_d) (the kernel sums dO against its stored ctx) + 16 u delta_mag (fp32 sum of 64 products).
* dv:   2 u8 dv_mag (Pd rounded, the store) + 2 eta_b dv_mag.
* dq:   2 u8 dq_mag (dS rounded, the store) + eta_b dq_mag2 (P's error times |dP m ds - delta|) + D dq_magp (delta's error D =
  bar(delta) + 4 u dpmax ds, with the fp32 dP, times scale sum P |k|).
* dk:   the same with the dk companions; eta_b and D are the worst over the (b, h) slice, since dk sums over queries.
* Relative L2 over each tensor: every rounding of a term t moves it by at most u8 |t| and has variance <= u8^2 t^2 / 3 (uniform
  in +- half an ulp, ulp <= 2^-7 |t|), so E|err_i|^2 <= u8^2 / 3 (sum_terms t^2 + ref_i^2) + (the exponent terms above, taken
  whole) + (scale sum P |k|)^2 var(delta) for dq / dk, var(delta) = sum_d dO_d^2 var(ctx_d) (its largest over the (b, h) slice
  for dk); bar = 1.5 sqrt(sum_i E|err_i|^2) / ||ref|| (skipped where ref = 0).  The squared-term sums are the *_sq companions.

Measured on an MI355X (worst error / bar over all cases): ctx 0.90, lse 0.62, delta 0.25, dq 0.62, dk 0.24, dv 0.89; relative L2
2.3e-3 on ctx, dq, dk, dv and delta at the engine's shapes (bars 4.8e-3 to 1.3e-2), <= 0.51 of its bar everywhere.  Scratch
mutations each fail this file: forward edge mask >= -> > and dK / dV key mask < -> <= (30+ cases each), the rescale skip
alpha != 1 -> alpha < 0.99 (test_running_maximum_rescale_is_exact and two more), dQ's delta without / (1 - p) (every dropout case), lse
times 1 + 1e-3 (31 cases); test_gpu_ops.py's attention tests miss the rescale and the lse ones.
* Exact: dK = dV = 0 bit for bit at padded keys; an utterance with klen <= 0 gives ctx = 0, lse = -inf, dqkv = 0; no NaN or inf
  anywhere else; klens = None and klens = [F] * B bit-identical (MASK = false against true in dK / dV); with p = 0 an utterance
  alone and one head repacked as nh = 1 bit-identical to the batch (strides, grid mapping); two runs bit-identical; nothing
  outside the output slices written; the bias column sums to fp32 summation noise of the stored dqkv.
"""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attention_ref as AR  # noqa: E402
from oracle import dropout_hash as DH  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8, U = 2.0 ** -8, 2.0 ** -24
SEED, STREAM = 0x1234ABCD5678, DH.ds_attn(7)
EDGE_F = (1, 2, 63, 64, 65, 127, 128, 129, 255, 257, 499, 1500)
POISON_V = 1000.0
# underflow: the forward may lose terms below 2^-114 of a row's largest probability (a rescale factor that underflows: its
# exponent offset can sit 12 below the maximum, attention.hip softmax_offset), the backward probabilities below 2^-126; times
# the dropout scale (<= 2), |v|, |dO|, |k| (< 8 here) and <= 2048 keys: < 2^-99
TINY = 2.0 ** -99


def _hip():
    import ssak_amd.hip as hip
    return hip


def edge_klens(F):
    return [0, 1, 63, 64, 65, 127, 128, 129, F - 1, F, F + 5, -3]


# ------------------------------------------------------------------ inputs
def make_inputs(B, F, nh, klens, regime, seed):
    """bf16 qkv [B*F, 3H] and dctx [B*F, H] on the device; K / V rows at keys >= klen poisoned."""
    g = torch.Generator().manual_seed(seed)
    H = nh * 64
    kls = AR.clamp_klens(klens, B, F)
    if regime == "large":
        mag = torch.randint(2, 5, (B, F, 2, nh, 64), generator=g).double() * 4  # 8, 12, 16: products are multiples of 64
        sgn = torch.randint(0, 2, (B, F, 2, nh, 64), generator=g).double() * 2 - 1
        qk = mag * sgn
    else:
        sd = 0.8 if regime == "mild" else 2.2
        qk = torch.randn(B, F, 2, nh, 64, generator=g, dtype=torch.float64) * sd
    v = torch.randn(B, F, nh, 64, generator=g, dtype=torch.float64)
    if regime in ("peaked", "large"):
        # per 16-query group: 0 -> maximum planted in the first key tile, 1 -> in the last valid tile, 2 -> none
        for b in range(B):
            kl = kls[b]
            if kl == 0:
                continue
            for i in range(F):
                pat = (i // 16) % 3
                if pat == 2:
                    continue
                t = (7 * i) % min(kl, 64) if pat == 0 else kl - 1 - (i % min(kl, 64))
                if regime == "peaked":
                    qk[b, i, 0] = 0.3 * qk[b, i, 0] + 0.6 * qk[b, t, 1]
                else:
                    qk[b, i, 0] = qk[b, t, 1]
    for b in range(B):  # poisoned padding: K aligned with the same row's Q, V = +-1000
        kl = kls[b]
        if kl < F:
            qk[b, kl:, 1] = 2 * qk[b, kl:, 0]
            v[b, kl:] = POISON_V * (torch.randint(0, 2, (F - kl, nh, 64), generator=g).double() * 2 - 1)
    qkv = torch.cat([qk[:, :, 0].reshape(B, F, H), qk[:, :, 1].reshape(B, F, H), v.reshape(B, F, H)], -1).reshape(B * F, 3 * H)
    dctx = torch.randn(B * F, H, generator=g) * 0.5
    return qkv.to(torch.bfloat16).to(DEV), dctx.to(torch.bfloat16).to(DEV)


# ------------------------------------------------------------------ launches (explicit outputs: delta is returned too)
def run_fwd(qkv, B, F, nh, klens, p, ctx=None, lse=None):
    hip = _hip()
    H = qkv.shape[1] // 3
    ctx = torch.full((B * F, H), float("nan"), dtype=torch.bfloat16, device=DEV) if ctx is None else ctx
    lse = torch.full((B, nh, F), float("nan"), device=DEV) if lse is None else lse
    kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device=DEV)
    hip.check(hip.lib.ssak_attention_fwd(hip.ptr(qkv), hip.ptr(ctx), hip.ptr(lse), hip.ptr(kl), B, F, nh, H, float(p), SEED, STREAM,
                                         hip.stream()))
    return ctx, lse


def run_bwd(qkv, ctx, lse, dctx, B, F, nh, klens, p, delta=None, dqkv=None):
    hip = _hip()
    H = qkv.shape[1] // 3
    delta = torch.full((B, nh, F), float("nan"), device=DEV) if delta is None else delta
    dqkv = torch.full_like(qkv, float("nan")) if dqkv is None else dqkv
    kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device=DEV)
    hip.check(hip.lib.ssak_attention_bwd(hip.ptr(qkv), hip.ptr(ctx), hip.ptr(lse), hip.ptr(kl), hip.ptr(dctx), hip.ptr(delta),
                                         hip.ptr(dqkv), B, F, nh, H, float(p), SEED, STREAM, 0, hip.stream()))
    return delta, dqkv


# ------------------------------------------------------------------ bars
def _rows_to_elems(x, B, F, nh):
    """[B, nh, F] per-row values -> [B*F, nh*64] (each row's value on its head's 64 columns)."""
    return x.permute(0, 2, 1)[..., None].expand(B, F, nh, 64).reshape(B * F, nh * 64)


def _bh_max(x, B, F, nh):
    return _rows_to_elems(x.amax(-1, keepdim=True).expand(B, nh, F), B, F, nh)


def check_case(qkv, dctx, B, F, nh, klens, p):
    """Run forward and backward, hold every output to its bar; returns {name: worst error / bar} (the test asserts <= 1)."""
    H = nh * 64
    kls = AR.clamp_klens(klens, B, F)
    ctx, lse = run_fwd(qkv, B, F, nh, klens, p)
    delta, dqkv = run_bwd(qkv, ctx, lse, dctx, B, F, nh, klens, p)
    torch.cuda.synchronize()
    r = AR.attention(qkv, B, F, nh, klens, dctx, p=p, seed=SEED, stream_id=STREAM, device=DEV)
    ds = DH.engine_scale(p) if DH.thresh16(p) else 1.0
    out = {}

    # ---- exact conventions
    for name, t in (("ctx", ctx), ("delta", delta), ("dqkv", dqkv)):
        assert torch.isfinite(t).all(), f"{name}: non-finite values"
    assert not torch.isnan(lse).any()
    for b, kl in enumerate(kls):
        rows = slice(b * F, (b + 1) * F)
        pad = dqkv[b * F + kl:(b + 1) * F, H:]  # dK | dV of padded keys
        assert bool((pad.view(torch.int16) == 0).all()), f"utterance {b}: dK / dV at padded keys not +0"
        if kl == 0:
            assert bool((ctx[rows].view(torch.int16) == 0).all()) and bool((dqkv[rows].view(torch.int16) == 0).all()), b
            assert bool(torch.isneginf(lse[b]).all()), b
        else:
            assert torch.isfinite(lse[b]).all(), b

    # ---- exponent-error and delta-error terms
    nkt = torch.tensor([math.ceil(kl / 64) for kl in kls], dtype=torch.float64, device=DEV)[:, None, None]
    fin = torch.isfinite(r["smax"])
    smax = torch.where(fin, r["smax"].abs(), torch.zeros_like(r["smax"]))
    lse_abs = torch.where(fin, r["lse"].abs(), torch.zeros_like(r["lse"]))
    eta_f = U * (6 * r["amax"] + nkt * smax + 4)
    lse_bar = eta_f + 4 * U * (smax + 24)
    eta_b = lse_bar + U * (6 * r["amax"] + 6 * lse_abs + 6)
    e = lambda x: _rows_to_elems(x, B, F, nh)
    m = lambda x: _bh_max(x, B, F, nh)

    def ratio(name, got, ref, bar):
        bar = bar + TINY
        err = (got.double() - ref).abs()
        bad = err > bar
        worst = float((err / bar.clamp_min(1e-300)).max()) if err.numel() else 0.0
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements over the bar, worst err/bar {worst:.3g}"
        out[name] = worst

    def rel_l2(name, got, ref, var):
        nref = float(ref.norm())
        if nref == 0.0:  # (e.g. dq at F = 1: dS = P (dP - delta) = 0 exactly; the elementwise bar holds what the kernel leaves)
            return
        rl = float((got.double() - ref).norm()) / nref
        bar = 1.5 * math.sqrt(float(var.sum())) / nref
        assert rl <= bar, f"{name}: rel L2 {rl:.3g} over its bar {bar:.3g}"
        out[name + "_relL2"] = rl
        out[name + "_relL2_bar"] = bar

    ctx_bar = 2 * U8 * r["ctx_mag"] + 2 * e(eta_f) * r["ctx_mag"] + TINY
    ratio("ctx", ctx, r["ctx"], ctx_bar)
    rel_l2("ctx", ctx, r["ctx"], U8 ** 2 / 3 * (r["ctx_sq"] + r["ctx"] ** 2) + (2 * e(eta_f) * r["ctx_mag"]) ** 2)
    ok = torch.isfinite(r["lse"])
    ratio("lse", lse[ok], r["lse"][ok], lse_bar[ok])

    do = dctx.double().abs()
    delta_bar = (do * ctx_bar).view(B, F, nh, 64).sum(-1).permute(0, 2, 1) + 16 * U * r["delta_mag"]
    ratio("delta", delta, r["delta"], delta_bar)
    ctx_var = U8 ** 2 / 3 * (r["ctx_sq"] + r["ctx"] ** 2)
    delta_var = (do ** 2 * ctx_var).view(B, F, nh, 64).sum(-1).permute(0, 2, 1)
    rel_l2("delta", delta, r["delta"], delta_var + (16 * U * r["delta_mag"]) ** 2)
    D = delta_bar + 4 * U * r["dpmax"] * ds

    dq, dk, dv = dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:]
    dq_extra = e(eta_b) * r["dq_mag2"] + e(D) * r["dq_magp"]
    dk_extra = m(eta_b) * r["dk_mag2"] + m(D) * r["dk_magp"]
    dv_extra = 2 * m(eta_b) * r["dv_mag"]
    ratio("dq", dq, r["dq"], 2 * U8 * r["dq_mag"] + dq_extra)
    ratio("dk", dk, r["dk"], 2 * U8 * r["dk_mag"] + dk_extra)
    ratio("dv", dv, r["dv"], 2 * U8 * r["dv_mag"] + dv_extra)
    # (delta's error enters the variances as its own variance, not its bound)
    rel_l2("dq", dq, r["dq"], U8 ** 2 / 3 * (r["dq_sq"] + r["dq"] ** 2) + (e(eta_b) * r["dq_mag2"]) ** 2 + r["dq_magp"] ** 2 * e(delta_var))
    rel_l2("dk", dk, r["dk"], U8 ** 2 / 3 * (r["dk_sq"] + r["dk"] ** 2) + (m(eta_b) * r["dk_mag2"]) ** 2 + r["dk_magp"] ** 2 * m(delta_var))
    rel_l2("dv", dv, r["dv"], U8 ** 2 / 3 * (r["dv_sq"] + r["dv"] ** 2) + dv_extra ** 2)
    return out


# ------------------------------------------------------------------ accuracy against float64
EDGE_CASES = [(F, "mild", 0.0) for F in EDGE_F]
EDGE_CASES += [(F, "peaked", 0.0) for F in (65, 129, 257, 499, 1500)]
EDGE_CASES += [(F, "large", 0.0) for F in (64, 129, 257, 499, 1500)]
EDGE_CASES += [(1, "mild", 0.1), (65, "mild", 0.1), (257, "mild", 0.5), (499, "peaked", 0.1), (128, "large", 0.5),
               (1500, "mild", 0.1)]


@pytest.mark.parametrize("F,regime,p", EDGE_CASES)
def test_edges_against_float64(F, regime, p):
    """Block and tile edges of F, every key-length edge in one batch (0 and negative: empty utterances; F + 5: clamped),
    three score regimes, dropout with the oracle mask."""
    B, nh = 12, 2
    klens = edge_klens(F)
    qkv, dctx = make_inputs(B, F, nh, klens, regime, seed=F * 31 + len(regime) + int(p * 10))
    check_case(qkv, dctx, B, F, nh, klens, p)


REAL_CASES = [  # name, B, F, nh, klens, p
    ("wav2vec2-base", 32, 499, 12, [499 - 13 * i for i in range(32)], 0.1),
    ("xlsr-large", 3, 749, 16, [749, 400, 130], 0.1),
    ("whisper-small", 2, 1500, 12, None, 0.0),
    ("whisper-tiny", 3, 1500, 6, None, 0.0),
]


@pytest.mark.parametrize("name,B,F,nh,klens,p", REAL_CASES, ids=[c[0] for c in REAL_CASES])
def test_engine_shapes_against_float64(name, B, F, nh, klens, p):
    qkv, dctx = make_inputs(B, F, nh, klens, "mild", seed=F + nh)
    check_case(qkv, dctx, B, F, nh, klens, p)


def rescale_inputs(F, kls, nh=2):
    """Every query q = [16, 1.25, 0...]; in utterance 0 keys 0-7 are [16, 1, 0...] and key e of the last tile is [16, 1.0625, 0...]
    (the maximum moves by 0.0098 in the last tile: alpha = 0.9903), in utterance 1 key e is [16, 9, 0...] (a move of 1.25), in
    utterance 2 the maximum stays in the first tile, in utterance 3 key 64 t is [16, 1 + t / 16, 0...] (a move of 0.0098 in
    every tile).  Other keys are [-16, 0...] (64 scaled units lower: probability ~1e-28).  The planted keys have probability
    exactly 1 (bf16 has no rounding to do on them), their V rows are +1 before the last tile and -1 in it; P is exact, so the
    result is held to one bf16 rounding of itself.  The moving keys sit at tile positions 0 mod 16 (lane group 0, whose maximum
    the forward's exponent offset follows: attention.hip softmax_offset); e = 32 into the last tile, or its first key."""
    B = len(kls)
    H = nh * 64
    g = torch.Generator().manual_seed(F)
    q = torch.zeros(B, F, nh, 64)
    q[..., 0], q[..., 1] = 16.0, 1.25
    k = torch.zeros(B, F, nh, 64)
    k[..., 0] = -16.0
    v = torch.randn(B, F, nh, 64, generator=g)
    for b, kl in enumerate(kls):
        k[b, :8, :, 0], k[b, :8, :, 1] = 16.0, 1.0
        v[b, :8] = 1.0
        if b == 0 or b == 1:
            e = 64 * ((kl - 1) // 64) + (32 if 64 * ((kl - 1) // 64) + 32 < kl else 0)
            k[b, e, :, 0], k[b, e, :, 1] = 16.0, 1.0625 if b == 0 else 9.0
            v[b, e] = -1.0
        if b == 3:
            for t in range(1, math.ceil(kl / 64)):
                k[b, 64 * t, :, 0], k[b, 64 * t, :, 1] = 16.0, 1.0 + t / 16
                v[b, 64 * t] = -1.0 if t % 2 else 1.0
    qkv = torch.cat([q.reshape(B, F, H), k.reshape(B, F, H), v.reshape(B, F, H)], -1).reshape(B * F, 3 * H)
    dctx = torch.randn(B * F, H, generator=g) * 0.5
    return qkv.to(torch.bfloat16).to(DEV), dctx.to(torch.bfloat16).to(DEV)


def test_running_maximum_rescale_is_exact():
    """The online softmax's accumulator rescale when the running maximum moves by a little (alpha = 0.9903), by a lot and
    in every tile (rescale_inputs): with exact probabilities ctx is held to u8 |ctx| + 1e-5 ctx_mag, where a skipped
    rescale is a ~1 % error.  The backward runs on the same inputs under the general bars."""
    F, nh = 300, 2
    kls = [300, 300, 129, 300]
    qkv, dctx = rescale_inputs(F, kls, nh)
    ctx, lse = run_fwd(qkv, len(kls), F, nh, kls, 0.0)
    r = AR.attention(qkv, len(kls), F, nh, kls, device=DEV)
    err = (ctx.double() - r["ctx"]).abs()
    bar = U8 * r["ctx"].abs() + 1e-5 * r["ctx_mag"]
    assert bool((err <= bar).all()), float((err / bar).max())
    check_case(qkv, dctx, len(kls), F, nh, kls, 0.0)


# ------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("F,p", [(65, 0.0), (499, 0.1), (130, 0.5)])
def test_no_klens_equals_full_klens(F, p):
    """klens = None (dK / dV without MASK) and klens = [F] * B (with it) are bit-identical, forward and backward; so are two
    runs."""
    B, nh = 3, 2
    qkv, dctx = make_inputs(B, F, nh, None, "peaked", seed=F)
    a = run_fwd(qkv, B, F, nh, None, p)
    b = run_fwd(qkv, B, F, nh, [F] * B, p)
    a2 = run_fwd(qkv, B, F, nh, None, p)
    ga = run_bwd(qkv, *a, dctx, B, F, nh, None, p)
    gb = run_bwd(qkv, *b, dctx, B, F, nh, [F] * B, p)
    ga2 = run_bwd(qkv, *a2, dctx, B, F, nh, None, p)
    for x, y, z in zip(a + ga, b + gb, a2 + ga2):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_utterance_and_head_independence():
    """p = 0: utterance b run alone (B = 1) and head h repacked as an nh = 1 q|k|v are bit-identical to the same rows of the
    B = 2, nh = 12 run (B nh = 24: the XCD-grouped grid mapping; alone, B nh = 12 and 2: the plain one)."""
    B, F, nh = 2, 257, 12
    H = nh * 64
    klens = [257, 130]
    qkv, dctx = make_inputs(B, F, nh, klens, "peaked", seed=4)
    ctx, lse = run_fwd(qkv, B, F, nh, klens, 0.0)
    delta, dqkv = run_bwd(qkv, ctx, lse, dctx, B, F, nh, klens, 0.0)
    for b in range(B):
        rows = slice(b * F, (b + 1) * F)
        c1, l1 = run_fwd(qkv[rows].contiguous(), 1, F, nh, klens[b:b + 1], 0.0)
        d1, g1 = run_bwd(qkv[rows].contiguous(), c1, l1, dctx[rows].contiguous(), 1, F, nh, klens[b:b + 1], 0.0)
        assert torch.equal(c1, ctx[rows]) and torch.equal(l1[0], lse[b]) and torch.equal(d1[0], delta[b]) and torch.equal(g1, dqkv[rows])
    for h in (0, 5, 11):
        cols = [slice(j * H + h * 64, j * H + (h + 1) * 64) for j in range(3)]
        q1 = torch.cat([qkv[:, c] for c in cols], 1).contiguous()
        c1, l1 = run_fwd(q1, B, F, 1, klens, 0.0)
        d1, g1 = run_bwd(q1, c1, l1, dctx[:, h * 64:(h + 1) * 64].contiguous(), B, F, 1, klens, 0.0)
        assert torch.equal(c1, ctx[:, h * 64:(h + 1) * 64]) and torch.equal(l1[:, 0], lse[:, h]) and torch.equal(d1[:, 0], delta[:, h])
        assert torch.equal(g1, torch.cat([dqkv[:, c] for c in cols], 1))


@pytest.mark.parametrize("F,p", [(1, 0.0), (65, 0.1), (129, 0.0), (257, 0.5)])
def test_writes_stay_inside_the_outputs(F, p):
    """ctx, lse, delta, dqkv, the bias workspace and bias_grad each sit inside a larger sentinel-filled buffer: nothing
    outside the slice changes (the last query block is partial), and the slices equal a plain run's."""
    hip = _hip()
    B, nh = 3, 2
    H = nh * 64
    klens = [F, 0, max(F - 3, 1)]
    qkv, dctx = make_inputs(B, F, nh, klens, "mild", seed=F + 5)
    ref_ctx, ref_lse = run_fwd(qkv, B, F, nh, klens, p)
    ref_delta, ref_dqkv = run_bwd(qkv, ref_ctx, ref_lse, dctx, B, F, nh, klens, p)
    PAD = 4096

    def framed(n, dtype, fill):
        buf = torch.full((PAD + n + PAD,), fill, dtype=dtype, device=DEV)
        return buf, buf[PAD:PAD + n]

    def untouched(buf, n, fill):
        outside = torch.cat([buf[:PAD], buf[PAD + n:]])
        return bool((outside.view(torch.int16 if outside.dtype == torch.bfloat16 else torch.int32) ==
                     torch.tensor([fill], dtype=outside.dtype).view(torch.int16 if outside.dtype == torch.bfloat16 else torch.int32).item()).all())

    cb, cv = framed(B * F * H, torch.bfloat16, 7.0)
    lb, lv = framed(B * nh * F, torch.float32, 7.0)
    run_fwd(qkv, B, F, nh, klens, p, ctx=cv.view(B * F, H), lse=lv.view(B, nh, F))
    torch.cuda.synchronize()
    assert untouched(cb, B * F * H, 7.0) and untouched(lb, B * nh * F, 7.0)
    assert torch.equal(cv.view(B * F, H), ref_ctx) and torch.equal(lv.view(B, nh, F), ref_lse)
    db, dv_ = framed(B * nh * F, torch.float32, 7.0)
    gb, gv = framed(B * F * 3 * H, torch.bfloat16, 7.0)
    run_bwd(qkv, ref_ctx, ref_lse, dctx, B, F, nh, klens, p, delta=dv_.view(B, nh, F), dqkv=gv.view(B * F, 3 * H))
    torch.cuda.synchronize()
    assert untouched(db, B * nh * F, 7.0) and untouched(gb, B * F * 3 * H, 7.0)
    assert torch.equal(dv_.view(B, nh, F), ref_delta) and torch.equal(gv.view(B * F, 3 * H), ref_dqkv)
    # the bias entry: workspace of exactly the advertised size, bias_grad [3H]
    nbytes = hip.lib.ssak_attention_bwd_bias_workspace_bytes(B, F, H)
    wb, wv = framed(nbytes // 4, torch.float32, 7.0)
    bb, bv = framed(3 * H, torch.float32, 7.0)
    bv.zero_()
    db.fill_(7.0)
    gb.fill_(7.0)
    kl = torch.tensor(klens, dtype=torch.int32, device=DEV)
    hip.check(hip.lib.ssak_attention_bwd_bias(hip.ptr(qkv), hip.ptr(ref_ctx), hip.ptr(ref_lse), hip.ptr(kl), hip.ptr(dctx), hip.ptr(dv_),
                                              hip.ptr(gv), hip.ptr(bv), B, F, nh, H, float(p), SEED, STREAM, hip.ptr(wv), nbytes,
                                              hip.stream()))
    torch.cuda.synchronize()
    for buf, n in ((db, B * nh * F), (gb, B * F * 3 * H), (wb, nbytes // 4), (bb, 3 * H)):
        assert untouched(buf, n, 7.0)
    assert torch.equal(gv.view(B * F, 3 * H), ref_dqkv) and torch.equal(dv_.view(B, nh, F), ref_delta)


@pytest.mark.parametrize("F,p", [(1, 0.0), (63, 0.1), (129, 0.0), (255, 0.5), (499, 0.1)])
def test_bias_sums_at_the_edges(F, p):
    """ssak_attention_bwd_bias over the edge key lengths (empty utterances, clamped ones, poisoned padding): dqkv
    bit-identical to ssak_attention_bwd's and bias_grad - start equal to the float64 column sums of the stored dqkv within
    fp32 summation noise, 2e-6 sum|dqkv| + 1e-6 (the bound of test_gpu_ops.py's bias test)."""
    hip = _hip()
    B, nh = 12, 2
    H = nh * 64
    klens = edge_klens(F)
    qkv, dctx = make_inputs(B, F, nh, klens, "peaked", seed=F + 77)
    ctx, lse = run_fwd(qkv, B, F, nh, klens, p)
    _, ref = run_bwd(qkv, ctx, lse, dctx, B, F, nh, klens, p)
    start = torch.randn(3 * H, generator=torch.Generator().manual_seed(F)).to(DEV)
    kw = dict(drop_p=p, seed=SEED, stream_id=STREAM)
    got, bias = hip.attention_bwd_bias(qkv, ctx, lse, dctx, B, F, nh, torch.tensor(klens), bias_grad=start.clone(), **kw)
    assert torch.equal(got, ref)
    want = ref.double().sum(0)
    tol = 2e-6 * ref.double().abs().sum(0) + 1e-6
    err = (bias.double() - start.double() - want).abs()
    assert bool((err <= tol).all()), float(err.max())


# ------------------------------------------------------------------ rejections
def test_argument_errors_before_any_launch():
    """head_dim != 64 and dropout with F > 16384 are argument errors (ValueError) raised before anything is launched: the
    buffers handed over are far too small for the shapes named, so a launch would be out of bounds."""
    hip = _hip()
    small = torch.zeros(1024, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(256, device=DEV)
    for H, nh in ((96, 1), (128, 1), (192, 2)):  # head dims 96, 128, 96
        with pytest.raises(ValueError):
            hip.check(hip.lib.ssak_attention_fwd(hip.ptr(small), hip.ptr(small), hip.ptr(lse), None, 1, 4, nh, H, 0.0, 0, 0, hip.stream()))
        with pytest.raises(ValueError):
            hip.check(hip.lib.ssak_attention_bwd(hip.ptr(small), hip.ptr(small), hip.ptr(lse), None, hip.ptr(small), hip.ptr(lse),
                                                 hip.ptr(small), 1, 4, nh, H, 0.0, 0, 0, 0, hip.stream()))
    F = 16385
    with pytest.raises(ValueError):
        hip.check(hip.lib.ssak_attention_fwd(hip.ptr(small), hip.ptr(small), hip.ptr(lse), None, 1, F, 1, 64, 0.1, 0, 0, hip.stream()))
    with pytest.raises(ValueError):
        hip.check(hip.lib.ssak_attention_bwd(hip.ptr(small), hip.ptr(small), hip.ptr(lse), None, hip.ptr(small), hip.ptr(lse),
                                             hip.ptr(small), 1, F, 1, 64, 0.1, 0, 0, 0, hip.stream()))
    nbytes = hip.lib.ssak_attention_bwd_bias_workspace_bytes(1, F, 64)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        hip.check(hip.lib.ssak_attention_bwd_bias(hip.ptr(small), hip.ptr(small), hip.ptr(lse), None, hip.ptr(small), hip.ptr(lse),
                                                  hip.ptr(small), hip.ptr(lse), 1, F, 1, 64, 0.1, 0, 0, hip.ptr(ws), nbytes, hip.stream()))
    torch.cuda.synchronize()
    assert bool((small == 0).all()) and bool((lse == 0).all())
