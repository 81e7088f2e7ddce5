"""GPU: the grouped positional convolution (ssak_amd/csrc/posconv.hip: the direct kernels and their weight plumbing), one stage at a time,
against the float64 restatement tests/posconv_ref.py (itself pinned to torch's conv1d / weight_norm under float64 autograd by
tests/test_posconv_ref.py), through the test-only entries ssak_debug_posconv_prepare / _pack / _direct / _wgrad / _weight_bwd.
The references run in float64 on the device, on exactly the bf16 inputs and bf16 weights the kernels read, so only a kernel's own
arithmetic is judged.

Geometries: H = 768, G = 16 (cg = 48, wav2vec2-base) and H = 1024, G = 16 (cg = 64, XLSR-large); K = 128 (the models') and K = 16
(the smallest K both the direct kernel and the weight gradient accept: the direct kernel's step loop then runs 8 / 16 steps
instead of 64 / 128 before its peeled last pair, the weight gradient has one (cg = 48) or two (cg = 64) tap blocks).

Which kernel each test reaches:

* posconv_direct_kernel<48>, <64>, forward (row0 = 0: bias, saved pre-activation, GELU) and input gradient (row0 = 1, flipped
  taps in the wb layout): test_direct_real and test_direct_integer, F in {1, 63, 127, 128, 129, 499, 511, 512, 513, 1024, 1500}
  (one frame; around the 128-frame wave slice; around the 512-frame workgroup tile: 1, 2 and 3 tiles) x B in {1, 2, 3}, and the
  train shape B = 32, F = 499 (K = 128, real data).  Forward as the engine launches it (bias, pre, GELU), without bias and pre,
  and without GELU; the input gradient without any of them.
* posconv_frag_kernel<48>, <64>: every test_direct_* case (the fragment-ordered copy is made from the wf / wb layout on each call).
* posconv_wgrad_kernel<48>, <64> + posconv_wgrad_sum_kernel: test_wgrad, (B, F) with B (F + K) = 512 + {0, 1, 127, 128, 129, 511}
  (the 128-row stage and the four row ranges of ceil(ceil(rows / 128) / 4) * 128 rows each), (1, 1) (K + 1 rows: two -- for
  K = 16 three -- of the four row ranges are empty and must contribute zeros), (2, 499), (4, 1500), (32, 499); integer and
  real data; both launches of every case bit-identical.
* posconv_pack_kernel<bf16>, <float>: test_pack (and every direct / wgrad case through its results).
* posconv_colnorm_kernel + posconv_colnorm_finalize_kernel + posconv_materialize_kernel<bf16>, <float>: test_prepare.
* posconv_colnorm_kernel (dot) + finalize + posconv_wbwd_kernel: test_weight_bwd, on a random dwf and on the weight gradient
  kernel's own output.

Data.  Integer cases: h, dpre uniform in {-2 .. 2}, weights uniform in {-1, 0, 1} given directly in the wf / wb layouts, bias in
{-3 .. 3}: every product and partial sum is an integer below 2^24, so fp32 accumulation is exact in ANY order; independent
random values are asymmetric under every index swap.  Real cases (posconv_ref.weights_case / direct_activations / wgrad_activations): h, dpre ~ N(0, 1)
as bf16, v ~ 0.02 N(0, 1), g = tap norm * (1 + 0.1 N(0, 1)), bias ~ 0.1 N(0, 1); with B >= 2 the first and last 64 frames of every
utterance are 8 times larger, so a window that reaches the neighbouring utterance (or a pack that loses the zero gap) moves
the outputs near the boundary by many times their bar.

Bars (u = 2^-24; bf16 storage rounds by at most 2^-8 relative).  No element is excluded from any comparison.

* Integer cases: pre, out (no GELU) and dX EQUAL the bf16 rounding (nearest even; ties are frequent among integers above 256)
  of the float64 result, the forward with and without bias; dwf equals the float64 result.
* pre, dX, out without GELU:  |got - ref| <= 2^-8 |ref| + C_ACC u A,   A = sum |x| |w| (+ |bias|) per element.
* out with GELU (applied by the kernel to the fp32 sum, not to the rounded pre): with d = C_ACC u A,
  |got - gelu(ref_pre)| <= 2^-8 |gelu| + (|gelu'(ref_pre)| + 0.7979 d) d + 1.65e-5 |ref_pre| + 2^-22 |gelu|:
  gelu' over [ref_pre - d, ref_pre + d] is within sup |gelu''| d = 0.7979 d of gelu'(ref_pre); the last two terms are the error
  of the bf16 engine's logistic GELU fit as test_gpu_rowwise.py states and tests it.
* dwf:  |got - ref| <= C_WGRAD u A_w,   A_w = sum |x| |dy|.
* C_ACC = 16, C_WGRAD = 16 come from the reference, not from the kernels (posconv_ref.py, re-measured by
  test_posconv_ref.py::test_accumulation_constants): an fp32 emulation of the kernels' summation ORDER (32-term slices summed left
  to right, slice sums added to an fp32 accumulator in step order; the weight gradient in 128-row stages over four row ranges
  and a fixed-order final sum) differs from float64 by at most 1.034 u A (forward) and 1.461 u A_w (weight gradient) on a sample
  of this module's cases (same seeds; four direct shapes, six weight-gradient shapes on group 0 and four taps); 8 times that --
  the allowance for the undocumented rounding inside a matrix instruction's 32-term slice -- rounded up to a power of two.  With
  these constants the 2^-8 |ref| term dominates the activations' bars (C_ACC u A ~ 1e-6 A ~ 5e-5 |ref|).
* Guard rows after the B F rows of out / pre keep their sentinel; out / pre start as NaN and every element is written.
* norms (||v_k||^2): 1e-5 relative (fp32 sums of cg + H / 16 + 16 sequential positive terms: (cg + H / 16 + 16) u <= 8.6e-6).
  wf, wb as bf16: one bf16 ulp of the float64 g v / ||v||, at every index of both layouts; as fp32: 1e-5 relative (half the norms'
  bar through the inverse square root, plus the roundings of rsqrt and two products).  A tap with g[k] = 0 gives exact zeros, a tap
  with ||v_k|| ~ 1e-6 of the others' stays finite and inside the same bars.
* dg, dv are accumulated onto non-zero starting values:  |got - start - ref| <= 1e-5 sum |terms| + 2^-23 (|start| + |ref|) (the
  form of the LayerNorm parameter gradients), terms of dg[k]: |dw v| / ||v_k||, of dv: |g| / ||v_k|| (|dw| + |v| sum |dw v| / ||v_k||^2).
* pack: equality with the reference layout (K / 2 leading zero rows, K zero rows after every utterance, K trailing), from a
  NaN-filled destination.
"""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import posconv_ref as P  # noqa: E402
import rowwise_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
EPS_BF = 2.0 ** -8
GEOMS = ((768, 16), (1024, 16))
TAPS = (128, 16)
DIRECT_F = (1, 63, 127, 128, 129, 499, 511, 512, 513, 1024, 1500)
GUARD = 512  # rows after the B F rows of out / pre
SENTINEL = -7.0


def _hip():
    import ssak_amd.hip as hip
    return hip


def _bf(x):
    """float64 values -> a contiguous bf16 device tensor (round to nearest even; exact for values that are bf16 already)."""
    return x.to(DEV).to(F32).to(BF).contiguous()


def _f32(x):
    return x.to(DEV).to(F32).contiguous()


def _check(name, got, ref, bar):
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape, name
    err = (got - ref).abs()
    bad = ~(err <= bar)  # (a NaN is bad)
    if bad.any():
        k = int(torch.argmax(torch.where(bad, torch.nan_to_num(err - bar, nan=float("inf")), torch.full_like(err, -1.0))))
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.numel()} outside the bar; worst at flat index {k} of shape "
                             f"{tuple(err.shape)}: got {got.flatten()[k].item()!r} ref {ref.flatten()[k].item()!r} "
                             f"bar {bar.flatten()[k].item()!r}")
    print(f"{name}: max err / bar = {float(torch.where(err > 0, err / bar, err).max()):.3f}")


def _guarded(B, F, H):
    """[B F + GUARD, H] bf16: NaN where the kernel must write, the sentinel behind."""
    t = torch.full((B * F + GUARD, H), SENTINEL, dtype=BF, device=DEV)
    t[:B * F] = float("nan")
    return t


def _written_and_guarded(name, t, B, F):
    assert not torch.isnan(t[:B * F]).any(), f"{name}: {int(torch.isnan(t[:B * F]).sum())} elements were not written"
    assert (t[B * F:] == SENTINEL).all(), f"{name}: rows past B F were written"
    return t[:B * F].view(B, F, -1)


@functools.lru_cache(maxsize=2)
def _weights(H, G, K):
    """The real-valued weights of one geometry on the device: g, v, bias (fp32 values), w = bf16(weight(g, v)) as float64."""
    return {k: x.to(DEV) for k, x in P.weights_case(H, G, K).items()}


def _direct_cases():
    for H, G in GEOMS:
        for K in TAPS:
            for F in DIRECT_F:
                for B in (1, 2, 3):
                    yield pytest.param(H, G, K, B, F, id=f"H{H}-K{K}-B{B}-F{F}")


def _gelu_bar(ref_pre, ref_out, A):
    d = P.C_ACC * U * A
    return (EPS_BF * ref_out.abs() + (P.gelu_grad(ref_pre).abs() + P.GELU_CURVATURE * d) * d
            + RR.PHI_FIT_MAX_ERR * ref_pre.abs() + 2.0 ** -22 * ref_out.abs())


# ------------------------------------------------------------------------------------------------ direct kernel, real data
def run_direct_real(H, G, K, B, F):
    hip = _hip()
    wt = _weights(H, G, K)
    act = {k: x.to(DEV) for k, x in P.direct_activations(B, F, H, K).items()}
    w, bias = wt["w"], wt["bias"]
    h16, d16 = _bf(act["h"]).view(B * F, H), _bf(act["dpre"]).view(B * F, H)
    wf16, wb16, bias32 = _bf(P.to_wf(w)), _bf(P.to_wb(w)), _f32(bias)
    ws = hip.debug_posconv_workspace(B, F, H, G, K, DEV)
    conv, _ = P.forward(act["h"], w, None)
    A0 = P.forward_abs_sum(act["h"], w, None)
    # forward as the engine launches it: bias, saved pre-activation, GELU
    out, pre = _guarded(B, F, H), _guarded(B, F, H)
    hip.debug_posconv_direct(h16, wf16, bias32, out, pre, B, F, G, K, gelu=True, workspace=ws)
    torch.cuda.synchronize()
    ref_pre, A = conv + bias, A0 + bias.abs()
    ref_out = P.gelu(ref_pre)
    _check("pre", _written_and_guarded("pre", pre, B, F), ref_pre, EPS_BF * ref_pre.abs() + P.C_ACC * U * A)
    _check("out (gelu)", _written_and_guarded("out", out, B, F), ref_out, _gelu_bar(ref_pre, ref_out, A))
    # without bias and without the saved pre-activation
    out = _guarded(B, F, H)
    hip.debug_posconv_direct(h16, wf16, None, out, None, B, F, G, K, gelu=True, workspace=ws)
    torch.cuda.synchronize()
    _check("out (gelu, no bias, no pre)", _written_and_guarded("out", out, B, F), P.gelu(conv), _gelu_bar(conv, P.gelu(conv), A0))
    # without GELU: out and pre are the same rounding of the same sum
    out, pre = _guarded(B, F, H), _guarded(B, F, H)
    hip.debug_posconv_direct(h16, wf16, None, out, pre, B, F, G, K, gelu=False, workspace=ws)
    torch.cuda.synchronize()
    got = _written_and_guarded("out", out, B, F)
    _check("out (no gelu)", got, conv, EPS_BF * conv.abs() + P.C_ACC * U * A0)
    assert torch.equal(got, _written_and_guarded("pre", pre, B, F)), "pre and the GELU-less out differ"
    # input gradient: the same kernel on the packed gradient with the flipped taps, one row further down
    dx = _guarded(B, F, H)
    hip.debug_posconv_direct(d16, wb16, None, dx, None, B, F, G, K, row0=1, gelu=False, workspace=ws)
    torch.cuda.synchronize()
    ref_dx = P.grad_input(act["dpre"], w)
    _check("dX", _written_and_guarded("dX", dx, B, F), ref_dx, EPS_BF * ref_dx.abs() + P.C_ACC * U * P.grad_input_abs_sum(act["dpre"], w))


@pytest.mark.parametrize("H,G,K,B,F", list(_direct_cases()))
def test_direct_real(H, G, K, B, F):
    """Forward (three ways) and input gradient of posconv_direct_kernel on real-valued data, per element against float64."""
    run_direct_real(H, G, K, B, F)


@pytest.mark.parametrize("H,G", GEOMS)
def test_direct_real_train_shape(H, G):
    """The train step's launch: B = 32, F = 499, K = 128."""
    run_direct_real(H, G, 128, 32, 499)


# ------------------------------------------------------------------------------------------------ direct kernel, integers
@pytest.mark.parametrize("H,G,K,B,F", list(_direct_cases()))
def test_direct_integer(H, G, K, B, F):
    """Integer data: the fp32 sums are exact in any order, so pre / out / dX must EQUAL the bf16 rounding of the float64 result --
    a dropped or doubled tap, a transposed fragment, a swapped tap pair, a flipped tap or a truncating store all change it."""
    hip = _hip()
    cg = H // G
    gen = torch.Generator().manual_seed(7 * H + 3 * K + 100 * B + F)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).to(F64).to(DEV)
    h, dpre = ri(-2, 2, B, F, H), ri(-2, 2, B, F, H)
    wf, wb, bias = ri(-1, 1, H, K, cg), ri(-1, 1, G, cg, K, cg), ri(-3, 3, H)
    ws = hip.debug_posconv_workspace(B, F, H, G, K, DEV)
    out, pre = _guarded(B, F, H), _guarded(B, F, H)
    hip.debug_posconv_direct(_bf(h).view(B * F, H), _bf(wf), _f32(bias), out, pre, B, F, G, K, gelu=False, workspace=ws)
    torch.cuda.synchronize()
    ref, _ = P.forward(h, P.from_wf(wf), bias)
    assert float(ref.abs().max()) < 2 ** 24
    want = _bf(ref)
    got_pre, got_out = _written_and_guarded("pre", pre, B, F), _written_and_guarded("out", out, B, F)
    assert torch.equal(got_pre, want), f"pre: {int((got_pre != want).sum())} of {want.numel()} differ from bf16(float64 result)"
    assert torch.equal(got_out, want), f"out: {int((got_out != want).sum())} of {want.numel()} differ from bf16(float64 result)"
    out = _guarded(B, F, H)  # the epilogue without bias and without the saved pre-activation
    hip.debug_posconv_direct(_bf(h).view(B * F, H), _bf(wf), None, out, None, B, F, G, K, gelu=False, workspace=ws)
    torch.cuda.synchronize()
    want, got = _bf(ref - bias), _written_and_guarded("out", out, B, F)
    assert torch.equal(got, want), f"out (no bias): {int((got != want).sum())} of {want.numel()} differ from bf16(float64 result)"
    dx = _guarded(B, F, H)
    hip.debug_posconv_direct(_bf(dpre).view(B * F, H), _bf(wb), None, dx, None, B, F, G, K, row0=1, gelu=False, workspace=ws)
    torch.cuda.synchronize()
    want = _bf(P.grad_input(dpre, P.from_wb(wb)))
    got = _written_and_guarded("dX", dx, B, F)
    assert torch.equal(got, want), f"dX: {int((got != want).sum())} of {want.numel()} differ from bf16(float64 result)"


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad_shapes(K):
    return [(1, 512 + r - K) for r in (0, 1, 127, 128, 129, 511)] + [(1, 1), (2, 499), (4, 1500), (32, 499)]


def _wgrad_cases():
    for H, G in GEOMS:
        for K in TAPS:
            for B, F in _wgrad_shapes(K):
                for kind in ("integer", "real"):
                    yield pytest.param(H, G, K, B, F, kind, id=f"H{H}-K{K}-B{B}-F{F}-{kind}")


def _run_wgrad(h, dpre, B, F, H, G, K):
    """Two launches, each from a NaN dwf and a NaN workspace (packed buffers and the four partials); returns both."""
    hip = _hip()
    cg = H // G
    h16, d16 = _bf(h).view(B * F, H), _bf(dpre).view(B * F, H)
    outs = []
    for _ in range(2):
        dwf = torch.full((G, K * cg, cg), float("nan"), dtype=F32, device=DEV)
        hip.debug_posconv_wgrad(h16, d16, dwf, B, F, G, K, workspace=hip.debug_posconv_workspace(B, F, H, G, K, DEV))
        torch.cuda.synchronize()
        outs.append(dwf)
    return outs


@pytest.mark.parametrize("H,G,K,B,F,kind", list(_wgrad_cases()))
def test_wgrad(H, G, K, B, F, kind):
    """posconv_wgrad_kernel + posconv_wgrad_sum_kernel at row counts around the 128-row stage and the four row ranges."""
    assert B * (F + K) * 4 < 2 ** 24
    if kind == "integer":
        gen = torch.Generator().manual_seed(5 * H + K + 100 * B + F)
        h, dpre = (torch.randint(-2, 3, (B, F, H), generator=gen).to(F64).to(DEV) for _ in range(2))
    else:
        act = P.wgrad_activations(B, F, H, K)
        h, dpre = act["h"].to(DEV), act["dpre"].to(DEV)
    a, b = _run_wgrad(h, dpre, B, F, H, G, K)
    assert not torch.isnan(a).any(), f"{int(torch.isnan(a).sum())} elements of dwf are NaN (unwritten, or an empty row range left its partial)"
    ref = P.grad_weight(h, dpre, K, G)
    if kind == "integer":
        assert torch.equal(a.to(F64), ref), f"{int((a.to(F64) != ref).sum())} of {ref.numel()} differ from the float64 result"
    else:
        _check("dwf", a, ref, P.C_WGRAD * U * P.grad_weight_abs_sum(h, dpre, K, G))
    assert torch.equal(a, b), "two launches differ"


# ------------------------------------------------------------------------------------------------ prepare / weight-norm backward
def _edge_weights(H, G, K):
    """g, v of the geometry with one tap of g = 0 and one tap whose ||v_k|| is ~1e-6 of the others'."""
    wt = _weights(H, G, K)
    g, v = wt["g"].clone(), wt["v"].clone()
    g[3] = 0.0
    v[:, :, 5] = (v[:, :, 5] * 1e-6).to(F32).to(F64)
    return g, v


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("K", TAPS)
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_prepare(H, G, K, dt):
    """k_posconv_prepare_t: tap norms, and g v / ||v|| at every index of the forward and the flipped layout."""
    hip = _hip()
    g, v = _edge_weights(H, G, K)
    wf, wb, norms = hip.debug_posconv_prepare(_f32(g), _f32(v), G, dt)
    torch.cuda.synchronize()
    nsq = P.tap_norms(v) ** 2
    _check("norms", norms[:K], nsq, 1e-5 * nsq)
    w = P.weight(g, v)
    if dt == BF:
        bar = torch.tensor(RR.bf16_ulp(w.cpu().numpy()), device=DEV)
    else:
        bar = 1e-5 * w.abs()
    _check("wf", wf, P.to_wf(w), P.to_wf(bar))
    _check("wb", wb, P.to_wb(w), P.to_wb(bar))
    assert (wf[:, 3, :] == 0).all() and (wb[:, :, K - 1 - 3, :] == 0).all(), "the tap with g = 0 is not exactly 0"


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("K", TAPS)
@pytest.mark.parametrize("source", ["random", "wgrad"])
def test_weight_bwd(H, G, K, source):
    """k_posconv_weight_bwd accumulates dg, dv onto non-zero starting values; dwf random, or what the weight gradient kernel wrote."""
    hip = _hip()
    cg = H // G
    g, v = _edge_weights(H, G, K)
    g32, v32 = _f32(g), _f32(v)
    _, _, norms = hip.debug_posconv_prepare(g32, v32, G, BF)
    gen = torch.Generator().manual_seed(H + K)
    if source == "random":
        dwf = torch.randn(G, K * cg, cg, generator=gen, dtype=F32).to(DEV)
    else:
        act = P.wgrad_activations(2, 499, H, K)
        dwf = _run_wgrad(act["h"].to(DEV), act["dpre"].to(DEV), 2, 499, H, G, K)[0]
    dg0, dv0 = torch.randn(K, generator=gen, dtype=F32).to(DEV), torch.randn(H, cg, K, generator=gen, dtype=F32).to(DEV)
    dg, dv = dg0.clone(), dv0.clone()
    hip.debug_posconv_weight_bwd(dwf, g32, v32, norms, dg, dv, G)
    torch.cuda.synchronize()
    ref = P.weight_norm_bwd(P.dwf_to_w(dwf.to(F64), K), g, v)
    assert torch.isfinite(dg).all() and torch.isfinite(dv).all()
    _check("dg", dg.to(F64) - dg0.to(F64), ref["dg"], 1e-5 * ref["terms_dg"] + 2.0 ** -23 * (dg0.to(F64).abs() + ref["dg"].abs()))
    _check("dv", dv.to(F64) - dv0.to(F64), ref["dv"], 1e-5 * ref["terms_dv"] + 2.0 ** -23 * (dv0.to(F64).abs() + ref["dv"].abs()))


# ------------------------------------------------------------------------------------------------ pack
@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("K", TAPS)
@pytest.mark.parametrize("B,F", [(1, 1), (2, 499), (3, 513)])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_pack(H, G, K, B, F, dt):
    """posconv_pack_kernel: the packed [G][rows][cg] layout with its K / 2 leading, K separating and K trailing zero rows."""
    hip = _hip()
    gen = torch.Generator().manual_seed(B + F)
    h = (torch.randn(B, F, H, generator=gen) + 3.0).to(dt).to(DEV)  # (no zeros: a gap row that took a frame shows)
    pg = hip.debug_posconv_pack(h.view(B * F, H), B, F, G, K)
    torch.cuda.synchronize()
    want = P.pack(h, K, G)
    assert pg.shape == want.shape
    assert not torch.isnan(pg).any(), "rows of the packed buffer were not written"
    assert torch.equal(pg, want), f"{int((pg != want).sum())} elements differ from the reference layout"
