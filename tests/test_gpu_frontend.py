"""GPU: the kernels that run only when the feature encoder trains (conv_frontend.hip) and the data movers of the Whisper front end
(whisper_frontend.hip), one launch function at a time, against the float64 restatement tests/frontend_ref.py (itself pinned to torch
under float64 autograd by tests/test_frontend_ref.py), through the test-only entries ssak_debug_conv0_bwd / _conv0_wgrad /
_conv0_bias / _col2im / _sum_slabs / _conv_weight_rearrange / _conv_wgrad_unrearrange / _col2im_k3s2 / _mel_to_cl / _add_rowvec /
_copy_rows_padded.  The references are fed exactly the values the kernels read (inputs already rounded to the storage type).

Which kernel each test reaches (every templated kernel as <bf16> and <float>):

* conv0_bwd_kernel<0, T>, conv0_bwd_gsums_kernel, conv0_bwd_affine_kernel, conv0_bwd_kernel<1, T>, conv0_bwd_dw_kernel
  (k_conv0_gn_gelu_bwd_t<T>): test_conv0_bwd, (C, T0, r, B) of frontend_ref.CONV0_BWD_SHAPES x both types: C = 512 (nq = 128,
  fl = 2) with T0 in {1, 2, 129, 1023, 1024, 1025, 2049} (one frame; fewer frames than lanes; around one 1024-frame workgroup;
  three workgroups with a one-frame tail), C = 64 (16, 16), 1024 (256, 1) and 8 (2, 128) at three T0 each; T = 5 (T0 - 1) + 10 + r,
  r in {0, 4}; B in {1, 3}.  Statistics from the float64 reference; test_conv0_bwd_with_the_forwards_statistics takes them from
  ssak_conv0_gn_gelu's workspace (C = 512, T0 = 1025, B = 3: conv0_moments_kernel + conv0_channel_stats_kernel feed the backward).
* conv0_wgrad_kernel<T> + conv0_wgrad_sum_kernel: test_conv0_wgrad, frontend_ref.CONV0_WGRAD_SHAPES: C in {512, 64, 2}, T0 in
  {1, 31, 33, 1599, 2048, 2049} (empty workgroups; 1 and 2 frames per workgroup; the tiny model's length; exactly one 64-frame chunk
  per workgroup; a chunk plus one frame), (k, s) = (10, 5) and one (4, 3), B in {1, 3}; integer and real data.
* conv0_bias_kernel<T>: test_conv0_bias, C in {512, 64} x T0 in {1, 127, 128, 129, 400} (around the 128-frame workgroup), with a
  bias and with the null pointer the engine passes for a bias-free model; integer and real data.
* col2im_kernel<T>: test_col2im, (k, s, C) in {(3, 2, 512), (2, 2, 512), (3, 2, 8), (10, 5, 32)} x Tout in {1, 2, 199} x
  Tin = (Tout - 1) s + k + r, r in {0, 1} x B in {1, 3}; test_col2im_grid_stride: B = 9, Tin = 4001, C = 512 (2 304 576 chunks of
  8 > 8192 x 256 threads: the grid-stride loop runs a second time).
* sum_slabs_kernel, conv_w_rearrange_kernel<T>, conv_wgrad_unrearrange_kernel: test_slabs_and_layouts, (Co, Ci, k) in
  {(512, 512, 3), (512, 512, 2), (8, 8, 3), (5, 7, 2)} x nb in {1, 3, 32}; test_sum_slabs_grid_stride: n = 4096 x 256 + 7.
* col2im_k3s2_kernel<T>: test_col2im_k3s2, H in {384, 8} x Tin in {2, 3, 100, 101} x B in {1, 3}; F = (Tin + 1) / 2 and
  RS1 = 2 align4(F + 1) as the engine sizes them, pre with its one-row lead in a [B RS1, H] buffer that is NaN elsewhere.
* mel_to_cl_kernel<T>: test_mel_to_cl, C in {80, 32, 33} x T in {1, 31, 32, 33, 100} x lead in {0, 1} x B in {1, 3}.
* add_rowvec_kernel<T>, copy_rows_padded_kernel<T>: test_add_rowvec_and_copy_rows, H in {384, 8} x F in {1, 50} x RS in {F, F + 3}
  x B in {1, 3}; test_row_movers_grid_stride: B = 440, F = 50, H = 384 (1 056 000 chunks > 4096 x 256).

Data.  Integer cases: small integers for x, d, w, bias, dxcol and the slabs, so that every partial sum is an integer below 2^24
and fp32 accumulation is exact in any order.  Real cases (frontend_ref.*_case): x ~ N(0, 1), w ~ 0.3 N(0, 1), gamma = 1 + 0.1 N,
beta = 0.1 N, dy / d / dxcol ~ N(0, 1) rounded to the storage type; with B >= 2 the first and last 64 frames or samples of each
utterance are 8 times larger, so a read across an utterance boundary moves results by many bars.  Fixed seeds.

Bars (u = 2^-24).  No element is excluded from any comparison.

* Movers: mel_to_cl, copy_rows_padded, rearrange (the bf16 / fp32 rounding of w), unrearrange and col2im on integer data: EQUAL
  to the reference.  add_rowvec, unrearrange and col2im on real data: at most two terms meet in every output of every case here
  (ceil(k / s) <= 2; asserted), so the fp32 sum of the rounded inputs is the float64 sum rounded once: EQUAL to the storage
  rounding of the float64 sum.
* sum_slabs: EQUAL to the fp32 left-to-right emulation (additions only, fixed order); on integers also to the float64 sum.
* conv0 weight gradient, conv0 + bias on integer data: EQUAL to the float64 result (+ start), or its bf16 rounding.
* Accumulated fp32 outputs:  |got - start - ref| <= C u sum |terms| + 2^-23 (|start| + |ref|) (+ the propagated term below), with
  sum |terms| the float64 reference's sum of the summands' magnitudes and C from the reference, not the kernels: 4 x the worst
  |fp32-order emulation - float64| / (u sum |terms|) over all real-valued cases of this module, rounded up to a power of two
  (frontend_ref.py; re-measured by test_frontend_ref.py::test_accumulation_constants):
      xh of the conv0 backward  3.7480 -> C_XHAT = 16      sum g, sum g xh  9.8111 -> C_GSUM = 64
      dw of the conv0 backward  7.4204 -> C_DW = 32        conv0 weight gradient  3.3346 -> C_WGRAD = 16
      conv0 + bias              3.7239 -> C_BIAS = 16
* conv0 backward's propagated term (frontend_ref.conv0_bwd_bars), per element with S = sum_k |w_k x_k| and E = the gelu' bar of
  test_gpu_rowwise.py (1.65e-5 + 2^-20 for the bf16 fit, 1e-6 for fp32):
      d_xh = C_XHAT u (S + |mean|) rstd + 2 u |xh|;   d_z = |gamma| d_xh + u (|gamma xh| + |z|);   d_g = |dy| (0.7979 d_z + E) + u |g|
      dbeta:  C_GSUM u sum |g| + sum d_g;     dgamma:  C_GSUM u sum |g xh| + sum (d_g |xh| + |g| d_xh)
      d_m1 = (C_GSUM u sum_t |g| + sum_t d_g) / T0 + u |m1|, d_m2 likewise;
      d_dv = |gamma| rstd (d_g + d_m1 + |xh| d_m2 + d_xh |m2|) + 4 u |gamma| rstd (|g| + |m1| + |xh m2|)
      dw:  C_DW u sum |dv x_k| + sum d_dv |x_k|
* conv0 + bias, real data: |got - ref| <= e |ref| + C_BIAS u (|bias| + S), e = 2^-8 for bf16 and 0 for fp32 storage.
* col2im_k3s2: |got - ref| <= e |ref| + 4 u sum |dxcol| |gelu'(pre)| + |sum dxcol| E, e = 2^-8 (bf16) or u (fp32); 4 u: one
  addition and one product in fp32, with a factor of two.  Rows >= Tin of every utterance are exactly zero.
* Destinations start as NaN (col2im, col2im_k3s2, sum_slabs, add_rowvec, copy_rows_padded, rearrange) or as a sentinel where
  the kernel must not write (mel_to_cl outside [lead, lead + T), the rows behind conv0 + bias); the scratch of the conv0
  backward and of the weight gradient starts as 0xFF bytes; dw, dgamma, dbeta start from N(0, 1) values; two launches of every
  conv0 backward / weight gradient case are bit-identical.

Worst err / bar on the MI355X: NOT RECORDED.  This module has not yet run on an MI355X, so there are no measured figures
to give; every bar above is derived from the reference alone.  _check prints "max err / bar" for each bar-checked comparison
(pytest -s): whoever runs the module first on the GPU should copy the per-kernel maxima here.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frontend_ref as F  # noqa: E402
import rowwise_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = F.U
SENTINEL = -7.0
NAN = float("nan")
DTYPES = pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])


def _hip():
    import ssak_amd.hip as hip
    return hip


def _dev(a, dt):
    """float64 values -> a contiguous device tensor of type dt (exact for values of that type)."""
    return torch.tensor(np.ascontiguousarray(a), dtype=F64).to(dt).to(DEV).contiguous()


def _host(t):
    return t.detach().to(F64).cpu().numpy()


def _sync():
    torch.cuda.synchronize()


def _check(name, got, ref, bar):
    assert got.shape == ref.shape, name
    err = np.abs(got - ref)
    bad = ~(err <= bar)  # (a NaN is bad)
    if bad.any():
        k = int(np.argmax(np.where(bad, np.nan_to_num(err - bar, nan=np.inf), -1.0)))
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.size} outside the bar; worst at flat index {k} of shape {err.shape}: "
                             f"got {got.flat[k]!r} ref {ref.flat[k]!r} bar {bar.flat[k]!r}")
    print(f"{name}: max err / bar = {float(np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0).max()):.3f}")


def _equal(name, got, want):
    assert got.shape == want.shape, name
    same = (got == want)
    assert same.all(), f"{name}: {int((~same).sum())} of {want.size} differ (NaN counts); first at flat index {int(np.argmin(same))}"


def _store(a, bf16):
    return RR.round_to(a, bf16)


# ------------------------------------------------------------------------------------------------ conv0 backward
def _run_conv0_bwd(c, bf16, sums, starts):
    """Two launches, each from the same starting values and a 0xFF scratch; returns (dw, dgamma, dbeta) - start as float64."""
    hip = _hip()
    dt = BF if bf16 else F32
    x, w, gamma, beta = (_dev(c[k], F32) for k in ("x", "w", "gamma", "beta"))
    dy = _dev(c["dy"], dt)
    B, T = c["x"].shape
    C = c["w"].shape[0]
    runs = []
    for _ in range(2):
        outs = [_dev(s, F32) for s in starts]
        ws = hip.debug_conv0_bwd_workspace(B, T, C, DEV)
        hip.debug_conv0_bwd(x, w, gamma, beta, dy, sums, *outs, workspace=ws)
        _sync()
        runs.append(outs)
    for a, b, name in zip(runs[0], runs[1], ("dw", "dgamma", "dbeta")):
        assert torch.equal(a, b), f"{name}: two launches differ"
    return [_host(o) - s for o, s in zip(runs[0], starts)]


def _check_conv0_bwd(p, got, starts, bf16, tag):
    bars = F.conv0_bwd_bars(p, bf16)
    for name, g, s in zip(("dw", "dgamma", "dbeta"), got, starts):
        assert np.isfinite(g).all(), f"{name}: not finite"
        _check(f"conv0_bwd {name} {tag}", g, p[name], bars[name] + 2.0 ** -23 * (np.abs(s) + np.abs(p[name])))


@pytest.mark.parametrize("C,T0,r,B", F.CONV0_BWD_SHAPES, ids=lambda v: str(v))
@DTYPES
def test_conv0_bwd(C, T0, r, B, bf16):
    """k_conv0_gn_gelu_bwd_t on the float64 reference's statistics: dw, dgamma, dbeta accumulated onto non-zero values."""
    c = F.conv0_bwd_case(C, T0, r, B, bf16)
    p = F.conv0_bwd(c["x"], c["w"], c["gamma"], c["beta"], c["dy"], bf16)
    sums = torch.tensor(np.stack([p["mean"], p["rstd"]], axis=-1), dtype=F64).to(DEV).contiguous()
    starts = F.start_values(C, (C, 10), (C,), (C,))
    got = _run_conv0_bwd(c, bf16, sums, starts)
    _check_conv0_bwd(p, got, starts, bf16, "bf16" if bf16 else "fp32")


@DTYPES
def test_conv0_bwd_with_the_forwards_statistics(bf16):
    """The statistics as ssak_conv0_gn_gelu leaves them at the start of its workspace ([B][C] (mean, rstd) doubles): the two
    halves fit together.  The reference is given the same statistics, after they are held to its own."""
    hip = _hip()
    C, T0, r, B = 512, 1025, 4, 3
    c = F.conv0_bwd_case(C, T0, r, B, bf16)
    T = c["x"].shape[1]
    nb = hip.lib.ssak_conv0_workspace_bytes(B, T, C)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.empty((B, T0, C), dtype=BF, device=DEV)
    x, w, gamma, beta = (_dev(c[k], F32) for k in ("x", "w", "gamma", "beta"))
    hip.check(hip.lib.ssak_conv0_gn_gelu(hip.ptr(x), hip.ptr(w), hip.ptr(gamma), hip.ptr(beta), hip.ptr(out), hip.ptr(ws), nb, B, T, C,
                                         hip.stream()))
    _sync()
    sums = ws[:B * C * 16].view(F64).view(B, C, 2).clone()
    st = sums.cpu().numpy()
    own = F.conv0_bwd(c["x"], c["w"], c["gamma"], c["beta"], c["dy"], bf16)
    # (fp64 moments of the input: var = E y^2 - mean^2 loses ~2^-52 (mean^2 + var) / var, far below 1e-9 here)
    assert np.allclose(st[..., 0], own["mean"], rtol=1e-9, atol=1e-12) and np.allclose(st[..., 1], own["rstd"], rtol=1e-9, atol=0)
    p = F.conv0_bwd(c["x"], c["w"], c["gamma"], c["beta"], c["dy"], bf16, stats=(st[..., 0], st[..., 1]))
    starts = F.start_values(C, (C, 10), (C,), (C,))
    got = _run_conv0_bwd(c, bf16, sums, starts)
    _check_conv0_bwd(p, got, starts, bf16, ("bf16" if bf16 else "fp32") + ", forward's statistics")


# ------------------------------------------------------------------------------------------------ conv0 weight gradient
@pytest.mark.parametrize("C,T0,B,k,s", F.CONV0_WGRAD_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["integer", "real"])
@DTYPES
def test_conv0_wgrad(C, T0, B, k, s, kind, bf16):
    hip = _hip()
    c = F.conv0_wgrad_case(C, T0, B, k, s, bf16, kind == "integer")
    (start,) = F.start_values(C + k, (C, k))
    if kind == "integer":
        start = np.round(4 * start)
    d, x = _dev(c["d"], BF if bf16 else F32), _dev(c["x"], F32)
    runs = []
    for _ in range(2):
        dw = _dev(start, F32)
        hip.debug_conv0_wgrad(d, x, dw, s)
        _sync()
        runs.append(dw)
    assert torch.equal(runs[0], runs[1]), "two launches differ"
    ref = F.conv0_wgrad(c["d"], c["x"], k, s)
    if kind == "integer":
        assert np.abs(ref).max() + 16 < 2 ** 24
        _equal("conv0_wgrad (integer)", _host(runs[0]), ref + start)
    else:
        _check("conv0_wgrad " + ("bf16" if bf16 else "fp32"), _host(runs[0]) - start, ref,
               F.C_WGRAD * U * F.conv0_wgrad_abs_sum(c["d"], c["x"], k, s) + 2.0 ** -23 * (np.abs(start) + np.abs(ref)))


# ------------------------------------------------------------------------------------------------ conv0 + bias
GUARD = 64


@pytest.mark.parametrize("C,T0,B", F.CONV0_BIAS_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["integer", "real"])
@DTYPES
def test_conv0_bias(C, T0, B, kind, bf16):
    hip = _hip()
    dt = BF if bf16 else F32
    c = F.conv0_bias_case(C, T0, B, kind == "integer")
    x, w = _dev(c["x"], F32), _dev(c["w"], F32)
    for bias in (c["bias"], None):
        out = torch.full((B * T0 + GUARD, C), SENTINEL, dtype=dt, device=DEV)
        out[:B * T0] = NAN
        hip.debug_conv0_bias(x, w, None if bias is None else _dev(bias, F32), out)
        _sync()
        assert (out[B * T0:] == SENTINEL).all(), "rows behind the output were written"
        got = _host(out[:B * T0]).reshape(B, T0, C)
        ref = F.conv0(c["x"], c["w"], bias)
        if kind == "integer":
            _equal("conv0_bias (integer)", got, _store(ref, bf16))
        else:
            _check("conv0_bias " + ("bf16" if bf16 else "fp32") + ("" if bias is not None else " (no bias)"), got, ref,
                   (2.0 ** -8 if bf16 else 0.0) * np.abs(ref) + F.C_BIAS * U * F.conv0_abs_sum(c["x"], c["w"], bias))


# ------------------------------------------------------------------------------------------------ col2im
@pytest.mark.parametrize("k,s,C", [(3, 2, 512), (2, 2, 512), (3, 2, 8), (10, 5, 32)])
@pytest.mark.parametrize("Tout", [1, 2, 199])
@DTYPES
def test_col2im(k, s, C, Tout, bf16):
    hip = _hip()
    dt = BF if bf16 else F32
    assert -(-k // s) <= 2  # at most two windows meet in a row: the fp32 sum is the float64 sum rounded once
    for r in (0, 1):
        for B in (1, 3):
            for integer in (True, False):
                Tin = (Tout - 1) * s + k + r
                d = F.col2im_case(k, s, C, Tout, r, B, bf16, integer)
                dx = torch.full((B, Tin, C), NAN, dtype=dt, device=DEV)
                hip.debug_col2im(_dev(d, dt), dx, k, s)
                _sync()
                _equal(f"col2im r={r} B={B} integer={integer}", _host(dx), _store(F.col2im(d, Tin, s), bf16))


def test_col2im_grid_stride():
    """B Tin C / 8 = 2 304 576 chunks > 8192 x 256 threads: the loop runs a second time.  Integer data, the reference on the device."""
    hip = _hip()
    B, Tin, C, k, s = 9, 4001, 512, 3, 2
    Tout = (Tin - k) // s + 1
    assert B * Tin * C // 8 > 8192 * 256 and (Tout - 1) * s + k == Tin
    gen = torch.Generator(device=DEV).manual_seed(11)
    d = torch.randint(-3, 4, (B, Tout, k, C), generator=gen, device=DEV).to(BF)
    dx = torch.full((B, Tin, C), NAN, dtype=BF, device=DEV)
    hip.debug_col2im(d, dx, k, s)
    _sync()
    ref = torch.zeros((B, Tin, C), dtype=F32, device=DEV)
    for kk in range(k):
        ref[:, kk:kk + (Tout - 1) * s + 1:s] += d[:, :, kk].to(F32)
    assert torch.equal(dx.to(F32), ref), f"{int((dx.to(F32) != ref).sum())} elements differ"


# ------------------------------------------------------------------------------------------------ slabs and weight layouts
@pytest.mark.parametrize("Co,Ci,k", [(512, 512, 3), (512, 512, 2), (8, 8, 3), (5, 7, 2)])
def test_slabs_and_layouts(Co, Ci, k):
    hip = _hip()
    n = Co * Ci * k
    for nb in (1, 3, 32):
        for integer in (True, False):
            sl = F.slabs_case(nb, n, integer)
            out = torch.full((n,), NAN, dtype=F32, device=DEV)
            hip.debug_sum_slabs(_dev(sl, F32), out)
            _sync()
            _equal(f"sum_slabs nb={nb}", _host(out), F.emulate_sum_slabs(sl).astype(np.float64))
            if integer:
                _equal(f"sum_slabs nb={nb} (integer)", _host(out), F.sum_slabs(sl))
    rng = np.random.default_rng(Co + Ci + k)
    w = rng.standard_normal((Co, Ci, k)).astype(np.float32).astype(np.float64)
    for bf16 in (True, False):
        out = torch.full((Co, k, Ci), NAN, dtype=BF if bf16 else F32, device=DEV)
        hip.debug_conv_weight_rearrange(_dev(w, F32), out)
        _sync()
        _equal("rearrange", _host(out), _store(F.weight_rearrange(w), bf16))
    for integer in (True, False):
        if integer:
            dwr, g0 = rng.integers(-1000, 1001, (Co, k, Ci)).astype(np.float64), rng.integers(-1000, 1001, (Co, Ci, k)).astype(np.float64)
        else:
            dwr, g0 = (rng.standard_normal(sh).astype(np.float32).astype(np.float64) for sh in ((Co, k, Ci), (Co, Ci, k)))
        g = _dev(g0, F32)
        hip.debug_conv_wgrad_unrearrange(_dev(dwr, F32), g)
        _sync()
        _equal("unrearrange", _host(g), RR.round_f32(F.wgrad_unrearrange(dwr, g0)))


def test_sum_slabs_grid_stride():
    hip = _hip()
    n = 4096 * 256 + 7
    sl = F.slabs_case(3, n, False)
    out = torch.full((n,), NAN, dtype=F32, device=DEV)
    hip.debug_sum_slabs(_dev(sl, F32), out)
    _sync()
    _equal("sum_slabs", _host(out), F.emulate_sum_slabs(sl).astype(np.float64))


# ------------------------------------------------------------------------------------------------ col2im_k3s2
@pytest.mark.parametrize("H", [384, 8])
@pytest.mark.parametrize("Tin", [2, 3, 100, 101])
@pytest.mark.parametrize("B", [1, 3])
@DTYPES
def test_col2im_k3s2(H, Tin, B, bf16):
    hip = _hip()
    dt = BF if bf16 else F32
    Fr = (Tin + 1) // 2
    RS1 = 2 * ((Fr + 1 + 3) // 4 * 4)  # the engine: RS2 = align_up(F + 1, 4), RS1 = 2 RS2
    assert RS1 >= Tin + 2
    dxcol, pre = F.col2im_k3s2_case(H, Tin, B, bf16)
    out = torch.full((B, RS1, H), NAN, dtype=dt, device=DEV)
    hip.debug_col2im_k3s2(_dev(dxcol, dt), _dev(F.pre_with_lead(pre, RS1, NAN), dt), out, Tin)
    _sync()
    got = _host(out)
    ref, acc, aacc, gp = F.col2im_k3s2(dxcol, pre, Tin, RS1, bf16)
    assert (got[:, Tin:] == 0).all(), "rows >= Tin are not zero"
    bar = (2.0 ** -8 if bf16 else U) * np.abs(ref[:, :Tin]) + 4 * U * aacc * np.abs(gp) + np.abs(acc) * F.gelu_grad_bar(bf16)
    _check("col2im_k3s2 " + ("bf16" if bf16 else "fp32"), got[:, :Tin], ref[:, :Tin], bar)


# ------------------------------------------------------------------------------------------------ movers
@pytest.mark.parametrize("C", [80, 32, 33])
@pytest.mark.parametrize("T", [1, 31, 32, 33, 100])
@DTYPES
def test_mel_to_cl(C, T, bf16):
    hip = _hip()
    dt = BF if bf16 else F32
    for lead in (0, 1):
        for B in (1, 3):
            RS = T + lead + 3
            mel = np.random.default_rng(C + T + lead + B).standard_normal((B, C, T)).astype(np.float32).astype(np.float64)
            cl = torch.full((B * RS + 8, C), SENTINEL, dtype=dt, device=DEV)
            hip.debug_mel_to_cl(_dev(mel, F32), cl, RS, lead)
            _sync()
            _equal(f"mel_to_cl lead={lead} B={B}", _host(cl), F.mel_to_cl(_store(mel, bf16), np.full((B * RS + 8, C), SENTINEL), RS, lead))


@pytest.mark.parametrize("H", [384, 8])
@pytest.mark.parametrize("Fr", [1, 50])
@DTYPES
def test_add_rowvec_and_copy_rows(H, Fr, bf16):
    hip = _hip()
    dt = BF if bf16 else F32
    for B in (1, 3):
        rng = np.random.default_rng(H + Fr + B)
        x, pos = (_store(rng.standard_normal(sh), bf16) for sh in ((B, Fr, H), (Fr, H)))
        out = torch.full((B, Fr, H), NAN, dtype=dt, device=DEV)
        hip.debug_add_rowvec(_dev(x, dt), _dev(pos, dt), out)
        _sync()
        _equal(f"add_rowvec B={B}", _host(out), _store(F.add_rowvec(x, pos), bf16))
        for RS in (Fr, Fr + 3):
            dst = torch.full((B, RS, H), NAN, dtype=dt, device=DEV)
            hip.debug_copy_rows_padded(_dev(x, dt), dst)
            _sync()
            _equal(f"copy_rows_padded B={B} RS={RS}", _host(dst), F.copy_rows_padded(x, RS))


def test_row_movers_grid_stride():
    """B F H / 8 = 1 056 000 chunks > 4096 x 256 threads.  The reference on the device (two bf16 terms: fp32 sum rounded once)."""
    hip = _hip()
    B, Fr, H = 440, 50, 384
    assert B * Fr * H // 8 > 4096 * 256
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((B, Fr, H), generator=gen, device=DEV).to(BF)
    pos = torch.randn((Fr, H), generator=gen, device=DEV).to(BF)
    out = torch.full((B, Fr, H), NAN, dtype=BF, device=DEV)
    hip.debug_add_rowvec(x, pos, out)
    dst = torch.full((B, Fr + 1, H), NAN, dtype=BF, device=DEV)
    hip.debug_copy_rows_padded(x, dst)
    _sync()
    assert torch.equal(out, (x.to(F64) + pos.to(F64)[None]).to(BF))
    assert torch.equal(dst[:, :Fr], x) and (dst[:, Fr:] == 0).all()
