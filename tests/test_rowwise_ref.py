"""CPU: the float64 restatement tests/rowwise_ref.py that tests/test_gpu_rowwise.py holds the row kernels to is itself right.

* Its LayerNorm backward (post-dropout, post-GELU, g2, g_res before the sum-dropout replay, pre-dropout, column sums) and its
  softmax backward equal torch float64 autograd of the same forward composition with the same fixed masks.
* Its lists of the dispatchers' specialised instantiations are exactly the LN_FWD_SPEC(..) / LN_BWD_SPEC(..) lists of
  norm_act.hip: a specialisation added without a test fails here.  Its GELU fit constants are common.h's, and the fit meets its
  stated error in exact arithmetic.
* The test-only C entries reject bad shapes before any launch.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rowwise_ref as RR  # noqa: E402

ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "ssak_amd", "csrc")


def _site_t(seed, site, shape):
    keep, sc = RR.site_mask(seed, site, shape)
    return None if keep is None else torch.tensor(keep.astype(np.float64) * sc)


# (pre, mid, post, g2, g_res, post_gelu): every operand of the composition, alone and together
LN_CASES = [
    (0.0, 0.0, 0.0, False, False, False),
    (0.1, 0.0, 0.0, True, False, False),
    (0.0, 0.0, 0.5, True, False, False),
    (0.0, 0.1, 0.0, False, True, False),
    (0.1, 0.5, 0.0, True, True, False),
    (0.5, 0.1, 0.1, True, True, False),
    (0.0, 0.0, 0.0, False, False, True),
    (0.0, 0.0, 0.1, True, False, True),
    (0.1, 0.1, 0.5, True, True, True),
]


@pytest.mark.parametrize("pre,mid,post,g2,gres,pgelu", LN_CASES)
def test_ln_reference_matches_float64_autograd(pre, mid, post, g2, gres, pgelu):
    """r = mid(res + pre(y)), out = post(gelu?(LN(r))), loss = <out, g1 + g2> + <r, g_res>: autograd's d/dres, d/dy, d/dgamma,
    d/dbeta and the column sums of d/dy == rowwise_ref.ln_bwd (fed with the forward's own r / mean / rstd) to 1e-12."""
    rng = np.random.default_rng(hash((pre, mid, post, g2, gres, pgelu)) % 2**32)
    M, C, eps, seed = 37, 48, 1e-5, 0xC0FFEE1234
    sp, sm, sq = (101, pre), (102, mid), (103, post)
    y, res = rng.standard_normal((M, C)), rng.standard_normal((M, C)) * 2 + 0.5
    gamma, beta = 1 + 0.3 * rng.standard_normal(C), 0.2 * rng.standard_normal(C)
    g1 = rng.standard_normal((M, C))
    G2 = rng.standard_normal((M, C)) if g2 else None
    GR = rng.standard_normal((M, C)) if gres else None
    ty, tres, tg, tb = (torch.tensor(v, requires_grad=True) for v in (y, res, gamma, beta))
    s = ty * _site_t(seed, sp, (M, C)) if pre else ty
    s = s + tres
    r = s * _site_t(seed, sm, (M, C)) if mid else s
    w = torch.nn.functional.layer_norm(r, (C,), tg, tb, eps)
    if pgelu:
        w = torch.nn.functional.gelu(w)
    out = w * _site_t(seed, sq, (M, C)) if post else w
    loss = (out * torch.tensor(g1 + (G2 if g2 else 0))).sum()
    if gres:
        loss = loss + (r * torch.tensor(GR)).sum()
    loss.backward()

    f = RR.ln_fwd(y, res, gamma, beta, eps=eps, seed=seed, pre=sp, mid=sm, post=sq, post_gelu=pgelu)
    assert np.allclose(f["r"], r.detach().numpy(), rtol=0, atol=1e-12)
    assert np.allclose(f["out"], out.detach().numpy(), rtol=0, atol=1e-12)
    b = RR.ln_bwd(g1, G2, f["r"], f["mean"], f["rstd"], gamma, GR, seed=seed, pre=sp, mid=sm, post=sq,
                  gelu_beta=beta if pgelu else None)
    for got, want in ((b["dr"], tres.grad), (b["dy"], ty.grad), (b["dgamma"], tg.grad), (b["dbeta"], tb.grad),
                      (b["dy_colsum"], ty.grad.sum(0))):
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # every position a site drops is exactly 0 where the kernels' bars say so
    for k, t in (("keep_mid", b["dr"]), ("keep_pre", b["dy"])):
        if b[k] is not None:
            assert (t[~b[k]] == 0).all()


def test_ln_reference_statistics_and_rounding():
    """Biased variance with eps inside the root; r_round applies before the statistics; bf16 rounding is round-to-nearest-even
    of the fp32 value (torch's cast); bf16_ulp is the bf16 spacing."""
    rng = np.random.default_rng(5)
    r = rng.standard_normal((9, 40)) * 3 + 1
    mean, rstd = RR.ln_stats(r, 1e-5)
    assert np.allclose(rstd, 1 / np.sqrt(r.var(axis=1, ddof=0) + 1e-5), rtol=1e-14)
    x = rng.standard_normal(100000) * np.exp2(rng.integers(-20, 20, 100000))
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).double().numpy()
    assert np.array_equal(RR.round_bf16(x), want)
    u = RR.bf16_ulp(x)
    assert (np.abs(want - x) <= 0.5 * u * (1 + 2.0**-15)).all()  # (+ the fp32 rounding before it)
    # one step of the bit pattern away from zero is one ulp
    nxt = torch.tensor(want, dtype=torch.bfloat16).view(torch.int16).add(1).view(torch.bfloat16).double().numpy()
    assert np.array_equal(np.abs(nxt - want), RR.bf16_ulp(want))
    f = RR.ln_fwd(r, None, np.ones(40), np.zeros(40), eps=1e-5, r_round=RR.round_bf16)
    assert np.array_equal(f["r"], RR.round_bf16(r))
    assert np.allclose(f["rstd"], RR.ln_stats(RR.round_bf16(r), 1e-5)[1], rtol=1e-14)


def test_softmax_reference_matches_float64_autograd():
    """Key mask per utterance (klens[row / rows_per_batch], 1, > cols, 0), pad columns, dropout: P / Pd == torch.softmax of the
    masked scores times the mask, dS == autograd of <Pd, dPd>; a row without any valid key is all 0 in P and dS."""
    rng = np.random.default_rng(11)
    nh, F, cols, ld, seed, site = 3, 5, 13, 24, 77, (9, 0.25)
    klens = np.array([13, 1, 40, 0])
    rows = len(klens) * nh * F
    S = rng.standard_normal((rows, ld)) * 4
    dPd = rng.standard_normal((rows, ld))
    f = RR.softmax_fwd(S, cols, klens, nh * F, seed=seed, site=site)
    kl = np.clip(klens, 0, cols)[np.arange(rows) // (nh * F)]
    valid = np.arange(ld)[None, :] < kl[:, None]
    tS = torch.tensor(S, requires_grad=True)
    P = torch.softmax(tS.masked_fill(torch.tensor(~valid), float("-inf")), dim=1)
    live = kl > 0
    P = torch.where(torch.tensor(live)[:, None], P, torch.zeros_like(P))
    Pd = P * _site_t(seed, site, (rows, ld))
    (Pd * torch.tensor(dPd)).sum().backward()
    assert np.allclose(f["P"], P.detach().numpy(), rtol=0, atol=1e-14)
    assert np.allclose(f["Pd"], Pd.detach().numpy(), rtol=0, atol=1e-14)
    assert np.allclose(f["P"][live].sum(1), 1.0) and (f["P"][~live] == 0).all() and (f["P"][~valid] == 0).all()
    b = RR.softmax_bwd(dPd, f["P"], cols, seed=seed, site=site)
    g = np.nan_to_num(tS.grad.numpy())
    assert np.abs(b["dS"] - g).max() < 1e-13
    assert (b["dS"][~live] == 0).all() and (b["dS"][:, cols:] == 0).all()


def test_gelu_reference_forms():
    """The fit constants are common.h's SSAK_PHI_C0..C3; in float64 the fit meets the error common.h states (so the device bar
    of tests/test_gpu_rowwise.py only adds fp32 rounding); gelu' forms are the derivatives of the gelu forms."""
    src = open(os.path.join(SRC, "common.h")).read()
    consts = tuple(float(re.search(rf"#define SSAK_PHI_C{i} \(([-0-9.e]+)f\)", src).group(1)) for i in range(4))
    assert consts == RR.PHI_C
    x = np.linspace(-12, 12, 960001)
    err = np.abs(RR.phi_fit(x) - RR.phi_exact(x))
    assert err.max() <= RR.PHI_FIT_MAX_ERR - 1e-7, err.max()
    h = 1e-6
    for g, dg in ((RR.gelu_exact, RR.gelu_grad_exact), (RR.gelu_fit, RR.gelu_grad_fit)):
        xs = x[np.abs(np.abs(x) - 6) > 1e-3][::97]
        num = (g(xs + h) - g(xs - h)) / (2 * h)
        # the fit's derivative keeps the exact density (common.h gelu_grad2): within the fit's error of the true derivative
        tol = 1e-7 if g is RR.gelu_exact else 1e-7 + RR.PHI_FIT_MAX_ERR * (1 + np.abs(xs) * 4)
        assert (np.abs(dg(xs) - num) <= tol).all()
    xt = torch.tensor(x)
    assert np.abs(RR.gelu_exact(x) - torch.nn.functional.gelu(xt).numpy()).max() < 1e-14


def _spec_list(name):
    src = open(os.path.join(SRC, "norm_act.hip")).read()
    src = re.sub(r"//[^\n]*", "", src)
    return [int(v) for v in re.findall(rf"\b{name}\((\d+)\)", src)]


def test_spec_lists_match_the_dispatchers():
    """norm_act.hip's LN_FWD_SPEC(..) / LN_BWD_SPEC(..) cases == the lists tests/test_gpu_rowwise.py enumerates, in both
    directions and without duplicates."""
    fwd, bwd = _spec_list("LN_FWD_SPEC"), _spec_list("LN_BWD_SPEC")
    assert len(fwd) == len(set(fwd)) and len(bwd) == len(set(bwd))
    assert sorted(fwd) == sorted(RR.LN_FWD_SPECS), (fwd, RR.LN_FWD_SPECS)
    assert sorted(bwd) == sorted(RR.LN_BWD_SPECS), (bwd, RR.LN_BWD_SPECS)


def test_debug_row_entries_reject_bad_shapes_before_any_launch():
    """SSAK_ERR_INVALID for C not a multiple of 8, C > 1536, M <= 0, ld > 1536, ld < cols, an unknown dtype and p outside
    [0, 1) -- decided on the host (every call here also lacks its operands, so nothing could launch)."""
    import ssak_amd.hip as h
    L = h.lib
    U = ctypes.c_uint64

    def fwd(M, C, dtype=0, p=0.0):
        return L.ssak_debug_layernorm_fwd(None, None, None, None, None, None, None, None, M, C, 1e-5, U(1), 0, p, 0, 0.0, 0, 0.0,
                                          0, dtype, None)

    def bwd(M, C, dtype=0):
        return L.ssak_debug_layernorm_bwd(None, None, None, None, None, None, None, None, None, None, None, None, None, M, C, U(1),
                                          0, 0.0, 0, 0.0, 0, 0.0, 0, dtype, None, 0, None)

    def last():
        return L.ssak_last_error().decode()

    for M, C in ((8, 12), (8, 1540), (8, 2048), (0, 768), (-3, 64)):
        assert fwd(M, C) == h.SSAK_ERR_INVALID and f"C={C}" in last()
        assert bwd(M, C) == h.SSAK_ERR_INVALID and f"C={C}" in last()
    assert fwd(8, 64, dtype=2) == h.SSAK_ERR_INVALID and "dtype" in last()
    assert bwd(8, 64, dtype=-1) == h.SSAK_ERR_INVALID and "dtype" in last()
    assert fwd(8, 64) == h.SSAK_ERR_INVALID and "neither" in last()
    assert bwd(8, 64) == h.SSAK_ERR_INVALID and "null" in last()
    for rows, cols, ld in ((4, 8, 1544), (4, 1600, 1600), (4, 16, 8), (4, 8, 12), (0, 8, 8), (4, 0, 8)):
        assert L.ssak_debug_softmax_fwd(None, None, None, None, rows, cols, ld, 1, U(0), 0, 0.0, 0, None) == h.SSAK_ERR_INVALID
        assert f"ld={ld}" in last()
        assert L.ssak_debug_softmax_bwd(None, None, None, rows, cols, ld, U(0), 0, 0.0, 1, None) == h.SSAK_ERR_INVALID
        assert f"ld={ld}" in last()
    assert L.ssak_debug_gelu(None, 16, None, None, 0, None) == h.SSAK_ERR_INVALID
    assert L.ssak_debug_layernorm_bwd_workspace_bytes(768) >= 3 * 768 * 4 * 768
