"""CPU: the float64 restatement tests/headopt_ref.py that tests/test_gpu_headopt.py holds sb_head.hip and optim.hip to is itself
right, and the bars of that test bite.

* Each function equals torch in float64 to 1e-12: F.layer_norm, F.batch_norm + F.leaky_relu (+ the fixed mask) forward and through
  autograd, torch.optim.AdamW and torch.optim.Adadelta behind clip_grad_norm_ (with a loss scale, which pins the clip convention).
* The launch-geometry arithmetic (lanes, workgroups, column blocks, loop trips) puts every GPU shape on the branch the GPU test's
  docstring names; the constants are read out of the kernel files, so a changed constant there makes the reader look here.
* On the inputs the GPU test uses, the reference stays inside the bars' preconditions (at most 1 % of a case's elements in the
  two-branch set, a handful inside the backward's sign window, clip cases on the intended side, the fp32 decay exact), the measured
  constants of the bars hold (fp32 re-evaluation with the kernel's summation shape, times 4), and each of these wrong
  restatements lands outside its bar at every shape where it differs from the right one: batch variance unbiased / running
  variance biased; eps outside the root; a missing 1 / (1 - p); the LeakyReLU slope on the wrong sign; dx without its
  mean(g xhat) term; a 0-based step in the bias correction; eps inside AdamW's root; weight decay coupled into AdamW's gradient
  (decoupled out of Adadelta's); Adadelta's delta from the updated acc_delta; the clip norm without grad_scale; a tail element
  left as it was; a row, a chunk of 8 columns, a float4 or a whole second loop trip left out of a sum.
"""
import math
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import headopt_ref as H  # noqa: E402

ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "ssak_amd", "csrc")
U = H.U


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


# ------------------------------------------------------------------------------------------------ pinned to torch float64
@pytest.mark.parametrize("B,n", [(3, 211), (1, 1), (2, 8)])
def test_utt_norm_matches_torch(B, n):
    rng = np.random.default_rng(n)
    x, dy = rng.standard_normal((B, n)) * 0.3 + 0.1, rng.standard_normal((B, n))
    y, mean, rstd = H.utt_norm_fwd(x, 1e-5)
    tx = _t(x, True)
    ty = F.layer_norm(tx, (n,), eps=1e-5)
    ty.backward(_t(dy))
    assert _rel(y, ty.detach().numpy()) < 1e-12 or n == 1
    tv, tm = torch.var_mean(tx.detach(), dim=1, unbiased=False)
    assert _rel(mean, tm.numpy()) < 1e-12 and _rel(rstd, torch.rsqrt(tv + 1e-5).numpy()) < 1e-12
    assert np.abs(H.utt_norm_bwd(dy, y, rstd) - tx.grad.numpy()).max() < 1e-12 * max(1.0, np.abs(tx.grad.numpy()).max())
    if n == 1:
        assert (y == 0).all() and rstd[0] == 1 / math.sqrt(1e-5)


@pytest.mark.parametrize("M,C,p", [(37, 16, 0.0), (53, 24, 0.15), (2, 8, 0.5)])
def test_batchnorm_matches_torch(M, C, p):
    rng = np.random.default_rng(M * C)
    x, dy = rng.standard_normal((M, C)) * 1.5 + 0.3, rng.standard_normal((M, C))
    gamma, beta = 1 + 0.3 * rng.standard_normal(C), 0.2 * rng.standard_normal(C)
    gamma[1], gamma[2] = -0.7, 0.0
    rm, rv = 0.1 * rng.standard_normal(C), 0.5 + rng.random(C)
    keep = H.DH.keep_mask(11, 3, (M, C), p) if p > 0 else None
    scale = H.DH.engine_scale(p)
    y, mean, rstd, nrm, nrv = H.batchnorm_act_fwd(x, gamma, beta, rm, rv, 0.1, 1e-5, True, 0.01, keep, scale)
    tx, tg, tb = _t(x, True), _t(gamma, True), _t(beta, True)
    trm, trv = _t(rm), _t(rv)
    ty = F.leaky_relu(F.batch_norm(tx, trm, trv, tg, tb, True, 0.1, 1e-5), 0.01)
    if keep is not None:
        ty = ty * _t(keep.astype(np.float64) * scale)
    ty.backward(_t(dy))
    assert _rel(y, ty.detach().numpy()) < 1e-12
    assert _rel(nrm, trm.numpy()) < 1e-12 and _rel(nrv, trv.numpy()) < 1e-12
    tv, tm = torch.var_mean(_t(x), dim=0, unbiased=False)
    assert _rel(mean, tm.numpy()) < 1e-12 and _rel(rstd, torch.rsqrt(tv + 1e-5).numpy()) < 1e-12
    dx, dgamma, dbeta, sg, sgx = H.batchnorm_act_bwd(dy, x, gamma, beta, mean, rstd, 0.01, keep, scale)
    assert _rel(dx, tx.grad.numpy()) < 1e-12 and _rel(dgamma, tg.grad.numpy()) < 1e-12 and _rel(dbeta, tb.grad.numpy()) < 1e-12
    assert np.array_equal(sg, dbeta) and np.array_equal(sgx, dgamma)
    # two row halves with the global totals and row count reproduce the whole batch (the synchronised form)
    h = M // 2
    parts = [H.batchnorm_act_bwd(dy[s], x[s], gamma, beta, mean, rstd, 0.01, None if keep is None else keep[s], scale)
             for s in (slice(0, h), slice(h, M))]
    tot = (parts[0][3] + parts[1][3], parts[0][4] + parts[1][4], M)
    dx2 = np.concatenate([H.batchnorm_act_bwd(dy[s], x[s], gamma, beta, mean, rstd, 0.01, None if keep is None else keep[s], scale,
                                              totals=tot)[0] for s in (slice(0, h), slice(h, M))])
    assert _rel(dx2, dx) < 1e-12
    s1, s2, rows = H.batchnorm_sums(x)
    assert rows == M and _rel(s1 / M, mean) < 1e-12 and _rel(1 / np.sqrt(s2 / M - (s1 / M) ** 2 + 1e-5), rstd) < 1e-9
    # evaluation: the running statistics, no dropout, statistics unchanged
    ye, me, re_, erm, erv = H.batchnorm_act_fwd(x, gamma, beta, nrm, nrv, 0.1, 1e-5, False, 0.01, keep, scale)
    te = F.leaky_relu(F.batch_norm(_t(x), _t(nrm), _t(nrv), _t(gamma), _t(beta), False, 0.1, 1e-5), 0.01)
    assert _rel(ye, te.numpy()) < 1e-12 and np.array_equal(erm, nrm) and np.array_equal(erv, nrv) and np.array_equal(me, nrm)


def test_batchnorm_single_row():
    x = np.array([[1.0, -2.0, 0.0, 3.0, 0.5, 0.25, 8.0, -1.0]])
    y, mean, rstd, nrm, nrv = H.batchnorm_act_fwd(x, np.ones(8), np.full(8, -0.5), np.zeros(8), np.ones(8), 0.1, 1e-5, True, 0.01, None, 1.0)
    assert np.array_equal(mean, x[0]) and np.allclose(rstd, 1e-5 ** -0.5) and np.allclose(y, -0.005)
    assert np.allclose(nrv, 0.9) and np.allclose(nrm, 0.1 * x[0])


@pytest.mark.parametrize("wd,gs,max_norm", [(0.0, 1.0, 1.0), (0.01, 0.25, 1.0), (0.01, 1.0, 0.0), (0.01, 0.5, 100.0)])
def test_adamw_matches_torch(wd, gs, max_norm):
    """Three steps; the kernel's gradients are the true ones divided by the loss scale gs, torch sees the true ones."""
    rng = np.random.default_rng(3)
    n = 301
    p0 = rng.standard_normal(n)
    tp = _t(p0, True)
    opt = torch.optim.AdamW([tp], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for step in (1, 2, 3):
        g_true = rng.standard_normal(n) * (0.3 if step == 2 else 0.01)
        tp.grad = _t(g_true)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        g_dev = g_true / gs
        coef = H.clip_coef(float((g_dev ** 2).sum()), max_norm, gs)
        p, m, v = H.adamw_step(p, g_dev, m, v, coef, 1e-3, 0.9, 0.999, 1e-8, wd, step)
    assert _rel(p, tp.detach().numpy()) < 1e-12
    st = opt.state[tp]
    assert _rel(m, st["exp_avg"].numpy()) < 1e-12 and _rel(v, st["exp_avg_sq"].numpy()) < 1e-12


@pytest.mark.parametrize("wd,gs,max_norm", [(0.0, 1.0, 5.0), (0.01, 0.25, 5.0), (0.01, 1.0, 0.0)])
def test_adadelta_matches_torch(wd, gs, max_norm):
    rng = np.random.default_rng(4)
    n = 257
    p0 = rng.standard_normal(n)
    tp = _t(p0, True)
    opt = torch.optim.Adadelta([tp], lr=1.0, rho=0.95, eps=1e-8, weight_decay=wd)
    p, sq, acc = p0.copy(), np.zeros(n), np.zeros(n)
    for step in range(4):
        g_true = rng.standard_normal(n) * (30.0 if step == 2 else 0.01)
        tp.grad = _t(g_true)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        g_dev = g_true / gs
        p, sq, acc = H.adadelta_step(p, g_dev, sq, acc, H.clip_coef(float((g_dev ** 2).sum()), max_norm, gs), 1.0, 0.95, 1e-8, wd)
    st = opt.state[tp]
    assert _rel(p, tp.detach().numpy()) < 1e-12
    assert _rel(sq, st["square_avg"].numpy()) < 1e-12 and _rel(acc, st["acc_delta"].numpy()) < 1e-12


# ------------------------------------------------------------------------------------------------ launch geometry
def _const(text, name):
    m = re.search(r"constexpr int %s = (\d+);" % name, text)
    assert m, name
    return int(m.group(1))


def test_kernel_constants():
    """The constants the geometry helper restates are the kernel files' (a change there: revisit the shapes of the GPU test)."""
    sb = open(os.path.join(SRC, "sb_head.hip")).read()
    op = open(os.path.join(SRC, "optim.hip")).read()
    assert _const(sb, "BN_ROW_BLOCKS") == H.BN_ROW_BLOCKS and _const(sb, "BN_STAT_THREADS") == H.BN_STAT_THREADS
    assert _const(sb, "UN_BLOCKS") == H.UN_BLOCKS
    assert "const RowMap m(C, 256);" in sb and "want > 4096 ? 4096 : want" in sb and "ssak_cdiv(M, lanes_a * 4)" in sb
    assert "fmin(512.0, (double)ssak_cdiv(n, 256 * Chunk<T>::N))" in sb
    assert "fmin(2048.0, (double)ssak_cdiv(n, 256))" in sb
    assert "fmin(1024.0, (double)ssak_cdiv(n, 1024))" in op and "fmin(4096.0, (double)ssak_cdiv(n, 1024))" in op
    assert "r += 4 * stride" in sb and sb.count("r += 2 * stride") == 2
    common = open(os.path.join(SRC, "common.h")).read()
    assert _const(common, "DROP_TABLE_N") >= max(C for _, C in H.BN_DROP_SHAPES)


# (M, C): lanes_s, idle_s, nb, cb_stat, live_last_s, steps_s, trips4, trips2, lanes_a, cb_apply, live_last_a, ab, apply_trips4, apply_trips2
GEOMETRY = {
    (1, 8): (1024, 0, 1, 1, 1, 0, 1, 1, 256, 1, 1, 1, 1, 1),
    (5, 8): (1024, 0, 1, 1, 1, 0, 1, 1, 256, 1, 1, 1, 1, 1),
    (1030, 24): (341, 1, 4, 1, 3, 0, 1, 1, 85, 1, 3, 4, 1, 2),
    (174700, 24): (341, 1, 512, 1, 3, 1, 1, 1, 85, 1, 3, 514, 1, 2),
    (700, 64): (128, 0, 6, 1, 8, 0, 1, 1, 32, 1, 8, 6, 1, 2),
    (1497, 1024): (8, 0, 188, 1, 128, 0, 1, 1, 2, 1, 128, 188, 1, 2),
    (4097, 1024): (8, 0, 512, 1, 128, 1, 1, 1, 2, 1, 128, 513, 1, 2),
    (513, 8192): (1, 0, 512, 1, 1024, 1, 1, 1, 1, 4, 256, 129, 1, 2),
    (2049, 8192): (1, 0, 512, 1, 1024, 3, 2, 3, 1, 4, 256, 513, 1, 2),
    (600, 8200): (1, 0, 512, 2, 1, 1, 1, 1, 1, 5, 1, 150, 1, 2),
    (16500, 2056): (3, 253, 512, 1, 257, 3, 3, 6, 1, 2, 1, 4096, 2, 3),
}


@pytest.mark.parametrize("M,C", H.BN_SHAPES)
def test_bn_geometry(M, C):
    g = H.bn_geometry(M, C)
    got = (g.lanes_s, g.idle_s, g.nb, g.cb_stat, g.live_last_s, g.steps_s, g.trips4, g.trips2, g.lanes_a, g.cb_apply, g.live_last_a,
           g.ab, g.apply_trips4, g.apply_trips2)
    assert got == GEOMETRY[(M, C)]
    assert g.lds_bytes <= 65536 and g.stride_s * 3 + M < 2 ** 31 and g.stride_a * 3 + M < 2 ** 31


def test_bn_shapes_reach_every_branch():
    gs = {s: H.bn_geometry(*s) for s in H.BN_SHAPES}
    assert gs[(1030, 24)].idle_s and gs[(1030, 24)].idle_a and gs[(1030, 24)].steps_s == 0       # idle thread, no unrolled step
    assert gs[(174700, 24)].idle_s and gs[(174700, 24)].steps_s >= 1                             # unrolled steps with an idle thread
    assert all(gs[s].steps_s == 0 for s in [(1, 8), (5, 8), (700, 64), (1497, 1024)])            # the old test's reach
    assert gs[(4097, 1024)].steps_s == 1 and 4097 - gs[(4097, 1024)].stride_s == 1               # u = 1 with one live row
    assert gs[(513, 8192)].lanes_s == 1 and gs[(2049, 8192)].trips4 == 2 and gs[(2049, 8192)].trips2 == 3
    assert gs[(600, 8200)].cb_stat == 2 and gs[(600, 8200)].live_last_s == 1 and gs[(600, 8200)].cb_apply == 5
    assert gs[(16500, 2056)].ab == H.BN_APPLY_CAP and gs[(16500, 2056)].apply_trips4 == 2 and gs[(16500, 2056)].cb_apply == 2
    assert gs[(16500, 2056)].live_last_a == 1
    assert {(M, C) for M, C, p in H.BN_CASES if p > 0} >= {(174700, 24), (2049, 8192), (600, 8200)}


def test_un_and_flat_geometry():
    for bf in (True, False):
        N, part, app = (8, 131072, 1048576) if bf else (4, 65536, 524288)
        trips = {n: H.un_geometry(n, bf) for _, n in H._un_sizes(bf)}
        assert all(trips[n].partial_trips == 1 and trips[n].apply_trips == 1 for n in (1, 3, 4, 7, 8))
        assert trips[1003].partial_trips == 1 and trips[1003].apply_trips == 4   # element by element: one workgroup strides
        assert trips[part + N].vector and trips[part + N].partial_trips == 2 and trips[part + N].apply_trips == 1
        assert not trips[part + N + 1].vector and trips[part + N + 1].partial_trips > 2
        assert H.un_geometry(part, bf).partial_trips == 1 and H.un_geometry(app, bf).apply_trips == 1
        assert trips[app + N].vector and trips[app + N].apply_trips == 2 and trips[app + N].ab == H.UN_APPLY_CAP
        assert not trips[3].vector and trips[8].vector and not trips[1003].vector
    s = {n: H.flat_geometry(n, H.SUMSQ_CAP, 1024) for n in H.SUMSQ_SIZES}
    assert s[3].items == 0 and s[3].tail == 3 and s[1027].blocks == 2 and s[1027].tail == 3 and s[1024].tail == 0
    assert s[1048579].capped and s[1048579].trips == 1 and s[1048583].capped and s[1048583].trips == 2 and s[1048583].tail == 3
    assert s[1310723].capped and s[1310723].trips == 2 and s[1310723].items - 1024 * 256 == 65536
    a = H.flat_geometry(4194309, H.ADAMW_CAP, 1024)
    assert a.capped and a.trips == 2 and a.tail == 1
    d = H.flat_geometry(524289, H.ADADELTA_CAP, 256)
    assert d.capped and d.trips == 2
    assert all(not H.flat_geometry(n, H.ADAMW_CAP, 1024).capped for n in H.OPT_SIZES)


# ------------------------------------------------------------------------------------------------ BatchNorm: constants, preconditions, bite
def _bn_bars_constants(d):
    """c_sum(depth) and k_stat(depth) are at least 4 x the error of the fp32 re-evaluation with the kernel's summation shape."""
    M, C = d.M, d.C
    x32 = d.x.astype(np.float32)
    s, q = H.column_sums_fp32(x32, x32, M, C)
    rs, rq, _ = H.batchnorm_sums(d.x)
    worst_sum = max(float((np.abs(s - rs) / (U * np.abs(d.x).sum(0) + H.TINY)).max()), float((np.abs(q - rq) / (U * rq + H.TINY)).max()))
    mu = s / M
    var = np.maximum(q / M - mu * mu, 0)
    mean32, rstd32 = H.round_f32(mu), H.round_f32(1 / np.sqrt(var + H.EPS))
    worst_mean = float((np.abs(mean32 - d.mean) / (U * (np.abs(d.mean) + np.sqrt(d.var)) + H.TINY)).max())
    den = U * (d.var + d.mean ** 2) / (d.var + H.EPS)
    ok = den > 0
    worst_rstd = float((np.maximum(np.abs(rstd32 / d.rstd - 1) - 2 * U, 0)[ok] / den[ok]).max()) if ok.any() else 0.0
    # the backward's totals: g and xhat evaluated in fp32 as the kernel does
    mu32, rs32 = d.mean32.astype(np.float32), d.rstd32.astype(np.float32)
    xh = (x32 - mu32) * rs32
    z = xh * d.gamma.astype(np.float32) + d.beta.astype(np.float32)
    dy32 = d.dy.astype(np.float32)
    g = np.where(z > 0, dy32, dy32 * np.float32(H.SLOPE))
    sg, sgx = H.column_sums_fp32(g, xh, M, C)
    worst_bwd = max(float((np.maximum(np.abs(sg - d.tot_g) - d.terms.flip_g - 4 * U * d.terms.abs_g, 0) / (U * d.terms.abs_g + H.TINY)).max()),
                    float((np.maximum(np.abs(sgx - d.tot_gx) - d.terms.flip_gx - 4 * U * d.terms.abs_gx, 0) / (U * d.terms.abs_gx + H.TINY)).max()))
    print(f"BN ({M}, {C}): depth {H.bn_geometry(M, C).depth}  sum {worst_sum:.3f}  bwd totals {worst_bwd:.3f}  mean {worst_mean:.3f}  rstd {worst_rstd:.3f}")
    assert 4 * max(worst_sum, worst_bwd) <= d.c_sum
    assert 4 * max(worst_mean, worst_rstd) <= d.k_stat


def _outside(ratio):
    return bool((np.asarray(ratio) > 1.0).any())


@pytest.mark.parametrize("M,C,p", H.BN_CASES)
def test_bn_bars_bite(M, C, p):
    d = H.bn_case(M, C, p)
    c = np.arange(C)
    kind = c % 4
    live = kind != 1 if M > 1 else np.zeros(C, bool)  # the constant columns are exempt from the count
    d_mean, d_rstd = H.stat_bars(d.mean, d.var, H.EPS, d.k_stat)
    args = (d.x, d.gamma, d.beta, d.mean, d.rstd, d_mean, d_rstd, H.SLOPE, d.keep, d.scale)
    right = H.bn_y_check(d.y, *args)
    # ---- preconditions, on the reference alone
    assert right.ratio.max() == 0.0 and right.dropped_nonzero == 0
    if live.any():
        assert right.ambiguous[:, live].mean() <= 0.01, right.ambiguous[:, live].mean()
        assert d.terms.amb[:, live].mean() <= 0.01
    assert not right.ambiguous[:, ~live].any() and not d.terms.amb[:, kind == 1].any()   # |beta| >= 0.05 keeps them out
    assert d.terms.flips <= max(2, 2e-6 * M * C), d.terms.flips
    assert (np.abs(d.beta) >= 0.049).all() and (d.gamma < 0).any() and (d.gamma == 0).any() == (C > 5) and (d.gamma > 0).any()
    if M > 1:
        assert (d.var[kind == 1] == 0).all() and (d.var[kind == 2] < 2e-5).all() and (d.var[kind == 2] > 2e-6 / M).all()
        assert np.allclose(d.mean[kind == 3], 8.0, atol=0.5) and (d.var[kind == 0] > 0.5).all()
        assert np.array_equal(H.round_bf16(d.x), d.x) and np.array_equal(H.round_bf16(d.dy), d.dy)
        assert np.median((np.abs(d.tot_gx) / (d.terms.abs_gx + H.TINY))[kind == 0]) > 0.1   # dy leans on xhat: c2 is not noise
    if p > 0:
        assert abs(d.keep.mean() - (1 - p)) < 0.02 + 1.0 / math.sqrt(M * C) and (d.y[~d.keep] == 0).all()
    # ---- statistics
    m_bar, r_rel = d_mean, d_rstd
    if M >= 2:
        unb = d.var * M / (M - 1)
        assert _outside(np.abs(1 / np.sqrt(unb + H.EPS) - d.rstd) / (r_rel * d.rstd)), "unbiased batch variance passes"
        rm_bar, rv_bar = H.running_bars(d.new_rm, d.new_rv, d.mean, d.var, M, H.MOMENTUM, d.k_stat)
        biased_rv = (1 - H.MOMENTUM) * d.run_var + H.MOMENTUM * d.var
        assert _outside(np.abs(biased_rv - d.new_rv) / rv_bar), "biased running variance passes"
    assert _outside(np.abs(1 / (np.sqrt(d.var) + H.EPS) - d.rstd) / (r_rel * d.rstd)), "eps outside the root passes"
    # ---- forward output and dx: element-wise, so the first 2048 rows of a large case carry them
    sl = slice(0, min(M, 2048))
    kp = None if d.keep is None else d.keep[sl]
    sargs = (d.x[sl], d.gamma, d.beta, d.mean, d.rstd, d_mean, d_rstd, H.SLOPE, kp, d.scale)
    z = (d.x[sl] - d.mean) * d.rstd * d.gamma + d.beta
    if p > 0:
        assert _outside(H.bn_y_check(H.apply_keep(H.leaky(z, H.SLOPE), kp, 1.0), *sargs).ratio), "a missing 1 / (1 - p) passes"
        leak = d.y[sl].copy()
        leak[~kp] = H.leaky(z, H.SLOPE)[~kp]
        assert H.bn_y_check(leak, *sargs).dropped_nonzero > 0
    wrong_sign = H.apply_keep(np.where(z > 0, z * H.SLOPE, z), kp, d.scale)
    assert _outside(H.bn_y_check(wrong_sign, *sargs).ratio), "the slope on the wrong sign passes"
    t = d.terms
    ts = SimpleNamespace(g=t.g[sl], g_alt=t.g_alt[sl], xh=t.xh[sl], amb=t.amb[sl])
    targs = (ts, d.gamma, d.rstd32, d.tot_g, d.tot_gx, d.bar_g, d.bar_gx, M)
    dx_ref = H.bn_dx_check(np.zeros_like(ts.g), *targs)[1]
    assert H.bn_dx_check(dx_ref, *targs)[0].max() == 0.0
    if M >= 2:
        assert _outside(H.bn_dx_check(d.gamma * d.rstd32 * (ts.g - d.tot_g / M), *targs)[0]), "dx without mean(g xhat) passes"
        assert _outside(np.abs(t.g_alt.sum(0) - d.tot_g) / d.bar_g), "leaky' on the wrong sign passes the totals"
    # one row, and one 8-column chunk of one row, left out of a column total
    s1, s2, _ = H.batchnorm_sums(d.x)
    bar1, bar2 = d.c_sum * U * np.abs(d.x).sum(0) + H.TINY, d.c_sum * U * s2 + H.TINY
    rows = sorted({M - 1, M // 2, 0})
    for r in rows:
        assert _outside(np.abs(d.x[r]) / bar1) and _outside(d.x[r] ** 2 / bar2), f"row {r} left out of the statistics passes"
        assert _outside(np.abs(t.g[r]) / d.bar_g) and (M == 1 or _outside(np.abs(t.g[r] * t.xh[r]) / d.bar_gx)), f"row {r} left out passes"
    if M >= 2:
        # A chunk of 8 columns of one row left out moves eight totals by that row's own terms, so it is caught wherever one of
        # the eight exceeds the column's bar.  It cannot be caught where all eight sit under c u sum|terms| -- at M = 174 700 that is
        # |g| <= 0.25, e.g. eight elements that are dropped or on the slope side -- which is inherent in comparing totals.  Asserted:
        # for x (no element is small in every column kind) every chunk of the probed rows is caught; for g at least 95 % of them are,
        # and every chunk whose |g| are all under the bar has |dy| leaky' scale under the bar too (it is small, not overlooked).
        for r in rows:
            cx = (np.abs(d.x[r]) / bar1 > 1).reshape(-1, 8).any(axis=1) | (d.x[r] ** 2 / bar2 > 1).reshape(-1, 8).any(axis=1)
            assert cx.all(), f"{int((~cx).sum())} chunks of row {r} left out of the statistics pass"
        cg = np.concatenate([(np.abs(t.g[r]) / d.bar_g > 1).reshape(-1, 8).any(axis=1) for r in rows])
        assert cg.mean() >= 0.95, f"only {cg.mean():.3f} of the chunks left out of sum g are caught"
    if p == 0:
        _bn_bars_constants(d)


# ------------------------------------------------------------------------------------------------ utterance normalisation
@pytest.mark.parametrize("bf16,B,n", H.UN_CASES)
def test_un_bars_bite(bf16, B, n):
    d = H.un_case(bf16, B, n)
    assert np.array_equal(H.round_to(d.x, bf16), d.x)
    assert d.var[1] == 0 and d.mean[1] == 0.5 and (d.y[1] == 0).all()
    if not bf16 and B > 2 and n > 8:
        assert d.mean[2] > 25 * math.sqrt(d.var[2])
    _, r_rel = H.stat_bars(d.mean, d.var, H.EPS, d.k)
    assert _outside(np.abs(1 / (np.sqrt(d.var) + H.EPS) - d.rstd) / (r_rel * d.rstd)), "eps outside the root passes"
    if 2 <= n <= 1003:
        # (past ~1e5 elements 1 / 2n is below the rigorous depth * u bound of the partial sums: the small sizes carry this one)
        assert _outside(np.abs(1 / np.sqrt(d.var * n / (n - 1) + H.EPS) - d.rstd) / (r_rel * d.rstd)), "unbiased variance passes"
    if n >= 7:
        bar = H.un_dx_bar(d)
        c1 = d.dy.mean(1, keepdims=True)
        assert _outside(np.abs(d.rstd32[:, None] * (d.dy - c1) - d.dx) / bar), "dx without mean(dy y) passes"
        assert _outside(np.abs(d.rstd32[:, None] * d.dy - d.dx) / bar), "dx without the mean terms passes"
        ybar = H.un_y_bar(d)
        assert _outside(np.abs(d.x * d.rstd[:, None] - d.y) / ybar), "y without the mean passes"
        skipped = d.y.copy()
        skipped[0, -1] = d.x[0, -1]
        assert _outside(np.abs(skipped - d.y) / ybar), "a tail element left as it was passes"
    g = H.un_geometry(n, bf16)
    if g.partial_trips > 1:
        # the first item of the partial pass's second trip (a vector of N elements, or one element) left out of utterance 0's sums.
        # At the apply-stride sizes one item is 1e-5 of the sum, under the rigorous (depth + 2) u of its eight trips: there the
        # whole second trip (64 x 256 items) is what is left out.
        w = (g.N if g.vector else 1) * (1 if g.apply_trips == 1 or not g.vector else H.UN_BLOCKS * H.UN_THREADS)
        lo = H.UN_BLOCKS * H.UN_THREADS * (g.N if g.vector else 1)
        x0, dy0, y0 = d.x[0], d.dy[0], d.y_st[0]
        m_bar, r_rel = H.stat_bars(d.mean, d.var, H.EPS, d.k)
        mu = (x0.sum() - x0[lo:lo + w].sum()) / n
        var = ((x0 * x0).sum() - (x0[lo:lo + w] ** 2).sum()) / n - mu * mu
        assert abs(mu - d.mean[0]) > m_bar[0] or abs(1 / math.sqrt(var + H.EPS) / d.rstd[0] - 1) > r_rel[0], "an item of the second trip left out"
        c1 = (dy0.sum() - dy0[lo:lo + w].sum()) / n
        c2 = ((dy0 * y0).sum() - (dy0 * y0)[lo:lo + w].sum()) / n
        assert _outside(np.abs(d.rstd32[0] * (dy0 - c1 - y0 * c2) - d.dx[0]) / H.un_dx_bar(d)[0]), "an item of the second trip left out (bwd)"


# ------------------------------------------------------------------------------------------------ optimizers
def test_optimizer_preconditions():
    lr, wd = np.float32(H.ADAM_LR), np.float32(H.WD)
    assert float(lr) == H.ADAM_LR
    decay32 = float(np.float32(1) - lr * wd)
    assert abs(decay32 - (1 - H.ADAM_LR * H.WD)) < 0.01 * U
    for b in (H.BETA1, H.BETA2, H.RHO):   # 1 - b is exact in fp32: the reference's (1 - b) is the kernel's
        assert float(np.float32(1) - np.float32(b)) == 1.0 - b
    want = {"clipped": 1, "not_clipped": -1, "max_norm0": 0, "no_norm": 0, "scale_clipped": 1, "scale_not_clipped": -1}
    for name, side in want.items():
        for cfgs in (H.ADAMW_CONFIGS, H.ADADELTA_CONFIGS):
            cfg = cfgs[name]
            got, margin = H.clip_side(cfg[1], cfg[2], cfg[3])
            assert got == side and margin > 0.2, (name, got, margin)
            coef = H.clip_coef(cfg[1], H.f32(cfg[2]), H.f32(cfg[3]))
            assert (coef < cfg[3] * 0.9) == (side == 1) and (side == 1 or coef == cfg[3])
    assert {c[5] for c in H.ADAMW_CONFIGS.values()} == {1, 2, 1000}
    assert {c[4] for c in H.ADAMW_CONFIGS.values()} == {0.0, H.WD} == {c[4] for c in H.ADADELTA_CONFIGS.values()}
    for n in (1027, 262147):
        d = H.opt_inputs(n)
        assert (d.g == 0).any() and (d.v == 0).any() and ((d.v > 0) & (d.v < 1e-18)).any() and ((d.g == 0) & (d.v == 0)).any()
        assert (d.m != 0).all() and (d.g[n - n % 4:] != 0).all() and (d.g * d.m >= 0).all() and (d.g * d.p >= 0).all()
    assert H.c_bc(1) > 1000 and H.c_bc(2) > 500 and H.c_bc(1000) < 34


def _adamw_wrong(n, cfg, which):
    shadow, sumsq, max_norm, gs, wd, step = cfg
    d = H.opt_inputs(n)
    lr, b1, b2, eps, wd = H.ADAM_LR, H.BETA1, H.BETA2, H.ADAM_EPS, H.f32(wd)
    coef = H.clip_coef(sumsq, H.f32(max_norm), H.f32(gs))
    if which == "clip_without_scale" and sumsq is not None and max_norm > 0:
        coef = gs * min(1.0, max_norm / (math.sqrt(sumsq) + 1e-6))
    gk = d.g * coef
    if which == "coupled_decay":
        gk = gk + wd * d.p
    m = b1 * d.m + (1 - b1) * gk
    v = b2 * d.v + (1 - b2) * gk * gk
    t = step - 1 if which == "zero_based_step" else step
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1, bc2 = np.float64(1 - b1 ** t), np.float64(1 - b2 ** t)
        denom = np.sqrt(v / bc2 + eps) if which == "eps_inside_root" else np.sqrt(v) / np.sqrt(bc2) + eps
        p = d.p * (1.0 if which == "coupled_decay" else 1 - lr * wd) - lr / bc1 * (m / denom)
    if which == "tail_skipped":
        p[n - 1] = d.p[n - 1]
    return p


@pytest.mark.parametrize("n", H.ADAMW_SIZES)
def test_adamw_bars_bite(n):
    for name in [c for m, c in H.opt_cases(H.ADAMW_SIZES, H.ADAMW_CONFIGS) if m == n]:
        cfg = H.ADAMW_CONFIGS[name]
        ref = H.adamw_reference(n, cfg)
        assert np.array_equal(_adamw_wrong(n, cfg, None), ref.p)
        wrongs = ["zero_based_step", "eps_inside_root", "tail_skipped"]
        if cfg[4] > 0:
            wrongs.append("coupled_decay")
        if cfg[3] != 1.0:
            wrongs.append("clip_without_scale")
        for w in wrongs:
            p = _adamw_wrong(n, cfg, w)
            assert not np.isfinite(p).all() or _outside(np.abs(p - ref.p) / ref.p_bar), (name, w)


@pytest.mark.parametrize("n", H.ADADELTA_SIZES)
def test_adadelta_bars_bite(n):
    d = H.opt_inputs(n)
    for name in [c for m, c in H.opt_cases(H.ADADELTA_SIZES, H.ADADELTA_CONFIGS) if m == n]:
        cfg = H.ADADELTA_CONFIGS[name]
        shadow, sumsq, max_norm, gs, wd = cfg
        ref = H.adadelta_reference(n, cfg)
        coef = H.clip_coef(sumsq, H.f32(max_norm), H.f32(gs))
        gk = d.g * coef + H.f32(wd) * d.p
        delta2 = np.sqrt(ref.acc + H.DELTA_EPS) / np.sqrt(ref.sq + H.DELTA_EPS) * gk     # the UPDATED acc_delta
        assert _outside(np.abs(d.p - delta2 - ref.p) / ref.p_bar), (name, "updated acc_delta")
        tail = ref.p.copy()
        tail[n - 1] = d.p[n - 1]
        assert _outside(np.abs(tail - ref.p) / ref.p_bar), (name, "tail")
        if gs != 1.0:
            c2 = gs * min(1.0, max_norm / (math.sqrt(sumsq) + 1e-6))
            p2 = H.adadelta_step(d.p, d.g, d.v, d.acc, c2, 1.0, H.RHO, H.DELTA_EPS, H.f32(wd))[0]
            assert _outside(np.abs(p2 - ref.p) / ref.p_bar), (name, "clip without the scale")
        if wd > 0:
            p3 = H.adadelta_step(d.p, d.g, d.v, d.acc, coef, 1.0, H.RHO, H.DELTA_EPS, 0.0)[0] * (1 - H.f32(wd))
            assert _outside(np.abs(p3 - ref.p) / ref.p_bar), (name, "decoupled decay")


@pytest.mark.parametrize("n", H.SUMSQ_SIZES)
def test_sumsq_bar_bites(n):
    d = H.sumsq_inputs(n)
    g = H.flat_geometry(n, H.SUMSQ_CAP, 1024)
    assert g.trips <= 2 and H.SUMSQ_ROUNDINGS == 39 and H.SUMSQ_BAR_U >= H.SUMSQ_ROUNDINGS
    sq = d.g ** 2
    assert sq[n - 1] > d.bar or n % 4 == 0, "the last element left out passes"
    if n >= 8:
        assert sq[4:8].sum() > d.bar, "a float4 left out passes"
    assert (d.second is not None) == (n in (1048583, 1310723))
    if d.second:
        lo, hi = d.second
        assert sq[lo:lo + 4].sum() > d.bar, "the first float4 of the second trip left out passes"
        assert sq[lo:hi].sum() > d.bar, "the second trip left out passes"
        assert abs((d.g[lo:lo + 4] ** 2).sum() - (d.g[0:4] ** 2).sum()) > d.bar, "the second trip reading the first trip's item passes"
