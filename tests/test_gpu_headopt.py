"""GPU: the kernels of ssak_amd/csrc/sb_head.hip and ssak_amd/csrc/optim.hip, one launch at a time through the C ABI, against the
float64 restatement tests/headopt_ref.py (pinned to torch float64 by tests/test_headopt_ref.py, which also shows on these very
inputs that each bar below rejects the usual wrong restatements and that the inputs meet the bars' preconditions).

Which kernel and loop branch each case reaches (tests/test_headopt_ref.py asserts this arithmetic per shape):

* bn_stats_partial_kernel (4 rows per trip) / bn_bwd_partial_kernel (2 rows per trip), RowMap over 1024 threads, test_batchnorm:
  (1, 8), (5, 8): one workgroup, 1024 lanes of which M hold a row, M = 1 gives var = 0;  (1030, 24): 341 lanes and one idle thread
  (rl == lanes), no unrolled step;  (174700, 24): M > 512 x 341, the unrolled step u = 1 loads rows with the idle thread present;
  (700, 64), (1497, 1024): the anchors of test_gpu_sb_head.py, u = 0 only;  (4097, 1024): u = 1 holds one row;  (513, 8192):
  lanes = 1, u = 1 holds one row;  (2049, 8192): the 4-row pass takes a second trip, the 2-row pass a third;  (600, 8200): second
  column block (grid.y = 2) with one live chunk;  (16500, 2056): 3 lanes and 253 idle threads, three trips of the 4-row pass.
* bn_apply_kernel / bn_bwd_apply_kernel, RowMap over 256 threads: idle thread at C = 24 (85 lanes); (600, 8200) the fifth column
  block with one live chunk; (16500, 2056) the grid cap of 4096 with lanes = 1: the forward loop's second trip (the backward's
  third), second column block with one live chunk.  Dropout p = 0.15 at (5, 8), (1030, 24), (174700, 24), (2049, 8192), (600, 8200).
* bn_stats_final_kernel, bn_bwd_final_kernel (coef and sums written or not), bn_running_kernel (evaluation mode, every case).
* bn_sums_final_kernel (ssak_batchnorm_stats), bn_stats_from_sums_kernel, bn_coef_from_sums_kernel, local_sums_out with dx = NULL:
  the synchronised form on two row halves at (5, 8), (1030, 24), (4097, 1024), (600, 8200).
* un_partial_kernel / un_fwd_apply_kernel / un_bwd_apply_kernel<bf16 | float>, test_utt_norm: n = 1, 3, 7 and 1003 element by element
  (1003: the one apply workgroup strides four times), n = 4 (fp32) / 8 vectors; the first vector multiple past 65 536 (fp32) /
  131 072 (bf16) makes the partial pass stride on the vector path, that + 1 on the scalar path; 524 292 (fp32) / 1 048 584 (bf16)
  with B = 2 make the apply pass stride.  stats = NULL at n = 4.
* sumsq_kernel / sumsq_final_kernel, test_grad_sumsq: n = 1, 3 tail only (n / 4 = 0); 4, 1024 no tail; 5, 1023, 1027, 262147 body
  and tail, 2 .. 257 workgroups; 1 048 579 the capped grid (1024) without a second trip; 1 048 583 the capped grid striding
  with one float4 in the second trip, 1 310 723 with 65 536 of them; _add onto 3.5.  g[4:8] and the first float4 of the second
  trip are +-4 there, so that a kernel which loses either misses the bar.
* adamw_kernel, test_adamw: the same n with the capped grid (4096) striding at 4 194 309; shadow / gnorm_sq present and NULL,
  max_norm 0 and 1 on both sides of the clip, grad_scale 1 and 0.25, weight_decay 0 and 0.01, step 1, 2, 1000 at n = 5 and 1027;
  NULL shadow and NULL gnorm_sq also at n = 3 (tail loop only) and at 4 194 309.
* adadelta_kernel, test_adadelta: the same n, the capped grid (2048) striding at 524 289; the same axes with weight_decay coupled,
  the NULL pointers also at n = 3 and 524 289.
* The other entry points of sb_head.hip (ssak_cast_bf16_f32 / cast_bf16_f32_kernel, ssak_cast_f32_bf16, ssak_colsum_bf16) are held
  by tests/test_gpu_ops.py::test_cast_and_colsum_helpers.

Data.  BatchNorm columns cycle through N(0.3, 1.5), a constant (var = 0, rstd = eps^-1/2, y = leaky(beta)), N(1e-3, 3e-3) (variance
near eps) and 8 + k / 16 (mean 8, spread 0.25, exact in bf16); gamma has negative and zero entries, |beta| >= 0.05, the running
statistics start away from (0, 1).  Utterances: N(0.1, 0.3), a constant, and N(-0.2, 0.5) (bf16) or mean 30 x std (fp32).
Optimizer state: m, v non-zero, v = 0 and 1e-20 on some elements (eps decides the denominator), g = 0 on every 7th, eight NaN guard
elements behind every buffer.  m and, for Adadelta, p carry the sign of g, so no sum in the update cancels and the update's
bar is relative to the update itself.

Bars (u = 2^-24; eps_st = 2^-8 for bf16 storage, 2^-22 for fp32), all in tests/headopt_ref.py:

* Dropped positions are exactly 0 in y; kept ones carry the scale through the value bar.
* mean within k u (|mu| + sigma), rstd within k u (var + mu^2) / (var + eps) + 2 u relative, of the float64 statistics of the
  stored input: d var <= 2 k u (var + mu^2) for the one-pass E[x^2] - mu^2 with fp32 partials and float64 totals (for var >> eps this is
  k u (1 + mu^2 / var), the conditioning of that form; it is never larger and stays finite on the constant columns).  Utterance normalisation: k = depth + 2,
  the rigorous bound, depth = the sequential fp32 additions behind one partial (trips x vector width + a 64-lane tree + 4 waves).
  BatchNorm: depth reaches 343 (rows per lane + lanes, added in order) and depth x u cannot tell 1 / M from 1 / (M - 1) at
  M = 174 700, so k = max(4, 0.7 sqrt(depth)): 4 x the measured worst error of the reference re-evaluated in numpy fp32 with the
  kernel's summation shape (2.84 at depth 342, i.e. 0.154 sqrt(depth); table in headopt_ref.py).  Running statistics: u |new| +
  momentum x those bars (x M / (M - 1) for the variance).
* Column totals (ssak_batchnorm_stats, dgamma, dbeta, local_sums_out): c u sum|terms|, c = max(4, 2.4 sqrt(depth)) by the same
  rule (measured 10.73 at depth 342 = 0.58 sqrt(depth)), + 4 u sum|terms| for the roundings inside a backward term, + |dy|
  (1 - slope) for the elements with |z| <= 4 u (|xhat gamma| + |beta|), whose sign three fp32 roundings may flip (at most a handful
  per case).  Row count in slot 2C exact.  grad_sumsq: 42 u sum g^2, rigorous: the longest path from one g to the result has
  39 roundings (its square 1, the float4's additions 3, s += of two trips 2, workgroup 0's tail 1, the 64-lane tree and four
  waves 6 + 4, the final pass over 1024 partials 6 + 16), 3 u are left for the second-order terms.
* y: eps_st |y| + lk scale ((4 u + d rstd) |xhat gamma| + 2 u |beta| + rstd |gamma| d mean), lk = 1 or the slope: the roundings of
  (x - mean) rstd and the fma, and the statistics' bars above (the last term is the cancellation in x - mean on the large-mean
  columns).  dx: eps_st |dx| + |gamma| rstd (4 u |g| + d c1 + |xhat| d c2 + 4 u |xhat c2| + 2 u |c1|) with d c = the totals' bars / M;
  the backward runs on the reference's statistics rounded to fp32, so forward error does not enter.  Elements with |z| < 2^-7
  (|xhat gamma| + |beta|) are compared against both LeakyReLU branches; they are at most 1 % of any case (asserted on the reference).
  The synchronised form meets the same bars on the whole x.
* Utterance normalisation: y within eps_st |y| + (3 u + d rstd) |xhat| + rstd d mean; dx within eps_st |dx| + rstd (d c1 + |y| d c2
  + 3 u (|dy| + |c1| + |y c2|)), d c = k u mean|terms|.
* AdamW: |p - ref| <= 2 u |ref| + c_bc(t) u |update|, |update| = |ref - decay p_old|; c_bc(t) = 32 + 2 b1^t / (1 - b1^t) + b2^t /
  (1 - b2^t) (1 049 at t = 1, 540 at t = 2, 33 at t = 1000): powf within 1 ulp moves 1 - b^t by 2 u b^t, the other 32 are the
  roundings of the expression (counted in headopt_ref.c_bc).  lr is the fp32 number at which the kernel's fp32 decay equals
  1 - lr wd to within 0.01 u (asserted in tests/test_headopt_ref.py; it is 4e-6 u).  m within 8 u, v within 16 u; shadow == bf16(p) exactly.  Adadelta: p within 2 u |ref| + 26 u |lr delta|, sq
  within 18 u, acc within 56 u.  Guard elements still NaN.
* Two launches on the same inputs are bit-identical, everywhere.
"""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import headopt_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = H.U
INVALID = -1


def _hip():
    import ssak_amd.hip as hip
    return hip


def _dev(a, dt=F32):
    return torch.tensor(np.asarray(a, dtype=np.float32)).to(dt).to(DEV).contiguous()


def _host(t):
    return t.double().cpu().numpy()


def _nan(shape, dt=F32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dt, device=DEV)


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)


def _guarded(a, dt=F32):
    """[n + GUARD] device tensor: the values, then NaN guard elements."""
    t = _nan(len(a) + H.GUARD, dt)
    t[:len(a)] = _dev(a, dt)
    return t


class Report:
    """Collects every miss of a case (a forward miss must not hide the backward's)."""

    def __init__(self):
        self.fails = []

    def ratio(self, name, ratio):
        ratio = np.asarray(ratio)
        if not np.isfinite(ratio).all():
            self.fails.append(f"{name}: non-finite")
            return
        w = float(ratio.max()) if ratio.size else 0.0
        print(f"  {name}: worst error / bar = {w:.3f}")
        if w > 1.0:
            k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            self.fails.append(f"{name}: {int((ratio > 1).sum())} of {ratio.size} outside the bar, worst {w:.3g} x bar at {k}")

    def bar(self, name, got, ref, bar):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        if not np.isfinite(got).all():
            self.fails.append(f"{name}: non-finite")
            return
        self.ratio(name, np.abs(got - ref) / bar)

    def true(self, name, cond):
        if not cond:
            self.fails.append(name)

    def done(self):
        assert not self.fails, "\n".join(self.fails)


# ------------------------------------------------------------------------------------------------ BatchNorm1d + LeakyReLU + dropout
def _bn_fwd(hip, x, rows, Cc, gamma, beta, rm, rv, training, p, gsums, ws):
    y = _nan((rows, Cc), BF)
    mean, rstd = _nan(Cc), _nan(Cc)
    hip.check(hip.lib.ssak_batchnorm_act_fwd(hip.ptr(x), hip.ptr(y), rows, Cc, hip.ptr(gamma), hip.ptr(beta), hip.ptr(rm), hip.ptr(rv),
                                             H.MOMENTUM, H.EPS, int(training), H.SLOPE, p, C.c_uint64(H.BN_SEED), H.BN_STREAM,
                                             hip.ptr(mean), hip.ptr(rstd), hip.ptr(gsums), hip.ptr(ws), ws.numel(), hip.stream()))
    torch.cuda.synchronize()
    return y, mean, rstd


def _bn_bwd(hip, dy, x, rows, Cc, gamma, beta, mean, rstd, p, dx, dg, db, lsums, gsums, ws):
    hip.check(hip.lib.ssak_batchnorm_act_bwd(hip.ptr(dy), hip.ptr(x), hip.ptr(dx), rows, Cc, hip.ptr(gamma), hip.ptr(beta), hip.ptr(mean),
                                             hip.ptr(rstd), H.SLOPE, p, C.c_uint64(H.BN_SEED), H.BN_STREAM, hip.ptr(dg), hip.ptr(db),
                                             hip.ptr(lsums), hip.ptr(gsums), hip.ptr(ws), ws.numel(), hip.stream()))
    torch.cuda.synchronize()


def _slice_terms(t, sl):
    return SimpleNamespace(g=t.g[sl], g_alt=t.g_alt[sl], xh=t.xh[sl], amb=t.amb[sl])


@pytest.mark.parametrize("M,Cc,p", H.BN_CASES, ids=[f"{M}x{Cc}-p{p}" for M, Cc, p in H.BN_CASES])
def test_batchnorm(M, Cc, p):
    hip = _hip()
    d = H.bn_case(M, Cc, p)
    R = Report()
    x, dy = _dev(d.x, BF), _dev(d.dy, BF)
    gamma, beta = _dev(d.gamma), _dev(d.beta)
    ws = _ws(hip.lib.ssak_batchnorm_workspace_bytes(Cc))
    d_mean, d_rstd = H.stat_bars(d.mean, d.var, H.EPS, d.k_stat)
    rm_bar, rv_bar = H.running_bars(d.new_rm, d.new_rv, d.mean, d.var, M, H.MOMENTUM, d.k_stat)

    def check_stats(tag, mean, rstd, rm, rv):
        R.bar(f"{tag} mean", _host(mean), d.mean, d_mean)
        R.bar(f"{tag} rstd", _host(rstd), d.rstd, d_rstd * d.rstd)
        R.bar(f"{tag} running_mean", _host(rm), d.new_rm, rm_bar)
        R.bar(f"{tag} running_var", _host(rv), d.new_rv, rv_bar)

    # ---- training forward
    rm, rv = _dev(d.run_mean), _dev(d.run_var)
    y, mean, rstd = _bn_fwd(hip, x, M, Cc, gamma, beta, rm, rv, True, p, None, ws)
    check_stats("fwd", mean, rstd, rm, rv)
    c = H.bn_y_check(_host(y), d.x, d.gamma, d.beta, d.mean, d.rstd, d_mean, d_rstd, H.SLOPE, d.keep, d.scale)
    R.ratio("fwd y", c.ratio)
    R.true(f"fwd y: {c.dropped_nonzero} dropped positions are not 0", c.dropped_nonzero == 0)
    rm2, rv2 = _dev(d.run_mean), _dev(d.run_var)
    y2, mean2, rstd2 = _bn_fwd(hip, x, M, Cc, gamma, beta, rm2, rv2, True, p, None, ws)
    R.true("fwd: two launches differ", all(torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32),
                                                       b.view(torch.int16 if b.dtype == BF else torch.int32))
                                           for a, b in ((y, y2), (mean, mean2), (rstd, rstd2), (rm, rm2), (rv, rv2))))
    del y2
    # ---- evaluation forward on the same inputs: the running statistics as given, no dropout whatever p says
    rm, rv = _dev(d.run_mean), _dev(d.run_var)
    ye, me, re_ = _bn_fwd(hip, x, M, Cc, gamma, beta, rm, rv, False, p, None, ws)
    e_rstd = 1.0 / np.sqrt(d.run_var + H.EPS)
    R.true("eval: mean is not running_mean", np.array_equal(_host(me), d.run_mean))
    R.true("eval: running statistics changed", np.array_equal(_host(rm), d.run_mean) and np.array_equal(_host(rv), d.run_var))
    R.bar("eval rstd", _host(re_), e_rstd, 2 * U * e_rstd)
    R.ratio("eval y", H.bn_y_check(_host(ye), d.x, d.gamma, d.beta, d.run_mean, e_rstd, 0.0, 2 * U, H.SLOPE, None, 1.0).ratio)
    del ye
    # ---- backward on the reference's statistics (rounded to fp32)
    mean32, rstd32 = _dev(d.mean32), _dev(d.rstd32)
    t = d.terms

    def run_bwd():
        dx, dg, db = _nan((M, Cc), BF), _nan(Cc), _nan(Cc)
        _bn_bwd(hip, dy, x, M, Cc, gamma, beta, mean32, rstd32, p, dx, dg, db, None, None, ws)
        return dx, dg, db
    dx, dg, db = run_bwd()
    R.bar("dgamma", _host(dg), d.tot_gx, d.bar_gx + U * np.abs(d.tot_gx))
    R.bar("dbeta", _host(db), d.tot_g, d.bar_g + U * np.abs(d.tot_g))
    R.ratio("dx", H.bn_dx_check(_host(dx), t, d.gamma, d.rstd32, d.tot_g, d.tot_gx, d.bar_g, d.bar_gx, M)[0])
    dx2, dg2, db2 = run_bwd()
    R.true("bwd: two launches differ", torch.equal(dx.view(torch.int16), dx2.view(torch.int16)) and
           torch.equal(dg.view(torch.int32), dg2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32)))
    del dx, dx2
    # ---- the synchronised form on two row halves
    if p == 0 and (M, Cc) in H.BN_SYNC_SHAPES:
        h = M // 2
        halves = [(slice(0, h), x[:h], dy[:h], h), (slice(h, M), x[h:], dy[h:], M - h)]
        gsum = np.zeros(2 * Cc + 1)
        for i, (sl, xs, _, rows) in enumerate(halves):
            sums = _nan(2 * Cc + 1, F64)
            hip.check(hip.lib.ssak_batchnorm_stats(hip.ptr(xs), rows, Cc, hip.ptr(sums), hip.ptr(ws), ws.numel(), hip.stream()))
            torch.cuda.synchronize()
            s = sums.cpu().numpy()
            r1, r2, _ = H.batchnorm_sums(d.x[sl])
            R.bar(f"stats[{i}] sum x", s[:Cc], r1, d.c_sum * U * np.abs(d.x[sl]).sum(0) + H.TINY)
            R.bar(f"stats[{i}] sum x^2", s[Cc:2 * Cc], r2, d.c_sum * U * r2 + H.TINY)
            R.true(f"stats[{i}]: row count {s[2 * Cc]!r}", s[2 * Cc] == rows)
            gsum += s
        gs = torch.tensor(gsum, dtype=F64, device=DEV)
        lsum = np.zeros(2 * Cc + 1)
        for i, (sl, xs, dys, rows) in enumerate(halves):
            rm, rv = _dev(d.run_mean), _dev(d.run_var)
            y, mean, rstd = _bn_fwd(hip, xs, rows, Cc, gamma, beta, rm, rv, True, 0.0, gs, ws)
            check_stats(f"sync[{i}]", mean, rstd, rm, rv)
            R.ratio(f"sync[{i}] y", H.bn_y_check(_host(y), d.x[sl], d.gamma, d.beta, d.mean, d.rstd, d_mean, d_rstd, H.SLOPE, None, 1.0).ratio)
            dg, db, ls = _nan(Cc), _nan(Cc), _nan(2 * Cc + 1, F64)
            _bn_bwd(hip, dys, xs, rows, Cc, gamma, beta, mean32, rstd32, 0.0, None, dg, db, ls, None, ws)
            s = ls.cpu().numpy()
            rg, rgx = t.g[sl].sum(0), (t.g[sl] * t.xh[sl]).sum(0)
            bg = (d.c_sum + 4) * U * np.abs(t.g[sl]).sum(0) + t.flip_g + H.TINY
            bgx = (d.c_sum + 4) * U * np.abs(t.g[sl] * t.xh[sl]).sum(0) + t.flip_gx + H.TINY
            R.bar(f"local_sums[{i}] sum g", s[:Cc], rg, bg)
            R.bar(f"local_sums[{i}] sum g xhat", s[Cc:2 * Cc], rgx, bgx)
            R.true(f"local_sums[{i}]: row count {s[2 * Cc]!r}", s[2 * Cc] == rows)
            R.bar(f"local dbeta[{i}]", _host(db), rg, bg + U * np.abs(rg))
            R.bar(f"local dgamma[{i}]", _host(dg), rgx, bgx + U * np.abs(rgx))
            lsum += s
        gl = torch.tensor(lsum, dtype=F64, device=DEV)
        for i, (sl, xs, dys, rows) in enumerate(halves):
            dx, dg, db = _nan((rows, Cc), BF), _nan(Cc), _nan(Cc)
            _bn_bwd(hip, dys, xs, rows, Cc, gamma, beta, mean32, rstd32, 0.0, dx, dg, db, None, gl, ws)
            R.true(f"sync[{i}]: the second backward call touched dgamma / dbeta", bool(torch.isnan(dg).all() and torch.isnan(db).all()))
            R.ratio(f"sync[{i}] dx", H.bn_dx_check(_host(dx), _slice_terms(t, sl), d.gamma, d.rstd32, d.tot_g, d.tot_gx, d.bar_g, d.bar_gx, M)[0])
    R.done()


# ------------------------------------------------------------------------------------------------ utterance normalisation
@pytest.mark.parametrize("bf16,B,n", H.UN_CASES, ids=[f"{'bf16' if b else 'fp32'}-{B}x{n}" for b, B, n in H.UN_CASES])
def test_utt_norm(bf16, B, n):
    hip = _hip()
    d = H.un_case(bf16, B, n)
    R = Report()
    dt = BF if bf16 else F32
    bits = torch.int16 if bf16 else torch.int32
    x, dy = _dev(d.x.ravel(), dt), _dev(d.dy.ravel(), dt)
    ws = _ws(hip.lib.ssak_utt_norm_workspace_bytes(B))
    want_stats = n != 4

    def fwd():
        y = _nan(B * n + H.GUARD, dt)
        stats = _nan((B, 2)) if want_stats else None
        hip.check(hip.lib.ssak_utt_norm_fwd(hip.ptr(x), hip.ptr(y), B, n, int(bf16), H.EPS, hip.ptr(stats), hip.ptr(ws), ws.numel(), hip.stream()))
        torch.cuda.synchronize()
        return y, stats
    y, stats = fwd()
    R.true("fwd: guard elements written", bool(torch.isnan(y[B * n:]).all()))
    R.bar("y", _host(y[:B * n]).reshape(B, n), d.y, H.un_y_bar(d))
    R.true("y of the constant utterance is not 0", bool((y[n:2 * n] == 0).all()))
    if want_stats:
        d_mean, d_rstd = H.stat_bars(d.mean, d.var, H.EPS, d.k)
        s = _host(stats)
        R.bar("mean", s[:, 0], d.mean, d_mean)
        R.bar("rstd", s[:, 1], d.rstd, d_rstd * d.rstd)
    y2, stats2 = fwd()
    R.true("fwd: two launches differ", torch.equal(y[:B * n].view(bits), y2[:B * n].view(bits)) and
           (not want_stats or torch.equal(stats.view(torch.int32), stats2.view(torch.int32))))
    # backward on the reference's stored y and its fp32 statistics
    ys = _dev(d.y_st.ravel(), dt)
    st = _dev(np.stack([d.mean, d.rstd32], axis=1))

    def bwd():
        dx = _nan(B * n + H.GUARD, dt)
        hip.check(hip.lib.ssak_utt_norm_bwd(hip.ptr(dy), hip.ptr(ys), hip.ptr(dx), B, n, int(bf16), hip.ptr(st), hip.ptr(ws), ws.numel(), hip.stream()))
        torch.cuda.synchronize()
        return dx
    dx = bwd()
    R.true("bwd: guard elements written", bool(torch.isnan(dx[B * n:]).all()))
    R.bar("dx", _host(dx[:B * n]).reshape(B, n), d.dx, H.un_dx_bar(d))
    R.true("bwd: two launches differ", torch.equal(dx[:B * n].view(bits), bwd()[:B * n].view(bits)))
    R.done()


# ------------------------------------------------------------------------------------------------ optimizers
@pytest.mark.parametrize("n", H.SUMSQ_SIZES)
def test_grad_sumsq(n):
    hip = _hip()
    d = H.sumsq_inputs(n)
    R = Report()
    g = _guarded(d.g)
    ws = _ws(4096)
    out = _nan(2)
    hip.check(hip.lib.ssak_grad_sumsq(hip.ptr(g), n, hip.ptr(out), hip.ptr(ws), 4096, hip.stream()))
    first = out.clone()
    hip.check(hip.lib.ssak_grad_sumsq(hip.ptr(g), n, hip.ptr(out), hip.ptr(ws), 4096, hip.stream()))
    torch.cuda.synchronize()
    R.bar("sumsq", out[0].item(), d.ref, d.bar)
    R.true("out[1] written", bool(torch.isnan(out[1])))
    R.true("two launches differ", torch.equal(first[:1].view(torch.int32), out[:1].view(torch.int32)))
    out[0] = 3.5
    hip.check(hip.lib.ssak_grad_sumsq_add(hip.ptr(g), n, hip.ptr(out), hip.ptr(ws), 4096, hip.stream()))
    torch.cuda.synchronize()
    R.bar("sumsq_add", out[0].item(), 3.5 + d.ref, d.bar + 2 * U * (3.5 + d.ref))
    R.done()


def _opt_cases(sizes, configs):
    return [pytest.param(n, name, id=f"{n}-{name}") for n, name in H.opt_cases(sizes, configs)]


@pytest.mark.parametrize("n,name", list(_opt_cases(H.ADAMW_SIZES, H.ADAMW_CONFIGS)))
def test_adamw(n, name):
    hip = _hip()
    cfg = H.ADAMW_CONFIGS[name]
    use_shadow, sumsq, max_norm, gs, wd, step = cfg
    d = H.opt_inputs(n)
    ref = H.adamw_reference(n, cfg)
    R = Report()
    g = _guarded(d.g)
    gn = None if sumsq is None else _dev([sumsq])

    def run():
        p, m, v = _guarded(d.p), _guarded(d.m), _guarded(d.v)
        sh = _nan(n + H.GUARD, BF) if use_shadow else None
        hip.check(hip.lib.ssak_adamw_step(hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), hip.ptr(sh), n, hip.ptr(gn), max_norm, gs,
                                          H.ADAM_LR, H.BETA1, H.BETA2, H.ADAM_EPS, wd, step, hip.stream()))
        torch.cuda.synchronize()
        return p, m, v, sh
    p, m, v, sh = run()
    R.bar("p", _host(p[:n]), ref.p, ref.p_bar)
    R.bar("m", _host(m[:n]), ref.m, ref.m_bar)
    R.bar("v", _host(v[:n]), ref.v, ref.v_bar)
    bufs = [p, m, v] + ([sh] if use_shadow else [])
    R.true("guard elements written", all(bool(torch.isnan(b[n:]).all()) for b in bufs))
    if use_shadow:
        R.true("shadow != bf16(p)", torch.equal(sh[:n].view(torch.int16), p[:n].to(BF).view(torch.int16)))
    again = run()
    R.true("two launches differ", all(torch.equal(a[:n].view(torch.int16 if a.dtype == BF else torch.int32),
                                                  b[:n].view(torch.int16 if b.dtype == BF else torch.int32))
                                      for a, b in zip((p, m, v, sh), again) if a is not None))
    R.done()


@pytest.mark.parametrize("n,name", list(_opt_cases(H.ADADELTA_SIZES, H.ADADELTA_CONFIGS)))
def test_adadelta(n, name):
    hip = _hip()
    cfg = H.ADADELTA_CONFIGS[name]
    use_shadow, sumsq, max_norm, gs, wd = cfg
    d = H.opt_inputs(n)
    ref = H.adadelta_reference(n, cfg)
    R = Report()
    g = _guarded(d.g)
    gn = None if sumsq is None else _dev([sumsq])

    def run():
        p, sq, acc = _guarded(d.p), _guarded(d.v), _guarded(d.acc)
        sh = _nan(n + H.GUARD, BF) if use_shadow else None
        hip.check(hip.lib.ssak_adadelta_step(hip.ptr(p), hip.ptr(g), hip.ptr(sq), hip.ptr(acc), hip.ptr(sh), n, hip.ptr(gn), max_norm, gs,
                                             1.0, H.RHO, H.DELTA_EPS, wd, hip.stream()))
        torch.cuda.synchronize()
        return p, sq, acc, sh
    p, sq, acc, sh = run()
    R.bar("p", _host(p[:n]), ref.p, ref.p_bar)
    R.bar("square_avg", _host(sq[:n]), ref.sq, ref.sq_bar)
    R.bar("acc_delta", _host(acc[:n]), ref.acc, ref.acc_bar)
    bufs = [p, sq, acc] + ([sh] if use_shadow else [])
    R.true("guard elements written", all(bool(torch.isnan(b[n:]).all()) for b in bufs))
    if use_shadow:
        R.true("shadow != bf16(p)", torch.equal(sh[:n].view(torch.int16), p[:n].to(BF).view(torch.int16)))
    again = run()
    R.true("two launches differ", all(torch.equal(a[:n].view(torch.int16 if a.dtype == BF else torch.int32),
                                                  b[:n].view(torch.int16 if b.dtype == BF else torch.int32))
                                      for a, b in zip((p, sq, acc, sh), again) if a is not None))
    R.done()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    """Misaligned pointers, n <= 0, C % 8 != 0, a short workspace, step = 0, global sums in evaluation mode: the error code comes
    back and the output buffers are as they were."""
    hip = _hip()
    lib, P, S = hip.lib, hip.ptr, hip.stream

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)
    M, Cc = 16, 32
    x = torch.ones(M * Cc + 16, dtype=BF, device=DEV)
    y = torch.full((M * Cc + 16,), 7.0, dtype=BF, device=DEV)
    f = [torch.full((2 * Cc + 8,), 7.0, device=DEV) for _ in range(8)]
    dbl = torch.full((2 * Cc + 1,), 7.0, dtype=F64, device=DEV)
    ws = _ws(lib.ssak_batchnorm_workspace_bytes(Cc))
    u64 = C.c_uint64(1)
    rcs = {}

    def bn_fwd(xp, yp, rows, cols, training, gsums, wsb):
        return lib.ssak_batchnorm_act_fwd(xp, yp, rows, cols, P(f[0]), P(f[1]), P(f[2]), P(f[3]), 0.1, 1e-5, training, 0.01, 0.0, u64, 0, P(f[4]),
                                          P(f[5]), gsums, P(ws), wsb, S())

    def bn_bwd(dyp, xp, dxp, rows, cols, wsb):
        return lib.ssak_batchnorm_act_bwd(dyp, xp, dxp, rows, cols, P(f[0]), P(f[1]), P(f[2]), P(f[3]), 0.01, 0.0, u64, 0, P(f[4]), P(f[5]), None,
                                          None, P(ws), wsb, S())
    rcs["bn fwd misaligned x"] = bn_fwd(off(x, 2), P(y), M, Cc, 1, None, ws.numel())
    rcs["bn fwd misaligned y"] = bn_fwd(P(x), off(y, 8), M, Cc, 1, None, ws.numel())
    rcs["bn fwd M = 0"] = bn_fwd(P(x), P(y), 0, Cc, 1, None, ws.numel())
    rcs["bn fwd C % 8"] = bn_fwd(P(x), P(y), M, 12, 1, None, ws.numel())
    rcs["bn fwd short workspace"] = bn_fwd(P(x), P(y), M, Cc, 1, None, ws.numel() - 1)
    rcs["bn fwd global sums in evaluation"] = bn_fwd(P(x), P(y), M, Cc, 0, P(dbl), ws.numel())
    rcs["bn bwd misaligned dx"] = bn_bwd(P(x), P(x), off(y, 4), M, Cc, ws.numel())
    rcs["bn bwd C % 8"] = bn_bwd(P(x), P(x), P(y), M, 20, ws.numel())
    rcs["bn bwd M = 0"] = bn_bwd(P(x), P(x), P(y), 0, Cc, ws.numel())
    rcs["bn bwd short workspace"] = bn_bwd(P(x), P(x), P(y), M, Cc, ws.numel() - 1)
    rcs["bn stats misaligned"] = lib.ssak_batchnorm_stats(off(x, 2), M, Cc, P(dbl), P(ws), ws.numel(), S())
    rcs["bn stats C % 8"] = lib.ssak_batchnorm_stats(P(x), M, 12, P(dbl), P(ws), ws.numel(), S())
    rcs["bn stats short workspace"] = lib.ssak_batchnorm_stats(P(x), M, Cc, P(dbl), P(ws), ws.numel() - 1, S())
    uws = _ws(lib.ssak_utt_norm_workspace_bytes(2))
    rcs["utt fwd misaligned"] = lib.ssak_utt_norm_fwd(off(x, 2), P(y), 2, 64, 1, 1e-5, P(f[4]), P(uws), uws.numel(), S())
    rcs["utt fwd n = 0"] = lib.ssak_utt_norm_fwd(P(x), P(y), 2, 0, 1, 1e-5, P(f[4]), P(uws), uws.numel(), S())
    rcs["utt fwd B = 0"] = lib.ssak_utt_norm_fwd(P(x), P(y), 0, 64, 1, 1e-5, P(f[4]), P(uws), uws.numel(), S())
    rcs["utt fwd short workspace"] = lib.ssak_utt_norm_fwd(P(x), P(y), 2, 64, 1, 1e-5, P(f[4]), P(uws), uws.numel() - 1, S())
    rcs["utt bwd misaligned"] = lib.ssak_utt_norm_bwd(P(x), P(x), off(y, 2), 2, 64, 1, P(f[0]), P(uws), uws.numel(), S())
    rcs["utt bwd n = 0"] = lib.ssak_utt_norm_bwd(P(x), P(x), P(y), 2, 0, 1, P(f[0]), P(uws), uws.numel(), S())
    rcs["utt bwd short workspace"] = lib.ssak_utt_norm_bwd(P(x), P(x), P(y), 2, 64, 1, P(f[0]), P(uws), uws.numel() - 1, S())
    sws = _ws(4096)
    rcs["sumsq misaligned"] = lib.ssak_grad_sumsq(off(f[0], 4), 8, P(f[6]), P(sws), 4096, S())
    rcs["sumsq n = 0"] = lib.ssak_grad_sumsq(P(f[0]), 0, P(f[6]), P(sws), 4096, S())
    rcs["sumsq short workspace"] = lib.ssak_grad_sumsq(P(f[0]), 8, P(f[6]), P(sws), 4095, S())
    rcs["sumsq_add misaligned"] = lib.ssak_grad_sumsq_add(off(f[0], 4), 8, P(f[6]), P(sws), 4096, S())
    rcs["sumsq_add short workspace"] = lib.ssak_grad_sumsq_add(P(f[0]), 8, P(f[6]), P(sws), 4095, S())

    def adamw(pp, shp, n, step):
        return lib.ssak_adamw_step(pp, P(f[0]), P(f[5]), P(f[6]), shp, n, None, 0.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, S())
    rcs["adamw misaligned p"] = adamw(off(f[4], 4), P(y), 8, 1)
    rcs["adamw misaligned shadow"] = adamw(P(f[4]), off(y, 2), 8, 1)
    rcs["adamw n = 0"] = adamw(P(f[4]), P(y), 0, 1)
    rcs["adamw step = 0"] = adamw(P(f[4]), P(y), 8, 0)
    rcs["adadelta n = 0"] = lib.ssak_adadelta_step(P(f[4]), P(f[0]), P(f[5]), P(f[6]), P(y), 0, None, 0.0, 1.0, 1.0, 0.95, 1e-8, 0.0, S())
    rcs["adadelta no params"] = lib.ssak_adadelta_step(None, P(f[0]), P(f[5]), P(f[6]), P(y), 8, None, 0.0, 1.0, 1.0, 0.95, 1e-8, 0.0, S())
    torch.cuda.synchronize()
    bad = {k: v for k, v in rcs.items() if v != INVALID}
    assert not bad, bad
    assert bool((y == 7.0).all()) and bool((dbl == 7.0).all()) and all(bool((t == 7.0).all()) for t in f)
