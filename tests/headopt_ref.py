"""Float64 numpy restatement of the SpeechBrain-head kernels of ssak_amd/csrc/sb_head.hip (utterance normalisation, BatchNorm1d +
LeakyReLU + dropout with its synchronised-statistics form, Adadelta) and of the optimizer kernels of ssak_amd/csrc/optim.hip
(sum of squares, AdamW), with the inputs, the launch-geometry arithmetic and the error bars that tests/test_headopt_ref.py (CPU)
and tests/test_gpu_headopt.py (GPU) share.

Written from what the kernels define, not from what they compute.  Every function takes the arrays as the kernel sees them
(bf16-stored inputs widened to float64, the fp32 scalars as the fp32 values that pass through the C ABI) and works in float64;
dropout masks come from ``oracle.dropout_hash.keep_mask`` and the scale from ``engine_scale``.  tests/test_headopt_ref.py pins the
functions to torch float64 (F.layer_norm, F.batch_norm + F.leaky_relu through autograd, torch.optim.AdamW / Adadelta with
clip_grad_norm_) and shows that every bar below rejects the usual wrong restatements on the very inputs the GPU test uses.

    utt_norm:   y = (x - mean) * rstd,  rstd = 1 / sqrt(var + eps), var BIASED over the n elements of the utterance
                dx = rstd * (dy - mean(dy) - y * mean(dy * y))          (y as stored by the forward)
    batchnorm:  z = (x - mean) * rstd * gamma + beta over the M rows, var BIASED, running_var updated with the UNBIASED one
                y = keep ? leaky(z) * scale : 0
                g = keep ? dy * leaky'(z) * scale : 0,  dbeta = sum g, dgamma = sum g xhat
                dx = gamma * rstd * (g - sum g / M - xhat * sum g xhat / M)
    clip:       coef = grad_scale * min(1, max_norm / (sqrt(sumsq) * grad_scale + 1e-6))     (coef = grad_scale without a norm)
    adamw:      g' = g coef; m = b1 m + (1 - b1) g'; v = b2 v + (1 - b2) g'^2
                p = p (1 - lr wd) - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),   t 1-based
    adadelta:   g' = g coef + wd p; sq = rho sq + (1 - rho) g'^2; delta = sqrt(acc + eps) / sqrt(sq + eps) * g'   (acc BEFORE its update)
                acc = rho acc + (1 - rho) delta^2;  p = p - lr delta
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

from oracle import dropout_hash as DH
from rowwise_ref import round_bf16, round_f32, round_to  # the one set of storage-rounding helpers of the suite

U = 2.0 ** -24  # fp32 unit roundoff
TINY = 1e-300


def f32(v) -> float:
    """A scalar as the fp32 value the C ABI passes, widened to float64."""
    return float(np.float32(v))


def eps_st(bf16: bool) -> float:
    return 2.0 ** -8 if bf16 else 2.0 ** -22


# ------------------------------------------------------------------------------------------------ utterance normalisation
def utt_norm_fwd(x, eps):
    """x [B, n] -> (y, mean [B], rstd [B]): two-pass biased variance, eps inside the root."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=1)
    var = ((x - mean[:, None]) ** 2).mean(axis=1)
    rstd = 1.0 / np.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None], mean, rstd


def utt_norm_bwd(dy, y, rstd):
    """dx of the header's formula on the STORED y."""
    dy, y = np.asarray(dy, dtype=np.float64), np.asarray(y, dtype=np.float64)
    c1 = dy.mean(axis=1, keepdims=True)
    c2 = (dy * y).mean(axis=1, keepdims=True)
    return np.asarray(rstd, dtype=np.float64)[:, None] * (dy - c1 - y * c2)


# ------------------------------------------------------------------------------------------------ BatchNorm1d + LeakyReLU + dropout
def col_stats(x):
    """(mean, biased variance) of each column, two-pass; M = 1 gives var = 0."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=0)
    return mean, ((x - mean) ** 2).mean(axis=0)


def leaky(z, slope):
    return np.where(z > 0, z, z * slope)


def apply_keep(v, keep, scale):
    return v if keep is None else np.where(keep, v * scale, 0.0)


def batchnorm_act_fwd(x, gamma, beta, run_mean, run_var, momentum, eps, training, slope, keep, scale):
    """Returns (y, mean, rstd, new_run_mean, new_run_var).  Evaluation mode normalises with the running statistics, leaves them
    as they are and applies no dropout."""
    x = np.asarray(x, dtype=np.float64)
    M = x.shape[0]
    gamma, beta = np.asarray(gamma, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    rm = None if run_mean is None else np.asarray(run_mean, dtype=np.float64)
    rv = None if run_var is None else np.asarray(run_var, dtype=np.float64)
    if training:
        mean, var = col_stats(x)
        if rm is not None:
            unb = var * (M / (M - 1.0)) if M > 1 else var
            rm, rv = (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * unb
    else:
        mean, var, keep = rm, rv, None
    rstd = 1.0 / np.sqrt(var + eps)
    y = apply_keep(leaky((x - mean) * rstd * gamma + beta, slope), keep, scale)
    return y, mean, rstd, rm, rv


def batchnorm_act_bwd(dy, x, gamma, beta, mean, rstd, slope, keep, scale, totals=None):
    """Returns (dx, dgamma, dbeta, sum g, sum g xhat) on the saved mean / rstd it is given.  ``totals = (sum g, sum g xhat, rows)``
    replaces the local totals in dx (the synchronised form: global totals over the global row count)."""
    dy, x = np.asarray(dy, dtype=np.float64), np.asarray(x, dtype=np.float64)
    gamma, rstd = np.asarray(gamma, dtype=np.float64), np.asarray(rstd, dtype=np.float64)
    xh = (x - np.asarray(mean, dtype=np.float64)) * rstd
    z = xh * gamma + np.asarray(beta, dtype=np.float64)
    g = apply_keep(np.where(z > 0, dy, dy * slope), keep, scale)
    sg, sgx = g.sum(axis=0), (g * xh).sum(axis=0)
    tg, tgx, rows = (sg, sgx, x.shape[0]) if totals is None else totals
    dx = gamma * rstd * (g - tg / rows - xh * (tgx / rows))
    return dx, sgx, sg, sg, sgx


def batchnorm_sums(x):
    x = np.asarray(x, dtype=np.float64)
    return x.sum(axis=0), (x * x).sum(axis=0), x.shape[0]


# ------------------------------------------------------------------------------------------------ optimizers
def clip_coef(sumsq, max_norm, grad_scale):
    """The header's convention; ``sumsq`` None (no norm buffer) or max_norm <= 0: the gradient scale alone."""
    if sumsq is None or not max_norm > 0:
        return float(grad_scale)
    return float(grad_scale) * min(1.0, float(max_norm) / (math.sqrt(float(sumsq)) * float(grad_scale) + f32(1e-6)))


def adamw_step(p, g, m, v, coef, lr, beta1, beta2, eps, wd, step):
    """Returns (p, m, v); step is 1-based."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    gk = g * coef
    m = beta1 * m + (1.0 - beta1) * gk
    v = beta2 * v + (1.0 - beta2) * gk * gk
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p = p * (1.0 - lr * wd) - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps))
    return p, m, v


def adadelta_step(p, g, sq, acc, coef, lr, rho, eps, wd):
    """Returns (p, sq, acc): torch.optim.Adadelta with coupled weight decay; delta uses acc BEFORE its update."""
    p, g, sq, acc = (np.asarray(a, dtype=np.float64) for a in (p, g, sq, acc))
    gk = g * coef + wd * p
    sq = rho * sq + (1.0 - rho) * gk * gk
    delta = np.sqrt(acc + eps) / np.sqrt(sq + eps) * gk
    return p - lr * delta, sq, rho * acc + (1.0 - rho) * delta * delta


# ------------------------------------------------------------------------------------------------ launch geometry
def cdiv(a, b):
    return -(-a // b)


BN_STAT_THREADS, BN_APPLY_THREADS, BN_ROW_BLOCKS, BN_APPLY_CAP = 1024, 256, 512, 4096
UN_BLOCKS, UN_THREADS, UN_APPLY_CAP = 64, 256, 512
SUMSQ_CAP, ADAMW_CAP, ADADELTA_CAP = 1024, 4096, 2048


def bn_geometry(M, C):
    """sb_head.hip's BnGrid and RowMap in integers: lanes, workgroups, column blocks and loop trips of every BatchNorm pass."""
    cpr = C // 8
    g = SimpleNamespace(cpr=cpr)
    g.cpb_s = min(cpr, BN_STAT_THREADS)
    g.lanes_s = BN_STAT_THREADS // g.cpb_s
    g.idle_s = BN_STAT_THREADS - g.lanes_s * g.cpb_s           # threads with rl == lanes
    g.cb_stat = cdiv(cpr, g.cpb_s)
    g.live_last_s = cpr - (g.cb_stat - 1) * g.cpb_s            # live chunks of the last column block
    g.nb = min(cdiv(M, g.lanes_s), BN_ROW_BLOCKS)
    g.stride_s = g.nb * g.lanes_s
    g.steps_s = min(3, (M - 1) // g.stride_s)                   # highest unrolled step u that loads a row (first trip)
    g.trips4 = cdiv(M, 4 * g.stride_s)                          # loop trips of the 4-row statistics pass (lane of row 0)
    g.trips2 = cdiv(M, 2 * g.stride_s)                          # ... of the 2-row backward partial pass
    g.depth = cdiv(M, g.stride_s) + min(g.lanes_s, M)           # sequential fp32 additions of non-zero terms behind one partial
    g.cpb_a = min(cpr, BN_APPLY_THREADS)
    g.lanes_a = BN_APPLY_THREADS // g.cpb_a
    g.idle_a = BN_APPLY_THREADS - g.lanes_a * g.cpb_a
    g.cb_apply = cdiv(cpr, g.cpb_a)
    g.live_last_a = cpr - (g.cb_apply - 1) * g.cpb_a
    g.ab = max(1, min(BN_APPLY_CAP, cdiv(M, g.lanes_a * 4)))
    g.stride_a = g.ab * g.lanes_a
    g.apply_trips4 = cdiv(M, 4 * g.stride_a)                    # forward apply (4 rows per trip)
    g.apply_trips2 = cdiv(M, 2 * g.stride_a)                    # backward apply (2 rows per trip)
    g.lds_bytes = 8 * g.lanes_s * g.cpb_s * 4
    return g


def un_geometry(n, bf16):
    """Utterance normalisation: vector width, path, loop trips of the partial pass (64 x 256 threads per utterance) and of the apply
    pass (min(512, ceil(n / (256 N))) workgroups), and the sequential fp32 additions behind one partial."""
    N = 8 if bf16 else 4
    g = SimpleNamespace(N=N, vector=n % N == 0)
    items = n // N if g.vector else n
    g.partial_trips = cdiv(items, UN_BLOCKS * UN_THREADS)
    g.ab = min(UN_APPLY_CAP, cdiv(n, UN_THREADS * N))
    g.apply_trips = cdiv(items, g.ab * UN_THREADS)
    g.depth = g.partial_trips * (N if g.vector else 1) + 6 + 4   # per thread, the 64-lane tree, the four waves
    return g


def flat_geometry(n, cap, per_block):
    """sumsq / adamw (float4 body of n / 4 items + a tail in workgroup 0, per_block = 1024) and adadelta (scalar, per_block = 256)."""
    g = SimpleNamespace(blocks=int(min(cap, cdiv(n, per_block))))
    vec = per_block == 1024
    g.items = n // 4 if vec else n
    g.tail = n % 4 if vec else 0
    g.trips = cdiv(g.items, g.blocks * 256)
    g.capped = cdiv(n, per_block) > cap
    return g


# ------------------------------------------------------------------------------------------------ fp32 re-evaluation
def column_sums_fp32(a, b, M, C):
    """The column totals (sum a, sum a b) with the SUMMATION SHAPE of bn_stats_partial_kernel / bn_bwd_partial_kernel re-evaluated
    in numpy fp32: each lane adds its rows in ascending order (s += a; q = fl(q + a b), one rounding as the fma), the lanes of a
    workgroup are added in order, the workgroups' partials in float64.  A second restatement for measuring the constants of the
    bars, not the code under test."""
    g = bn_geometry(M, C)
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    st = g.stride_s
    s, q = np.zeros((st, C), np.float32), np.zeros((st, C), np.float32)
    for r0 in range(0, M, st):
        k = min(st, M - r0)
        s[:k] += a[r0:r0 + k]
        q[:k] = (q[:k].astype(np.float64) + a[r0:r0 + k].astype(np.float64) * b[r0:r0 + k].astype(np.float64)).astype(np.float32)
    s, q = s.reshape(g.nb, g.lanes_s, C), q.reshape(g.nb, g.lanes_s, C)
    ps, pq = np.zeros((g.nb, C), np.float32), np.zeros((g.nb, C), np.float32)
    for l in range(g.lanes_s):
        ps += s[:, l]
        pq += q[:, l]
    return ps.astype(np.float64).sum(axis=0), pq.astype(np.float64).sum(axis=0)


# ------------------------------------------------------------------------------------------------ constants of the bars
# The rigorous bound of a partial sum is depth * u (depth sequential fp32 additions, up to 343 at C = 24); it could not tell a
# variance divided by M - 1 from one divided by M at M = 174 700 (1 / 2M = 48 u), nor a missing row from a rounding error.  The
# roundings of a sequential sum add up like a random walk, sqrt(depth) u, and that is what the fp32 re-evaluation with the
# kernel's summation shape (column_sums_fp32) shows.  Measured by tests/test_headopt_ref.py::test_bn_bars_bite on every
# BatchNorm shape, worst over the columns, in units of u x (sum|terms|  |  |mu| + sigma  |  (var + mu^2) / (var + eps)):
#     (M, C)          depth   column totals   mean    rstd
#     (1030, 24)        342      10.73        0.83    2.84      <- the worst of each: 0.58 sqrt(depth), <= 1 (the fp32 rounding
#     (174700, 24)      343       6.81        0.91    1.91         of the mean itself), 0.154 sqrt(depth)
#     (700, 64)         129       4.78        0.94    1.10
#     (16500, 2056)      14       0.27        0.97    0
#     every other       <= 10    <= 0.20      0.97    0         (the sums of g and g xhat, of mixed sign: below 4 u everywhere)
# The constants are 4 x those laws, and the test asserts 4 x measured <= constant at every shape.
def c_sum(depth):
    return max(4.0, 2.4 * math.sqrt(depth))


def k_stat(depth):
    return max(4.0, 0.7 * math.sqrt(depth))


EPS, MOMENTUM, SLOPE = f32(1e-5), f32(0.1), f32(0.01)
BN_SEED, BN_STREAM = 0x5EED00C0FFEE1234, 7


# ------------------------------------------------------------------------------------------------ BatchNorm inputs and bars
BN_SHAPES = [(1, 8), (5, 8), (1030, 24), (174700, 24), (700, 64), (1497, 1024), (4097, 1024), (513, 8192), (2049, 8192),
             (600, 8200), (16500, 2056)]
BN_DROP_SHAPES = [(5, 8), (1030, 24), (174700, 24), (2049, 8192), (600, 8200)]
BN_CASES = [(M, C, 0.0) for M, C in BN_SHAPES] + [(M, C, 0.15) for M, C in BN_DROP_SHAPES]
BN_SYNC_SHAPES = [(5, 8), (1030, 24), (4097, 1024), (600, 8200)]


def bn_inputs(M, C):
    """x, dy (values bf16 holds, as float64), gamma, beta, running statistics (fp32 values).  Columns cycle through N(0.3, 1.5), a
    constant, N(1e-3, 3e-3) and 8 + k / 16 (|k| <= 6: mean 8, spread 0.25, exact in bf16); gamma is negative on every third column
    and 0 on columns 5, 16, 27, ..; |beta| >= 0.05; dy leans on xhat so that both column totals are far from 0."""
    rng = np.random.default_rng(1000003 * M + C)
    x = rng.standard_normal((M, C)) * 1.5 + 0.3
    c = np.arange(C)
    kind = c % 4
    x[:, kind == 1] = (((c[kind == 1] // 4) % 5) - 2) / 4.0
    n2, n3 = int((kind == 2).sum()), int((kind == 3).sum())
    x[:, kind == 2] = rng.standard_normal((M, n2)) * 3e-3 + 1e-3
    x[:, kind == 3] = 8.0 + rng.integers(-6, 7, (M, n3)) / 16.0
    x = round_bf16(x)
    gamma = 1.0 + 0.3 * rng.standard_normal(C)
    gamma[c % 3 == 1] *= -1.0
    gamma[c % 11 == 5] = 0.0
    beta = np.where(rng.random(C) < 0.5, -1.0, 1.0) * (0.05 + 0.2 * np.abs(rng.standard_normal(C)))
    mean, var = col_stats(x)
    dy = rng.standard_normal((M, C)) + 0.1 + 0.3 * (x - mean) / (np.sqrt(var) + 1e-3)
    return SimpleNamespace(x=x, dy=round_bf16(dy), gamma=round_f32(gamma), beta=round_f32(beta),
                           run_mean=round_f32(0.1 * rng.standard_normal(C)), run_var=round_f32(0.5 + rng.random(C)))


def stat_bars(mean, var, eps, k):
    """(|mean error| bar, relative rstd error bar) of statistics from fp32 partials and float64 totals in the one-pass form
    var = E[x^2] - mean^2: d var <= 2 k u (var + mean^2), d rstd / rstd = d var / (2 (var + eps))."""
    return k * U * (np.abs(mean) + np.sqrt(var)) + TINY, k * U * (var + mean * mean) / (var + eps) + 2 * U


def running_bars(new_rm, new_rv, mean, var, M, momentum, k):
    unb = M / (M - 1.0) if M > 1 else 1.0
    return (U * np.abs(new_rm) + momentum * stat_bars(mean, var, 1.0, k)[0],
            U * np.abs(new_rv) + momentum * unb * 2 * k * U * (var + mean * mean) + TINY)


def bn_y_check(got, x, gamma, beta, mean, rstd, d_mean, d_rstd_rel, slope, keep, scale, bf16=True):
    """Worst (error / bar) of a stored forward output against the float64 composition on (mean, rstd), with the statistics'
    own error bars d_mean (absolute) and d_rstd_rel.  Returns SimpleNamespace(ratio [M, C], ambiguous [M, C], dropped_nonzero)."""
    xh = (x - mean) * rstd
    a = np.abs(xh * gamma)
    z = xh * gamma + beta
    amb = np.abs(z) < 2.0 ** -7 * (a + np.abs(beta))
    floor = (4 * U + d_rstd_rel) * a + 2 * U * np.abs(beta) + rstd * np.abs(gamma) * d_mean
    sc = scale if keep is not None else 1.0
    y_pos, y_neg = z * sc, z * slope * sc
    ref = np.where(z > 0, y_pos, y_neg)
    lk = np.where(z > 0, 1.0, slope)
    err = np.abs(got - ref)
    bar = (eps_st(bf16) + 2 * U) * np.abs(ref) + lk * sc * floor + TINY
    ratio = err / bar
    if amb.any():
        alt = np.where(z > 0, y_neg, y_pos)[amb]
        bar_a = (eps_st(bf16) + 2 * U) * np.maximum(np.abs(ref[amb]), np.abs(alt)) + sc * floor[amb] + TINY
        ratio[amb] = np.minimum(err[amb], np.abs(got[amb] - alt)) / bar_a
    dropped_nonzero = 0
    if keep is not None:
        dropped_nonzero = int((got[~keep] != 0).sum())
        ratio = np.where(keep, ratio, 0.0)
    return SimpleNamespace(ratio=ratio, ambiguous=amb, dropped_nonzero=dropped_nonzero)


def bn_bwd_terms(dy, x, gamma, beta, mean, rstd, slope, keep, scale):
    """The summands of the backward's column totals and what the bars need: g, xhat, sum |g|, sum |g xhat| and the allowance for
    elements whose z the kernel's fp32 evaluation (3 roundings on the saved fp32 statistics) may put on the other side of 0."""
    xh = (x - mean) * rstd
    a = np.abs(xh * gamma)
    z = xh * gamma + beta
    sc = scale if keep is not None else 1.0
    g = apply_keep(np.where(z > 0, dy, dy * slope), keep, scale)
    flip = np.abs(z) <= 4 * U * (a + np.abs(beta))
    fl = np.where(flip, np.abs(dy) * (1.0 - slope) * sc, 0.0)
    if keep is not None:
        fl = np.where(keep, fl, 0.0)
    amb = np.abs(z) < 2.0 ** -7 * (a + np.abs(beta))
    g_alt = apply_keep(np.where(z > 0, dy * slope, dy), keep, scale)
    return SimpleNamespace(g=g, g_alt=g_alt, xh=xh, amb=amb, abs_g=np.abs(g).sum(axis=0), abs_gx=np.abs(g * xh).sum(axis=0),
                           flip_g=fl.sum(axis=0), flip_gx=(fl * np.abs(xh)).sum(axis=0), flips=int(flip.sum()))


def total_bars(t, c):
    """Bars of (sum g, sum g xhat): c u sum|terms| for the fp32 partial sums, 4 u sum|terms| for the roundings inside each term
    (g: two products; g xhat: the subtraction, the product by rstd and the fma), and the flip allowance."""
    return (c + 4) * U * t.abs_g + t.flip_g + TINY, (c + 4) * U * t.abs_gx + t.flip_gx + TINY


def bn_dx_check(got, t, gamma, rstd, tot_g, tot_gx, bar_g, bar_gx, rows, bf16=True):
    """error / bar of a stored dx against gamma rstd (g - c1 - xhat c2), c1 = tot_g / rows, c2 = tot_gx / rows with the totals'
    bars; elements of the 2^-7 set are compared against both LeakyReLU branches."""
    c1, c2 = tot_g / rows, tot_gx / rows
    d1, d2 = bar_g / rows + U * np.abs(c1), bar_gx / rows + U * np.abs(c2)
    gr = np.abs(gamma) * rstd
    tail = d1 + np.abs(t.xh) * d2 + 4 * U * np.abs(t.xh * c2) + 2 * U * np.abs(c1)
    ref = gamma * rstd * (t.g - c1 - t.xh * c2)
    err = np.abs(got - ref)
    ratio = err / ((eps_st(bf16) + 2 * U) * np.abs(ref) + gr * (4 * U * np.abs(t.g) + tail) + TINY)
    if t.amb.any():
        alt = (gamma * rstd * (t.g_alt - c1 - t.xh * c2))[t.amb]
        bar_a = (eps_st(bf16) + 2 * U) * np.maximum(np.abs(ref[t.amb]), np.abs(alt)) \
            + (gr * (4 * U * np.maximum(np.abs(t.g), np.abs(t.g_alt)) + tail))[t.amb] + TINY
        ratio[t.amb] = np.minimum(err[t.amb], np.abs(got[t.amb] - alt)) / bar_a
    return ratio, ref


@functools.lru_cache(maxsize=2)
def bn_case(M, C, p):
    """Inputs and float64 reference of one BatchNorm case, computed once and shared (treat as read-only).  The backward's saved
    statistics are the reference's, rounded to fp32: what the kernel is given, so that forward error does not enter."""
    d = bn_inputs(M, C)
    d.M, d.C, d.p = M, C, p
    depth = bn_geometry(M, C).depth
    d.c_sum, d.k_stat = c_sum(depth), k_stat(depth)
    d.keep = DH.keep_mask(BN_SEED, BN_STREAM, (M, C), p) if p > 0 else None
    d.scale = DH.engine_scale(p)
    d.y, d.mean, d.rstd, d.new_rm, d.new_rv = batchnorm_act_fwd(d.x, d.gamma, d.beta, d.run_mean, d.run_var, MOMENTUM, EPS, True,
                                                                SLOPE, d.keep, d.scale)
    d.var = col_stats(d.x)[1]
    d.mean32, d.rstd32 = round_f32(d.mean), round_f32(d.rstd)
    d.terms = bn_bwd_terms(d.dy, d.x, d.gamma, d.beta, d.mean32, d.rstd32, SLOPE, d.keep, d.scale)
    d.tot_g, d.tot_gx = d.terms.g.sum(axis=0), (d.terms.g * d.terms.xh).sum(axis=0)
    d.bar_g, d.bar_gx = total_bars(d.terms, d.c_sum)
    return d


# ------------------------------------------------------------------------------------------------ utterance-normalisation inputs and bars
def _un_sizes(bf16):
    N, part, app = (8, 131072, 1048576) if bf16 else (4, 65536, 524288)
    return [(3, n) for n in (1, 3, 4, 7, 8, 1003, part + N, part + N + 1)] + [(2, app + N)]


UN_CASES = [(bf, B, n) for bf in (True, False) for B, n in _un_sizes(bf)]


@functools.lru_cache(maxsize=2)
def un_case(bf16, B, n):
    """Utterances: N(0.1, 0.3); the constant 0.5 (var = 0, y = 0); N(-0.2, 0.5) in bf16, mean 30 x std (N(3, 0.1)) in fp32.
    dy = N(0.2, 1) + 0.3 y leans on y, so that mean(dy y) is about 0.3 and not noise of size 1 / sqrt(n)."""
    rng = np.random.default_rng(7919 * n + B + 2 * int(bf16))
    x = rng.standard_normal((B, n)) * 0.3 + 0.1
    x[1] = 0.5
    if B > 2:
        x[2] = rng.standard_normal(n) * 0.5 - 0.2 if bf16 else rng.standard_normal(n) * 0.1 + 3.0
    d = SimpleNamespace(bf16=bf16, B=B, n=n, x=round_to(x, bf16))
    d.y, d.mean, d.rstd = utt_norm_fwd(d.x, EPS)
    d.dy = round_to(rng.standard_normal((B, n)) + 0.2 + 0.3 * d.y, bf16)
    d.var = ((d.x - d.mean[:, None]) ** 2).mean(axis=1)
    d.k = un_geometry(n, bf16).depth + 2
    d.y_st, d.rstd32 = round_to(d.y, bf16), round_f32(d.rstd)      # what the backward kernel is given
    d.dx = utt_norm_bwd(d.dy, d.y_st, d.rstd32)
    return d


def un_y_bar(d):
    """Bar of the stored y: eps_st |y| + (3 u + d rstd) |xhat| + rstd d mean, statistics' bars with k = depth + 2."""
    d_mean, d_rstd = stat_bars(d.mean, d.var, EPS, d.k)
    return (eps_st(d.bf16) + 2 * U) * np.abs(d.y) + (3 * U + d_rstd[:, None]) * np.abs(d.y) + (d.rstd * d_mean)[:, None] + TINY


def un_dx_bar(d):
    """c1 = mean dy and c2 = mean dy y from fp32 partials of `depth` sequential terms: k u mean|terms| each; then three roundings."""
    c1, c2 = d.dy.mean(axis=1, keepdims=True), (d.dy * d.y_st).mean(axis=1, keepdims=True)
    d1 = d.k * U * np.abs(d.dy).mean(axis=1, keepdims=True)
    d2 = d.k * U * np.abs(d.dy * d.y_st).mean(axis=1, keepdims=True)
    rs = d.rstd32[:, None]
    return (eps_st(d.bf16) + 2 * U) * np.abs(d.dx) + rs * (d1 + np.abs(d.y_st) * d2 + 3 * U * (np.abs(d.dy) + np.abs(c1) + np.abs(d.y_st * c2))) + TINY


# ------------------------------------------------------------------------------------------------ optimizer inputs and bars
OPT_SIZES = [1, 3, 4, 5, 1023, 1024, 1027, 262147]
# past the cap of 1024 workgroups: + 3 does not stride yet (n / 4 = 1024 x 256 items), + 7 strides with ONE float4 in the second
# trip, 1 310 723 with 65 536 of them
SUMSQ_SIZES = OPT_SIZES + [1048576 + 3, 1048576 + 7, 1310720 + 3]
ADAMW_SIZES = OPT_SIZES + [4194304 + 5]
ADADELTA_SIZES = OPT_SIZES + [524288 + 1]
GUARD = 8

BETA1, BETA2, ADAM_EPS, RHO, DELTA_EPS = f32(0.9), f32(0.999), f32(1e-8), f32(0.95), f32(1e-8)
WD = f32(0.01)
# the fp32 number next to 1e-3 at which the kernel's fp32 decay = fl(1 - fl(lr wd)) is 1 - lr wd to within 0.01 u (asserted by
# tests/test_headopt_ref.py), so that the 2 u |p| of the bar goes to the two roundings of p decay - update and not to a constant
ADAM_LR = 0.0010013580322265625  # = 0x3A834000 as fp32

# name: (shadow, sumsq or None, max_norm, grad_scale, weight_decay, step)
ADAMW_CONFIGS = {
    "clipped": (True, 9.0, 1.0, 1.0, WD, 2),
    "not_clipped": (True, 0.25, 1.0, 1.0, WD, 2),
    "max_norm0": (True, 9.0, 0.0, 1.0, WD, 2),
    "no_norm": (True, None, 1.0, 1.0, WD, 2),
    "scale_clipped": (True, 64.0, 1.0, 0.25, WD, 2),
    "scale_not_clipped": (True, 9.0, 1.0, 0.25, WD, 2),
    "no_shadow": (False, 9.0, 1.0, 1.0, WD, 2),
    "no_decay": (True, 9.0, 1.0, 1.0, 0.0, 2),
    "step1": (True, 9.0, 1.0, 1.0, WD, 1),
    "step1000": (True, 9.0, 1.0, 1.0, WD, 1000),
}
# name: (shadow, sumsq or None, max_norm, grad_scale, weight_decay)
ADADELTA_CONFIGS = {
    "clipped": (True, 9.0, 1.0, 1.0, 0.0),
    "not_clipped": (True, 0.25, 1.0, 1.0, 0.0),
    "max_norm0": (True, 9.0, 0.0, 1.0, 0.0),
    "no_norm": (True, None, 1.0, 1.0, 0.0),
    "scale_clipped": (True, 64.0, 1.0, 0.25, 0.0),
    "scale_not_clipped": (True, 9.0, 1.0, 0.25, 0.0),
    "no_shadow": (False, 9.0, 1.0, 1.0, 0.0),
    "decay": (True, 9.0, 1.0, 1.0, WD),
}
CONFIG_SIZES = (5, 1027)  # every configuration runs at these; every size runs "clipped"


def opt_cases(sizes, configs):
    """(n, configuration name): "clipped" at every size, every configuration at CONFIG_SIZES, and the two NULL-pointer
    configurations also at n = 3 (tail loop only) and at the last size (the capped, striding grid)."""
    out = []
    for n in sizes:
        for name in configs:
            if name == "clipped" or n in CONFIG_SIZES or (name in ("no_shadow", "no_norm") and n in (3, sizes[-1])):
                out.append((n, name))
    return out


def clip_side(sumsq, max_norm, grad_scale):
    """+1 clipped, -1 not clipped, 0 no clip at all; with the margin to the threshold."""
    if sumsq is None or not max_norm > 0:
        return 0, math.inf
    nrm = math.sqrt(sumsq) * grad_scale
    return (1 if nrm > max_norm else -1), abs(nrm / max_norm - 1.0)


@functools.lru_cache(maxsize=4)
def opt_inputs(n):
    """fp32 values (as float64): p ~ N(0, 1); g ~ N(0, 1e-2) with every 7th exactly 0; m with the sign of g (no cancellation in
    b1 m + (1 - b1) g', so the update's bar is relative to the update itself) and |m| ~ 1e-2; v ~ g^2-sized, 0 on every 5th element
    and 1e-20 on every 11th (eps decides the denominator there, with g = 0 on every 35th and 77th); Adadelta's sq like v and
    acc ~ 1e-6, 0 on every 5th; the tail elements (n % 4) of g are never 0."""
    rng = np.random.default_rng(n)
    i = np.arange(n)
    g = rng.standard_normal(n) * 1e-2
    g[i % 7 == 0] = 0.0
    g[(i >= n - n % 4) & (g == 0)] = 3e-3
    sgn = np.where(g != 0, np.sign(g), np.where(rng.random(n) < 0.5, -1.0, 1.0))
    m = sgn * (1e-3 + 1e-2 * np.abs(rng.standard_normal(n)))
    v = (1e-2 * rng.standard_normal(n)) ** 2 + 1e-7
    v[i % 5 == 0] = 0.0
    v[i % 11 == 0] = 1e-20
    acc = 1e-6 * (0.5 + rng.random(n))
    acc[i % 5 == 0] = 0.0
    p = sgn * (0.05 + np.abs(rng.standard_normal(n)))  # (with the sign of g: Adadelta's g' = g coef + wd p does not cancel either)
    return SimpleNamespace(n=n, p=round_f32(p), g=round_f32(g), m=round_f32(m), v=round_f32(v), acc=round_f32(acc))


def c_bc(step):
    """Relative error of the kernel's update in units of u.  powf is within 1 ulp (<= 2 u b^t absolute), so
    bc1 = 1 - b1^t carries 2 b1^t / (1 - b1^t) + 1 and sqrt(bc2) half of 2 b2^t / (1 - b2^t) + 1, plus 1.  The rest: coef 5 (sqrt,
    two products, sum, quotient), g' 1, m 2 more (8 in all), v 16 and its root 9, the quotient by sqrt(bc2) 1, + eps 1, m / denom
    1, lr / bc1 1, their product 1: 32 with the two ones above."""
    b1, b2 = BETA1 ** step, BETA2 ** step
    return 32.0 + 2.0 * b1 / (1.0 - b1) + b2 / (1.0 - b2)


def adamw_reference(n, cfg):
    shadow, sumsq, max_norm, gs, wd, step = cfg
    d = opt_inputs(n)
    coef = clip_coef(sumsq, f32(max_norm), f32(gs))
    p, m, v = adamw_step(d.p, d.g, d.m, d.v, coef, ADAM_LR, BETA1, BETA2, ADAM_EPS, f32(wd), step)
    upd = np.abs(p - (1.0 - ADAM_LR * f32(wd)) * d.p)
    return SimpleNamespace(p=p, m=m, v=v, upd=upd, p_bar=2 * U * np.abs(p) + c_bc(step) * U * upd + TINY, m_bar=8 * U * np.abs(m) + TINY,
                           v_bar=16 * U * np.abs(v) + TINY)


def adadelta_reference(n, cfg):
    """Bars, in the AdamW structure: g' carries 7 u (coef 5, two roundings), sq 18 u, delta 24 u (two roots of sums, a quotient,
    the product with g'), acc 2 x 24 + 4 = 52 u on its delta^2 part -- 56 u of acc; p within 2 u |p| + 26 u |lr delta|."""
    shadow, sumsq, max_norm, gs, wd = cfg
    d = opt_inputs(n)
    coef = clip_coef(sumsq, f32(max_norm), f32(gs))
    p, sq, acc = adadelta_step(d.p, d.g, d.v, d.acc, coef, 1.0, RHO, DELTA_EPS, f32(wd))
    upd = np.abs(p - d.p)
    return SimpleNamespace(p=p, sq=sq, acc=acc, upd=upd, p_bar=2 * U * np.abs(p) + 26 * U * upd + TINY, sq_bar=18 * U * np.abs(sq) + TINY,
                           acc_bar=56 * U * np.abs(acc) + TINY)


# Roundings on the longest path from one g to the result: its square 1, the three additions of a float4's squares 3, s += of its
# own trip and of the second trip 2, the tail element of workgroup 0 added last 1, the 64-lane tree 6, the four waves 4, the final
# pass over the 1024 partials 6 + 16: 39.  The bar is 42 u sum g^2 (3 u for the second-order terms).
SUMSQ_ROUNDINGS = 1 + 3 + 2 + 1 + (6 + 4) + (6 + 16)
SUMSQ_BAR_U = 42.0
PROBE = np.array([4.0, -4.0, 4.0, -4.0])


@functools.lru_cache(maxsize=4)
def sumsq_inputs(n):
    """g ~ N(0, 1) in fp32.  The n % 4 tail elements are +-4, and so are, at the sizes past the grid cap, the float4 g[4:8] and the
    FIRST float4 of the second loop trip (item 1024 x 256): each of them is 16 or 64 against a bar of 42 u sum g^2 <= 3.3, so a
    kernel that loses the tail, a float4 or the second trip misses the bar.  ``second`` is the element range of the second trip."""
    rng = np.random.default_rng(n + 17)
    g = rng.standard_normal(n)
    if n % 4:
        g[n - n % 4:] = PROBE[:n % 4]
    geo = flat_geometry(n, SUMSQ_CAP, 1024)
    second = (4 * geo.blocks * 256, 4 * geo.items) if geo.trips > 1 else None
    if geo.capped:
        g[4:8] = PROBE
        if second:
            g[second[0]:second[0] + 4] = PROBE
    g = round_f32(g)
    ref = float((g * g).sum())
    return SimpleNamespace(g=g, ref=ref, bar=SUMSQ_BAR_U * U * ref, second=second)
