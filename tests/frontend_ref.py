"""Float64 restatement of the kernels that run only when the feature encoder trains (ssak_amd/csrc/conv_frontend.hip: the
conv0 + GroupNorm + GELU backward, the conv0 weight gradient, conv0 + bias, col2im, the slab sum and the weight re-layouts) and
of the data movers of the Whisper front end (whisper_frontend.hip: col2im of the k = 3, s = 2, pad = 1 convolution fused with
GELU', mel -> channels-last, the position add, the padded row copy, the weight-gradient un-rearrangement).

Written from the definitions in numpy, not from the kernels' loops.  ``tests/test_frontend_ref.py`` pins every function to torch
under float64 autograd (or to plain indexing); ``tests/test_gpu_frontend.py`` holds the kernels to it.

conv0 = Conv1d(1, C, k = 10, stride 5, no bias), x [B, T] -> v [B, T0, C], T0 = (T - 10) / 5 + 1; GroupNorm with one group per
channel (statistics over t per (b, c)), then GELU::

    v = conv1d(x, w);  mean, var over t;  rstd = 1 / sqrt(max(var, 0) + 1e-5);  xh = (v - mean) rstd;  z = gamma xh + beta
    g = dy gelu'(z);   dbeta = sum_{b,t} g;   dgamma = sum_{b,t} g xh
    dv = gamma rstd (g - mean_t g - xh mean_t(g xh));   dw[c][k] = sum_{b,t} dv x[b, 5 t + k]

gelu' is the exact form for fp32 storage and the logistic fit of common.h for bf16 (rowwise_ref.gelu_forms).

The fp32 emulations (``emulate_*``) restate the ORDER in which the kernels add, every operation rounded to fp32; they are what the
accumulation constants at the end of the module are derived from.  A fused multiply-add is emulated as the fp32 rounding of the
float64 a b + c (the product of two fp32 numbers is exact in float64; the double rounding of the sum is immaterial here).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowwise_ref as RR  # noqa: E402

F64, F32 = np.float64, np.float32
U = 2.0 ** -24
KS0, ST0 = 10, 5
FR_STATS = 1024          # frames per workgroup of conv0_bwd_kernel
C0W_BLOCKS = 32          # workgroups per utterance of conv0_wgrad_kernel
GELU_CURVATURE = 0.7979  # sup |gelu''| = sqrt(2 / pi), rounded up (tests/posconv_ref.py)


def gelu_grad_bar(bf16: bool) -> float:
    """The error of the kernels' gelu' as tests/test_gpu_rowwise.py states and tests it: the bf16 engine's logistic fit against
    the exact form, the fp32 mode's erff form."""
    return RR.PHI_FIT_MAX_ERR + 2.0 ** -20 if bf16 else 1e-6


# ------------------------------------------------------------------------------------------------ conv0 and its backward
def windows(x, k=KS0, s=ST0):
    """x [B, T] -> [B, T0, k]: frame t holds x[b, s t : s t + k] (a view)."""
    return np.lib.stride_tricks.sliding_window_view(np.asarray(x, dtype=F64), k, axis=1)[:, ::s]


def conv0(x, w, bias=None, k=KS0, s=ST0):
    """[B, T0, C] = conv1d(x, w) (+ bias)."""
    v = windows(x, k, s) @ np.asarray(w, dtype=F64).T
    return v if bias is None else v + np.asarray(bias, dtype=F64)


def conv0_abs_sum(x, w, bias=None, k=KS0, s=ST0):
    a = np.abs(windows(x, k, s)) @ np.abs(np.asarray(w, dtype=F64)).T
    return a if bias is None else a + np.abs(np.asarray(bias, dtype=F64))


def conv0_stats(v):
    """(mean, rstd) [B, C] of v [B, T0, C] over t, the variance biased and centred."""
    mean = v.mean(axis=1)
    var = ((v - mean[:, None]) ** 2).mean(axis=1)
    return mean, 1.0 / np.sqrt(np.maximum(var, 0.0) + 1e-5)


def conv0_bwd(x, w, gamma, beta, dy, bf16: bool, stats=None):
    """The backward of gelu(GroupNorm(conv0(x)) gamma + beta) from dy [B, T0, C]; stats = (mean, rstd) [B, C] to use instead of
    the reference's own.  Returns the gradients and every intermediate the bars and the emulations need."""
    w, gamma, beta, dy = (np.asarray(a, dtype=F64) for a in (w, gamma, beta, dy))
    win = windows(x)
    v = win @ w.T
    mean, rstd = conv0_stats(v) if stats is None else (np.asarray(s, dtype=F64) for s in stats)
    xh = (v - mean[:, None]) * rstd[:, None]
    z = gamma * xh + beta
    g = dy * RR.gelu_forms(bf16)[1](z)
    m1, m2 = g.mean(axis=1), (g * xh).mean(axis=1)
    dv = gamma * rstd[:, None] * (g - m1[:, None] - xh * m2[:, None])
    dw = np.einsum("btc,btk->ck", dv, win)
    return dict(win=win, v=v, mean=mean, rstd=rstd, xh=xh, z=z, g=g, m1=m1, m2=m2, dv=dv, dy=dy, w=w, gamma=gamma,
                dbeta=g.sum(axis=(0, 1)), dgamma=(g * xh).sum(axis=(0, 1)), dw=dw)


def conv0_bwd_bars(p, bf16: bool):
    """Bars of dbeta, dgamma [C] and dw [C, 10] (without the 2^-23 (|start| + |ref|) of the accumulation onto the caller's values),
    from per-element bounds summed over the reduction.  With S = sum_k |w_k x_k|:

        d_xh = C_XHAT u (S + |mean|) rstd + 2 u |xh|          the kernel's xh: fp32 dot product, float-cast mean and rstd
        d_z  = |gamma| d_xh + u (|gamma xh| + |z|)             the affine in fp32
        d_g  = |dy| (0.7979 d_z + E_gelu') + u |g|             gelu' moves by at most sup |gelu''| d_z; E_gelu' as test_gpu_rowwise.py
        dbeta  <= C_GSUM u sum |g|    + sum d_g
        dgamma <= C_GSUM u sum |g xh| + sum (d_g |xh| + |g| d_xh)
        d_m1 = (C_GSUM u sum_t |g| + sum_t d_g) / T0 + u |m1|,   d_m2 likewise with g xh
        d_dv = |gamma| rstd (d_g + d_m1 + |xh| d_m2 + d_xh |m2|) + 4 u |gamma| rstd (|g| + |m1| + |xh m2|)
        dw   <= C_DW u sum |dv x_k| + sum d_dv |x_k|
    """
    aw = np.abs(p["win"])
    T0 = aw.shape[1]
    ag, axh, agam = np.abs(p["g"]), np.abs(p["xh"]), np.abs(p["gamma"])
    rstd, am1, am2 = p["rstd"][:, None], np.abs(p["m1"])[:, None], np.abs(p["m2"])[:, None]
    S = aw @ np.abs(p["w"]).T
    d_xh = C_XHAT * U * (S + np.abs(p["mean"])[:, None]) * rstd + 2 * U * axh
    d_z = agam * d_xh + U * (agam * axh + np.abs(p["z"]))
    d_g = np.abs(p["dy"]) * (GELU_CURVATURE * d_z + gelu_grad_bar(bf16)) + U * ag
    t_gx = d_g * axh + ag * d_xh
    d_m1 = (C_GSUM * U * ag.sum(axis=1) + d_g.sum(axis=1)) [:, None] / T0 + U * am1
    d_m2 = (C_GSUM * U * (ag * axh).sum(axis=1) + t_gx.sum(axis=1))[:, None] / T0 + U * am2
    d_dv = agam * rstd * (d_g + d_m1 + axh * d_m2 + d_xh * am2) + 4 * U * agam * rstd * (ag + am1 + axh * am2)
    return dict(dbeta=C_GSUM * U * ag.sum(axis=(0, 1)) + d_g.sum(axis=(0, 1)),
                dgamma=C_GSUM * U * (ag * axh).sum(axis=(0, 1)) + t_gx.sum(axis=(0, 1)),
                dw=C_DW * U * np.einsum("btc,btk->ck", np.abs(p["dv"]), aw) + np.einsum("btc,btk->ck", d_dv, aw))


def conv0_wgrad(d, x, k=KS0, s=ST0):
    """dw [C, k] = sum_{b,t} d[b, t, c] x[b, s t + k]."""
    return np.einsum("btc,btk->ck", np.asarray(d, dtype=F64), windows(x, k, s))


def conv0_wgrad_abs_sum(d, x, k=KS0, s=ST0):
    return np.einsum("btc,btk->ck", np.abs(np.asarray(d, dtype=F64)), np.abs(windows(x, k, s)))


# ------------------------------------------------------------------------------------------------ col2im
def col2im(dxcol, Tin: int, s: int):
    """dxcol [B, Tout, k, C] -> dx [B, Tin, C]: dxcol[b, t, kk] is added into row t s + kk; rows no window reaches stay zero."""
    dxcol = np.asarray(dxcol, dtype=F64)
    B, Tout, k, C = dxcol.shape
    assert (Tout - 1) * s + k <= Tin
    dx = np.zeros((B, Tin, C), dtype=F64)
    for kk in range(k):
        dx[:, kk:kk + (Tout - 1) * s + 1:s] += dxcol[:, :, kk]
    return dx


def col2im_k3s2(dxcol, pre, Tin: int, RS1: int, bf16: bool):
    """Input gradient of Conv1d(k = 3, stride 2, padding 1): dxcol [B, F, 3, H] is added into row 2 t + kk - 1 where that lies in
    [0, Tin), then multiplied by gelu'(pre), pre [B, Tin, H].  Returns (out [B, RS1, H] with rows >= Tin zero, the sum before
    the multiplication, sum |terms|, gelu'(pre)), the last three [B, Tin, H]."""
    dxcol, pre = np.asarray(dxcol, dtype=F64), np.asarray(pre, dtype=F64)
    B, Fr, k, H = dxcol.shape
    assert k == 3 and Fr == (Tin + 2 - 3) // 2 + 1
    acc, aacc = np.zeros((B, Tin + 2, H), dtype=F64), np.zeros((B, Tin + 2, H), dtype=F64)  # row u + 1: the padded input
    for kk in range(3):
        acc[:, kk:kk + 2 * (Fr - 1) + 1:2] += dxcol[:, :, kk]
        aacc[:, kk:kk + 2 * (Fr - 1) + 1:2] += np.abs(dxcol[:, :, kk])
    acc, aacc = acc[:, 1:Tin + 1], aacc[:, 1:Tin + 1]
    gp = RR.gelu_forms(bf16)[1](pre)
    out = np.zeros((B, RS1, H), dtype=F64)
    out[:, :Tin] = acc * gp
    return out, acc, aacc, gp


def pre_with_lead(pre, RS1: int, fill: float):
    """pre [B, Tin, H] -> the buffer [B * RS1, H] the kernel reads: row u of utterance b at row b RS1 + 1 + u, `fill` elsewhere."""
    B, Tin, H = pre.shape
    buf = np.full((B * RS1, H), fill, dtype=F64)
    for b in range(B):
        buf[b * RS1 + 1:b * RS1 + 1 + Tin] = pre[b]
    return buf


# ------------------------------------------------------------------------------------------------ the movers
def mel_to_cl(mel, cl, RS: int, lead: int):
    """mel [B, C, T] -> a copy of cl [rows, C] with row b RS + lead + t = mel[b, :, t]."""
    out = np.array(cl, dtype=F64)
    B, C, T = mel.shape
    for b in range(B):
        out[b * RS + lead:b * RS + lead + T] = np.asarray(mel[b], dtype=F64).T
    return out


def add_rowvec(x, pos):
    return np.asarray(x, dtype=F64) + np.asarray(pos, dtype=F64)[None]


def copy_rows_padded(src, RS: int):
    B, Fr, H = src.shape
    out = np.zeros((B, RS, H), dtype=F64)
    out[:, :Fr] = src
    return out


def weight_rearrange(w):
    """w [Co, Ci, k] -> [Co, k, Ci]."""
    return np.ascontiguousarray(np.asarray(w, dtype=F64).transpose(0, 2, 1))


def wgrad_unrearrange(dwr, g):
    """g [Co, Ci, k] + dwr [Co, k, Ci] transposed back."""
    return np.asarray(g, dtype=F64) + np.asarray(dwr, dtype=F64).transpose(0, 2, 1)


def sum_slabs(slabs):
    return np.asarray(slabs, dtype=F64).sum(axis=0)


# ------------------------------------------------------------------------------------------------ fp32 emulations of the ORDER
def _fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _seq_sum(x, axis=0):
    """Left-to-right fp32 sum."""
    x = np.moveaxis(x.astype(F32), axis, 0)
    s = np.zeros_like(x[0])
    for i in range(x.shape[0]):
        s = s + x[i]
    return s


def emulate_sum_slabs(slabs):
    """s = 0; s += slabs[b] for b = 0 .. nb - 1, in fp32."""
    return _seq_sum(slabs)


def emulate_dot(win, w, start=None):
    """a = start (0); a = fma(w[c][k], x[k], a) for k = 0 .. 9: the kernels' 10-tap chain.  -> [B, T0, C] fp32."""
    win, w = win.astype(F32), np.asarray(w).astype(F32)
    a = np.zeros(win.shape[:2] + (w.shape[0],), dtype=F32) if start is None else np.broadcast_to(
        np.asarray(start).astype(F32), win.shape[:2] + (w.shape[0],)).copy()
    for k in range(w.shape[1]):
        a = _fma(w[None, None, :, k], win[:, :, k, None], a)
    return a


def emulate_xhat(p):
    """(fma chain - float(mean)) * float(rstd), each operation in fp32."""
    v = emulate_dot(p["win"], p["w"])
    return (v - p["mean"].astype(F32)[:, None]) * p["rstd"].astype(F32)[:, None]


def _lane_chains(a, b, fl: int):
    """One workgroup of conv0_bwd_kernel: a [nfr, C, ...] (and b, broadcastable, or None) -> [C, ...] fp32.  Thread (q, fli) runs
    acc = fma(a[f], b[f], acc) (acc += a[f] without b) over its frames f = fli, fli + fl, ...; the fl partials are then added left
    to right.  (Frames past nfr are padded with zeros, which change nothing.)"""
    if b is not None:
        a, b = np.broadcast_arrays(a, b)
    nfr = a.shape[0]
    steps = -(-nfr // fl)
    pad = [(0, steps * fl - nfr)] + [(0, 0)] * (a.ndim - 1)
    a = np.pad(a.astype(F32), pad).reshape((steps, fl) + a.shape[1:])
    if b is not None:
        b = np.pad(b.astype(F32), pad).reshape(a.shape)
    acc = np.zeros(a.shape[1:], dtype=F32)
    for i in range(steps):
        acc = acc + a[i] if b is None else _fma(a[i], b[i], acc)
    return _seq_sum(acc)


def emulate_conv0_bwd_sums(p):
    """dbeta, dgamma, dw as conv0_bwd_kernel<0 / 1> and their second stages order the additions, fed the float64 reference's g,
    xh, dv and x rounded to fp32: per-thread chains and the fl partials in fp32, the workgroups of an utterance in double (g, g xh)
    and the utterances in double, cast to fp32 at the end; dw: the (b, workgroup) slabs left to right in fp32."""
    B, T0, C = p["g"].shape
    fl = 256 // (C // 4)
    nblk = -(-T0 // FR_STATS)
    gs, gx = np.zeros((B, C), dtype=F64), np.zeros((B, C), dtype=F64)
    dw = np.zeros((C, KS0), dtype=F32)
    for b in range(B):
        for blk in range(nblk):
            sl = slice(blk * FR_STATS, min(T0, (blk + 1) * FR_STATS))
            g, xh = p["g"][b, sl], p["xh"][b, sl]
            gs[b] += _lane_chains(g, None, fl).astype(F64)
            gx[b] += _lane_chains(g, xh, fl).astype(F64)
            dw = dw + _lane_chains(p["dv"][b, sl, :, None], p["win"][b, sl, None, :], fl)
    return gs.sum(axis=0).astype(F32), gx.sum(axis=0).astype(F32), dw


def emulate_conv0_wgrad(d, x, k=KS0, s=ST0):
    """conv0_wgrad_kernel + conv0_wgrad_sum_kernel: each of the 32 workgroups of an utterance runs one fma chain per (c, tap) over
    its ceil(T0 / 32) frames (64-frame chunks only restage the samples: the accumulators live across them); the 32 B slabs are then
    added left to right in fp32."""
    win = windows(x, k, s).astype(F32)
    d = np.asarray(d).astype(F32)
    B, T0, C = d.shape
    per = -(-T0 // C0W_BLOCKS)
    pad = C0W_BLOCKS * per - T0
    dd = np.pad(d, [(0, 0), (0, pad), (0, 0)]).reshape(B, C0W_BLOCKS, per, C)
    ww = np.pad(win, [(0, 0), (0, pad), (0, 0)]).reshape(B, C0W_BLOCKS, per, k)
    acc = np.zeros((B, C0W_BLOCKS, C, k), dtype=F32)
    for t in range(per):
        acc = _fma(dd[:, :, t, :, None], ww[:, :, t, None, :], acc)
    return _seq_sum(acc.reshape(B * C0W_BLOCKS, C, k))


# ------------------------------------------------------------------------------------------------ seeded test data
def _edges(n: int, B: int):
    """1 everywhere, 8 on the first and last 64 positions when the batch has more than one utterance: a read across an
    utterance boundary then moves a result by many bars."""
    e = np.ones(n)
    if B >= 2:
        e[:64] = 8.0
        e[-64:] = 8.0
    return e


def conv0_bwd_case(C: int, T0: int, r: int, B: int, bf16: bool):
    """x ~ N(0, 1), w ~ 0.3 N(0, 1), gamma = 1 + 0.1 N, beta = 0.1 N as fp32 values; dy ~ N(0, 1) rounded to the storage type;
    T = 5 (T0 - 1) + 10 + r."""
    T = ST0 * (T0 - 1) + KS0 + r
    rng = np.random.default_rng(1000 * C + 10 * T0 + r + 7 * B + (1 if bf16 else 0))
    f = lambda a: a.astype(F32).astype(F64)
    return dict(x=f(rng.standard_normal((B, T)) * _edges(T, B)), w=f(0.3 * rng.standard_normal((C, KS0))),
                gamma=f(1.0 + 0.1 * rng.standard_normal(C)), beta=f(0.1 * rng.standard_normal(C)),
                dy=RR.round_to(rng.standard_normal((B, T0, C)) * _edges(T0, B)[None, :, None], bf16))


def conv0_wgrad_case(C: int, T0: int, B: int, k: int, s: int, bf16: bool, integer: bool):
    T = s * (T0 - 1) + k + (T0 % 3)  # (0 .. 2 trailing samples that belong to no frame)
    rng = np.random.default_rng(2000 * C + 10 * T0 + 7 * B + k + (1 if bf16 else 0))
    if integer:
        return dict(x=rng.integers(-3, 4, (B, T)).astype(F64), d=rng.integers(-2, 3, (B, T0, C)).astype(F64))
    return dict(x=(rng.standard_normal((B, T)) * _edges(T, B)).astype(F32).astype(F64),
                d=RR.round_to(rng.standard_normal((B, T0, C)) * _edges(T0, B)[None, :, None], bf16))


def col2im_case(k: int, s: int, C: int, Tout: int, r: int, B: int, bf16: bool, integer: bool):
    rng = np.random.default_rng(3000 * k + 100 * s + C + 10 * Tout + r + 7 * B + (1 if bf16 else 0))
    if integer:
        return rng.integers(-3, 4, (B, Tout, k, C)).astype(F64)
    return RR.round_to(rng.standard_normal((B, Tout, k, C)) * _edges(Tout, B)[None, :, None, None], bf16)


def col2im_k3s2_case(H: int, Tin: int, B: int, bf16: bool):
    """(dxcol [B, F, 3, H], pre [B, Tin, H]) rounded to the storage type; pre ~ 1.5 N(0, 1) so that gelu' covers its range."""
    Fr = (Tin + 1) // 2
    rng = np.random.default_rng(4000 * H + 10 * Tin + 7 * B + (1 if bf16 else 0))
    return (RR.round_to(rng.standard_normal((B, Fr, 3, H)) * _edges(Fr, B)[None, :, None, None], bf16),
            RR.round_to(1.5 * rng.standard_normal((B, Tin, H)), bf16))


def start_values(seed: int, *shapes):
    """Non-zero fp32 starting values ~ N(0, 1) of the accumulated outputs."""
    rng = np.random.default_rng(9000 + seed)
    return [rng.standard_normal(sh).astype(F32).astype(F64) for sh in shapes]


def conv0_bias_case(C: int, T0: int, B: int, integer: bool):
    T = ST0 * (T0 - 1) + KS0 + (T0 % 5)
    rng = np.random.default_rng(6000 * C + 10 * T0 + B)
    if integer:
        return dict(x=rng.integers(-3, 4, (B, T)).astype(F64), w=rng.integers(-2, 3, (C, KS0)).astype(F64),
                    bias=rng.integers(-3, 4, C).astype(F64))
    f = lambda a: a.astype(F32).astype(F64)
    return dict(x=f(rng.standard_normal((B, T)) * _edges(T, B)), w=f(0.3 * rng.standard_normal((C, KS0))),
                bias=f(0.1 * rng.standard_normal(C)))


def slabs_case(nb: int, n: int, integer: bool):
    rng = np.random.default_rng(5000 + nb + n)
    if integer:
        return rng.integers(-1000, 1001, (nb, n)).astype(F64)
    return rng.standard_normal((nb, n)).astype(F32).astype(F64)


# the shapes of tests/test_gpu_frontend.py (C, T0, r, B): C = 512 with every T0; every C and every T0 at both storage types
CONV0_BWD_T0 = (1, 2, 129, 1023, 1024, 1025, 2049)
CONV0_BWD_SHAPES = ((512, 1, 0, 3), (512, 2, 4, 1), (512, 129, 0, 3), (512, 1023, 4, 1), (512, 1024, 0, 3), (512, 1025, 4, 3),
                    (512, 2049, 0, 3),
                    (64, 2, 0, 3), (64, 1025, 4, 1), (64, 2049, 0, 3),
                    (1024, 1, 4, 1), (1024, 1024, 4, 3), (1024, 2049, 0, 1),
                    (8, 129, 4, 3), (8, 1023, 0, 1), (8, 2049, 4, 3))
# (C, T0, B, k, s)
CONV0_WGRAD_SHAPES = ((512, 1, 1, 10, 5), (512, 31, 3, 10, 5), (512, 33, 1, 10, 5), (512, 1599, 3, 10, 5), (512, 2048, 1, 10, 5),
                      (512, 2049, 3, 10, 5), (64, 1, 3, 10, 5), (64, 33, 3, 10, 5), (64, 1599, 1, 10, 5), (64, 2049, 1, 10, 5),
                      (2, 31, 1, 10, 5), (2, 2048, 3, 10, 5), (2, 2049, 3, 10, 5), (64, 2049, 3, 4, 3))
CONV0_BIAS_SHAPES = tuple((C, T0, B) for C in (512, 64) for T0, B in ((1, 3), (127, 1), (128, 3), (129, 3), (400, 1)))


def _pow2_ceil(x: float) -> float:
    return 2.0 ** math.ceil(math.log2(x))


# ------------------------------------------------------------------------------------------------ accumulation constants
# Each constant C of a bar  C u sum |terms|  is 4 x (the worst |fp32-order emulation - float64| / (u sum |terms|)) over ALL
# real-valued cases of the GPU module (every shape of CONV0_BWD_SHAPES, CONV0_WGRAD_SHAPES and CONV0_BIAS_SHAPES, both storage
# types, same seeds; tests/test_frontend_ref.py::test_accumulation_constants measures the ratios again and holds the constants to
# this rule), rounded up to a power of two.  The 4 covers the compiler's freedom to contract and reassociate within a thread;
# these are plain fma chains of known order (no matrix instructions).  Measured (the worst case of the sums is C = 1024, T0 = 1024,
# B = 3: one thread then adds all 1024 frames of a channel in one chain, the 8 x larger edge frames first):
#   xh = (dot - float(mean)) float(rstd), in units of u (S + |mean|) rstd after 2 u |xh| is taken off:  3.7480 -> 15.0 -> C_XHAT = 16
#   sum g, sum g xh (conv0_bwd_kernel<0>, gsums, affine):                                                9.8111 -> 39.2 -> C_GSUM = 64
#   dw of the conv0 backward (conv0_bwd_kernel<1>, dw):                                                  7.4204 -> 29.7 -> C_DW = 32
#   dw of conv0_wgrad_kernel + conv0_wgrad_sum_kernel:                                                   3.3346 -> 13.3 -> C_WGRAD = 16
#   conv0 + bias (the 10-tap chain started from the bias):                                               3.7239 -> 14.9 -> C_BIAS = 16
MEASURED = dict(xhat=3.7480, gsum=9.8111, dw=7.4204, wgrad=3.3346, bias=3.7239)
C_XHAT = 16.0
C_GSUM = 64.0
C_DW = 32.0
C_WGRAD = 16.0
C_BIAS = 16.0
