"""Float64 numpy restatement of the row kernels of ssak_amd/csrc/norm_act.hip (LayerNorm forward / backward with their fused
residual, dropout sites, post-GELU and column sums; the attention softmax forward / backward; the GELU forms of common.h).

Written from what the kernels define, not from what they compute: every value is float64, dropout masks come from
``oracle.dropout_hash.keep_mask`` and scales from ``engine_scale``.  ``tests/test_rowwise_ref.py`` checks the backward here
against torch float64 autograd of the same composition (so the reference is right independently of the kernels), and
``tests/test_gpu_rowwise.py`` holds the kernels to it.

LayerNorm forward (``k_layernorm_fwd_t``)::

    r   = mid(res + pre(y))                      rounded to the storage type when r_out is stored
    out = post(gelu?((r - mean) * rstd * gamma + beta)),   rstd = 1 / sqrt(var + eps), var BIASED (divided by C)

LayerNorm backward (``k_layernorm_bwd_t``), on the saved r / mean / rstd::

    a  = post(g1 + g2) [* gelu'(xhat * gamma + beta)]       xhat = (r - mean) * rstd
    dgamma += sum_rows a * xhat,  dbeta += sum_rows a
    dr = mid(rstd * (a gamma - mean(a gamma) - xhat * mean(a gamma xhat)) + g_res)      (g_res BEFORE the sum-dropout replay)
    dy = pre(dr),  dy_colsum += sum_rows dy

where site(v) = v * scale where the site keeps, 0 where it drops (the backward replays the forward's masks).
"""
from __future__ import annotations

import numpy as np
from scipy.special import erf

from oracle import dropout_hash as DH

# the specialised instantiations of norm_act.hip's dispatchers (bf16, C = 768 / 1024): bit sets of LN_FWD_SPEC(..) /
# LN_BWD_SPEC(..).  tests/test_rowwise_ref.py parses the source and asserts that these are exactly its lists.
LN_FWD_SPECS = (1, 2, 35, 39, 17, 18, 43, 47, 42)
LN_BWD_SPECS = (0, 16, 32, 48, 1, 17, 33, 49, 3, 19, 35, 51, 8, 24, 36, 52)
# forward bits: 1 y, 2 res, 4 pre-, 8 sum-, 16 post-dropout, 32 r_out;  backward: 1 dy, 2 pre-, 4 sum-, 8 post-dropout, 16 g2, 32 g_res
FWD_Y, FWD_RES, FWD_PRE, FWD_MID, FWD_POST, FWD_ROUT = 1, 2, 4, 8, 16, 32
BWD_DY, BWD_PRE, BWD_MID, BWD_POST, BWD_G2, BWD_GRES = 1, 2, 4, 8, 16, 32

# common.h SSAK_PHI_C0..C3: the bf16 GELU's logistic fit, Phi(x) ~ 1 / (1 + 2^(x (c0 + c1 x^2 + c2 x^4 + c3 x^6))), |x| <= 6
PHI_C = (-2.302147388458252, -0.10512793809175491, 0.00039503577863797545, 5.9617443184833974e-05)
PHI_FIT_MAX_ERR = 1.65e-5  # what common.h claims for max |Phi_fit - Phi| over the real line (fp32 evaluation included)


# ------------------------------------------------------------------------------------------------ storage types
def round_bf16(x) -> np.ndarray:
    """x -> fp32 -> bf16 (round to nearest even), as float64: what a kernel's fp32 value becomes when stored as bf16."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def round_f32(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def round_to(x, bf16: bool) -> np.ndarray:
    return round_bf16(x) if bf16 else round_f32(x)


def bf16_ulp(x) -> np.ndarray:
    """The spacing of bf16 numbers at |x| (8 significant bits): 2^(floor(log2 |x|) - 7); that of the smallest normal at 0."""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), np.finfo(np.float32).tiny)
    return np.exp2(np.floor(np.log2(a)) - 7)


# ------------------------------------------------------------------------------------------------ GELU
def phi_exact(x):
    return 0.5 * (1.0 + erf(np.asarray(x, dtype=np.float64) / np.sqrt(2.0)))


def gelu_exact(x):
    x = np.asarray(x, dtype=np.float64)
    return x * phi_exact(x)


def gelu_grad_exact(x):
    x = np.asarray(x, dtype=np.float64)
    return phi_exact(x) + x * np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def phi_fit(x):
    """common.h phi2 in float64: the logistic fit of the normal CDF with x clamped to [-6, 6]."""
    xc = np.clip(np.asarray(x, dtype=np.float64), -6.0, 6.0)
    s = xc * xc
    q = (((PHI_C[3] * s + PHI_C[2]) * s + PHI_C[1]) * s + PHI_C[0]) * xc
    return 1.0 / (1.0 + np.exp2(q))


def gelu_fit(x):
    x = np.asarray(x, dtype=np.float64)
    return x * phi_fit(x)


def gelu_grad_fit(x):
    """common.h gelu_grad2: Phi_fit(x) + x phi(x) with the exact density (not clamped)."""
    x = np.asarray(x, dtype=np.float64)
    return phi_fit(x) + x * np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def gelu_forms(bf16: bool):
    """(gelu, gelu') as the kernels of that storage type define them: the fit for bf16, erf for fp32."""
    return (gelu_fit, gelu_grad_fit) if bf16 else (gelu_exact, gelu_grad_exact)


# ------------------------------------------------------------------------------------------------ dropout sites
def site_mask(seed: int, site, shape):
    """(keep [rows, cols] bool, scale) of a site given as (site id, p); (None, 1.0) when the site is off."""
    sid, p = site
    if p <= 0:
        return None, 1.0
    return DH.keep_mask(seed, sid, shape, p), DH.engine_scale(p)


def apply_site(v, keep, scale):
    return v if keep is None else np.where(keep, v * scale, 0.0)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd(y, res, gamma, beta, *, eps, seed=0, pre=(0, 0.0), mid=(0, 0.0), post=(0, 0.0), post_gelu=False, r_round=None,
           gelu=gelu_exact, want_out=True):
    """Returns dict(r, mean, rstd, out, keep_pre, keep_mid, keep_post).  y / res float64 [M, C] (either may be None);
    r_round: callable applied to r before the statistics (the storage rounding of a stored r_out) or None."""
    x = y if y is not None else res
    M, C = x.shape
    kp, sp = site_mask(seed, pre, (M, C))
    km, sm = site_mask(seed, mid, (M, C))
    kq, sq = site_mask(seed, post, (M, C))
    v = np.zeros((M, C))
    if y is not None:
        v = apply_site(np.asarray(y, dtype=np.float64), kp, sp)
    if res is not None:
        v = v + np.asarray(res, dtype=np.float64)
    v = apply_site(v, km, sm)
    if r_round is not None:
        v = r_round(v)
    out = dict(r=v, keep_pre=kp, keep_mid=km, keep_post=kq, mean=None, rstd=None, out=None)
    if not want_out:
        return out
    mean, rstd = ln_stats(v, eps)
    w = (v - mean[:, None]) * rstd[:, None] * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)
    if post_gelu:
        w = gelu(w)
    out.update(mean=mean, rstd=rstd, out=apply_site(w, kq, sq))
    return out


def ln_stats(r, eps):
    """(mean, rstd) of each row with the BIASED variance and eps inside the square root."""
    r = np.asarray(r, dtype=np.float64)
    mean = r.mean(axis=1)
    var = ((r - mean[:, None]) ** 2).mean(axis=1)
    return mean, 1.0 / np.sqrt(var + eps)


def ln_bwd(g1, g2, r, mean, rstd, gamma, g_res, *, seed=0, pre=(0, 0.0), mid=(0, 0.0), post=(0, 0.0), gelu_beta=None,
           gelu_grad=gelu_grad_exact):
    """Returns dict(dr, dy, dgamma, dbeta, dy_colsum, a, terms) in float64.  ``terms``: per-output arrays of the summands'
    magnitudes (sum |.| over rows) for the column sums' bars."""
    r = np.asarray(r, dtype=np.float64)
    M, C = r.shape
    gamma = np.asarray(gamma, dtype=np.float64)
    kp, sp = site_mask(seed, pre, (M, C))
    km, sm = site_mask(seed, mid, (M, C))
    kq, sq = site_mask(seed, post, (M, C))
    a = np.asarray(g1, dtype=np.float64)
    if g2 is not None:
        a = a + np.asarray(g2, dtype=np.float64)
    a = apply_site(a, kq, sq)
    xh = (r - np.asarray(mean, dtype=np.float64)[:, None]) * np.asarray(rstd, dtype=np.float64)[:, None]
    if gelu_beta is not None:
        a = a * gelu_grad(xh * gamma + np.asarray(gelu_beta, dtype=np.float64))
    dyv = a * gamma
    s1 = dyv.mean(axis=1, keepdims=True)
    s2 = (dyv * xh).mean(axis=1, keepdims=True)
    d = np.asarray(rstd, dtype=np.float64)[:, None] * (dyv - s1 - xh * s2)
    if g_res is not None:
        d = d + np.asarray(g_res, dtype=np.float64)
    d = apply_site(d, km, sm)
    dy = apply_site(d, kp, sp)
    return dict(dr=d, dy=dy, dgamma=(a * xh).sum(axis=0), dbeta=a.sum(axis=0), dy_colsum=dy.sum(axis=0), a=a,
                terms=dict(dgamma=np.abs(a * xh).sum(axis=0), dbeta=np.abs(a).sum(axis=0), dy_colsum=np.abs(dy).sum(axis=0)),
                keep_pre=kp, keep_mid=km, keep_post=kq)


# ------------------------------------------------------------------------------------------------ softmax
def key_lengths(rows: int, cols: int, klens=None, rows_per_batch: int = 1) -> np.ndarray:
    """Valid keys of each row: min(klens[row / rows_per_batch], cols), at least 0; all cols without klens."""
    if klens is None:
        return np.full(rows, cols, dtype=np.int64)
    kl = np.asarray(klens, dtype=np.int64)[np.arange(rows) // rows_per_batch]
    return np.clip(kl, 0, cols)


def softmax_fwd(S, cols: int, klens=None, rows_per_batch: int = 1, *, seed=0, site=(0, 0.0)):
    """S [rows, ld] -> dict(P, Pd, valid, keep): softmax over each row's valid keys, 0 elsewhere (a row without any: all 0)."""
    S = np.asarray(S, dtype=np.float64)
    rows, ld = S.shape
    kl = key_lengths(rows, cols, klens, rows_per_batch)
    valid = np.arange(ld)[None, :] < kl[:, None]
    m = np.where(valid, S, -np.inf).max(axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    e = np.where(valid, np.exp(np.where(valid, S, 0.0) - m), 0.0)
    tot = e.sum(axis=1, keepdims=True)
    P = np.where(tot > 0, e / np.where(tot > 0, tot, 1.0), 0.0)
    keep, sc = site_mask(seed, site, (rows, ld))
    return dict(P=P, Pd=apply_site(P, keep, sc), valid=valid, keep=keep)


def softmax_bwd(dPd, P, cols: int, *, seed=0, site=(0, 0.0)):
    """dS = P * (dP - sum(P dP)) over columns < cols (0 beyond), dP = drop(dPd).  Returns dict(dS, dP, dot)."""
    P = np.asarray(P, dtype=np.float64)
    rows, ld = P.shape
    inside = np.arange(ld)[None, :] < cols
    keep, sc = site_mask(seed, site, (rows, ld))
    dP = np.where(inside, apply_site(np.asarray(dPd, dtype=np.float64), keep, sc), 0.0)
    Pm = np.where(inside, P, 0.0)
    dot = (Pm * dP).sum(axis=1, keepdims=True)
    return dict(dS=Pm * (dP - dot), dP=dP, dot=dot)
