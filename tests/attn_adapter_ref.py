"""Float64 numpy restatement of the closing row kernel of an adapter layer (ssak_amd/csrc/attn_adapter.hip), with the bf16
emulation and the error bar derived from the roundings the kernel makes.

What the kernel defines (transformers modeling_wav2vec2.py: Wav2Vec2AttnAdapterLayer :930-952 after the feed-forward residual
of Wav2Vec2EncoderLayerStableLayerNorm :644-647, then the LayerNorm that opens the next layer)::

    r2  = res + y
    n   = LN_a(r2)            = (r2 - mean) * rstd * ga + ba,   rstd = 1 / sqrt(var + eps_a), var BIASED
    t   = relu(n W1^T + b1)                                     W1 [A, H]
    r2' = r2 + t W2^T + b2                                      W2 [H, A]     -> stored (rounded to the storage type)
    out = LN_next(stored r2') = (r2' - mean') * rstd' * gn + bn               -> stored

``tests/test_attn_adapter_ref.py`` checks :func:`fused_tail` against ``Wav2Vec2AttnAdapterLayer`` + ``nn.LayerNorm`` in float64
(so the reference is right independently of the kernel); ``tests/test_gpu_mms.py`` holds the kernel to it.

The bar of r2' (:func:`r2p_bar`).  u = 2^-24 is the fp32 unit roundoff; e = 2^-9 (half a bf16 ulp, relative) for bf16 storage
and 0 for fp32 storage -- the kernel of the fp32-exact mode rounds nothing below fp32, so only the u terms remain, which is
the form of the bar the float row-kernel tests use (one storage ulp + u x the terms of the sum).  The kernel's roundings, in
order (nothing here is fitted to what the kernel returns).  Every term is a worst-case bound with absolute values summed,
except the H independent bf16 roundings of step 1 inside the sum of step 2: each is at most e |n_h| and they are independent
of one another, so their sum is bounded by RSS_K = 4 times the root of the sum of the squared bounds (each rounding error has
standard deviation <= e |n_h| / sqrt(3): 4 root-sum-squares is 6.9 standard deviations of the sum, probability < 1e-11 per
element; the linear sum of 1 280 such bounds would be 0.15 at H = 1 280, a bar that a kernel without b2 passes):

1. LN_a in fp32: |n_k - n| <= floor_n = 1e-5 (|xhat ga| + |ba|) + 4e-6 rstd mean|r2| |ga|  (the fp32 statistics: the floor the
   LayerNorm forward test uses, tests/test_gpu_rowwise.py), then n_k is rounded to bf16 before the MFMA:
   e_n = e (|n| + floor_n) [independent per element] + floor_n [common to a row: summed linearly].
2. Down-projection, fp32 accumulation of H products (bf16 x bf16 products are exact in fp32) in whatever order the eight
   partial tiles and the MFMA take: e_t = RSS_K e sqrt((|n| + floor_n)^2 (W1^2)^T) + floor_n |W1|^T + (H + 8) u (|n| |W1|^T + |b1|).  ReLU is 1-Lipschitz, so it passes e_t on;
   relu(t) is then rounded to bf16: e_th = e_t + e (|t| + e_t).
3. Up-projection over A terms (+ 16 zero terms of the instruction's K = 32), + b2, + r2 in fp32:
   e_d = e_th |W2|^T + (A + 3) u (|t| |W2|^T + |b2| + |r2|) + 2 u |y + res terms|.
4. The store: one ulp of the storage type at r2'.

out is checked against LN_next of the r2' the kernel STORED, so the errors above do not enter it: the LayerNorm forward bar of
tests/test_gpu_rowwise.py applies unchanged (eps_st |ref| + 1.2 floor).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import rowwise_ref as RR  # noqa: E402

U = 2.0 ** -24
RSS_K = 4.0


def ln(r, gamma, beta, eps):
    mean, rstd = RR.ln_stats(r, eps)
    return (r - mean[:, None]) * rstd[:, None] * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)


def fused_tail(y, res, ga, ba, w1, b1, w2, b2, gn, bn, *, eps_a=1e-5, eps_n=1e-5, r_round=None, op_round=None):
    """dict(r2, n, t, delta, r2p, r2p_stored, out) in float64.  ``r_round``: the storage rounding of the stored r2' (None: none);
    ``op_round``: the rounding of the two products' activation operands (the bf16 emulation; None: none)."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    r2 = f(res) + (f(y) if y is not None else 0.0)
    n = ln(r2, ga, ba, eps_a)
    n_op = op_round(n) if op_round else n
    t = np.maximum(n_op @ f(w1).T + f(b1), 0.0)
    t_op = op_round(t) if op_round else t
    delta = t_op @ f(w2).T + f(b2)
    r2p = r2 + delta
    stored = r_round(r2p) if r_round else r2p
    return dict(r2=r2, n=n, t=t, delta=delta, r2p=r2p, r2p_stored=stored, out=ln(stored, gn, bn, eps_n))


def fused_tail_bf16(y, res, ga, ba, w1, b1, w2, b2, gn, bn, **kw):
    """The kernel's bf16 arithmetic in float64: LN_a(r2) and relu(..) rounded to bf16 on their way into the MFMAs, r2' rounded
    to bf16 when stored; every sum exact.  What remains between this and the kernel is fp32 accumulation."""
    return fused_tail(y, res, ga, ba, w1, b1, w2, b2, gn, bn, r_round=RR.round_bf16, op_round=RR.round_bf16, **kw)


def ln_floor(r, gamma, beta, eps):
    """The fp32-statistics floor of a LayerNorm output (tests/test_gpu_rowwise.py, `out`)."""
    mean, rstd = RR.ln_stats(r, eps)
    xg = np.abs((r - mean[:, None]) * rstd[:, None] * np.asarray(gamma, dtype=np.float64))
    return 1e-5 * (xg + np.abs(beta)) + 4e-6 * (rstd * np.abs(r).mean(axis=1))[:, None] * np.abs(gamma)


def r2p_bar(y, res, ga, ba, w1, b1, w2, b2, *, eps_a=1e-5, bf16: bool):
    """Per-element bound on |kernel r2' - float64 r2'| (the module docstring's steps 1-4)."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    e = 2.0 ** -9 if bf16 else 0.0
    ref = fused_tail(y, res, ga, ba, w1, b1, w2, b2, ga, ba, eps_a=eps_a)
    r2, n, t = ref["r2"], ref["n"], ref["t"]
    H, A = r2.shape[1], f(w1).shape[0]
    aw1, aw2 = np.abs(f(w1)), np.abs(f(w2))
    fl = ln_floor(r2, ga, ba, eps_a)
    e_t = RSS_K * e * np.sqrt(((np.abs(n) + fl) ** 2) @ (aw1 ** 2).T) + fl @ aw1.T + (H + 8) * U * (np.abs(n) @ aw1.T + np.abs(f(b1)))
    e_th = e_t + e * (t + e_t)
    terms = (np.abs(f(y)) if y is not None else 0.0) + np.abs(f(res))
    e_d = e_th @ aw2.T + (A + 3) * U * (t @ aw2.T + np.abs(f(b2)) + np.abs(r2)) + 2 * U * terms
    ulp = RR.bf16_ulp(ref["r2p"]) if bf16 else 2.0 ** -23 * np.abs(ref["r2p"]) + 1e-45
    return ulp + e_d
