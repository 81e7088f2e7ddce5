"""Float64 torch restatement of the fused attention of ssak_amd/csrc/attention.hip (head_dim 64), forward and backward, with the
magnitude companions that the bars of tests/test_gpu_attention.py are built from.

Written from what the kernels define, not from what they compute.  Per utterance b and head h, with q, k, v the bf16 inputs
taken exactly into float64, scale = 64^-0.5, kl = min(max(klens[b], 0), F) (F when klens is None) and keys j >= kl masked::

    S     = scale q k^T                        (masked keys: -inf)
    P     = softmax_rows(S)                    a row with no valid key (kl = 0) is all 0, not NaN
    lse   = logsumexp_rows(S)                  natural log; -inf for a row with no valid key
    Pd    = P * keep * ds                      keep = oracle.dropout_hash.attention_keep_mask, ds = engine_scale(p)
    ctx   = Pd v
    delta = rowsum(dO * ctx)
    dP    = dO v^T
    dS    = P * (dP * keep * ds - delta)       the softmax backward of dPd = dP through the dropout
    dq    = scale dS k,   dk = scale dS^T q,   dv = Pd^T dO

Magnitude companions (the same contractions over absolute values; every one is >= |its quantity|):

    ctx_mag  = Pd |v|                          dv_mag   = Pd^T |dO|
    dq_mag   = scale |dS| |k|                  dk_mag   = scale |dS|^T |q|
    dq_mag2  = scale (P |dP keep ds - delta|) |k|,   dk_mag2 = its transpose form with |q|
    dq_magp  = scale P |k|                     dk_magp  = scale P^T |q|       (carriers of an error in delta)
    delta_mag = sum_d |dO ctx|
    smax     = row max of the valid scaled scores (-inf for kl = 0)
    amax     = row max over valid keys of scale sum_d |q_d k_d|  (what an fp32 sum of the 64 score terms is rounded against)
    dpmax    = row max over valid keys of sum_d |dO_d v_d|         (the same for dP)

and the sums of squared terms, for the expected size of independent roundings of those terms (a variance, not a bound):

    ctx_sq = Pd^2 v^2,  dv_sq = (Pd^2)^T dO^2,  dq_sq = scale^2 dS^2 k^2,  dk_sq = scale^2 (dS^2)^T q^2,  delta_sq = sum_d (dO ctx)^2

``tests/test_attention_ref.py`` pins this restatement to torch float64 autograd of an explicit masked softmax.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import dropout_hash as DH

HD = 64
SCALE = HD ** -0.5


def clamp_klens(klens, B: int, F: int) -> list[int]:
    """The kernels' key lengths: F without klens, else every entry clamped into [0, F]."""
    if klens is None:
        return [F] * B
    return [min(max(int(x), 0), F) for x in (klens.tolist() if hasattr(klens, "tolist") else klens)]


def keep_mask(B: int, F: int, nh: int, p: float, seed: int, stream_id: int, device, b: int | None = None) -> torch.Tensor | None:
    """bool [B, nh, F, F] (None without dropout): the kernels' mask, oracle.dropout_hash.attention_keep_mask; with ``b`` only
    utterance b's [nh, F, F] (its rows (b * nh + h) * F + q of the same function)."""
    if DH.thresh16(p) == 0:
        return None
    if b is None:
        return torch.from_numpy(DH.attention_keep_mask(seed, stream_id, B, nh, F, p)).to(device)
    rk = DH.rowkey(seed, stream_id, np.arange(b * nh * F, (b + 1) * nh * F, dtype=np.uint64))[:, None]
    cm = DH.colmul(np.arange(F, dtype=np.uint64))[None, :]
    w = (rk * cm) & np.uint64(0xFFFFFFFF)
    return torch.from_numpy((w >= np.uint64(DH.thresh16(p) << 16)).reshape(nh, F, F)).to(device)


def attention(qkv: torch.Tensor, B: int, F: int, nh: int, klens=None, dctx: torch.Tensor | None = None, p: float = 0.0,
              seed: int = 0, stream_id: int = 0, keep: torch.Tensor | None = None, device=None) -> dict:
    """qkv [B*F, 3H] (bf16 or any float), dctx [B*F, H] or None -> dict of float64 tensors on ``device`` (qkv's by default):
    ctx [B*F, H], lse [B, nh, F], ctx_mag, smax, amax; with dctx also delta [B, nh, F], delta_mag, dqkv [B*F, 3H] (dq | dk | dv)
    and the gradient companions dq_mag, dq_mag2, dq_magp, dk_mag, dk_mag2, dk_magp, dv_mag, each [B*F, H].  ``keep``
    overrides the oracle mask (bool [B, nh, F, F]); ``p`` gives the scale either way.  One utterance at a time (the [nh, F, F]
    intermediates of one utterance are what is alive)."""
    device = qkv.device if device is None else torch.device(device)
    H = nh * HD
    assert qkv.shape == (B * F, 3 * H), qkv.shape
    kls = clamp_klens(klens, B, F)
    ds = DH.engine_scale(p) if DH.thresh16(p) else 1.0
    x = qkv.to(device=device, dtype=torch.float64).view(B, F, 3, nh, HD)
    g = None if dctx is None else dctx.to(device=device, dtype=torch.float64).view(B, F, nh, HD)
    f64 = dict(dtype=torch.float64, device=device)
    out = {"ctx": torch.zeros(B, F, nh, HD, **f64), "ctx_mag": torch.zeros(B, F, nh, HD, **f64), "ctx_sq": torch.zeros(B, F, nh, HD, **f64),
           "lse": torch.full((B, nh, F), float("-inf"), **f64), "smax": torch.full((B, nh, F), float("-inf"), **f64),
           "amax": torch.zeros(B, nh, F, **f64)}
    if g is not None:
        out["delta"] = torch.zeros(B, nh, F, **f64)
        out["delta_mag"] = torch.zeros(B, nh, F, **f64)
        out["delta_sq"] = torch.zeros(B, nh, F, **f64)
        out["dpmax"] = torch.zeros(B, nh, F, **f64)
        for n in ("dq", "dk", "dv", "dq_mag", "dq_mag2", "dq_magp", "dk_mag", "dk_mag2", "dk_magp", "dv_mag", "dq_sq", "dk_sq",
                  "dv_sq"):
            out[n] = torch.zeros(B, F, nh, HD, **f64)
    for b in range(B):
        kl = kls[b]
        if kl == 0:  # no valid key: ctx = 0, lse = -inf, every gradient and companion 0
            continue
        q = x[b, :, 0].transpose(0, 1)           # [nh, F, HD]
        k = x[b, :kl, 1].transpose(0, 1)         # [nh, kl, HD]
        v = x[b, :kl, 2].transpose(0, 1)
        s = SCALE * (q @ k.transpose(1, 2))      # [nh, F, kl]
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - m)
        den = e.sum(-1, keepdim=True)
        P = e / den
        out["lse"][b] = (m + torch.log(den))[..., 0]
        out["smax"][b] = m[..., 0]
        out["amax"][b] = (SCALE * (q.abs() @ k.abs().transpose(1, 2))).amax(-1)
        kb = keep[b] if keep is not None else keep_mask(B, F, nh, p, seed, stream_id, device, b)
        M = torch.full_like(P, ds) if kb is None else kb[:, :, :kl].to(torch.float64) * ds
        Pd = P * M
        o = Pd @ v                               # [nh, F, HD]
        out["ctx"][b] = o.transpose(0, 1)
        out["ctx_mag"][b] = (Pd @ v.abs()).transpose(0, 1)
        out["ctx_sq"][b] = ((Pd * Pd) @ (v * v)).transpose(0, 1)
        if g is None:
            continue
        do = g[b].transpose(0, 1)                # [nh, F, HD]
        delta = (do * o).sum(-1)
        out["delta"][b] = delta
        out["delta_mag"][b] = (do * o).abs().sum(-1)
        out["delta_sq"][b] = ((do * o) ** 2).sum(-1)
        out["dpmax"][b] = (do.abs() @ v.abs().transpose(1, 2)).amax(-1)
        dP = do @ v.transpose(1, 2)              # [nh, F, kl]
        r = dP * M - delta[..., None]
        dS = P * r
        Pr = P * r.abs()
        qa, ka = q.abs(), k.abs()
        out["dq"][b] = (SCALE * (dS @ k)).transpose(0, 1)
        out["dq_mag"][b] = (SCALE * (dS.abs() @ ka)).transpose(0, 1)
        out["dq_mag2"][b] = (SCALE * (Pr @ ka)).transpose(0, 1)
        out["dq_magp"][b] = (SCALE * (P @ ka)).transpose(0, 1)
        out["dk"][b, :kl] = (SCALE * (dS.transpose(1, 2) @ q)).transpose(0, 1)
        out["dk_mag"][b, :kl] = (SCALE * (dS.abs().transpose(1, 2) @ qa)).transpose(0, 1)
        out["dk_mag2"][b, :kl] = (SCALE * (Pr.transpose(1, 2) @ qa)).transpose(0, 1)
        out["dk_magp"][b, :kl] = (SCALE * (P.transpose(1, 2) @ qa)).transpose(0, 1)
        out["dv"][b, :kl] = (Pd.transpose(1, 2) @ do).transpose(0, 1)
        out["dv_mag"][b, :kl] = (Pd.transpose(1, 2) @ do.abs()).transpose(0, 1)
        out["dq_sq"][b] = (SCALE ** 2 * ((dS * dS) @ (k * k))).transpose(0, 1)
        out["dk_sq"][b, :kl] = (SCALE ** 2 * ((dS * dS).transpose(1, 2) @ (q * q))).transpose(0, 1)
        out["dv_sq"][b, :kl] = ((Pd * Pd).transpose(1, 2) @ (do * do)).transpose(0, 1)
    for n in list(out):
        if out[n].dim() == 4:
            out[n] = out[n].reshape(B * F, H)
    if g is not None:
        out["dqkv"] = torch.cat([out["dq"], out["dk"], out["dv"]], 1)
    return out
