"""float64 NumPy restatement of the utterance-classification chain of ssak_amd/csrc/classify.hip.  TEST INFRASTRUCTURE ONLY.

    hidden [B, F, H] -> pool over time (mean | sum | max, over the frames < len) -> x [B, H]
    z = (x * m1) W1^T + b1;  a = tanh(z);  logits = (a * m2) W2^T + b2
    probs = softmax(logits);  loss = mean_b -log probs[b, label_b]

``m1`` / ``m2`` are the dropout factors of the head's two sites, passed explicitly (keep * scale, or None): the tests fetch the
device's masks and hand them in.  Max pooling reports the LOWEST frame that attains the maximum (``np.argmax``'s rule), and only
that frame receives gradient.  Held to torch autograd in float64 by tests/test_classify_ref.py.
"""
from __future__ import annotations

import numpy as np

MODES = ("mean", "sum", "max")


def _lens(lens, B, F):
    return np.full(B, F, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64)


def pool_fwd(hidden, lens=None, mode="mean"):
    """-> (pooled [B, H] float64, argmax [B, H] int64 | None)."""
    h = np.asarray(hidden, dtype=np.float64)
    B, F, H = h.shape
    n = _lens(lens, B, F)
    assert ((n >= 1) & (n <= F)).all()
    pooled = np.empty((B, H))
    argmax = np.zeros((B, H), dtype=np.int64) if mode == "max" else None
    for b in range(B):
        v = h[b, :n[b]]
        if mode == "mean":
            pooled[b] = v.sum(0) / n[b]
        elif mode == "sum":
            pooled[b] = v.sum(0)
        elif mode == "max":
            argmax[b] = v.argmax(0)  # first occurrence
            pooled[b] = v.max(0)
        else:
            raise ValueError(mode)
    return pooled, argmax


def pool_abs_sum(hidden, lens=None):
    """sum over the pooled frames of |hidden| [B, H]: the scale of the fp32 accumulation bound."""
    h = np.abs(np.asarray(hidden, dtype=np.float64))
    B, F, _ = h.shape
    n = _lens(lens, B, F)
    return np.stack([h[b, :n[b]].sum(0) for b in range(B)])


def pool_bwd(dpooled, F, lens=None, mode="mean", argmax=None):
    """-> d hidden [B, F, H] float64, zero at frames >= len and (max) off the argmax frame."""
    g = np.asarray(dpooled, dtype=np.float64)
    B, H = g.shape
    n = _lens(lens, B, F)
    out = np.zeros((B, F, H))
    for b in range(B):
        if mode == "mean":
            out[b, :n[b]] = g[b] / n[b]
        elif mode == "sum":
            out[b, :n[b]] = g[b]
        elif mode == "max":
            out[b, np.asarray(argmax)[b], np.arange(H)] = g[b]
        else:
            raise ValueError(mode)
    return out


def head_fwd(x, W1, b1, W2, b2, m1=None, m2=None):
    """-> dict(xd, z, a, ad, logits), all float64."""
    x, W1, b1, W2, b2 = (np.asarray(t, dtype=np.float64) for t in (x, W1, b1, W2, b2))
    xd = x if m1 is None else x * np.asarray(m1, dtype=np.float64)
    z = xd @ W1.T + b1
    a = np.tanh(z)
    ad = a if m2 is None else a * np.asarray(m2, dtype=np.float64)
    return dict(xd=xd, z=z, a=a, ad=ad, logits=ad @ W2.T + b2)


def head_bwd(dlogits, x, W1, W2, fwd, m1=None, m2=None):
    """-> dict(dW1, db1, dW2, db2, dx, dz) from ``fwd`` = head_fwd's result."""
    g, W1, W2 = (np.asarray(t, dtype=np.float64) for t in (dlogits, W1, W2))
    dad = g @ W2
    da = dad if m2 is None else dad * np.asarray(m2, dtype=np.float64)
    dz = da * (1.0 - fwd["a"] ** 2)
    dxd = dz @ W1
    dx = dxd if m1 is None else dxd * np.asarray(m1, dtype=np.float64)
    return dict(dW2=g.T @ fwd["ad"], db2=g.sum(0), dW1=dz.T @ fwd["xd"], db1=dz.sum(0), dx=dx, dz=dz)


def softmax_ce(logits, labels=None, grad_scale=1.0):
    """-> (probs [B, C], loss | None, dlogits | None): mean cross-entropy and (softmax - onehot) / B * grad_scale."""
    l = np.asarray(logits, dtype=np.float64)
    B, C = l.shape
    e = np.exp(l - l.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    if labels is None:
        return p, None, None
    y = np.asarray(labels, dtype=np.int64)
    assert ((y >= 0) & (y < C)).all()
    loss = -np.log(p[np.arange(B), y]).mean()
    onehot = np.zeros_like(p)
    onehot[np.arange(B), y] = 1.0
    return p, loss, (p - onehot) / B * grad_scale


def classify(hidden, lens, mode, W1, b1, W2, b2, labels, m1=None, m2=None):
    """The whole chain and its gradients -> dict(pooled, argmax, logits, probs, loss, dhidden, dW1, db1, dW2, db2)."""
    hidden = np.asarray(hidden, dtype=np.float64)
    pooled, argmax = pool_fwd(hidden, lens, mode)
    f = head_fwd(pooled, W1, b1, W2, b2, m1, m2)
    probs, loss, dlogits = softmax_ce(f["logits"], labels)
    g = head_bwd(dlogits, pooled, W1, W2, f, m1, m2)
    dhidden = pool_bwd(g["dx"], hidden.shape[1], lens, mode, argmax)
    return dict(pooled=pooled, argmax=argmax, logits=f["logits"], probs=probs, loss=loss, dhidden=dhidden,
                dW1=g["dW1"], db1=g["db1"], dW2=g["dW2"], db2=g["db2"])
