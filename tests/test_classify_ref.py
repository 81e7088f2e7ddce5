"""CPU: tests/classify_ref.py (the float64 restatement the GPU classification tests compare against) held to torch autograd
in float64, at 1e-10 -- pooling with lengths in all three modes, the head with explicit dropout factors, softmax + mean
cross-entropy, and the gradients of the whole chain."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classify_ref as R  # noqa: E402

TOL = 1e-10
B, F, H = 3, 37, 72
LENS = (37, 1, 20)


def _case(C, with_masks, seed=0):
    rng = np.random.default_rng(seed)
    d = dict(hidden=rng.standard_normal((B, F, H)), W1=rng.standard_normal((H, H)) / np.sqrt(H), b1=0.1 * rng.standard_normal(H),
             W2=rng.standard_normal((C, H)) / np.sqrt(H), b2=0.1 * rng.standard_normal(C), labels=rng.integers(0, C, B))
    d["m1"] = (rng.random((B, H)) >= 0.25) / 0.75 if with_masks else None
    d["m2"] = (rng.random((B, H)) >= 0.25) / 0.75 if with_masks else None
    return d


def _torch_chain(d, lens, mode):
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in d.items() if k in ("hidden", "W1", "b1", "W2", "b2")}
    rows = []
    for b in range(B):
        v = t["hidden"][b, :(F if lens is None else lens[b])]
        rows.append(v.mean(0) if mode == "mean" else v.sum(0) if mode == "sum" else v.max(0)[0])
    x = torch.stack(rows)
    if d["m1"] is not None:
        x = x * torch.tensor(d["m1"])
    a = torch.tanh(torch.nn.functional.linear(x, t["W1"], t["b1"]))
    if d["m2"] is not None:
        a = a * torch.tensor(d["m2"])
    logits = torch.nn.functional.linear(a, t["W2"], t["b2"])
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor(d["labels"], dtype=torch.long))
    loss.backward()
    return logits.detach().numpy(), torch.softmax(logits, 1).detach().numpy(), loss.item(), {k: v.grad.numpy() for k, v in t.items()}


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("lens", [None, LENS], ids=["all", "lens"])
@pytest.mark.parametrize("C,with_masks", [(2, False), (5, True)])
def test_chain_matches_autograd(mode, lens, C, with_masks):
    d = _case(C, with_masks)
    logits, probs, loss, g = _torch_chain(d, lens, mode)
    r = R.classify(d["hidden"], lens, mode, d["W1"], d["b1"], d["W2"], d["b2"], d["labels"], d["m1"], d["m2"])
    assert np.abs(r["logits"] - logits).max() < TOL
    assert np.abs(r["probs"] - probs).max() < TOL and np.abs(r["probs"].sum(1) - 1).max() < TOL
    assert abs(r["loss"] - loss) < TOL
    for name, key in (("hidden", "dhidden"), ("W1", "dW1"), ("b1", "db1"), ("W2", "dW2"), ("b2", "db2")):
        assert np.abs(r[key] - g[name]).max() < TOL, name
    if lens is not None:
        for b in range(B):
            assert (r["dhidden"][b, lens[b]:] == 0).all()


def test_max_takes_the_lowest_frame_on_a_tie():
    h = np.zeros((1, 5, 8))
    h[0, 1] = h[0, 3] = 2.0  # the maximum twice: frame 1 wins
    h[0, 4, 0] = 2.0
    pooled, argmax = R.pool_fwd(h, None, "max")
    assert (pooled == 2.0).all() and (argmax == 1).all()
    pooled, argmax = R.pool_fwd(h, [1], "max")
    assert (pooled == 0.0).all() and (argmax == 0).all()
    d = R.pool_bwd(np.ones((1, 8)), 5, None, "max", np.ones((1, 8), dtype=np.int64))
    assert (d[0, 1] == 1).all() and d.sum() == 8


def test_softmax_without_labels_and_grad_scale():
    l = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]])
    p, loss, g = R.softmax_ce(l)
    assert loss is None and g is None and np.abs(p[1] - 1 / 3).max() < 1e-15
    _, loss, g = R.softmax_ce(l, [2, 0], grad_scale=4.0)
    _, _, g1 = R.softmax_ce(l, [2, 0])
    assert np.abs(g - 4 * g1).max() < 1e-15 and abs(loss - (-(np.log(p[0, 2]) + np.log(p[1, 0])) / 2)) < 1e-15
