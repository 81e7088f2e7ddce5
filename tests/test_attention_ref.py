"""CPU: tests/attention_ref.py (the float64 restatement the fused attention kernels are held to) against torch float64 autograd
of an explicit masked softmax, with dropout by oracle.dropout_hash.attention_keep_mask and engine_scale.  Ragged key lengths,
klen = 0 (compared against the engine's zero convention), klen > F and klen < 0 (clamped like the kernels)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attention_ref as AR  # noqa: E402
from oracle import dropout_hash as DH  # noqa: E402

SEED, STREAM = 0x0BADC0DE12345, DH.ds_attn(3)


def _autograd(qkv, dctx, B, F, nh, kls, p):
    """Plain autograd: softmax over the first kl keys of each utterance, Pd = P * keep * engine_scale, ctx = Pd v; the
    gradient of sum(ctx * dctx).  Utterances with kl = 0 are skipped (torch would give NaN); their rows stay 0."""
    H = nh * 64
    x = qkv.double().view(B, F, 3, nh, 64).clone().requires_grad_(True)
    keep = AR.keep_mask(B, F, nh, p, SEED, STREAM, "cpu")
    ds = DH.engine_scale(p)
    ctx = torch.zeros(B, F, nh, 64, dtype=torch.float64)
    lse = torch.full((B, nh, F), float("-inf"), dtype=torch.float64)
    outs = []
    for b in range(B):
        if kls[b] == 0:
            continue
        q, k, v = x[b, :, 0].transpose(0, 1), x[b, :, 1].transpose(0, 1), x[b, :, 2].transpose(0, 1)
        s = q @ k.transpose(1, 2) * 64 ** -0.5
        s = s.masked_fill(torch.arange(F)[None, None, :] >= kls[b], float("-inf"))
        pr = torch.softmax(s, -1)
        if keep is not None:
            pr = pr * keep[b] * ds
        o = pr @ v
        outs.append((b, o))
        lse[b] = torch.logsumexp(s, -1).detach()
    loss = sum((o * dctx.double().view(B, F, nh, 64)[b].transpose(0, 1)).sum() for b, o in outs)
    loss.backward()
    for b, o in outs:
        ctx[b] = o.detach().transpose(0, 1)
    return ctx.reshape(B * F, H), lse, x.grad.reshape(B * F, 3 * H)


CASES = [  # B, F, nh, klens, p
    (3, 70, 2, [70, 1, 66], 0.0),
    (3, 70, 2, [0, 70, 33], 0.0),
    (4, 65, 1, [100, -3, 64, 65], 0.0),
    (3, 40, 2, [40, 0, 17], 0.1),
    (2, 33, 3, [33, 5], 0.5),
    (2, 20, 1, None, 0.3),
]


@pytest.mark.parametrize("B,F,nh,klens,p", CASES)
def test_reference_matches_autograd(B, F, nh, klens, p):
    g = torch.Generator().manual_seed(B * 1000 + F)
    H = nh * 64
    qkv = (torch.randn(B * F, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    dctx = torch.randn(B * F, H, generator=g).to(torch.bfloat16)
    kls = AR.clamp_klens(None if klens is None else torch.tensor(klens), B, F)
    r = AR.attention(qkv, B, F, nh, None if klens is None else torch.tensor(klens), dctx, p=p, seed=SEED, stream_id=STREAM)
    ctx, lse, grad = _autograd(qkv, dctx, B, F, nh, kls, p)
    assert torch.allclose(r["ctx"], ctx, rtol=1e-12, atol=1e-12)
    assert torch.equal(torch.isinf(r["lse"]), torch.isinf(lse))
    fin = torch.isfinite(lse)
    assert torch.allclose(r["lse"][fin], lse[fin], rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["dqkv"], grad, rtol=1e-10, atol=1e-12)
    # delta = rowsum(dO * ctx) per (b, h, q)
    o = ctx.view(B, F, nh, 64)
    want = (o * dctx.double().view(B, F, nh, 64)).sum(-1).permute(0, 2, 1)
    assert torch.allclose(r["delta"], want, rtol=1e-12, atol=1e-12)
    # the companions bound their quantities
    for n, m in (("ctx", "ctx_mag"), ("dq", "dq_mag"), ("dk", "dk_mag"), ("dv", "dv_mag"), ("delta", "delta_mag")):
        assert bool((r[n].abs() <= r[m] * (1 + 1e-12) + 1e-300).all()), n
    assert bool((r["dq"].abs() <= r["dq_mag2"] * (1 + 1e-12) + 1e-300).all())
    assert bool((r["dk"].abs() <= r["dk_mag2"] * (1 + 1e-12) + 1e-300).all())
    # klen = 0: zeros and -inf, not NaN; keys at or beyond the (clamped) key length get no dK / dV
    for b, kl in enumerate(kls):
        rows = slice(b * F, (b + 1) * F)
        if kl == 0:
            assert bool((r["ctx"][rows] == 0).all()) and bool((r["dqkv"][rows] == 0).all())
            assert bool(torch.isneginf(r["lse"][b]).all())
        assert bool((r["dqkv"][b * F + kl:(b + 1) * F, H:] == 0).all())
    for n, t in r.items():
        assert not torch.isnan(t).any(), n


def test_key_length_clamps():
    """klen above F counts as F, a negative one as 0, as in the kernels."""
    assert AR.clamp_klens(torch.tensor([5, 99, -3, 0]), 4, 10) == [5, 10, 0, 0]
    assert AR.clamp_klens(None, 2, 7) == [7, 7]
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(2 * 30, 3 * 64, generator=g).to(torch.bfloat16)
    dctx = torch.randn(2 * 30, 64, generator=g).to(torch.bfloat16)
    a = AR.attention(qkv, 2, 30, 1, torch.tensor([45, -3]), dctx)
    b = AR.attention(qkv, 2, 30, 1, torch.tensor([30, 0]), dctx)
    for n in a:
        assert torch.equal(a[n], b[n]), n


def test_softmax_scores_and_magnitudes():
    """smax is the row max of the valid scaled scores and lse - smax lies in [0, log kl]; amax bounds |S|."""
    g = torch.Generator().manual_seed(11)
    B, F, nh = 2, 50, 2
    qkv = (torch.randn(B * F, 3 * nh * 64, generator=g) * 3).to(torch.bfloat16)
    r = AR.attention(qkv, B, F, nh, torch.tensor([50, 7]))
    gap = r["lse"] - r["smax"]
    assert bool((gap >= 0).all()) and bool((gap[0] <= torch.log(torch.tensor(50.0))).all()) and bool((gap[1] <= 2.0).all())
    assert bool((r["smax"].abs() <= r["amax"]).all())


def test_per_utterance_mask_is_the_oracle_mask():
    """The per-utterance mask the reference generates (to keep B = 32 x 12 heads x 499^2 off the host at once) is the slice
    of oracle.dropout_hash.attention_keep_mask."""
    whole = AR.keep_mask(3, 37, 2, 0.25, SEED, STREAM, "cpu")
    for b in range(3):
        assert torch.equal(AR.keep_mask(3, 37, 2, 0.25, SEED, STREAM, "cpu", b), whole[b])
