"""CPU: the float64 restatement of the adapter layer's fused tail (tests/attn_adapter_ref.py) against the modules it restates --
``Wav2Vec2AttnAdapterLayer`` of transformers (LayerNorm -> Linear(H, A) -> ReLU -> Linear(A, H), added to its input) followed by
``nn.LayerNorm`` -- in float64 to 1e-12, and the properties of the bf16 emulation and of the bar that the GPU test relies on."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_adapter_ref as AR  # noqa: E402
import rowwise_ref as RR  # noqa: E402


def _adapter_module(H, A):
    try:
        from transformers import Wav2Vec2Config
        from transformers.models.wav2vec2.modeling_wav2vec2 import Wav2Vec2AttnAdapterLayer
        return Wav2Vec2AttnAdapterLayer(Wav2Vec2Config(hidden_size=H, adapter_attn_dim=A)).double()
    except ImportError:  # the same module written out (modeling_wav2vec2.py:930-952)
        class Layer(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.norm, self.linear_1 = torch.nn.LayerNorm(H), torch.nn.Linear(H, A)
                self.act_fn, self.linear_2 = torch.nn.ReLU(), torch.nn.Linear(A, H)

            def forward(self, h):
                return self.linear_2(self.act_fn(self.linear_1(self.norm(h))))
        return Layer().double()


def _case(rng, M, H, A):
    g = lambda *s: rng.standard_normal(s)
    return dict(y=0.7 * g(M, H), res=1.5 * g(M, H) + 0.3, ga=1 + 0.2 * g(H), ba=0.1 * g(H), w1=g(A, H) / np.sqrt(H), b1=0.3 * g(A),
                w2=g(H, A) / np.sqrt(A), b2=0.1 * g(H), gn=1 + 0.2 * g(H), bn=0.1 * g(H))


@pytest.mark.parametrize("M,H,A,eps_n", [(5, 64, 16, 1e-5), (3, 1280, 16, 1e-5), (4, 72, 16, 1e-3)])
def test_fused_tail_is_the_adapter_layer_then_layernorm(M, H, A, eps_n):
    rng = np.random.default_rng(M * H)
    c = _case(rng, M, H, A)
    ad = _adapter_module(H, A)
    assert ad.norm.eps == 1e-5  # a plain nn.LayerNorm: not config.layer_norm_eps
    nxt = torch.nn.LayerNorm(H, eps=eps_n).double()
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    with torch.no_grad():
        for p, v in ((ad.norm.weight, c["ga"]), (ad.norm.bias, c["ba"]), (ad.linear_1.weight, c["w1"]), (ad.linear_1.bias, c["b1"]),
                     (ad.linear_2.weight, c["w2"]), (ad.linear_2.bias, c["b2"]), (nxt.weight, c["gn"]), (nxt.bias, c["bn"])):
            p.copy_(t(v))
        h = t(c["res"]) + t(c["y"])
        h2 = h + ad(h)
        out = nxt(h2)
    ref = AR.fused_tail(**c, eps_n=eps_n)
    assert np.abs(ref["r2p"] - h2.numpy()).max() < 1e-12
    assert np.abs(ref["out"] - out.numpy()).max() < 1e-12
    # y = None: r2 = res
    c2 = dict(c, y=None, res=c["res"] + c["y"])
    assert np.abs(AR.fused_tail(**c2, eps_n=eps_n)["r2p"] - ref["r2p"]).max() < 1e-12


def test_bf16_emulation_stays_inside_the_bar_and_the_bar_is_not_slack():
    """The emulation makes exactly the roundings the bar counts (and none of fp32's), so it must sit inside the bar; and a bar
    that a wrong kernel passes shows nothing: dropping the adapter's bias
    b2, its ReLU or its LayerNorm affine moves r2' outside it."""
    rng = np.random.default_rng(7)
    for H in (64, 1280):
        c = _case(rng, 9, H, 16)
        for k in ("y", "res", "w1", "w2"):
            c[k] = RR.round_bf16(c[k])
        kw = {k: c[k] for k in ("y", "res", "ga", "ba", "w1", "b1", "w2", "b2")}
        ref = AR.fused_tail(**c)
        emu = AR.fused_tail_bf16(**c)
        bar = AR.r2p_bar(**kw, bf16=True)
        assert (np.abs(emu["r2p_stored"] - ref["r2p"]) <= bar).all()
        bar32 = AR.r2p_bar(**kw, bf16=False)
        assert (bar32 < bar).all()
        for wrong in (dict(c, b2=0 * c["b2"]), dict(c, w1=-c["w1"]), dict(c, ga=np.ones(H), ba=np.zeros(H))):
            bad = AR.fused_tail(**wrong)["r2p"]
            assert (np.abs(bad - ref["r2p"]) > bar).mean() > 0.5


def test_exact_structure_cases():
    rng = np.random.default_rng(3)
    c = _case(rng, 6, 64, 16)
    z = AR.fused_tail(**dict(c, w2=0 * c["w2"], b2=0 * c["b2"]))
    assert (z["r2p"] == z["r2"]).all()
    off = AR.fused_tail(**dict(c, b1=c["b1"] - 1e4))
    assert (off["t"] == 0).all() and np.abs(off["r2p"] - (off["r2"] + c["b2"])).max() == 0
