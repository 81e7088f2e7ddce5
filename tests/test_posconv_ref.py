"""CPU: tests/posconv_ref.py (the float64 restatement the positional-convolution kernels are held to) against torch's own
grouped conv1d and weight_norm parametrisation under float64 autograd, its layouts against their index formulas, the
accumulation constants against the rule that defines them, and the argument checks of the test-only entries (host side)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import posconv_ref as P  # noqa: E402
import rowwise_ref as RR  # noqa: E402

F64 = torch.float64
GEOMS = [(96, 2, 16), (128, 2, 16), (96, 2, 8), (192, 3, 4), (96, 2, 5)]  # (H, G, K): cg = 48, 64, 48, 64, and an odd K


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _torch_model(g, v, bias, h, G):
    """transformers' Wav2Vec2PositionalConvEmbedding without the activation: weight_norm(Conv1d(H, H, K, padding = K // 2,
    groups = G), dim = 2), the last frame removed when K is even.  Returns (pre, the parametrised conv)."""
    H, cg, K = v.shape
    conv = torch.nn.Conv1d(H, H, K, padding=K // 2, groups=G, dtype=F64)
    conv = torch.nn.utils.parametrizations.weight_norm(conv, name="weight", dim=2)
    with torch.no_grad():
        conv.parametrizations.weight.original0.copy_(g.view(1, 1, K))
        conv.parametrizations.weight.original1.copy_(v)
        conv.bias.copy_(bias)
    y = conv(h.transpose(1, 2))
    if K % 2 == 0:
        y = y[..., :-1]
    return y.transpose(1, 2), conv


@pytest.mark.parametrize("H,G,K", GEOMS)
@pytest.mark.parametrize("B,F", [(1, 1), (2, 7), (3, 21)])
def test_reference_equals_torch_autograd(H, G, K, B, F):
    gen = torch.Generator().manual_seed(H + K + 10 * B + F)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    cg = H // G
    g, v, bias = rn(K).abs() + 0.5, rn(H, cg, K), rn(H)
    h = rn(B, F, H).requires_grad_(True)
    dpre = rn(B, F, H)
    y, conv = _torch_model(g, v, bias, h, G)
    y.backward(dpre)
    w = P.weight(g, v)
    assert _rel(w, conv.weight.detach()) < 1e-12
    pre, act = P.forward(h.detach(), w, bias)
    assert _rel(pre, y.detach()) < 1e-12
    assert _rel(act, torch.nn.functional.gelu(y.detach())) < 1e-12
    assert _rel(P.grad_input(dpre, w), h.grad) < 1e-12
    dwf = P.grad_weight(h.detach(), dpre, K, G)
    dw = P.dwf_to_w(dwf, K)
    wn = P.weight_norm_bwd(dw, g, v)
    assert _rel(wn["dg"], conv.parametrizations.weight.original0.grad.view(K)) < 1e-12
    assert _rel(wn["dv"], conv.parametrizations.weight.original1.grad) < 1e-12
    # dW itself: autograd of the un-normalised convolution
    wl = w.clone().requires_grad_(True)
    yy = torch.nn.functional.conv1d(h.detach().transpose(1, 2), wl, bias, padding=K // 2, groups=G)
    (yy[..., :-1] if K % 2 == 0 else yy).backward(dpre.transpose(1, 2))
    assert _rel(dw, wl.grad) < 1e-12
    assert torch.equal(P.w_to_dwf(dw), dwf)
    # the abs_sum variants are the same sums over magnitudes
    A, _ = P.forward(h.detach().abs(), w.abs(), bias.abs())
    assert torch.equal(P.forward_abs_sum(h.detach(), w, bias), A)
    assert (P.forward_abs_sum(h.detach(), w, bias) >= pre.abs() * (1 - 1e-12)).all()
    assert (P.grad_input_abs_sum(dpre, w) >= P.grad_input(dpre, w).abs() * (1 - 1e-12)).all()
    assert (P.grad_weight_abs_sum(h.detach(), dpre, K, G) >= dwf.abs() * (1 - 1e-12)).all()
    assert (wn["terms_dg"] >= wn["dg"].abs() * (1 - 1e-12)).all() and (wn["terms_dv"] >= wn["dv"].abs() * (1 - 1e-12)).all()


def test_gelu_is_the_rowwise_restatement():
    x = torch.linspace(-9, 9, 2001, dtype=F64)
    assert np.abs(P.gelu(x).numpy() - RR.gelu_exact(x.numpy())).max() < 1e-14
    assert np.abs(P.gelu_grad(x).numpy() - RR.gelu_grad_exact(x.numpy())).max() < 1e-14
    # sup |gelu''| by central differences of gelu'
    d2 = (P.gelu_grad(x + 1e-5) - P.gelu_grad(x - 1e-5)) / 2e-5
    assert float(d2.abs().max()) <= P.GELU_CURVATURE and abs(float(d2.abs().max()) - math.sqrt(2 / math.pi)) < 1e-6
    y = torch.randn(1000, dtype=F64) * 100
    assert np.array_equal(P.bf16_values(y).numpy(), RR.round_bf16(y.numpy()))


@pytest.mark.parametrize("H,G,K", [(96, 2, 4), (128, 2, 6)])
def test_layouts_follow_their_index_formulas(H, G, K):
    cg = H // G
    w = torch.arange(H * cg * K, dtype=F64).view(H, cg, K)
    wf, wb, dwf = P.to_wf(w), P.to_wb(w), P.w_to_dwf(w)
    assert wf.shape == (H, K, cg) and wb.shape == (G, cg, K, cg) and dwf.shape == (G, K * cg, cg)
    for o in (0, 1, cg - 1, cg, H - 1):
        grp, n = divmod(o, cg)
        for c in (0, 5, cg - 1):
            for k in range(K):
                assert wf[o, k, c] == w[o, c, k]
                assert wb[grp, c, K - 1 - k, n] == w[o, c, k]
                assert dwf[grp, k * cg + c, n] == w[o, c, k]
    assert torch.equal(P.from_wf(wf), w) and torch.equal(P.from_wb(wb), w) and torch.equal(P.dwf_to_w(dwf, K), w)
    B, F = 3, 5
    h = torch.arange(1, B * F * H + 1, dtype=F64).view(B, F, H)
    pg = P.pack(h, K, G)
    assert pg.shape == (G, K // 2 + B * (F + K) + K, cg)
    want = torch.zeros_like(pg)
    for b in range(B):
        for t in range(F):
            for grp in range(G):
                want[grp, K // 2 + b * (F + K) + t] = h[b, t, grp * cg:(grp + 1) * cg]
    assert torch.equal(pg, want)


def _pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x))


def test_accumulation_constants():
    """C_ACC and C_WGRAD are 8 x (the fp32 emulation of the kernels' summation ORDER against float64, in units of u A), rounded
    up to a power of two.  Measured on a SAMPLE of the GPU module's own cases -- the same weights and activations, seed for seed
    (posconv_ref.weights_case / direct_activations / wgrad_activations), at a few of its shapes for both group widths and both
    tap counts; for the weight gradient on group 0 and four taps (first, second, middle, last) of each."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    U = 2.0 ** -24
    worst = 0.0
    for H, K, B, F in ((768, 128, 2, 129), (768, 16, 3, 63), (1024, 128, 1, 63), (1024, 16, 2, 129)):
        c = dict(P.weights_case(H, 16, K), **P.direct_activations(B, F, H, K))
        pre, _ = P.forward(c["h"], c["w"], c["bias"])
        A = P.forward_abs_sum(c["h"], c["w"], c["bias"])
        em = P.emulate_forward(c["h"], c["w"], c["bias"]).double()
        assert (A > 0).all()
        worst = max(worst, float(((em - pre).abs() / (U * A)).max()))
    print(f"forward: max |emulation - float64| / (u A) = {worst:.4f}")
    assert _pow2_ceil(8 * worst) == P.C_ACC
    worst = 0.0
    for H, K, B, F in ((768, 128, 2, 499), (768, 16, 1, 497), (1024, 128, 2, 499), (1024, 16, 2, 499), (768, 128, 1, 385), (768, 16, 1, 1)):
        cg = H // 16
        c = P.wgrad_activations(B, F, H, K)
        taps = [0, 1, K // 2, K - 1]
        ref = P.grad_weight(c["h"], c["dpre"], K, 16)[0].view(K, cg, cg)[taps]
        Aw = P.grad_weight_abs_sum(c["h"], c["dpre"], K, 16)[0].view(K, cg, cg)[taps]
        em = P.emulate_grad_weight(c["h"], c["dpre"], K, 16, taps).double()
        err = (em - ref).abs()
        assert (err[Aw == 0] == 0).all()
        worst = max(worst, float((err[Aw > 0] / (U * Aw[Aw > 0])).max()))
    print(f"weight gradient: max |emulation - float64| / (u A_w) = {worst:.4f}")
    assert _pow2_ceil(8 * worst) == P.C_WGRAD


def test_debug_entries_reject_without_gpu_compute():
    """Argument validation of the ssak_debug_posconv_* entries happens on the host, before any launch."""
    import ssak_amd.hip as h
    L = h.lib
    assert L.ssak_debug_posconv_workspace_bytes(2, 499, 768, 16, 128) >= 2 * 16 * (64 + 2 * 627 + 128) * 48 * 2 + 768 * 128 * 48 * (2 + 16)
    assert L.ssak_debug_posconv_workspace_bytes(2, 499, 1024, 16, 16) > 0
    ws = ctypes.c_void_p(16)  # never dereferenced: every call below is rejected first
    for H, G, K in ((768, 16, 24), (1024, 16, 12), (512, 16, 128), (768, 24, 128), (768, 16, 2048)):
        assert L.ssak_debug_posconv_workspace_bytes(1, 10, H, G, K) == 0
        assert L.ssak_debug_posconv_direct(ws, ws, None, ws, None, 1, 10, H, G, K, 0, 0, ws, 1 << 40, None) == h.SSAK_ERR_INVALID
        assert L.ssak_debug_posconv_wgrad(ws, ws, ws, 1, 10, H, G, K, ws, 1 << 40, None) == h.SSAK_ERR_INVALID
    assert L.ssak_debug_posconv_direct(ws, ws, None, ws, None, 1, 10, 768, 16, 128, 0, 0, ws, 64, None) == h.SSAK_ERR_INVALID
    assert b"workspace" in L.ssak_last_error()
    assert L.ssak_debug_posconv_direct(ws, ws, None, ws, None, 1, 10, 768, 16, 128, 2, 0, ws, 1 << 40, None) == h.SSAK_ERR_INVALID
    assert L.ssak_debug_posconv_direct(None, ws, None, ws, None, 1, 10, 768, 16, 128, 0, 0, ws, 1 << 40, None) == h.SSAK_ERR_INVALID
    assert L.ssak_debug_posconv_prepare(ws, ws, ws, ws, ws, 768, 16, 128, 2, None) == h.SSAK_ERR_INVALID
    assert L.ssak_debug_posconv_prepare(ws, ws, ws, ws, ws, 772, 16, 128, 0, None) == h.SSAK_ERR_INVALID
    assert L.ssak_debug_posconv_pack(ws, ws, 0, 10, 768, 16, 128, 0, None) == h.SSAK_ERR_INVALID
    assert L.ssak_debug_posconv_weight_bwd(ws, ws, ws, ws, ws, None, 768, 16, 128, None) == h.SSAK_ERR_INVALID
