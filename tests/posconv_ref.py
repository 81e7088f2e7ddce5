"""Float64 restatement of the grouped, weight-normed positional convolution of the Wav2Vec2 encoder
(``Conv1d(H, H, K, padding = K // 2, groups = G)`` under ``weight_norm(dim = 2)``, the last frame dropped for even K, then GELU),
of its gradients and of the layouts the kernels of ssak_amd/csrc/posconv.hip exchange.

Written from the definition in plain torch, one tap at a time, and device-agnostic: every function computes where its inputs
live, so the largest cases run in float64 on the device.  ``tests/test_posconv_ref.py`` pins every function to
``torch.nn.functional.conv1d`` and ``torch.nn.utils.parametrizations.weight_norm`` under float64 autograd;
``tests/test_gpu_posconv.py`` holds the kernels to it.

Shapes: h, dpre, pre [B, F, H];  w, v [H, cg, K] (w[o, c, k]: output channel o = group * cg + n, input channel c of o's group);
g [K];  bias [H].

    w[o, c, k]   = g[k] v[o, c, k] / ||v[:, :, k]||
    pre[b, t, o] = bias[o] + sum_{c, k} w[o, c, k] h[b, t + k - K // 2, group(o) * cg + c]        (h = 0 outside [0, F))
    dx[b, s, group * cg + c] = sum_{n, k} w[group * cg + n, c, k] dpre[b, s - k + K // 2, group * cg + n]
    dw[o, c, k]  = sum_{b, t} dpre[b, t, o] h[b, t + k - K // 2, group(o) * cg + c]
    dot[k] = sum_{o, c} dw v,   dg[k] = dot[k] / ||v_k||,   dv = g / ||v_k|| (dw - v dot / ||v_k||^2)

Kernel layouts (index formulas from the comments of posconv.hip):

    wf[o][k][c]                = w[o, c, k]                         forward operand
    wb[group][c][K - 1 - k][n] = w[group * cg + n, c, k]            input-gradient operand (flipped taps)
    dwf[group][k * cg + c][n]  = dw[group * cg + n, c, k]           what the weight gradient writes
    packed[group][K // 2 + b (F + K) + t][c] = h[b, t, group * cg + c], every other row 0, K // 2 + B (F + K) + K rows

The fp32 emulations at the end restate the ORDER in which the direct kernels add (not their arithmetic inside a matrix
instruction, which is undocumented): they are what the accumulation constants of tests/test_gpu_posconv.py are derived from.
"""
from __future__ import annotations

import math

import torch

F64 = torch.float64


def _d(x):
    return x.to(F64)


# ------------------------------------------------------------------------------------------------ GELU
# (gelu, gelu_grad and bf16_values below restate rowwise_ref.gelu_exact / gelu_grad_exact / round_bf16, which are numpy and so
# host-only, in torch: the references of the largest cases run in float64 on the device.  tests/test_posconv_ref.py holds them
# to the numpy versions.)
def gelu(x):
    """x Phi(x) with the exact normal CDF (tests/rowwise_ref.py: gelu_exact), in torch."""
    x = _d(x)
    return x * 0.5 * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    """Phi(x) + x phi(x)."""
    x = _d(x)
    return 0.5 * (1.0 + torch.special.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


GELU_CURVATURE = 0.7979  # sup |gelu''| = gelu''(0) = 2 phi(0) = sqrt(2 / pi), rounded up


# ------------------------------------------------------------------------------------------------ weight norm
def tap_norms(v):
    """||v[:, :, k]|| [K]."""
    return _d(v).pow(2).sum(dim=(0, 1)).sqrt()


def weight(g, v):
    return _d(g) * _d(v) / tap_norms(v)


def weight_norm_bwd(dw, g, v):
    """dw [H, cg, K] -> dict(dg [K], dv [H, cg, K], terms_dg, terms_dv): the gradients of sum(dw * weight(g, v)) and, per output,
    the sum of the magnitudes of the terms a kernel adds to form it (for the bars)."""
    dw, g, v = _d(dw), _d(g), _d(v)
    n = tap_norms(v)
    dot = (dw * v).sum(dim=(0, 1))
    adot = (dw * v).abs().sum(dim=(0, 1))
    return dict(dg=dot / n, dv=g / n * (dw - v * dot / (n * n)), terms_dg=adot / n,
                terms_dv=g.abs() / n * (dw.abs() + v.abs() * adot / (n * n)))


# ------------------------------------------------------------------------------------------------ convolution
def _padded(x, K, G):
    """[B, F, H] -> [B, K // 2 + F + K, G, cg]: frame t at row K // 2 + t, zeros around."""
    B, F, H = x.shape
    p = torch.zeros((B, K // 2 + F + K, H), dtype=F64, device=x.device)
    p[:, K // 2:K // 2 + F] = _d(x)
    return p.view(B, -1, G, H // G)


def _groups(w, G):
    H, cg, K = w.shape
    assert H == G * cg
    return _d(w).view(G, cg, cg, K)  # [group, n, c, k]


def _conv(h, w, G):
    B, F, H = h.shape
    K = w.shape[2]
    hp, wg = _padded(h, K, G), _groups(w, G)
    y = torch.zeros((B, F, G, H // G), dtype=F64, device=h.device)
    for k in range(K):
        y += torch.einsum("bfgc,gnc->bfgn", hp[:, k:k + F], wg[..., k])
    return y.reshape(B, F, H)


def forward(h, w, bias=None):
    """(pre, gelu(pre)); the even-K rule: the F + 1-th output frame of the padded convolution is dropped."""
    pre = _conv(h, w, w.shape[0] // w.shape[1])
    if bias is not None:
        pre = pre + _d(bias)
    return pre, gelu(pre)


def forward_abs_sum(h, w, bias=None):
    """A[b, t, o] = sum |h| |w| (+ |bias|): the sum of the magnitudes of the terms of pre."""
    a = _conv(h.abs(), w.abs(), w.shape[0] // w.shape[1])
    return a if bias is None else a + _d(bias).abs()


def grad_input(dpre, w):
    B, F, H = dpre.shape
    _, cg, K = w.shape
    G = H // cg
    wg = _groups(w, G)
    # dx[s] takes dpre[s - k + K // 2]: row K // 2 + (s - k + K // 2) = s + (2 (K // 2) - k) of the padded gradient
    dp = torch.zeros((B, F + 2 * (K // 2) + 1, G, cg), dtype=F64, device=dpre.device)
    dp[:, K // 2:K // 2 + F] = _d(dpre).view(B, F, G, cg)
    dx = torch.zeros((B, F, G, cg), dtype=F64, device=dpre.device)
    for k in range(K):
        r = 2 * (K // 2) - k
        dx += torch.einsum("bfgn,gnc->bfgc", dp[:, r:r + F], wg[..., k])
    return dx.reshape(B, F, H)


def grad_input_abs_sum(dpre, w):
    return grad_input(dpre.abs(), w.abs())


def grad_weight(h, dpre, K, G):
    """dwf [G, K * cg, cg] (the kernel's index order, see the module docstring)."""
    B, F, H = h.shape
    cg = H // G
    hp = _padded(h, K, G)
    d = _d(dpre).view(B, F, G, cg)
    out = torch.zeros((G, K, cg, cg), dtype=F64, device=h.device)
    for k in range(K):
        out[:, k] = torch.einsum("bfgc,bfgn->gcn", hp[:, k:k + F], d)
    return out.reshape(G, K * cg, cg)


def grad_weight_abs_sum(h, dpre, K, G):
    """A_w = sum |h| |dpre|, in the dwf order."""
    return grad_weight(h.abs(), dpre.abs(), K, G)


# ------------------------------------------------------------------------------------------------ layouts
def to_wf(w):
    return w.permute(0, 2, 1).contiguous()  # [H, K, cg]


def from_wf(wf):
    return wf.permute(0, 2, 1).contiguous()


def to_wb(w):
    H, cg, K = w.shape
    return w.view(H // cg, cg, cg, K).flip(3).permute(0, 2, 3, 1).contiguous()  # [group, c, K - 1 - k, n]


def from_wb(wb):
    G, cg, K, _ = wb.shape
    return wb.permute(0, 3, 1, 2).flip(3).reshape(G * cg, cg, K).contiguous()


def dwf_to_w(dwf, K):
    """dwf [G, K * cg, cg] -> dw [H, cg, K]."""
    G, _, cg = dwf.shape
    return dwf.view(G, K, cg, cg).permute(0, 3, 2, 1).reshape(G * cg, cg, K).contiguous()


def w_to_dwf(dw):
    H, cg, K = dw.shape
    return dw.view(H // cg, cg, cg, K).permute(0, 3, 2, 1).reshape(H // cg, K * cg, cg).contiguous()


def pack(h, K, G):
    """[B, F, H] -> [G, K // 2 + B (F + K) + K, cg] in h's type."""
    B, F, H = h.shape
    cg = H // G
    out = torch.zeros((G, K // 2 + B * (F + K) + K, cg), dtype=h.dtype, device=h.device)
    for b in range(B):
        r = K // 2 + b * (F + K)
        out[:, r:r + F] = h[b].view(F, G, cg).permute(1, 0, 2)
    return out


# ------------------------------------------------------------------------------------------------ fp32 emulations of the ORDER
def _seq_sum_f32(x, dim):
    """Left-to-right fp32 sum along dim."""
    x = x.movedim(dim, 0)
    s = torch.zeros_like(x[0])
    for i in range(x.shape[0]):
        s = s + x[i]
    return s


def emulate_forward(h, w, bias=None):
    """pre as posconv_direct_kernel orders its additions, every addition rounded to fp32: the K cg products of an output in
    (tap, channel) order, cut into slices of 32 (one matrix instruction each: cg = 48 packs two taps into three slices, cg = 64 one
    tap into two); a slice is summed left to right and the slice sums are added to the accumulator in step order; the bias last.
    h, w hold bf16 values, so every product is exact in fp32."""
    B, F, H = h.shape
    _, cg, K = w.shape
    G = H // cg
    f32 = torch.float32
    hp = _padded(h, K, G).to(f32)
    wg = _groups(w, G).to(f32).permute(0, 1, 3, 2).reshape(G, cg, K * cg)  # [group, n, (k, c)]
    win = hp.unfold(1, K, 1)[:, :F].permute(0, 1, 2, 4, 3).reshape(B, F, G, K * cg)  # [b, t, group, (k, c)]
    acc = torch.empty((B, F, H), dtype=f32)
    for t in range(0, F, 8):  # (8 frames at a time: the products of one frame are G cg K cg floats)
        prod = win[:, t:t + 8, :, None, :] * wg[None, None]  # [b, t, group, n, K cg]
        sl = _seq_sum_f32(prod.view(B, -1, G, cg, K * cg // 32, 32), 5)
        acc[:, t:t + 8] = _seq_sum_f32(sl, 4).reshape(B, -1, H)
    return acc if bias is None else acc + bias.to(f32)


def emulate_grad_weight(h, dpre, K, G, taps, group=0):
    """dwf[group][tap * cg + c][n] for the given taps as posconv_wgrad_kernel + posconv_wgrad_sum_kernel order their additions in
    fp32: the packed rows r in [0, B (F + K)) in four ranges of per_split = ceil(ceil(rows / 128) / 4) * 128 rows; inside a range
    stages of 128 rows, four slices of 32 rows each (one matrix instruction), a slice summed left to right, slice sums added to
    the range's accumulator in order; the four partials added as ((p0 + p1) + p2) + p3.  Returns [len(taps), cg, cg]."""
    B, F, H = h.shape
    cg = H // G
    f32 = torch.float32
    x = pack(h, K, G)[group].to(f32)     # [rows_per_group, cg]
    dy = pack(dpre, K, G)[group].to(f32)
    rows, lead = B * (F + K), K // 2
    per_split = (-(-rows // 128) + 3) // 4 * 128
    pad = 4 * per_split + K + lead
    x = torch.cat([x, torch.zeros((max(0, pad - x.shape[0]), cg), dtype=f32)])
    dy = torch.cat([dy, torch.zeros((max(0, pad - dy.shape[0]), cg), dtype=f32)])
    out = []
    for tap in taps:
        parts = []
        for s in range(4):
            lo = s * per_split
            hi = min(rows, lo + per_split)
            n = max(0, -(-(hi - lo) // 128)) * 128  # whole stages: the rows past `hi` meet zero rows of dy
            if n == 0:
                parts.append(torch.zeros((cg, cg), dtype=f32))
                continue
            prod = x[lo + tap:lo + tap + n, :, None] * dy[lead + lo:lead + lo + n, None, :]  # [n, c, n']
            parts.append(_seq_sum_f32(_seq_sum_f32(prod.view(n // 32, 32, cg, cg), 1), 0))
        out.append(((parts[0] + parts[1]) + parts[2]) + parts[3])
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------ seeded test data
def bf16_values(x):
    """x rounded to bf16 (round to nearest even), as float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def real_weights(seed, H, G, K):
    """v ~ 0.02 N(0, 1), g = tap norm * (1 + 0.1 N(0, 1)), bias ~ 0.1 N(0, 1) (fp32 values, as float64)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    v = (0.02 * rn(H, H // G, K)).to(torch.float32).to(F64)
    g = (tap_norms(v) * (1.0 + 0.1 * rn(K))).to(torch.float32).to(F64)
    return dict(v=v, g=g, bias=(0.1 * rn(H)).to(torch.float32).to(F64))


def real_activations(seed, B, F, H):
    """h, dpre ~ N(0, 1) rounded to bf16; for B >= 2 the first and last 64 frames of every utterance are scaled by 8, so that a
    window that reaches into the neighbouring utterance, or misses the zero gap, is far outside any bar."""
    gen = torch.Generator().manual_seed(seed)
    h, dpre = (torch.randn(B, F, H, generator=gen, dtype=torch.float32) for _ in range(2))
    if B >= 2:
        edge = torch.ones(F)
        edge[:64] = 8.0
        edge[-64:] = 8.0
        h, dpre = h * edge[None, :, None], dpre * edge[None, :, None]
    return dict(h=h.to(torch.bfloat16).to(F64), dpre=dpre.to(torch.bfloat16).to(F64))


def weights_case(H, G, K):
    """The weights of one geometry in every real-valued kernel test, with w = bf16(weight(g, v)): the reference is fed what the
    kernels are fed."""
    c = real_weights(H + K, H, G, K)
    c["w"] = bf16_values(weight(c["g"], c["v"]))
    return c


def direct_activations(B, F, H, K):
    """h, dpre of the direct kernel's case (B, F) in tests/test_gpu_posconv.py."""
    return real_activations(1000 * B + F + K, B, F, H)


def wgrad_activations(B, F, H, K):
    """h, dpre of the weight gradient's case (B, F) in tests/test_gpu_posconv.py."""
    return real_activations(2000 * B + F + K, B, F, H)


# Accumulation constants of the bars |got - ref| <= 2^-8 |ref| + C_ACC u A (pre, dX) and <= C_WGRAD u A_w (dwf), u = 2^-24.
# Derived from the emulations above, not from the kernels: max |emulation - float64| / (u A) over a sample of the GPU module's
# own cases (same seeds; the shapes, group and taps are listed in tests/test_posconv_ref.py::test_accumulation_constants, which
# measures it again and holds the constants to the rule) is
#   forward / dX (emulate_forward; the input gradient is the same kernel): 1.034   -> 8 * 1.034 = 8.3   -> C_ACC = 16
#   weight gradient (emulate_grad_weight):                                   1.461   -> 8 * 1.461 = 11.7  -> C_WGRAD = 16
# 8 = the allowance for the undocumented rounding inside a 32-term matrix-instruction slice; rounded up to a power of two.
C_ACC = 16
#   weight gradient (emulate_grad_weight):                                   0.970   -> 8 * 0.970 = 7.8  -> C_WGRAD = 8
# 8 = the allowance for the undocumented rounding inside a 32-term matrix-instruction slice; rounded up to a power of two.
C_ACC = 16.0
C_WGRAD = 16.0
