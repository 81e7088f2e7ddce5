"""CPU: tests/frontend_ref.py (the float64 restatement the feature-encoder backward kernels and the Whisper front end's data movers
are held to) against torch under float64 autograd and plain indexing; the accumulation constants against the rule that defines
them; the bars of tests/test_gpu_frontend.py against wrong variants of each operation (same cases, same seeds: a wrong result must
leave the bar at some element); and the argument checks of the test-only entries (host side).

Wrong variants and what catches them (test_bars_bite_*):
  conv0 backward -- the xh mean_t(g xh) term dropped; means divided by T0 - 1 (caught at T0 = 2; at T0 = 2049 the change is
  below the gelu' term of the bar); the last frame of a 1024-frame block skipped; another utterance's mean and rstd; the tap
  index off by one.  col2im -- t >= Tout not excluded; d % s != 0 taken as a hit.  col2im_k3s2 -- pre read without its one-row
  lead.  sum_slabs -- one slab omitted.
  NOT catchable: "samples at or beyond T read as the next utterance's instead of zero".  The entries, like the engine, derive
  T0 = (T - k) / s + 1 from T, so the last frame ends at sample s (T0 - 1) + k - 1 < T: no frame of any conv0 kernel reaches
  sample T, and the `s < T` guard only protects the staging loop's reads past the last window
  (test_no_frame_reaches_past_the_utterance states this).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frontend_ref as F  # noqa: E402
import rowwise_ref as RR  # noqa: E402

T64 = torch.float64
U = F.U


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------------ pins to torch
@pytest.mark.parametrize("C,T0,r,B", [(8, 1, 0, 1), (8, 2, 4, 3), (16, 37, 0, 2), (4, 130, 4, 3)])
def test_conv0_bwd_equals_torch_autograd(C, T0, r, B):
    rng = np.random.default_rng(C + T0 + B)
    T = 5 * (T0 - 1) + 10 + r
    x, w = rng.standard_normal((B, T)), 0.3 * rng.standard_normal((C, 10))
    gamma, beta, dy = 1 + 0.1 * rng.standard_normal(C), 0.1 * rng.standard_normal(C), rng.standard_normal((B, T0, C))
    tw, tg, tb = (torch.tensor(a, dtype=T64, requires_grad=True) for a in (w, gamma, beta))
    v = torch.nn.functional.conv1d(torch.tensor(x)[:, None], tw[:, None], stride=5)
    y = torch.nn.functional.gelu(torch.group_norm(v, C, tg, tb, 1e-5, False))
    y.backward(torch.tensor(dy).transpose(1, 2))
    p = F.conv0_bwd(x, w, gamma, beta, dy, bf16=False)
    assert _rel(p["v"], v.detach().transpose(1, 2).numpy()) < 1e-12
    if T0 > 1:  # (one frame: xh = 0, the gradient of w vanishes identically -- compared absolutely below)
        assert _rel(p["dw"], tw.grad.numpy()) < 1e-9
    assert np.abs(p["dw"] - tw.grad.numpy()).max() < 1e-9
    assert np.abs(p["dgamma"] - tg.grad.numpy()).max() < 1e-10 and np.abs(p["dbeta"] - tb.grad.numpy()).max() < 1e-10
    # the bf16 engine's fit form: its gelu' is within the stated bar of the exact form, at every element
    q = F.conv0_bwd(x, w, gamma, beta, dy, bf16=True)
    bar = F.gelu_grad_bar(True)
    assert bar == RR.PHI_FIT_MAX_ERR + 2.0 ** -20 and F.gelu_grad_bar(False) == 1e-6
    assert (np.abs(q["g"] - p["g"]) <= np.abs(dy) * bar).all()
    assert (np.abs(q["dbeta"] - p["dbeta"]) <= np.abs(dy).sum(axis=(0, 1)) * bar).all()
    # explicit statistics are used as given
    s = F.conv0_bwd(x, w, gamma, beta, dy, bf16=False, stats=(p["mean"], p["rstd"]))
    assert np.array_equal(s["dw"], p["dw"])


def test_conv0_forward_and_weight_gradient_are_direct_sums():
    rng = np.random.default_rng(3)
    for k, s in ((10, 5), (4, 3)):
        B, T0, C = 2, 9, 6
        T = s * (T0 - 1) + k + 2
        x, d, bias = rng.standard_normal((B, T)), rng.standard_normal((B, T0, C)), rng.standard_normal(C)
        tw = torch.tensor(rng.standard_normal((C, k)), requires_grad=True)
        y = torch.nn.functional.conv1d(torch.tensor(x)[:, None], tw[:, None], torch.tensor(bias), stride=s)
        y.backward(torch.tensor(d).transpose(1, 2))
        assert _rel(F.conv0(x, tw.detach().numpy(), bias, k, s), y.detach().transpose(1, 2).numpy()) < 1e-12
        assert _rel(F.conv0_wgrad(d, x, k, s), tw.grad.numpy()) < 1e-12
        assert (F.conv0_wgrad_abs_sum(d, x, k, s) >= np.abs(F.conv0_wgrad(d, x, k, s)) * (1 - 1e-12)).all()
        assert (F.conv0_abs_sum(x, tw.detach().numpy(), bias, k, s) >= np.abs(y.detach().transpose(1, 2).numpy()) * (1 - 1e-12)).all()


@pytest.mark.parametrize("k,s", [(3, 2), (2, 2), (10, 5)])
@pytest.mark.parametrize("Tout,r,B", [(1, 0, 1), (2, 1, 3), (13, 1, 2)])
def test_col2im_equals_torch_autograd(k, s, Tout, r, B):
    """col2im(dy @ Wr) is the input gradient of the channels-last Conv1d(k, s)."""
    rng = np.random.default_rng(k + s + Tout)
    Ci, Co, Tin = 8, 5, (Tout - 1) * s + k + r
    W, dy = rng.standard_normal((Co, Ci, k)), rng.standard_normal((B, Tout, Co))
    h = torch.tensor(rng.standard_normal((B, Tin, Ci)), requires_grad=True)
    torch.nn.functional.conv1d(h.transpose(1, 2), torch.tensor(W), stride=s).backward(torch.tensor(dy).transpose(1, 2))
    Wr = F.weight_rearrange(W)
    for co in range(Co):
        for kk in range(k):
            assert np.array_equal(Wr[co, kk], W[co, :, kk])
    dxcol = (dy @ Wr.reshape(Co, k * Ci)).reshape(B, Tout, k, Ci)
    dx = F.col2im(dxcol, Tin, s)
    assert np.abs(dx - h.grad.numpy()).max() < 1e-12
    if r:
        assert (dx[:, (Tout - 1) * s + k:] == 0).all()


@pytest.mark.parametrize("Tin,B", [(2, 1), (3, 3), (10, 2), (11, 2)])
def test_col2im_k3s2_equals_torch_autograd(Tin, B):
    rng = np.random.default_rng(Tin)
    H, Co, Fr = 8, 5, (Tin + 1) // 2
    W, dy = rng.standard_normal((Co, H, 3)), rng.standard_normal((B, Fr, Co))
    pre = torch.tensor(rng.standard_normal((B, Tin, H)), requires_grad=True)
    y = torch.nn.functional.conv1d(torch.nn.functional.gelu(pre).transpose(1, 2), torch.tensor(W), stride=2, padding=1)
    assert y.shape[2] == Fr
    y.backward(torch.tensor(dy).transpose(1, 2))
    dxcol = (dy @ F.weight_rearrange(W).reshape(Co, 3 * H)).reshape(B, Fr, 3, H)
    RS1 = Tin + 3
    out, acc, aacc, gp = F.col2im_k3s2(dxcol, pre.detach().numpy(), Tin, RS1, bf16=False)
    assert np.abs(out[:, :Tin] - pre.grad.numpy()).max() < 1e-12 and (out[:, Tin:] == 0).all()
    assert (aacc >= np.abs(acc) * (1 - 1e-12)).all() and np.array_equal(out[:, :Tin], acc * gp)
    buf = F.pre_with_lead(pre.detach().numpy(), RS1, 9.0)
    for b in range(B):
        assert np.array_equal(buf[b * RS1 + 1:b * RS1 + 1 + Tin], pre.detach().numpy()[b]) and (buf[b * RS1] == 9.0).all()


def test_movers_follow_their_index_maps():
    rng = np.random.default_rng(0)
    B, C, T, RS, lead = 3, 5, 7, 10, 1
    mel, cl0 = rng.standard_normal((B, C, T)), np.full((B * RS + 2, C), -7.0)
    cl = F.mel_to_cl(mel, cl0, RS, lead)
    want = cl0.copy()
    for b in range(B):
        for t in range(T):
            for c in range(C):
                want[b * RS + lead + t, c] = mel[b, c, t]
    assert np.array_equal(cl, want)
    x, pos = rng.standard_normal((B, T, C)), rng.standard_normal((T, C))
    assert all(np.array_equal(F.add_rowvec(x, pos)[b, t], x[b, t] + pos[t]) for b in range(B) for t in range(T))
    pad = F.copy_rows_padded(x, RS)
    assert pad.shape == (B, RS, C) and np.array_equal(pad[:, :T], x) and (pad[:, T:] == 0).all()
    w, g = rng.standard_normal((4, 3, 2)), rng.standard_normal((4, 3, 2))
    wr = F.weight_rearrange(w)
    un = F.wgrad_unrearrange(wr, g)
    for co in range(4):
        for ci in range(3):
            for k in range(2):
                assert wr[co, k, ci] == w[co, ci, k] and un[co, ci, k] == g[co, ci, k] + w[co, ci, k]
    sl = rng.standard_normal((5, 11))
    assert np.allclose(F.sum_slabs(sl), sum(sl[b] for b in range(5)), rtol=1e-15, atol=0)
    ints = F.slabs_case(3, 100, True)
    assert np.array_equal(F.emulate_sum_slabs(ints).astype(np.float64), F.sum_slabs(ints))


def test_no_frame_reaches_past_the_utterance():
    """Why `samples at or beyond T read as the next utterance's` cannot be caught: with T0 derived from T no window reaches T."""
    for k, s in ((10, 5), (4, 3)):
        for T in range(k, k + 40):
            T0 = (T - k) // s + 1
            assert s * (T0 - 1) + k - 1 < T
    for C, T0, r, B in F.CONV0_BWD_SHAPES:
        c = F.conv0_bwd_case(C, T0, r, B, True) if T0 <= 2 else None
        if c is not None:
            assert F.windows(c["x"]).shape[1] == T0 and c["x"].shape[1] == 5 * (T0 - 1) + 10 + r


# ------------------------------------------------------------------------------------------------ accumulation constants
DT2 = (True, False)
BWD_CASES = tuple((sh, bf) for sh in F.CONV0_BWD_SHAPES for bf in DT2)
WGRAD_CASES = tuple((sh, bf) for sh in F.CONV0_WGRAD_SHAPES for bf in DT2)
BIAS_CASES = F.CONV0_BIAS_SHAPES


def test_accumulation_constants():
    """Every constant is 4 x max |fp32-order emulation - float64| / (u sum |terms|) over ALL real-valued cases of the GPU module
    (every shape at both storage types, seed for seed), rounded up to a power of two; the measured ratios are the ones
    frontend_ref.py records."""
    m = dict(xhat=0.0, gsum=0.0, dw=0.0, wgrad=0.0, bias=0.0)

    def ratio(em, ref, a):
        err = np.abs(em.astype(np.float64) - ref)
        assert (err[a == 0] == 0).all()  # (no terms, e.g. xh = 0 at T0 = 1: the sum is exactly zero)
        return float((err[a > 0] / (U * a[a > 0])).max(initial=0.0))

    for (C, T0, r, B), bf in BWD_CASES:
        c = F.conv0_bwd_case(C, T0, r, B, bf)
        p = F.conv0_bwd(c["x"], c["w"], c["gamma"], c["beta"], c["dy"], bf)
        S = np.abs(p["win"]) @ np.abs(p["w"]).T
        den = U * (S + np.abs(p["mean"])[:, None]) * p["rstd"][:, None]
        exh = np.abs(F.emulate_xhat(p).astype(np.float64) - p["xh"])
        m["xhat"] = max(m["xhat"], float((np.maximum(exh - 2 * U * np.abs(p["xh"]), 0.0) / den).max()))
        db, dg, dw = F.emulate_conv0_bwd_sums(p)
        ag = np.abs(p["g"])
        m["gsum"] = max(m["gsum"], ratio(db, p["dbeta"], ag.sum(axis=(0, 1))), ratio(dg, p["dgamma"], (ag * np.abs(p["xh"])).sum(axis=(0, 1))))
        m["dw"] = max(m["dw"], ratio(dw, p["dw"], np.einsum("btc,btk->ck", np.abs(p["dv"]), np.abs(p["win"]))))
    for (C, T0, B, k, s), bf in WGRAD_CASES:
        c = F.conv0_wgrad_case(C, T0, B, k, s, bf, False)
        m["wgrad"] = max(m["wgrad"], ratio(F.emulate_conv0_wgrad(c["d"], c["x"], k, s), F.conv0_wgrad(c["d"], c["x"], k, s),
                                           F.conv0_wgrad_abs_sum(c["d"], c["x"], k, s)))
    for C, T0, B in BIAS_CASES:
        c = F.conv0_bias_case(C, T0, B, False)
        m["bias"] = max(m["bias"], ratio(F.emulate_dot(F.windows(c["x"]), c["w"], c["bias"]), F.conv0(c["x"], c["w"], c["bias"]),
                                         F.conv0_abs_sum(c["x"], c["w"], c["bias"])))
    print("measured:", {k: round(v, 4) for k, v in m.items()})
    for k, const in (("xhat", F.C_XHAT), ("gsum", F.C_GSUM), ("dw", F.C_DW), ("wgrad", F.C_WGRAD), ("bias", F.C_BIAS)):
        assert F._pow2_ceil(4 * m[k]) == const, (k, m[k], const)
        assert abs(m[k] - F.MEASURED[k]) < 5e-3, (k, m[k], F.MEASURED[k])
    # the emulations themselves are exact on integers and stay within the bars they define
    c = F.conv0_wgrad_case(64, 33, 3, 10, 5, True, True)
    assert np.array_equal(F.emulate_conv0_wgrad(c["d"], c["x"]).astype(np.float64), F.conv0_wgrad(c["d"], c["x"]))


# ------------------------------------------------------------------------------------------------ the bars bite
def _wrong_conv0_bwd(c, bf16, variant):
    x, w, gamma, beta, dy = c["x"], c["w"], c["gamma"], c["beta"], c["dy"]
    p = F.conv0_bwd(x, w, gamma, beta, dy, bf16)
    B, T0, _ = dy.shape
    win = p["win"]
    if variant == "tap_off_by_one":
        win = F.windows(np.concatenate([x[:, 1:], np.zeros((B, 1))], axis=1))
    mean, rstd = p["mean"], p["rstd"]
    if variant == "other_utterance_stats":
        mean, rstd = np.roll(mean, 1, axis=0), np.roll(rstd, 1, axis=0)
    xh = (win @ w.T - mean[:, None]) * rstd[:, None]
    g = dy * RR.gelu_forms(bf16)[1](gamma * xh + beta)
    keep = np.ones(T0)
    if variant == "last_frame_of_block":
        keep[F.FR_STATS - 1::F.FR_STATS] = 0.0
    keep = keep[None, :, None]
    div = T0 - 1 if variant == "t0_minus_1" else T0
    m1, m2 = (g * keep).sum(axis=1) / div, (g * xh * keep).sum(axis=1) / div
    dv = gamma * rstd[:, None] * (g - m1[:, None] - (0.0 if variant == "mean_term_dropped" else xh * m2[:, None])) * keep
    return p, dict(dbeta=(g * keep).sum(axis=(0, 1)), dgamma=(g * xh * keep).sum(axis=(0, 1)), dw=np.einsum("btc,btk->ck", dv, win))


@pytest.mark.parametrize("variant,shape,bf16", [
    ("mean_term_dropped", (512, 129, 0, 3), True), ("t0_minus_1", (512, 2, 4, 1), True), ("t0_minus_1", (64, 2, 0, 3), False),
    ("last_frame_of_block", (512, 1024, 0, 3), True), ("last_frame_of_block", (512, 1024, 0, 3), False),
    ("other_utterance_stats", (512, 129, 0, 3), True), ("tap_off_by_one", (512, 129, 0, 3), False),
    ("tap_off_by_one", (8, 129, 4, 3), True)])
def test_bars_bite_conv0_bwd(variant, shape, bf16):
    C = shape[0]
    c = F.conv0_bwd_case(*shape, bf16)
    p, wrong = _wrong_conv0_bwd(c, bf16, variant)
    bars = F.conv0_bwd_bars(p, bf16)
    dw0, dg0, db0 = F.start_values(C, (C, 10), (C,), (C,))
    out = 0
    for k, start in (("dw", dw0), ("dgamma", dg0), ("dbeta", db0)):
        assert np.isfinite(bars[k]).all() and (bars[k] >= 0).all()
        out += int((np.abs(wrong[k] - p[k]) > bars[k] + 2.0 ** -23 * (np.abs(start) + np.abs(p[k]))).sum())
    assert out > 0, f"{variant} stays inside every bar"


@pytest.mark.parametrize("k,s,C,Tout,r,B", [(3, 2, 512, 199, 1, 3), (10, 5, 32, 2, 1, 3), (3, 2, 8, 1, 1, 3)])
def test_bars_bite_col2im_tout(k, s, C, Tout, r, B):
    """t >= Tout not excluded: row (Tout - 1) s + k takes the next utterance's first window (its own storage continues there)."""
    d = F.col2im_case(k, s, C, Tout, r, B, True, False)
    Tin = (Tout - 1) * s + k + r
    flat = np.concatenate([d.reshape(B * Tout, k, C), np.zeros((k, k, C))])
    wrong = np.zeros((B, Tin, C))
    for b in range(B):
        for u in range(Tin):
            for kk in range(k):
                dd = u - kk
                if dd >= 0 and dd % s == 0:
                    wrong[b, u] += flat[b * Tout + dd // s, kk]
    assert (RR.round_bf16(wrong) != RR.round_bf16(F.col2im(d, Tin, s))).any()


@pytest.mark.parametrize("k,s,C,Tout,r,B", [(3, 2, 8, 2, 0, 1), (10, 5, 32, 199, 1, 1)])
def test_bars_bite_col2im_stride(k, s, C, Tout, r, B):
    """d % s != 0 taken as a hit (t = d / s rounded down)."""
    d = F.col2im_case(k, s, C, Tout, r, B, False, True)
    Tin = (Tout - 1) * s + k + r
    wrong = np.zeros((B, Tin, C))
    for u in range(Tin):
        for kk in range(k):
            if u - kk >= 0 and (u - kk) // s < Tout:
                wrong[:, u] += d[:, (u - kk) // s, kk]
    assert (wrong != F.col2im(d, Tin, s)).any()


@pytest.mark.parametrize("H,Tin,B,bf16", [(8, 3, 1, True), (384, 100, 3, False)])
def test_bars_bite_col2im_k3s2_lead(H, Tin, B, bf16):
    dxcol, pre = F.col2im_k3s2_case(H, Tin, B, bf16)
    RS1 = 2 * ((((Tin + 1) // 2) + 1 + 3) // 4 * 4)
    out, acc, aacc, gp = F.col2im_k3s2(dxcol, pre, Tin, RS1, bf16)
    buf = F.pre_with_lead(pre, RS1, 0.0).reshape(B, RS1, H)
    wrong = acc * RR.gelu_forms(bf16)[1](buf[:, :Tin])  # row u read at b RS1 + u
    bar = (2.0 ** -8 if bf16 else U) * np.abs(out[:, :Tin]) + 4 * U * aacc * np.abs(gp) + np.abs(acc) * F.gelu_grad_bar(bf16)
    assert (np.abs(wrong - out[:, :Tin]) > bar).any()


def test_bars_bite_sum_slabs():
    for nb, n, integer in ((3, 8 * 8 * 3, True), (32, 5 * 7 * 2, False)):
        sl = F.slabs_case(nb, n, integer)
        ref = F.emulate_sum_slabs(sl)
        for omit in (0, nb // 2, nb - 1):
            assert (F.emulate_sum_slabs(np.delete(sl, omit, axis=0)) != ref).any()


# ------------------------------------------------------------------------------------------------ the entries' argument checks
def test_debug_entries_reject_without_gpu_compute():
    """Argument validation of the ssak_debug_* entries of ABI 570 happens on the host, before any launch."""
    import ssak_amd.hip as h
    L = h.lib
    ws = ctypes.c_void_p(16)  # never dereferenced: every call below is rejected first
    INV = h.SSAK_ERR_INVALID
    # conv0 backward: [B][nblk][C / 4][40] partials + [B][C][2] doubles
    assert L.ssak_debug_conv0_bwd_workspace_bytes(3, 5 * 2048 + 10, 512) >= (3 * 3 * 128 * 40 + 3 * 512 * 4) * 4
    assert L.ssak_debug_conv0_bwd_workspace_bytes(1, 9, 512) == 0 and L.ssak_debug_conv0_bwd_workspace_bytes(1, 100, 24) == 0
    big = 1 << 40
    assert L.ssak_debug_conv0_bwd(ws, ws, ws, ws, ws, ws, ws, ws, ws, 1, 100, 512, 2, ws, big, None) == INV
    assert L.ssak_debug_conv0_bwd(ws, ws, ws, ws, ws, None, ws, ws, ws, 1, 100, 512, 0, ws, big, None) == INV
    assert L.ssak_debug_conv0_bwd(ws, ws, ws, ws, ws, ws, ws, ws, ws, 1, 100, 24, 0, ws, big, None) == INV
    assert L.ssak_debug_conv0_bwd(ws, ws, ws, ws, ws, ws, ws, ws, ws, 1, 9, 512, 0, ws, big, None) == INV
    assert L.ssak_debug_conv0_bwd(ws, ws, ws, ws, ws, ws, ws, ws, ws, 1, 100, 512, 0, ws, 64, None) == INV
    assert b"workspace" in L.ssak_last_error()
    assert L.ssak_debug_conv0_wgrad_workspace_bytes(3, 512, 10) == 3 * 32 * 512 * 10 * 4
    assert L.ssak_debug_conv0_wgrad(ws, ws, ws, 1, 100, 1024, 10, 5, 0, ws, big, None) == INV
    assert L.ssak_debug_conv0_wgrad(ws, ws, ws, 1, 100, 64, 11, 5, 0, ws, big, None) == INV
    assert L.ssak_debug_conv0_wgrad(ws, ws, ws, 1, 100, 64, 10, 6, 0, ws, big, None) == INV
    assert L.ssak_debug_conv0_wgrad(ws, ws, ws, 1, 100, 63, 10, 5, 1, ws, big, None) == INV
    assert L.ssak_debug_conv0_wgrad(ws, ws, ws, 1, 100, 64, 10, 5, 0, ws, 64, None) == INV
    assert L.ssak_debug_conv0_bias(ws, ws, None, None, 1, 100, 512, 0, None) == INV
    assert L.ssak_debug_conv0_bias(ws, ws, None, ws, 1, 100, 20, 0, None) == INV
    assert L.ssak_debug_col2im(ws, ws, 1, 5, 2, 12, 3, 2, 0, None) == INV and b"multiple of 8" in L.ssak_last_error()
    assert L.ssak_debug_col2im(ws, ws, 0, 5, 2, 8, 3, 2, 0, None) == INV
    assert L.ssak_debug_sum_slabs(ws, 0, 10, ws, None) == INV and L.ssak_debug_sum_slabs(None, 1, 10, ws, None) == INV
    assert L.ssak_debug_conv_weight_rearrange(ws, ws, 4, 4, 3, 3, None) == INV
    assert L.ssak_debug_conv_wgrad_unrearrange(ws, None, 4, 4, 3, None) == INV
    assert L.ssak_debug_col2im_k3s2(ws, ws, ws, 1, 50, 100, 100, 384, 0, None) == INV  # RS1 must exceed Tin
    assert L.ssak_debug_col2im_k3s2(ws, ws, ws, 1, 49, 100, 104, 384, 0, None) == INV  # F = (Tin + 1) / 2
    assert L.ssak_debug_col2im_k3s2(ws, ws, ws, 1, 50, 100, 104, 380, 0, None) == INV
    assert L.ssak_debug_mel_to_cl(ws, ws, 1, 80, 100, 100, 1, 0, None) == INV  # RS >= lead + T
    assert L.ssak_debug_add_rowvec(ws, ws, ws, 1, 10, 12, 0, None) == INV
    assert L.ssak_debug_copy_rows_padded(ws, ws, 1, 10, 9, 8, 0, None) == INV
