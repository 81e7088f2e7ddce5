"""GPU: the four LoRA kernels (ssak_amd/csrc/whisper_lora.hip) against the float64 restatements of tests/whisper_lora_ref.py, each a
function of the kernel's OWN inputs (the device's bf16 operands, the site's keep bits from ssak_debug_dropout_mask).

Bars, per element, by the method of tests/test_gpu_whisper_train_kernels.py: u8 = 2^-8 of the result per bf16 store, and
(T + c) u (u = 2^-24) of the sum of the terms' magnitudes per fp32 accumulation, T and c counted from the kernel's summation order.
Any order of adding n fp32 terms is within (n - 1) u sum |terms| of the exact sum, and an accumulation is at most as deep as its
longest chain: a 16x16x32 MFMA adds 32 products in an order of its own (depth <= 32) and then its accumulator (one more), so a K
loop of T steps is a chain of at most T + 32 roundings; c = 32 + 2 adds the multiplication by the scale (s, or 1 / (1 - p)) and the
final addition (of y, of dx) or a spare.
  t   = bf16(scale * xd-sum):   T = D_in / 32 steps                      (T + 34) u sum |xd| |A|          + u8 |t|
  y   = bf16(y + s t B^T):      T = ceil(r / 32), from the ROUNDED t     (T + 34) u (|y| + s |t| |B|^T)   + u8 |y|
  dt  = bf16(s dy B):           T = D_out / 32                           (T + 34) u s |dy| |B|            + u8 |dt|
  dx  = bf16(dx + keep dt A /(1-p)): T = ceil(r / 32), ROUNDED dt        (T + 34) u (|dx| + |dt| |A| /(1-p)) + u8 |dx|
  dB, dA (fp32, no bf16 store): a first-stage partial walks its 512 rows 32 at a time (16 steps), the second stage adds the P
                                partials in order and scales:            (16 + P + 34) u (magnitude sum)
  merge = bf16(W + s sum_j B A): r FMAs in a chain, the scale, the add   (r + 2) u (|W| + s |B| |A|)      + u8 |out|
Integer cases (small-integer operands, p = 0.5 so that 1 / (1 - p) = 2): every fp32 sum is exact, so the device must produce the
correctly rounded result bit for bit.  Every test prints its worst error / bar before it asserts.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import whisper_lora_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U, U8 = 2.0 ** -24, 2.0 ** -8
PART_ROWS = 512
M_PARTS = 3 * PART_ROWS + 37  # three whole first-stage partials of bwd_weights and a remainder
SEED, SITE = 0x1234_5678_9ABC_DEF0, 4096 + 5


def bf(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).to(DEV)


def f64(t):
    return t.double().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def block(values):
    """``values`` [M, D] as the middle column block of a [M, 3 D] bf16 tensor whose other columns are NaN -> (whole, block view)."""
    M, D = values.shape
    whole = torch.full((M, 3 * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    whole[:, D:2 * D] = bf(values)
    return whole, whole[:, D:2 * D]


def untouched(whole, before, D):
    a, b = bits(whole), bits(before)
    return np.array_equal(a[:, :D], b[:, :D]) and np.array_equal(a[:, 2 * D:], b[:, 2 * D:])


def keep_of(p, M, D_in, seed=SEED, site=SITE):
    from ssak_amd import hip
    if p == 0:
        return None, 1.0
    keep, scale = hip.debug_dropout_mask(seed, site, p, M, D_in, DEV)
    assert abs(scale - LR.drop_scale(p)) <= 2.0 ** -22 * scale  # (the library's fp32 value; the references below use it)
    return keep.cpu().numpy().astype(np.float64), float(scale)


def report(what, got, want, bar):
    err = np.abs(got - want)
    worst = float((err / np.maximum(bar, 1e-300)).max())
    print(f"{what}: worst |err| {float(err.max()):.3e}, worst err/bar {worst:.3f}")
    return worst


CASES = [(128, 128, r, M, p) for r in (8, 32) for M in (1, 37, M_PARTS) for p in (0.0, 0.05, 0.5)]
CASES += [(768, 768, 32, 300, 0.05), (128, 256, 8, 37, 0.05), (256, 128, 64, 37, 0.05), (128, 128, 16, 37, 0.5), (128, 128, 64, 37, 0.0)]


@pytest.mark.parametrize("D_in,D_out,r,M,p", CASES)
def test_training_kernels_against_float64(D_in, D_out, r, M, p):
    from ssak_amd import hip
    rng = np.random.default_rng(D_in + 7 * D_out + 13 * r + M)
    s = 2.0  # lora_alpha / r of the reference
    A, B = bf(rng.standard_normal((r, D_in)) / math.sqrt(D_in)), bf(rng.standard_normal((D_out, r)) * 0.1)
    x_whole, x = block(rng.standard_normal((M, D_in)))
    y_whole, y = block(rng.standard_normal((M, D_out)))
    dy_whole, dy = block(rng.standard_normal((M, D_out)) * 0.01)
    dx_whole, dx = block(rng.standard_normal((M, D_in)) * 0.01)
    fresh_whole, fresh = block(np.full((M, D_in), np.nan))
    keep, scale = keep_of(p, M, D_in)
    An, Bn, xn, y0, dyn, dx0 = f64(A), f64(B), f64(x), f64(y), f64(dy), f64(dx)
    KS, P = math.ceil(r / 32), math.ceil(M / PART_ROWS)
    worst = {}
    # ---- forward
    t = torch.full((M, r), float("nan"), dtype=torch.bfloat16, device=DEV)
    y_before = y_whole.clone()
    hip.lora_fwd(x, A, B, y, s, t=t, seed=SEED, site=SITE, drop_p=p)
    torch.cuda.synchronize()
    want, mag = LR.lora_fwd_t(xn, An, keep, scale)
    worst["t"] = report("t", f64(t), want, (D_in // 32 + 34) * U * mag + U8 * np.abs(want))
    tn = f64(t)
    want, mag = LR.lora_fwd_y(y0, tn, Bn, s)
    worst["y"] = report("y", f64(y), want, (KS + 34) * U * mag + U8 * np.abs(want))
    assert untouched(y_whole, y_before, D_out), "lora_fwd wrote outside its column block"
    # the validation pass: no t, the same y
    y2_whole, y2 = block(y0)
    hip.lora_fwd(x, A, B, y2, s, t=None, seed=SEED, site=SITE, drop_p=p)
    assert np.array_equal(bits(y2), bits(y)), "t = None changes y"
    # ---- input gradient
    dt = torch.full((M, r), float("nan"), dtype=torch.bfloat16, device=DEV)
    dx_before, dy_before = dx_whole.clone(), dy_whole.clone()
    hip.lora_bwd_input(dy, A, B, dt, s, dx=dx, accumulate=True, seed=SEED, site=SITE, drop_p=p)
    torch.cuda.synchronize()
    want, mag = LR.lora_bwd_dt(dyn, Bn, s)
    worst["dt"] = report("dt", f64(dt), want, (D_out // 32 + 34) * U * mag + U8 * np.abs(want))
    dtn = f64(dt)
    want, mag = LR.lora_bwd_dx(dtn, An, keep, scale, dx0)
    worst["dx+="] = report("dx (accumulate)", f64(dx), want, (KS + 34) * U * mag + U8 * np.abs(want))
    assert untouched(dx_whole, dx_before, D_in) and np.array_equal(bits(dy_whole), bits(dy_before))
    dt2 = torch.empty_like(dt)
    hip.lora_bwd_input(dy, A, B, dt2, s, dx=fresh, accumulate=False, seed=SEED, site=SITE, drop_p=p)
    want, mag = LR.lora_bwd_dx(dtn, An, keep, scale)
    worst["dx="] = report("dx (written)", f64(fresh), want, (KS + 34) * U * mag + U8 * np.abs(want))
    assert np.array_equal(bits(dt2), bits(dt)) and bool(torch.isnan(fresh_whole[:, :D_in]).all()) and bool(torch.isnan(fresh_whole[:, 2 * D_in:]).all())
    dt3 = torch.empty_like(dt)
    hip.lora_bwd_input(dy, A, B, dt3, s, dx=None, seed=SEED, site=SITE, drop_p=p)  # (the cross v_proj: no input gradient)
    assert np.array_equal(bits(dt3), bits(dt))
    # ---- weight gradients, written (the buffers start as NaN), twice the same bits
    out = []
    for _ in range(2):
        dA = torch.full((r, D_in), float("nan"), dtype=torch.float32, device=DEV)
        dB = torch.full((D_out, r), float("nan"), dtype=torch.float32, device=DEV)
        hip.lora_bwd_weights(dy, t, dt, x, dA, dB, s, seed=SEED, site=SITE, drop_p=p)
        torch.cuda.synchronize()
        out.append((dA, dB))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1])), "two runs differ"
    wB, wA, mB, mA = LR.lora_bwd_weights(dyn, tn, dtn, xn, s, keep, scale)
    worst["dB"] = report("dB", f64(out[0][1]), wB, (16 + P + 34) * U * mB)
    worst["dA"] = report("dA", f64(out[0][0]), wA, (16 + P + 34) * U * mA)
    assert np.abs(wB).max() > 0 and np.abs(wA).max() > 0
    assert all(v <= 1.0 for v in worst.values()), worst


def rne_bf16_bits(a):
    return bits(torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16))


@pytest.mark.parametrize("r", (8, 64))
def test_integer_cases_are_bit_exact(r):
    """Small-integer operands, s = 2, p = 0.5 (scale 2): every product and fp32 sum is an integer below 2^24."""
    from ssak_amd import hip
    D_in, D_out, M, p, s = 128, 128, M_PARTS, 0.5, 2.0
    rng = np.random.default_rng(r)
    A, B = bf(rng.integers(-1, 2, (r, D_in))), bf(rng.integers(-1, 2, (D_out, r)))
    x, y = bf(rng.integers(-2, 3, (M, D_in))), bf(rng.integers(-8, 9, (M, D_out)))
    dy, dx = bf(rng.integers(-2, 3, (M, D_out))), bf(rng.integers(-8, 9, (M, D_in)))
    keep, scale = keep_of(p, M, D_in)
    assert scale == 2.0
    An, Bn, xn, y0, dyn, dx0 = f64(A), f64(B), f64(x), f64(y), f64(dy), f64(dx)
    t, dt = torch.empty((M, r), dtype=torch.bfloat16, device=DEV), torch.empty((M, r), dtype=torch.bfloat16, device=DEV)
    hip.lora_fwd(x, A, B, y, s, t=t, seed=SEED, site=SITE, drop_p=p)
    assert np.array_equal(bits(t), rne_bf16_bits(LR.lora_fwd_t(xn, An, keep, scale)[0])), "t"
    tn = f64(t)
    assert np.array_equal(bits(y), rne_bf16_bits(LR.lora_fwd_y(y0, tn, Bn, s)[0])), "y"
    hip.lora_bwd_input(dy, A, B, dt, s, dx=dx, accumulate=True, seed=SEED, site=SITE, drop_p=p)
    assert np.array_equal(bits(dt), rne_bf16_bits(LR.lora_bwd_dt(dyn, Bn, s)[0])), "dt"
    dtn = f64(dt)
    assert np.array_equal(bits(dx), rne_bf16_bits(LR.lora_bwd_dx(dtn, An, keep, scale, dx0)[0])), "dx"
    dA, dB = torch.empty((r, D_in), dtype=torch.float32, device=DEV), torch.empty((D_out, r), dtype=torch.float32, device=DEV)
    hip.lora_bwd_weights(dy, t, dt, x, dA, dB, s, seed=SEED, site=SITE, drop_p=p)
    wB, wA, mB, mA = LR.lora_bwd_weights(dyn, tn, dtn, xn, s, keep, scale)
    assert max(mB.max(), mA.max()) < 2 ** 24
    print(f"integer case r = {r}: largest |t| {np.abs(tn).max():.0f}, |dB| {np.abs(wB).max():.0f}, |dA| {np.abs(wA).max():.0f}")
    assert np.array_equal(f64(dB), wB) and np.array_equal(f64(dA), wA)


def test_the_mask_is_the_sites_mask():
    """dt = the first unit vector in every row and A's first row without a zero: dx is zero exactly where the site drops."""
    from ssak_amd import hip
    D, r, M, p = 128, 8, 37, 0.5
    A = np.zeros((r, D))
    A[0] = 1 + np.arange(D) % 3
    B = np.zeros((D, r))
    B[0, 0] = 1
    dy = np.zeros((M, D))
    dy[:, 0] = 1
    zeros = {}
    for seed, site in ((SEED, SITE), (SEED, SITE + 1), (SEED + 1, SITE)):
        dx = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device=DEV)
        dt = torch.empty((M, r), dtype=torch.bfloat16, device=DEV)
        hip.lora_bwd_input(bf(dy), bf(A), bf(B), dt, 1.0, dx=dx, seed=seed, site=site, drop_p=p)
        assert np.array_equal(f64(dt), np.eye(r)[np.zeros(M, dtype=int)])
        keep = hip.debug_dropout_mask(seed, site, p, M, D, DEV)[0].cpu().numpy().astype(bool)
        z = f64(dx) == 0
        assert np.array_equal(z, ~keep), (seed, site)
        assert np.array_equal(f64(dx)[keep], np.broadcast_to(2 * A[0], (M, D))[keep])
        zeros[(seed, site)] = z
    print("dropped fractions:", {k: float(v.mean()) for k, v in zeros.items()})
    base = zeros[(SEED, SITE)]
    assert not np.array_equal(base, zeros[(SEED, SITE + 1)]) and not np.array_equal(base, zeros[(SEED + 1, SITE)])
    # the forward reads the same bits: x = 1, A = the first unit row -> t[:, 0] = 2 * the kept columns that A's first row selects
    x = np.ones((M, D))
    A1 = np.zeros((r, D))
    A1[0] = 1
    t = torch.empty((M, r), dtype=torch.bfloat16, device=DEV)
    y = torch.zeros((M, D), dtype=torch.bfloat16, device=DEV)
    hip.lora_fwd(bf(x), bf(A1), bf(B), y, 1.0, t=t, seed=SEED, site=SITE, drop_p=p)
    assert np.array_equal(f64(t)[:, 0], 2.0 * (~base).sum(1))


@pytest.mark.parametrize("D_in,D_out,r", [(128, 128, 8), (768, 768, 32), (128, 256, 16), (512, 128, 64)])
def test_merge_against_float64(D_in, D_out, r):
    from ssak_amd import hip
    rng = np.random.default_rng(r)
    s = 2.0
    W = torch.from_numpy(rng.standard_normal((D_out, D_in)).astype(np.float32) * 0.05).to(DEV)
    A = torch.from_numpy((rng.standard_normal((r, D_in)) / math.sqrt(D_in)).astype(np.float32)).to(DEV)
    B = torch.from_numpy(rng.standard_normal((D_out, r)).astype(np.float32) * 0.1).to(DEV)
    out = torch.full((D_out, D_in), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.lora_merge(W, A, B, out, s)
    want, mag = LR.lora_merge(f64(W), f64(A), f64(B), s)
    worst = report(f"merge {D_out} x {D_in}, r = {r}", f64(out), want, (r + 2) * U * mag + U8 * np.abs(want))
    assert worst <= 1.0
    f32 = torch.empty_like(W)
    out2 = torch.empty_like(out)
    hip.lora_merge(W, A, B, out2, s, w_out_f32=f32)
    assert np.array_equal(bits(out2), bits(out)) and np.array_equal(bits(f32.to(torch.bfloat16)), bits(out))
    # B = 0: the shadow of W itself
    hip.lora_merge(W, A, torch.zeros_like(B), out2, s)
    assert np.array_equal(bits(out2), bits(W.to(torch.bfloat16)))


def test_unmerge_restores_the_shadow_bit_for_bit(tmp_path):
    import gen_golden_whisper_dec as G
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    m = WhisperSeq2Seq.from_pretrained(G.write_folder(np.load(G.GOLDEN), str(tmp_path / "tiny")))
    m.add_lora(r=8, alpha=16, dropout=0.0, seed=3)
    m.load_lora_state_dict({k: torch.from_numpy(v.astype(np.float32)) for k, v in LR.random_lora(G.LAYERS, G.D, 8, seed=1).items()})
    before = m.dec_shadow.clone()
    with m.lora_merged():
        torch.cuda.synchronize()
        changed = [n for n in m.layout if not torch.equal(m._w(n[len("model.decoder."):]).view(torch.int16),
                                                          before[m.layout[n][0]:m.layout[n][0] + m.layout[n][1]].view(m.layout[n][2]).view(torch.int16))]
        assert sorted(changed) == sorted(w for w, _, _ in m._lora_targets()), changed
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int16), m.dec_shadow.view(torch.int16)) and not m._lora_merged
