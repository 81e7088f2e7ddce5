"""Float64 numpy restatement of the augmentation contract of ssak_amd/augment.py (kernels: ssak_amd/csrc/augment.hip).

* ``reverb``: checked on the CPU against the reference's own ``Reverberation._reverberate`` (tests/golden/augment_reverb.npz,
  made by tests/gen_golden_augment.py).
* ``time_stretch``: librosa.effects.time_stretch spelled out for librosa >= 0.10 defaults -- parity with librosa unpinned (librosa
  absent); ``stft`` and ``istft`` are pinned to torch.stft / torch.istft in float64 (tests/test_augment_ref.py).
* ``noise_mix``: audiomentations' AddBackgroundNoise (relative RMS) -- parity unpinned (audiomentations absent).
* ``gain``: in float32, as audiomentations computes it (float32 samples times a Python float).
* ``reverb_f32`` / ``time_stretch_f32``: the same formulas with every array float32 / complex64 (scipy.fft computes in single
  precision for single-precision input).  They are the yardstick of tests/test_gpu_augment_edges.py -- how far careful float32
  arithmetic lands from the float64 restatement on a case -- and never the expected value.
* ``reverb_edge_cases`` / ``gain_noise_edge_cases`` / ``stretch_edge_cases``: the inputs of tests/test_gpu_augment_edges.py, built
  here so that tests/test_augment_ref.py can hold the yardstick to 1e-6 on the very same cases without a GPU.
"""
from __future__ import annotations

import numpy as np

N_FFT, HOP = 2048, 512


def gain(x, gain_lin):
    return (np.asarray(x, dtype=np.float32) * np.float32(gain_lin)).astype(np.float32)


def noise_mix(x, noise, start, snr_amp):
    """y = x + n * (rms(x) / snr_amp) / rms(n), n = noise[start : start + min(L, N)] tiled to L; rms(n) < 1e-9 -> x."""
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    S = min(L, len(noise))
    if L == 0 or S == 0:
        return x.copy()
    seg = np.asarray(noise[start:start + S], dtype=np.float64)
    n_rms = np.sqrt(np.mean(seg ** 2))
    if n_rms < 1e-9:
        return x.copy()
    n = np.tile(seg, -(-L // S))[:L]
    return x + n * (np.sqrt(np.mean(x ** 2)) / snr_amp) / n_rms


def reverb(x, h):
    """augment_reverberation.py _reverberate(rescale_amp="avg") for one mono utterance."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    L = len(x)
    d = int(np.argmax(np.abs(h)))
    ht = h[:L]
    k = np.concatenate([ht[d:], np.zeros(L - len(ht)), ht[:d]])
    conv = np.fft.irfft(np.fft.rfft(x) * np.fft.rfft(k), n=L)
    return conv / (np.mean(np.abs(conv)) + 1e-14) * np.mean(np.abs(x))


def _hann():
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)


def stft(y):
    w = _hann()
    yp = np.pad(np.asarray(y, dtype=np.float64), (N_FFT // 2, N_FFT // 2))
    F = 1 + len(y) // HOP
    frames = np.stack([yp[f * HOP:f * HOP + N_FFT] for f in range(F)], axis=1)
    return np.fft.rfft(frames * w[:, None], axis=0)  # [1025, F]


def phase_vocoder(S, rate):
    F = S.shape[1]
    steps = np.arange(0, F, rate, dtype=np.float64)
    Sp = np.pad(S, [(0, 0), (0, 2)])
    phi = np.linspace(0, np.pi * HOP, S.shape[0])
    acc = np.angle(S[:, 0])
    out = np.zeros((S.shape[0], len(steps)), dtype=np.complex128)
    for t, s in enumerate(steps):
        k = int(np.floor(s))
        a = s - k
        c = Sp[:, k:k + 2]
        mag = (1.0 - a) * np.abs(c[:, 0]) + a * np.abs(c[:, 1])
        out[:, t] = mag * np.exp(1j * acc)
        dp = np.angle(c[:, 1]) - np.angle(c[:, 0]) - phi
        dp = dp - 2.0 * np.pi * np.round(dp / (2.0 * np.pi))
        acc = acc + phi + dp
    return out


def istft(D, length):
    w = _hann()
    n = min(D.shape[1], int(np.ceil((length + N_FFT) / HOP)))
    D = D[:, :n].copy()
    D[0].imag = 0
    D[-1].imag = 0
    frames = np.fft.irfft(D, n=N_FFT, axis=0) * w[:, None]
    total = N_FFT + HOP * (n - 1)
    y = np.zeros(total)
    wss = np.zeros(total)
    for f in range(n):
        y[f * HOP:f * HOP + N_FFT] += frames[:, f]
        wss[f * HOP:f * HOP + N_FFT] += w ** 2
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    y = y[N_FFT // 2:]
    return np.pad(y, (0, max(0, length - len(y))))[:length]


def time_stretch(y, rate):
    L = len(y)
    return istft(phase_vocoder(stft(y), rate), int(round(L / rate)))


def err_max(y, ref):
    """max|y - ref| / max|ref|; max|y| where ref is all zero (0 for empty arrays)."""
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    m = float(np.abs(ref).max())
    return float(np.abs(y - ref).max()) / m if m > 0.0 else float(np.abs(y).max())


# ------------------------------------------------------------------------------------------------ the float32 yardstick
def reverb_f32(x, h):
    """``reverb`` in float32 / complex64; the two mean-|.| sums in float64, the scale rounded once, as in the kernels."""
    import scipy.fft as sfft
    x = np.asarray(x, dtype=np.float32)
    h = np.asarray(h, dtype=np.float32)
    L = len(x)
    d = int(np.argmax(np.abs(h)))
    ht = h[:L]
    k = np.concatenate([ht[d:], np.zeros(L - len(ht), dtype=np.float32), ht[:d]])
    X, K = sfft.rfft(x), sfft.rfft(k)
    assert X.dtype == np.complex64 and K.dtype == np.complex64
    conv = sfft.irfft(X * K, n=L)
    assert conv.dtype == np.float32
    s = np.float32(np.mean(np.abs(x), dtype=np.float64) / (np.mean(np.abs(conv), dtype=np.float64) + 1e-14))
    y = conv * s
    assert y.dtype == np.float32
    return y


def _hann_f32():
    return _hann().astype(np.float32)


def stft_f32(y):
    import scipy.fft as sfft
    w = _hann_f32()
    yp = np.pad(np.asarray(y, dtype=np.float32), (N_FFT // 2, N_FFT // 2))
    F = 1 + len(y) // HOP
    frames = np.stack([yp[f * HOP:f * HOP + N_FFT] for f in range(F)], axis=1) * w[:, None]
    assert frames.dtype == np.float32
    S = sfft.rfft(frames, axis=0)
    assert S.dtype == np.complex64
    return S


def phase_vocoder_f32(S, rate):
    """Magnitudes and angles from float32 (np.abs, np.arctan2), the interpolation and the phase accumulator in float64, the
    accumulator reduced to [-pi, pi] before its float32 sine and cosine."""
    assert S.dtype == np.complex64
    F = S.shape[1]
    steps = np.arange(0, F, rate, dtype=np.float64)
    Sp = np.pad(S, [(0, 0), (0, 2)])
    mags, angs = np.abs(Sp), np.arctan2(Sp.imag, Sp.real)
    assert mags.dtype == np.float32 and angs.dtype == np.float32
    phi = np.linspace(0, np.pi * HOP, S.shape[0])
    acc = angs[:, 0].astype(np.float64)
    out = np.zeros((S.shape[0], len(steps)), dtype=np.complex64)
    two_pi = 2.0 * np.pi
    for t, s in enumerate(steps):
        k = int(np.floor(s))
        a = s - k
        mag = (1.0 - a) * mags[:, k].astype(np.float64) + a * mags[:, k + 1].astype(np.float64)
        red = (acc - two_pi * np.round(acc / two_pi)).astype(np.float32)
        out[:, t].real = (mag * np.cos(red)).astype(np.float32)
        out[:, t].imag = (mag * np.sin(red)).astype(np.float32)
        dp = angs[:, k + 1].astype(np.float64) - angs[:, k].astype(np.float64) - phi
        dp = dp - two_pi * np.round(dp / two_pi)
        acc = acc + phi + dp
    return out


def istft_f32(D, length):
    import scipy.fft as sfft
    assert D.dtype == np.complex64
    w = _hann_f32()
    n = min(D.shape[1], int(np.ceil((length + N_FFT) / HOP)))
    D = D[:, :n].copy()
    D[0].imag = 0
    D[-1].imag = 0
    frames = sfft.irfft(D, n=N_FFT, axis=0)
    assert frames.dtype == np.float32
    frames = frames * w[:, None]
    total = N_FFT + HOP * (n - 1)
    y = np.zeros(total, dtype=np.float32)
    wss = np.zeros(total, dtype=np.float32)
    for f in range(n):
        y[f * HOP:f * HOP + N_FFT] += frames[:, f]
        wss[f * HOP:f * HOP + N_FFT] += w * w
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    y = y[N_FFT // 2:]
    y = np.pad(y, (0, max(0, length - len(y))))[:length]
    assert y.dtype == np.float32
    return y


def time_stretch_f32(y, rate):
    L = len(y)
    return istft_f32(phase_vocoder_f32(stft_f32(y), rate), int(round(L / rate)))


# ------------------------------------------------------------------------------------------------ the edge cases
# (numpy only and deterministic: tests/test_augment_ref.py checks the yardstick on them, tests/test_gpu_augment_edges.py the kernels)
REVERB_T = 70000
KIND_REVERB, KIND_GAIN = "reverb", "gain"


def _rir(rng, n):
    return (rng.standard_normal(n) * np.exp(-np.arange(n) / max(n / 6.0, 1.0))).astype(np.float32)


def reverb_edge_cases():
    """The ragged reverberation batch: a list of dicts (name, kind, x, h, d).  ``d`` is the index handed over as RIR_PEAK;
    it is argmax|h| throughout (where a case places the peak, it writes a tap larger than every other there)."""
    rng = np.random.default_rng(20)
    cases = []

    def add(name, L, Lh, kind=KIND_REVERB, x_zero=False, h_zero=False, h_scale=1.0, peak=None):
        x = np.zeros(L, dtype=np.float32) if x_zero else (rng.standard_normal(L) * 0.1).astype(np.float32)
        h = np.zeros(Lh, dtype=np.float32) if h_zero else _rir(rng, Lh) * np.float32(h_scale)
        if peak is not None:
            h[peak] = np.float32(8.0)
        cases.append(dict(name=name, kind=kind, x=x, h=h, d=int(np.argmax(np.abs(h)))))

    add("L1_h1_k1", 1, 1)
    add("L1_h5_truncated_to_one", 1, 5)
    add("L2_h2_k2", 2, 2)
    add("L3_h7_k3", 3, 7)
    add("L64_h64_k7", 64, 64)
    add("L2049_h2048_need_4096", 2049, 2048)
    add("L2048_h2049_truncated_by_one", 2048, 2049)
    add("L4097_h1_k13", 4097, 1)
    add("L8192_h300_k14", 8192, 300)
    add("L8193_h300_k14", 8193, 300)
    add("L70000_h9000_k17", 70000, 9000)
    add("L70000_h9000_quiet_rir", 70000, 9000, h_scale=1e-6)
    add("L0", 0, 40)
    add("L5000_gain_row", 5000, 40, kind=KIND_GAIN)
    add("L4000_zero_x", 4000, 300, x_zero=True)
    add("L4000_zero_rir", 4000, 300, h_zero=True)
    add("L1000_h1500_peak_at_L_minus_1", 1000, 1500, peak=999)
    add("L1000_h1500_peak_at_L", 1000, 1500, peak=1000)
    add("L1000_h1500_peak_at_Lh_minus_1", 1000, 1500, peak=1499)
    add("L1000_h300_peak_at_0", 1000, 300, peak=0)
    return cases


def reverb_pow24_case():
    """(x, h) of the 2^24-point row: L = 2^23 with 3 taps needs 2^23 + 2 points."""
    rng = np.random.default_rng(21)
    x = (rng.standard_normal(1 << 23, dtype=np.float32) * np.float32(0.1))
    return x, np.array([0.3, 1.0, -0.45], dtype=np.float32)


GN_T = 20000


def gain_noise_edge_cases():
    """(noises, rows): the noise bank and a list of dicts (name, kind in {"noise", "gain", "none", "reverb"}, x, and for the
    noise rows noise / start / snr_amp, for the gain rows gain_lin)."""
    rng = np.random.default_rng(22)
    noises = [np.array([0.25], dtype=np.float32),
              (rng.standard_normal(3000) * 0.05).astype(np.float32),
              (rng.standard_normal(20000) * 0.2).astype(np.float32),
              (rng.standard_normal(64000) * 0.3).astype(np.float32),
              np.full(5000, 1.1e-9, dtype=np.float32),
              np.full(5000, 0.9e-9, dtype=np.float32)]
    rows = []

    def x_of(L):
        return (rng.standard_normal(L) * 0.1).astype(np.float32)

    def noise(name, L, f, start, snr_db):
        rows.append(dict(name=name, kind="noise", x=x_of(L), noise=f, start=start, snr_amp=10 ** (snr_db / 20)))

    noise("L1_long_noise_start_N_minus_S", 1, 3, 64000 - 1, 7.0)
    noise("L1_one_sample_noise", 1, 0, 0, 3.0)
    noise("L8191_one_sample_noise_tiled", 8191, 0, 0, 11.0)
    noise("L8192_short_noise_tiled", 8192, 1, 0, 5.0)
    noise("L8193_long_noise_start_0", 8193, 3, 0, 17.0)
    noise("L20000_noise_S_eq_L_eq_N", 20000, 2, 0, 9.0)
    noise("L20000_long_noise_start_N_minus_S", 20000, 3, 64000 - 20000, 29.0)
    noise("L1500_short_noise_start_N_minus_S", 1500, 1, 3000 - 1500, 4.0)
    noise("L0_noise_row", 0, 1, 0, 10.0)
    noise("L8193_noise_rms_1.1e-9", 8193, 4, 0, 20.0)
    noise("L8193_noise_rms_0.9e-9", 8193, 5, 0, 20.0)
    for L, db in ((1, -5.3), (8193, 4.1), (20000, -0.7)):
        rows.append(dict(name=f"L{L}_gain", kind="gain", x=x_of(L), gain_lin=10 ** (db / 20)))
    rows.append(dict(name="L8192_none_row", kind="none", x=x_of(8192)))
    rows.append(dict(name="L8191_reverb_row", kind="reverb", x=x_of(8191)))
    return noises, rows


STRETCH_LENS = (1, 511, 512, 513, 1535, 1536, 2047, 2048, 2049, 5000)
STRETCH_RATES = (0.5, 0.8, 1.0, 1.3, 2.0)
# L / rate lands on a half: Python's round, and the kernel's nearbyint, go to the even neighbour
STRETCH_HALVES = {(513, 2.0): 256, (515, 2.0): 258, (5, 2.0): 2, (1, 2.0): 0}
STRETCH_T = 5000


def stretch_edge_cases():
    """Launches of the time-stretch test: a list of lists of dicts (name, x, rate), rates mixed within each launch."""
    rng = np.random.default_rng(23)
    pairs = [(L, r) for L in STRETCH_LENS for r in STRETCH_RATES] + [(515, 2.0), (5, 2.0)]
    rows = [dict(name=f"L{L}_rate{r}", x=(rng.standard_normal(L) * 0.1).astype(np.float32), rate=r) for L, r in pairs]
    rows.append(dict(name="L0_rate1.3", x=np.zeros(0, dtype=np.float32), rate=1.3))
    rows.append(dict(name="L2049_zeros_rate0.8", x=np.zeros(2049, dtype=np.float32), rate=0.8))
    return [rows[i::3] for i in range(3)]


def augment_one(x, row, cols, noise_bank=None, rir_bank=None):
    """One utterance through the whole contract, given its table row (``cols``: ssak_amd.hip for the column indices)."""
    kind = int(row[cols.AUG_KIND])
    if kind == cols.AUG_GAIN:
        y = gain(x, row[cols.AUG_GAIN_LIN]).astype(np.float64)
    elif kind == cols.AUG_NOISE_MIX:
        y = noise_mix(x, noise_bank[int(row[cols.AUG_NOISE])], int(row[cols.AUG_NOISE_START]), row[cols.AUG_SNR_AMP])
    elif kind == cols.AUG_REVERB:
        y = reverb(x, rir_bank[int(row[cols.AUG_RIR])])
    else:
        y = np.asarray(x, dtype=np.float64)
    return time_stretch(y, row[cols.AUG_RATE])
