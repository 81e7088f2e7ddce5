"""Float64 numpy restatement of the augmentation contract of ssak_amd/augment.py (kernels: ssak_amd/csrc/augment.hip).

* ``reverb``: checked on the CPU against the reference's own ``Reverberation._reverberate`` (tests/golden/augment_reverb.npz,
  made by tests/gen_golden_augment.py).
* ``time_stretch``: librosa.effects.time_stretch spelled out for librosa >= 0.10 defaults -- parity unpinned (librosa absent).
* ``noise_mix``: audiomentations' AddBackgroundNoise (relative RMS) -- parity unpinned (audiomentations absent).
* ``gain``: in float32, as audiomentations computes it (float32 samples times a Python float).
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
