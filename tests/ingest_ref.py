"""Float64 numpy restatement of the audio ingest stages (ssak_amd/csrc/ingest.hip, ssak_amd/csrc/features.hip): PCM decode
and channel average, windowed-sinc resampling, zero-mean / unit-variance normalisation.

Written from what the kernels' headers define, not from what they compute; numpy only, nothing imported from ssak_amd or
oracle.  ``tests/test_ingest_ref.py`` checks it against the project's fp32 oracle (oracle/resample_ref.py) and measures what
fp32 arithmetic of the kernel's own form costs against it; ``tests/test_gpu_ingest_kernels.py`` holds the kernels to it.

PCM (``ssak_pcm_to_mono_f32``): little-endian samples, u8 -> (v - 128) / 128, i16 -> v / 2^15, i32 -> v / 2^31, mean over the
channels of a frame.

Resampling (``ssak_resample_sinc``, torchaudio.functional.resample with its defaults: sinc_interp_hann, lowpass_filter_width 6,
rolloff 0.99), o, n = the rates divided by their gcd::

    base  = min(o, n) * 0.99,   width = ceil(6 o / base),   taps = 2 width + o
    t     = clamp((phase_j + (k - width) / o) * base, -6, 6)                      j in [0, n), k in [0, taps)
    h[j,k] = sinc(pi t) * cos(pi t / 12)^2 * base / o
    y[m]  = sum_k h[j,k] * x[q o + k - width],   q, j = divmod(m, n),   x = 0 outside [0, len),   m < ceil(n len / o)

``phase_j`` is -j / n.  torchaudio divides an int64 arange by an int there, which is a *float32* division, before the value
meets the float64 index grid; the product reproduces that on purpose (``quirk=True``, the default).  ``quirk=False`` is the
exact phase.

Normalisation (``ssak_wave_normalize``): (x - mean) / sqrt(var + 1e-7) over [0, len), var biased; zeros after; mask 1 / 0.
"""
from __future__ import annotations

import math

import numpy as np

LOWPASS_WIDTH = 6.0
ROLLOFF = 0.99
NORM_EPS = 1e-7


# ------------------------------------------------------------------------------------------------ PCM
def pcm_to_mono(raw_bytes, channels: int, width: int) -> np.ndarray:
    """Interleaved little-endian PCM bytes -> float64 [frames] in [-1, 1): decode, then the mean over the channels."""
    raw = np.frombuffer(bytes(raw_bytes), dtype=np.uint8)
    if width == 1:
        v = (raw.astype(np.float64) - 128.0) / 128.0
    elif width == 2:
        v = raw.view("<i2").astype(np.float64) / 32768.0
    elif width == 4:
        v = raw.view("<i4").astype(np.float64) / 2147483648.0
    else:
        raise ValueError(f"sample width {width}")
    return v.reshape(-1, channels).mean(axis=1)


# ------------------------------------------------------------------------------------------------ resampling
def resample_plan(orig_sr: int, new_sr: int):
    """(o, n, width, taps)."""
    g = math.gcd(int(orig_sr), int(new_sr))
    o, n = int(orig_sr) // g, int(new_sr) // g
    base = min(o, n) * ROLLOFF
    width = math.ceil(LOWPASS_WIDTH * o / base)
    return o, n, width, 2 * width + o


def resample_taps(orig_sr: int, new_sr: int, quirk: bool = True) -> np.ndarray:
    """float64 [n, taps] filter table."""
    o, n, width, taps = resample_plan(orig_sr, new_sr)
    base = min(o, n) * ROLLOFF
    j = np.arange(n)
    if quirk:
        phase = ((-j).astype(np.float32) / np.float32(n)).astype(np.float64)
    else:
        phase = -j.astype(np.float64) / n
    k = np.arange(taps, dtype=np.float64)
    t = (phase[:, None] + ((k - width) / o)[None, :]) * base
    t = np.clip(t, -LOWPASS_WIDTH, LOWPASS_WIDTH)
    window = np.cos(t * math.pi / LOWPASS_WIDTH / 2.0) ** 2
    a = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(a == 0.0, 1.0, np.sin(a) / a)
    return s * (window * (base / o))


def out_len(length: int, o: int, n: int) -> int:
    return -(-(n * int(length)) // o)


def resample(x, orig_sr: int, new_sr: int, taps_f32=None, quirk: bool = True) -> np.ndarray:
    """float64 resampling of the 1-D signal x, every output evaluated from the definition (a gather and a dot product per
    output; no convolution, no padding).  ``taps_f32``: a [n, taps] (or flat) table to use instead of resample_taps, e.g. the
    fp32 table a library produced -- the result then isolates indexing and accumulation from the table's rounding."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    o, n, width, taps = resample_plan(orig_sr, new_sr)
    if o == n:
        return x.copy()
    h = resample_taps(orig_sr, new_sr, quirk) if taps_f32 is None else np.asarray(taps_f32, dtype=np.float64).reshape(n, taps)
    length = len(x)
    olen = out_len(length, o, n)
    y = np.zeros(olen, dtype=np.float64)
    k = np.arange(taps)
    step = max(1, (1 << 22) // taps)
    for m0 in range(0, olen, step):
        m = np.arange(m0, min(olen, m0 + step))
        q, j = np.divmod(m, n)
        idx = (q * o)[:, None] + (k - width)[None, :]
        ok = (idx >= 0) & (idx < length)
        xg = np.where(ok, x[np.clip(idx, 0, max(length - 1, 0))] if length else 0.0, 0.0)
        y[m] = np.sum(h[j] * xg, axis=1)
    return y


def resample_fp32_fma(x, orig_sr: int, new_sr: int, taps_f32) -> np.ndarray:
    """The same sum as a sequential fp32 fused multiply-add chain over k = 0 .. taps-1 (one rounding per tap: the product of
    two fp32 numbers is exact in float64, the accumulator is rounded to fp32 after each add).  x and taps_f32 are fp32 values."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64).reshape(-1)
    o, n, width, taps = resample_plan(orig_sr, new_sr)
    h = np.asarray(taps_f32, dtype=np.float32).astype(np.float64).reshape(n, taps)
    length = len(x)
    olen = out_len(length, o, n)
    q, j = np.divmod(np.arange(olen), n)
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + 2 * o)])  # xp[i + width] = x[i]
    acc = np.zeros(olen, dtype=np.float32)
    for k in range(taps):
        acc = (acc.astype(np.float64) + h[j, k] * xp[q * o + k]).astype(np.float32)
    return acc.astype(np.float64)


# ------------------------------------------------------------------------------------------------ normalisation
def normalize(x, length=None):
    """(float64 [T] normalised over [0, length) and 0 after, int32 [T] mask).  A length of 0 gives all zeros."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    T = len(x)
    n = T if length is None else min(max(int(length), 0), T)
    y = np.zeros(T, dtype=np.float64)
    mask = np.zeros(T, dtype=np.int32)
    if n > 0:
        v = x[:n]
        mean = v.mean()
        var = np.mean((v - mean) ** 2)
        y[:n] = (v - mean) / np.sqrt(var + NORM_EPS)
        mask[:n] = 1
    return y, mask
