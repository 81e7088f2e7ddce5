"""Float64 numpy restatement of the TimeDomainSpecAugment contract of the SpeechBrain recipe (the docstring of
ssak_amd/augment.py), written from the contract and not from the product code: nothing here imports ssak_amd.

Stages 2 (DropFreq: one 101-tap notch product for the batch, applied as a cross-correlation) and 3 (DropChunk: ranges set to
zero), the draws of all three stages, and the fp32 dot-product bound the GPU tests hold the kernel to.
"""
import math

import numpy as np

TAPS = 101
PAD = 50


def blackman_periodic(n=TAPS):
    k = np.arange(n, dtype=np.float64)
    return 0.42 - 0.5 * np.cos(2 * math.pi * k / n) + 0.08 * np.cos(4 * math.pi * k / n)


def _sinc(z):
    z = np.asarray(z, dtype=np.float64)
    safe = np.where(z == 0, 1.0, z)
    return np.where(z == 0, 1.0, np.sin(safe) / safe)


def notch(f):
    """notch_filter(f, 101, 0.05): low-pass at f plus spectrally inverted low-pass at f + 0.1."""
    n = np.arange(TAPS, dtype=np.float64) - PAD
    w = blackman_periodic()
    lo = _sinc(3 * f * n) * w
    lo = lo / lo.sum()
    hi = _sinc(3 * (f + 0.1) * n) * w
    hi = hi / -hi.sum()
    hi[PAD] += 1
    return lo + hi


def correlate_same(g, h):
    """out[j] = sum_k h[k] * g_pad[j + k], g zero-padded by len(h) // 2 on both sides (what conv1d computes)."""
    p = len(h) // 2
    gp = np.concatenate([np.zeros(p), np.asarray(g, dtype=np.float64), np.zeros(p)])
    return np.array([np.dot(h, gp[j:j + len(h)]) for j in range(len(g))])


def convolve_same(g, h):
    """The other orientation (a true convolution): only to show that it is NOT the contract."""
    return correlate_same(g, np.asarray(h)[::-1])


def compose(freqs, op=correlate_same):
    g = np.zeros(TAPS)
    g[PAD] = 1.0
    for f in freqs:
        g = op(g, notch(f))
    return g


def fir(x, g):
    """y[b, t] = sum_k g[k] * x[b, t + k - len(g) // 2], zeros outside the row; x [B, T], float64."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    p = len(g) // 2
    xp = np.pad(x, ((0, 0), (p, p)))
    win = np.lib.stride_tricks.sliding_window_view(xp, len(g), axis=1)  # [B, T, ntaps]
    return win @ g


def fir_abs(x, g):
    """sum_k |g[k]| * |x[b, t + k - half]|: the scale of the fp32 rounding bound."""
    return fir(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(g, dtype=np.float64)))


def fir_bound(x, g):
    """|fl(sum of n products) - exact| <= gamma_n * sum |g_k x_k| with gamma_n <= (n + 1) u for fp32's u = 2^-24, for any
    order of the n = len(g) terms, with or without FMA (Higham, Accuracy and Stability, section 3.1); 1e-30 covers terms of
    denormal size.  For 101 taps: 102 * 2^-24 * sum |g_k| |x_k| + 1e-30."""
    return (len(g) + 1) * 2.0 ** -24 * fir_abs(x, g) + 1e-30


def drop_chunks(y, chunks):
    """chunks: per row a list of (start, end); samples [start, end) clipped to the row are set to 0."""
    y = np.array(y, copy=True)
    T = y.shape[1]
    for b, row in enumerate(chunks):
        for s, e in row:
            s, e = max(0, int(s)), min(T, int(e))
            if e > s:
                y[b, s:e] = 0.0
    return y


def ceil_div(a, b):
    return -(-int(a) // int(b))


def draw(seed, step, positions, lengths, speeds=(95, 100, 105), sample_rate=16000, perturb_prob=1.0, drop_freq_prob=1.0,
         drop_chunk_prob=1.0, freq_count=(0, 3), chunk_count=(0, 5), chunk_length=(1000, 2000)):
    """The draws of one (shard of a) global batch -> dict(speed, freqs, out_lens, chunks): batch-level draws from
    default_rng([seed, step]) in the order speed (u, index), DropFreq (u, count, frequencies), DropChunk (u); an utterance's
    chunks from default_rng([seed, step, position]) in the order count, lengths, starts."""
    rng = np.random.default_rng([seed, step])
    u1 = rng.random()
    i = int(rng.integers(len(speeds)))
    u2 = rng.random()
    count = int(rng.integers(freq_count[0], freq_count[1] + 1))
    freqs = [float(u) * (1 - 1e-14) + 1e-14 for u in rng.random(count)]
    u3 = rng.random()
    speed = speeds[i] if not u1 > perturb_prob else 100
    if u2 > drop_freq_prob:
        freqs = []
    new_sr = sample_rate * speed // 100
    d = math.gcd(sample_rate, new_sr)
    orig_r, new_r = sample_rate // d, new_sr // d
    out_lens = [ceil_div(L * new_r, orig_r) for L in lengths]
    chunks = []
    for pos, L in zip(positions, out_lens):
        r = np.random.default_rng([seed, step, pos])
        n = int(r.integers(chunk_count[0], chunk_count[1] + 1))
        row = []
        if n:
            ln = [int(v) for v in r.integers(chunk_length[0], chunk_length[1] + 1, size=n)]
            st = [int(v) for v in r.integers(0, max(0, L - max(ln)) + 1, size=n)]
            row = [(s, s + l) for s, l in zip(st, ln)]
        chunks.append(row if not u3 > drop_chunk_prob else [])
    return {"speed": speed, "ratio": (orig_r, new_r), "freqs": freqs, "out_lens": out_lens, "chunks": chunks}
