"""Float64 numpy restatement of the helper kernels the wav2vec2 engine launches between its row kernels and GEMMs (SpecAugment
forward / backward and the masked column sum, add, the gelu-grad product, the batched bf16 transpose, the deferred second-stage
reductions, the waveform normalisation), the inputs ``tests/test_gpu_helpers.py`` feeds them and the assertions it makes.

Written from what the kernels define, not from what they compute.  The storage roundings and the GELU forms are
``rowwise_ref``'s.  ``tests/test_helpers_ref.py`` pins the SpecAugment pair to torch float64 autograd and shows, on the inputs
built here, that every assertion below rejects the obvious wrong restatements; ``tests/test_gpu_helpers.py`` holds the kernels to
this module through the test-only entries of ABI 660.

Definitions::

    specaug_fwd   row (b, t) of h:  0 where t >= flens[b];  else embed (rounded to the storage type) where mask[b, t];  else unchanged
    specaug_bwd   dembed += sum of the rows of dh with mask[b, t] and t < flens[b];  then every masked or padding row of dh = 0
    colsum        out[n] += sum_m X[m, n] over the rows with rowmask[m] != 0 and m % F < flens[m / F] (each test optional)
    add           round_st(round_f32(a + b));     gelu-grad product  dy * gelu'(pre)  (bf16: the logistic fit, fp32: erf)
    transpose     dst [C, R] = src [R, C]^T;      reduce  out[c] += sum_k partial[k * stride + c]
    wave_normalize  (x - mean) / sqrt(var + 1e-7) over the valid samples, var biased; padding 0, mask 1 / 0; length 0: all 0
"""
from __future__ import annotations

import functools

import numpy as np

import rowwise_ref as RR

U = 2.0 ** -24  # the fp32 unit roundoff

# ------------------------------------------------------------------------------------------------ the cases of the GPU test
SPECAUG_B, SPECAUG_F = 3, 37
SPECAUG_FLENS = (37, 20, 0)
SPECAUG_C = (8, 136, 768)         # fewer columns than the kernel's 128 threads, not a multiple of 128, several trips
SPECAUG_BWD_SHAPES = tuple((SPECAUG_F, c) for c in SPECAUG_C) + ((700, 8),)   # F = 700: M = 2100 > 2048 rows
SPECAUG_FLENS_LONG = (0, 333, 700)  # (the rows beyond 2048, which the capped row groups reach on their second trip, are valid ones)
COLSUM_M = (1, 31, 32, 33, 2048, 2049)
COLSUM_N = (8, 64, 72)
COLSUM_F = 13                     # frames per utterance of the masked column sum alone: divides none of the M above
ELEMWISE_GRID_CAP = 4096 * 256    # threads of gelu_grad_mul_kernel / add_kernel's capped grid, 8 elements each
ELEMWISE_N = (8, 2048, 2056, ELEMWISE_GRID_CAP * 8 + 8)
TRANSPOSE_SHAPES = ((8, 8), (64, 64), (65, 63), (72, 200), (136, 328), (1, 129))
TRANSPOSE_CAP = 112               # transpose.hip TR_CAP: matrices per launch
REDUCE_SLOTS = (1, 16, 17, 240, 241, 256, 257, 600)
REDUCE_NCOLS = (1, 63, 64, 65, 200)
REDUCE_CAP = 32                   # kernels.h ReduceSink::CAP
WAVE_T = (8191, 8193, 16385)


# ------------------------------------------------------------------------------------------------ storage types and bits
def to_bits(x, bf16: bool) -> np.ndarray:
    """The bit patterns (uint16 / uint32) of values the storage type holds exactly."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
    if not bf16:
        return b.copy()
    assert not (b & 0xFFFF).any(), "not bf16 values"
    return (b >> 16).astype(np.uint16)


def from_bits(b, bf16: bool) -> np.ndarray:
    b = np.asarray(b)
    w = (b.astype(np.uint32) << 16) if bf16 else b.astype(np.uint32)
    return w.view(np.float32).astype(np.float64)


def pattern_bits(n: int, bf16: bool, salt: int = 0) -> np.ndarray:
    """n finite bit patterns, a different one per element (bf16: within any 65 536 consecutive elements): i times an odd constant
    plus salt; a pattern whose exponent field is all ones (Inf / NaN) has its top exponent bit cleared."""
    i = np.arange(n, dtype=np.uint64)
    if bf16:
        p = ((i * 40503 + 12345 + salt) & 0xFFFF).astype(np.uint16)
        return np.where((p & 0x7F80) == 0x7F80, p & 0xBFFF, p).astype(np.uint16)
    p = ((i * 2654435761 + 97 + salt) & 0xFFFFFFFF).astype(np.uint32)
    return np.where((p & 0x7F800000) == 0x7F800000, p & 0xBFFFFFFF, p).astype(np.uint32)


def neighbours(x: float, bf16: bool):
    """(the storage type's next value towards 0, x, the next one away from 0)."""
    b = to_bits(np.array([x]), bf16).astype(np.int64)[0]
    return tuple(float(from_bits(np.array([v], dtype=np.uint16 if bf16 else np.uint32), bf16)[0]) for v in (b - 1, b, b + 1))


def ulp_st(x, bf16: bool) -> np.ndarray:
    """One unit in the last place of the storage type at |x| (tests/test_gpu_rowwise.py's)."""
    return RR.bf16_ulp(x) if bf16 else 2.0 ** -23 * np.abs(x) + 1e-45


# ------------------------------------------------------------------------------------------------ the restatements
def _pad_rows(B: int, F: int, flens) -> np.ndarray:
    if flens is None:
        return np.zeros((B, F), dtype=bool)
    return np.arange(F)[None, :] >= np.asarray(flens, dtype=np.int64)[:, None]


def _mask_rows(B: int, F: int, mask) -> np.ndarray:
    return np.zeros((B, F), dtype=bool) if mask is None else np.asarray(mask).reshape(B, F) != 0


def specaug_fwd(h, mask, flens, embed, bf16: bool) -> np.ndarray:
    """h [B, F, C] float64 -> the rows after SpecAugment and padding; padding wins over the mask."""
    h = np.asarray(h, dtype=np.float64)
    B, F, _ = h.shape
    pad, mk = _pad_rows(B, F, flens), _mask_rows(B, F, mask)
    out = h.copy()
    if mask is not None:
        out[mk] = RR.round_to(embed, bf16)
    out[pad] = 0.0
    return out


def specaug_bwd(dh, mask, flens, dembed):
    """(dh', dembed', terms): dembed' = dembed + the sum of the masked non-padding rows (taken BEFORE they are zeroed), dh' = dh
    with every masked or padding row 0; terms [C] = the sum of those rows' magnitudes (for the column sum's bar)."""
    dh = np.asarray(dh, dtype=np.float64)
    B, F, C = dh.shape
    pad, mk = _pad_rows(B, F, flens), _mask_rows(B, F, mask)
    take = mk & ~pad
    de = np.asarray(dembed, dtype=np.float64) + dh[take].sum(axis=0)
    out = dh.copy()
    out[mk | pad] = 0.0
    return out, de, np.abs(dh[take]).sum(axis=0)


def colsum(X, N: int, rowmask=None, flens=None, F: int = 0):
    """(sums [N], sum of magnitudes [N]) of the first N columns of X [M, ld] over the counted rows."""
    X = np.asarray(X, dtype=np.float64)
    M = X.shape[0]
    take = np.ones(M, dtype=bool)
    if rowmask is not None:
        take = np.asarray(rowmask) != 0
        if flens is not None:
            m = np.arange(M)
            take &= (m % F) < np.asarray(flens, dtype=np.int64)[m // F]
    return X[take, :N].sum(axis=0), np.abs(X[take, :N]).sum(axis=0)


def add(a, b, bf16: bool) -> np.ndarray:
    """An fp32 add, then the round-to-nearest-even conversion to the storage type."""
    return RR.round_to(RR.round_f32(np.asarray(a, dtype=np.float64) + np.asarray(b, dtype=np.float64)), bf16)


def gelu_grad_mul(dy, pre, bf16: bool) -> np.ndarray:
    return np.asarray(dy, dtype=np.float64) * RR.gelu_forms(bf16)[1](pre)


def transpose(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x).T)


def reduce(partial, slots: int, ncols: int) -> np.ndarray:
    """partial [>= slots, stride] -> the sum of its first `slots` rows over the first ncols columns, float64."""
    return np.asarray(partial, dtype=np.float64)[:slots, :ncols].sum(axis=0)


def wave_normalize(x, lens):
    """x [B, T], lens [B] -> (normalised float64 [B, T], mask int32 [B, T])."""
    x = np.asarray(x, dtype=np.float64)
    B, T = x.shape
    out, mask = np.zeros((B, T)), np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        n = int(min(max(int(lens[b]), 0), T))
        if n == 0:
            continue
        v = x[b, :n]
        out[b, :n] = (v - v.mean()) / np.sqrt(v.var() + 1e-7)
        mask[b, :n] = 1
    return out, mask


# ------------------------------------------------------------------------------------------------ the assertions
def check_equal(name, got, ref):
    """Bit-exact (integer bit patterns) or value-exact (integer-valued floats)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} != {ref.shape}"
    bad = got != ref
    if bad.any():
        k = np.unravel_index(np.argmax(bad), bad.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} differ; first at {k}: got {got[k]!r} ref {ref[k]!r}")


def check_bar(name, got, ref, bar):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} != {ref.shape}"
    assert np.isfinite(got).all(), f"{name}: non-finite"
    err = np.abs(got - ref)
    bar = np.broadcast_to(bar, err.shape)
    bad = err > bar
    if bad.any():
        k = np.unravel_index(np.argmax(err - bar), err.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.size} outside the bar; worst at {k}: got {got[k]!r} ref {ref[k]!r} "
                             f"bar {bar[k]!r}")


def colsum_bar(start, ref, terms) -> np.ndarray:
    """The bar tests/test_gpu_rowwise.py holds its column sums to: 1e-5 sum|terms| + 2^-23 (|start| + |ref|)."""
    return 1e-5 * np.asarray(terms) + 2.0 ** -23 * (np.abs(start) + np.abs(ref))


def product_bar(ref, dy, bf16: bool) -> np.ndarray:
    """One storage ulp of the reference + 1e-6 |dy| (the bar tests/test_gpu_rowwise.py::test_gelu_forms holds gelu' to)."""
    return ulp_st(ref, bf16) + 1e-6 * np.abs(dy)


def reduce_bar(slots: int, terms) -> np.ndarray:
    """slots u sum|terms|: a column's sum takes at most ceil(slots / 16) - 1 + 15 <= slots fp32 additions (one slot group's, then
    the sixteen group sums'), each within u of a partial sum that is at most sum|terms|."""
    return slots * U * np.asarray(terms)


# ------------------------------------------------------------------------------------------------ the inputs
def specaug_mask(B: int, F: int, flens, seed: int = 0) -> np.ndarray:
    """A seeded mask [B, F] uint8 of about 30 % of the rows."""
    rng = np.random.default_rng(1000 + 7 * F + seed)
    return (rng.random((B, F)) < 0.3).astype(np.uint8)


def specaug_flens(F: int):
    return np.array(SPECAUG_FLENS if F == SPECAUG_F else SPECAUG_FLENS_LONG, dtype=np.int32)


def specaug_embed(C: int) -> np.ndarray:
    return np.random.default_rng(C).uniform(0.1, 1.0, C).astype(np.float32)   # (non-zero: an embedding row is no padding row)


def specaug_dh(F: int, C: int, bf16: bool, integer: bool):
    """(dh [B, F, C], dembed start [C]) as float64 values the storage type holds exactly.  integer: dh in -3 .. 3 and the start in
    1 .. 9, so that every partial sum of a column (at most 3 * B * F + 9 < 2^24) is exact in fp32 in any order."""
    rng = np.random.default_rng(31 * F + C + (1 if integer else 0))
    if integer:
        return rng.integers(-3, 4, (SPECAUG_B, F, C)).astype(np.float64), rng.integers(1, 10, C).astype(np.float64)
    return RR.round_to(rng.standard_normal((SPECAUG_B, F, C)), bf16), RR.round_f32(rng.standard_normal(C) + 3.0)


def colsum_scratch_floats(M: int, N: int) -> int:
    """What k_colsum_t needs for its two-stage path: one partial row per row group, min(64, ceil(M / 32)) of them."""
    return min(64, -(-M // 32)) * N


def colsum_case(M: int, N: int, bf16: bool, integer: bool):
    """X [M, N + 8] with NaN in the 8 pad columns, rowmask [M] (~50 %, row 0 set), flens [ceil(M / COLSUM_F)], start [N]."""
    rng = np.random.default_rng(M * 131 + N + (1 if integer else 0))
    X = np.full((M, N + 8), np.nan)
    X[:, :N] = rng.integers(-3, 4, (M, N)) if integer else RR.round_to(rng.standard_normal((M, N)), bf16)
    rowmask = (rng.random(M) < 0.5).astype(np.uint8)
    rowmask[0] = 1
    flens = np.array([(7, 0, COLSUM_F, 1)[i % 4] for i in range(-(-M // COLSUM_F))], dtype=np.int32)
    start = rng.integers(1, 10, N).astype(np.float64) if integer else RR.round_f32(rng.standard_normal(N) + 3.0)
    return X, rowmask, flens, start


def gelu_edges(bf16: bool):
    """+-6 (where the fit's argument is clamped) with the storage type's neighbours either side, and the ends of [-12, 12]."""
    lo, mid, hi = neighbours(6.0, bf16)
    return np.array([mid, -mid, lo, -lo, hi, -hi, -12.0, 12.0])


@functools.lru_cache(maxsize=2)
def elementwise_case(n: int, bf16: bool):
    """(dy / a, pre, b) [n] float64, rounded to the storage type.  pre: the eight values of gelu_edges first, then [-12, 12] evenly;
    dy, b ~ N(0, 1), a = dy."""
    rng = np.random.default_rng(n % 100003 + (7 if bf16 else 0))
    pre = np.linspace(-12.0, 12.0, n)
    pre[:8] = gelu_edges(bf16)
    dy = rng.standard_normal(n, dtype=np.float32).astype(np.float64)
    b = rng.standard_normal(n, dtype=np.float32).astype(np.float64) * 3.0
    return RR.round_to(dy, bf16), RR.round_to(pre, bf16), RR.round_to(b, bf16)


def transpose_src(R: int, C: int, salt: int = 0) -> np.ndarray:
    return pattern_bits(R * C, True, salt).reshape(R, C)


def reduce_jobs(integer: bool = True, seed: int = 0):
    """The 32 jobs of the direct call: (partial [slots, stride] with NaN in the pad columns, start [ncols], slots, ncols), every
    value of REDUCE_SLOTS and REDUCE_NCOLS several times, stride = ncols + 3.  integer: partials in -4 .. 4 (never all 0 in a row:
    column 0 of every slot is non-zero), the start in 1 .. 9; else N(0, 1) partials onto a start of 0 (so that the final += rounds
    nothing and reduce_bar covers the whole error)."""
    rng = np.random.default_rng(4242 + seed)
    jobs = []
    for i in range(REDUCE_CAP):
        slots, ncols = REDUCE_SLOTS[i % 8], REDUCE_NCOLS[(i + i // 8) % 5]
        P = np.full((slots, ncols + 3), np.nan)
        if integer:
            P[:, :ncols] = rng.integers(-4, 5, (slots, ncols))
            P[:, 0] = rng.integers(1, 5, slots)
            start = rng.integers(1, 10, ncols).astype(np.float64)
        else:
            P[:, :ncols] = RR.round_f32(rng.standard_normal((slots, ncols)))
            start = np.zeros(ncols)
        jobs.append((P, start, slots, ncols))
    return jobs


REDUCE_SHARED = (1, 6)                   # two of reduce_jobs' jobs with one ncols (63) and different slots (16, 257)
REDUCE_SINK_CALLS = (3,) * 10 + (3, 2)  # 30 jobs queued, a call of 3 that does not fit, a call of 2 that fills the sink


def sink_jobs():
    """35 integer jobs for REDUCE_SINK_CALLS: job i (slots, ncols) cycling through small sizes; jobs 30 and 0 share their out (the
    call that runs at once adds into a vector a queued job also adds into).  Returns (jobs, out_of): out_of[i] = index of the
    output vector of job i."""
    rng = np.random.default_rng(99)
    jobs, out_of = [], []
    for i in range(sum(REDUCE_SINK_CALLS)):
        slots, ncols = (1, 16, 17, 33, 5)[i % 5], 65 if i in (0, 30) else (1, 63, 64, 65, 200)[i % 5]
        P = np.full((slots, ncols + 3), np.nan)
        P[:, :ncols] = rng.integers(-4, 5, (slots, ncols))
        P[:, 0] = rng.integers(1, 5, slots)
        jobs.append((P, rng.integers(1, 10, ncols).astype(np.float64), slots, ncols))
        out_of.append(0 if i == 30 else i)
    return jobs, out_of


def wave_case(T: int):
    """(x [5, T] fp32, lens): N(0.3, 0.1) signal, 7.0 in the padding; the length-2 row holds 0.25 and 0.35."""
    rng = np.random.default_rng(T)
    lens = np.array([T, T - 1, 2, 1, 0], dtype=np.int32)
    x = (rng.standard_normal((5, T)) * 0.1 + 0.3).astype(np.float32)
    x[2, :2] = (0.25, 0.35)
    for b, n in enumerate(lens):
        x[b, n:] = 7.0
    return x, lens
