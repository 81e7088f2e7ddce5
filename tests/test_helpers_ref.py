"""CPU: the float64 restatement tests/helpers_ref.py that tests/test_gpu_helpers.py holds the engine's helper kernels to is itself
right, and the GPU test's assertions have teeth.

* The SpecAugment pair equals torch float64 autograd of ``where(pad, 0, where(mask, embed, h))``.
* On the very inputs the GPU test uses, each of its assertions (helpers_ref.check_equal / check_bar with the bars of
  helpers_ref) rejects the obvious wrong restatements: the mask winning over padding, padding rows or unmasked rows counted
  into dembed, dh zeroed before the sum is taken, a missing last chunk of 8, a transposed tile written untransposed, a
  reduction that drops its last slot or the second of two jobs that share an out.
* The inputs meet the conditions the GPU cases rely on (which rows the mask holds, exact integer sums, the grid-cap size, the
  GELU clamp points, the shapes' dispatch edges).
* The test-only C entries of ABI 660 reject bad arguments before any launch.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import helpers_ref as HR  # noqa: E402
import rowwise_ref as RR  # noqa: E402

BOTH = pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp32"])


def _rejects(name, got, ref, bar=None):
    """The GPU test's assertion on (got, ref) fails."""
    with pytest.raises(AssertionError):
        if bar is None:
            HR.check_equal(name, got, ref)
        else:
            HR.check_bar(name, got, ref, bar)


# ------------------------------------------------------------------------------------------------ SpecAugment
@pytest.mark.parametrize("use_mask,use_flens", [(True, True), (True, False), (False, True), (False, False)])
def test_specaug_reference_matches_float64_autograd(use_mask, use_flens):
    """out = where(pad, 0, where(mask, embed, h)), loss = <out, g>: autograd's d/dh and d/dembed == specaug_bwd(g)."""
    B, F, C = HR.SPECAUG_B, HR.SPECAUG_F, 8
    rng = np.random.default_rng(3)
    mask = HR.specaug_mask(B, F, None) if use_mask else None
    flens = HR.specaug_flens(F) if use_flens else None
    h, g, embed = rng.standard_normal((B, F, C)), rng.standard_normal((B, F, C)), rng.standard_normal(C)
    th, te = torch.tensor(h, requires_grad=True), torch.tensor(embed, requires_grad=True)
    out = th
    if use_mask:
        out = torch.where(torch.tensor(mask != 0)[:, :, None], te, out)
    if use_flens:
        pad = torch.arange(F)[None, :] >= torch.tensor(flens.astype(np.int64))[:, None]
        out = torch.where(pad[:, :, None], torch.zeros_like(out), out)
    if out.requires_grad:
        (out * torch.tensor(g)).sum().backward()
    # (fp32 "rounding" of float64 values would move them: compare the forward with the embedding as given)
    f = HR.specaug_fwd(h, mask, flens, embed, bf16=False)
    want = out.detach().numpy()
    moved = f != h
    assert np.array_equal(f[~moved], want[~moved]) and np.allclose(f[moved], want[moved], rtol=1e-7, atol=0)
    start = rng.standard_normal(C)
    dh, dembed, terms = HR.specaug_bwd(g, mask, flens, start)
    assert np.array_equal(dh, th.grad.numpy() if th.grad is not None else g)
    want_e = te.grad.numpy() if te.grad is not None else np.zeros(C)
    assert np.abs(dembed - start - want_e).max() <= 1e-12
    assert (terms >= np.abs(dembed - start) - 1e-12).all()
    if not use_mask and not use_flens:
        assert np.array_equal(f, h) and np.array_equal(dh, g)


@pytest.mark.parametrize("F", [HR.SPECAUG_F, 700])
def test_specaug_mask_holds_every_kind_of_row(F):
    """About 30 % of the rows; a masked valid row, a masked padding row and an unmasked padding row in the utterances where
    such rows exist: one utterance has no padding, one has all four kinds of row, one (length 0) is all padding.  F = 37 has them
    in that order (flens 37, 20, 0); F = 700 in the opposite one, so that the rows beyond 2048 are valid ones."""
    flens = HR.specaug_flens(F)
    mask = HR.specaug_mask(HR.SPECAUG_B, F, flens) != 0
    full, part, empty = (int(np.flatnonzero(c)[0]) for c in (flens == F, (flens > 0) & (flens < F), flens == 0))
    assert tuple(HR.specaug_flens(HR.SPECAUG_F)) == (37, 20, 0) and sorted((full, part, empty)) == [0, 1, 2]
    assert 0.2 < mask.mean() < 0.4
    pad = np.arange(F)[None, :] >= flens[:, None]
    assert (mask[full] & ~pad[full]).any() and (~mask[full] & ~pad[full]).any() and not pad[full].any()
    for kind in (mask[part] & ~pad[part], mask[part] & pad[part], ~mask[part] & pad[part], ~mask[part] & ~pad[part]):
        assert kind.any()
    assert pad[empty].all() and mask[empty].any() and (~mask[empty]).any()
    if F == 700:  # masked valid rows on both trips of the capped row groups
        m = np.arange(HR.SPECAUG_B * F).reshape(HR.SPECAUG_B, F)
        assert (mask & ~pad & (m < 2048)).any() and (mask & ~pad & (m >= 2048)).any()
    assert HR.SPECAUG_B * 700 > 2048 == 64 * 32  # the F = 700 shape: more rows than the capped grid's 64 row groups x 32 rows


@BOTH
@pytest.mark.parametrize("C", HR.SPECAUG_C)
def test_specaug_fwd_assertion_rejects_wrong_restatements(bf, C):
    B, F = HR.SPECAUG_B, HR.SPECAUG_F
    flens, mask, embed = HR.specaug_flens(F), HR.specaug_mask(B, F, None), HR.specaug_embed(C)
    bits = HR.pattern_bits(B * F * C, bf).reshape(B, F, C)
    # a different pattern per element of an utterance (bf16: but for the 1 in 256 that had an Inf / NaN exponent cleared), and
    # no two rows alike anywhere
    assert len(np.unique(bits[0])) >= F * C - (F * C // 256 if bf else 0)
    assert len(np.unique(bits.reshape(B * F, C), axis=0)) == B * F
    h = HR.from_bits(bits, bf)
    assert np.array_equal(HR.to_bits(h, bf), bits) and np.isfinite(h).all()
    ref = HR.to_bits(HR.specaug_fwd(h, mask, flens, embed, bf), bf)
    assert (RR.round_to(embed, bf) != 0).all()
    # the mask winning over padding
    wrong = HR.specaug_fwd(h, None, flens, embed, bf)
    wrong[mask != 0] = RR.round_to(embed, bf)
    _rejects("h", HR.to_bits(wrong, bf), ref)
    # the embedding not rounded to the storage type (bf16), padding ignored, the mask ignored, a stray write of a neighbour row
    if bf:
        assert (RR.round_bf16(embed) != embed).any()
    _rejects("h", HR.to_bits(HR.specaug_fwd(h, mask, None, embed, bf), bf), ref)
    _rejects("h", HR.to_bits(HR.specaug_fwd(h, None, flens, embed, bf), bf), ref)
    stray = HR.specaug_fwd(h, mask, flens, embed, bf)
    t = int(np.flatnonzero(mask[0] == 0)[0])
    stray[0, t] = stray[0, t + 1] if mask[0, t + 1] == 0 else h[0, t - 1]
    _rejects("h", HR.to_bits(stray, bf), ref)
    # no mask and no lengths: bit-identical
    assert np.array_equal(HR.to_bits(HR.specaug_fwd(h, None, None, embed, bf), bf), bits)


@BOTH
@pytest.mark.parametrize("F,C", HR.SPECAUG_BWD_SHAPES)
@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
def test_specaug_bwd_assertions_reject_wrong_restatements(bf, F, C, integer):
    B = HR.SPECAUG_B
    flens, mask = HR.specaug_flens(F), HR.specaug_mask(B, F, None)
    dh, start = HR.specaug_dh(F, C, bf, integer)
    assert np.array_equal(RR.round_to(dh, bf), dh) and np.array_equal(RR.round_f32(start), start) and (start != 0).all()
    ref_dh, ref_e, terms = HR.specaug_bwd(dh, mask, flens, start)
    if integer:
        assert np.array_equal(dh, np.round(dh)) and np.abs(dh).sum(axis=(0, 1)).max() + start.max() < 2 ** 24

        def rejects(got):
            _rejects("dembed", got, ref_e)
    else:
        bar = HR.colsum_bar(start, ref_e - start, terms)

        def rejects(got):
            _rejects("dembed", got - start, ref_e - start, bar)
    pad = np.arange(F)[None, :] >= flens[:, None]
    mk = mask != 0
    rejects(start + dh[mk].sum(axis=0))                       # padding rows counted
    rejects(start + dh[~pad].sum(axis=0))                     # unmasked rows counted
    rejects(start + ref_dh[mk & ~pad].sum(axis=0))            # dh zeroed before the sum is taken
    rejects(ref_e - start)                                    # the sum assigned instead of added
    rejects(start + dh[mk & ~pad][:-1].sum(axis=0))           # the last counted row dropped
    if F == 700:  # only the first trip over the 64 row groups: rows beyond 2048 never read
        m = np.arange(B * F).reshape(B, F) < 2048
        rejects(start + dh[mk & ~pad & m].sum(axis=0))
    # dh: a masked row or a padding row left standing
    for keep in (mk & ~pad, pad & ~mk):
        wrong = ref_dh.copy()
        wrong[keep] = dh[keep]
        _rejects("dh", HR.to_bits(wrong, bf), HR.to_bits(ref_dh, bf))


# ------------------------------------------------------------------------------------------------ masked column sum
@BOTH
@pytest.mark.parametrize("M", HR.COLSUM_M)
def test_colsum_assertions_reject_wrong_restatements(bf, M):
    for N in HR.COLSUM_N:
        for integer in (True, False):
            X, rowmask, flens, start = HR.colsum_case(M, N, bf, integer)
            assert X.shape == (M, N + 8) and np.isnan(X[:, N:]).all() and np.isfinite(X[:, :N]).all()
            assert len(flens) * HR.COLSUM_F >= M > (len(flens) - 1) * HR.COLSUM_F and all(m % HR.COLSUM_F for m in HR.COLSUM_M if m > 1)
            for rm, fl in ((None, None), (rowmask, None), (rowmask, flens)):
                ref, terms = HR.colsum(X, N, rm, fl, HR.COLSUM_F)
                assert np.isfinite(ref).all()
                if integer:
                    assert np.abs(X[:, :N]).sum(axis=0).max() + 9 < 2 ** 24

                    def rejects(got):
                        _rejects("colsum", start + got, start + ref)
                else:
                    def rejects(got):
                        _rejects("colsum", got, ref, HR.colsum_bar(start, ref, terms))
                rejects(np.where(np.arange(N) >= N - 8, 0.0, ref))          # a missing last chunk of 8 columns
                rejects(ref - X[0, :N])                                     # a dropped row (row 0 always counts)
                if rm is not None and M > 1:
                    rejects(HR.colsum(X, N)[0])                             # the row mask ignored
                if fl is not None and M > HR.COLSUM_F:
                    rejects(HR.colsum(X, N, rm)[0])                         # the lengths ignored
    # the scratch the two-stage path needs, and the capped row groups
    assert [HR.colsum_scratch_floats(m, 8) // 8 for m in HR.COLSUM_M] == [1, 1, 1, 2, 64, 64]
    assert HR.colsum_scratch_floats(2100, 8) == 64 * 8 and HR.colsum_scratch_floats(HR.SPECAUG_B * HR.SPECAUG_F, 768) == 4 * 768


# ------------------------------------------------------------------------------------------------ add, gelu-grad product
@BOTH
@pytest.mark.parametrize("n", HR.ELEMWISE_N)
def test_elementwise_assertions_reject_wrong_restatements(bf, n):
    assert HR.ELEMWISE_N[-1] == 4096 * 256 * 8 + 8 and all(v % 8 == 0 for v in HR.ELEMWISE_N)
    dy, pre, b = HR.elementwise_case(n, bf)
    for v in (dy, pre, b):
        assert v.shape == (n,) and np.array_equal(RR.round_to(v, bf), v)
    lo, mid, hi = HR.neighbours(6.0, bf)
    assert mid == 6.0 and (hi - 6.0) == (6.0 - lo) == (2.0 ** -5 if bf else 2.0 ** -21)  # one ulp of [4, 8) either side
    assert pre.min() == -12.0 and pre.max() == 12.0
    for e in (lo, mid, hi):
        assert (pre == e).any() and (pre == -e).any()
    if n > 8:  # [-12, 12] evenly (the eight leading values were replaced by the edges)
        assert np.abs(np.diff(np.sort(pre))).max() <= max(9 * 24.0 / (n - 1), 2.0 ** -3)
    # add: bit-exact
    ref = HR.add(dy, b, bf)
    nan = np.full(8, np.nan)
    short = np.concatenate([ref[:-8], nan])                   # a missing last chunk of 8 (the output starts from NaN)
    with pytest.raises(AssertionError):
        HR.check_equal("add", short, ref)
    if bf and n > 8:
        _rejects("add", RR.round_bf16(dy + b + HR.ulp_st(dy + b, True) * 0.51), ref)      # rounded up, not to nearest
    # product: one storage ulp + 1e-6 |dy|
    ref = HR.gelu_grad_mul(dy, pre, bf)
    bar = HR.product_bar(ref, dy, bf)
    HR.check_bar("product", RR.round_to(ref, bf), ref, bar)   # (the storage rounding itself passes)
    _rejects("product", np.concatenate([ref[:-8], nan]), ref, bar)
    _rejects("product", np.concatenate([ref[:-8], np.zeros(8)]), ref, bar)
    if n > 8:
        if not bf:  # the other GELU form: the fit is ~1e-5 from erf (under bf16's storage ulp, far over fp32's)
            _rejects("product", HR.gelu_grad_mul(dy, pre, True), ref, bar)
        _rejects("product", dy * RR.phi_exact(pre), ref, bar)     # Phi without the density term
    _rejects("product", dy * RR.gelu_forms(bf)[0](pre), ref, bar)  # gelu instead of gelu'


# ------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("R,C", HR.TRANSPOSE_SHAPES + ((64, 72), (8, 16)))
def test_transpose_assertion_rejects_an_untransposed_tile(R, C):
    src = HR.transpose_src(R, C)
    ref = HR.transpose(src)
    assert ref.shape == (C, R) and ref.flags["C_CONTIGUOUS"] and len(np.unique(src)) >= R * C - R * C // 256
    # every 64 x 64 tile lands at its transposed place but is written as read
    wrong = ref.copy()
    for r0 in range(0, R, 64):
        for c0 in range(0, C, 64):
            t = src[r0:r0 + 64, c0:c0 + 64]
            k = min(t.shape)
            wrong[c0:c0 + k, r0:r0 + k] = t[:k, :k]
    if min(R, C) > 1:
        _rejects("dst", wrong, ref)
    # the matrix copied, not transposed; the edge tiles' ragged part dropped
    if min(R, C) > 1:
        _rejects("dst", src.reshape(C, R), ref)
    if R % 64 or C % 64:
        wrong = ref.copy()
        wrong[C - C % 64 if C % 64 else C:, :] = 0
        wrong[:, R - R % 64 if R % 64 else R:] = 0
        _rejects("dst", wrong, ref)
    # which path the kernel takes: 16-byte vectors need both dimensions to be multiples of 8
    vec = {(8, 8): True, (64, 64): True, (65, 63): False, (72, 200): True, (136, 328): True, (1, 129): False, (64, 72): True,
           (8, 16): True}[(R, C)]
    assert ((R | C) & 7 == 0) == vec
    assert HR.TRANSPOSE_CAP + 1 == 113


# ------------------------------------------------------------------------------------------------ reductions
def test_reduce_assertions_reject_wrong_restatements():
    jobs = HR.reduce_jobs()
    assert len(jobs) == HR.REDUCE_CAP
    assert {j[2] for j in jobs} == set(HR.REDUCE_SLOTS) and {j[3] for j in jobs} == set(HR.REDUCE_NCOLS)
    for P, start, slots, ncols in jobs:
        assert P.shape == (slots, ncols + 3) and np.isnan(P[:, ncols:]).all() and (start != 0).all()
        assert np.array_equal(P[:, :ncols], np.round(P[:, :ncols])) and np.abs(P[:, :ncols]).sum(axis=0).max() + 9 < 2 ** 24
        ref = start + HR.reduce(P, slots, ncols)
        _rejects("out", start + HR.reduce(P, slots - 1, ncols) if slots > 1 else start, ref)   # the last slot dropped
        _rejects("out", ref - start, ref)                                                      # assigned, not added
        _rejects("out", np.concatenate([start[:1], ref[1:]]), ref)                             # a column left out
        if slots > 16:
            _rejects("out", start + P[::16, :ncols].sum(axis=0), ref)                          # only slot group 0
    # two jobs that share an out: the second one lost
    (P0, s0, k0, n0), (P1, _, k1, n1) = (jobs[i] for i in HR.REDUCE_SHARED)
    assert n0 == n1
    both = s0 + HR.reduce(P0, k0, n0) + HR.reduce(P1, k1, n1)
    _rejects("shared out", s0 + HR.reduce(P0, k0, n0), both)
    _rejects("shared out", s0 + HR.reduce(P1, k1, n1), both)
    # the sink scenario: 30 jobs fit, a call of 3 does not, a call of 2 fills the sink
    calls = HR.REDUCE_SINK_CALLS
    sj, out_of = HR.sink_jobs()
    assert len(sj) == sum(calls) == 35
    n, queued, direct = 0, 0, 0
    for c in calls:
        if n + c <= HR.REDUCE_CAP:
            n, queued = n + c, queued + c
        else:
            direct += c
    assert (queued, direct) == (32, 3) and n == HR.REDUCE_CAP
    assert out_of[30] == 0 and sj[30][3] == sj[0][3] and sorted(set(out_of)) == [i for i in range(35) if i != 30]
    # the real-valued case: the bar rejects a dropped slot
    for P, start, slots, ncols in HR.reduce_jobs(integer=False)[2:8]:
        ref, terms = HR.reduce(P, slots, ncols), np.abs(P[:slots, :ncols]).sum(axis=0)
        _rejects("out", HR.reduce(P, slots - 1, ncols), ref, HR.reduce_bar(slots, terms))


# ------------------------------------------------------------------------------------------------ waveform normalisation
@pytest.mark.parametrize("T", HR.WAVE_T)
def test_wave_reference_and_inputs(T):
    from oracle import w2v2_ref as R
    x, lens = HR.wave_case(T)
    assert T % 4 != 0 and list(lens) == [T, T - 1, 2, 1, 0] and abs(float(x[2, 0]) - float(x[2, 1])) >= 0.01
    for b in range(5):
        assert (x[b, lens[b]:] == 7.0).all()
    ref, mask = HR.wave_normalize(x, lens)
    assert (mask == (np.arange(T)[None, :] < lens[:, None])).all() and (ref[mask == 0] == 0).all()
    assert (ref[3] == 0).all() and (ref[4] == 0).all() and np.allclose(np.abs(ref[2, :2]), 1.0, atol=1e-4)
    for b in (0, 1):
        v = ref[b, :lens[b]]
        assert abs(v.mean()) < 1e-9 and abs(v.var() - 1) < 1e-4
    # the feature extractor's own formula (fp32) on the rows it handles
    other = R.zero_mean_unit_var_norm([x[b] for b in range(3)], lens[:3])
    assert np.abs(np.asarray(other) - ref[:3]).max() < 5e-5
    # the 5e-5 bar rejects: the unbiased variance on the length-2 row, padding entering the statistics, eps left out of a
    # constant row
    _rejects("wave", np.where(np.arange(T) < 2, ref[2] / np.sqrt(2.0), 0.0), ref[2], 5e-5)
    v = x[1].astype(np.float64)
    _rejects("wave", np.where(np.arange(T) < T - 1, (v - v.mean()) / np.sqrt(v.var() + 1e-7), 0.0), ref[1], 5e-5)


# ------------------------------------------------------------------------------------------------ the C entries' validation
def test_debug_helper_entries_reject_bad_arguments_before_any_launch():
    """SSAK_ERR_INVALID, decided on the host: every call here also lacks its operands or names a shape no kernel is built for."""
    import ssak_amd.hip as h
    L = h.lib
    assert L.ssak_version() == h.ABI_VERSION == 660

    def last():
        return L.ssak_last_error().decode()

    one = ctypes.c_void_p(16)  # (never dereferenced: every call below is refused first)
    assert L.ssak_debug_specaug_fwd(None, None, None, None, 1, 1, 8, 0, None) == h.SSAK_ERR_INVALID and "h null" in last()
    assert L.ssak_debug_specaug_fwd(one, None, None, None, 1, 1, 8, 2, None) == h.SSAK_ERR_INVALID and "dtype" in last()
    assert L.ssak_debug_specaug_fwd(one, one, None, None, 1, 1, 8, 0, None) == h.SSAK_ERR_INVALID and "embedding" in last()
    assert L.ssak_debug_specaug_bwd(one, one, None, one, 1, 1, 12, 0, None, 0, None) == h.SSAK_ERR_INVALID and "C=12" in last()
    assert L.ssak_debug_specaug_bwd(None, one, None, one, 1, 1, 8, 1, None, 0, None) == h.SSAK_ERR_INVALID
    for M, N, ld in ((0, 8, 8), (4, 12, 16), (4, 8, 12), (4, 16, 8)):
        assert L.ssak_debug_colsum(one, ld, M, N, one, None, 0, None, None, 0, 0, None) == h.SSAK_ERR_INVALID and f"ld={ld}" in last()
    assert L.ssak_debug_colsum(one, 8, 4, 8, one, None, 0, None, one, 4, 0, None) == h.SSAK_ERR_INVALID and "rowmask" in last()
    assert L.ssak_debug_colsum(one, 8, 4, 8, one, None, 0, one, one, 0, 0, None) == h.SSAK_ERR_INVALID and "F > 0" in last()
    assert L.ssak_debug_colsum(one, 8, 4, 8, one, None, 0, None, None, 0, 3, None) == h.SSAK_ERR_INVALID and "dtype" in last()
    for fn in (L.ssak_debug_gelu_grad_mul, L.ssak_debug_add):
        assert fn(one, one, one, 12, 0, None) == h.SSAK_ERR_INVALID and "n=12" in last()
        assert fn(one, one, one, 0, 0, None) == h.SSAK_ERR_INVALID
        assert fn(None, one, one, 8, 0, None) == h.SSAK_ERR_INVALID
        assert fn(one, one, one, 8, 7, None) == h.SSAK_ERR_INVALID and "dtype" in last()
    assert L.ssak_debug_transpose_batched(0, None, None, None, None, None) == h.SSAK_ERR_INVALID
    vp1, i1 = (ctypes.c_void_p * 1), (ctypes.c_int * 1)
    assert L.ssak_debug_transpose_batched(1, vp1(16), vp1(16), i1(0), i1(8), None) == h.SSAK_ERR_INVALID and "bad matrix 0" in last()
    assert L.ssak_debug_transpose_batched(1, vp1(None), vp1(16), i1(8), i1(8), None) == h.SSAK_ERR_INVALID

    def reduce(stride, slots, ncols, calls, n=1):
        q, d = ctypes.c_int(-1), ctypes.c_int(-1)
        vpn, inn = (ctypes.c_void_p * n), (ctypes.c_int * n)
        rc = L.ssak_debug_reduce(n, vpn(*[16] * n), vpn(*[16] * n), (ctypes.c_long * n)(*[stride] * n), inn(*[slots] * n),
                                 inn(*[ncols] * n), len(calls), (ctypes.c_int * len(calls))(*calls), 1, ctypes.byref(q), ctypes.byref(d),
                                 None)
        return rc

    assert reduce(8, 1, 8, [2]) == h.SSAK_ERR_INVALID and "add up" in last()
    assert reduce(8, 1, 8, [0, 1]) == h.SSAK_ERR_INVALID
    assert reduce(8, 1, 8, [33], n=33) == h.SSAK_ERR_INVALID and "33 jobs" in last()
    assert reduce(4, 1, 8, [1]) == h.SSAK_ERR_INVALID and "stride=4" in last()
    assert reduce(8, 0, 8, [1]) == h.SSAK_ERR_INVALID and "slots=0" in last()
    assert reduce(8, 1, 0, [1]) == h.SSAK_ERR_INVALID
    assert L.ssak_debug_reduce(0, None, None, None, None, None, 0, None, 0, None, None, None) == h.SSAK_ERR_INVALID
