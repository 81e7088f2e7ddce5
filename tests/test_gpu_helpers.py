"""GPU: the helper kernels the wav2vec2 engine launches between its row kernels and GEMMs, one launch function at a time, against
the float64 restatement tests/helpers_ref.py (itself pinned by tests/test_helpers_ref.py, which also shows that every assertion
made here rejects the obvious wrong restatements on these very inputs), through the test-only entries of ABI 660:
ssak_debug_specaug_fwd / _bwd, ssak_debug_colsum, ssak_debug_gelu_grad_mul, ssak_debug_add, ssak_debug_transpose_batched,
ssak_debug_reduce -- and two edges of existing entries (ssak_cast_f32_bf16, ssak_wave_normalize).

Which kernel instantiation and branch each case reaches (T = both bf16 and float unless named):

* specaug_fwd_kernel<T> (one 128-thread workgroup per row): C = 8 (120 idle threads), 136 (a second, partial trip), 768 (six
  trips); mask and lengths, mask alone, lengths alone (embed = NULL), neither (k_specaug_fwd_t returns before any launch):
  test_specaug_fwd.
* specaug_bwd_kernel<T> + colsum_kernel<T> with rowmask / flens / F, as k_specaug_bwd_t chains them: the same shapes and
  M = 3 x 700 = 2100 rows (gridDim.y capped at 64 row groups of 32: the groups' second trip); the two-stage path (partial rows
  + reduce_jobs_kernel), the atomic path (scratch = NULL) and the fall-back to atomics of a scratch one float too small; mask
  alone, lengths alone (no column sum: dembed untouched), neither: test_specaug_bwd.
* colsum_kernel<T> alone: M = 1, 31, 32, 33 (one row group, partly filled, full, a second one), 2048, 2049 (64 groups; one
  row on the second trip), N = 8 (one chunk of a 64-column block), 64, 72 (a second block with one live chunk), ld = N + 8 with
  NaN in the pad columns, no mask / rowmask with flens = NULL / rowmask + flens with F = 13, both paths: test_colsum.
* gelu_grad_mul_kernel<T> / add_kernel<T>: n = 8 (one live thread), 2048 (one full workgroup), 2056 (a second workgroup with one
  live thread), 8 388 616 = 4096 x 256 x 8 + 8 (the capped grid; thread 0 of block 0 takes a second trip of the grid-stride loop):
  test_add, test_gelu_grad_mul.
* transpose_bf16_kernel: the 16-byte path with full tiles (64, 64), with a partly filled tile (8, 8) and with ragged edge tiles
  in both directions (72, 200), (136, 328); the element-wise path for odd dimensions (65, 63), (1, 129) and for a misaligned
  source of an (64, 72) matrix; six matrices of different shapes in one launch; 113 matrices = two launches (112 + 1):
  test_transpose_*.
* reduce_jobs_kernel through k_reduce -> reduce_launch (direct) and through ReduceSink + k_reduce_flush: one call of 32 jobs
  (slots 1 .. 600: the unrolled loop's bounds 240 / 241 / 256 / 257, ncols 1 .. 200: partly filled column blocks, stride = ncols
  + 3); a sink that fills up (30 queued, a call of 3 that does not fit and runs at once, a call of 2 that fills it, the flush);
  reduce_launch's cut at a repeated out, within one call and across queued calls: test_reduce_*.
* cast_f32_bf16_kernel's scalar tail alone (n = 1 .. 7: no full float4): test_cast_below_one_vector.
* norm_stats_kernel / norm_apply_kernel with T % 4 != 0 (every chunk on the scalar path; T = 8191, 8193, 16385: one chunk not
  full, a second chunk of one sample, a third) and lengths T, T - 1, 2, 1, 0: test_wave_normalize_unaligned.

Bars (u = 2^-24, the fp32 unit roundoff):

* SpecAugment forward, dh after the backward, add, transpose, cast: bit-exact.  The kernels copy, zero or convert; add is one
  fp32 addition and one round-to-nearest-even conversion (tests/test_gpu_ops.py::test_cast_and_colsum_helpers pins the
  conversion), so the reference round_st(round_f32(a + b)) leaves no slack.  Untouched rows carry a distinct bit pattern per
  element and every output buffer is followed by guard elements that must come back unchanged.
* Column sums and reductions of small integers (|x| <= 4, column totals < 2^24): every partial sum is an integer fp32 holds
  exactly, so the result is bit-exact whatever the summation order -- two-stage, atomic, queued or direct.
* Real-valued column sums, added onto non-zero starting values: |got - start - ref| <= 1e-5 sum|terms| + 2^-23 (|start| +
  |ref|), the bar of tests/test_gpu_rowwise.py (at most 2100 fp32 additions per column: 2100 u = 1.3e-4 worst case, ~sqrt of
  that typically; 1e-5 is the bar the LayerNorm column sums already meet at 16 000 rows).  Two two-stage launches are
  bit-identical.
* gelu-grad product: |got - ref| <= one storage ulp of ref + 1e-6 |dy|; ref = dy gelu_grad_fit(pre) (bf16) or dy
  gelu_grad_exact(pre) (fp32).  1e-6 is what test_gelu_forms holds gelu' to in both forms; the fp32 multiplication and the
  storage rounding are within the ulp.
* Real-valued reduction (onto a start of 0, so the final += is exact): queued and direct bit-identical; |got - ref| <= slots u
  sum|terms| (at most ceil(slots / 16) - 1 additions within a slot group and 15 across the groups, <= slots in all, each within
  u of a partial sum of at most sum|terms|).
* Waveform normalisation: 5e-5 absolute, the bar of tests/test_gpu_ops.py::test_wave_normalize_full_size (values are O(1)
  to O(5); fp32 statistics merged in double); mask exact, padding exactly 0, rows of length 1 and 0 all zero.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import helpers_ref as HR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
PATHS = ("two_stage", "atomic", "short_scratch")


def _hip():
    import ssak_amd.hip as hip
    return hip


def _bits_dev(bits, dt):
    """Bit patterns (uint16 for bf16, uint32 for fp32) -> a device tensor of that type."""
    signed = np.ascontiguousarray(bits).view(np.int16 if dt == BF else np.int32)
    return torch.from_numpy(signed.copy()).view(dt).to(DEV)


def _bits_host(t):
    v = t.detach().cpu().contiguous()
    return v.view(torch.int16).numpy().view(np.uint16) if t.dtype == BF else v.view(torch.int32).numpy().view(np.uint32)


def _vals_dev(x, dt):
    """Float64 values the storage type holds exactly -> device."""
    return torch.tensor(np.asarray(x, dtype=np.float32), device=DEV).to(dt).contiguous()


def _host(t):
    return t.detach().double().cpu().numpy()


def _u8(a):
    return None if a is None else torch.tensor(np.asarray(a, dtype=np.uint8), device=DEV)


def _i32(a):
    return None if a is None else torch.tensor(np.asarray(a, dtype=np.int32), device=DEV)


# ------------------------------------------------------------------------------------------------ SpecAugment forward
@DTYPES
@pytest.mark.parametrize("C", HR.SPECAUG_C)
def test_specaug_fwd(dt, C):
    """Rows of length-0 / padded / full utterances under a 30 % mask: bit-exact, untouched rows and the guard untouched."""
    hip, bf = _hip(), dt == BF
    B, F = HR.SPECAUG_B, HR.SPECAUG_F
    flens, mask, embed = HR.specaug_flens(F), HR.specaug_mask(B, F, None), HR.specaug_embed(C)
    bits = HR.pattern_bits(B * F * C + C, bf)
    h = HR.from_bits(bits[:B * F * C], bf).reshape(B, F, C)
    t_embed = torch.tensor(embed, device=DEV)
    for use_mask, use_flens in ((True, True), (True, False), (False, True), (False, False)):
        m, fl = (mask if use_mask else None), (flens if use_flens else None)
        buf = _bits_dev(bits, dt)
        hip.debug_specaug_fwd(buf[:B * F * C].view(B, F, C), _u8(m), _i32(fl), t_embed if use_mask else None)
        torch.cuda.synchronize()
        got = _bits_host(buf)
        ref = HR.to_bits(HR.specaug_fwd(h, m, fl, embed, bf), bf)
        name = f"h (mask={use_mask}, flens={use_flens})"
        HR.check_equal(name, got[:B * F * C].reshape(B, F, C), ref)
        HR.check_equal(name + " guard", got[B * F * C:], bits[B * F * C:])
        if not use_mask and not use_flens:
            HR.check_equal(name + " untouched", got, bits)


# ------------------------------------------------------------------------------------------------ SpecAugment backward
def _scratch(path, need):
    """(scratch tensor, scratch_floats) of a column-sum path; the scratch starts from NaN."""
    if path == "atomic":
        return None, 0
    s = torch.full((need,), float("nan"), dtype=F32, device=DEV)
    return s, (need if path == "two_stage" else need - 1)


@DTYPES
@pytest.mark.parametrize("F,C", HR.SPECAUG_BWD_SHAPES, ids=[f"F{f}-C{c}" for f, c in HR.SPECAUG_BWD_SHAPES])
@pytest.mark.parametrize("path", PATHS)
def test_specaug_bwd(dt, F, C, path):
    """dembed += the masked valid rows (before they are zeroed), masked and padding rows of dh zeroed, on the three column-sum
    paths: integer data bit-exact, real data within the column sums' bar; the two-stage path twice, bit-identical."""
    hip, bf = _hip(), dt == BF
    B = HR.SPECAUG_B
    flens, mask = HR.specaug_flens(F), HR.specaug_mask(B, F, None)
    need = HR.colsum_scratch_floats(B * F, C)
    guard = HR.from_bits(HR.pattern_bits(C, bf, salt=5), bf)
    for integer in (True, False):
        dh, start = HR.specaug_dh(F, C, bf, integer)
        for use_mask, use_flens in ((True, True), (True, False), (False, True), (False, False)):
            m, fl = (mask if use_mask else None), (flens if use_flens else None)
            ref_dh, ref_e, terms = HR.specaug_bwd(dh, m, fl, start)

            def launch():
                buf = _vals_dev(np.concatenate([dh.reshape(-1), guard]), dt)
                de = _vals_dev(np.concatenate([start, [123.0]]), F32)
                s, nf = _scratch(path, need)
                hip.debug_specaug_bwd(buf[:B * F * C].view(B, F, C), _u8(m), _i32(fl), de[:C], s, nf)
                torch.cuda.synchronize()
                return _host(buf), _host(de)

            got_dh, got_e = launch()
            name = f"(integer={integer}, mask={use_mask}, flens={use_flens}, {path})"
            HR.check_equal("dh " + name, HR.to_bits(got_dh[:B * F * C], bf).reshape(B, F, C), HR.to_bits(ref_dh, bf))
            HR.check_equal("dh guard " + name, got_dh[B * F * C:], guard)
            assert got_e[C] == 123.0, "dembed guard " + name
            if integer or not use_mask:
                HR.check_equal("dembed " + name, got_e[:C], ref_e)
            else:
                HR.check_bar("dembed " + name, got_e[:C] - start, ref_e - start, HR.colsum_bar(start, ref_e - start, terms))
            if path == "two_stage" and use_mask and use_flens:
                again = launch()
                HR.check_equal("dembed, second launch " + name, again[1], got_e)


# ------------------------------------------------------------------------------------------------ the column sum alone
@DTYPES
@pytest.mark.parametrize("M", HR.COLSUM_M)
@pytest.mark.parametrize("path", ("two_stage", "atomic"))
def test_colsum(dt, M, path):
    """k_colsum_t as the engine calls it (out +=), ld = N + 8 with NaN in the pad columns: no mask, a row mask, a row mask with
    lengths (F = 13)."""
    hip, bf = _hip(), dt == BF
    for N in HR.COLSUM_N:
        for integer in (True, False):
            X, rowmask, flens, start = HR.colsum_case(M, N, bf, integer)
            tX = _vals_dev(X, dt)
            assert tX.shape == (M, N + 8) and bool(torch.isnan(tX[:, N:]).all())
            for rm, fl in ((None, None), (rowmask, None), (rowmask, flens)):
                ref, terms = HR.colsum(X, N, rm, fl, HR.COLSUM_F)
                out = _vals_dev(np.concatenate([start, [123.0]]), F32)
                s, nf = _scratch(path, HR.colsum_scratch_floats(M, N))
                hip.debug_colsum(tX, N, out[:N], s, nf, _u8(rm), _i32(fl), HR.COLSUM_F if fl is not None else 0)
                torch.cuda.synchronize()
                got = _host(out)
                name = f"colsum (N={N}, integer={integer}, rowmask={rm is not None}, flens={fl is not None})"
                assert got[N] == 123.0, name + " guard"
                if integer:
                    HR.check_equal(name, got[:N], start + ref)
                else:
                    HR.check_bar(name, got[:N] - start, ref, HR.colsum_bar(start, ref, terms))


# ------------------------------------------------------------------------------------------------ add, gelu-grad product
def _elementwise(dt, n, which):
    hip, bf = _hip(), dt == BF
    dy, pre, b = HR.elementwise_case(n, bf)
    sentinel = np.full(8, 77.0)
    t1 = _vals_dev(np.concatenate([dy, sentinel]), dt)
    t2 = _vals_dev(np.concatenate([b if which == "add" else pre, sentinel]), dt)
    out = torch.full((n + 8,), float("nan"), dtype=dt, device=DEV)
    out[n:] = 77.0
    (hip.debug_add if which == "add" else hip.debug_gelu_grad_mul)(t1, t2, out, n)
    torch.cuda.synchronize()
    got = _host(out)
    HR.check_equal(which + " sentinel", got[n:], sentinel)
    return got[:n], dy, pre, b


@DTYPES
@pytest.mark.parametrize("n", HR.ELEMWISE_N)
def test_add(dt, n):
    """add_kernel: bit-exact against round_st(round_f32(a + b)), nothing written behind element n."""
    got, a, _, b = _elementwise(dt, n, "add")
    HR.check_equal("add", got, HR.add(a, b, dt == BF))


@DTYPES
@pytest.mark.parametrize("n", HR.ELEMWISE_N)
def test_gelu_grad_mul(dt, n):
    """gelu_grad_mul_kernel over pre in [-12, 12] with the clamp points +-6 and their neighbours."""
    got, dy, pre, _ = _elementwise(dt, n, "product")
    ref = HR.gelu_grad_mul(dy, pre, dt == BF)
    HR.check_bar("product", got, ref, HR.product_bar(ref, dy, dt == BF))


# ------------------------------------------------------------------------------------------------ batched transpose
GUARD = 64


def _transpose(shapes, src_offset_elems=0):
    """One k_transpose_bf16_batched call on matrices of `shapes`; every destination is followed by GUARD guard elements."""
    hip = _hip()
    srcs, dsts, refs = [], [], []
    for i, (R, C) in enumerate(shapes):
        bits = HR.transpose_src(R, C, salt=977 * i)
        buf = _bits_dev(np.concatenate([np.zeros(src_offset_elems, dtype=np.uint16), bits.reshape(-1)]), BF)
        srcs.append(buf)
        dsts.append(_bits_dev(HR.pattern_bits(R * C + GUARD, True, salt=31 + i), BF))
        refs.append(HR.transpose(bits))
    hip.debug_transpose_batched([s.data_ptr() + 2 * src_offset_elems for s in srcs], [d.data_ptr() for d in dsts],
                                [r for r, _ in shapes], [c for _, c in shapes])
    torch.cuda.synchronize()
    for i, (R, C) in enumerate(shapes):
        got = _bits_host(dsts[i])
        HR.check_equal(f"dst {i} ({R}, {C})", got[:R * C].reshape(C, R), refs[i])
        HR.check_equal(f"dst {i} ({R}, {C}) guard", got[R * C:], HR.pattern_bits(R * C + GUARD, True, salt=31 + i)[R * C:])


@pytest.mark.parametrize("R,C", HR.TRANSPOSE_SHAPES)
def test_transpose_one_matrix(R, C):
    """The 16-byte path (full, partly filled and ragged edge tiles) and the element-wise path of odd dimensions."""
    _transpose([(R, C)])


def test_transpose_misaligned_source():
    """(64, 72): dimensions that allow the 16-byte path, a source two bytes off a 16-byte boundary: the element-wise path."""
    _transpose([(64, 72)], src_offset_elems=1)


def test_transpose_mixed_batch():
    """All the shapes in one launch: each workgroup finds its matrix and its tile."""
    _transpose(list(HR.TRANSPOSE_SHAPES))


def test_transpose_more_than_one_launch():
    """113 distinct (8, 16) matrices: a launch of 112 and one of 1 that must use the second group's pointers."""
    _transpose([(8, 16)] * (HR.TRANSPOSE_CAP + 1))


# ------------------------------------------------------------------------------------------------ deferred reductions
def _reduce(jobs, out_of, calls, use_sink):
    """jobs [(partial, start, slots, ncols)], out_of[i] = the output vector job i adds into (its start is that of the first job
    naming it).  Returns ({vector: host array without its guard}, queued, direct)."""
    hip = _hip()
    outs = {}
    for i, o in enumerate(out_of):
        if o not in outs:
            outs[o] = torch.tensor(np.concatenate([jobs[i][1], [123.0]]), dtype=F32, device=DEV)
    parts = [torch.tensor(j[0], dtype=F32, device=DEV) for j in jobs]
    table = [(parts[i], outs[out_of[i]], jobs[i][0].shape[1], jobs[i][2], jobs[i][3]) for i in range(len(jobs))]
    queued, direct = hip.debug_reduce(table, calls, use_sink)
    torch.cuda.synchronize()
    res = {}
    for o, t in outs.items():
        h = _host(t)
        assert h[-1] == 123.0, f"out {o}: guard overwritten"
        res[o] = h[:-1]
    return res, queued, direct


def _reduce_ref(jobs, out_of):
    ref = {}
    for i, o in enumerate(out_of):
        P, start, slots, ncols = jobs[i]
        ref[o] = ref.get(o, start) + HR.reduce(P, slots, ncols)
    return ref


@pytest.mark.parametrize("use_sink", [False, True], ids=["direct", "queued"])
def test_reduce_one_call_of_32_jobs(use_sink):
    """A full table: every loop bound of the sixteen-loads-in-flight loop and partly filled column blocks, stride > ncols, outs
    starting non-zero; integer partials, bit-exact.  Queued: the 32 jobs fill the sink exactly and run in the flush."""
    jobs = HR.reduce_jobs()
    out_of = list(range(len(jobs)))
    got, queued, direct = _reduce(jobs, out_of, [len(jobs)], use_sink)
    assert (queued, direct) == ((32, 0) if use_sink else (0, 32))
    for o, r in _reduce_ref(jobs, out_of).items():
        HR.check_equal(f"out {o} (slots {jobs[o][2]}, ncols {jobs[o][3]})", got[o], r)


def test_reduce_sink_overflow():
    """Calls of 3 until 30 jobs wait, a call of 3 that does not fit (it must run at once, whole), a call of 2 that fits, the
    flush; the call that ran at once and a queued job add into one vector.  Every out is right and the counts say which way
    each job went."""
    jobs, out_of = HR.sink_jobs()
    got, queued, direct = _reduce(jobs, out_of, list(HR.REDUCE_SINK_CALLS), True)
    assert (queued, direct) == (32, 3), "the overflow branch of k_reduce was not taken as expected"
    for o, r in _reduce_ref(jobs, out_of).items():
        HR.check_equal(f"out {o}", got[o], r)
    # the same calls without a sink
    got, queued, direct = _reduce(jobs, out_of, list(HR.REDUCE_SINK_CALLS), False)
    assert (queued, direct) == (0, 35)
    for o, r in _reduce_ref(jobs, out_of).items():
        HR.check_equal(f"out {o} (direct)", got[o], r)


@pytest.mark.parametrize("calls,use_sink", [([2], False), ([2], True), ([1, 1], True), ([1, 1], False)],
                         ids=["one_call-direct", "one_call-queued", "two_calls-queued", "two_calls-direct"])
def test_reduce_shared_out(calls, use_sink):
    """Two jobs adding into the same vector (plain += in the kernel: reduce_launch must not put them into one launch): both
    contributions arrive, whether the jobs come in one call or are queued by two."""
    all_jobs = HR.reduce_jobs()
    jobs = [all_jobs[i] for i in HR.REDUCE_SHARED]
    got, queued, direct = _reduce(jobs, [0, 0], calls, use_sink)
    assert (queued, direct) == ((2, 0) if use_sink else (0, 2))
    HR.check_equal("shared out", got[0], _reduce_ref(jobs, [0, 0])[0])
    # ... and with a third job between them that adds elsewhere
    jobs = [jobs[0], all_jobs[3], jobs[1]]
    got, _, _ = _reduce(jobs, [0, 1, 0], [3] if len(calls) == 1 else [1, 1, 1], use_sink)
    for o, r in _reduce_ref(jobs, [0, 1, 0]).items():
        HR.check_equal(f"shared out, three jobs: out {o}", got[o], r)


def test_reduce_real_valued():
    """N(0, 1) partials: the queued and the direct second stage are bit-identical (one summation order, whatever shares the
    launch) and within slots u sum|terms| of float64."""
    jobs = HR.reduce_jobs(integer=False)
    out_of = list(range(len(jobs)))
    a, _, _ = _reduce(jobs, out_of, [len(jobs)], False)
    b, queued, _ = _reduce(jobs, out_of, [5, 9, 18], True)
    assert queued == 32
    for o, (P, start, slots, ncols) in enumerate(jobs):
        HR.check_equal(f"out {o}: queued against direct", b[o], a[o])
        ref, terms = HR.reduce(P, slots, ncols), np.abs(P[:slots, :ncols]).sum(axis=0)
        assert not start.any()
        HR.check_bar(f"out {o}", a[o], ref, HR.reduce_bar(slots, terms))


# ------------------------------------------------------------------------------------------------ edges of existing entries
def test_cast_below_one_vector():
    """ssak_cast_f32_bf16 for n = 1 .. 7: the scalar tail without any full vector; nothing written behind element n."""
    hip = _hip()
    g = torch.Generator().manual_seed(7)
    for n in range(1, 8):
        x = torch.randn(8, generator=g).to(DEV)
        out = torch.full((8,), 77.0, dtype=BF, device=DEV)
        hip.check(hip.lib.ssak_cast_f32_bf16(hip.ptr(x), hip.ptr(out), n, hip.stream()))
        torch.cuda.synchronize()
        assert torch.equal(out[:n], x[:n].to(BF)), n
        assert bool((out[n:] == 77.0).all()), n


@pytest.mark.parametrize("T", HR.WAVE_T)
def test_wave_normalize_unaligned(T):
    """T % 4 != 0: every chunk takes the scalar path in both kernels; lengths T, T - 1, 2, 1, 0 with 7.0 in the padding."""
    hip = _hip()
    x, lens = HR.wave_case(T)
    out, mask = hip.wave_normalize(torch.tensor(x, device=DEV), torch.tensor(lens, device=DEV), return_mask=True)
    torch.cuda.synchronize()
    ref, ref_mask = HR.wave_normalize(x, lens)
    got, got_mask = _host(out), mask.cpu().numpy()
    HR.check_equal("mask", got_mask, ref_mask)
    HR.check_bar("normalised", got, ref, 5e-5)
    assert (got[ref_mask == 0] == 0).all(), "padding is not exactly 0"
    assert (got[3] == 0).all() and (got[4] == 0).all(), "rows of length 1 and 0 are not all zero"
