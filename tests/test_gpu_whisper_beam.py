"""GPU: Whisper beam search (ABI 630) -- ssak_dec_beam_topk, ssak_dec_beam_select, ssak_dec_kv_reorder (ssak_amd/csrc/whisper_beam.hip),
ssak_dec_attention_step_grouped (whisper_generate.hip), ``WhisperSeq2Seq._beam_step`` / ``generate(beam_size=...)`` (ssak_amd/whisper_seq2seq.py),
``transcribe(beam_size=...)`` and ``python -m ssak_amd.whisper_infer --beam_size`` -- against the float64 restatements
tests/whisper_beam_ref.py (held to whisper's literal dict form by tests/test_whisper_beam_ref.py), tests/whisper_timestamps_ref.py and
tests/whisper_generate_ref.py.  Every case prints its distances before it asserts.

Bars (fixed before the first run).  u = 2^-24.
* ssak_dec_beam_topk.  Candidate tokens and their slot order: exact (the device orders by the logit, the restatement by the
  float64 log-prob, the same order; equal logits are equal log-probs in both).  Log-probs: the greedy step's formula
  (tests/test_gpu_whisper_generate.py) with x_t the candidate's logit: rel = (4 D + K + 6) u, D = max_c |x_c - M| over the columns
  the rules allow BEFORE the mass decision (the columns the kernel's sums run over; M their maximum), K = ceil(V / 256) + 10,
  bar = rel + 2 u (|log s| + |M| + |lse|) + 2 u (|x_t| + |logprob|), s = the final row's sum of exp(x - M).
  The first candidate at nb = 1 against ssak_dec_greedy_step / ssak_dec_timestamp_step on the same buffers: token and fp32 log-prob
  equal bit for bit (the kernels share the scan, the reductions and the log-prob arithmetic of whisper_step.h).
* ssak_dec_beam_select: everything exact; the score is one fp32 add (np.float32 in the restatement).
* ssak_dec_kv_reorder: gathered rows bit-exact, every other byte unchanged.  ssak_dec_attention_step_grouped: bit for bit.
* The loop by hand: tokens, sources, finished lists exact; sums within (the row's log-prob bar + u |sum|).  A step is exempt only
  when the float64 margin between two candidates whose order matters -- neighbours in the walk up to the candidate behind the
  last one read, and neighbours among each offering row's first K + 1 columns -- is below 4 x that bar; at most one step.  The
  float64 restatement alone (whisper_beam_ref.search_array on whisper_decoder_ref, the same prompt and open-token list, on the
  CPU) showed 0 such (audio, step) pairs of 24, its smallest margin 2.2e-3.
* generate: beam_size = 1 against the default call: tokens identical, |sum difference| <= n u sum |logprob|.  Every candidate's
  per-token log-probs against the project's teacher-forced pass: 2 x 7.76e-2 (each path within 7.76e-2 of float64).
"""
import json
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_beam_ref as BR  # noqa: E402
import whisper_decoder_ref as WR  # noqa: E402
import whisper_generate_ref as GR  # noqa: E402
import whisper_timestamps_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
LP_BAR = 7.76e-2
V, LDV, EOS, PAD, NOTS, TSB = 127, 128, G.EOT, 3, G.NO_TIMESTAMPS, G.NO_TIMESTAMPS + 1
De, MAXP = 136, 16
NB, K = 3, 4


@pytest.fixture(scope="module")
def hip():
    import ssak_amd.hip as hip
    return hip


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


def mask_of(ids, n=V):
    m = np.zeros(n, np.uint8)
    m[list(ids)] = 1
    return torch.from_numpy(m).to(DEV)


# ------------------------------------------------------------------------------------------------------------ 1. top-K
def ref_row(x64, hist, timestamps, sup, bsup, first, max_initial, tsb=TSB, nots=NOTS, eos=EOS):
    """-> (log-prob [V] of the processed row, -inf where masked; pre = the columns allowed before the mass decision)."""
    n = x64.shape[0]
    if timestamps:
        pre = TR.allowed_columns(n, hist, tsb, nots, eos, max_initial, sup, bsup if first else None)
        row = TR.timestamp_step_row(x64, hist, tsb, nots, eos, max_initial, sup, bsup if first else None)
        final = row["mask"]
    else:
        pre = np.ones(n, dtype=bool)
        for ids in (sup, bsup if first else None):
            if ids:
                pre[list(ids)] = False
        final = pre
    if not final.any():
        return np.full(n, -np.inf), pre
    return BR.log_softmax(np.where(final, x64, -np.inf)), pre


def topk_bar(x64, pre, lp_row, token):
    M = x64[pre].max()
    Dm = np.abs(x64[pre] - M).max()
    final = np.isfinite(lp_row)
    s = np.exp(x64[final] - M).sum()
    rel = (4 * Dm + math.ceil(x64.shape[0] / 256) + 10 + 6) * U
    return rel + 2 * U * (abs(np.log(s)) + abs(M) + abs(M + np.log(s))) + 2 * U * (abs(x64[token]) + abs(lp_row[token]))


def run_topk(hip, x, Vn, hists, t, name, nb=NB, timestamps=True, ts_in=None, done=None, sup=(), bsup=(), max_initial=-1, tsb=TSB, nots=NOTS, eos=EOS,
             ldt=8):
    """One launch on rows x [R, ldv] (R a multiple of nb) whose histories (length t) sit in the token buffer; every row against
    the float64 restatement.  -> (cand_token, cand_logprob) as numpy."""
    R, Kn = x.shape[0], nb + 1
    assert R % nb == 0
    tokens = torch.full((R, ldt), -5, dtype=torch.int32)
    for r, h in enumerate(hists):
        assert len(h) == t
        tokens[r, :t] = torch.tensor(h, dtype=torch.int32)
    done = [0] * (R // nb) if done is None else done
    ct = torch.full((R, Kn), 77, dtype=torch.int32, device=DEV)
    cl = torch.full((R, Kn), 9.0, dtype=torch.float32, device=DEV)
    hip.dec_beam_topk(x.to(DEV) if x.device.type == "cpu" else x, Vn, nb, done=torch.tensor(done, dtype=torch.uint8, device=DEV), cand_token=ct,
                      cand_logprob=cl, eos_id=eos, t=t, suppress=mask_of(sup, Vn) if sup else None, begin_suppress=mask_of(bsup, Vn) if bsup else None,
                      first=t == 0, timestamps=timestamps, ts_begin=tsb, no_timestamps_id=nots, max_initial=max_initial,
                      tokens=tokens.to(DEV) if timestamps else None,
                      ts_last=torch.tensor(ts_in if ts_in is not None else [-1] * R, dtype=torch.int32, device=DEV) if timestamps else None)
    torch.cuda.synchronize()
    ct, cl = ct.cpu().numpy(), cl.double().cpu().numpy()
    x64 = x[:, :Vn].double().cpu().numpy()
    worst = 0.0
    for r in range(R):
        if done[r // nb]:
            assert (ct[r] == 77).all() and (cl[r] == 9.0).all(), (name, r, "a done audio's rows are untouched")
            continue
        lp_row, pre = ref_row(x64[r], list(hists[r]), timestamps, list(sup), list(bsup), t == 0, max_initial if max_initial >= 0 else None, tsb, nots,
                              eos)
        want = BR.topk_stable(lp_row, Kn)
        n = len(want)
        assert ct[r, :n].tolist() == [c for c, _ in want], (name, r, ct[r].tolist(), want)
        assert (ct[r, n:] == -1).all() and (cl[r, n:] == -np.inf).all(), (name, r, "unused slots hold -1 / -inf")
        for k, (c, lp) in enumerate(want):
            err, bar = abs(cl[r, k] - lp), topk_bar(x64[r], pre, lp_row, c)
            worst = max(worst, err / bar)
            assert err <= bar, (name, r, k, err, bar)
    print(f"beam top-K {name}: tokens {ct.tolist()}, worst log-prob err / bar {worst:.3f}")
    return ct, cl


def base_rows(R, seed, ldv=LDV, Vn=V):
    x = torch.randn(R, ldv, generator=torch.Generator().manual_seed(seed))
    x[:, Vn:] = 1e30
    return x


def test_beam_topk_planted_rows(hip):
    """The rule states of tests/test_gpu_whisper_timestamps.py's planted rows (V = 127 in 128 columns, +1e30 in the pad column),
    nb = 3, K = 4, rows grouped by step; every row's K candidates against the restatement."""
    # ---- t = 0: first step with max_initial 5 and both masks, then without max_initial
    x = base_rows(6, 41)
    x[0, 17] = 12.0
    x[0, TSB + 2] = 6.0
    x[1, TSB + 9] = 12.0
    x[1, TSB + 5] = 6.0
    x[2, TSB + 1] = 12.0
    x[2, TSB + 3] = 9.0
    x[2, TSB + 0] = 6.0
    x[3, NOTS] = 12.0
    x[3, TSB + 4] = 6.0
    x[4, TSB + 1] = 12.0
    x[5, TSB + 4] = 6.0
    x[5, EOS] = 12.0
    sup, bsup = [TSB + 1, 50], [TSB + 3, 60]
    ct, _ = run_topk(hip, x, V, [[]] * 6, 0, "t=0 max_initial=5", sup=sup, bsup=bsup, max_initial=5, ts_in=[120, 121, 122, 123, 77, 125])
    assert ct[[0, 1, 2, 3, 5], 0].tolist() == [TSB + 2, TSB + 5, TSB, TSB + 4, TSB + 4] and (ct >= TSB).all() and (ct <= TSB + 5).all()
    ct, _ = run_topk(hip, x, V, [[]] * 6, 0, "t=0 no max_initial", sup=sup, bsup=bsup, ts_in=[-1] * 6)
    assert ct[[0, 1, 2, 3, 5], 0].tolist() == [TSB + 2, TSB + 9, TSB, TSB + 4, TSB + 4] and (ct >= TSB).all()
    # ---- t = 1, after [ts]: timestamps masked although they dominate; an eos row; a row with TWO allowed columns (fewer than K)
    x = base_rows(3, 42)
    x[0, TSB + 6:V] = 12.0
    x[0, 33] = 6.0
    x[1, EOS] = 9.0
    hists = [[TSB + 2]] * 3
    ct, _ = run_topk(hip, x, V, hists, 1, "t=1", ts_in=[TSB + 2] * 3)
    assert ct[0, 0] == 33 and ct[1, 0] == EOS and (ct < TSB).all()
    few = [c for c in range(TSB) if c not in (20, 61)]
    ct, cl = run_topk(hip, x, V, hists, 1, "t=1, two allowed columns", ts_in=[TSB + 2] * 3, sup=few)
    assert sorted(ct[0, :2].tolist()) == [20, 61] and ct[0, 2:].tolist() == [-1, -1] and np.isinf(cl[0, 2:]).all()
    # ---- t = 2, after [ts, text]: the mass rule won (every candidate a timestamp) and lost; <|notimestamps|>; an exact tie
    x = base_rows(6, 43)
    x[0, 40] = 8.0
    x[0, TSB:V] = 6.2
    x[0, TSB + 7] = 7.0
    x[0, TSB + 1] = 30.0
    x[1, 40] = 12.0
    x[2, NOTS] = 20.0
    x[2, 41] = 9.0
    x[3, TSB + 8] = x[3, TSB + 12] = 9.0
    hists = [[TSB + 4, 7]] * 6
    ct, cl = run_topk(hip, x, V, hists, 2, "t=2", ts_in=[TSB + 4] * 6)
    assert ct[0].tolist() == [TSB + 7, TSB + 5, TSB + 6, TSB + 8], "mass won: timestamps only, the tie of the 6.2s to the lowest columns"
    assert ct[1, 0] == 40 and ct[2, 0] == 41 and ct[3, :2].tolist() == [TSB + 8, TSB + 12] and cl[3, 0] == cl[3, 1]
    # ---- t = 3, after [ts, text, ts]; t = 4, after [ts, text, ts, ts]
    x = base_rows(3, 44)
    x[0, 40] = 15.0
    x[0, TSB + 2] = 14.0
    x[0, TSB + 6] = 9.0
    x[1, EOS] = 12.0
    ct, _ = run_topk(hip, x, V, [[TSB + 4, 7, TSB + 6]] * 3, 3, "t=3", ts_in=[TSB + 6] * 3)
    assert ct[0, 0] == TSB + 6 and ct[1, 0] == EOS and (ct >= EOS).all()
    x = base_rows(3, 45)
    x[0, TSB + 9] = 12.0
    x[0, 21] = 6.0
    ct, _ = run_topk(hip, x, V, [[TSB + 4, 7, TSB + 6, TSB + 6]] * 3, 4, "t=4", ts_in=[TSB + 6] * 3)
    assert ct[0, 0] == 21 and (ct < TSB).all()


def test_beam_topk_greedy_mode_done_audio_and_paths(hip):
    """The greedy predicate (the two masks alone; tokens / ts_last not given); a done audio's rows untouched; an unaligned ldv (the
    non-vector path); nb = 1, 5, 8."""
    x = base_rows(6, 51)
    top = float(x[:, :V].max())
    x[0, 50] = top + 5      # suppressed
    x[1, 60] = top + 3      # begin-suppressed
    x[2, 17] = x[2, 90] = top + 1
    x[3, EOS] = top + 2
    x[5, V - 1] = top + 2
    for first in (True, False):
        ct, cl = run_topk(hip, x, V, [[]] * 6 if first else [[5, 6]] * 6, 0 if first else 2, f"greedy mode first={first}", timestamps=False,
                          sup=[50, 120], bsup=[60, 3], done=[0, 1])
        assert ct[0, 0] != 50 and (ct[1, 0] == 60) == (not first) and ct[2, :2].tolist() == [17, 90] and cl[2, 0] == cl[2, 1]
    xo = torch.full((6, 131), 1e30)
    xo[:, :V] = x[:, :V]
    a, la = run_topk(hip, xo.to(DEV)[:, :129], V, [[TSB + 4, 7]] * 6, 2, "unaligned ldv", ts_in=[TSB + 4] * 6)
    b, lb = run_topk(hip, x, V, [[TSB + 4, 7]] * 6, 2, "aligned", ts_in=[TSB + 4] * 6)
    assert np.array_equal(a, b), "the vector and the scalar path choose the same candidates (their sums run in another order: both within the bar)"
    for nb in (1, 5, 8):
        run_topk(hip, base_rows(2 * nb, 52 + nb), V, [[TSB + 4, 7]] * (2 * nb), 2, f"nb={nb}", nb=nb, ts_in=[TSB + 4] * (2 * nb))


def test_beam_topk_vocabulary_width(hip):
    """V = 51 865 in a 51 872-column buffer: the best columns sit at the end, the very best in the one-column tail behind the vector
    loop; with the rules (ts_begin 50 364, after [ts, text]) and without."""
    Vw, ldv, tsb, nots, eos = 51865, 51872, 50364, 50363, 50257
    x = 3 * torch.randn(3, ldv, generator=torch.Generator().manual_seed(47))
    x[:, Vw:] = 1e30
    x[0, 1000] = 40.0
    x[1, Vw - 1] = 40.0
    x[1, Vw - 2] = 39.0
    x[1, Vw - 5] = 38.0
    x[2, Vw - 1] = 30.0
    x[2, 7] = 30.0
    x[2, Vw - 3] = 29.0  # (with the rules: S_ts = 1 + e^-1 against a text maximum at M, a margin of 0.31)
    hists = [[tsb + 10, 500]] * 3
    ct, _ = run_topk(hip, x, Vw, hists, 2, "V=51865 with rules", ts_in=[tsb + 10] * 3, max_initial=50, tsb=tsb, nots=nots, eos=eos)
    assert ct[0, 0] == 1000 and ct[1, :3].tolist() == [Vw - 1, Vw - 2, Vw - 5]
    ct, _ = run_topk(hip, x, Vw, hists, 2, "V=51865 greedy mode", timestamps=False, tsb=tsb, nots=nots, eos=eos)
    assert ct[1, :3].tolist() == [Vw - 1, Vw - 2, Vw - 5] and ct[2, :2].tolist() == [7, Vw - 1]


def step_and_top1(hip, x, hists, t, timestamps, ts_in=None, sup=(), bsup=(), max_initial=-1, ldt=8):
    """ssak_dec_beam_topk at nb = 1, then the token step (ssak_dec_timestamp_step with ``timestamps``, else ssak_dec_greedy_step), on
    the same device logits, masks, histories and ts_last; every row unfinished -> (the step's tokens [R] int32 and log-probs [R] fp32,
    the top-K's first candidates, the same types), on the host."""
    R = x.shape[0]
    tokens = torch.full((R, ldt), -5, dtype=torch.int32)
    for r, h in enumerate(hists):
        assert len(h) == t
        tokens[r, :t] = torch.tensor(h, dtype=torch.int32)
    tokens = tokens.to(DEV)
    lps = torch.full((R, ldt), 9.0, dtype=torch.float32, device=DEV)
    ts_last = torch.tensor(ts_in if ts_in is not None else [-1] * R, dtype=torch.int32, device=DEV)
    ct = torch.full((R, 2), 77, dtype=torch.int32, device=DEV)
    cl = torch.full((R, 2), 9.0, dtype=torch.float32, device=DEV)
    masks = dict(suppress=mask_of(sup) if sup else None, begin_suppress=mask_of(bsup) if bsup else None, first=t == 0)
    rules = dict(ts_begin=TSB, no_timestamps_id=NOTS, max_initial=max_initial, ts_last=ts_last) if timestamps else {}
    hip.dec_beam_topk(x, V, 1, done=torch.zeros(R, dtype=torch.uint8, device=DEV), cand_token=ct, cand_logprob=cl, eos_id=EOS, t=t,
                      timestamps=timestamps, tokens=tokens if timestamps else None, **masks, **rules)
    step = hip.dec_timestamp_step if timestamps else hip.dec_greedy_step
    step(x, V, finished=torch.zeros(R, dtype=torch.uint8, device=DEV), n_unfinished=torch.zeros(1, dtype=torch.int32, device=DEV), tokens=tokens,
         logprobs=lps, t=t, eos_id=EOS, pad_id=PAD, **masks, **rules)
    torch.cuda.synchronize()
    return tokens[:, t].cpu(), lps[:, t].cpu(), ct[:, 0].cpu(), cl[:, 0].cpu()


def test_token_step_is_the_top1_of_the_beam(hip):
    """The greedy and the timestamp step against dec_beam_topk_kernel's first candidate at nb = 1, BIT FOR BIT (fp32 ``==``, no
    tolerance): the two share the scan, the reduction and the log-probability arithmetic.  Six rows per launch of the planted
    states above and of tests/test_gpu_whisper_timestamps.py, each on the vector path (128 columns) and on the scalar path (the
    129-column view of a 131-column buffer)."""
    g = base_rows(6, 51)  # greedy mode: suppressed / begin-suppressed maxima, an exact tie, eos, the last column
    top = float(g[:, :V].max())
    g[0, 50] = top + 5
    g[1, 60] = top + 3
    g[2, 17] = g[2, 90] = top + 1
    g[3, EOS] = top + 2
    g[5, V - 1] = top + 2
    x0 = base_rows(6, 41)  # rules, t = 0, max_initial 5, both masks, junk in ts_last
    x0[0, 17] = 12.0
    x0[0, TSB + 2] = 6.0
    x0[1, TSB + 9] = 12.0
    x0[1, TSB + 5] = 6.0
    x0[2, TSB + 1] = 12.0
    x0[2, TSB + 3] = 9.0
    x0[2, TSB + 0] = 6.0
    x0[3, NOTS] = 12.0
    x0[3, TSB + 4] = 6.0
    x0[4, TSB + 1] = 12.0
    x0[5, TSB + 4] = 6.0
    x0[5, EOS] = 12.0
    x1 = base_rows(6, 42)  # rules, t = 1, after [ts]: timestamps masked although they dominate; eos
    x1[0, TSB + 6:V] = 12.0
    x1[0, 33] = 6.0
    x1[1, EOS] = 9.0
    x2 = base_rows(6, 43)  # rules, t = 2, after [ts, text]: the mass rule won (row 0) and lost (row 1); <|notimestamps|>; an exact tie
    x2[0, 40] = 8.0
    x2[0, TSB:V] = 6.2
    x2[0, TSB + 7] = 7.0
    x2[0, TSB + 1] = 30.0
    x2[1, 40] = 12.0
    x2[2, NOTS] = 20.0
    x2[2, 41] = 9.0
    x2[3, TSB + 8] = x2[3, TSB + 12] = 9.0
    cases = [("greedy first", g, [[]] * 6, 0, dict(timestamps=False, sup=[50, 120], bsup=[60, 3]), {0: None, 2: 17, 3: EOS, 5: V - 1}),
             ("greedy not first", g, [[5, 6]] * 6, 2, dict(timestamps=False, sup=[50, 120], bsup=[60, 3]), {1: 60, 2: 17, 3: EOS}),
             ("rules t=0", x0, [[]] * 6, 0, dict(timestamps=True, sup=[TSB + 1, 50], bsup=[TSB + 3, 60], max_initial=5, ts_in=[120, 121, 122, 123, 77, 125]),
              {0: TSB + 2, 1: TSB + 5, 2: TSB, 3: TSB + 4, 5: TSB + 4}),
             ("rules t=1", x1, [[TSB + 2]] * 6, 1, dict(timestamps=True, ts_in=[TSB + 2] * 6), {0: 33, 1: EOS}),
             ("rules t=2", x2, [[TSB + 4, 7]] * 6, 2, dict(timestamps=True, ts_in=[TSB + 4] * 6), {0: TSB + 7, 1: 40, 2: 41, 3: TSB + 8})]
    for name, x, hists, t, kw, planted in cases:
        wide = torch.full((6, 131), 1e30)
        wide[:, :V] = x[:, :V]
        for path, xd in (("vector", x.to(DEV)), ("scalar", wide.to(DEV)[:, :129])):
            tok, lp, ct, cl = step_and_top1(hip, xd, hists, t, **kw)
            print(f"token step vs top-1, {name}, {path} path: tokens {tok.tolist()} / {ct.tolist()}, log-probs as int32 "
                  f"{lp.view(torch.int32).tolist()} / {cl.view(torch.int32).tolist()}")
            for r, want in planted.items():
                assert want is None or int(tok[r]) == want, (name, path, r, int(tok[r]), want)
            assert int(tok[0]) != 50 and bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())
            assert torch.equal(tok, ct), (name, path, "tokens")
            assert bool((lp == cl).all()), (name, path, "log-probs: fp32 ==, no tolerance")


# ------------------------------------------------------------------------------------------------------------ 2. select
@pytest.fixture(scope="module")
def tables():
    g = torch.Generator().manual_seed(31)
    return torch.randn(V, De, generator=g).to(torch.bfloat16), torch.randn(MAXP, De, generator=g).to(torch.bfloat16)


def run_select(hip, tables, name, nb, t, audios, ldt, next_pos=5, with_ts=True):
    """``audios``: per audio dict(hist [nb][t], lph [nb][t], sums [nb], ct [nb][K], cl [nb][K], fin = [(tokens, sum)], done, ts_last
    [nb]).  One launch; everything the kernel writes against whisper_beam_ref.update_array in np.float32."""
    Bn, Kn, R = len(audios), nb + 1, len(audios) * nb
    E, Pz = tables
    f32 = np.float32
    tokens = np.full((R, ldt), -5, np.int32)
    lps = np.full((R, ldt), 9.0, f32)
    sums, ct, cl = np.zeros((Bn, nb), f32), np.zeros((R, Kn), np.int32), np.zeros((R, Kn), f32)
    ts_last = np.zeros(R, np.int32)
    fin_tok, fin_lp = np.full((Bn, nb, ldt), -7, np.int32), np.full((Bn, nb, ldt), 5.0, f32)
    fin_len, fin_sum, n_fin, done = np.full((Bn, nb), -3, np.int32), np.full((Bn, nb), 4.0, f32), np.zeros(Bn, np.int32), np.zeros(Bn, np.uint8)
    for b, a in enumerate(audios):
        for j in range(nb):
            tokens[b * nb + j, :t], lps[b * nb + j, :t] = a["hist"][j], a["lph"][j]
        sums[b], ct[b * nb:(b + 1) * nb], cl[b * nb:(b + 1) * nb], ts_last[b * nb:(b + 1) * nb] = a["sums"], a["ct"], a["cl"], a["ts_last"]
        n_fin[b], done[b] = len(a["fin"]), a["done"]
        for k, (ft, fs) in enumerate(a["fin"]):
            fin_tok[b, k, :len(ft)], fin_len[b, k], fin_sum[b, k] = ft, len(ft), fs
    before = dict(tokens=tokens.copy(), lps=lps.copy(), fin_tok=fin_tok.copy(), fin_lp=fin_lp.copy(), fin_len=fin_len.copy(), fin_sum=fin_sum.copy())
    d = {k: torch.from_numpy(v).to(DEV) for k, v in dict(tokens=tokens, lps=lps, sums=sums, ct=ct, cl=cl, ts_last=ts_last, fin_tok=fin_tok, fin_lp=fin_lp,
                                                          fin_len=fin_len, fin_sum=fin_sum, n_fin=n_fin, done=done).items()}
    src = torch.full((R,), -9, dtype=torch.int32, device=DEV)
    n_unf = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    h_next = torch.full((R, De), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.dec_beam_select(d["ct"], d["cl"], nb, V, sum_logprob=d["sums"], src=src, tokens=d["tokens"], logprobs=d["lps"], t=t, fin_tokens=d["fin_tok"],
                        fin_logprobs=d["fin_lp"], fin_len=d["fin_len"], fin_sum=d["fin_sum"], n_fin=d["n_fin"], done=d["done"], n_unfinished=n_unf,
                        eos_id=EOS, pad_id=PAD, ts_last=d["ts_last"] if with_ts else None, ts_begin=TSB, embed_tokens=E.to(DEV),
                        embed_positions=Pz.to(DEV), next_pos=next_pos, h_next=h_next)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    src = src.cpu().numpy()
    want_tok_all, n_not_done = [], 0
    for b, a in enumerate(audios):
        fin = [(list(ft), f32(fs)) for ft, fs in a["fin"]]
        n0 = len(fin)
        cands = [[(int(c), f32(l)) for c, l in zip(a["ct"][j], a["cl"][j]) if c >= 0] for j in range(nb)]
        tok, sr, new, lpn, dn = BR.update_array([list(h) for h in a["hist"]], [f32(s) for s in a["sums"]], cands, nb, EOS, PAD, fin, bool(a["done"]))
        rows = slice(b * nb, (b + 1) * nb)
        assert src[rows].tolist() == [b * nb + s for s in sr], (name, b, src[rows].tolist(), sr)
        assert got["tokens"][rows, t].tolist() == tok, (name, b, got["tokens"][rows, t].tolist(), tok)
        assert np.array_equal(got["lps"][rows, t], np.array(lpn, f32)), (name, b)
        for i, s in enumerate(sr):  # the histories follow the sources, the columns behind t stay
            assert np.array_equal(got["tokens"][b * nb + i, :t], before["tokens"][b * nb + s, :t]), (name, b, i, "token history")
            assert np.array_equal(got["lps"][b * nb + i, :t], before["lps"][b * nb + s, :t]), (name, b, i, "log-prob history")
        assert (got["tokens"][rows, t + 1:] == -5).all() and (got["lps"][rows, t + 1:] == 9.0).all()
        assert np.array_equal(got["sums"][b], np.array(new, f32)), (name, b, got["sums"][b], new)
        if with_ts and not a["done"]:
            want_ts = [tk if tk >= TSB else a["ts_last"][s] for tk, s in zip(tok, sr)]
            assert got["ts_last"][rows].tolist() == want_ts, (name, b, got["ts_last"][rows].tolist(), want_ts)
        else:
            assert got["ts_last"][rows].tolist() == list(a["ts_last"])
        assert got["n_fin"][b] == len(fin) and got["done"][b] == int(dn), (name, b, got["n_fin"][b], len(fin), dn)
        for k in range(nb):
            if n0 <= k < len(fin):
                ft, fs = fin[k]
                j = next(s for s in range(nb) if list(a["hist"][s]) == ft[:-1] and any(c == EOS for c in a["ct"][s]))
                lp_eos = next(l for c, l in zip(a["ct"][j], a["cl"][j]) if c == EOS)
                assert got["fin_tok"][b, k, :t + 1].tolist() == ft and got["fin_len"][b, k] == t + 1 and got["fin_sum"][b, k] == fs
                assert np.array_equal(got["fin_lp"][b, k, :t], before["lps"][b * nb + j, :t]) and got["fin_lp"][b, k, t] == f32(lp_eos)
                assert (got["fin_tok"][b, k, t + 1:] == -7).all()
            else:
                for key in ("fin_tok", "fin_lp", "fin_len", "fin_sum"):
                    assert np.array_equal(got[key][b, k], before[key][b, k]), (name, b, k, key, "an untouched slot of the finished store")
        n_not_done += not dn
        want_tok_all += tok
    assert int(n_unf.item()) == n_not_done, (name, int(n_unf.item()), n_not_done)
    want_h = (E[torch.tensor(want_tok_all)].float() + Pz[next_pos].float()[None]).to(torch.bfloat16)
    assert torch.equal(h_next.cpu().view(torch.int16), want_h.view(torch.int16)), "h_next is defined bit for bit"
    print(f"beam select {name}: sources {src.tolist()}, tokens {got['tokens'][:, t].tolist()}, n_fin {got['n_fin'].tolist()}, done {got['done'].tolist()}, "
          f"n_unfinished {int(n_unf.item())}: all exact")
    return got, src


def planted_audio(rng, nb, t, sums, ct, cl, fin=(), done=0, ts_last=None):
    hist = [[int(x) for x in rng.integers(4, 90, t)] for _ in range(nb)]
    if ts_last is None:
        ts_last = [-1] * nb
    return dict(hist=hist, lph=(-rng.random((nb, t))).astype(np.float32), sums=sums, ct=ct, cl=cl, fin=list(fin), done=done, ts_last=ts_last)


def test_beam_select_planted(hip, tables):
    """nb = 3, K = 4, t = 5, one audio per case, one launch.  Log-probs are multiples of 2^-4, so the fp32 sums are exact and ties are
    exact."""
    rng = np.random.default_rng(71)
    INF, t = -np.inf, 5
    lo = [-20.0, -21.0, -22.0, -23.0]
    A = []
    # 0: no eos; three beams offer, the best three of twelve
    A.append(planted_audio(rng, NB, t, [-1.0, -2.0, -3.0], [[10, 11, 12, 13], [20, 21, 22, 23], [30, 31, 32, 33]],
                           [[-0.5, -1.5, -6.0, -7.0], [-0.25, -4.0, -6.0, -7.0], [-0.125, -5.0, -6.0, -7.0]], ts_last=[TSB + 1, TSB + 2, TSB + 3]))
    # 1: eos ranked first: stored, three live follow
    A.append(planted_audio(rng, NB, t, [-1.0, -2.0, -3.0], [[EOS, 11, 12, 13], [20, 21, 22, 23], [30, 31, 32, 33]],
                           [[-0.25, -1.5, -6.0, -7.0], [-0.25, -4.0, -6.0, -7.0], [-0.125, -5.0, -6.0, -7.0]]))
    # 2: eos behind the third live candidate: never seen
    A.append(planted_audio(rng, NB, t, [-1.0, -2.0, -3.0], [[10, 11, 12, EOS], [20, 21, 22, 23], [30, 31, 32, 33]],
                           [[-0.5, -0.75, -1.0, -1.25], [-4.0, -5.0, -6.0, -7.0], [-4.0, -5.0, -6.0, -7.0]]))
    # 3: two eos with n_fin = nb - 1: only the first is stored, the audio becomes done
    prev = [([5, 6, EOS], -1.5), ([7, EOS], -2.5)]
    A.append(planted_audio(rng, NB, t, [-1.0, -2.0, -3.0], [[EOS, 11, 12, 13], [EOS, 21, 22, 23], [30, 31, 32, 33]],
                           [[-0.25, -1.5, -6.0, -7.0], [-0.25, -4.0, -6.0, -7.0], [-0.125, -5.0, -6.0, -7.0]], fin=prev))
    # 4: an audio that was done: pad, identity, nothing else moves
    full = [([5, 6, EOS], -1.5), ([7, EOS], -2.5), ([8, 9, 10, EOS], -3.5)]
    A.append(planted_audio(rng, NB, t, [-1.0, -2.0, -3.0], [[10, 11, 12, 13]] * 3, [lo] * 3, fin=full, done=1, ts_last=[TSB, TSB + 1, TSB + 2]))
    # 5: -inf beams: only beam 0 offers (the first step of a call)
    A.append(planted_audio(rng, NB, t, [0.0, INF, INF], [[10, 11, 12, 13]] * 3, [[-0.5, -1.0, -1.5, -2.0]] * 3))
    # 6: -inf beams and missing candidates: the candidates run out, the third slot gets pad / -inf / itself
    A.append(planted_audio(rng, NB, t, [INF, -1.0, INF], [[10, 11, 12, 13], [20, 21, -1, -1], [30, 31, 32, 33]],
                           [[-0.5, -1.0, -1.5, -2.0], [-0.5, -1.0, INF, INF], [-0.5, -1.0, -1.5, -2.0]], ts_last=[TSB + 1, TSB + 2, TSB + 3]))
    # 7: score ties decided by (beam, rank): -1 + -1.5 = -2 + -0.5 = -1.5 + -1 (beams 0, 1, 2), and within beam 0 two equal log-probs
    A.append(planted_audio(rng, NB, t, [-1.0, -2.0, -1.5], [[10, 11, 12, 13], [20, 21, 22, 23], [30, 31, 32, 33]],
                           [[-1.5, -1.5, -6.0, -7.0], [-0.5, -4.0, -6.0, -7.0], [-1.0, -5.0, -6.0, -7.0]]))
    # 8: sources [1, 1, 0]: a source repeated and overwritten while still needed
    A.append(planted_audio(rng, NB, t, [-2.0, -0.5, -9.0], [[10, 11, 12, 13], [20, 21, 22, 23], [30, 31, 32, 33]],
                           [[-0.125, -20.0, -21.0, -22.0], [-0.125, -0.25, -20.0, -21.0], lo], ts_last=[TSB + 1, TSB + 2, TSB + 3]))
    # 9: a full cycle [1, 2, 0]; the new tokens of slots 0 and 2 are timestamps (ts_last set), slot 1 carries its source's
    A.append(planted_audio(rng, NB, t, [-3.0, -1.0, -2.0], [[TSB + 9, 11, 12, 13], [TSB + 8, 21, 22, 23], [30, 31, 32, 33]],
                           [[-0.125, -30.0, -31.0, -32.0], [-0.125, -30.0, -31.0, -32.0], [-0.125, -30.0, -31.0, -32.0]], ts_last=[TSB + 1, TSB + 2, TSB + 3]))
    got, src = run_select(hip, tables, "planted", NB, t, A, ldt=8)
    s = lambda b: [int(x) - b * NB for x in src[b * NB:(b + 1) * NB]]
    tk = lambda b: got["tokens"][b * NB:(b + 1) * NB, t].tolist()
    assert s(0) == [0, 1, 0] and tk(0) == [10, 20, 11]
    assert got["n_fin"][1] == 1 and tk(1) == [20, 11, 30] and got["n_fin"][2] == 0 and tk(2) == [10, 11, 12]
    assert got["n_fin"][3] == 3 and got["done"][3] == 1 and got["fin_sum"][3, 2] == np.float32(-1.25)
    assert tk(4) == [PAD] * 3 and s(4) == [0, 1, 2] and tk(5) == [10, 11, 12] and s(5) == [0, 0, 0]
    assert tk(6) == [20, 21, PAD] and s(6) == [1, 1, 2] and np.isinf(got["sums"][6, 2])
    assert tk(7) == [10, 11, 20] and s(7) == [0, 0, 1], "ties: beam 0 rank 0, beam 0 rank 1, beam 1"
    assert s(8) == [1, 1, 0] and s(9) == [1, 2, 0]
    assert got["ts_last"][27:30].tolist() == [TSB + 8, TSB + 3, TSB + 9] and got["ts_last"][24:27].tolist() == [TSB + 2, TSB + 2, TSB + 1]
    # the same launch without timestamps: ts_last is not touched
    run_select(hip, tables, "planted, no ts_last", NB, t, A, ldt=8, with_ts=False)
    # an audio staying done across two further launches is the done case above; an audio BECOMING done and then frozen:
    nxt = dict(A[3], fin=[(got["fin_tok"][3, k, :got["fin_len"][3, k]].tolist(), float(got["fin_sum"][3, k])) for k in range(3)], done=1,
               hist=[r[:t + 1].tolist() for r in got["tokens"][9:12]], lph=got["lps"][9:12, :t + 1], sums=got["sums"][3].tolist())
    g2, s2 = run_select(hip, tables, "became done, next step", NB, t + 1, [nxt], ldt=8)
    assert g2["tokens"][:, t + 1].tolist() == [PAD] * 3 and s2.tolist() == [0, 1, 2]


def test_beam_select_wide(hip, tables):
    """nb = 8, t = 223 (the histories of 8 x 223 x 8 bytes in LDS), random candidates with eos among them, -inf beams, quantised
    log-probs (ties); three audios."""
    rng = np.random.default_rng(72)
    nb, t, Kn = 8, 223, 9
    A = []
    for a in range(3):
        ct = np.stack([rng.choice(np.r_[4:90, EOS, EOS + 20], Kn, replace=False) for _ in range(nb)]).astype(np.int32)
        cl = -np.sort(rng.integers(1, 40, (nb, Kn)) / 8.0, axis=1)
        sums = (-rng.integers(0, 40, nb) / 4.0).astype(np.float32)
        sums[rng.integers(0, nb)] = -np.inf
        fin = [([int(x) for x in rng.integers(4, 90, 3 + k)] + [EOS], -3.0 - k) for k in range(5 + a)]
        A.append(planted_audio(rng, nb, t, sums.tolist(), ct.tolist(), cl.tolist(), fin=fin, ts_last=[TSB + j for j in range(nb)]))
    got, _ = run_select(hip, tables, "nb=8 t=223", nb, t, A, ldt=230)
    assert got["n_fin"].max() > 5


# ------------------------------------------------------------------------------------------------------------ 3. cache reorder
@pytest.mark.parametrize("nb", [1, 5, 8])
def test_kv_reorder(hip, nb):
    """2 layers, B = 3, D = 128 (rows of 256 elements), keys [2, 9) of a 12-key cache laid out with gaps as run_step of
    tests/test_gpu_whisper_generate.py builds its buffer: keys 2 D + 24 apart, rows cap * ld + 8 apart, layers a further 16.  The
    16-bit patterns count up through the buffer, so any two positions within an audio's rows of a layer differ (they are less than
    65 536 elements apart).  Audio 0 keeps identity, audio 1 repeats sources, audio 2 is a cycle; then all identity."""
    layers, Bn, cap, W = 2, 3, 12, 256
    R = Bn * nb
    ld = W + 24
    rs = cap * ld + 8
    ls = R * rs + 16
    assert (nb - 1) * rs + rs < 65536
    flat = (torch.arange(layers * ls + 8, dtype=torch.int32) % 65536).to(torch.int16).to(DEV)
    before = flat.clone()
    cache = torch.as_strided(flat.view(torch.bfloat16), (layers, R, cap, W), (ls, rs, ld, 1), 8)
    src = list(range(R))
    if nb > 1:
        src[nb:2 * nb] = [nb + (nb - 1 if i % 2 else 1) for i in range(nb)]          # repeats (beam 0 -> 1: overwritten while needed)
        src[2 * nb:3 * nb] = [2 * nb + (i + 1) % nb for i in range(nb)]              # the full cycle
    for name, s in (("identity / repeats / cycle", src), ("identity", list(range(R)))):
        flat.copy_(before)
        hip.dec_kv_reorder(cache, torch.tensor(s, dtype=torch.int32, device=DEV), nb, 2, 9)
        torch.cuda.synchronize()
        want = before.clone()
        wc = torch.as_strided(want, (layers, R, cap, W), (ls, rs, ld, 1), 8)
        bc = torch.as_strided(before, (layers, R, cap, W), (ls, rs, ld, 1), 8)
        for r in range(R):
            wc[:, r, 2:9] = bc[:, s[r], 2:9]
        moved = int((want != before).sum())
        differ = int((flat != want).sum())
        print(f"kv reorder nb={nb} {name}: {moved} elements move, {differ} of {flat.numel()} differ from the gather (gaps and other keys included)")
        assert differ == 0
        assert moved > 0 or s == list(range(R))


# ------------------------------------------------------------------------------------------------------------ 4. grouped attention
NH, D = 2, 128


def dev_bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("n_split", [1, 5])
@pytest.mark.parametrize("n_keys", [33, 131])
def test_grouped_attention_step(hip, n_keys, n_split):
    """group = 3 on a cross buffer of 2 utterances against ssak_dec_attention_step on the buffer replicated per row; group = 1 against
    the same entry; with and without klens.  The buffers are strided views with NaN in the gaps and past klens."""
    rng = np.random.default_rng(100 * n_keys + n_split)
    Bu, g = 2, 3
    R = Bu * g
    q = dev_bf16(rng.standard_normal((R, D)) * 0.8)
    k = rng.standard_normal((Bu, n_keys, D)) * 0.8
    v = rng.standard_normal((Bu, n_keys, D))
    cap, ld = n_keys + 5, 2 * D + 24

    def build(kk, vv, klens):
        n = kk.shape[0]
        bs = cap * ld + 8
        buf = torch.full((n * bs,), float("nan"), dtype=torch.bfloat16, device=DEV)
        kd = torch.as_strided(buf, (n, cap, D), (bs, ld, 1), 8)
        vd = torch.as_strided(buf, (n, cap, D), (bs, ld, 1), D + 24)
        for b in range(n):
            m = n_keys if klens is None else klens[b]
            kd[b, :m].copy_(dev_bf16(kk[b, :m]))
            vd[b, :m].copy_(dev_bf16(vv[b, :m]))
        return kd, vd

    for klens in ((n_keys, n_keys // 2 + 1), None):
        kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device=DEV)
        kd, vd = build(k, v, klens)
        got = hip.dec_attention_step_grouped(q, kd, vd, n_keys, NH, g, klens=kl, n_split=n_split)
        rep_kl = None if klens is None else [klens[r // g] for r in range(R)]
        kr, vr = build(np.repeat(k, g, 0), np.repeat(v, g, 0), rep_kl)
        want = hip.dec_attention_step(q, kr, vr, n_keys, NH, klens=None if klens is None else torch.tensor(rep_kl, dtype=torch.int32, device=DEV),
                                      n_split=n_split)
        one = hip.dec_attention_step_grouped(q, kr, vr, n_keys, NH, 1, klens=None if klens is None else torch.tensor(rep_kl, dtype=torch.int32,
                                                                                                                     device=DEV), n_split=n_split)
        torch.cuda.synchronize()
        d1 = int((got.view(torch.int16) != want.view(torch.int16)).sum())
        d2 = int((one.view(torch.int16) != want.view(torch.int16)).sum())
        print(f"grouped attention n_keys={n_keys} n_split={n_split} klens={klens}: group=3 {d1} / group=1 {d2} of {got.numel()} elements differ")
        assert d1 == 0 and d2 == 0 and bool(torch.isfinite(got.float()).all())


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_launch_nothing(hip, tables):
    E, Pz = tables
    R = 2 * NB
    x = base_rows(R, 48).to(DEV)
    i32 = lambda *s, fill=-5: torch.full(s, fill, dtype=torch.int32, device=DEV)
    f32 = lambda *s, fill=9.0: torch.full(s, fill, dtype=torch.float32, device=DEV)
    done = torch.zeros(2, dtype=torch.uint8, device=DEV)
    ct, cl = i32(R, K, fill=77), f32(R, K)
    with pytest.raises(ValueError, match="nb=9"):
        hip.dec_beam_topk(base_rows(18, 1).to(DEV), V, 9, done=done, cand_token=i32(18, 10, fill=77), cand_logprob=f32(18, 10), eos_id=EOS)
    with pytest.raises(ValueError, match="nb=0"):
        hip.check(hip.lib.ssak_dec_beam_topk(hip.ptr(x), LDV, 2, 0, V, None, None, 0, 0, 0, 0, -1, EOS, None, 0, 0, None, hip.ptr(done), 1, hip.ptr(ct),
                                             hip.ptr(cl), hip.stream()))
    with pytest.raises(ValueError, match="K="):  # buffers of nb + 2 columns
        hip.dec_beam_topk(x, V, NB, done=done, cand_token=i32(R, K + 1, fill=77), cand_logprob=f32(R, K + 1), eos_id=EOS)
    assert hip.lib.ssak_dec_beam_topk(hip.ptr(x), LDV, 2, NB, V, None, None, 0, 0, 0, 0, -1, EOS, None, 0, 0, None, None, K, hip.ptr(ct), hip.ptr(cl),
                                      hip.stream()) == hip.SSAK_ERR_INVALID, "a NULL done"
    with pytest.raises(ValueError, match="tokens and ts_last"):
        hip.dec_beam_topk(x, V, NB, done=done, cand_token=ct, cand_logprob=cl, eos_id=EOS, timestamps=True, ts_begin=TSB, no_timestamps_id=NOTS)
    torch.cuda.synchronize()
    assert bool((ct == 77).all()) and bool((cl == 9.0).all()), "a refused top-K launched"
    # select
    tokens, lps, sums, src = i32(R, 8), f32(R, 8), f32(2, NB, fill=0.0), i32(R, fill=-9)
    n_unf, h_next = i32(1, fill=77), torch.full((R, De), 7.0, dtype=torch.bfloat16, device=DEV)
    kw = dict(sum_logprob=sums, src=src, tokens=tokens, logprobs=lps, fin_tokens=i32(2, NB, 8), fin_logprobs=f32(2, NB, 8), fin_len=i32(2, NB),
              fin_sum=f32(2, NB), n_fin=i32(2, fill=0), done=done, n_unfinished=n_unf, eos_id=EOS, pad_id=PAD, embed_tokens=E.to(DEV),
              embed_positions=Pz.to(DEV), h_next=h_next)
    with pytest.raises(ValueError, match="K="):
        hip.dec_beam_select(i32(R, K + 1), f32(R, K + 1), NB, V, t=0, **kw)
    with pytest.raises(ValueError, match="step t"):
        hip.dec_beam_select(ct, cl, NB, V, t=8, **kw)
    with pytest.raises(ValueError, match="overruns"):
        hip.dec_beam_select(ct, cl, NB, V, t=0, next_pos=MAXP, **kw)
    with pytest.raises(ValueError, match="nb=9"):
        big = dict(kw, sum_logprob=f32(1, 9), src=i32(9), tokens=i32(9, 8), logprobs=f32(9, 8), fin_tokens=i32(1, 9, 8), fin_logprobs=f32(1, 9, 8),
                   fin_len=i32(1, 9), fin_sum=f32(1, 9), n_fin=i32(1), done=done[:1], h_next=None)
        hip.dec_beam_select(i32(9, 10), f32(9, 10), 9, V, t=0, **big)
    with pytest.raises(ValueError, match="ts_begin"):
        hip.dec_beam_select(ct, cl, NB, V, t=0, ts_last=i32(R), ts_begin=EOS, **kw)
    with pytest.raises(ValueError, match="nb=0"):
        hip.check(hip.lib.ssak_dec_beam_select(hip.ptr(ct), hip.ptr(cl), 2, 0, 1, V, hip.ptr(sums), hip.ptr(src), hip.ptr(tokens), hip.ptr(lps), 8, 0, None,
                                               0, hip.ptr(kw["fin_tokens"]), hip.ptr(kw["fin_logprobs"]), hip.ptr(kw["fin_len"]), hip.ptr(kw["fin_sum"]),
                                               hip.ptr(kw["n_fin"]), hip.ptr(done), hip.ptr(n_unf), None, None, 0, 0, 0, EOS, PAD, None, hip.stream()))
    torch.cuda.synchronize()
    assert bool((tokens == -5).all()) and int(n_unf.item()) == 77 and bool((h_next == 7.0).all()) and bool((src == -9).all()), "a refused select launched"
    # reorder
    cache = torch.full((2, R, 12, 256), 3.0, dtype=torch.bfloat16, device=DEV)
    perm = torch.tensor([1, 2, 0, 4, 5, 3], dtype=torch.int32, device=DEV)
    for lo, hi in ((2, 13), (-1, 4), (5, 4)):
        with pytest.raises(ValueError, match="outside the cache"):
            hip.dec_kv_reorder(cache, perm, NB, lo, hi)
    with pytest.raises(ValueError, match="nb=9"):
        hip.dec_kv_reorder(torch.zeros((1, 9, 4, 64), dtype=torch.bfloat16, device=DEV), torch.arange(9, dtype=torch.int32, device=DEV), 9, 0, 4)
    with pytest.raises(ValueError, match="nb=0"):
        hip.check(hip.lib.ssak_dec_kv_reorder(hip.ptr(cache), hip.ptr(perm), 2, 2, 0, 12, 256, cache.stride(0), cache.stride(1), cache.stride(2), 0, 4,
                                              hip.stream()))
    assert hip.lib.ssak_dec_kv_reorder(hip.ptr(cache), None, 2, 2, NB, 12, 256, cache.stride(0), cache.stride(1), cache.stride(2), 0, 4,
                                       hip.stream()) == hip.SSAK_ERR_INVALID, "a NULL src"
    # grouped attention: a group that does not divide the rows
    q = torch.zeros((R, D), dtype=torch.bfloat16, device=DEV)
    kv = torch.zeros((2, 8, 2 * D), dtype=torch.bfloat16, device=DEV)
    ctx = torch.full((R, D), 7.0, dtype=torch.bfloat16, device=DEV)
    for g in (4, 0):
        with pytest.raises(ValueError, match="group"):
            hip.dec_attention_step_grouped(q, kv[:, :, :D], kv[:, :, D:], 4, NH, g, ctx=ctx)
    torch.cuda.synchronize()
    assert bool((ctx == 7.0).all()) and bool((cache == 3.0).all()), "a refused call launched"


# ------------------------------------------------------------------------------------------------------------ 6. the loop by hand
B = 3
N_NEW = 8
KEEP = sorted(np.random.default_rng(7).choice(100, size=10, replace=False).tolist())  # the open text ids (the timestamp test's draw)
SUPPRESS = list(range(G.SOT, NOTS + 1)) + [t for t in range(EOS) if t not in KEEP]     # every special but eos, 90 of the 100 text ids
OPEN = [c for c in range(G.V) if c not in SUPPRESS and c < TSB]                         # without timestamps: 10 text ids and eos
SUPPRESS_NO_TS = SUPPRESS + list(range(TSB, G.V))


@pytest.fixture(scope="module")
def model(golden):
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    gen = json.loads(str(golden["generation_config_json"]))
    cfg = WhisperSeq2SeqConfig.from_hf_dict(json.loads(str(golden["config_json"])),
                                            lang_to_id={str(c): int(i) for c, i in zip(golden["lang_codes"], golden["lang_ids"])},
                                            task_to_id=gen["task_to_id"], no_timestamps_token_id=gen["no_timestamps_token_id"],
                                            max_initial_timestamp_index=5)
    m = WhisperSeq2Seq(cfg)
    m.load_decoder_state_dict({k[2:]: torch.from_numpy(WR.bf16_from_bits(golden[k]).astype(np.float32)) for k in golden.files if k.startswith("w/")})
    return m


@pytest.fixture(scope="module")
def enc(golden):
    return torch.from_numpy(WR.bf16_from_bits(golden["enc"]).astype(np.float32)).to(torch.bfloat16)


def greedy_bar(x64, mask, token, lp):
    xs = x64[mask]
    m = xs.max()
    s = np.exp(xs - m).sum()
    rel = (4 * np.abs(xs - m).max() + math.ceil(x64.shape[0] / 256) + 10 + 6) * U
    return rel + 2 * U * (abs(np.log(s)) + abs(m) + abs(m + np.log(s))) + 2 * U * (abs(x64[token]) + abs(lp))


@pytest.fixture(scope="module")
def hand_loop(model, enc, golden, hip):
    """The beam loop written out with the stepping primitives, language "en", without timestamps, N_NEW tokens at most; at every
    step the float64 array-form update on the device's own logits and state."""
    enc_lens = golden["enc_lens"]
    prompt = model.default_prompt(B, "en")
    P = prompt.shape[1]
    st = model._gen_begin(enc.to(DEV), enc_lens, cap=P + N_NEW, group=NB)
    logits = model._gen_prefill(st, prompt).repeat_interleave(NB, dim=0)
    bs = model._beam_begin(st, P, N_NEW, EOS, EOS, model._token_mask(SUPPRESS_NO_TS, "s"), None, None)
    mask = np.ones(G.V, dtype=bool)
    mask[SUPPRESS_NO_TS] = False
    fins = [[] for _ in range(B)]
    exempt, worst, steps = 0, 0.0, 0
    for i in range(N_NEW):
        x64 = logits[:, :G.V].double().cpu().numpy()
        tok0 = bs.tokens.cpu().numpy()
        sums0, done0 = bs.sums.double().cpu().numpy(), bs.done.cpu().numpy()
        model._beam_step(st, bs, logits, last=i + 1 == N_NEW)
        torch.cuda.synchronize()
        tok1, src1, sums1 = bs.tokens.cpu().numpy(), bs.src.cpu().numpy(), bs.sums.double().cpu().numpy()
        step_margin, step_bar = np.inf, 0.0
        for b in range(B):
            margin_b, bar_b = np.inf, 1e-300
            rows = range(b * NB, (b + 1) * NB)
            hist = [tok0[r, :i].tolist() for r in rows]
            lps = [BR.log_softmax(np.where(mask, x64[r], -np.inf)) for r in rows]
            cands = [BR.topk_stable(lps[j], K) if (not done0[b] and sums0[b, j] > -np.inf) else [] for j in range(NB)]
            fin_before = len(fins[b])
            tok, src, new, _, dn = BR.update_array(hist, list(sums0[b]), cands, NB, EOS, EOS, fins[b], bool(done0[b]))
            # the margins that decide this audio's step: neighbours in the walk, neighbours in each offering row's first K + 1 columns
            if not done0[b]:
                walk = sorted(sums0[b, j] + lp for j in range(NB) for _, lp in cands[j])
                walk = walk[::-1][:NB + (len(fins[b]) - fin_before) + 1]
                gaps = [a - c for a, c in zip(walk, walk[1:])]
                for j in range(NB):
                    if cands[j]:
                        top = sorted(lps[j][mask])[::-1][:K + 1]
                        gaps += [a - c for a, c in zip(top, top[1:])]
                        bar_b = max([bar_b] + [greedy_bar(x64[b * NB + j], mask, c, lp) + U * abs(sums0[b, j] + lp) for c, lp in cands[j]])
                margin_b = min([margin_b] + gaps)
                step_margin, step_bar = min(step_margin, margin_b), max(step_bar, bar_b)
            ok = (tok1[b * NB:(b + 1) * NB, i].tolist() == tok and src1[b * NB:(b + 1) * NB].tolist() == [b * NB + s for s in src]
                  and int(bs.n_fin[b]) == len(fins[b]) and bool(bs.done[b]) == dn)
            if ok:
                for k, (ft, fs) in enumerate(fins[b]):
                    ok = ok and bs.fin_tokens[b, k, :int(bs.fin_len[b, k])].tolist() == ft
                for s_dev, s_ref in zip(sums1[b], new):
                    if np.isfinite(s_ref):
                        worst = max(worst, abs(s_dev - s_ref) / bar_b)
                        ok = ok and abs(s_dev - s_ref) <= bar_b
                    else:
                        ok = ok and s_dev == s_ref
            if not ok:
                assert margin_b < 4 * bar_b, (i, b, tok, tok1[b * NB:(b + 1) * NB, i].tolist(), src, margin_b, bar_b)
                exempt += 1
                fins[b] = [(bs.fin_tokens[b, k, :int(bs.fin_len[b, k])].tolist(), float(bs.fin_sum[b, k])) for k in range(int(bs.n_fin[b]))]
        print(f"hand loop step {i}: tokens {tok1[:, i].tolist()} sources {src1.tolist()} n_fin {bs.n_fin.tolist()} smallest deciding margin "
              f"{step_margin:.3e} (4 x bar {4 * step_bar:.3e})")
        steps = i + 1
        if i + 1 == N_NEW:
            break
        logits = model._gen_step(st, bs.h_next)
    print(f"hand loop: {exempt} exempt steps of {steps}, worst |sum - float64| / bar {worst:.3f}")
    assert exempt <= 1
    return dict(tokens=bs.tokens.cpu().numpy(), logprobs=bs.logprobs.cpu().numpy(), sums=bs.sums.cpu().numpy(), fin_tokens=bs.fin_tokens.cpu().numpy(),
                fin_len=bs.fin_len.cpu().numpy(), fin_sum=bs.fin_sum.cpu().numpy(), n_fin=bs.n_fin.cpu().numpy(), steps=steps)


def test_loop_by_hand_against_float64(hand_loop):
    assert hand_loop["steps"] == N_NEW and (hand_loop["n_fin"] <= NB).all()


@pytest.mark.parametrize("poll_every", [0, 1, 8])
def test_generate_equals_the_hand_loop(model, enc, golden, hand_loop, poll_every):
    from ssak_amd.whisper_seq2seq import beam_finalize, beam_rank
    r = model.generate(enc, language="en", max_new_tokens=N_NEW, enc_lens=golden["enc_lens"], suppress_tokens=SUPPRESS_NO_TS, beam_size=NB,
                       poll_every=poll_every)
    h = hand_loop
    for b in range(B):
        cands = beam_finalize(h["tokens"].reshape(B, NB, -1)[b], h["sums"][b], h["fin_tokens"][b], h["fin_len"][b], h["fin_sum"][b], h["n_fin"][b],
                              h["steps"], NB)
        assert r.beams[b] == [(c[0], c[1]) for c in cands], (b, r.beams[b], cands)
        w = beam_rank(cands)
        assert r.tokens[b] == cands[w][0] and r.sum_logprob[b] == cands[w][1]
        want = BR.finalize(h["tokens"].reshape(B, NB, -1)[b, :, :h["steps"]].tolist(), list(h["sums"][b].astype(np.float64)),
                           [(h["fin_tokens"][b, k, :h["fin_len"][b, k]].tolist(), float(h["fin_sum"][b, k])) for k in range(h["n_fin"][b])], NB)
        assert [c[:3] for c in cands] == want and w == BR.rank(want), "the host half against the restatement"
    assert np.array_equal(r.avg_logprob, r.sum_logprob / (r.lens + 1)) and r.no_speech_prob is None


# ------------------------------------------------------------------------------------------------------------ 7. generate
@pytest.mark.parametrize("timestamps", [False, True])
def test_beam_one_is_greedy(model, enc, golden, timestamps):
    kw = dict(enc_lens=golden["enc_lens"], suppress_tokens=SUPPRESS if timestamps else SUPPRESS_NO_TS, timestamps=timestamps)
    if not timestamps:
        kw["max_new_tokens"] = 12
    a = model.generate(enc, **kw)
    b = model.generate(enc, beam_size=1, **kw)
    bound = a.logprobs.shape[1] * U * np.abs(a.logprobs).sum(-1)
    diff = np.abs(a.sum_logprob - b.sum_logprob)
    print(f"beam_size=1 timestamps={timestamps}: tokens {b.tokens}; |sum difference| {diff.tolist()} (bars {bound.tolist()})")
    assert a.tokens == b.tokens and np.array_equal(a.lens, b.lens)
    assert (diff <= bound).all() and np.array_equal(a.logprobs, b.logprobs[:, :a.logprobs.shape[1]])
    if timestamps:
        assert np.array_equal(a.no_speech_prob, b.no_speech_prob)


STARVED_OPEN = [c for c in OPEN if c != EOS][:2]                       # the two columns a starved first step may choose
STARVE_BEGIN = [c for c in OPEN if c not in STARVED_OPEN]              # begin_suppress_tokens that leave those two


@pytest.mark.parametrize("starve", [None, "begin_suppress", "max_initial"])
def test_candidates_against_teacher_forcing(model, enc, golden, starve):
    """Every returned candidate of generate(beam_size=3): its per-token log-probs against the processed log-softmax of the project's
    own teacher-forced decode_logits on prompt + candidate (a cache row gathered from the wrong beam, or a beam without the
    prompt's cache rows, fails here), its sum against their fp32 running sum.  ``starve``: the first step offers only TWO columns
    -- a begin-suppress list that leaves two, or timestamps with max_initial_timestamp_index = 1 -- so the third slot holds no
    hypothesis after step 0 and is filled from a live beam at step 1.  With timestamps a position whose float64 mass decision on
    the teacher-forced row has a margin below 2 x 7.76e-2 is exempt (the two paths may mask differently there)."""
    enc_lens = golden["enc_lens"]
    ts = starve == "max_initial"
    sup = SUPPRESS if ts else SUPPRESS_NO_TS
    bsup = STARVE_BEGIN if starve == "begin_suppress" else None
    kw = dict(language="en", enc_lens=enc_lens, suppress_tokens=sup, beam_size=NB, begin_suppress_tokens=bsup)
    if not ts:
        kw["max_new_tokens"] = N_NEW
    was = model.config.max_initial_timestamp_index
    try:
        if ts:
            model.config.max_initial_timestamp_index = 1
        r = model.generate(enc, timestamps=ts, **kw)
        prompt = model.default_prompt(B, "en", timestamps=ts)
        P = prompt.shape[1]
        if starve:  # the situation is the one meant: after the first step the third slot of every audio is empty
            st = model._gen_begin(enc.to(DEV), enc_lens, cap=P + 2, group=NB)
            logits = model._gen_prefill(st, prompt).repeat_interleave(NB, dim=0)
            assert torch.equal(st.self_kv[:, 1::NB, :P], st.self_kv[:, ::NB, :P]) and torch.equal(st.self_kv[:, 2::NB, :P], st.self_kv[:, ::NB, :P])
            assert bool((st.self_kv[:, ::NB, :P] != 0).any()), "every beam holds the prompt's cache rows"
            bs = model._beam_begin(st, P, 2, EOS, EOS, model._token_mask(sup, "s"), model._token_mask(bsup, "b"),
                                   dict(ts_begin=TSB, no_timestamps_id=NOTS, max_initial=1) if ts else None)
            model._beam_step(st, bs, logits)
            s0 = bs.sums.cpu().numpy()
            assert np.isfinite(s0[:, :2]).all() and np.isinf(s0[:, 2]).all(), s0
    finally:
        model.config.max_initial_timestamp_index = was
    assert all(len(c) == NB for c in r.beams), "the empty slot was filled again"
    worst, exempt, n_pos = 0.0, 0, 0
    for k in range(NB):
        n = max(len(r.beams[b][k][0]) for b in range(B))
        full = np.full((B, P + n), EOS, dtype=np.int64)
        full[:, :P] = prompt
        for b in range(B):
            full[b, P:P + len(r.beams[b][k][0])] = r.beams[b][k][0]
        logits = model.decode_logits(enc, full, enc_lens).double().cpu().numpy()
        for b in range(B):
            toks, s = r.beams[b][k]
            lps = r.beam_logprobs[b][k]
            assert len(lps) == len(toks) and not np.isin(toks, sup).any()
            if starve == "begin_suppress":
                assert toks[0] in STARVED_OPEN
            run = np.float32(0.0)
            for i, tkn in enumerate(toks):
                x = logits[b, P - 1 + i]
                n_pos += 1
                if ts:
                    row = TR.timestamp_step_row(x, list(toks[:i]), TSB, NOTS, EOS, 1, sup)
                    lsm = BR.log_softmax(np.where(row["mask"], x, -np.inf))
                    if row["margin"] < 2 * LP_BAR:
                        exempt += 1
                    else:
                        worst = max(worst, abs(lps[i] - lsm[tkn]))
                else:
                    lsm = GR.log_softmax(GR.process(x[None], sup, bsup, i == 0))[0]
                    worst = max(worst, abs(lps[i] - lsm[tkn]))
                run = np.float32(run + np.float32(lps[i]))
            assert float(run) == s, (b, k, float(run), s, "the sum is the fp32 running sum of the per-token log-probs")
    print(f"candidates vs teacher forcing, starve={starve}: beams {r.beams}; worst |log-prob difference| {worst:.3e} (bar {2 * LP_BAR:.3e}), "
          f"{exempt} of {n_pos} positions exempt")
    assert worst <= 2 * LP_BAR and exempt <= 0.10 * n_pos


def test_no_allowed_first_column(model, enc, golden):
    """Every first-step column suppressed (the caller's error; greedy generate emits pad): one empty candidate per utterance."""
    r = model.generate(enc, language="en", max_new_tokens=3, enc_lens=golden["enc_lens"], suppress_tokens=SUPPRESS_NO_TS, begin_suppress_tokens=OPEN,
                       beam_size=NB, poll_every=0)
    assert r.tokens == [[]] * B and r.beams == [[([], 0.0)]] * B and r.lens.tolist() == [0] * B and r.token_array.shape == (B, 0)


def test_alone_and_permuted(model, enc, golden):
    enc_lens = np.asarray(golden["enc_lens"])
    kw = dict(language="en", max_new_tokens=N_NEW, suppress_tokens=SUPPRESS_NO_TS, beam_size=NB)
    r = model.generate(enc, enc_lens=enc_lens, **kw)
    perm = [2, 0, 1]
    p = model.generate(enc[perm], enc_lens=enc_lens[perm], **kw)
    for i, b in enumerate(perm):
        assert p.beams[i] == r.beams[b] and p.tokens[i] == r.tokens[b], ("permuted", b)
    for b in range(B):
        one = model.generate(enc[b:b + 1], enc_lens=enc_lens[b:b + 1], **kw)
        assert one.beams[0] == r.beams[b] and one.tokens[0] == r.tokens[b], ("alone", b, one.beams[0], r.beams[b])


@pytest.mark.parametrize("length_penalty", [None, 1.0])
def test_generate_timestamps_grammar(model, enc, golden, length_penalty):
    r = model.generate(enc, enc_lens=golden["enc_lens"], suppress_tokens=SUPPRESS, timestamps=True, beam_size=NB, length_penalty=length_penalty)
    print(f"generate(timestamps=True, beam_size=3, length_penalty={length_penalty}): tokens {r.tokens}, beams {r.beams}")
    assert r.no_speech_prob is not None and r.no_speech_prob.shape == (B,)
    for b in range(B):
        for toks, _ in r.beams[b]:
            TR.check_grammar(toks, TSB, EOS, NOTS, 5)
            assert not np.isin(toks, SUPPRESS).any() and len(toks) <= 16
        cands = [(t, s, bool(t) and t[-1] == EOS) for t, s in r.beams[b]]
        assert r.tokens[b] == cands[BR.rank(cands, length_penalty)][0]


def test_generate_refusals(model, enc):
    for bad in (0, 9):
        with pytest.raises(ValueError, match="beam_size"):
            model.generate(enc, language="en", max_new_tokens=2, beam_size=bad)
    with pytest.raises(ValueError, match="65535"):
        model.generate(torch.zeros((8192, 1, G.D), dtype=torch.bfloat16), language="en", max_new_tokens=2, beam_size=8)
    with pytest.raises(ValueError, match="length_penalty"):
        model.generate(enc, language="en", max_new_tokens=2, length_penalty=1.0)


# ------------------------------------------------------------------------------------------------------------ 8. transcribe, command line
from test_gpu_whisper_timestamps import SUPPRESS_T, VT, _Stored, long_generation_config, long_model, long_weights, noise  # noqa: E402,F401


def test_transcribe_with_a_beam(long_model, noise):
    """transcribe(beam_size=2) on the timestamp test's seeded model: a 5 s and a 31 s file (two windows).  Segments and seeks are
    re-derived from the returned tokens; beam_size = 1 is the default call."""
    from ssak_amd.whisper_transcribe import segments_from_window
    m, files = long_model, [noise[0], noise[1]]
    res = m.transcribe(files, beam_size=2, _max_rounds=64)
    ts_begin = NOTS + 1
    for r, s in zip(res, (5, 31)):
        assert r.content_frames == s * 100 and r.seeks[0] == 0 and r.seeks[-1] == r.content_frames and len(r.windows) == len(r.seeks) - 1
        segs = []
        for w, nxt in zip(r.windows, r.seeks[1:]):
            TR.check_grammar(w.tokens, ts_begin, EOS, NOTS, 50)
            assert not np.isin(w.tokens, SUPPRESS_T).any() and len(w.tokens) <= 16
            sg, new_seek = segments_from_window(w.tokens, w.seek, w.segment_frames, ts_begin, EOS, 2, w.avg_logprob, w.no_speech_prob, 0.6, -1.0)
            assert min(new_seek, r.content_frames) == nxt
            segs += sg
        assert segs == r.segments
    assert len(res[1].windows) >= 2
    print(f"transcribe(beam_size=2): seeks {[r.seeks for r in res]}, segments {[len(r.segments) for r in res]}")
    one, dflt = m.transcribe(files, beam_size=1, _max_rounds=64), m.transcribe(files, _max_rounds=64)
    for a, b in zip(one, dflt):
        assert a.seeks == b.seeks and [w.tokens for w in a.windows] == [w.tokens for w in b.windows] and a.language == b.language


def test_command_line_beam(long_weights, noise, tmp_path, capsys):
    from ssak_amd import whisper_infer
    from ssak_amd.data import load_audio
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    folder = G.write_folder(_Stored(long_weights, long_generation_config()), str(tmp_path / "model"), max_source_positions=1500, encoder_layers=1,
                            config_overrides={"vocab_size": VT})
    path = str(tmp_path / "noise5.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(16000)
        f.writeframes((noise[0].numpy() * 32767).astype("<i2").tobytes())
    m = WhisperSeq2Seq.from_pretrained(folder)
    audio = torch.from_numpy(load_audio(path))
    whisper_infer.main([path, "--model", folder, "--language", "en", "--timestamps", "--beam_size", "2"])
    lines = capsys.readouterr().out.strip().splitlines()
    want = m.transcribe([audio], language="en", beam_size=2)[0].segments
    assert len(lines) == len(want)
    for line, sg in zip(lines, want):
        assert [int(t) for t in line.split("\t")[3].split()] == [t for t in sg.tokens if t < NOTS + 1]
    whisper_infer.main([path, "--model", folder, "--language", "en", "--max_new_tokens", "5", "--beam_size", "2"])
    lines = capsys.readouterr().out.strip().splitlines()
    ids = [int(t) for t in lines[0].split("\t")[1].split()]
    assert len(lines) == 1 and lines[0].split("\t")[0] == path and 1 <= len(ids) <= 5 and all(0 <= t < VT for t in ids)
    with pytest.raises(SystemExit):
        whisper_infer.main([path, "--model", folder, "--beam_size", "9"])
