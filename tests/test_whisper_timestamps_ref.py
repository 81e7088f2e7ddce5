"""CPU: the float64 restatement of the timestamp step, tests/whisper_timestamps_ref.py, against
``transformers.generation.logits_process.WhisperTimeStampLogitsProcessor`` followed by arg-max and ``log_softmax`` in float64, on
the fixture's id layout (V = 127, eos 100, ``<|notimestamps|>`` 110, timestamps 111-126): identical masks and tokens, log-probs
within 1e-9.  And the host half of long-form transcription, ``ssak_amd.whisper_transcribe.segments_from_window`` /
``seek_loop``, on hand-worked token lists and a scripted decoder stub.  The transformers test skips where it is not installed.
"""
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_timestamps_ref as TR  # noqa: E402

from ssak_amd.whisper_transcribe import seek_loop, segments_from_window  # noqa: E402

V, EOS, NOTS, TSB = G.V, G.EOT, G.NO_TIMESTAMPS, G.NO_TIMESTAMPS + 1
N_CASES = 2400


def random_case(rng):
    """(logits [V], history, suppress ids, max_initial).  Histories of 0-8 tokens: grammatical ones grown by the rules' own
    masks, and arbitrary mixes of text and timestamps; the timestamps' share of the mass is drawn so that both outcomes of the
    mass decision occur."""
    n = int(rng.integers(0, 9))
    if rng.random() < 0.5:
        hist = []
        while len(hist) < n:
            ok = TR.allowed_columns(V, hist, TSB, NOTS, EOS, None)
            ok[EOS:TSB] = False
            ids = np.flatnonzero(ok)
            ts = ids[ids >= TSB]
            hist.append(int(rng.choice(ts if ts.size and rng.random() < 0.5 else ids)))
    else:
        hist = [int(rng.integers(TSB, V)) if rng.random() < 0.4 else int(rng.integers(0, EOS)) for _ in range(n)]
    x = 3.0 * rng.standard_normal(V)
    x[TSB:] += rng.uniform(-6.0, 4.0)
    suppress = sorted(set(rng.integers(0, V, size=int(rng.integers(0, 6))).tolist()))
    return x, hist, suppress, (None, 5)[int(rng.integers(0, 2))]


def test_step_against_transformers_float64():
    pytest.importorskip("transformers")
    import torch
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    rng = np.random.default_rng(620)
    prompt = [G.SOT, G.LANG0, G.TRANSCRIBE]
    took_ts = took_text = 0
    worst = 0.0
    for case in range(N_CASES):
        x, hist, suppress, max_initial = random_case(rng)
        cfg = types.SimpleNamespace(no_timestamps_token_id=NOTS, eos_token_id=EOS, bos_token_id=EOS, max_initial_timestamp_index=max_initial)
        proc = WhisperTimeStampLogitsProcessor(cfg, begin_index=len(prompt))
        scores = torch.from_numpy(x.copy())[None]
        scores[:, suppress] = -float("inf")  # (transformers' suppress processors run before the timestamp processor)
        out = proc(torch.tensor([prompt + hist]), scores)[0]
        r = TR.timestamp_step_row(x, hist, TSB, NOTS, EOS, max_initial, suppress)
        hf_mask = torch.isfinite(out).numpy()
        assert np.array_equal(hf_mask, r["mask"]), (case, hist, max_initial)
        assert hf_mask.any()
        lsm = torch.log_softmax(out, -1)
        tok = int(lsm.argmax())
        assert tok == r["token"], (case, hist)
        worst = max(worst, abs(float(lsm[tok]) - r["logprob"]))
        before = TR.allowed_columns(V, hist, TSB, NOTS, EOS, max_initial, suppress)
        took_ts += bool(before[:TSB].any() and not r["mask"][:TSB].any())
        took_text += tok < TSB
        assert r["ts_last"] == TR.last_timestamp(hist + [tok], TSB)
    print(f"{N_CASES} cases: max |log-prob difference| {worst:.3e}; the mass decision masked the text in {took_ts}, text chosen in {took_text}")
    assert worst < 1e-9 and took_ts > 100 and took_text > 100


def test_step_rules_by_hand():
    """Each rule on a row small enough to work by hand (V = 12, eos 4, <|notimestamps|> 6, timestamps 7-11)."""
    kw = dict(ts_begin=7, no_timestamps=6, eos=4)
    x = np.zeros(12)
    r = TR.timestamp_step_row(x, [], max_initial=2, **kw)
    assert r["mask"].tolist() == [False] * 7 + [True] * 3 + [False] * 2 and r["token"] == 7 and abs(r["logprob"] + np.log(3)) < 1e-12
    r = TR.timestamp_step_row(x, [8], **kw)  # after [ts]: no timestamp; text mass only
    assert r["mask"].tolist() == [True] * 6 + [False] * 6 and r["token"] == 0 and r["ts_last"] == 8
    r = TR.timestamp_step_row(x, [8, 1], **kw)  # timestamps 9.. allowed: 3 x e^0 outweighs one text token -> timestamps only
    assert r["mask"].tolist() == [False] * 9 + [True] * 3 and r["token"] == 9 and abs(r["logprob"] + np.log(3)) < 1e-12 and r["ts_last"] == 9
    y = x.copy()
    y[2] = 5.0  # log 3 < 5: the text token stays
    r = TR.timestamp_step_row(y, [8, 1], **kw)
    assert r["token"] == 2 and r["mask"].sum() == 9 and r["ts_last"] == 8
    assert abs(r["margin"] - abs(np.log(3) - 5 - (5.0 - 5.0))) < 1e-12
    r = TR.timestamp_step_row(x, [8, 1, 9], **kw)  # text below eos masked; 9 itself allowed again
    assert TR.allowed_columns(12, [8, 1, 9], 7, 6, 4).tolist() == [False] * 4 + [True, True, False] + [False, False, True, True, True]
    assert r["mask"].tolist() == [False] * 9 + [True] * 3 and r["token"] == 9, "log 3 > 0: the two specials go as well"
    r = TR.timestamp_step_row(x, [8, 1, 9, 9], **kw)
    assert r["mask"].tolist() == [True] * 6 + [False] * 6
    toks, lps, fin, rows = TR.timestamp_step(np.zeros((2, 12)), [[8], [8]], [True, False], pad=5, **kw)
    assert toks.tolist() == [5, 0] and lps[0] == 0.0 and fin.tolist() == [True, False] and rows[0] is None


# ------------------------------------------------------------------------------------------------------------ the seek rules
T0 = 111  # ts_begin; input_stride 2: one timestamp step = 0.02 s = 2 frames
SEG = dict(ts_begin=T0, eos=100)


def spans(segs):
    return [(round(s.start, 6), round(s.end, 6), s.tokens) for s in segs]


def test_segments_no_timestamp_and_only_zero():
    segs, seek = segments_from_window([5, 6, 7], 0, 3000, **SEG)
    assert spans(segs) == [(0.0, 30.0, [5, 6, 7])] and seek == 3000
    segs, seek = segments_from_window([T0], 1000, 3000, **SEG)  # one segment of the whole window without text: dropped
    assert segs == [] and seek == 4000
    segs, seek = segments_from_window([], 0, 3000, **SEG)
    assert segs == [] and seek == 3000


def test_segments_single_pair_then_eos():
    """[<|0.00|> text text <|0.10|>] eos: no consecutive pair; the segment ends at the last timestamp, the seek takes the window."""
    segs, seek = segments_from_window([T0, 5, 6, T0 + 5], 1000, 3000, **SEG)
    assert spans(segs) == [(10.0, 10.1, [T0, 5, 6, T0 + 5])] and seek == 4000 and segs[0].seek == 1000


def test_segments_two_pairs_ending_in_a_pair():
    toks = [T0, 5, T0 + 5, T0 + 5, 6, T0 + 10, T0 + 10]
    segs, seek = segments_from_window(toks, 1000, 3000, **SEG)
    assert spans(segs) == [(10.0, 10.1, [T0, 5, T0 + 5]), (10.1, 10.2, [T0 + 5, 6, T0 + 10])]
    assert seek == 1000 + 10 * 2, "the seek moves by the last timestamp"


def test_segments_trailing_text_and_single_ending():
    segs, seek = segments_from_window([T0, 5, T0 + 5, T0 + 5, 6, 7], 0, 3000, **SEG)  # the trailing run is decoded again from 0.1 s
    assert spans(segs) == [(0.0, 0.1, [T0, 5, T0 + 5])] and seek == 10
    segs, seek = segments_from_window([T0, 5, T0 + 5, T0 + 5, 6, T0 + 10], 0, 3000, **SEG)  # single ending: the tail is a segment
    assert spans(segs) == [(0.0, 0.1, [T0, 5, T0 + 5]), (0.1, 0.2, [T0 + 5, 6, T0 + 10])] and seek == 3000


def test_segments_without_text_are_dropped():
    """Slices [<|0.00|> <|sot|> <|0.10|>] (a special is no text) and [<|0.20|>] (start == end) go; the one with text stays."""
    toks = [T0, 101, T0 + 5, T0 + 5, 5, T0 + 10, T0 + 10, T0 + 10, 6, T0 + 15, T0 + 15]
    segs, seek = segments_from_window(toks, 0, 3000, **SEG)
    assert spans(segs) == [(0.1, 0.2, [T0 + 5, 5, T0 + 10]), (0.2, 0.3, [T0 + 10, 6, T0 + 15])] and seek == 30


def test_segments_no_speech_skip_and_rescue():
    toks = [T0, 5, T0 + 5]
    kw = dict(no_speech_prob=0.9, no_speech_threshold=0.6, logprob_threshold=-1.0)
    assert segments_from_window(toks, 200, 3000, avg_logprob=-2.0, **kw, **SEG) == ([], 3200)
    segs, seek = segments_from_window(toks, 200, 3000, avg_logprob=-0.5, **kw, **SEG)
    assert spans(segs) == [(2.0, 2.1, toks)] and seek == 3200 and segs[0].avg_logprob == -0.5 and segs[0].no_speech_prob == 0.9
    segs, _ = segments_from_window(toks, 200, 3000, avg_logprob=-2.0, no_speech_prob=0.5, no_speech_threshold=0.6, logprob_threshold=-1.0, **SEG)
    assert len(segs) == 1, "below the threshold nothing is skipped"


def test_segments_short_last_window():
    segs, seek = segments_from_window([5, 6], 2000, 500, **SEG)
    assert spans(segs) == [(20.0, 25.0, [5, 6])] and seek == 2500
    segs, seek = segments_from_window([T0, 5, T0 + 50, T0 + 50, 6, T0 + 400, T0 + 400], 2000, 500, **SEG)  # a timestamp past the content
    assert seek == 2800 and len(segs) == 2


def test_seek_loop_on_a_scripted_decoder():
    """Three files of 5 s, 31 s and 47 s; the stub answers by (file, seek).  The short file leaves after round one."""
    content = [500, 3100, 4700]
    script = {(0, 0): ([T0, 5, T0 + 100], -0.3, 0.1),                                     # single ending: the window
              (1, 0): ([T0, 5, T0 + 1000, T0 + 1000, 6, T0 + 1200, T0 + 1200], -0.3, 0.1),  # to 24 s
              (1, 2400): ([T0, 7], -0.3, 0.1),                                             # 7 s left, no closing timestamp
              (2, 0): ([T0, 5, 6], -0.3, 0.1),
              (2, 3000): ([T0, 5, T0 + 10], -1.5, 0.8)}                                    # silent: skipped
    calls = []

    def decode(active, seeks, frames):
        calls.append((list(active), list(seeks), list(frames)))
        return [script[(f, s)] for f, s in zip(active, seeks)]

    out = seek_loop(content, decode, T0, 100, 2, 0.6, -1.0, max_rounds=4)
    assert calls == [([0, 1, 2], [0, 0, 0], [500, 3000, 3000]), ([1, 2], [2400, 3000], [700, 1700])]
    assert [o[2] for o in out] == [[0, 500], [0, 2400, 3100], [0, 3000, 4700]]
    assert [len(o[0]) for o in out] == [1, 3, 1] and [len(o[1]) for o in out] == [1, 2, 2]
    assert spans(out[1][0])[2] == (24.0, 31.0, [T0, 7]) and spans(out[0][0]) == [(0.0, 2.0, [T0, 5, T0 + 100])]
    with pytest.raises(RuntimeError, match="rounds"):
        seek_loop(content, decode, T0, 100, 2, 0.6, -1.0, max_rounds=1)
