"""CPU: the float64 restatement of greedy generation, tests/whisper_generate_ref.py, against ``transformers`` in float64 on the
tiny model of tests/golden/whisper_dec_tiny.npz (``gen_golden_whisper_dec.hf_model``): identical tokens, log-probabilities
within 1e-9; and its split-and-combine softmax against ``whisper_decoder_ref.attention`` at 1e-12, an empty split among the pieces.

The transformers side is a loop over ``model(..., past_key_values=..., use_cache=True)`` from a given encoder output and prompt
with transformers' OWN two suppress processors applied to the last row -- ``WhisperForConditionalGeneration.generate`` wraps the
same loop in prompt, language and timestamp handling that would have to be switched off piece by piece.  transformers' Whisper
decoder takes no encoder mask, so each utterance runs alone on the first ``enc_lens[b]`` frames of its encoder output, as in the
fixture's generator.  The transformers tests skip where it is not installed.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_decoder_ref as WR  # noqa: E402
import whisper_generate_ref as GR  # noqa: E402

N_NEW = 10
SUPPRESS = list(range(G.EOT, G.NO_TIMESTAMPS + 1))  # every special token, as Whisper's own list does: the text ids remain


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


@pytest.fixture(scope="module")
def weights(golden):
    return {k[2:]: WR.bf16_from_bits(golden[k]) for k in golden.files if k.startswith("w/")}


def prompts():
    return np.array([[G.SOT, G.LANG0 + b, G.TRANSCRIBE, G.NO_TIMESTAMPS] for b in range(G.B)])


def hf_greedy(model, enc, prompt, n_new, eos, suppress, begin_suppress):
    """One utterance: (tokens, log-probabilities) until ``eos`` or ``n_new`` tokens, transformers' cache and processors."""
    import torch
    from transformers import SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor
    procs = [SuppressTokensLogitsProcessor(suppress)] if suppress else []
    if begin_suppress:
        procs.append(SuppressTokensAtBeginLogitsProcessor(begin_suppress, begin_index=len(prompt)))
    ids = torch.tensor([list(prompt)])
    enc_out = (torch.from_numpy(np.asarray(enc, dtype=np.float64))[None],)
    past, feed, toks, lps = None, ids, [], []
    with torch.no_grad():
        for _ in range(n_new):
            out = model(encoder_outputs=enc_out, decoder_input_ids=feed, past_key_values=past, use_cache=True)
            past = out.past_key_values
            scores = out.logits[:, -1]
            for proc in procs:
                scores = proc(ids, scores)
            lsm = torch.log_softmax(scores, -1)
            tok = int(lsm.argmax(-1))
            toks.append(tok)
            lps.append(float(lsm[0, tok]))
            feed = torch.tensor([[tok]])
            ids = torch.cat([ids, feed], 1)
            if tok == eos:
                break
    return toks, lps


def test_greedy_against_transformers_float64(golden, weights):
    pytest.importorskip("transformers")
    model = G.hf_model({k: v for k, v in weights.items()})
    enc, enc_lens = WR.bf16_from_bits(golden["enc"]), [int(v) for v in golden["enc_lens"]]
    pr = prompts()
    free = GR.generate(weights, G.NH, G.LAYERS, enc, pr, N_NEW, G.EOT, G.EOT, SUPPRESS, None, enc_lens)
    assert (free["lens"] == N_NEW).all() and not np.isin(free["tokens"], SUPPRESS).any()
    # an eos that occurs (utterance 0's token at step 3) and a begin-suppressed step-0 token (utterance 1's)
    eos, begin = int(free["tokens"][0, 3]), [int(free["tokens"][1, 0])]
    sup = [s for s in SUPPRESS if s != eos]
    ref = GR.generate(weights, G.NH, G.LAYERS, enc, pr, N_NEW, eos, G.EOT, sup, begin, enc_lens)
    assert ref["tokens"][1, 0] != begin[0] and ref["lens"][0] <= 4
    for b in range(G.B):
        toks, lps = hf_greedy(model, enc[b, :enc_lens[b]], pr[b], N_NEW, eos, sup, begin)
        n = int(ref["lens"][b])
        d = float(np.abs(np.array(lps) - ref["logprobs"][b, :n]).max())
        print(f"utterance {b}: {n} tokens {toks}, max |log-prob difference| {d:.3e}")
        assert toks == ref["tokens"][b, :n].tolist() and d < 1e-9
        assert (ref["tokens"][b, n:] == G.EOT).all() and (ref["logprobs"][b, n:] == 0).all(), "a finished row pads with log-probability 0"


def test_greedy_step_rules():
    """The lowest id wins a tie; a suppressed maximum is not chosen and does not enter the log-softmax; begin_suppress acts only
    when ``first``; finished rows emit pad with log-probability 0 and stay finished; eos finishes a row."""
    x = np.zeros((4, 9))
    x[0, [2, 6]] = 5.0
    x[1, 4], x[1, 7] = 9.0, 3.0
    x[2, 1] = 4.0
    x[3, 8] = 2.0
    tok, lp, fin = GR.greedy_step(x, [False, False, False, True], eos=1, pad=0, suppress=[4], begin_suppress=[7], first=False)
    assert tok.tolist() == [2, 7, 1, 0] and fin.tolist() == [False, False, True, True] and lp[3] == 0.0
    want = 3.0 - np.log(np.exp(3.0) + 7.0)  # row 1 without column 4
    assert abs(lp[1] - want) < 1e-12
    tok, _, _ = GR.greedy_step(x, [False] * 4, eos=1, pad=0, suppress=[4], begin_suppress=[7], first=True)
    assert tok[1] == 0


@pytest.mark.parametrize("n_keys,n_split", [(1, 1), (1, 5), (33, 2), (33, 5), (131, 1), (131, 5)])
def test_split_and_combine_softmax(n_keys, n_split):
    """Partials per split, combined in order, equal the one-piece softmax; klens = 1 leaves every split but the first empty (at
    n_split = 5), and the rows past n_keys / klens are NaN."""
    rng = np.random.default_rng(n_keys * 10 + n_split)
    B, nh, cap = 3, 2, n_keys + 3
    q = rng.standard_normal((B, nh * 64))
    k, v = rng.standard_normal((B, cap, nh * 64)), rng.standard_normal((B, cap, nh * 64))
    for klens in (None, (n_keys, 1, n_keys // 2 + 1)):
        kk, vv = k.copy(), v.copy()
        kk[:, n_keys:] = vv[:, n_keys:] = np.nan
        if klens is not None:
            for b, n in enumerate(klens):
                kk[b, n:] = vv[b, n:] = np.nan
        got = GR.split_attention(q, kk, vv, nh, n_keys, n_split, klens)
        want = WR.attention(q[:, None], np.nan_to_num(kk[:, :n_keys]), np.nan_to_num(vv[:, :n_keys]), nh, klens)[:, 0]
        assert np.isfinite(got).all() and np.abs(got - want).max() < 1e-12
        if klens is not None:
            assert np.abs(got[1] - v[1, 0]).max() < 1e-15, "one visible key: ctx is its value row"


# ------------------------------------------------------------------------------------------------------------ host finalisation
def _rows(rows, pad):
    """[(tokens, logprobs)] per row, as long as the longest -> int32 / float64 arrays the way the loop leaves them."""
    n = max(len(t) for t, _ in rows)
    tok, lp = np.full((len(rows), n), pad, dtype=np.int32), np.zeros((len(rows), n))
    for r, (t, l) in enumerate(rows):
        tok[r, :len(t)], lp[r, :len(l)] = t, l
    return tok, lp


def test_rows_finalize_greedy():
    """eos mid-row (the row goes on with pad and 0), no eos (length = steps), eos at the first step.  Every log-probability is a small
    dyadic number, so every sum below is exact."""
    from ssak_amd.whisper_seq2seq import rows_finalize
    eos, pad = 9, 0
    tok, lp = _rows([([5, 6, eos, pad, pad], [-0.5, -0.25, -1.0]), ([3, 4, 5, 6, 7], [-0.5] * 5), ([eos, pad, pad, pad, pad], [-2.0])], pad)
    out = rows_finalize(tok, lp, 5, eos, pad)
    assert out["tokens"] == [[5, 6, eos], [3, 4, 5, 6, 7], [eos]] and out["lens"].tolist() == [3, 5, 1] and out["lens"].dtype == np.int64
    assert out["token_array"].dtype == np.int32 and out["token_array"].tolist() == [[5, 6, eos, pad, pad], [3, 4, 5, 6, 7], [eos, pad, pad, pad, pad]]
    assert out["logprobs"].dtype == np.float64 and out["logprobs"].tolist() == [[-0.5, -0.25, -1.0, 0, 0], [-0.5] * 5, [-2.0, 0, 0, 0, 0]]
    assert out["sum_logprob"].tolist() == [-1.75, -2.5, -2.0] and out["avg_logprob"].tolist() == [-1.75 / 4, -2.5 / 6, -1.0]
    assert "samples" not in out and "sample_logprobs" not in out
    # fewer steps than the arrays are wide (the loop stopped early): nothing past them is read; the arrays are as wide as the longest row
    out = rows_finalize(tok, lp, 2, eos, pad)
    assert out["tokens"] == [[5, 6], [3, 4], [eos]] and out["sum_logprob"].tolist() == [-0.75, -1.0, -2.0]
    assert out["token_array"].tolist() == [[5, 6], [3, 4], [eos, pad]]


def test_rows_finalize_pad_is_eos():
    """pad == eos: the row ends with its FIRST eos; the pads after it are no tokens, and a log-probability left past the end is dropped."""
    from ssak_amd.whisper_seq2seq import rows_finalize
    eos = pad = 9
    tok, lp = _rows([([5, eos, eos, eos], [-0.5, -0.25, -8.0]), ([1, 2, 3, eos], [-1.0] * 4)], pad)
    out = rows_finalize(tok, lp, 4, eos, pad)
    assert out["tokens"] == [[5, eos], [1, 2, 3, eos]] and out["lens"].tolist() == [2, 4]
    assert out["token_array"].tolist() == [[5, eos, pad, pad], [1, 2, 3, eos]]
    assert out["logprobs"].tolist() == [[-0.5, -0.25, 0, 0], [-1.0] * 4] and out["sum_logprob"].tolist() == [-0.75, -4.0]


def test_rows_finalize_best_of():
    """Two utterances x three rows, score = sum / tokens before eos.  Utterance 0: -1 / 1, -0.75 / 3, -2 / 2 -> the middle row, under
    every ``length_penalty`` tried (its sum is the largest too).  Utterance 1: -3 / 4 (no eos), -2 / 1, -1 / 2 -> the last row; with
    ``length_penalty`` a the scores are sum / ((5 + n) / 6) ** a: a = 1 gives -2, -2, -6 / 7 -> the last; a = 4 gives -0.593, -2,
    -0.540 -> the last; a = 8 gives -0.117, -2, -0.291 -> the first."""
    from ssak_amd.whisper_seq2seq import rows_finalize
    eos, pad = 9, 0
    rows = [([5, eos], [-0.5, -0.5]), ([5, 6, 7, eos], [-0.25, -0.25, -0.125, -0.125]), ([5, 6, eos], [-1.0, -0.5, -0.5]),
            ([1, 2, 3, 4], [-0.75] * 4), ([1, eos], [-1.0, -1.0]), ([1, 2, eos], [-0.5, -0.25, -0.25])]
    tok, lp = _rows(rows, pad)
    out = rows_finalize(tok, lp, 4, eos, pad, best_of=3)
    assert out["tokens"] == [[5, 6, 7, eos], [1, 2, eos]] and out["lens"].tolist() == [4, 3]
    assert out["token_array"].tolist() == [[5, 6, 7, eos], [1, 2, eos, pad]]
    assert out["logprobs"].tolist() == [[-0.25, -0.25, -0.125, -0.125], [-0.5, -0.25, -0.25, 0]]
    assert out["sum_logprob"].tolist() == [-0.75, -1.0] and out["avg_logprob"].tolist() == [-0.75 / 5, -0.25]
    assert out["samples"] == [[(t, float(sum(l))) for t, l in rows[:3]], [(t, float(sum(l))) for t, l in rows[3:]]]
    assert [[l.tolist() for l in u] for u in out["sample_logprobs"]] == [[l for _, l in rows[:3]], [l for _, l in rows[3:]]]
    for penalty, want in ((0.0, [[5, 6, 7, eos], [1, 2, eos]]), (1.0, [[5, 6, 7, eos], [1, 2, eos]]), (4.0, [[5, 6, 7, eos], [1, 2, eos]]),
                          (8.0, [[5, 6, 7, eos], [1, 2, 3, 4]])):
        assert rows_finalize(tok, lp, 4, eos, pad, best_of=3, length_penalty=penalty)["tokens"] == want, penalty
    # best_of = 1 lists its one candidate per utterance and sums the whole row
    one = rows_finalize(tok, lp, 4, eos, pad, best_of=1)
    assert one["tokens"] == [t for t, _ in rows] and [len(u) for u in one["samples"]] == [1] * 6
