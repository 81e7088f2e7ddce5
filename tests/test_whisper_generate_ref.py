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
