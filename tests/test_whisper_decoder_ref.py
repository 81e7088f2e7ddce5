"""CPU: the float64 restatement tests/whisper_decoder_ref.py against ``transformers.WhisperForConditionalGeneration`` in float64
(logits of every position and ``.loss`` at 1e-10, on the seeded tiny model of tests/gen_golden_whisper_dec.py), its language rule
against a direct restatement of ``whisper.decoding.detect_language``'s masking, and the stored fixture against both.  The tests
that need ``transformers`` skip where it is not installed; the others check the restatement's own pieces (``q_offset``,
``klens``, ``allowed``, the bf16 rounding) against each other and against torch."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_decoder_ref as WR  # noqa: E402

TOL = 1e-10


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


@pytest.fixture(scope="module")
def weights(golden):
    return {k[2:]: WR.bf16_from_bits(golden[k]) for k in golden.files if k.startswith("w/")}


def test_bf16_round_is_torch_round_to_nearest_even():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4096, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-6, 6, (4096,), generator=g).double()
    x[:4] = torch.tensor([1.00390625, 1.01171875, 0.0, -1.00390625])  # ties: to even mantissa
    want = x.float().to(torch.bfloat16).double().numpy()
    got = WR.bf16_round(x.numpy())
    assert np.array_equal(got, want)
    assert np.array_equal(WR.bf16_from_bits(WR.bf16_bits(got)), got)


def test_attention_masks_against_explicit_softmax():
    rng = np.random.default_rng(1)
    B, Lq, Lk, nh = 2, 5, 12, 2
    q, k, v = (rng.standard_normal((B, n, nh * 64)) for n in (Lq, Lk, Lk))
    klens, off = [12, 9], 7
    got = WR.attention(q, k, v, nh, klens, True, off)
    for b in range(B):
        for h in range(nh):
            sl = slice(64 * h, 64 * h + 64)
            for i in range(Lq):
                n = min(klens[b], off + i + 1)
                s = torch.from_numpy(q[b, i, sl] @ k[b, :n, sl].T / 8.0)
                want = torch.softmax(s, -1).numpy() @ v[b, :n, sl]
                assert np.abs(got[b, i, sl] - want).max() < 1e-12
    # the incremental step (one query at q_offset) is the last row of the whole causal pass
    full = WR.attention(k[:, :8], k[:, :8], v[:, :8], nh, None, True, 0)
    step = WR.attention(k[:, 7:8], k[:, :8], v[:, :8], nh, None, True, 7)
    assert np.abs(full[:, 7:8] - step).max() < 1e-12


def test_token_logprobs_against_torch():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((5, 203)) * 3
    x[3, 17] = x[3, 90] = x[3].max() + 1.0  # a tie: the lowest id
    tg = np.array([3, -100, 202, 90, 0])
    r = WR.token_logprobs(x, tg)
    lsm = torch.log_softmax(torch.from_numpy(x), -1).numpy()
    assert np.abs(r["lse"] - torch.logsumexp(torch.from_numpy(x), -1).numpy()).max() < 1e-12
    assert r["logprob"][1] == 0.0 and r["argmax"][3] == 17
    for i in (0, 2, 3, 4):
        assert abs(r["logprob"][i] - lsm[i, tg[i]]) < 1e-12
    allowed = [5, 17, 40, 90, 150, 201, 202]
    ra = WR.token_logprobs(x, tg, allowed)
    want = torch.softmax(torch.from_numpy(x[:, allowed]), -1).numpy()
    assert np.abs(ra["probs"] - want).max() < 1e-14 and ra["argmax"][3] == 17


def test_language_rule_is_detect_language_masking(golden):
    """whisper/decoding.py detect_language: ``mask = ones(V, bool); mask[all_language_tokens] = False; logits[:, mask] = -inf;
    language_tokens = logits.argmax(-1); probs = logits.softmax(-1)``, then the probabilities of the language tokens."""
    logits = torch.from_numpy(golden["hf_logits"][:, 0].copy())
    lang_ids = [int(i) for i in golden["lang_ids"]]
    mask = torch.ones(logits.shape[-1], dtype=torch.bool)
    mask[lang_ids] = False
    logits[:, mask] = -np.inf
    want_tok = logits.argmax(-1).numpy()
    want = logits.softmax(-1)[:, lang_ids].numpy()
    tok, probs = WR.language_probs(golden["hf_logits"][:, 0], lang_ids)
    assert np.array_equal(tok, want_tok)
    assert np.abs(probs - want).max() < 1e-14
    assert np.abs(probs - golden["lang_probs"]).max() < 1e-14
    top = np.sort(probs, -1)
    assert float((top[:, -1] - top[:, -2]).min()) >= G.MARGIN  # what lets the GPU test demand every arg-max


def test_fixture_is_the_restatement(golden, weights):
    """The stored transformers results against the restatement with ``enc_lens`` as a key mask (transformers ran each utterance on
    its truncated encoder output) -- runs without transformers."""
    enc, tokens = WR.bf16_from_bits(golden["enc"]), golden["tokens"]
    lens, enc_lens = [int(v) for v in golden["lens"]], [int(v) for v in golden["enc_lens"]]
    logits = WR.decoder_logits(weights, G.NH, G.LAYERS, enc, tokens, enc_lens)
    assert np.abs(logits - golden["hf_logits"]).max() < TOL
    sc = WR.scores(logits, tokens, lens)
    assert np.abs(sc["loss"] - golden["hf_loss"]).max() < TOL and abs(sc["batch_loss"] - float(golden["hf_batch_loss"])) < TOL
    assert list(sc["n_scored"]) == [11, 1, 6]
    assert np.all(sc["logprobs"][1, 1:] == 0) and np.all(sc["logprobs"][2, 6:] == 0)
    assert np.allclose(sc["avg_logprob"], sc["sum_logprob"] / (sc["n_scored"] + 1), rtol=0, atol=0)


def test_restatement_against_transformers_float64(golden, weights):
    pytest.importorskip("transformers")
    enc, tokens = WR.bf16_from_bits(golden["enc"]), golden["tokens"]
    lens = [int(v) for v in golden["lens"]]
    model = G.hf_model(weights)
    labels = WR.shifted_targets(tokens, lens)
    hf_logits, hf_loss = G.hf_forward(model, enc, tokens, labels)  # the whole batch, every encoder frame visible
    logits = WR.decoder_logits(weights, G.NH, G.LAYERS, enc, tokens)
    err = float(np.abs(logits - hf_logits).max())
    loss = WR.scores(logits, tokens, lens)["batch_loss"]
    print(f"logits max abs err {err:.3g}, loss {loss:.12f} vs {hf_loss:.12f}")
    assert err < TOL and abs(loss - hf_loss) < TOL
    # an utterance alone on its truncated encoder output = the key mask (how the fixture was made)
    b, n = 2, int(golden["enc_lens"][2])
    one, one_loss = G.hf_forward(model, enc[b:b + 1, :n], tokens[b:b + 1], labels[b:b + 1])
    assert np.abs(one[0] - golden["hf_logits"][b]).max() < TOL and abs(one_loss - float(golden["hf_loss"][b])) < TOL
    # a position offset (the next pull request's incremental step) moves only the position rows
    step = WR.decoder_logits(weights, G.NH, G.LAYERS, enc[:1], tokens[:1, :1], pos_offset=3)
    h0 = WR.embed(weights["model.decoder.embed_tokens.weight"], weights["model.decoder.embed_positions.weight"], tokens[:1, :1], 3)
    assert np.array_equal(h0[0, 0], weights["model.decoder.embed_tokens.weight"][tokens[0, 0]] + weights["model.decoder.embed_positions.weight"][3])
    assert step.shape == (1, 1, G.V)
