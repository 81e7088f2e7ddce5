"""CPU: the restatement tests/whisper_sample_ref.py draws from the right distribution, and the host half of Whisper sampling and
temperature fallback -- ``ssak_amd.whisper_transcribe.decode_with_fallback``, the ``best_of`` ranking through
``ssak_amd.whisper_seq2seq.beam_rank``, the command line's temperature schedule -- on its own.  Every case prints its figures
before it asserts.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_decoder_ref as WR  # noqa: E402
import whisper_sample_ref as SR  # noqa: E402
import whisper_timestamps_ref as TR  # noqa: E402
from oracle import dropout_hash as DH  # noqa: E402

from ssak_amd.whisper_transcribe import compression_ratio, decode_with_fallback  # noqa: E402


# ------------------------------------------------------------------------------------------------------------ the noise
def test_hash_is_the_oracles():
    rng = np.random.default_rng(0)
    for _ in range(8):
        seed = int(rng.integers(0, 2 ** 63)) * 2 + 1
        idx = rng.integers(0, 2 ** 63, size=256).astype(np.uint64)
        assert np.array_equal(DH.hash_u32(seed, SR.DS_SAMPLE, idx), SR.hash_u32(np.uint64(seed), SR.DS_SAMPLE, idx))


def test_uniform_is_inside_the_unit_interval_and_exact_in_fp32():
    u = SR.uniforms(SR.CHI_SEED, 7, np.arange(4096), 64)
    print(f"u in [{u.min():.3e}, 1 - {1 - u.max():.3e}]")
    assert u.min() >= 2.0 ** -24 and u.max() <= 1 - 2.0 ** -24 and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    k = u * 2.0 ** 24
    assert np.array_equal(k, np.floor(k)) and (k.astype(np.int64) % 2 == 1).all(), "an odd multiple of 2^-24"
    g = SR.gumbel(SR.CHI_SEED, 7, np.arange(4096), 64)
    assert g.min() >= -np.log(24 * np.log(2)) - 1e-12 and g.max() <= 24 * np.log(2) + 1e-6


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_draws_follow_softmax(temperature):
    """65 536 rows of one 8-column row, then 65 536 steps of one row: chi-square of the counts against softmax(x / T) below the
    99.9 % point of chi-square(7) = 24.322; the draws of rows r and r + 1 uncorrelated within 4 / sqrt(N)."""
    x = SR.chi_logits()
    N = SR.CHI_N
    tok, single = SR.draw_rows(x, temperature, SR.CHI_SEED, 3, np.arange(N))
    chi, counts = SR.chi_square(tok, x, temperature)
    corr = np.corrcoef(tok[:-1], tok[1:])[0, 1]
    print(f"T = {temperature}: over rows chi-square {chi:.3f} (bar {SR.CHI2_7_999}), counts {counts.astype(int).tolist()}, "
          f"corr(r, r + 1) {corr:+.4f} (bar {4 / np.sqrt(N):.4f}), accept sets of one column {single.mean():.4f}")
    assert chi < SR.CHI2_7_999 and abs(corr) <= 4 / np.sqrt(N)
    tok_t, _ = SR.draw_rows(x, temperature, SR.CHI_SEED, np.arange(N), np.full(N, 5))
    chi_t, counts_t = SR.chi_square(tok_t, x, temperature)
    print(f"T = {temperature}: over steps chi-square {chi_t:.3f}, counts {counts_t.astype(int).tolist()}")
    assert chi_t < SR.CHI2_7_999
    # the vectorised draw is the per-row restatement
    toks, _, _, rows = SR.sample_step(np.tile(x.astype(np.float64), (64, 1)), np.zeros(64, bool), 0, 0, temperature, SR.CHI_SEED, 3)
    assert np.array_equal(toks, tok[:64]) and all((len(r["accept"]) == 1) == s for r, s in zip(rows, single[:64]))


def test_random_rows_accept_sets_are_single():
    """The GPU test's random rows (65 x 127, T = 0.8, steps 0 .. 2, with and without the rules): at most 1 % of the accept sets hold
    more than one column, and with the rules the mass decision's margin is beyond what fp32 can flip."""
    x = SR.random_rows()[:, :SR.RANDOM_V].astype(np.float64)
    many = total = 0
    margin = np.inf
    for t, hist in ((0, []), (1, [G.NO_TIMESTAMPS + 3]), (2, [G.NO_TIMESTAMPS + 3, 7])):
        for hists in (None, [hist] * SR.RANDOM_ROWS):
            _, _, _, rows = SR.sample_step(x, np.zeros(SR.RANDOM_ROWS, bool), G.EOT, G.EOT, SR.RANDOM_T, SR.RANDOM_SEED, t, hists,
                                           ts_begin=G.NO_TIMESTAMPS + 1, no_timestamps=G.NO_TIMESTAMPS, max_initial=5)
            many += sum(len(r["accept"]) > 1 for r in rows)
            total += len(rows)
            if hists is not None:
                margin = min(margin, min(TR.timestamp_step_row(x[r], hist, G.NO_TIMESTAMPS + 1, G.NO_TIMESTAMPS, G.EOT, 5)["margin"]
                                         for r in range(SR.RANDOM_ROWS)))
    print(f"random rows: {many} of {total} accept sets hold more than one column; smallest mass margin {margin:.3e}")
    assert many <= 0.01 * total and margin >= 1e-3


def test_generate_near_tie_share():
    """``generate(temperature=0.7, best_of=3, seed=GEN_SEED)`` in float64 on the tiny fixture, with and without the timestamp rules:
    at most an eighth of the steps have a top-two score gap below 2 x 7.76e-2 / T (what the GPU test may excuse a quarter of)."""
    golden = np.load(G.GOLDEN)
    w = {k[2:]: WR.bf16_from_bits(golden[k]) for k in golden.files if k.startswith("w/")}
    enc, enc_lens = WR.bf16_from_bits(golden["enc"]), [int(v) for v in golden["enc_lens"]]
    for timestamps in (False, True):
        prompt, sup, rules = SR.gen_case(golden, timestamps)
        r = SR.generate(w, G.NH, G.LAYERS, enc, prompt, SR.GEN_NEW, G.EOT, G.EOT, SR.GEN_T, DH.step_seed_sequence(SR.GEN_SEED, 1)[0], n=SR.GEN_N,
                        timestamps=rules, suppress=sup, enc_lens=enc_lens)
        gaps = r["gaps"][np.isfinite(r["gaps"])]
        near = int((gaps < SR.GEN_BAR).sum())
        print(f"timestamps={timestamps}: lens {r['lens'].tolist()}, {near} of {gaps.size} steps below {SR.GEN_BAR:.4f}, smallest gap {gaps.min():.3e}")
        assert near <= gaps.size / 8
        if timestamps:
            for row, n in zip(r["tokens"], r["lens"]):
                TR.check_grammar([int(t) for t in row[:n]], G.NO_TIMESTAMPS + 1, G.EOT, G.NO_TIMESTAMPS, 5)
        assert len({tuple(row) for row in r["tokens"][:SR.GEN_N]}) > 1, "the candidates of an audio differ by their row"


def test_sample_call_seed_is_the_engines_sequence():
    from ssak_amd.whisper_seq2seq import sample_call_seed
    for s in (0, 7, 1234, SR.GEN_SEED):
        assert sample_call_seed(s) == DH.step_seed_sequence(s, 1)[0]


# ------------------------------------------------------------------------------------------------------------ decode_with_fallback
class FakeDecoder:
    """``decode_at`` by script: results[(window, temperature)] -> (tokens, avg_logprob, no_speech_prob); records its calls."""

    def __init__(self, results, default=([1, 2, 3], -0.1, 0.0)):
        self.results, self.default, self.calls = results, default, []

    def __call__(self, indices, temperature):
        self.calls.append((list(indices), temperature))
        return [self.results.get((i, temperature), self.default) for i in indices]


TEMPS = (0.0, 0.4, 0.8)
BAD, GOOD = ([1, 2, 3], -2.0, 0.0), ([4, 5], -0.2, 0.0)


def test_fallback_decodes_only_failing_windows_in_order():
    dec = FakeDecoder({(1, 0.0): BAD, (3, 0.0): BAD, (1, 0.4): GOOD, (3, 0.4): BAD, (3, 0.8): BAD})
    out = decode_with_fallback(dec, TEMPS, 4, 2.4, -1.0, 0.6, None)
    print(f"calls {dec.calls}; temperatures {[o[3] for o in out]}")
    assert dec.calls == [([0, 1, 2, 3], 0.0), ([1, 3], 0.4), ([3], 0.8)]
    assert [o[3] for o in out] == [0.0, 0.4, 0.0, 0.8] and out[1][:3] == GOOD
    assert out[3][:3] == BAD, "the last temperature's result stands whatever it is"
    assert all(o[4] == 0.0 for o in out), "text_of=None: no ratio is taken"


def test_fallback_single_temperature_makes_one_call():
    dec = FakeDecoder({(0, 0.0): BAD})
    out = decode_with_fallback(dec, (0.0,), 2, 2.4, -1.0, 0.6, None)
    assert dec.calls == [([0, 1], 0.0)] and out[0][:4] == BAD + (0.0,)
    with pytest.raises(ValueError):
        decode_with_fallback(dec, (), 2, 2.4, -1.0, 0.6, None)


def test_fallback_each_threshold_alone_and_none_is_inert():
    text_of = lambda ids: "".join("ab"[i % 2] for i in ids)
    rep, plain = list(range(200)), [0, 0, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 0]
    r_rep, r_plain = compression_ratio(text_of(rep)), compression_ratio(text_of(plain))
    print(f"compression ratios: repetitive {r_rep:.2f}, plain {r_plain:.2f}")
    assert r_rep > 2.4 > r_plain
    results = {(0, 0.0): (rep, -0.1, 0.0), (1, 0.0): (plain, -0.1, 0.0), (2, 0.0): (plain, -2.0, 0.0)}
    # the compression ratio alone
    dec = FakeDecoder(results)
    out = decode_with_fallback(dec, TEMPS, 3, 2.4, None, None, text_of)
    assert dec.calls[1] == ([0], 0.4) and out[0][3] == 0.4 and out[1][4] == r_plain and out[2][3] == 0.0
    # the log-probability alone
    dec = FakeDecoder(results)
    out = decode_with_fallback(dec, TEMPS, 3, None, -1.0, None, text_of)
    assert dec.calls[1] == ([2], 0.4) and out[0][3] == 0.0 and out[0][4] == r_rep
    # both off: nothing is decoded again; text_of=None switches the ratio off although its threshold is set
    for kw in (dict(compression_ratio_threshold=None, logprob_threshold=None, text_of=text_of),
               dict(compression_ratio_threshold=2.4, logprob_threshold=None, text_of=None)):
        dec = FakeDecoder(results)
        out = decode_with_fallback(dec, TEMPS, 3, no_speech_threshold=0.6, **kw)
        assert len(dec.calls) == 1 and [o[3] for o in out] == [0.0] * 3
    # ids from ts_begin on are not part of the text
    dec = FakeDecoder({(0, 0.0): ([0, 1, 500, 501], -0.1, 0.0)})
    seen = []
    decode_with_fallback(dec, (0.0,), 1, 2.4, -1.0, 0.6, lambda ids: seen.append(ids) or "x", ts_begin=500)
    assert seen == [[0, 1]]


def test_fallback_no_speech_exemption():
    """no_speech_prob above its threshold AND avg_logprob below its threshold: silence, no retry -- also where the text compresses
    too well; with either threshold None the exemption is off."""
    text_of = lambda ids: "a" * len(ids)
    silent = (list(range(300)), -2.0, 0.9)
    for kw, calls in ((dict(logprob_threshold=-1.0, no_speech_threshold=0.6), 1), (dict(logprob_threshold=-1.0, no_speech_threshold=None), 3),
                      (dict(logprob_threshold=None, no_speech_threshold=0.6), 3), (dict(logprob_threshold=-1.0, no_speech_threshold=0.95), 3)):
        dec = FakeDecoder({}, default=silent)
        out = decode_with_fallback(dec, TEMPS, 1, compression_ratio_threshold=2.4, text_of=text_of, **kw)
        print(f"{kw}: {len(dec.calls)} calls, temperature {out[0][3]}")
        assert len(dec.calls) == calls
    dec = FakeDecoder({}, default=(list(range(300)), -0.5, 0.9))  # loud enough: not silence, the ratio drives it on
    decode_with_fallback(dec, TEMPS, 1, 2.4, -1.0, 0.6, text_of)
    assert len(dec.calls) == 3


# ------------------------------------------------------------------------------------------------------------ best_of ranking
def test_best_of_ranking_on_planted_candidates():
    from ssak_amd.whisper_seq2seq import beam_rank
    eos = 100
    cands = [([5, 6, 7, eos], -3.0, True, 0),  # -1.0 per token
             ([5, eos], -0.5, True, 1),        # -0.5 per token: the best average
             ([eos], -0.01, True, 2),          # length 0: -inf, never chosen although its sum is the highest
             ([5, 6, 7, 8], -2.4, False, 3)]   # no eos: 4 tokens, -0.6 per token
    assert beam_rank(cands) == 1
    assert beam_rank(cands[2:]) == 1 and beam_rank(cands[2:3]) == 0
    # length_penalty 1: sum / ((5 + n) / 6): -3 / (8 / 6) = -2.25, -0.5 / 1 = -0.5, -2.4 / 1.5 = -1.6
    assert beam_rank(cands, 1.0) == 1
    assert beam_rank([([5, 6, 7, 8, 9, 9, 9, eos], -2.1, True, 0), ([5, eos], -0.4, True, 1)]) == 0
    assert beam_rank([([5, 6, 7, 8, 9, 9, 9, eos], -2.1, True, 0), ([5, eos], -0.4, True, 1)], 0.0) == 1, "penalty 0 ranks by the sum"


# ------------------------------------------------------------------------------------------------------------ the command line
def test_command_line_temperature_schedule(capsys):
    from ssak_amd.whisper_infer import parse_args, temperature_schedule
    base = ["a.wav", "--model", "dir"]
    a = parse_args(base + ["--timestamps", "--accurate", "--seed", "7"])
    print(f"--accurate: temperatures {a.temperatures}")
    assert (a.beam_size, a.best_of, a.temperature_increment_on_fallback, a.seed) == (5, 5, 0.2, 7)
    assert len(a.temperatures) == 6 and np.allclose(a.temperatures, [0.0, 0.2, 0.4, 0.6, 0.8, 1.0], atol=1e-12)
    assert a.temperatures == tuple(float(t) for t in np.arange(0.0, 1.0 + 1e-6, 0.2))
    a = parse_args(base + ["--timestamps", "--temperature_increment_on_fallback", "0.2"])
    assert len(a.temperatures) == 6 and a.beam_size is None and a.best_of is None
    a = parse_args(base)
    assert a.temperatures == (0.0,) and (a.compression_ratio_threshold, a.logprob_threshold, a.no_speech_threshold, a.seed) == (2.4, -1.0, 0.6, 1234)
    a = parse_args(base + ["--temperature", "0.5", "--best_of", "3"])
    assert a.temperatures == (0.5,) and a.best_of == 3
    a = parse_args(base + ["--timestamps", "--accurate", "--beam_size", "2"])
    assert a.beam_size == 2 and a.best_of == 5, "a later flag overrides --accurate"
    assert temperature_schedule(0.4, 0.3) == tuple(float(t) for t in np.arange(0.4, 1.0 + 1e-6, 0.3))
    for bad in (["--accurate"], ["--temperature_increment_on_fallback", "0.2"], ["--best_of", "9"], ["--temperature", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    capsys.readouterr()
