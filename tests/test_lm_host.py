"""CPU: the ARPA loader and host tables of ssak_amd.lm, and the CPU restatement of the LM beam search contract
(tests/lm_beam_ref.py) against the exhaustive objective and against greedy decoding."""
import os

import numpy as np
import pytest

from ssak_amd import synth
from ssak_amd.data import CharTokenizer
from ssak_amd.lm import LN10, NgramLM, label_classes, read_arpa

import lm_beam_ref as R
import lm_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "tests", "golden", "lm_tiny.arpa")


@pytest.fixture(scope="module")
def tiny():
    return NgramLM(TINY, CharTokenizer(synth.VOCAB))


def test_arpa_sections_and_counts(tiny):
    order, counts, sections = read_arpa(TINY)
    assert order == 3 and counts == [33, 22, 8] and tiny.counts == counts
    assert [len(s[0]) for s in sections] == counts
    # "été" / "ça" cannot be spelled with a-z: dropped with every n-gram that uses them ("ça va": "va" is no unigram either)
    assert tiny.skipped == [2, 2, 1]
    assert "été" not in tiny.word_id and "monde" in tiny.word_id and "aujourd'hui" in tiny.word_id


def test_backoff_scores_by_hand(tiny):
    w = tiny.word_id
    p = lambda ctx, x: float(tiny.log10p([w[c] for c in ctx], w[x]))
    assert p(["bonjour", "le"], "monde") == pytest.approx(-0.2)                 # trigram
    assert p(["bonjour", "le"], "chat") == pytest.approx(-0.3 + -1.5)           # bo(bonjour le) + P(chat | le)
    assert p(["bonjour", "le"], "maison") == pytest.approx(-0.3 + -0.6 + -2.7)  # + bo(le) + P(maison)
    assert p(["monde", "il"], "chat") == pytest.approx(-0.3 + -2.6)             # no bo(monde il): bo(il) + P(chat)
    assert p(["<s>"], "bonjour") == pytest.approx(-0.3)
    assert p([], "le") == pytest.approx(-1.1)
    assert p(["le", "monde"], "</s>") == pytest.approx(-0.3)
    # an OOV word scores as <unk>: P(<unk> | le) = bo(le) + P(<unk>)
    assert p(["le"], "<unk>") == pytest.approx(-0.6 + -2.0)
    # only the trailing run of valid ids counts, at most order-1 of them
    assert float(tiny.log10p([-1, w["bonjour"], w["le"]], w["monde"])) == pytest.approx(-0.2)
    assert float(tiny.log10p([w["bonjour"], -1, w["le"]], w["monde"])) == pytest.approx(-0.8)


def test_unk_is_added_when_absent(tmp_path):
    src = open(TINY).read().replace("ngram 1=33", "ngram 1=32").replace("-2.0\t<unk>\n", "")
    (tmp_path / "nounk.arpa").write_text(src)
    lm = NgramLM(str(tmp_path / "nounk.arpa"), CharTokenizer(synth.VOCAB))
    assert lm.words[lm.unk] == "<unk>" and float(lm.uni[lm.unk, 0]) == -100.0


@pytest.mark.parametrize("content, msg", [
    (b"mmap lm http://kheafield.com/code format version 5\n\0\0\0\1", "binary"),
    (b"\x00\x01\x02\x03garbage", "binary"),
    (b"hello world\n", "expected '\\\\data\\\\'"),
    (b"", "empty"),
    (b"\\data\\\nngram 1=2\n\n\\1-grams:\n-1.0\t<s>\n", "end"),
    (b"\\data\\\nngram 1=1\nngram 2=1\n\n\\1-grams:\n-1.0\t<s>\n\n\\3-grams:\n-1 a b c\n\n\\end\\\n", "2-grams"),
    (b"\\data\\\nngram 1=1\n\n\\1-grams:\nx\t<s>\n\n\\end\\\n", "1-gram line"),
    (b"\\data\\\n" + b"".join(b"ngram %d=0\n" % k for k in range(1, 8)), "order 7"),
])
def test_malformed_and_binary_files_are_rejected(tmp_path, content, msg):
    path = tmp_path / "bad.arpa"
    path.write_bytes(content)
    with pytest.raises(ValueError, match=msg):
        NgramLM(str(path), CharTokenizer(synth.VOCAB))


@pytest.mark.parametrize("max_load", [0.5, 0.97])
def test_host_tables_find_every_ngram_and_prefix(tmp_path, max_load):
    """Every n-gram and every unigram prefix is found by the device's probing, within the table's bound; absent keys
    terminate; at a 0.97 load factor the probe chains are long (collisions exercised)."""
    rng = np.random.default_rng(3)
    words = synth.synth_words(rng, 600)
    synth.write_arpa(str(tmp_path / "g.arpa"), words, [3000, 3000], seed=4)
    tok = CharTokenizer(synth.VOCAB)
    lm = NgramLM(str(tmp_path / "g.arpa"), tok, max_load=max_load)
    _, _, sections = read_arpa(str(tmp_path / "g.arpa"))
    longest = 0
    for k in (2, 3):
        cap = len(lm.ng_keys[k - 2])
        for t, p, b in zip(*sections[k - 1]):
            hit, probes = lm.probe_ngram([lm.word_id[x] for x in t])
            assert hit is not None and hit[0] == p and hit[1] == b and probes <= cap
            longest = max(longest, probes)
        miss, probes = lm.probe_ngram([lm.word_id["<s>"]] * k)
        assert miss is None and probes <= cap
    for w in words:
        node = 0
        for ch in w:
            node, probes = lm.probe_trie(node, tok.index[ch])
            assert node > 0 and probes <= len(lm.trie)
        assert lm.words[lm.node_word[node]] == w
    assert lm.probe_trie(0, tok.index["|"])[0] == -1
    if max_load > 0.9:
        assert longest > 8


def _ab_setup(tmp_path, seed):
    vocab = ["<pad>", "|", "a", "b"]
    tok = CharTokenizer(vocab)
    rng = np.random.default_rng(seed)
    words = ["a", "b", "ab", "ba", "aa", "bab"]
    synth.write_arpa(str(tmp_path / f"ab{seed}.arpa"), words, [20, 20], seed=seed)
    lm = NgramLM(str(tmp_path / f"ab{seed}.arpa"), tok)
    return tok, label_classes(tok), lm, rng


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_exhaustive_search(tmp_path, seed):
    """Pruning off and a beam holding every (prefix, last): the restatement returns argmax_y [log P_ctc(y|x) + LM(y)]."""
    tok, cls, lm, rng = _ab_setup(tmp_path, seed)
    T = int(rng.integers(1, 7))
    logits = (rng.standard_normal((T, 4)) * 2).astype(np.float32)
    alpha, beta = (0.5, 1.0) if seed % 2 == 0 else (1.3, -0.4)
    ids, score = R.beam_decode(logits, T, lm, cls, 0, alpha, beta, beam_width=100000, beam_prune_logp=-np.inf,
                               token_min_logp=-np.inf)
    want, best = R.exhaustive(logits, T, lm, cls, 0, alpha, beta)
    assert ids == want or R.objective(logits, T, ids, lm, cls, 0, alpha, beta) >= best - 1e-5 * abs(best)
    assert score == pytest.approx(best, rel=1e-5, abs=1e-5)


@pytest.mark.parametrize("seed", range(4))
def test_restatement_width_one_without_lm_is_greedy(tmp_path, seed):
    tok = CharTokenizer(synth.VOCAB)
    lm = NgramLM(TINY, tok)
    rng = np.random.default_rng(seed)
    T = int(rng.integers(1, 60))
    logits = (rng.standard_normal((T, len(tok))) * 4).astype(np.float32)
    logits[:, 0] += 2.0  # some blanks, so that repeats survive collapse
    ids, _ = R.beam_decode(logits, T, lm, label_classes(tok), tok.pad_token_id, alpha=0.0, beta=0.0, beam_width=1)
    assert ids == R.greedy(logits, T, tok.pad_token_id)


def test_lm_term_prefers_the_lm_word(tiny):
    """The contract's LM score of a label sequence: 'bonjour le monde' beats 'bonjour le mode' by the LM alone."""
    tok = CharTokenizer(synth.VOCAB)
    sc = R.Scorer(tiny, label_classes(tok), 0.5, 1.0, -10.0)
    good = sc.final(sc.of_labels(tok.encode("bonjour le monde")))
    bad = sc.final(sc.of_labels(tok.encode("bonjour le mode")))
    assert good > bad
    want = 0.5 * float(LN10) * (-0.3 - 0.1 - 0.2 - 0.3) + 3 * 1.0  # P(bonjour|<s>) P(le|<s> bonjour) P(monde|..) P(</s>|le monde)
    assert float(good) == pytest.approx(want, rel=1e-6)


# ------------------------------------------------------------------------------------------------- the shared case table
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["name"])
def test_case_float32_restatement_agrees_with_float64(tmp_path, case, record_property):
    """Every case of tests/lm_cases.py (the GPU tests decode the same): the float32 and float64 restatements return the same
    transcript and scores within 1e-4; margin, fp32 noise and the decisive flag are those the table records (the margin is
    float64 arithmetic: 1 %; the noise depends on the host's float32 exp / log: a factor of 2); one run takes < 3 s."""
    b = C.build(case, tmp_path)
    runs = [C.analyse(b, u) for u in range(len(b.x))]
    for u, a in enumerate(runs):
        print(f"{case['name']} u{u}: margin {a['margin']:.3e} noise {a['noise']:.3e} ratio {a['margin'] / max(a['noise'], 1e-30):.0f} "
              f"decisive {a['decisive']} kept {a['max_kept']} tie cutoffs {a['tie_cutoffs']} seconds {a['seconds'][0]:.2f} {a['seconds'][1]:.2f}")
        assert a["ids32"] == a["ids"] and a["split"] is None
        assert a["score32"] == pytest.approx(a["score"], rel=1e-4)
        assert max(a["seconds"]) < 3.0
    w = C.worst(runs)
    record_property("margin", w["margin"])
    record_property("noise", w["noise"])
    record_property("decisive", w["decisive"])
    margin, noise, decisive = C.table_row(case["name"])
    assert all(a["decisive"] for a in runs) == case["decisive"] == decisive
    assert w["margin"] == pytest.approx(margin, rel=1e-2) and noise / 2 <= w["noise"] <= noise * 2
    if case["kind"] == "width":
        assert w["max_kept"] == case["W"]  # the beam fills
    if b.ties:
        assert w["tie_cutoffs"] >= 1  # a tied group straddles the cutoff
        wrong, _ = R.beam_decode(b.x[0], b.lens[0], b.lm, b.cls, b.blank, dtype=np.float64, ties=True, tie_sign=-1, **b.kw)
        assert wrong != w["ids"]  # and the opposite tie rule would show in the transcript


def test_case_table_covers_the_edges():
    by = C.BY_NAME
    assert {by[n]["n_labels"] for n in by if n.startswith("strip")} == {5, 64, 65, 256, 257, 300, 1024}
    assert {by[n]["W"] for n in by if n.startswith("width")} == {2, 63, 64, 65, 255, 256}
    assert [by[n]["W"] * by[n]["n_labels"] for n in ("keys4096", "keys4097", "keys9600")] == [4096, 4097, 9600]
    assert sum(not c["decisive"] for c in C.CASES) <= 3
    assert all(c["decisive"] for c in C.CASES if c["name"] not in ("long", "keys4096", "keys4097", "keys9600"))


def test_long_context_changes_the_transcript(tmp_path):
    """The order-6 LM and the same file cut to its bigrams decode the same acoustics differently (one word)."""
    b6, b2 = C.build(C.BY_NAME["order6"], tmp_path), C.build(C.BY_NAME["order2t"], tmp_path)
    assert np.array_equal(b6.x, b2.x) and b6.lm.order == 6 and b2.lm.order == 2
    assert np.array_equal(b6.lm.uni, b2.lm.uni) and np.array_equal(b6.lm.ng_val[0], b2.lm.ng_val[0])
    t6 = b6.tok.decode(C.analyse(b6)["ids"], group_tokens=False).split()
    t2 = b2.tok.decode(C.analyse(b2)["ids"], group_tokens=False).split()
    assert len(t6) == len(t2) >= 10 and sum(x != y for x, y in zip(t6, t2)) == 1
