"""CPU: the two float64 forms of whisper's beam-search update in tests/whisper_beam_ref.py -- the literal dict keyed by sequence and
the array form the kernels implement -- give the same next tokens, sources, sums and finished lists, in order, on seeded cases with
exact ties; full loops on a scripted table-driven decoder agree through finalisation and ranking."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import whisper_beam_ref as BR  # noqa: E402

EOS, PAD = 3, 0
NBS = (1, 2, 3, 5, 8)
CASES_PER_NB = 420  # 5 x 420 = 2 100 seeded single-step cases


def _row(rng, V, quantise):
    x = rng.standard_normal(V) * 2.0
    return np.round(x * 2) / 2 if quantise else x


@pytest.mark.parametrize("nb", NBS)
def test_update_forms_agree(nb):
    rng = np.random.default_rng(100 + nb)
    seen = dict(eos_in_topk=0, ties=0, first=0, stored=0, ran_out=0, became_done=0)
    for case in range(CASES_PER_NB):
        V = int(rng.integers(12, 41))
        quantise = case % 3 == 0
        first = case % 5 == 0
        n_hist = 0 if first else int(rng.integers(1, 6))
        if first:  # whisper's first step: identical prefixes and rows, sums [0, -inf, ...]
            hist = [[] for _ in range(nb)]
            sums = [0.0] + [-np.inf] * (nb - 1)
            row = _row(rng, V, quantise)
            rows = np.stack([row] * nb)
        else:
            hist = [[int(t) for t in rng.integers(4, V, n_hist)] + [j + V] for j in range(nb)]  # (distinct prefixes, as a search keeps them)
            sums = list(np.round(rng.standard_normal(nb) * 3, 1) if quantise else rng.standard_normal(nb) * 3)
            for j in range(nb):
                if rng.random() < 0.15:
                    sums[j] = -np.inf
            rows = np.stack([_row(rng, V, quantise) for _ in range(nb)])
        if rng.random() < 0.2:  # rows with fewer than K allowed columns
            keep = int(rng.integers(1, nb + 1))
            rows[:, keep:] = -np.inf
        lps = BR.log_softmax(rows)
        n_prev = int(rng.integers(0, nb))
        prev = [([7, 8, k, EOS], -1.0 - k) for k in range(n_prev)]
        fin_d = {tuple(t): s for t, s in prev}
        fin_a = list(prev)
        nxt, src_d, sums_d, completed = BR.update_dict(hist, sums, lps, nb, EOS, fin_d)
        cands = [BR.topk_stable(lps[j], nb + 1) for j in range(nb)]
        tok_a, src_a, sums_a, lp_a, done = BR.update_array(hist, sums, cands, nb, EOS, PAD, fin_a, False)
        live = [i for i in range(nb) if sums_a[i] > -np.inf]
        assert [tok_a[i] for i in live] == [s[-1] for s in nxt] and [src_a[i] for i in live] == src_d
        assert [sums_a[i] for i in live] == sums_d and len(live) == len(nxt)
        assert all(tok_a[i] == PAD and src_a[i] == i for i in range(len(live), nb))
        assert [(tuple(t), s) for t, s in fin_a] == list(fin_d.items()) and done == completed
        for i in live:  # the per-token log-prob is the candidate's own
            assert lp_a[i] == dict(cands[src_a[i]])[tok_a[i]]
        seen["eos_in_topk"] += any(EOS in dict(c) for c in cands)
        flat = [sums[j] + lp for j in range(nb) if sums[j] > -np.inf for _, lp in cands[j]]
        seen["ties"] += len(set(flat)) < len(flat)
        seen["first"] += first
        seen["stored"] += len(fin_a) > n_prev
        seen["ran_out"] += len(live) < nb
        seen["became_done"] += done
    print(f"nb={nb}: {CASES_PER_NB} cases, {seen}")
    assert seen["eos_in_topk"] > 20 and seen["first"] > 50 and seen["stored"] > 10 and seen["ran_out"] > 5  # (the cases do reach the branches)
    assert seen["ties"] > 20 or nb == 1


def test_whispers_own_first_step():
    """Sums all 0 and identical prefixes -- whisper's literal first step, where its dict keeps one copy of each sequence -- against the
    [0, -inf, ...] start of the array form: the same tokens and sums."""
    rng = np.random.default_rng(7)
    for nb in NBS:
        for _ in range(40):
            V = int(rng.integers(12, 41))
            row = _row(rng, V, True)
            lps = BR.log_softmax(np.stack([row] * nb))
            fin_d, fin_a = {}, []
            nxt, _, sums_d, _ = BR.update_dict([[] for _ in range(nb)], [0.0] * nb, lps, nb, EOS, fin_d)
            cands = [BR.topk_stable(lps[j], nb + 1) for j in range(nb)]
            tok, src, sums_a, _, _ = BR.update_array([[] for _ in range(nb)], [0.0] + [-np.inf] * (nb - 1), cands, nb, EOS, PAD, fin_a, False)
            n = len(nxt)
            assert tok[:n] == [s[-1] for s in nxt] and sums_a[:n] == sums_d and src[:n] == [0] * n
            assert [(tuple(t), s) for t, s in fin_a] == list(fin_d.items())


def _scripted(seed, V, quantise, eos_bias):
    """A table-driven decoder: the log-softmax row is a fixed function of the prefix (a table filled on first use)."""
    table = {}

    def fn(prefix):
        key = tuple(prefix)
        if key not in table:
            rng = np.random.default_rng([seed, len(key)] + [int(t) for t in key])
            x = _row(rng, V, quantise)
            x[EOS] += eos_bias * len(key)
            table[key] = BR.log_softmax(x)
        return table[key]
    return fn


@pytest.mark.parametrize("length_penalty", [None, 0.6, 1.0])
@pytest.mark.parametrize("nb", NBS)
def test_full_loops_agree(nb, length_penalty):
    """Each audio alone through whisper's loop against the lock-step batch of the array form (done audios frozen): the same
    candidates in the same order and the same winner.  eos grows likelier with the prefix, so audios finish at different steps."""
    fns = [_scripted(10 * nb + a, 14 + 3 * a, a % 2 == 0, 0.5 + 0.25 * a) for a in range(6)]
    max_new = 9
    batch, steps = BR.search_array(fns, nb, EOS, PAD, max_new, length_penalty)
    n_fin = 0
    for a, fn in enumerate(fns):
        cands, w = BR.search_dict(fn, nb, EOS, max_new, length_penalty)
        assert batch[a][0] == cands and batch[a][1] == w, a
        n_fin += sum(c[2] for c in cands)
    assert n_fin > 0 and steps <= max_new


def test_length_zero_and_penalty():
    cands = [([EOS], -0.1, True), ([5, 6, EOS], -2.0, True), ([5, 6, 7, 8], -3.0, False)]
    assert BR.rank(cands) == 2  # -inf, -1.0, -0.75
    assert BR.rank(cands, 1.0) == 1  # -inf, -2 / (7 / 6) = -1.714, -3 / (9 / 6) = -2.0
    assert BR.rank(cands, 3.0) == 2  # -2 / (7 / 6) ** 3 = -1.259, -3 / 1.5 ** 3 = -0.889
    assert BR.rank([([EOS], -0.1, True), ([EOS], -0.2, True)]) == 0  # all -inf: np.argmax takes the lowest index
    assert BR.rank([([4, EOS], -1.0, True), ([9], -1.0, False)]) == 0  # a tie goes to the lowest index


@pytest.mark.parametrize("seed", range(8))
def test_beam_one_is_the_argmax_loop(seed):
    fn = _scripted(seed, 20, seed % 2 == 0, 0.4)
    want = BR.greedy(fn, EOS, 12)
    (cands, w), = BR.search_array([fn], 1, EOS, PAD, 12)[0]
    assert w == 0 and (cands[0][0], cands[0][1]) == want
