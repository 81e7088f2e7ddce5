"""GPU: CTC beam search with an ARPA n-gram LM (ssak_ctc_lm_beam_decode / ssak_lm_query, ssak_amd.lm) against the host
tables, greedy decoding, the exhaustive objective and the CPU restatement (tests/lm_beam_ref.py); the case table of
tests/lm_cases.py (vocabulary strips, extra columns, candidate key storage, beam widths, exact ties, LM orders, a long
utterance, -inf logits) against the float64 restatement; determinism, argument checks, and
``python -m ssak_amd.infer --arpa`` end to end."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ssak_amd import synth
from ssak_amd.data import CharTokenizer
from ssak_amd.lm import NgramLM, label_classes

import lm_beam_ref as R
import lm_cases as C
from lm_cases import peaked as _peaked

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "tests", "golden", "lm_tiny.arpa")
TOK = CharTokenizer(synth.VOCAB)
BLANK = TOK.pad_token_id


@pytest.fixture(scope="module")
def tiny():
    return NgramLM(TINY, TOK).to("cuda:0")


def _decode(logits, lens, lm, **kw):
    from ssak_amd import lm as L
    ids, n, score = L.decode(torch.from_numpy(np.ascontiguousarray(logits)).cuda(), torch.tensor(lens, dtype=torch.int32),
                             lm, TOK, **kw)
    torch.cuda.synchronize()
    ids, n, score = ids.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy()
    assert (n >= 0).all()
    return [list(ids[b, :n[b]]) for b in range(len(n))], score, ids


SENTENCES = ["bonjour le monde", "il est un petit chat", "merci bien", "dans la maison", "le chien et le chat",
             "bonjour la maison", "zorglub le monde", "tout grand"]


def test_lm_query_matches_host_tables(tmp_path):
    """100 k random (context, word) queries on a generated 3-gram LM built at load factor 0.97 (long collision chains):
    device and host read the same slots and add the same fp32 values in the same order -> equal bit for bit."""
    from ssak_amd import hip
    rng = np.random.default_rng(0)
    words = synth.synth_words(rng, 3000)
    synth.write_arpa(str(tmp_path / "q.arpa"), words, [20000, 20000], seed=1)
    lm = NgramLM(str(tmp_path / "q.arpa"), TOK, max_load=0.97).to("cuda:0")
    Q = 100_000
    nw = len(lm.words)
    ctx = rng.integers(0, nw, (Q, 2)).astype(np.int32)
    w = rng.integers(0, nw, Q).astype(np.int32)
    # a third of the queries along stored n-grams (hits at every order), some with a missing older word
    k2, k3 = lm.ng_keys
    tri = k3[k3[:, 0] >= 0]
    sel = rng.integers(0, len(tri), Q // 3)
    ctx[:Q // 3], w[:Q // 3] = tri[sel, :2], tri[sel, 2]
    ctx[Q // 3:Q // 3 + 5000, 0] = -1
    got = hip.lm_query(lm.desc, torch.from_numpy(ctx).cuda(), torch.from_numpy(w).cuda()).cpu().numpy()
    want = np.array([lm.log10p(list(ctx[q]), int(w[q])) for q in range(Q)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_width_one_without_lm_equals_greedy(tiny):
    from ssak_amd import hip
    rng = np.random.default_rng(1)
    B, F = 33, 80
    x = (rng.standard_normal((B, F, len(TOK))) * 4).astype(np.float32)
    x[:, :, BLANK] += 2.0
    lens = rng.integers(2, F + 1, B)
    lens[0], lens[1], lens[2] = 0, 1, F
    got, _, ids = _decode(x, lens, tiny, alpha=0.0, beta=0.0, beam_width=1)
    g_ids, g_n = hip.ctc_greedy_decode(torch.from_numpy(x).cuda(), torch.tensor(lens, dtype=torch.int32).cuda(), BLANK)
    g_ids, g_n = g_ids.cpu().numpy(), g_n.cpu().numpy()
    assert np.array_equal(ids, g_ids)
    assert [len(g) for g in got] == list(g_n) and got[0] == [] and len(got[1]) <= 1


def _exhaustive_objective(tmp_path, order):
    from ssak_amd import lm as L
    tok = CharTokenizer(["<pad>", "|", "a", "b", "<s>"])
    cls = label_classes(tok)
    synth.write_arpa(str(tmp_path / "ab.arpa"), ["a", "b", "ab", "ba", "aa", "bab"], [20] * (order - 1), seed=2)
    lm = NgramLM(str(tmp_path / "ab.arpa"), tok).to("cuda:0")
    assert lm.order == order
    rng = np.random.default_rng(2)
    B, T = 6, 5
    x = (rng.standard_normal((B, T, 5)) * 2).astype(np.float32)
    ids, n, score = L.decode(torch.from_numpy(x).cuda(), torch.full((B,), T, dtype=torch.int32), lm, tok, alpha=0.7, beta=0.5,
                             beam_width=256, beam_prune_logp=-np.inf, token_min_logp=-np.inf)
    ids, n, score = ids.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy()
    for b in range(B):
        want, best = R.exhaustive(x[b], T, lm, cls, 0, 0.7, 0.5)
        got = list(ids[b, :n[b]])
        assert got == want or R.objective(x[b], T, got, lm, cls, 0, 0.7, 0.5) >= best - 1e-5 * abs(best), (b, got, want)
        assert float(score[b]) == pytest.approx(best, rel=1e-4, abs=1e-4)


def test_exhaustive_objective_small(tmp_path):
    """T = 5, labels {blank, |, a, b, <s> (a label without text)}, beam 256, pruning off: the exhaustive argmax.  (The beam
    no longer holds every (prefix, last) in the last frame; what it drops is far below the winner.)"""
    _exhaustive_objective(tmp_path, 3)


@pytest.mark.parametrize("order", [1, 6])
def test_exhaustive_objective_small_other_orders(tmp_path, order):
    """The same with a unigram LM (no context, no n-gram table) and with an order-6 LM (all five context slots)."""
    _exhaustive_objective(tmp_path, order)


@pytest.mark.parametrize("W", [1, 8, 100, 256])
def test_matches_restatement_on_peaked_posteriors(tiny, W):
    rng = np.random.default_rng(10 + W)
    xs = [_peaked(rng, s) for s in SENTENCES]
    F = max(len(x) for x in xs)
    x = np.stack([np.concatenate([a, np.zeros((F - len(a), len(TOK)), np.float32)]) for a in xs])
    lens = [len(a) for a in xs]
    got, score, _ = _decode(x, lens, tiny, alpha=0.5, beta=1.0, beam_width=W)
    cls = label_classes(TOK)
    for b in range(len(xs)):
        want, ws = R.beam_decode(x[b], lens[b], tiny, cls, BLANK, 0.5, 1.0, beam_width=W)
        assert got[b] == want, (b, TOK.decode(got[b], group_tokens=False), TOK.decode(want, group_tokens=False))
        assert float(score[b]) == pytest.approx(ws, rel=1e-4)


def test_matches_restatement_on_flat_logits(tiny):
    """Flat logits (S_t = the whole vocabulary): near-ties at the cutoff may resolve differently on ulp differences, so the
    scores agree to 1e-3 and a different transcript must be as good under the exact objective."""
    rng = np.random.default_rng(5)
    B, F, W = 4, 24, 16
    x = rng.standard_normal((B, F, len(TOK))).astype(np.float32)
    got, score, _ = _decode(x, [F] * B, tiny, alpha=0.5, beta=1.0, beam_width=W)
    cls = label_classes(TOK)
    for b in range(B):
        want, ws = R.beam_decode(x[b], F, tiny, cls, BLANK, 0.5, 1.0, beam_width=W)
        assert float(score[b]) == pytest.approx(ws, rel=1e-3)
        if got[b] != want:
            og = R.objective(x[b], F, got[b], tiny, cls, BLANK, 0.5, 1.0)
            ow = R.objective(x[b], F, want, tiny, cls, BLANK, 0.5, 1.0)
            assert og == pytest.approx(ow, rel=1e-3)


def test_lm_changes_the_transcript(tiny):
    """Acoustics prefer 'bonjour le mode' (the frame of 'n' is more blank than 'n'); the LM prefers 'monde'."""
    rows = []
    for ch in "bonjour le monde":
        r = np.zeros(len(TOK), np.float32)
        if ch == "n" and rows and len(rows) > 20:
            r[BLANK], r[TOK.index["n"]] = 5.0, 3.5
        else:
            r[TOK.encode(ch)[0]] = 8.0
        rows.append(r)
        r = np.zeros(len(TOK), np.float32)
        r[BLANK] = 8.0
        rows.append(r)
    x = np.stack(rows)[None]
    got0, _, _ = _decode(x, [x.shape[1]], tiny, alpha=0.0, beta=1.0)
    got5, _, _ = _decode(x, [x.shape[1]], tiny, alpha=0.5, beta=1.0)
    assert TOK.decode(got0[0], group_tokens=False) == "bonjour le mode"
    assert TOK.decode(got5[0], group_tokens=False) == "bonjour le monde"


def test_deterministic_and_batch_independent(tiny):
    rng = np.random.default_rng(7)
    xs = [_peaked(rng, s, conf=0.6) for s in SENTENCES] + [rng.standard_normal((30, len(TOK))).astype(np.float32)]
    F = max(len(a) for a in xs)
    x = np.stack([np.concatenate([a, rng.standard_normal((F - len(a), len(TOK))).astype(np.float32)]) for a in xs])
    lens = [len(a) for a in xs]
    g1, s1, i1 = _decode(x, lens, tiny, beam_width=64)
    g2, s2, i2 = _decode(x, lens, tiny, beam_width=64)
    assert np.array_equal(i1, i2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    for b in range(len(xs)):
        ga, sa, _ = _decode(np.ascontiguousarray(x[b:b + 1, :lens[b]]), [lens[b]], tiny, beam_width=64)
        assert ga[0] == g1[b] and sa.view(np.uint32)[0] == s1.view(np.uint32)[b]


def test_bad_arguments_are_rejected(tiny):
    from ssak_amd import hip
    x = torch.zeros((2, 5, len(TOK)), device="cuda:0")
    cls = torch.from_numpy(label_classes(TOK)).cuda()
    kw = dict(n_labels=len(TOK), blank=BLANK, label_class=cls, alpha=0.5, beta=1.0, beam_width=8, beam_prune_logp=-10.0,
              token_min_logp=-5.0, unk_score_offset=-10.0)
    with pytest.raises(ValueError, match="beam_width"):
        hip.ctc_lm_beam_decode(x, None, tiny.desc, **dict(kw, beam_width=257))
    big = torch.zeros((1, 3, 1025), device="cuda:0")
    with pytest.raises(ValueError, match="n_labels"):
        hip.ctc_lm_beam_decode(big, None, tiny.desc, **dict(kw, n_labels=1025,
                                                            label_class=torch.zeros(1025, dtype=torch.uint8, device="cuda:0")))
    need = hip.lib.ssak_ctc_lm_beam_workspace_bytes(2, 5, len(TOK), 8)
    small = torch.empty(need - 8, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="workspace"):
        hip.ctc_lm_beam_decode(x, None, tiny.desc, workspace=small, **kw)
    ids, n, _ = hip.ctc_lm_beam_decode(x, None, tiny.desc, workspace=torch.empty(need, dtype=torch.uint8, device="cuda:0"), **kw)
    torch.cuda.synchronize()
    assert (n.cpu() >= 0).all()


def test_infer_cli_with_arpa(tmp_path):
    """python -m ssak_amd.infer DATA --model DIR --arpa lm.arpa --use_ids with an untrained model (flat posteriors): one
    line per utterance, equal to ssak_amd.lm.decode over transformers_compute_logits of the same batches; a file that is
    not ARPA text fails with the loader's message."""
    from oracle import w2v2_ref as R2
    from ssak_amd import data as D
    from ssak_amd import lm as L
    from ssak_amd.checkpoint import save_pretrained
    from ssak_amd.config import Wav2Vec2Config
    from ssak_amd.infer import transformers_compute_logits, transformers_load_model
    from ssak_amd.model import Wav2Vec2ForCTC
    rng = np.random.default_rng(0)
    kd = tmp_path / "kaldi"
    (kd / "audio").mkdir(parents=True)
    with open(kd / "wav.scp", "w") as fw, open(kd / "text", "w") as ft, open(kd / "utt2dur", "w") as fd:
        for i in range(5):
            n = int(rng.integers(12000, 24000))
            D.write_wav(str(kd / "audio" / f"u{i}.wav"), synth.synth_wave(rng, n))
            fw.write(f"utt{i} {kd}/audio/u{i}.wav\n")
            ft.write(f"utt{i} {synth.synth_text(rng, 3, 6)}\n")
            fd.write(f"utt{i} {n / 16000:.3f}\n")
    oc = dataclasses.replace(R2.W2V2Config.tiny(), layerdrop=0.0)
    d = dataclasses.asdict(oc)
    d.pop("initializer_range")
    model = Wav2Vec2ForCTC(Wav2Vec2Config(**d))
    model.load_state_dict(R2.init_params(oc, 1))
    save_pretrained(model, CharTokenizer(synth.VOCAB), str(tmp_path / "model"))
    del model
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "ssak_amd.infer", str(kd), "--model", str(tmp_path / "model"), "--use_ids", "--batch_size", "3"]
    r = subprocess.run(cmd + ["--arpa", TINY], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 5 and [l.split(" ")[0] for l in lines] == [f"utt{i}" for i in range(5)]
    model, tok = transformers_load_model(str(tmp_path / "model"))
    lm = L.load_arpa(TINY, tok, model.device)
    want = []
    for batch in D.to_audio_batches([str(kd)], batch_size=3, output_ids=True):
        logits = transformers_compute_logits(model, tok, [a for a, _ in batch]).to(model.device).contiguous()
        lens = torch.tensor([model.num_frames(len(a)) for a, _ in batch], dtype=torch.int32)
        ids, n, _ = L.decode(logits, lens, lm, tok)
        ids, n = ids.cpu().numpy(), n.cpu().numpy()
        want += [" ".join((k, tok.decode(ids[i, :n[i]], group_tokens=False))) for i, (_, k) in enumerate(batch)]
    assert lines == want
    (tmp_path / "bin.arpa").write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\0\0\0\1")
    r = subprocess.run(cmd + ["--arpa", str(tmp_path / "bin.arpa")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "not an ARPA text file" in r.stderr


# ------------------------------------------------------------------------------------------------- the case table (tests/lm_cases.py)
_REF = {}


def _reference(built):
    """The float64 / float32 analysis of a case's utterances, computed once per case."""
    name = built.case["name"]
    if name not in _REF:
        _REF[name] = [C.analyse(built, u) for u in range(len(built.x))]
    return _REF[name]


def _decode_case(built, x=None, lens=None, workspace=None):
    """-> (ids [B, F], n [B], score [B]) numpy, through hip.ctc_lm_beam_decode as ssak_amd.lm.decode calls it."""
    from ssak_amd import hip
    x = built.x if x is None else x
    lens = built.lens if lens is None else lens
    lm = built.lm.to("cuda:0") if built.lm.device is None else built.lm
    cls = torch.from_numpy(built.cls).cuda()
    ids, n, score = hip.ctc_lm_beam_decode(torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.tensor(lens, dtype=torch.int32),
                                           lm.desc, n_labels=len(built.tok), blank=built.blank, label_class=cls,
                                           unk_score_offset=-10.0, workspace=workspace, **built.kw)
    torch.cuda.synchronize()
    ids, n, score = ids.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy()
    assert (n >= 0).all()
    return ids, n, score


def _check_case(built, ids, n, score):
    """A decisive case: the float64 restatement's transcript exactly, its score to 1e-4.  Otherwise the equivalence check
    of test_matches_restatement_on_flat_logits: score to 1e-3, a different transcript as good under the exact objective."""
    case = built.case
    for u, a in enumerate(_reference(built)):
        got = [int(v) for v in ids[u, :n[u]]]
        print(f"LMCASE {case['name']} u{u}: margin {a['margin']:.3e} noise {a['noise']:.3e} decisive {a['decisive']} "
              f"|device - f64| {abs(float(score[u]) - a['score']):.3e} = {abs(float(score[u]) - a['score']) / a['noise']:.2f} x noise, "
              f"same transcript {got == a['ids']}")
        assert a["decisive"] == case["decisive"]
        if case["decisive"]:
            assert got == a["ids"], (case["name"], u, got, a["ids"])
            assert float(score[u]) == pytest.approx(a["score"], rel=1e-4)
        else:
            assert float(score[u]) == pytest.approx(a["score"], rel=1e-3)
            if got != a["ids"]:
                args = (built.lm, built.cls, built.blank, built.kw["alpha"], built.kw["beta"])
                og = R.objective(built.x[u], built.lens[u], got, *args)
                ow = R.objective(built.x[u], built.lens[u], a["ids"], *args)
                assert og == pytest.approx(ow, rel=1e-3)


def _names(prefix):
    return [c["name"] for c in C.CASES if c["name"].startswith(prefix)]


@pytest.mark.parametrize("name", _names("strip"))
def test_label_strips(tmp_path, name):
    """5 .. 1024 labels: the log-softmax, argmax and S_t compaction over one to four strips of 256 labels (strip1024_all:
    token_min_logp = -inf, so S_t is all 1024 labels and fills across the four strips)."""
    built = C.build(C.BY_NAME[name], tmp_path)
    _check_case(built, *_decode_case(built))


@pytest.mark.parametrize("name", _names("extra"))
def test_extra_columns_are_not_read(tmp_path, name):
    """n_labels < V with +50 in the surplus columns: the same bits as the run on the first n_labels columns alone."""
    built = C.build(C.BY_NAME[name], tmp_path)
    NL = built.case["n_labels"]
    assert built.x.shape[2] > NL and (built.x[:, :, NL:] == 50.0).all()
    ids, n, score = _decode_case(built)
    ids2, n2, score2 = _decode_case(built, x=built.x[:, :, :NL])
    assert np.array_equal(ids, ids2) and np.array_equal(n, n2) and np.array_equal(score.view(np.uint32), score2.view(np.uint32))
    _check_case(built, ids, n, score)


@pytest.mark.parametrize("name", _names("keys"))
def test_candidate_key_storage(tmp_path, name):
    """W * n_labels = 4096 (keys in LDS), 4097 and 9600 (keys in the workspace), pruning off so that every beam x label is
    a candidate; the workspace is exactly ssak_ctc_lm_beam_workspace_bytes() bytes inside a larger buffer whose bytes in
    front of it and behind it must stay as they were."""
    from ssak_amd import hip
    built = C.build(C.BY_NAME[name], tmp_path)
    B, F, V = built.x.shape
    need = hip.lib.ssak_ctc_lm_beam_workspace_bytes(B, F, V, built.case["W"])
    guard = 4096
    big = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ws = big[guard:guard + need]
    assert ws.numel() == need and ws.data_ptr() % 256 == 0
    ids, n, score = _decode_case(built, workspace=ws)
    big = big.cpu().numpy()
    assert (big[:guard] == 0xA5).all() and (big[guard + need:] == 0xA5).all()
    assert (big[guard:guard + need] != 0xA5).any()
    assert _reference(built)[0]["max_kept"] == built.case["W"]
    _check_case(built, ids, n, score)


@pytest.mark.parametrize("name", _names("width"))
def test_beam_width_edges(tmp_path, name):
    """W = 2, 63, 64, 65, 255, 256 on peaked posteriors: the beam fills (asserted on the restatement), so tid < take, the
    rank-by-count sort and the scans run at and across the wave boundaries."""
    built = C.build(C.BY_NAME[name], tmp_path)
    assert _reference(built)[0]["max_kept"] == built.case["W"]
    _check_case(built, *_decode_case(built))


@pytest.mark.parametrize("name", _names("tie"))
def test_exact_ties_go_to_the_smaller_index(tmp_path, name):
    """Every non-blank label has the same logit in a frame and most labels begin no LM word, so whole groups of candidates
    have bit-identical totals in any arithmetic and a group straddles the cutoff (asserted on the restatement): the
    survivors are the lowest enumeration indices, hence the restatement's transcript (tie*_empty: two labels without text
    with identical columns)."""
    built = C.build(C.BY_NAME[name], tmp_path)
    x = built.x[0]
    assert all(len({float(v) for i, v in enumerate(row) if i != built.blank}) == 1 for row in x)
    assert _reference(built)[0]["tie_cutoffs"] >= 1
    _check_case(built, *_decode_case(built))


@pytest.mark.parametrize("name", ["order1", "order2", "order3", "order6"])
def test_lm_orders(tmp_path, name):
    """Orders 1 (no context), 2, 3 and 6 (SSAK_LM_MAX_ORDER: all five context slots) on a ten-word sentence, one word OOV."""
    built = C.build(C.BY_NAME[name], tmp_path)
    assert built.lm.order == built.case["order"]
    ids, n, score = _decode_case(built)
    text = built.tok.decode(ids[0, :n[0]], group_tokens=False).split()
    assert len(text) >= 10 and sum(w not in built.lm.word_id for w in text) >= 1
    _check_case(built, ids, n, score)


def test_long_context_changes_the_transcript(tmp_path):
    """The order-6 LM and the same file cut to its bigrams, same acoustics: one word differs, by the long context alone."""
    out = []
    for name in ("order6", "order2t"):
        built = C.build(C.BY_NAME[name], tmp_path)
        ids, n, score = _decode_case(built)
        _check_case(built, ids, n, score)
        out.append(built.tok.decode(ids[0, :n[0]], group_tokens=False).split())
    assert len(out[0]) == len(out[1]) and sum(a != b for a, b in zip(*out)) == 1


@pytest.mark.parametrize("order", [1, 2, 6])
def test_lm_query_other_orders(tmp_path, order):
    """ssak_lm_query at orders 1 (null context), 2 and 6 against NgramLM.log10p, bit for bit; ids >= n_words give NaN."""
    from ssak_amd import hip
    rng = np.random.default_rng(order)
    words = synth.synth_words(rng, 500)
    synth.write_arpa(str(tmp_path / "q.arpa"), words, [4000] * (order - 1), seed=order)
    lm = NgramLM(str(tmp_path / "q.arpa"), TOK, max_load=0.97).to("cuda:0")
    assert lm.order == order
    Q, nw, nc = 20_000, len(lm.words), order - 1
    ctx = rng.integers(0, nw, (Q, nc)).astype(np.int32)
    w = rng.integers(0, nw, Q).astype(np.int32)
    if order > 1:  # a third along stored n-grams of the highest order, some with missing older words
        top = lm.ng_keys[-1]
        top = top[top[:, 0] >= 0]
        sel = rng.integers(0, len(top), Q // 3)
        ctx[:Q // 3], w[:Q // 3] = top[sel, :nc], top[sel, nc]
        for q in range(Q // 3, Q // 3 + 3000):
            ctx[q, :int(rng.integers(1, nc + 1))] = -1
    bad = np.arange(Q - 200, Q)
    w[bad[:100]] = nw + rng.integers(0, 5, 100)
    if order > 1:
        ctx[bad[100:], rng.integers(0, nc, 100)] = nw + rng.integers(0, 5, 100)
    else:
        w[bad[100:]] = nw
    got = hip.lm_query(lm.desc, torch.from_numpy(ctx).cuda() if order > 1 else None, torch.from_numpy(w).cuda()).cpu().numpy()
    assert np.isnan(got[bad]).all()
    good = np.arange(Q - 200)
    want = np.array([lm.log10p(list(ctx[q]), int(w[q])) for q in good], dtype=np.float32)
    assert np.array_equal(got[good].view(np.uint32), want.view(np.uint32))


def test_long_utterance(tmp_path):
    """F = 1500, W = 16, lengths (1500, 1371): the node store 1 + F * W, the prefix hash as it grows, transcripts of ~600
    labels and their read-back; n is the winner's depth, ids[n:] = -1, and the result is that of the utterance alone."""
    built = C.build(C.BY_NAME["long"], tmp_path)
    ids, n, score = _decode_case(built)
    _check_case(built, ids, n, score)
    for u, L in enumerate(built.lens):
        assert 400 < n[u] <= L and (ids[u, :n[u]] >= 0).all() and (ids[u, n[u]:] == -1).all()
        if built.case["decisive"]:
            assert n[u] == len(_reference(built)[u]["ids"])
    i1, n1, s1 = _decode_case(built, x=built.x[1:2, :built.lens[1]], lens=[built.lens[1]])
    assert n1[0] == n[1] and np.array_equal(i1[0, :n1[0]], ids[1, :n[1]]) and (i1[0, n1[0]:] == -1).all()
    assert s1.view(np.uint32)[0] == score.view(np.uint32)[1]


def test_masked_columns(tmp_path):
    """-inf logits: a third of the non-blank columns in every frame (lp = the floor ln 1e-15), all but the blank in one."""
    built = C.build(C.BY_NAME["masked"], tmp_path)
    x = built.x[0]
    assert np.isneginf(x).sum(axis=1).min() >= 10 and np.isneginf(x).sum(axis=1).max() == x.shape[1] - 1
    _check_case(built, *_decode_case(built))
