"""GPU: CTC beam search with an ARPA n-gram LM (ssak_ctc_lm_beam_decode / ssak_lm_query, ssak_amd.lm) against the host
tables, greedy decoding, the exhaustive objective and the CPU restatement (tests/lm_beam_ref.py); determinism, argument
checks, and ``python -m ssak_amd.infer --arpa`` end to end."""
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


def _peaked(rng, text, conf=0.3, F=None):
    """Posteriors of a label sequence: each label held 1-2 frames then blank, a confusable second label in some frames."""
    labs = TOK.encode(text)
    rows = []
    for l in labs:
        for _ in range(int(rng.integers(1, 3))):
            r = rng.standard_normal(len(TOK)).astype(np.float32) * 0.5
            r[l] += 9.0
            if rng.random() < conf:
                r[int(rng.integers(5, 31))] += 7.5
            rows.append(r)
        r = rng.standard_normal(len(TOK)).astype(np.float32) * 0.5
        r[BLANK] += 8.0
        rows.append(r)
    x = np.stack(rows)
    if F is not None:
        x = np.concatenate([x, np.zeros((F - len(x), len(TOK)), np.float32)])
    return x


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


def test_exhaustive_objective_small(tmp_path):
    """T = 4, labels {blank, |, a, b}, beam 256 (holds every (prefix, last)), pruning off: the exhaustive argmax."""
    from ssak_amd import lm as L
    tok = CharTokenizer(["<pad>", "|", "a", "b"])
    cls = label_classes(tok)
    synth.write_arpa(str(tmp_path / "ab.arpa"), ["a", "b", "ab", "ba", "aa", "bab"], [20, 20], seed=2)
    lm = NgramLM(str(tmp_path / "ab.arpa"), tok).to("cuda:0")
    rng = np.random.default_rng(2)
    B, T = 6, 4
    x = (rng.standard_normal((B, T, 4)) * 2).astype(np.float32)
    ids, n, score = L.decode(torch.from_numpy(x).cuda(), torch.full((B,), T, dtype=torch.int32), lm, tok, alpha=0.7, beta=0.5,
                             beam_width=256, beam_prune_logp=-np.inf, token_min_logp=-np.inf)
    ids, n, score = ids.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy()
    for b in range(B):
        want, best = R.exhaustive(x[b], T, lm, cls, 0, 0.7, 0.5)
        got = list(ids[b, :n[b]])
        assert got == want or R.objective(x[b], T, got, lm, cls, 0, 0.7, 0.5) >= best - 1e-5 * abs(best), (b, got, want)
        assert float(score[b]) == pytest.approx(best, rel=1e-4, abs=1e-4)


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
