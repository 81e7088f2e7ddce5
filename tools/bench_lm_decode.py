"""CTC beam search with an ARPA n-gram LM on the device (ssak_amd.lm.decode): ms per batch of 32 x 10 s (499 frames, V = 32).

LM: a seeded synthetic 3-gram ARPA (about 50 k unigrams, 1 M n-grams in all; ssak_amd.synth.write_arpa) written to a
temporary directory; its load + upload time is reported.  Two logit workloads:
  peaked -- posteriors of LM-sampled transcripts (each label 1-2 frames then a blank frame, a confusable second label in 30 %
            of the label frames): |S_t| is 1-3, what a trained model gives;
  flat   -- N(0, 1) logits, every token in S_t: the worst case (an untrained model).
Timed with device events after warm-up.  The CPU restatement (tests/lm_beam_ref.py, not pyctcdecode) is timed on one
peaked utterance as context only.

    python tools/bench_lm_decode.py [--beam 100] [--iters 20]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ssak_amd import lm as L  # noqa: E402
from ssak_amd import synth  # noqa: E402
from ssak_amd.data import CharTokenizer  # noqa: E402


def peaked_logits(rng, lm, tok, B, F):
    V = len(tok)
    p = 10.0 ** lm.uni[:, 0].astype(np.float64)
    spellable = np.array([i for i, w in enumerate(lm.words) if not w.startswith("<")])
    p = p[spellable] / p[spellable].sum()
    x = np.empty((B, F, V), np.float32)
    for b in range(B):
        rows = []
        while len(rows) < F:
            w = lm.words[spellable[rng.choice(len(spellable), p=p)]]
            for l in tok.encode(w + " "):
                for _ in range(int(rng.integers(1, 3))):
                    r = rng.standard_normal(V).astype(np.float32) * 0.5
                    r[l] += 9.0
                    if rng.random() < 0.3:
                        r[int(rng.integers(5, 31))] += 7.5
                    rows.append(r)
                r = rng.standard_normal(V).astype(np.float32) * 0.5
                r[tok.pad_token_id] += 8.0
                rows.append(r)
        x[b] = np.stack(rows[:F])
    return x


def time_decode(x, lens, lm, tok, beam, iters, warmup=3):
    for _ in range(warmup):
        L.decode(x, lens, lm, tok, beam_width=beam)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        L.decode(x, lens, lm, tok, beam_width=beam)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beam", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=499)
    ap.add_argument("--unigrams", type=int, default=50000)
    ap.add_argument("--ngrams", type=int, default=950000, help="bigrams + trigrams")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement's timing")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lm_decode needs the GPU"
    rng = np.random.default_rng(0)
    tok = CharTokenizer(synth.VOCAB)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "lm.arpa")
        t = time.perf_counter()
        synth.write_arpa(path, synth.synth_words(rng, a.unigrams), [a.ngrams // 2, a.ngrams - a.ngrams // 2], seed=1)
        t_gen = time.perf_counter() - t
        t = time.perf_counter()
        lm = L.load_arpa(path, tok, "cuda:0")
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t
    B, F = a.batch, a.frames
    lens = torch.full((B,), F, dtype=torch.int32)
    out = dict(tool="bench_lm_decode", B=B, F=F, V=len(tok), beam=a.beam, lm_counts=lm.counts, lm_skipped=lm.skipped,
               lm_table_mb=round(lm.nbytes() / 2**20, 1), arpa_generate_s=round(t_gen, 2), arpa_load_upload_s=round(t_load, 2))
    xp = peaked_logits(rng, lm, tok, B, F)
    xf = rng.standard_normal((B, F, len(tok))).astype(np.float32)
    for name, x in (("peaked", xp), ("flat", xf)):
        xd = torch.from_numpy(x).cuda()
        ms = time_decode(xd, lens, lm, tok, a.beam, a.iters)
        out[f"{name}_ms_per_batch"] = round(ms, 3)
        out[f"{name}_utt_per_s"] = round(B / ms * 1e3, 1)
    if not a.no_cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import lm_beam_ref as R
        t = time.perf_counter()
        R.beam_decode(xp[0], F, lm, L.label_classes(tok), tok.pad_token_id, 0.5, 1.0, beam_width=a.beam)
        out["cpu_restatement_peaked_s_per_utt"] = round(time.perf_counter() - t, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
