"""Whisper-small long-form transcription with timestamps on one MI355X (DESIGN.md "Whisper long-form transcription").  Seeded random
weights at whisper-small's shapes (d_model 768, 12 + 12 layers of 12 heads, ffn 3072, 51 865 tokens of which 1501 timestamps from
50 364, 1500 encoder frames); nothing is read from disk.

usage: python tools/bench_whisper_transcribe.py [reps=15] [parts=ab]

(a) ssak_dec_timestamp_step against ssak_dec_greedy_step per launch: B = 32, V = 51 865 in a 51 872-column fp32 buffer, the
    history [timestamp, text] (both of the rules' intervals open, the mass decision taken), eos suppressed so that no row
    finishes (ts_last moves up when launches of a train emit timestamps; every launch reads the same bytes).  A figure is the
    time of one launch inside a train of 48 back-to-back launches between two device events, rotating over 4 logits buffers (6.6 MB each: as in the real loop, where the vocabulary projection has just written them, they are
    cache-resident); median and range over ``reps`` trains after 3 warm-up trains, the two entries' trains alternating in one
    process.  It is one launch among about 90 per token.
(b) ``transcribe`` of 32 files of 90 s of noise, batch_size 32: audio-seconds per second of wall time (median and range over
    max(3, reps // 5) runs after one warm-up run), with the rounds and the sampled tokens counted.  Random weights decode every
    window to its 224-token limit, which a trained model does not: the figure is a floor for the decoder's share.
Prints one JSON line.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TRAIN = 48
V, LDV, EOS, NOTS = 51865, 51872, 50257, 50363
TSB = NOTS + 1


def trains(fns, reps, warmup=3):
    us = {k: [] for k in fns}
    for it in range(warmup + reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3 / TRAIN)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def step_case(hip, reps, B=32, D=768, n_buf=4):
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    bufs = [3 * torch.randn(B, LDV, generator=g, device=dev) for _ in range(n_buf)]
    E = (torch.randn(V + 7, D, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    Pz = (torch.randn(448, D, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    sup = torch.zeros(V, dtype=torch.uint8, device=dev)
    sup[EOS:NOTS] = 1
    tokens = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    tokens[:, 0], tokens[:, 1] = TSB + 10, 500
    lps = torch.zeros((B, 8), dtype=torch.float32, device=dev)
    fin, n_unf = torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ts_last = torch.full((B,), TSB + 10, dtype=torch.int32, device=dev)
    h_next = torch.empty((B, D), dtype=torch.bfloat16, device=dev)
    kw = dict(finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=2, eos_id=EOS, pad_id=EOS, suppress=sup, embed_tokens=E,
              embed_positions=Pz, next_pos=5, h_next=h_next)

    def run_greedy():
        for i in range(TRAIN):
            hip.dec_greedy_step(bufs[i % n_buf], V, **kw)

    def run_ts():
        for i in range(TRAIN):
            hip.dec_timestamp_step(bufs[i % n_buf], V, ts_begin=TSB, no_timestamps_id=NOTS, ts_last=ts_last, max_initial=50, **kw)

    run_ts()
    torch.cuda.synchronize()
    took_ts = int((tokens[:, 2] >= TSB).sum())
    ts_last.fill_(TSB + 10)
    r = trains({"greedy": run_greedy, "timestamp": run_ts}, reps)
    out = {"B": B, "V": V, "rows_that_chose_a_timestamp": took_ts}
    for name, (med, lo, hi) in r.items():
        out[name] = {"median_us": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2)}
    out["timestamp_over_greedy"] = round(r["timestamp"][0] / r["greedy"][0], 3)
    out["ranges_overlap"] = bool(r["timestamp"][1] <= r["greedy"][2] and r["greedy"][1] <= r["timestamp"][2])
    return out


def make_model():
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    cfg = WhisperSeq2SeqConfig(eos_token_id=EOS, pad_token_id=EOS, no_timestamps_token_id=NOTS, suppress_tokens=list(range(EOS + 1, NOTS + 1)),
                               begin_suppress_tokens=[220, EOS])  # whisper-small; no language tokens: the prompt is [<|startoftranscript|>]
    model = WhisperSeq2Seq(cfg)
    g = torch.Generator().manual_seed(0)
    model.dec_params.copy_((torch.randn(model.dec_params.numel(), generator=g) * 0.02).to(model.device))
    for name in model.layout:  # LayerNorm scales around 1
        if name.endswith("layer_norm.weight"):
            model.dec_param(name).fill_(1.0)
    model.sync_decoder_shadow()
    return model


def transcribe_case(model, runs, n_files=32, seconds=90):
    rng = np.random.default_rng(3)
    waves = [torch.from_numpy((0.1 * rng.standard_normal(16000 * seconds)).astype(np.float32)) for _ in range(n_files)]
    count = {"rounds": 0, "tokens": 0, "windows": 0}
    gen = model.generate

    def counting(enc, **kw):
        r = gen(enc, **kw)
        count["rounds"] += 1
        count["windows"] += enc.shape[0]
        count["tokens"] += int(r.lens.sum())
        return r

    model.generate = counting
    try:
        secs = []
        for it in range(1 + runs):
            for k in count:
                count[k] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = model.transcribe(waves, batch_size=n_files)
            torch.cuda.synchronize()
            if it:
                secs.append(time.perf_counter() - t0)
    finally:
        del model.generate
    audio = n_files * seconds
    rate = sorted(audio / s for s in secs)
    return {"files": n_files, "seconds_each": seconds, "runs": runs, "rounds": count["rounds"], "windows": count["windows"],
            "sampled_tokens": count["tokens"], "segments": sum(len(r.segments) for r in res),
            "wall_s_median": round(statistics.median(secs), 3), "audio_s_per_s_median": round(statistics.median(rate), 1),
            "audio_s_per_s_min": round(rate[0], 1), "audio_s_per_s_max": round(rate[-1], 1)}


def main():
    import ssak_amd.hip as hip
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    parts = sys.argv[2] if len(sys.argv) > 2 else "ab"
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    out = {"config": "whisper-small, long-form transcription with timestamps", "reps": reps, "launches_per_train": TRAIN}
    if "a" in parts:
        out["step"] = step_case(hip, reps)
    if "b" in parts:
        out["transcribe"] = transcribe_case(make_model(), max(3, reps // 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
