"""Whisper-small greedy generation on one MI355X (DESIGN.md "Whisper generation").  Seeded random weights at whisper-small's shapes
(d_model 768, 12 decoder layers of 12 heads, ffn 3072, 51 865 tokens, 1500 encoder frames), the encoder output given: nothing is
read from disk.

usage: python tools/bench_whisper_generate.py [reps=15] [parts=abc]

(a) The two attention entries at one query per (utterance, head), on the same buffers, interleaved in one process:
    ssak_dec_attention_step (library-chosen split) and ssak_dec_attention_fwd at Lq = 1; B in {1, 32}, 12 heads, cross n_keys =
    1500, self n_keys in {64, 448} in a 448-row cache.  A figure is the time of one launch inside a train of 48 back-to-back
    launches between two device events (a single launch is a few tens of microseconds: below what an event pair resolves), the
    train rotating over enough k|v buffers that no launch finds its keys in the Infinity Cache where the real loop would not
    (twelve layers' buffers; at B = 32 cross, 4 buffers of 147 MB); median and range over ``reps`` trains after 3 warm-up trains,
    the two entries' trains alternating.  Bytes per second: the k and v rows of the visible keys, once.
(b) ``generate`` end to end at B = 32 and B = 1: 64 new tokens after a 4-token prompt, eos suppressed; ms per token, tokens/s,
    the one-off cost (cross k|v + prefill) and the share of kernel time spent in matrix products (ssak_prof_* kernel time of the products over the step's wall time, a separate run).
(c) What the cache is worth: the only loop possible without it, greedy decoding through ``decode_logits`` on the growing
    sequence, 8 tokens at B = 32, timed once.
Prints one JSON line.
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TRAIN = 48
EOS = 50257


def trains(fns, reps, warmup=3):
    """fns: name -> callable that issues one train of TRAIN launches.  Alternates the callables; -> name -> per-launch microseconds
    (median, min, max) over ``reps`` trains."""
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


def attention_case(hip, B, nh, n_keys, cap, kind, n_buf, reps, g):
    D = nh * 64
    dev = "cuda:0"
    bufs = [(torch.randn(B, cap, 2 * D, generator=g, device=dev) * 0.5).to(torch.bfloat16) for _ in range(n_buf)]
    q = (torch.randn(B, D, generator=g, device=dev) * 0.5).to(torch.bfloat16)
    ctx = torch.empty(B, D, dtype=torch.bfloat16, device=dev)
    ws = hip.dec_attention_step_workspace(B, nh, 0, dev)
    st = hip.stream()
    P, L = hip.ptr, hip.lib
    step_args = [(P(q), D, P(b[:, :, :D]), 2 * D, cap * 2 * D, P(b[:, :, D:]), 2 * D, cap * 2 * D, n_keys, None, B, nh, 64, 0, P(ws), ws.numel() * 4,
                  P(ctx), st) for b in bufs]
    causal, q_off = (1, n_keys - 1) if kind == "self" else (0, 0)
    fwd_args = [(P(q), D, P(b[:, :, :D]), 2 * D, P(b[:, :, D:]), 2 * D, cap, None, None, B, 1, nh, 64, causal, q_off, P(ctx), st) for b in bufs]

    def run_step():
        for i in range(TRAIN):
            hip.check(L.ssak_dec_attention_step(*step_args[i % n_buf]))

    def run_fwd():
        for i in range(TRAIN):
            hip.check(L.ssak_dec_attention_fwd(*fwd_args[i % n_buf]))

    # the two entries agree before either is timed
    run_step()
    a = ctx.float().clone()
    hip.check(L.ssak_dec_attention_fwd(*fwd_args[(TRAIN - 1) % n_buf]))
    torch.cuda.synchronize()
    agree = float((a - ctx.float()).abs().max())
    r = trains({"step": run_step, "fwd": run_fwd}, reps)
    nbytes = B * n_keys * 2 * D * 2
    out = {"B": B, "kind": kind, "n_keys": n_keys, "buffers": n_buf, "max_abs_difference": round(agree, 5)}
    for name, (med, lo, hi) in r.items():
        out[name] = {"median_us": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2), "TB_per_s": round(nbytes / med / 1e6, 3)}
    s, f = r["step"], r["fwd"]
    out["step_wins_beyond_range"] = bool(s[2] < f[1])  # the slowest step train is faster than the fastest fwd train
    out["fwd_over_step"] = round(f[0] / s[0], 2)
    del bufs
    torch.cuda.empty_cache()
    return out


def make_model():
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    cfg = WhisperSeq2SeqConfig(eos_token_id=EOS, pad_token_id=EOS)  # whisper-small
    model = WhisperSeq2Seq(cfg)
    g = torch.Generator().manual_seed(0)
    model.dec_params.copy_((torch.randn(model.dec_params.numel(), generator=g) * 0.02).to(model.device))
    for name in model.layout:  # LayerNorm scales around 1
        if name.endswith("layer_norm.weight"):
            model.dec_param(name).fill_(1.0)
    model.sync_decoder_shadow()
    return model, g


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def generate_case(hip, model, g, B, n_new, reps):
    cfg = model.config
    enc = torch.randn(B, cfg.max_source_positions, cfg.d_model, generator=g).to(torch.bfloat16).to(model.device)
    prompt = np.array([cfg.decoder_start_token_id, 50259, 50359, 50363], dtype=np.int64)
    gen = lambda: model.generate(enc, prompt=prompt, max_new_tokens=n_new, suppress_tokens=[EOS], poll_every=8)

    def once():
        st = model._gen_begin(enc, None, cap=len(prompt) + n_new)
        return model._gen_prefill(st, np.tile(prompt, (B, 1)))

    for _ in range(2):
        r = gen()
        once()
    assert r.steps == n_new and np.isfinite(r.logprobs).all()
    total = [event_ms(gen)[0] for _ in range(reps)]
    oneoff = [event_ms(once)[0] for _ in range(reps)]
    med, off = statistics.median(total), statistics.median(oneoff)
    per_tok = (med - off) / (n_new - 1)  # n_new - 1 token steps follow the prefill (the last selection needs no further step)
    out = {"B": B, "new_tokens": n_new, "total_median_ms": round(med, 2), "total_min_ms": round(min(total), 2), "total_max_ms": round(max(total), 2),
           "one_off_median_ms": round(off, 2), "one_off_min_ms": round(min(oneoff), 2), "one_off_max_ms": round(max(oneoff), 2),
           "ms_per_token_step": round(per_tok, 3), "tokens_per_s": round(B / per_tok * 1e3, 1)}
    # the share of the token step spent in matrix products: ssak_prof_* kernel time of the products (every launch timed: a run of
    # its own) over the step's wall time
    st = model._gen_begin(enc, None, cap=len(prompt) + n_new)
    logits = model._gen_prefill(st, np.tile(prompt, (B, 1)))
    h = torch.zeros(B, cfg.d_model, dtype=torch.bfloat16, device=model.device)
    torch.cuda.synchronize()
    hip.prof_enable(1)
    hip.prof_collect()
    for _ in range(8):
        model._gen_step(st, h)
    torch.cuda.synchronize()
    rows = hip.prof_collect()
    hip.prof_enable(0)
    tot = sum(r[2] for r in rows)
    mm = sum(r[2] for r in rows if "gemm" in r[0])
    out["profiled_kernel_ms_per_step"] = round(tot / 8, 3)
    out["product_ms_per_step"] = round(mm / 8, 3)
    out["product_share_of_token_step"] = round(mm / 8 / per_tok, 3)
    out["profiled_kernels"] = sorted(((r[0], round(r[2] / 8, 4)) for r in rows), key=lambda x: -x[1])[:6]
    return out


def baseline_case(model, g, B, n_new):
    cfg = model.config
    enc = torch.randn(B, cfg.max_source_positions, cfg.d_model, generator=g).to(torch.bfloat16).to(model.device)
    seq = np.tile(np.array([cfg.decoder_start_token_id, 50259, 50359, 50363], dtype=np.int64), (B, 1))

    def loop():
        s = seq
        for _ in range(n_new):
            logits = model.decode_logits(enc, s)[:, -1]
            logits[:, EOS] = float("-inf")
            s = np.concatenate([s, logits.argmax(-1).cpu().numpy()[:, None]], 1)
        return s

    model.decode_logits(enc, seq)  # (warm-up of the first shape)
    ms, _ = event_ms(loop)
    return {"B": B, "new_tokens": n_new, "total_ms_once": round(ms, 1), "ms_per_token": round(ms / n_new, 2)}


def main():
    import ssak_amd.hip as hip
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    parts = sys.argv[2] if len(sys.argv) > 2 else "abc"
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    out = {"config": "whisper-small decoder, generation", "reps": reps, "launches_per_train": TRAIN, "hbm_streaming_TB_per_s": 6.3}
    if "a" in parts:
        g = torch.Generator(device="cuda:0").manual_seed(1)
        out["attention"] = []
        for B in (1, 32):
            for kind, n_keys, cap in (("cross", 1500, 1500), ("self", 64, 448), ("self", 448, 448)):
                n_buf = 4 if (B == 32 and kind == "cross") else 12
                out["attention"].append(attention_case(hip, B, 12, n_keys, cap, kind, n_buf, reps, g))
    if "b" in parts or "c" in parts:
        model, g = make_model()
        if "b" in parts:
            out["generate"] = [generate_case(hip, model, g, B, 64, max(3, reps // 3)) for B in (32, 1)]
        if "c" in parts:
            out["no_cache_baseline"] = baseline_case(model, g, 32, 8)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
