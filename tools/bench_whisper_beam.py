"""Whisper-small beam search on one MI355X (DESIGN.md "Whisper beam search").  Seeded random weights at whisper-small's shapes (d_model
768, 12 decoder layers of 12 heads, ffn 3072, 51 865 tokens, 1500 encoder frames), the encoder output given; nothing is read from disk.

usage: python tools/bench_whisper_beam.py [reps=9] [parts=ab]

(a) ms per token step, 8 audios x 5 beams (``_gen_step`` at 40 rows with the grouped cross-attention, then ``_beam_step``: top-K,
    select, cache reorder) against greedy at 40 rows (``_gen_step`` at 40 utterances, then ``ssak_dec_greedy_step``): the same row
    count.  A figure is the time of one step inside a train of 32 consecutive steps (cache rows 4 .. 36 in use) between two device
    events; median and range over ``reps`` trains after 2 warm-up trains, the two sides alternating in one process.  eos is
    suppressed, so nothing finishes.
(b) per-launch times of ssak_dec_beam_topk, ssak_dec_beam_select and ssak_dec_kv_reorder at 40 rows with 64 and 224 cache rows
    in use (trains of 48 launches, as tools/bench_whisper_transcribe.py times its entries): the top-K rotates over 4 logits buffers,
    the reorder runs a full cycle of sources (every beam moves) over [4, rows), its bytes read + written per second.
Prints one JSON line.
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, LDV, EOS, NOTS = 51865, 51872, 50257, 50363
TSB = NOTS + 1
B_AUDIO, NB, P = 8, 5, 4
ROWS = B_AUDIO * NB


def trains(fns, reps, per_train, warmup=2):
    us = {k: [] for k in fns}
    for it in range(warmup + reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3 / per_train)
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in us.items()}


def make_model():
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    cfg = WhisperSeq2SeqConfig(eos_token_id=EOS, pad_token_id=EOS, no_timestamps_token_id=NOTS)
    model = WhisperSeq2Seq(cfg)
    g = torch.Generator().manual_seed(0)
    model.dec_params.copy_((torch.randn(model.dec_params.numel(), generator=g) * 0.02).to(model.device))
    for name in model.layout:  # LayerNorm scales around 1
        if name.endswith("layer_norm.weight"):
            model.dec_param(name).fill_(1.0)
    model.sync_decoder_shadow()
    return model


def step_case(model, hip, reps, steps=32):
    dev = model.device
    g = torch.Generator(device=dev).manual_seed(1)
    enc = torch.randn((ROWS, 1500, 768), generator=g, device=dev).to(torch.bfloat16)
    sup = model._token_mask(list(range(EOS, NOTS + 1)), "suppress")
    prompt = np.tile(np.array([[50258, 50259, 50359, NOTS]], dtype=np.int64), (ROWS, 1))
    E, Pz = model._w("embed_tokens.weight"), model._w("embed_positions.weight")
    cap = P + steps + 1
    # greedy at 40 utterances
    sg = model._gen_begin(enc, cap=cap)
    lg0 = model._gen_prefill(sg, prompt).clone()
    tokens = torch.zeros((ROWS, steps + 1), dtype=torch.int32, device=dev)
    lps = torch.zeros((ROWS, steps + 1), dtype=torch.float32, device=dev)
    fin, n_unf = torch.zeros(ROWS, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    h_next = torch.empty((ROWS, 768), dtype=torch.bfloat16, device=dev)

    def run_greedy():
        sg.t = P
        logits = lg0
        for i in range(steps):
            hip.dec_greedy_step(logits, V, finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=i, eos_id=EOS, pad_id=EOS, suppress=sup,
                                first=i == 0, embed_tokens=E, embed_positions=Pz, next_pos=P + i, h_next=h_next)
            logits = model._gen_step(sg, h_next)

    # 8 audios x 5 beams
    sb = model._gen_begin(enc[:B_AUDIO], cap=cap, group=NB)
    lb0 = model._gen_prefill(sb, prompt[:B_AUDIO]).repeat_interleave(NB, dim=0)
    bs = model._beam_begin(sb, P, steps + 1, EOS, EOS, sup, None, None)

    def run_beam():
        sb.t, bs.i = P, 0
        bs.sums.fill_(float("-inf"))
        bs.sums[:, 0] = 0.0
        logits = lb0
        for i in range(steps):
            model._beam_step(sb, bs, logits)
            logits = model._gen_step(sb, bs.h_next)

    out = trains({"greedy_40_rows": run_greedy, "beam_8x5": run_beam}, reps, steps)
    out["beam_over_greedy"] = round(out["beam_8x5"]["median_us"] / out["greedy_40_rows"]["median_us"], 3)
    out["steps_per_train"] = steps
    out["live_beams_at_the_end"] = int((bs.sums > float("-inf")).sum())
    return out


def kernel_case(hip, reps, rows_in_use, train=48, layers=12, D=768, n_buf=4):
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    bufs = [3 * torch.randn(ROWS, LDV, generator=g, device=dev) for _ in range(n_buf)]
    E = (torch.randn(V + 7, D, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    Pz = (torch.randn(448, D, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    sup = torch.zeros(V, dtype=torch.uint8, device=dev)
    sup[EOS:NOTS] = 1  # eos among them: nothing finishes
    t = rows_in_use - P  # history entries per beam
    ldt = 448
    tokens = torch.randint(0, 50000, (ROWS, ldt), generator=g, device=dev).to(torch.int32)
    tokens[:, t - 2] = TSB + 10
    lps = torch.zeros((ROWS, ldt), dtype=torch.float32, device=dev)
    ts_last = torch.full((ROWS,), TSB + 10, dtype=torch.int32, device=dev)
    done = torch.zeros(B_AUDIO, dtype=torch.uint8, device=dev)
    ct = torch.zeros((ROWS, NB + 1), dtype=torch.int32, device=dev)
    cl = torch.zeros((ROWS, NB + 1), dtype=torch.float32, device=dev)
    sums = torch.zeros((B_AUDIO, NB), dtype=torch.float32, device=dev)
    src = torch.zeros(ROWS, dtype=torch.int32, device=dev)
    fin_t, fin_l = torch.zeros((B_AUDIO, NB, ldt), dtype=torch.int32, device=dev), torch.zeros((B_AUDIO, NB, ldt), dtype=torch.float32, device=dev)
    fin_n, fin_s = torch.zeros((B_AUDIO, NB), dtype=torch.int32, device=dev), torch.zeros((B_AUDIO, NB), dtype=torch.float32, device=dev)
    n_fin, n_unf = torch.zeros(B_AUDIO, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    h_next = torch.empty((ROWS, D), dtype=torch.bfloat16, device=dev)
    cache = torch.randn((layers, ROWS, 448, 2 * D), generator=g, device=dev).to(torch.bfloat16)
    cycle = torch.tensor([b * NB + (j + 1) % NB for b in range(B_AUDIO) for j in range(NB)], dtype=torch.int32, device=dev)

    def run_topk():
        for i in range(train):
            hip.dec_beam_topk(bufs[i % n_buf], V, NB, done=done, cand_token=ct, cand_logprob=cl, eos_id=EOS, t=t, suppress=sup, timestamps=True,
                              ts_begin=TSB, no_timestamps_id=NOTS, max_initial=50, tokens=tokens, ts_last=ts_last)

    def run_select():
        for i in range(train):
            hip.dec_beam_select(ct, cl, NB, V, sum_logprob=sums, src=src, tokens=tokens, logprobs=lps, t=t, fin_tokens=fin_t, fin_logprobs=fin_l,
                                fin_len=fin_n, fin_sum=fin_s, n_fin=n_fin, done=done, n_unfinished=n_unf, eos_id=EOS, pad_id=EOS, ts_last=ts_last,
                                ts_begin=TSB, embed_tokens=E, embed_positions=Pz, next_pos=rows_in_use, h_next=h_next)

    def run_reorder():
        for i in range(train):
            hip.dec_kv_reorder(cache, cycle, NB, P, rows_in_use)

    run_topk()
    torch.cuda.synchronize()
    out = trains({"topk": run_topk, "select": run_select, "kv_reorder": run_reorder}, reps, train)
    moved = 2 * layers * ROWS * (rows_in_use - P) * 2 * D * 2  # bytes read + written by one reorder
    out["kv_reorder"]["bytes_read_plus_written"] = moved
    out["kv_reorder"]["GB_per_s_median"] = round(moved / out["kv_reorder"]["median_us"] / 1e3, 1)
    out["n_finished_after"] = int(n_fin.sum())
    return out


def main():
    import ssak_amd.hip as hip
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    parts = sys.argv[2] if len(sys.argv) > 2 else "ab"
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    out = {"config": f"whisper-small, beam search, {B_AUDIO} audios x {NB} beams = {ROWS} rows", "reps": reps}
    if "a" in parts:
        out["token_step"] = step_case(make_model(), hip, reps)
    if "b" in parts:
        out["kernels"] = {f"{n}_rows_in_use": kernel_case(hip, reps, n) for n in (64, 224)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
