"""Whisper-small sampling on one MI355X (DESIGN.md "Whisper sampling and temperature fallback").  Seeded random weights at
whisper-small's shapes (d_model 768, 12 decoder layers of 12 heads, ffn 3072, 51 865 tokens, 1500 encoder frames), the encoder output
given; nothing is read from disk.

usage: python tools/bench_whisper_sample.py [reps=9] [parts=ab]

(a) per launch at 40 rows, V = 51 865 in a 51 872-column fp32 buffer, history ``[ts, text]``: ssak_dec_sample_step (T = 0.2, with the
    timestamp rules and without) against ssak_dec_timestamp_step and ssak_dec_greedy_step, the same buffers, in the same run.  A
    figure is the time of one launch inside a train of 48 launches that rotate over 4 logits buffers, between two device events;
    median and range over ``reps`` trains after 2 warm-up trains, the entries alternating in one process.
(b) ms per token step, 8 audios x ``best_of`` = 5 at T = 0.2 (``_gen_step`` at 40 rows with the grouped cross-attention, then
    ssak_dec_sample_step) against 8 audios x 5 beams (``_beam_step``) and against greedy at 40 rows (ssak_dec_greedy_step): the same
    row count, trains of 32 consecutive steps (cache rows 4 .. 36 in use), as tools/bench_whisper_beam.py times them.  eos is
    suppressed, so nothing finishes.
Prints one JSON line.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_whisper_beam import B_AUDIO, EOS, LDV, NB, NOTS, P, ROWS, TSB, V, make_model, trains  # noqa: E402

TEMPERATURE, SEED = 0.2, 1234


def launch_case(hip, reps, train=48, D=768, n_buf=4):
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    bufs = [3 * torch.randn(ROWS, LDV, generator=g, device=dev) for _ in range(n_buf)]
    E = (torch.randn(V + 7, D, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    Pz = (torch.randn(448, D, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    sup = torch.zeros(V, dtype=torch.uint8, device=dev)
    sup[EOS:NOTS] = 1  # eos among them: nothing finishes
    ldt, t = 448, 2
    tokens = torch.full((ROWS, ldt), 500, dtype=torch.int32, device=dev)
    tokens[:, 0] = TSB + 10
    lps = torch.zeros((ROWS, ldt), dtype=torch.float32, device=dev)
    ts_last = torch.full((ROWS,), TSB + 10, dtype=torch.int32, device=dev)
    fin, n_unf = torch.zeros(ROWS, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    h_next = torch.empty((ROWS, D), dtype=torch.bfloat16, device=dev)
    kw = dict(finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=t, eos_id=EOS, pad_id=EOS, suppress=sup, embed_tokens=E,
              embed_positions=Pz, next_pos=P + t, h_next=h_next)
    rules = dict(ts_begin=TSB, no_timestamps_id=NOTS, max_initial=50, ts_last=ts_last)

    def loop(step, **more):
        def run():
            for i in range(train):
                step(bufs[i % n_buf], V, **kw, **more)
        return run

    fns = {"greedy_step": loop(hip.dec_greedy_step), "timestamp_step": loop(hip.dec_timestamp_step, **rules),
           "sample_step": loop(hip.dec_sample_step, temperature=TEMPERATURE, seed=SEED),
           "sample_step_with_rules": loop(hip.dec_sample_step, temperature=TEMPERATURE, seed=SEED, **rules)}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = trains(fns, reps, train)
    out["sample_with_rules_over_timestamp"] = round(out["sample_step_with_rules"]["median_us"] / out["timestamp_step"]["median_us"], 3)
    out["sample_over_greedy"] = round(out["sample_step"]["median_us"] / out["greedy_step"]["median_us"], 3)
    out["rows"], out["launches_per_train"] = ROWS, train
    return out


def step_case(model, hip, reps, steps=32):
    dev = model.device
    g = torch.Generator(device=dev).manual_seed(1)
    enc = torch.randn((ROWS, 1500, 768), generator=g, device=dev).to(torch.bfloat16)
    sup = model._token_mask(list(range(EOS, NOTS + 1)), "suppress")
    prompt = np.tile(np.array([[50258, 50259, 50359, NOTS]], dtype=np.int64), (ROWS, 1))
    E, Pz = model._w("embed_tokens.weight"), model._w("embed_positions.weight")
    cap = P + steps + 1
    tokens = torch.zeros((ROWS, steps + 1), dtype=torch.int32, device=dev)
    lps = torch.zeros((ROWS, steps + 1), dtype=torch.float32, device=dev)
    fin, n_unf = torch.zeros(ROWS, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    h_next = torch.empty((ROWS, 768), dtype=torch.bfloat16, device=dev)
    kw = dict(finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, eos_id=EOS, pad_id=EOS, suppress=sup, embed_tokens=E,
              embed_positions=Pz, h_next=h_next)
    # greedy at 40 utterances
    sg = model._gen_begin(enc, cap=cap)
    lg0 = model._gen_prefill(sg, prompt).clone()

    def run_greedy():
        sg.t = P
        logits = lg0
        for i in range(steps):
            hip.dec_greedy_step(logits, V, t=i, first=i == 0, next_pos=P + i, **kw)
            logits = model._gen_step(sg, h_next)

    # 8 audios x best_of 5: the grouped cross-attention, every row its own cache
    ss = model._gen_begin(enc[:B_AUDIO], cap=cap, group=NB)
    ls0 = model._gen_prefill(ss, prompt[:B_AUDIO]).repeat_interleave(NB, dim=0)

    def run_sample():
        ss.t = P
        logits = ls0
        for i in range(steps):
            hip.dec_sample_step(logits, V, t=i, first=i == 0, next_pos=P + i, temperature=TEMPERATURE, seed=SEED, **kw)
            logits = model._gen_step(ss, h_next)

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

    out = trains({"greedy_40_rows": run_greedy, "sample_8x5": run_sample, "beam_8x5": run_beam}, reps, steps)
    out["sample_over_greedy"] = round(out["sample_8x5"]["median_us"] / out["greedy_40_rows"]["median_us"], 3)
    out["sample_over_beam"] = round(out["sample_8x5"]["median_us"] / out["beam_8x5"]["median_us"], 3)
    out["steps_per_train"] = steps
    out["distinct_tokens_in_the_last_sampled_step"] = int(tokens[:, steps - 1].unique().numel())
    return out


def main():
    import ssak_amd.hip as hip
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    parts = sys.argv[2] if len(sys.argv) > 2 else "ab"
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    out = {"config": f"whisper-small, sampling at T = {TEMPERATURE}, {B_AUDIO} audios x best_of {NB} = {ROWS} rows", "reps": reps}
    if "a" in parts:
        out["per_launch"] = launch_case(hip, reps)
    if "b" in parts:
        out["token_step"] = step_case(make_model(), hip, reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
