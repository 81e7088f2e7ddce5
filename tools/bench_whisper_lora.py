"""Whisper-small LoRA fine-tuning on one MI355X next to full fine-tuning, in one process: the train step of ssak_amd/whisper_train.py
(``forward_train(features, labels)``, ``backward()``, ``WhisperAdamW.step()``) three ways on the same seeded weights -- every
parameter, the decoder only (``freeze_encoder``), and the reference's LoRA adapters (r 32, lora_alpha 64, lora_dropout 0.05 on the
decoder's q_proj / v_proj; B nonzero) on the frozen bf16 base.  The LoRA step does a strict subset of the base's work, so it must
not be slower than either; how much faster it is gets reported.  Nothing is read from disk.

usage: python tools/bench_whisper_lora.py [B=32] [L=64,448] [reps=5]

Per (B, L): medians over ``reps`` of device-event time after 2 warm-up steps, and the LoRA step taken apart (encoder forward,
decoder forward, backward, optimizer).  Per launch: ``ssak_lora_fwd``, ``ssak_lora_bwd_input`` (accumulating into dx) and
``ssak_lora_bwd_weights`` at M = B L and M = B S (the cross v_proj's rows), each next to a device copy that moves the bytes the
kernel must move.  Prints one JSON line per (B, L) and one for the kernels.
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def stats(t):
    return {"median": round(t[0], 2), "min": round(t[1], 2), "max": round(t[2], 2)}


def lora_phases(model, opt, feats, labels, reps):
    names = ("encoder_forward", "decoder_forward", "backward", "optimizer")
    acc = {n: [] for n in names}
    for it in range(reps + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        hidden = model.encode(feats)
        ev[1].record()
        model.forward_train(hidden, labels)
        ev[2].record()
        model.backward()
        ev[3].record()
        opt.step()
        ev[4].record()
        ev[4].synchronize()
        if it >= 2:
            for i, n in enumerate(names):
                acc[n].append(ev[i].elapsed_time(ev[i + 1]))
    return {n: round(statistics.median(v), 3) for n, v in acc.items()}


def kernel_rows(Ms, reps, D=768, r=32, p=0.05):
    from ssak_amd import hip
    dev = "cuda:0"
    g = torch.Generator().manual_seed(1)
    bf = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(torch.bfloat16).to(dev)

    def copy_us(nbytes):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        return round(timed(lambda: dst.copy_(src), reps * 4)[0] * 1e3, 1)

    out = {}
    A, B = bf(r, D), bf(D, r)
    for M in Ms:
        x, y3, dy3, dx = bf(M, D), bf(M, 3 * D), bf(M, 3 * D), bf(M, D)
        y, dy = y3[:, 2 * D:], dy3[:, 2 * D:]  # the v block of a packed q|k|v product
        t, dt = torch.empty((M, r), dtype=torch.bfloat16, device=dev), torch.empty((M, r), dtype=torch.bfloat16, device=dev)
        dA, dB = torch.empty((r, D), device=dev), torch.empty((D, r), device=dev)
        ws = hip._ws(hip.lib.ssak_lora_bwd_weights_workspace_bytes(M, D, D, r), dev)
        rows = {
            "lora_fwd": (lambda: hip.lora_fwd(x, A, B, y, 2.0, t=t, seed=1, site=hip.LORA_SITE_BASE, drop_p=p), 2 * M * (3 * D + r)),
            "lora_bwd_input": (lambda: hip.lora_bwd_input(dy, A, B, dt, 2.0, dx=dx, accumulate=True, seed=1, site=hip.LORA_SITE_BASE, drop_p=p),
                               2 * M * (3 * D + r)),
            "lora_bwd_weights": (lambda: hip.lora_bwd_weights(dy, t, dt, x, dA, dB, 2.0, seed=1, site=hip.LORA_SITE_BASE, drop_p=p, workspace=ws),
                                 2 * M * (2 * D + 2 * r) + 2 * ws.numel()),
        }
        for name, (fn, nbytes) in rows.items():
            med, lo, hi = timed(fn, reps * 4)
            out[f"{name}_M{M}"] = {"median_us": round(med * 1e3, 1), "min_us": round(lo * 1e3, 1), "max_us": round(hi * 1e3, 1), "bytes": nbytes,
                                   "gbytes_per_s": round(nbytes / med / 1e6, 1), "copy_same_bytes_us": copy_us(nbytes)}
    return out


def main():
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    from ssak_amd.whisper_train import TRAIN_ROW_CHUNK, WhisperAdamW
    Bs = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "32").split(",")]
    Ls = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "64,448").split(",")]
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    cfg = WhisperSeq2SeqConfig(pad_token_id=50257, eos_token_id=50257)  # whisper-small
    model = WhisperSeq2Seq(cfg)
    model.row_chunk = TRAIN_ROW_CHUNK
    g = torch.Generator().manual_seed(0)
    model.dec_params.copy_((torch.randn(model.dec_params.numel(), generator=g) * 0.02).to(model.device))
    for name in model.layout:
        if name.endswith("layer_norm.weight"):
            model.dec_param(name).fill_(1.0)
        if name.endswith("k_proj.bias"):
            model.dec_param(name).zero_()
    model.sync_decoder_shadow()
    enc = model.encoder
    enc.params.copy_((torch.randn(enc.params.numel(), generator=g) * 0.02).to(model.device))
    for name in enc.layout:
        if name.endswith("layer_norm.weight"):
            enc.param(name).fill_(1.0)
    enc.sync_weights(full=True)
    batches = [(B, L, torch.randn(B, cfg.num_mel_bins, 2 * cfg.max_source_positions, generator=g).to(model.device),
                torch.randint(0, 50257, (B, L), generator=g).numpy()) for B in Bs for L in Ls]
    results = {(B, L): {} for B, L, _, _ in batches}

    def run(key, opt):
        for B, L, feats, labels in batches:
            def step():
                model.forward_train(feats, labels)
                model.backward()
                opt.step()
            torch.cuda.reset_peak_memory_stats()
            results[(B, L)][key] = dict(step_ms=stats(timed(step, reps)), peak_memory_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))

    # the full steps first, on lr = 0 so that the LoRA step sees the same base; then their gradient buffer and moments go
    for key, freeze in (("full", False), ("full_freeze_encoder", True)):
        model.freeze_encoder = freeze
        opt = WhisperAdamW(model, lr=0.0, weight_decay=0.0, warmup_steps=0)
        run(key, opt)
        del opt
    model._dec_grads = None
    torch.cuda.empty_cache()
    model.add_lora(r=32, alpha=64, dropout=0.05, seed=1)
    with torch.no_grad():
        for name, (off, n, _) in model._lora["layout"].items():
            if ".lora_B." in name:
                model.lora_params[off:off + n].copy_((torch.randn(n, generator=g) * 0.02).to(model.device))
    model.sync_lora_shadow()
    opt = WhisperAdamW(model, lr=1e-5, weight_decay=0.01, warmup_steps=0)
    run("lora", opt)
    for B, L, feats, labels in batches:
        r = results[(B, L)]
        lora, full, frozen = (r[k]["step_ms"]["median"] for k in ("lora", "full", "full_freeze_encoder"))
        print(json.dumps({"config": "whisper-small, LoRA r 32 / alpha 64 / dropout 0.05 vs full fine-tuning", "B": B, "L": L, "reps": reps,
                          "row_chunk": model.row_chunk, "trainable_parameters": int(model.lora_params.numel()), **r,
                          "lora_phase_ms": lora_phases(model, opt, feats, labels, reps),
                          "speedup_vs_full": round(full / lora, 2), "speedup_vs_full_freeze_encoder": round(frozen / lora, 2),
                          "lora_not_slower": bool(lora <= full and lora <= frozen)}), flush=True)
    S = cfg.max_source_positions
    print(json.dumps({"kernels": kernel_rows(sorted({B * L for B, L, _, _ in batches} | {max(Bs) * S}), reps)}), flush=True)


if __name__ == "__main__":
    main()
