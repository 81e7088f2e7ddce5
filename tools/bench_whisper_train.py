"""Whisper-small full fine-tuning on one MI355X: the train step of ssak_amd/whisper_train.py (encoder forward, teacher-forced decoder
forward, decoder backward, encoder backward, clip + AdamW over both halves) on 30 s windows given as input features.  Seeded random
weights at whisper-small's shapes (d_model 768, 12 + 12 layers of 12 heads, ffn 3072, 51 865 tokens, 1500 encoder frames): nothing
is read from disk.

usage: python tools/bench_whisper_train.py [B=8,32] [L=64,448] [reps=5] [row_chunk=2048,256]

Per (B, L, row_chunk), medians over ``reps`` of device-event time after 2 warm-up steps: the whole step through the public path
(``forward_train(features, labels)``, ``backward()``, ``WhisperAdamW.step()``) and the same step taken apart (the encoder engine's
``forward_hidden``, ``forward_train`` on its output, ``backward``, ``backward_hidden``, the optimizer).  Work for the roof: matrix
products and attention only, 2 M N K each, backward counted as twice the forward, against the dense bf16 peak bench.py uses.
Per launch: ``ssak_dec_attention_bwd`` (self-attention at L = 448; cross-attention at 448 x 1500) and ``ssak_dec_ce_bwd`` (256 rows
of the vocabulary) next to a device copy that moves the same number of bytes.  Prints one JSON line per (B, L, row_chunk) and one for
the kernels.
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BF16_TFLOPS = 2500.0  # the dense bf16 MFMA peak bench.py measures against


def forward_flops(cfg, B, L):
    D, F, S, V = cfg.d_model, cfg.decoder_ffn_dim, cfg.max_source_positions, (cfg.vocab_size + 7) // 8 * 8
    enc = cfg.encoder_layers * (2 * B * S * D * (4 * D + 2 * cfg.encoder_ffn_dim) + 4 * B * S * S * D)
    enc += 2 * B * 2 * S * cfg.num_mel_bins * 3 * D + 2 * B * S * D * 3 * D
    rows = B * L
    dec = cfg.decoder_layers * (2 * rows * D * (6 * D + 2 * F) + 2 * B * S * D * 2 * D + 4 * B * L * D * (L / 2 + S)) + 2 * rows * D * V
    return enc, dec


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


def phases(model, opt, feats, labels, reps):
    """The step taken apart, each phase between its own pair of events."""
    from ssak_amd import hip
    names = ("encoder_forward", "decoder_forward", "decoder_backward", "encoder_backward", "optimizer")
    acc = {n: [] for n in names}
    enc_model = model.encoder
    for it in range(reps + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        enc_model.train()
        hidden, _ = enc_model.forward_hidden(feats)
        enc_model.training = False
        ev[1].record()
        model.forward_train(hidden, labels)
        ev[2].record()
        d_enc = model.backward()
        ev[3].record()
        d_bf = torch.empty(d_enc.shape, dtype=torch.bfloat16, device=d_enc.device)
        hip.check(hip.lib.ssak_cast_f32_bf16(hip.ptr(d_enc), hip.ptr(d_bf), d_enc.numel(), hip.stream()))
        enc_model.backward_hidden(d_bf)
        model.encoder_grads_ready = True  # (backward() saw an encoder output; the encoder's gradients were filled here)
        ev[4].record()
        opt.step()
        ev[5].record()
        ev[5].synchronize()
        if it >= 2:
            for i, n in enumerate(names):
                acc[n].append(ev[i].elapsed_time(ev[i + 1]))
    return {n: round(statistics.median(v), 3) for n, v in acc.items()}


def kernel_rows(reps):
    """Per launch: the two attention backward shapes and the cross-entropy backward, next to a copy of the same bytes."""
    from ssak_amd import hip
    dev, nh, D, B = "cuda:0", 12, 768, 8
    g = torch.Generator().manual_seed(1)
    bf = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    out = {}

    def copy_ms(nbytes):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        return timed(lambda: dst.copy_(src), reps * 4)[0]

    for name, Lq, Lk, causal in (("self_L448", 448, 448, True), ("cross_448x1500", 448, 1500, False)):
        q, do = bf(B * Lq, D), bf(B * Lq, D)
        k, v = bf(B * Lk, D), bf(B * Lk, D)
        ctx, lse = hip.dec_attention_fwd_lse(q, k, v, B, Lq, Lk, nh, causal=causal)
        dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
        delta = torch.empty_like(lse)
        med, lo, hi = timed(lambda: hip.lib.ssak_dec_attention_bwd(
            hip.ptr(q), D, hip.ptr(k), D, hip.ptr(v), D, Lk, None, None, B, Lq, nh, 64, int(causal), 0, hip.ptr(ctx), hip.ptr(lse), hip.ptr(do),
            hip.ptr(dq), D, hip.ptr(dk), D, hip.ptr(dv), D, hip.ptr(delta), hip.stream()), reps * 4)
        nbytes = 2 * D * (4 * B * Lq + 4 * B * Lk) + 12 * B * nh * Lq
        flops = 10 * B * nh * 64 * Lq * Lk * (0.5 if causal else 1.0)  # five products of 2 Lq Lk 64 per head
        out["attention_bwd_" + name] = {"B": B, "median_us": round(med * 1e3, 1), "min_us": round(lo * 1e3, 1), "max_us": round(hi * 1e3, 1),
                                        "tflops": round(flops / med / 1e9, 1), "bytes": nbytes, "copy_same_bytes_us": round(copy_ms(nbytes) * 1e3, 1)}
    R, V, Vp = 256, 51865, 51872
    logits = (torch.randn(R, Vp, generator=g) * 3).to(dev)
    targets = np.random.default_rng(0).integers(0, V, R).astype(np.int32)
    tg_d = torch.from_numpy(targets).to(dev)
    dl = torch.empty((R, Vp), dtype=torch.bfloat16, device=dev)
    row_loss, loss_sum = torch.empty(R, device=dev), torch.zeros(1, device=dev)
    med, lo, hi = timed(lambda: hip.lib.ssak_dec_ce_bwd(hip.ptr(logits), R, V, Vp, hip.ptr(tg_d), hip._hp(targets), 1.0 / R, hip.ptr(dl), Vp,
                                                        hip.ptr(row_loss), hip.ptr(loss_sum), hip.stream()), reps * 4)
    nbytes = R * Vp * 6
    out["ce_bwd_256x51865"] = {"median_us": round(med * 1e3, 1), "min_us": round(lo * 1e3, 1), "max_us": round(hi * 1e3, 1), "bytes": nbytes,
                               "gbytes_per_s_one_read": round(nbytes / med / 1e6, 1), "copy_same_bytes_us": round(copy_ms(nbytes) * 1e3, 1)}
    return out


def main():
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    from ssak_amd.whisper_train import WhisperAdamW
    Bs = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "8,32").split(",")]
    Ls = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "64,448").split(",")]
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    chunks = [int(x) for x in (sys.argv[4] if len(sys.argv) > 4 else "2048,256").split(",")]
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    cfg = WhisperSeq2SeqConfig(pad_token_id=50257, eos_token_id=50257)  # whisper-small
    model = WhisperSeq2Seq(cfg)
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
    opt = WhisperAdamW(model, lr=1e-5, weight_decay=0.01, warmup_steps=0)
    for B in Bs:
        feats = torch.randn(B, cfg.num_mel_bins, 2 * cfg.max_source_positions, generator=g).to(model.device)
        for L, chunk in ((L, c) for L in Ls for c in chunks):
            labels = torch.randint(0, 50257, (B, L), generator=g).numpy()
            model.row_chunk = chunk

            def step():
                model.forward_train(feats, labels)
                model.backward()
                opt.step()

            med, lo, hi = timed(step, reps)
            fe, fd = forward_flops(cfg, B, L)
            out = {"config": "whisper-small full fine-tuning", "B": B, "L": L, "reps": reps, "row_chunk": model.row_chunk,
                   "step_ms": {"median": round(med, 2), "min": round(lo, 2), "max": round(hi, 2)}, "utterances_per_s": round(B / med * 1e3, 1),
                   "audio_s_per_s": round(30 * B / med * 1e3, 1), "algorithmic_tflop_per_step": round(3 * (fe + fd) / 1e12, 2),
                   "roof_fraction": round(3 * (fe + fd) / (med * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                   "phase_ms": phases(model, opt, feats, labels, reps), "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
            print(json.dumps(out), flush=True)
    print(json.dumps({"kernels": kernel_rows(reps)}), flush=True)


if __name__ == "__main__":
    main()
