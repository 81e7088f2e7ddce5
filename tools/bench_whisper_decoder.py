"""Whisper-small decoder on one MI355X: transcript scoring at L = 64 and language identification, B = 32, on a given encoder
output (the encoder has its own benchmark, tools/bench_whisper.py).  Seeded random weights at whisper-small's shapes (d_model 768,
12 decoder layers of 12 heads, ffn 3072, 51 865 tokens, 1500 encoder frames): nothing is read from disk.

usage: python tools/bench_whisper_decoder.py [B=32] [L=64] [reps=20]

Each figure is the median over ``reps`` calls of device-event time around one whole call (``score`` includes its device-to-host
copy of the [B, L - 1] log-probabilities and the host sums; ``detect_language`` its arg-max read-back), after 3 warm-up calls of
the same shapes.  Prints one JSON line.  Work counted for the rates: matrix products only, 2 M N K each.
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gemm_flops(cfg, B, L, S):
    D, F, V = cfg.d_model, cfg.decoder_ffn_dim, (cfg.vocab_size + 7) // 8 * 8
    rows = B * L
    per_layer = 2 * rows * D * (3 * D + D + D + D) + 2 * B * S * D * 2 * D + 2 * rows * D * F * 2  # self qkv + out, cross q + out; cross k|v; ffn
    attn = 4 * B * L * D * (L / 2 + S)  # q k^T and p v over the visible keys
    return cfg.decoder_layers * (per_layer + attn) + 2 * rows * D * V


def timed(fn, reps, warmup=3):
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


def main():
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    langs = {f"l{i:02d}"[:3]: 50259 + i for i in range(99)}
    cfg = WhisperSeq2SeqConfig(lang_to_id=langs)  # whisper-small
    model = WhisperSeq2Seq(cfg)
    g = torch.Generator().manual_seed(0)
    model.dec_params.copy_((torch.randn(model.dec_params.numel(), generator=g) * 0.02).to(model.device))
    for name in model.layout:  # LayerNorm scales around 1
        if name.endswith("layer_norm.weight"):
            model.dec_param(name).fill_(1.0)
    model.sync_decoder_shadow()
    S = cfg.max_source_positions
    enc = torch.randn(B, S, cfg.d_model, generator=g).to(torch.bfloat16).to(model.device)
    tokens = torch.randint(0, 50257, (B, L), generator=g).numpy()
    tokens[:, 0] = cfg.decoder_start_token_id
    out = {"config": "whisper-small decoder", "B": B, "L": L, "S": S, "reps": reps, "row_chunk": model.row_chunk}
    med, lo, hi = timed(lambda: model.score(enc, tokens), reps)
    fl = gemm_flops(cfg, B, L, S)
    out["score"] = {"median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "utterances_per_s": round(B / med * 1e3, 1),
                    "tokens_per_s": round(B * (L - 1) / med * 1e3, 1), "product_tflops": round(fl / med / 1e9, 2)}
    med, lo, hi = timed(lambda: model.detect_language(enc), reps)
    fl = gemm_flops(cfg, B, 1, S)
    out["detect_language"] = {"median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                              "utterances_per_s": round(B / med * 1e3, 1), "product_tflops": round(fl / med / 1e9, 2)}
    assert np.isfinite(model.score(enc, tokens).sum_logprob).all()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
