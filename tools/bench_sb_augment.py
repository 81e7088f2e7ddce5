"""Timing of the SpeechBrain recipe's TimeDomainSpecAugment on the device (ssak_amd/augment.py), per training batch of the
recipe's size, B = 32 utterances of 10 s at 16 kHz:

* the speed change (``ssak_resample_sinc``) at speeds 95 and 105;
* the fused FIR + chunk-drop pass (``ssak_augment_fir_drop``, 101 taps, 5 chunks per row);
* for scale, the gain rows of ``ssak_augment_gain_noise`` on the same tensor in the same process: the project's plain
  one-read-one-write pass over the same bytes;
* the recipe's frozen-encoder training step (wav2vec2-base, random weights, Adadelta on the head) without and with the
  augmentation in front of it, draws and table uploads included.

Device events around ``--iters`` back-to-back launches after ``--warmup`` launches; prints one JSON line.  Needs the GPU:

    python tools/bench_sb_augment.py [--batch 32] [--seconds 10] [--iters 50] [--steps 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ssak_amd import augment as A  # noqa: E402
from ssak_amd import hip  # noqa: E402


def timed_us(fn, warmup, iters):
    """Mean microseconds of one call: device events around ``iters`` calls on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed training steps per variant (0: kernels only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sb_augment.py needs the GPU: there is no CPU path to time")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    B, T = args.batch, int(args.seconds * 16000)
    rng = np.random.default_rng(0)
    x = torch.from_numpy((rng.standard_normal((B, T)) * 0.1).astype(np.float32)).to(dev)
    lens_h = np.full(B, T, dtype=np.int32)
    lens = torch.from_numpy(lens_h).to(dev)
    aug = A.TimeDomainSpecAugmentDevice(seed=1)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "samples": T, "iters": args.iters}

    # the speed change
    for speed in (95, 105):
        t = aug.draw(1, range(B), lens_h)
        t.speed, t.ratio, t.taps = speed, aug._plan(speed)[:2], None
        t.counts[:] = 0
        aug.apply(x, lens, t)  # builds the filter table of this speed
        res[f"resample_{speed}_us"] = round(timed_us(lambda: aug.apply(x, lens, t), args.warmup, args.iters), 1)

    # FIR + drop: 101 taps, max_chunks chunks in every row
    taps = torch.from_numpy(A.compose_notches([0.12, 0.37, 0.71]).astype(np.float32)).to(dev)
    M = aug.max_chunks
    ch = np.zeros((B, M, 2), dtype=np.int32)
    ch[:, :, 0] = rng.integers(0, T - 2000, (B, M))
    ch[:, :, 1] = ch[:, :, 0] + rng.integers(1000, 2001, (B, M))
    cnt_h = np.full(B, M, dtype=np.int32)
    chd, cnt = torch.from_numpy(ch).to(dev), torch.from_numpy(cnt_h).to(dev)
    out = torch.empty_like(x)
    res["fir_drop_us"] = round(timed_us(lambda: hip.augment_fir_drop(x, taps, chd, cnt, cnt_h, out=out), args.warmup, args.iters), 1)
    res["fir_only_us"] = round(timed_us(lambda: hip.augment_fir_drop(x, taps, out=out), args.warmup, args.iters), 1)
    res["copy_drop_us"] = round(timed_us(lambda: hip.augment_fir_drop(x, None, chd, cnt, cnt_h, out=out), args.warmup, args.iters), 1)

    # the gain pass on the same tensor
    p = np.zeros((B, hip.AUG_NCOL), dtype=np.float64)
    p[:, hip.AUG_KIND], p[:, hip.AUG_GAIN_LIN], p[:, hip.AUG_RATE] = hip.AUG_GAIN, 0.7, 1.0
    pd = torch.from_numpy(p).to(dev)
    ws = torch.empty(max(int(hip.lib.ssak_augment_gain_noise_workspace_bytes(B, T)), 16), dtype=torch.uint8, device=dev)
    res["gain_us"] = round(timed_us(lambda: hip.augment_gain_noise(x, lens, lens_h, pd, p, None, out=out, workspace=ws), args.warmup, args.iters), 1)
    res["fir_to_gain"] = round(res["fir_drop_us"] / res["gain_us"], 2)
    moved = 2.0 * B * T * 4
    res["fir_drop_GBps"] = round(moved / res["fir_drop_us"] / 1e3, 1)
    res["gain_GBps"] = round(moved / res["gain_us"] / 1e3, 1)
    res["fir_GFMAps"] = round(101.0 * B * T / res["fir_only_us"] / 1e3, 1)

    # the recipe's frozen-encoder step
    if args.steps > 0:
        from ssak_amd.config import Wav2Vec2Config
        from ssak_amd.model import Wav2Vec2ForCTC
        from ssak_amd.sb_head import Brain, CTCHead
        cfg = Wav2Vec2Config()
        model = Wav2Vec2ForCTC(cfg, device=dev)
        head = CTCHead(cfg.hidden_size, 1024, 76, device=dev, seed=1)
        brain = Brain(model, head, freeze_wav2vec=True)
        toks = torch.from_numpy(rng.integers(1, 70, (B, 100)).astype(np.int64))
        tl = torch.ones(B)
        xh = x.cpu()

        def step(k, augment):
            w, wl = xh, torch.ones(B)
            if augment:
                t = aug.draw(k, range(B), lens_h)
                w, l2 = aug.apply(xh.to(dev), lens, t)
                wl = l2.cpu().to(torch.float32) / w.shape[1]
            return float(brain.fit_batch(w, wl, toks, tl).item())

        for name, on in (("step_plain_ms", False), ("step_augmented_ms", True), ("step_plain_again_ms", False), ("step_augmented_again_ms", True)):
            for k in range(3):
                step(1000 + k, on)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.steps):
                step(k + 1, on)
            b.record()
            torch.cuda.synchronize()
            res[name] = round(a.elapsed_time(b) / args.steps, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
