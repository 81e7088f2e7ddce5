"""train --data_augment on the device (ssak_amd.augment, ssak_amd/csrc/augment.hip): ms per batch of B = 32 x 10 s.

Kernel legs (device events after warm-up, synthetic banks): gain, background noise (10 files of 20 s), reverberation with
0.5, 1 and 2 s RIRs, time stretch alone, and the reference's mix (a uniform choice among the three, then the time stretch)
through ``SpeechAugmentDevice.apply``.  Train legs: the base B = 32 step of ``ssak_amd.train --online`` fed from a Kaldi folder
of 10 s WAV files, with and without augmentation (the augmentation runs on the ingest stream, one batch ahead).

    python tools/bench_augment.py [--iters 20] [--steps 20] [--no-train]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ssak_amd import augment as A  # noqa: E402
from ssak_amd import hip  # noqa: E402
from ssak_amd.data import write_wav  # noqa: E402

DEV = "cuda:0"


def _timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def _folders(d, rng, rir_s):
    os.makedirs(os.path.join(d, "noise"), exist_ok=True)
    for k in range(10):
        write_wav(os.path.join(d, "noise", f"n{k}.wav"), (rng.standard_normal(320000) * 0.1).astype(np.float32))
    rooms = os.path.join(d, "rirs", "room")
    os.makedirs(rooms, exist_ok=True)
    with open(os.path.join(rooms, "rir_list"), "w") as f:
        for k in range(8):
            n = int(rir_s * 16000)
            h = (rng.standard_normal(n) * np.exp(-np.arange(n) / (0.15 * n))).astype(np.float32) * 0.2
            h[40] = 0.9
            write_wav(os.path.join(rooms, f"r{k}.wav"), h)
            f.write(f"--rir-id r{k} --room-id room room/r{k}.wav\n")
    return os.path.join(d, "noise"), os.path.join(d, "rirs") + "/[room/rir_list]"


def kernel_legs(iters, B=32, T=160000):
    rng = np.random.default_rng(0)
    x = torch.from_numpy((rng.standard_normal((B, T)) * 0.1).astype(np.float32)).to(DEV)
    lens_h = np.full(B, T, np.int32)
    lens = torch.from_numpy(lens_h).to(DEV)
    out = {}
    d = tempfile.mkdtemp(prefix="ssak_aug_")
    try:
        for rir_s in (0.5, 1.0, 2.0):
            noise_dir, rir_arg = _folders(os.path.join(d, str(rir_s)), rng, rir_s)
            aug = A.SpeechAugmentDevice(noise_dir, rir_arg, 16000, 69, DEV)
            tab = aug.draw(0, range(B), lens_h)
            if rir_s == 1.0:
                for name, kind in (("gain", hip.AUG_GAIN), ("noise", hip.AUG_NOISE_MIX)):
                    p = tab.params.copy()
                    p[:, hip.AUG_KIND] = kind
                    pd = torch.from_numpy(p).to(DEV)
                    out[f"{name}_ms"] = _timed(lambda: hip.augment_gain_noise(x, lens, lens_h, pd, p, aug.noise.desc), iters)
                p = tab.params.copy()
                pd = torch.from_numpy(p).to(DEV)
                T_out = int(tab.out_lens.max())
                out["time_stretch_ms"] = _timed(lambda: hip.augment_time_stretch(x, lens, lens_h, pd, p, T_out), iters)
                out["mix_ms"] = _timed(lambda: aug.apply(x, lens, tab), iters)
                out["mix_kinds"] = np.bincount(tab.params[:, hip.AUG_KIND].astype(int), minlength=3).tolist()
            p = tab.params.copy()
            p[:, hip.AUG_KIND] = hip.AUG_REVERB
            p[:, hip.AUG_RIR_PEAK] = [aug.rir_peaks[int(r)] for r in p[:, hip.AUG_RIR]]
            pd = torch.from_numpy(p).to(DEV)
            y = torch.empty_like(x)
            out[f"reverb_{rir_s:g}s_ms"] = _timed(lambda: hip.augment_reverb(x, lens, lens_h, pd, p, aug.rirs.desc, aug.max_rir, out=y), iters)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


def train_legs(steps, warmup=5, B=32, n_files=512):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from side_benches import _w2v2_state
    from ssak_amd.config import Wav2Vec2Config
    from ssak_amd.data import CharTokenizer, length_grouped_batches, load_kaldi, pad_labels, remove_special_words
    from ssak_amd.ingest import BatchPrefetcher, DeviceIngest
    from ssak_amd.model import Wav2Vec2ForCTC
    from ssak_amd.synth import VOCAB, write_kaldi_folder
    from ssak_amd.trainer import AdamW, Trainer
    d = tempfile.mkdtemp(prefix="ssak_aug_kaldi_")
    try:
        write_kaldi_folder(os.path.join(d, "k"), n_files, threads=min(16, len(os.sched_getaffinity(0))))
        noise_dir, rir_arg = _folders(d, np.random.default_rng(1), 1.0)
        utts = load_kaldi(os.path.join(d, "k"), 1.0, 15.0)
        tok = CharTokenizer(VOCAB)
        labels = [tok.encode(remove_special_words(u.text)) for u in utts]
        plan = length_grouped_batches([int(u.duration * 16000) for u in utts], B, np.random.RandomState(69))[:warmup + steps]
        model = Wav2Vec2ForCTC(Wav2Vec2Config(), device=DEV, freeze_feature_encoder=True, seed=69).train()
        model.load_state_dict(_w2v2_state(model))
        trainer = Trainer(model, AdamW(model, lr=1e-4, weight_decay=0.0, max_grad_norm=1.0, warmup_steps=500, total_steps=100000))
        res = {}
        for name, aug in (("online", None), ("online_augment", A.SpeechAugmentDevice(noise_dir, rir_arg, 16000, 69, DEV))):
            ingest = DeviceIngest(16000, DEV, augment=aug)
            feed = iter(BatchPrefetcher(ingest, [[(utts[i].path, None, None) for i in m] for m in plan], depth=3,
                                        labels=[pad_labels([labels[i] for i in m]) for m in plan],
                                        keys=[(k, list(range(len(m)))) for k, m in enumerate(plan)]))
            for k in range(len(plan)):
                if k == warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                x, ln, lab = next(feed)
                trainer.train_step(x, ln, lab, raw=False)
            torch.cuda.synchronize()
            res[f"{name}_ms_per_step"] = round((time.perf_counter() - t0) / steps * 1e3, 3)
        res["augment_overhead_pct"] = round(100 * (res["online_augment_ms_per_step"] / res["online_ms_per_step"] - 1), 2)
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    res = {"batch": "32 x 10 s", **kernel_legs(a.iters)}
    if not a.no_train:
        res.update(train_legs(a.steps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
