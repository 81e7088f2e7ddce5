"""train --data_augment on the device (ssak_amd/csrc/augment.hip, ssak_amd/augment.py): each kernel against the float64
restatement (tests/augment_ref.py) and the reverberation against the reference's own output (tests/golden/augment_reverb.npz),
the whole pipeline on a ragged batch, argument checks, and the CLI end to end."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import augment_ref as R  # noqa: E402

from ssak_amd import augment as A  # noqa: E402
from ssak_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _batch(xs, T=None):
    T = T or max(len(x) for x in xs)
    w = np.zeros((len(xs), T), dtype=np.float32)
    for i, x in enumerate(xs):
        w[i, :len(x)] = x
    lens = np.array([len(x) for x in xs], dtype=np.int32)
    return torch.from_numpy(w).to(DEV), torch.from_numpy(lens).to(DEV), lens


def _rows(n, **cols):
    p = np.zeros((n, hip.AUG_NCOL), dtype=np.float64)
    p[:, hip.AUG_KIND] = hip.AUG_NONE
    p[:, hip.AUG_RATE] = 1.0
    for k, v in cols.items():
        p[:, getattr(hip, "AUG_" + k)] = v
    return p


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def test_gain_matches_to_one_ulp():
    rng = np.random.default_rng(0)
    xs = [rng.standard_normal(n).astype(np.float32) * 0.1 for n in (16000, 9000, 20001)]
    x, lens, lh = _batch(xs)
    p = _rows(3, KIND=hip.AUG_GAIN)
    p[:, hip.AUG_GAIN_DB] = [-6.0, 0.7, 5.9]
    p[:, hip.AUG_GAIN_LIN] = 10 ** (p[:, hip.AUG_GAIN_DB] / 20)
    y = hip.augment_gain_noise(x, lens, lh, torch.from_numpy(p).to(DEV), p, None).cpu().numpy()
    for i, xi in enumerate(xs):
        want = R.gain(xi, p[i, hip.AUG_GAIN_LIN])
        ulp = np.abs(y[i, :len(xi)].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1
        assert np.all(y[i, len(xi):] == 0)


def test_noise_mix_long_tiled_and_silent_noise():
    rng = np.random.default_rng(1)
    noises = [rng.standard_normal(64000).astype(np.float32) * 0.3, rng.standard_normal(3000).astype(np.float32) * 0.05,
              np.zeros(20000, dtype=np.float32)]
    bank = A._Bank(noises, DEV)
    xs = [rng.standard_normal(n).astype(np.float32) * 0.1 for n in (16000, 12000, 8000, 15000)]
    x, lens, lh = _batch(xs)
    p = _rows(4, KIND=hip.AUG_NOISE_MIX)
    p[:, hip.AUG_NOISE] = [0, 1, 2, 0]
    p[:, hip.AUG_NOISE_START] = [12345, 0, 0, 64000 - 15000]
    p[:, hip.AUG_SNR_DB] = [5.0, 20.0, 30.0, 49.0]
    p[:, hip.AUG_SNR_AMP] = 10 ** (p[:, hip.AUG_SNR_DB] / 20)
    y = hip.augment_gain_noise(x, lens, lh, torch.from_numpy(p).to(DEV), p, bank.desc).cpu().numpy()
    for i, xi in enumerate(xs):
        want = R.noise_mix(xi, noises[int(p[i, hip.AUG_NOISE])], int(p[i, hip.AUG_NOISE_START]), p[i, hip.AUG_SNR_AMP])
        assert _rel(y[i, :len(xi)], want) <= 1e-6, i
    assert np.array_equal(y[2, :8000], xs[2])  # silent noise: y = x
    # in place gives the same bits
    y2 = hip.augment_gain_noise(x, lens, lh, torch.from_numpy(p).to(DEV), p, bank.desc, out=x).cpu().numpy()
    assert np.array_equal(y, y2)


def _golden():
    g = np.load(os.path.join(HERE, "golden", "augment_reverb.npz"))
    for name in ("smallroom", "mediumroom", "largeroom", "truncated"):
        x = g["x"] if name != "truncated" else g["x"][:int(g["truncated_len"])]
        h = g["rir_" + ("largeroom" if name == "truncated" else name)].astype(np.float32) / np.float32(32768)
        yield name, x.astype(np.float32), h, g["y_" + name]


def test_reverb_matches_reference_golden():
    cases = list(_golden())
    bank = A._Bank([h for _, _, h, _ in cases], DEV)
    x, lens, lh = _batch([c[1] for c in cases])
    p = _rows(len(cases), KIND=hip.AUG_REVERB)
    p[:, hip.AUG_RIR] = range(len(cases))
    p[:, hip.AUG_RIR_PEAK] = [int(np.argmax(np.abs(h))) for _, _, h, _ in cases]
    y = hip.augment_reverb(x, lens, lh, torch.from_numpy(p).to(DEV), p, bank.desc, int(bank.lengths.max())).cpu().numpy()
    for i, (name, xi, h, want) in enumerate(cases):
        err = _rel(y[i, :len(xi)], want)
        assert err <= 2e-5, (name, err)
        assert np.all(y[i, len(xi):] == 0)


def test_reverb_long_utterance_four_step():
    """15 s with a 2 s RIR: a 2^19-point FFT (both four-step factors of 512 / 1024 points)."""
    rng = np.random.default_rng(2)
    x = (rng.standard_normal(240000) * 0.1).astype(np.float32)
    h = (rng.standard_normal(32000) * np.exp(-np.arange(32000) / 4000)).astype(np.float32)
    h[300] = 10.0
    bank = A._Bank([h], DEV)
    xd, lens, lh = _batch([x])
    p = _rows(1, KIND=hip.AUG_REVERB, RIR=0, RIR_PEAK=int(np.argmax(np.abs(h))))
    y = hip.augment_reverb(xd, lens, lh, torch.from_numpy(p).to(DEV), p, bank.desc, 32000).cpu().numpy()[0]
    assert _rel(y, R.reverb(x, h)) <= 2e-5


def test_time_stretch_against_restatement():
    rng = np.random.default_rng(4)
    xs = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in (16000, 23457, 511, 40000)]
    for rate in (0.95, 1.0, 1.05):
        x, lens, lh = _batch(xs)
        p = _rows(len(xs), RATE=rate)
        T_out = max(round(len(v) / rate) for v in xs)
        y, ol = hip.augment_time_stretch(x, lens, lh, torch.from_numpy(p).to(DEV), p, T_out)
        y, ol = y.cpu().numpy(), ol.cpu().numpy()
        for i, xi in enumerate(xs):
            n = round(len(xi) / rate)
            assert ol[i] == n
            want = R.time_stretch(xi, rate)
            assert _rel(y[i, :n], want) <= 1e-4, (rate, i, _rel(y[i, :n], want))
            assert np.all(y[i, n:] == 0)
            if rate == 1.0:
                assert np.abs(y[i, :n] - xi).max() <= 1e-5 * max(1.0, np.abs(xi).max())


def _write_wav(path, x):
    from ssak_amd.data import write_wav
    os.makedirs(os.path.dirname(path), exist_ok=True)
    write_wav(path, x)


def _augment_dirs(tmp_path, rng):
    noise = tmp_path / "noise"
    _write_wav(str(noise / "a" / "long.wav"), (rng.standard_normal(80000) * 0.2).astype(np.float32))
    _write_wav(str(noise / "short.wav"), (rng.standard_normal(4000) * 0.2).astype(np.float32))
    rirs = tmp_path / "rirs"
    lines = []
    for k, n in enumerate((4000, 12000)):
        h = (rng.standard_normal(n) * np.exp(-np.arange(n) / 800)).astype(np.float32) * 0.3
        h[50 + 100 * k] = 0.9
        _write_wav(str(rirs / "rooms" / f"r{k}.wav"), h)
        lines.append(f"--rir-id r{k} --room-id room{k} rooms/r{k}.wav")
    lines.append("--rir-id gone --room-id room9 rooms/missing.wav")
    (rirs / "rooms" / "rir_list").write_text("\n".join(lines) + "\n")
    return str(noise), f"{rirs}/[rooms/rir_list]"


def test_pipeline_ragged_batch(tmp_path):
    rng = np.random.default_rng(5)
    noise_dir, rir_arg = _augment_dirs(tmp_path, rng)
    aug = A.SpeechAugmentDevice(noise_dir, rir_arg, 16000, seed=11, device=DEV)
    assert len(aug.noise_paths) == 2 and len(aug.rir_paths) == 2 and aug.kinds == [hip.AUG_GAIN, hip.AUG_NOISE_MIX, hip.AUG_REVERB]
    xs = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in (16000, 21000, 9000, 30000, 18000, 12345)]
    # a step whose draws cover every transform
    step = next(s for s in range(200) if {int(r[hip.AUG_KIND]) for r in aug.draw(s, range(len(xs)), [len(v) for v in xs]).params} == {0, 1, 2})
    table = aug.draw(step, range(len(xs)), [len(v) for v in xs])
    x, lens, _ = _batch(xs)
    y, ol = aug.apply(x, lens, table)
    y, ol = y.cpu().numpy(), ol.cpu().numpy()
    assert np.array_equal(ol, table.out_lens) and y.shape[1] == (int(table.out_lens.max()) + 7) // 8 * 8
    for i, xi in enumerate(xs):
        n = int(ol[i])
        assert np.all(y[i, n:] == 0)
        want = R.augment_one(xi, table.params[i], hip, aug.noise.host, aug.rirs.host)
        assert len(want) == n and _rel(y[i, :n], want) <= 1e-4, (i, int(table.params[i, hip.AUG_KIND]), _rel(y[i, :n], want))
    # bit-identical on a second run, and for one utterance alone (its own row, its own length) vs in the batch
    y2, _ = aug.apply(x, lens, table)
    assert np.array_equal(y, y2.cpu().numpy())
    for i in (1, 3):
        one = A.AugmentTable(table.params[i:i + 1].copy(), table.lens[i:i + 1].copy(), table.out_lens[i:i + 1].copy())
        xa, la, _ = _batch([xs[i]])
        ya, _ = aug.apply(xa, la, one)
        n = int(ol[i])
        assert np.array_equal(ya.cpu().numpy()[0, :n], y[i, :n])


def test_bad_arguments_are_rejected():
    x, lens, lh = _batch([np.ones(16000, np.float32)])
    p = _rows(1, RATE=2.5)
    with pytest.raises(ValueError, match="rate"):
        hip.augment_time_stretch(x, lens, lh, torch.from_numpy(p).to(DEV), p, 16000)
    p = _rows(1, RATE=0.95)
    with pytest.raises(ValueError, match="output samples"):
        hip.augment_time_stretch(x, lens, lh, torch.from_numpy(p).to(DEV), p, 16000)
    p = _rows(1, KIND=hip.AUG_NOISE_MIX, SNR_AMP=2.0)
    with pytest.raises(ValueError, match="empty bank"):
        hip.augment_gain_noise(x, lens, lh, torch.from_numpy(p).to(DEV), p, None)
    bank = A._Bank([np.ones(1000, np.float32)], DEV)
    p = _rows(1, KIND=hip.AUG_NOISE_MIX, SNR_AMP=2.0, NOISE=1)
    with pytest.raises(ValueError, match="noise file"):
        hip.augment_gain_noise(x, lens, lh, torch.from_numpy(p).to(DEV), p, bank.desc)
    p = _rows(1, KIND=hip.AUG_REVERB)
    with pytest.raises(ValueError, match="empty bank"):
        hip.augment_reverb(x, lens, lh, torch.from_numpy(p).to(DEV), p, None, 1)
    p = _rows(1, KIND=hip.AUG_REVERB, RIR=0, RIR_PEAK=1000)
    with pytest.raises(ValueError, match="peak"):
        hip.augment_reverb(x, lens, lh, torch.from_numpy(p).to(DEV), p, bank.desc, 1000)
    assert hip.lib.ssak_augment_time_stretch(None, None, None, 1, 1, None, None, None, None, 1, None, 0, None) == hip.SSAK_ERR_INVALID
    bad = np.array([20000], dtype=np.int32)
    p = _rows(1, RATE=1.0)
    with pytest.raises(ValueError, match="lens"):
        hip.augment_time_stretch(x, lens, bad, torch.from_numpy(p).to(DEV), p, 30000)


def _cfg(Wav2Vec2Config, oc):
    d = dataclasses.asdict(oc)
    d.pop("initializer_range")
    return Wav2Vec2Config(**d)


def test_train_cli_with_data_augment(tmp_path):
    from ssak_amd import data as D
    from ssak_amd.checkpoint import load_pretrained, load_state_dict_file, save_pretrained
    from ssak_amd.config import Wav2Vec2Config
    from ssak_amd.model import Wav2Vec2ForCTC
    from ssak_amd.synth import VOCAB, synth_text, synth_wave
    from ssak_amd.train import evaluate, prepare, tok_pad
    from oracle import w2v2_ref as R2
    rng = np.random.default_rng(0)
    kd = tmp_path / "kaldi"
    (kd / "audio").mkdir(parents=True)
    with open(kd / "wav.scp", "w") as fw, open(kd / "text", "w") as ft, open(kd / "utt2dur", "w") as fd:
        for i in range(8):
            n = int(rng.integers(16000, 24000))
            D.write_wav(str(kd / "audio" / f"u{i}.wav"), synth_wave(rng, n))
            fw.write(f"utt{i} {kd}/audio/u{i}.wav\n")
            ft.write(f"utt{i} {synth_text(rng, 3, 6)}\n")
            fd.write(f"utt{i} {n / 16000:.3f}\n")
    noise_dir, rir_arg = _augment_dirs(tmp_path, rng)
    oc = dataclasses.replace(R2.W2V2Config.tiny(), layerdrop=0.0)
    base = Wav2Vec2ForCTC(_cfg(Wav2Vec2Config, oc))
    base.load_state_dict(R2.init_params(oc, 1))
    save_pretrained(base, D.CharTokenizer(VOCAB), str(tmp_path / "base"))
    del base
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(out, *extra):
        r = subprocess.run([sys.executable, "-m", "ssak_amd.train", str(kd), str(kd), "--base_model", str(tmp_path / "base"),
                            "--batch_size", "4", "--num_epochs", "10", "--eval_steps", "10", "--learning_rate", "3e-3",
                            "--min_duration", "0", "--output_dir", str(out), *extra], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return r

    aug_flags = ("--data_augment", "--data_augment_noise", noise_dir, "--data_augment_rir", rir_arg)
    run(tmp_path / "out", *aug_flags)
    runs = [d for d in os.listdir(tmp_path / "out") if d.endswith("_augment_online")]
    assert len(runs) == 1
    run_dir = tmp_path / "out" / runs[0]
    assert (run_dir / "checkpoint-10").is_dir() and (run_dir / "checkpoint-20").is_dir()
    assert (run_dir / "final" / "model.safetensors").exists()
    st = json.load(open(run_dir / "checkpoint-20" / "trainer_state.json"))
    losses = [e["loss"] for e in st["log_history"] if "loss" in e]
    assert len(losses) == 2 and all(np.isfinite(losses))
    # the same run without augmentation trains on other audio
    run(tmp_path / "plain", "--online")
    plain = tmp_path / "plain" / [d for d in os.listdir(tmp_path / "plain") if d.endswith("_adamwt_online")][0]
    losses_p = [e["loss"] for e in json.load(open(plain / "checkpoint-20" / "trainer_state.json"))["log_history"] if "loss" in e]
    assert losses_p[0] != losses[0]
    # evaluation is never augmented: the first checkpoint's eval_loss is an in-process evaluate of its weights, no augmenter
    st1 = json.load(open(run_dir / "checkpoint-10" / "trainer_state.json"))
    eval1 = [e["eval_loss"] for e in st1["log_history"] if "eval_loss" in e][-1]
    model, tok = load_pretrained(str(tmp_path / "base"), device=DEV, ctc_loss_reduction="mean", ctc_zero_infinity=True,
                                 layerdrop=0.0, pad_token_id=tok_pad(str(tmp_path / "base")))
    model.load_state_dict(load_state_dict_file(str(run_dir / "checkpoint-10")))
    vu = D.load_kaldi(str(kd), 0, 15)
    vw, vl = prepare(vu, tok)
    got = evaluate(model, tok, vw, vl, 4)["eval_loss"]
    assert abs(got - eval1) <= 1e-4 * abs(eval1), (got, eval1)
    # resume from checkpoint-10 reproduces the uninterrupted run's second loss
    import shutil
    shutil.copytree(tmp_path / "out", tmp_path / "out_resume")
    rr = tmp_path / "out_resume" / runs[0]
    shutil.rmtree(rr / "checkpoint-20")
    shutil.rmtree(rr / "final")
    r = run(tmp_path / "out_resume", *aug_flags)
    assert "resuming from" in r.stdout and "checkpoint-10" in r.stdout
    losses_r = [e["loss"] for e in json.load(open(rr / "checkpoint-20" / "trainer_state.json"))["log_history"] if "loss" in e]
    assert losses_r[0] == losses[0] and abs(losses_r[1] - losses[1]) < 1e-3 * abs(losses[1])
