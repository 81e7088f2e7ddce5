"""Host side of train --data_augment (ssak_amd/augment.py): RIR lists, the noise folder, the keyed draws, and the float64
restatement (tests/augment_ref.py) against the reference's own reverberation (tests/golden/augment_reverb.npz)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import augment_ref as R  # noqa: E402

from ssak_amd import augment as A  # noqa: E402
from ssak_amd import hip  # noqa: E402
from ssak_amd.data import shard_batch  # noqa: E402


def _touch(path, data=b"RIFF"):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def test_rir_list_parsing(tmp_path):
    root = tmp_path / "rirs"
    _touch(str(root / "rooms" / "Room001" / "a.wav"))
    _touch(str(root / "rooms" / "Room001" / "c.wav"))
    (root / "rooms" / "rir_list").write_text(
        "--rir-id small-Room001-00001 --room-id small-Room001 rooms/Room001/a.wav\n"
        "--rir-id small-Room001-00002 --room-id small-Room001 --rt60 0.4 --probability 0.5 rooms/Room001/missing.wav\n"
        "\n"
        "--rir-id x --room-id y --receiver-position-id r --source-position-id s --drr 1 --cte 2 rooms/Room001/c.wav\n")
    got = A.parse_rir_arg(f"{root}/[rooms/rir_list]")
    assert got == (str(root), ["rooms/rir_list"])
    paths = A.parse_rir_list(*got[0:1], got[1][0])
    assert paths == [f"{root}/rooms/Room001/a.wav", f"{root}/rooms/Room001/c.wav"]  # the missing entry is skipped
    assert A.parse_rir_arg("") is None
    with pytest.raises(RuntimeError, match=r"syntax must be /root/folder/\[rir/file1,rir/file2,...\]"):
        A.parse_rir_arg(str(root / "rooms" / "rir_list"))
    with pytest.raises(RuntimeError, match="RIR list file .* does not exist"):
        A.parse_rir_arg(f"{root}/[rooms/rir_list,other/rir_list]")
    with pytest.raises(SystemExit):  # a line without the required options: argparse's error, as in the reference
        (root / "bad_list").write_text("rooms/Room001/a.wav\n")
        A.parse_rir_list(str(root), "bad_list")


def test_noise_folder_scan(tmp_path):
    for rel in ("b/2.wav", "a/z.WAV", "a/sub/1.wav", "c.flac", "notes.txt", "b/readme"):
        _touch(str(tmp_path / rel))
    got = [os.path.relpath(p, tmp_path) for p in A.scan_noise_dir(str(tmp_path))]
    assert got == sorted(["a/sub/1.wav", "a/z.WAV", "b/2.wav", "c.flac"])


KINDS3 = [hip.AUG_GAIN, hip.AUG_NOISE_MIX, hip.AUG_REVERB]


def test_draws_are_keyed_not_streamed():
    a = A.draw_row(69, 7, 3, 32000, KINDS3, [320000, 5000], 4)
    b = A.draw_row(69, 7, 3, 32000, KINDS3, [320000, 5000], 4)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, A.draw_row(69, 8, 3, 32000, KINDS3, [320000, 5000], 4))
    assert not np.array_equal(a, A.draw_row(70, 7, 3, 32000, KINDS3, [320000, 5000], 4))
    # one global batch of 7 utterances at step 12, split over 1 or 2 ranks: every utterance gets the same row
    whole = [11, 4, 9, 2, 30, 5, 8]
    lens = {i: 16000 + 1000 * i for i in whole}
    one = {i: A.draw_row(1, 12, whole.index(i), lens[i], KINDS3, [320000], 2) for i in whole}
    for world in (2, 3):
        for rank in range(world):
            mine = shard_batch(whole, rank, world)
            for i in mine:
                assert np.array_equal(A.draw_row(1, 12, whole.index(i), lens[i], KINDS3, [320000], 2), one[i])


def test_draw_ranges_and_frequencies():
    rows = np.stack([A.draw_row(5, s, p, 24000 + 37 * p, KINDS3, [320000, 20000, 3000], 6) for s in range(300) for p in range(10)])
    kinds = rows[:, hip.AUG_KIND].astype(int)
    freq = np.bincount(kinds, minlength=3) / len(kinds)
    assert np.all(np.abs(freq - 1 / 3) < 0.04), freq
    g = rows[:, hip.AUG_GAIN_DB]
    assert g.min() >= -6 and g.max() < 6 and g.min() < -5.9 and g.max() > 5.9
    assert np.allclose(rows[:, hip.AUG_GAIN_LIN], 10 ** (g / 20))
    s = rows[:, hip.AUG_SNR_DB]
    assert s.min() >= 5 and s.max() < 50 and np.allclose(rows[:, hip.AUG_SNR_AMP], 10 ** (s / 20))
    r = rows[:, hip.AUG_RATE]
    assert r.min() >= 0.95 and r.max() < 1.05 and r.min() < 0.951 and r.max() > 1.049
    nf = rows[:, hip.AUG_NOISE].astype(int)
    assert set(nf) == {0, 1, 2} and set(rows[:, hip.AUG_RIR].astype(int)) == set(range(6))
    L = np.array([24000 + 37 * p for _ in range(300) for p in range(10)])
    hi = np.maximum(0, np.array([320000, 20000, 3000])[nf] - L - 1600)
    st = rows[:, hip.AUG_NOISE_START]
    assert np.all(st >= 0) and np.all(st <= hi) and np.all(st[nf == 2] == 0) and st[nf == 0].max() > 0.9 * hi[nf == 0].max()
    assert np.array_equal(rows[:, hip.AUG_OUT_LEN], [round(l / q) for l, q in zip(L, r)])
    # only the transforms that exist are drawn
    only_gain = np.stack([A.draw_row(5, s, 0, 16000, [hip.AUG_GAIN], [], 0) for s in range(50)])
    assert set(only_gain[:, hip.AUG_KIND].astype(int)) == {hip.AUG_GAIN}


def _golden():
    g = np.load(os.path.join(HERE, "golden", "augment_reverb.npz"))
    for name in ("smallroom", "mediumroom", "largeroom", "truncated"):
        x = g["x"] if name != "truncated" else g["x"][:int(g["truncated_len"])]
        h = g["rir_" + ("largeroom" if name == "truncated" else name)].astype(np.float32) / np.float32(32768)
        yield name, x, h, g["y_" + name]


def test_restated_reverb_matches_reference_golden():
    for name, x, h, want in _golden():
        got = R.reverb(x, h)
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert err <= 1e-6, (name, err)


def test_time_stretch_identity_at_rate_one():
    rng = np.random.default_rng(3)
    for L in (511, 512, 16000, 20001):
        x = rng.standard_normal(L)
        y = R.time_stretch(x, 1.0)
        assert len(y) == L and np.abs(y - x).max() <= 1e-9


def test_stretched_sine_keeps_its_bin():
    t = np.arange(32000)
    f_bin = 100  # bin 100 of a 2048-point frame at 16 kHz: 781.25 Hz
    x = np.sin(2 * np.pi * f_bin * t / 2048)
    for rate in (0.95, 1.05):
        y = R.time_stretch(x, rate)
        assert len(y) == round(32000 / rate)
        spec = np.abs(np.fft.rfft(y[4096:4096 + 16384] * np.hanning(16384)))
        assert abs(int(np.argmax(spec)) / 8 - f_bin) <= 0.25  # (8 bins of the long FFT per frame bin)
