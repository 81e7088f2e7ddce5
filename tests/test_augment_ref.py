"""CPU: the float64 restatement tests/augment_ref.py that the augmentation kernels are held to, and the float32 yardstick
of tests/test_gpu_augment_edges.py.

* ``stft`` and ``istft`` equal torch.stft / torch.istft (n_fft 2048, hop 512, periodic Hann, center=True, pad_mode "constant")
  in float64 within 1e-12 (``err_max``; measured: stft <= 4e-14, istft <= 2e-15) over L in {1, 511, 512, 513, 2047, 2048, 2049,
  5000, 23457} and rates {0.5, 1.0, 1.3, 2.0}.  torch.istft rejects an output of length 0 (L = 1 at rate 2): there the
  restatement returns an empty array.  This pins the transform pair of ``time_stretch``; the phase vocoder between them is
  librosa's, spelled out, and stays unpinned (librosa is not installed).
* The float32 restatements (``reverb_f32``, ``time_stretch_f32``: scipy's single-precision FFT, np.arctan2 on float32, the
  phase accumulator and the mean-|.| sums in float64) stay within 1e-6 of the float64 ones, elementwise over max|ref|, on every
  case of the GPU edge tests: the yardstick is a sane number and the cases are well conditioned.  Measured: reverberation
  3e-10 to 5e-7, time stretch 3e-8 to 5e-7.
* ``len(time_stretch(x, rate)) == round(len(x) / rate)``, on the halves too (round half to even).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import augment_ref as R  # noqa: E402

TORCH_LENS = (1, 511, 512, 513, 2047, 2048, 2049, 5000, 23457)
TORCH_RATES = (0.5, 1.0, 1.3, 2.0)
YARDSTICK_BAR = 1e-6


def _window():
    return torch.hann_window(R.N_FFT, periodic=True, dtype=torch.float64)


def _wave(L, seed):
    return np.random.default_rng(seed).standard_normal(L) * 0.1


def test_err_max():
    assert R.err_max([1.0, 2.5], [1.0, 2.0]) == 0.25
    assert R.err_max([0.0, -3.0], [0.0, 0.0]) == 3.0
    assert R.err_max(np.zeros(0), np.zeros(0)) == 0.0
    assert np.isnan(R.err_max([np.nan, 1.0], [1.0, 1.0]))  # (a NaN passes no `<=` bar)
    with pytest.raises(AssertionError):
        R.err_max(np.zeros(3), np.zeros(4))


@pytest.mark.parametrize("L", TORCH_LENS)
def test_stft_is_torch_stft(L):
    x = _wave(L, L)
    want = torch.stft(torch.from_numpy(x), R.N_FFT, hop_length=R.HOP, window=_window(), center=True, pad_mode="constant",
                      return_complex=True).numpy()
    got = R.stft(x)
    assert got.shape == want.shape == (R.N_FFT // 2 + 1, 1 + L // R.HOP)
    err = max(R.err_max(got.real, want.real), R.err_max(got.imag, want.imag))
    print(f"stft L={L}: {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("L", TORCH_LENS)
def test_istft_is_torch_istft(L):
    x = _wave(L, 100 + L)
    for rate in TORCH_RATES:
        D = R.phase_vocoder(R.stft(x), rate)
        n = int(round(L / rate))
        got = R.istft(D, n)
        assert got.shape == (n,)
        if n == 0:  # (L = 1, rate 2: torch.istft refuses an empty output)
            assert (L, rate) == (1, 2.0)
            continue
        want = torch.istft(torch.from_numpy(D), R.N_FFT, hop_length=R.HOP, window=_window(), center=True, length=n).numpy()
        err = R.err_max(got, want)
        print(f"istft L={L} rate={rate}: {err:.2e}")
        assert err <= 1e-12, (L, rate, err)


def test_time_stretch_length_is_pythons_round():
    for (L, rate), n in R.STRETCH_HALVES.items():
        assert (L / rate) % 1 == 0.5 and round(L / rate) == n
        assert len(R.time_stretch(_wave(L, 7), rate)) == n
        assert len(R.time_stretch_f32(_wave(L, 7).astype(np.float32), rate)) == n
    for launch in R.stretch_edge_cases():
        for c in launch:
            assert len(R.time_stretch(c["x"], c["rate"])) == round(len(c["x"]) / c["rate"])


def test_reverb_f32_yardstick_on_the_edge_cases():
    worst = 0.0
    for c in R.reverb_edge_cases():
        if c["kind"] != R.KIND_REVERB or len(c["x"]) == 0:
            continue
        assert c["d"] == int(np.argmax(np.abs(c["h"])))
        y32 = R.reverb_f32(c["x"], c["h"])
        assert y32.dtype == np.float32
        Y = R.err_max(y32, R.reverb(c["x"], c["h"]))
        print(f"reverb_f32 vs float64 {c['name']}: {Y:.2e}")
        assert Y <= YARDSTICK_BAR, (c["name"], Y)
        worst = max(worst, Y)
    assert worst > 0.0


def test_reverb_f32_yardstick_at_2_to_the_24():
    x, h = R.reverb_pow24_case()
    y32 = R.reverb_f32(x, h)
    assert y32.dtype == np.float32
    Y = R.err_max(y32, R.reverb(x, h))
    print(f"reverb_f32 vs float64, L = 2^23: {Y:.2e}")
    assert Y <= YARDSTICK_BAR


def test_time_stretch_f32_yardstick_on_the_edge_cases():
    worst = 0.0
    for launch in R.stretch_edge_cases():
        for c in launch:
            y32 = R.time_stretch_f32(c["x"], c["rate"])
            assert y32.dtype == np.float32
            Y = R.err_max(y32, R.time_stretch(c["x"], c["rate"]))
            print(f"time_stretch_f32 vs float64 {c['name']}: {Y:.2e}")
            assert Y <= YARDSTICK_BAR, (c["name"], Y)
            worst = max(worst, Y)
    assert worst > 0.0


def test_edge_case_tables_hold_what_the_gpu_tests_need():
    """The sizes each case is there for (FFT log2 of the reverberation rows; the noise segment arithmetic)."""
    def logn(L, Lh):
        need = L + min(L, Lh) - 1
        k = 0
        while (1 << k) < need:
            k += 1
        return max(k, 1)

    cases = {c["name"]: c for c in R.reverb_edge_cases()}
    want = {"L1_h1_k1": 1, "L1_h5_truncated_to_one": 1, "L2_h2_k2": 2, "L3_h7_k3": 3, "L64_h64_k7": 7, "L2049_h2048_need_4096": 12,
            "L2048_h2049_truncated_by_one": 12, "L4097_h1_k13": 13, "L8192_h300_k14": 14, "L8193_h300_k14": 14,
            "L70000_h9000_k17": 17, "L70000_h9000_quiet_rir": 17}
    for name, k in want.items():
        assert logn(len(cases[name]["x"]), len(cases[name]["h"])) == k, name
    assert 2049 + 2048 - 1 == 4096 and max(len(c["x"]) for c in cases.values()) == R.REVERB_T
    assert [cases[n]["d"] for n in ("L1000_h1500_peak_at_L_minus_1", "L1000_h1500_peak_at_L", "L1000_h1500_peak_at_Lh_minus_1",
                                    "L1000_h300_peak_at_0")] == [999, 1000, 1499, 0]
    x, h = R.reverb_pow24_case()
    assert logn(len(x), len(h)) == 24
    noises, rows = R.gain_noise_edge_cases()
    assert sorted(len(n) for n in noises[:4]) == [1, 3000, 20000, 64000]
    assert {len(r["x"]) for r in rows} >= {0, 1, 8191, 8192, 8193, 20000} and max(len(r["x"]) for r in rows) == R.GN_T
    for r in rows:
        if r["kind"] == "noise":
            N, L = len(noises[r["noise"]]), len(r["x"])
            assert 0 <= r["start"] <= N - min(L, N), r["name"]
    rms = [float(np.sqrt(np.mean(n.astype(np.float64) ** 2))) for n in noises[4:]]
    assert rms[0] >= 1e-9 > rms[1]
