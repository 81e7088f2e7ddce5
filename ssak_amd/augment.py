"""``train --data_augment`` on the device: the reference's ``SpeechAugment`` as wav2vec_train.py:258-273 builds it
(``apply_prob=1``, ``speed=True``, ``gain=True``, noise and reverberation when given, ``apply_speed_separately=True``;
ssak/utils/augment.py:123-180), applied to training batches only, between the resample and the normalisation of
``DeviceIngest`` (kernels: ssak_amd/csrc/augment.hip).

Per training utterance of length L (samples at 16 kHz, before augmentation):

1. One transform, drawn uniformly from those available, in the order Gain, AddBackgroundNoise (``--data_augment_noise``),
   Reverberation (``--data_augment_rir``):

   * Gain: ``gain_db ~ U(-6, 6)``, ``y = x * f32(10^(gain_db / 20))`` in fp32.
   * AddBackgroundNoise (audiomentations, relative RMS): ``snr_db ~ U(5, 50)``, a noise file drawn uniformly, and a start drawn
     uniformly in whole samples over ``[0, max(0, N - L - 1600)]`` (audiomentations' 0.1 s margin; the exact offset rule
     differs between audiomentations versions and is pinned nowhere: this is the rule here).  The segment is
     ``noise[start : start + min(L, N)]``, tiled by repetition up to L; ``rms`` over the segment before tiling;
     ``y = x + n * (rms(x) / 10^(snr_db / 20)) / rms(n)``, or ``y = x`` when ``rms(n) < 1e-9``.
   * Reverberation (augment_reverberation.py:104-177): an RIR drawn uniformly; ``d = argmax|h|`` over the full RIR; h cut to
     its first L samples; ``[h[d:], zeros, h[:d]]`` of length L (no rotation when ``d >= L``); circular convolution of length
     L; ``y = conv / (mean|conv| + 1e-14) * mean|x|``.

2. Then always TimeStretch: ``rate ~ U(0.95, 1.05)``, ``librosa.effects.time_stretch(y, rate)`` with librosa >= 0.10's
   defaults (n_fft 2048, hop 512, periodic Hann, ``center=True`` with zero padding), output length ``round(L / rate)``.
   The phase vocoder's time steps are ``np.arange(0, F, rate)`` in fp64 and its phase accumulator is kept in fp64: librosa's
   float32 accumulator reaches ~5e5 rad where one float32 ulp is ~0.03 rad, so the contract is the fp64 one, not librosa's
   bits.

Draws: every parameter is drawn on the host from ``np.random.default_rng([seed, step, position in the global batch])``, in the
order transform, gain, snr, noise file, noise start, RIR, rate (all drawn whatever the transform), so the same utterance at the
same step gets the same augmentation at any world size, any shard split and after a resume, and a checkpoint needs no new RNG
state.  Noise files and RIRs must be PCM WAV (the ingest's reader); other sample rates go through ``ssak_resample_sinc``.

``TimeDomainSpecAugment`` of the SpeechBrain recipe
---------------------------------------------------
The recipe's finetune yaml sets ``augmentation: !new:speechbrain.lobes.augment.TimeDomainSpecAugment`` with
``speeds: [95, 100, 105]`` and wav2vec_train.py:45-46 applies it to every training batch.  ``TimeDomainSpecAugmentDevice`` is the
project's own contract for it, modelled on speechbrain 0.5 (speechbrain is not installed and the reference holds no vector of
it): **parity with speechbrain's bits is unpinned**.  Training batches only, never validation.  Input: the padded batch
``x [B, T]`` fp32 with zero padding and the absolute lengths ``L [B]``.  Three stages, in this order:

1. Speed perturbation, one draw for the whole global batch: ``i ~ integers(len(speeds))``,
   ``new_sr = sample_rate * speeds[i] // 100``; the padded batch is resampled ``sample_rate -> new_sr`` with
   ``ssak_resample_sinc`` (torchaudio's windowed-sinc formula; speechbrain's own ``Resample`` is a Kaldi-style filter: a stated
   deviation) and then treated as ``sample_rate`` audio.  ``T' = ceil(T * new_r / orig_r)`` and ``L' = ceil(L * new_r / orig_r)``
   with the reduced rates (16000 -> 15200 is 20:19, 16000 -> 16800 is 20:21); speed 100 copies nothing.  The resampler is given
   the lengths, so a row is exactly zero from ``L'`` on: resampling the zero padding itself (speechbrain resamples the padded
   tensor) would leave the few samples of filter tail behind ``L'`` only where the batch's padding has room for them, and the
   rows would then depend on how the global batch was split.  Samples before ``L'`` are the same either way.
2. DropFreq, one filter for the whole global batch: ``count ~ integers(drop_freq_count_low, drop_freq_count_high + 1)``
   (defaults 0, 3), then ``count`` frequencies ``f = u * (1 - 1e-14) + 1e-14``, ``u ~ U[0, 1)``.  Per frequency a 101-tap notch
   in float64 on the host (``notch_filter(f, 101, 0.05)``: centre ``f + 0.05``, cut-offs ``f`` and ``f + 0.1``):
   ``n = arange(101) - 50``; ``w[k] = 0.42 - 0.5 cos(2 pi k / 101) + 0.08 cos(4 pi k / 101)`` (the periodic Blackman window);
   ``sinc(z) = sin(z) / z``, 1 at the centre tap; ``lo = sinc(3 f n) * w``, ``lo /= sum(lo)``; ``hi = sinc(3 (f + 0.1) n) * w``,
   ``hi /= -sum(hi)``, ``hi[50] += 1``; ``notch = lo + hi``.  The batch filter starts as a unit impulse at tap 50 and for each
   notch in turn becomes ``g_new[j] = sum_k notch[k] * g_pad[j + k]`` (g zero-padded by 50 on both sides: 101 taps stay).  The
   signal is filtered the same way, ``y[b, t] = sum_k g[k] * x[b, t + k - 50]`` with zeros outside ``[0, T')``.  Both are
   CROSS-CORRELATIONS, as ``torch.nn.functional.conv1d`` is: the periodic window makes the taps asymmetric by about 1.5e-3, so
   the orientation is part of the contract.  Taps go to the device as fp32; ``count == 0`` leaves the batch bit-identical.
3. DropChunk, per utterance: ``n ~ integers(drop_chunk_count_low, drop_chunk_count_high + 1)`` (defaults 0, 5), ``n`` lengths
   ``~ integers(drop_chunk_length_low, drop_chunk_length_high + 1)`` (defaults 1000, 2000),
   ``start_max = max(0, L' - max(lengths))``, ``n`` starts ``~ integers(0, start_max + 1)``; samples ``[start, start + length)``,
   clipped to ``[0, T')``, are set to 0; chunks may overlap.  Placement uses the absolute ``L'``, not speechbrain's
   ``floor(rel_len * T')``, which depends on the shard's padding.  ``drop_chunk_noise_factor`` must be 0.

``perturb_prob``, ``drop_freq_prob``, ``drop_chunk_prob`` (defaults 1): each stage draws ``u ~ U[0, 1)`` and is skipped when
``u > p``; all draws are made whether the stage runs or not.  Batch-level draws come from
``np.random.default_rng([seed, step])`` in the order: speed ``u``, ``i``; DropFreq ``u``, ``count``, the ``count`` frequencies;
DropChunk ``u``.  The chunk draws of an utterance come from ``np.random.default_rng([seed, step, position in the global
batch])`` in the order ``n``, the lengths, the starts (no further draw when ``n == 0``).  ``step`` is the recipe loop's global
step counter, so the rule above holds here too: same utterance, same step, same augmentation at any world size and after a
resume, with no new checkpoint state.  Stages 2 and 3 are one kernel (``ssak_augment_fir_drop``).
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import shlex
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip

GAIN_DB = (-6.0, 6.0)
SNR_DB = (5.0, 50.0)
RATE = (0.95, 1.05)
NOISE_MARGIN_S = 0.1
# audiomentations' audio extensions (find_audio_files); only PCM WAV decodes here, the others raise at load
AUDIO_EXTENSIONS = (".aac", ".aif", ".aiff", ".flac", ".m4a", ".mp3", ".mp4", ".ogg", ".opus", ".wav", ".webm")
RIR_SYNTAX_ERROR = "--data_augment_rir syntax must be /root/folder/[rir/file1,rir/file2,...]"


def parse_rir_arg(arg: str) -> Optional[Tuple[str, List[str]]]:
    """``ROOT/[a/rir_list,b/rir_list]`` -> (ROOT, [lists]) (wav2vec_train.py:260-266); '' -> None (no reverberation)."""
    if not arg:
        return None
    if "[" not in arg:
        raise RuntimeError(RIR_SYNTAX_ERROR)
    root = arg.split("[")[0].rstrip("/")
    lists = arg.split("[")[1].split("]")[0].split(",")
    for f in lists:
        if not os.path.isfile(os.path.join(root, f)):
            raise RuntimeError("RIR list file {} does not exist".format(os.path.join(root, f)))
    return root, lists


def _rir_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(add_help=False)  # augment_reverberation.py:72-83
    p.add_argument("--rir-id", type=str, required=True)
    p.add_argument("--room-id", type=str, required=True)
    p.add_argument("--receiver-position-id", type=str, default=None)
    p.add_argument("--source-position-id", type=str, default=None)
    p.add_argument("--rt60", type=float, default=None)
    p.add_argument("--drr", type=float, default=None)
    p.add_argument("--cte", type=float, default=None)
    p.add_argument("--probability", type=float, default=None)
    p.add_argument("rir_rspecifier", type=str)
    return p


def parse_rir_list(root: str, rir_file: str) -> List[str]:
    """The RIR paths of one list (``_parse_rir_list``): PATH relative to ROOT; pipes and missing files are skipped; blank lines
    are ignored."""
    parser, out = _rir_parser(), []
    with open(os.path.join(root, rir_file)) as f:
        for line in f:
            if not line.strip():
                continue
            rir = parser.parse_args(shlex.split(line.strip()))
            path = root + "/" + rir.rir_rspecifier
            if len(rir.rir_rspecifier.split()) == 1 and os.path.exists(path):
                out.append(path)
    return out


def scan_noise_dir(noise_dir: str) -> List[str]:
    """Audio files under ``noise_dir``, recursively, in sorted order."""
    found = []
    for dirpath, _, files in os.walk(noise_dir, followlinks=True):
        found += [os.path.join(dirpath, f) for f in files if f.lower().endswith(AUDIO_EXTENSIONS)]
    return sorted(found)


class AugmentTable:
    """The draws of one batch: ``params`` fp64 [B, hip.AUG_NCOL] (ssak_hip.h SSAK_AUG_* columns), the lengths before (``lens``)
    and after (``out_lens``) augmentation, host side."""
    __slots__ = ("params", "lens", "out_lens")

    def __init__(self, params: np.ndarray, lens: np.ndarray, out_lens: np.ndarray):
        self.params, self.lens, self.out_lens = params, lens, out_lens


def draw_row(seed: int, step: int, pos: int, L: int, kinds: Sequence[int], noise_lens: Sequence[int], n_rirs: int,
             sample_rate: int = 16000) -> np.ndarray:
    """One utterance's row of the table (module docstring: the draw contract)."""
    rng = np.random.default_rng([int(seed) % (1 << 63), int(step), int(pos)])
    row = np.zeros(hip.AUG_NCOL, dtype=np.float64)
    kind = kinds[int(rng.integers(len(kinds)))]
    gain_db = float(rng.uniform(*GAIN_DB))
    snr_db = float(rng.uniform(*SNR_DB))
    nf = int(rng.integers(len(noise_lens))) if noise_lens else 0
    hi = max(0, int(noise_lens[nf]) - int(L) - int(NOISE_MARGIN_S * sample_rate)) if noise_lens else 0
    start = int(rng.integers(hi + 1))
    rir = int(rng.integers(n_rirs)) if n_rirs else 0
    rate = float(rng.uniform(*RATE))
    row[hip.AUG_KIND] = kind
    row[hip.AUG_GAIN_DB], row[hip.AUG_GAIN_LIN] = gain_db, 10.0 ** (gain_db / 20.0)
    row[hip.AUG_SNR_DB], row[hip.AUG_SNR_AMP] = snr_db, 10.0 ** (snr_db / 20.0)
    row[hip.AUG_NOISE], row[hip.AUG_NOISE_START] = nf, start
    row[hip.AUG_RIR] = rir
    row[hip.AUG_RATE] = rate
    row[hip.AUG_OUT_LEN] = round(int(L) / rate)
    return row


class _Bank:
    """Signals resident on the device, concatenated, with their host mirrors (``ssak_audio_bank``)."""

    def __init__(self, waves: List[np.ndarray], device):
        self.host = waves
        self.lengths = np.array([len(w) for w in waves], dtype=np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths[:-1], dtype=np.int64)]).astype(np.int64)
        self.data = torch.from_numpy(np.concatenate(waves).astype(np.float32)).to(device)
        self.offsets_d = torch.from_numpy(self.offsets).to(device)
        self.lengths_d = torch.from_numpy(self.lengths).to(device)
        self.desc = hip.AudioBank(len(waves), self.data.data_ptr(), self.offsets_d.data_ptr(), self.lengths_d.data_ptr(),
                                  self.offsets.ctypes.data, self.lengths.ctypes.data)


class SpeechAugmentDevice:
    """Banks loaded once; ``draw`` on the host, ``apply`` on the current stream (DeviceIngest's, in training)."""

    def __init__(self, noise_dir: Optional[str], rir_arg: Optional[str], sample_rate: int = 16000, seed: int = 69, device="cuda:0"):
        from .ingest import DeviceIngest
        self.sample_rate, self.seed, self.device = sample_rate, int(seed), torch.device(device)
        self.noise_paths = scan_noise_dir(noise_dir) if noise_dir else []
        if noise_dir and not self.noise_paths:
            raise RuntimeError(f"no audio file under --data_augment_noise {noise_dir}")
        rr = parse_rir_arg(rir_arg or "")
        self.rir_paths = [p for f in rr[1] for p in parse_rir_list(rr[0], f)] if rr else []
        if rr and not self.rir_paths:
            raise RuntimeError(f"no RIR file found in the lists of --data_augment_rir {rir_arg}")
        self.kinds = [hip.AUG_GAIN] + ([hip.AUG_NOISE_MIX] if self.noise_paths else []) + ([hip.AUG_REVERB] if self.rir_paths else [])
        ing = DeviceIngest(sample_rate, self.device, normalize=False, readers=4)

        def load(paths):
            out = []
            for i in range(0, len(paths), 64):
                w, l = ing.load_batch([(p, None, None) for p in paths[i:i + 64]])
                w, l = w.cpu().numpy(), l.cpu().numpy()
                out += [w[j, :l[j]].copy() for j in range(len(l))]
            return out

        self.noise = _Bank(load(self.noise_paths), self.device) if self.noise_paths else None
        self.rirs = _Bank(load(self.rir_paths), self.device) if self.rir_paths else None
        if self.noise is not None and (self.noise.lengths <= 0).any():
            raise RuntimeError(f"empty noise file {self.noise_paths[int(np.argmin(self.noise.lengths))]}")
        if self.rirs is not None and (self.rirs.lengths <= 0).any():
            raise RuntimeError(f"empty RIR file {self.rir_paths[int(np.argmin(self.rirs.lengths))]}")
        self.rir_peaks = [int(np.argmax(np.abs(h))) for h in self.rirs.host] if self.rirs is not None else []
        self.max_rir = int(self.rirs.lengths.max()) if self.rirs is not None else 1

    def draw(self, step: int, positions: Sequence[int], lengths: Sequence[int]) -> AugmentTable:
        noise_lens = [] if self.noise is None else [int(n) for n in self.noise.lengths]
        n_rirs = 0 if self.rirs is None else len(self.rir_paths)
        rows = [draw_row(self.seed, step, p, L, self.kinds, noise_lens, n_rirs, self.sample_rate) for p, L in zip(positions, lengths)]
        params = np.stack(rows) if rows else np.zeros((0, hip.AUG_NCOL))
        for r in params:
            if int(r[hip.AUG_KIND]) == hip.AUG_REVERB:
                r[hip.AUG_RIR_PEAK] = self.rir_peaks[int(r[hip.AUG_RIR])]
        return AugmentTable(params, np.asarray(lengths, dtype=np.int32), params[:, hip.AUG_OUT_LEN].astype(np.int32))

    def apply(self, waves: torch.Tensor, lens: torch.Tensor, table: AugmentTable, params_d: Optional[torch.Tensor] = None):
        """(waves [B, T] fp32, lens [B]) -> (augmented waves [B, T'], lens'), T' = max(out_lens) rounded up to 8; padding zero."""
        B, T = waves.shape
        if params_d is None:
            params_d = torch.from_numpy(table.params).to(waves.device, non_blocking=False)
        kinds = table.params[:, hip.AUG_KIND].astype(int)
        y = hip.augment_gain_noise(waves, lens, table.lens, params_d, table.params, None if self.noise is None else self.noise.desc)
        if (kinds == hip.AUG_REVERB).any():
            hip.augment_reverb(y, lens, table.lens, params_d, table.params, self.rirs.desc, self.max_rir, out=y)
        T_out = max(int(table.out_lens.max()) if B else 1, 1)
        T_out = (T_out + 7) // 8 * 8
        return hip.augment_time_stretch(y, lens, table.lens, params_d, table.params, T_out)


# ------------------------------------------------------------------ the SpeechBrain recipe's TimeDomainSpecAugment
NOTCH_TAPS = 101
NOTCH_WIDTH = 0.05


def notch_filter(f: float, taps: int = NOTCH_TAPS, width: float = NOTCH_WIDTH) -> np.ndarray:
    """The notch of one dropped frequency, float64 [taps] (module docstring, stage 2)."""
    pad = taps // 2
    n = np.arange(taps, dtype=np.float64) - pad
    k = np.arange(taps, dtype=np.float64)
    w = 0.42 - 0.5 * np.cos(2.0 * np.pi * k / taps) + 0.08 * np.cos(4.0 * np.pi * k / taps)

    def sinc(z):
        out = np.ones_like(z)
        nz = z != 0
        out[nz] = np.sin(z[nz]) / z[nz]
        return out

    lo = sinc(3.0 * f * n) * w
    lo /= lo.sum()
    hi = sinc(3.0 * (f + 2.0 * width) * n) * w
    hi /= -hi.sum()
    hi[pad] += 1.0
    return lo + hi


def compose_notches(freqs: Sequence[float], taps: int = NOTCH_TAPS) -> np.ndarray:
    """The batch filter of the dropped frequencies: a unit impulse cross-correlated with each notch in turn, float64 [taps]."""
    pad = taps // 2
    g = np.zeros(taps, dtype=np.float64)
    g[pad] = 1.0
    for f in freqs:
        g = np.correlate(np.pad(g, pad), notch_filter(float(f), taps), mode="valid")
    return g


class TdsaTable:
    """The draws of one batch, host side: ``speed`` (percent; 100 = not perturbed) and its index ``speed_index`` (None when the
    stage is skipped), ``freqs`` and their filter ``taps`` (fp32 [101]; None = no filter), the chunk table ``chunks``
    [B, max_chunks, 2] int32 (start, end) with ``counts`` [B] int32, the lengths before (``lens``) and after (``out_lens``) the
    speed change and the reduced rates ``ratio`` = (orig_r, new_r)."""
    __slots__ = ("speed", "speed_index", "freqs", "taps", "chunks", "counts", "lens", "out_lens", "ratio")


class TimeDomainSpecAugmentDevice:
    """``speechbrain.lobes.augment.TimeDomainSpecAugment`` under its own argument names (module docstring: the contract; parity
    with speechbrain's bits is unpinned).  ``draw`` is host only; ``apply`` runs on the current stream."""

    def __init__(self, perturb_prob: float = 1.0, drop_freq_prob: float = 1.0, drop_chunk_prob: float = 1.0, speeds: Sequence[int] = (95, 100, 105),
                 sample_rate: int = 16000, drop_freq_count_low: int = 0, drop_freq_count_high: int = 3, drop_chunk_count_low: int = 0,
                 drop_chunk_count_high: int = 5, drop_chunk_length_low: int = 1000, drop_chunk_length_high: int = 2000,
                 drop_chunk_noise_factor: float = 0, seed: int = 69):
        if float(drop_chunk_noise_factor) != 0.0:
            raise ValueError(f"TimeDomainSpecAugment: drop_chunk_noise_factor = {drop_chunk_noise_factor} is not supported (dropped chunks "
                             "are set to zero): it must be 0")
        self.speeds = [int(s) for s in speeds]
        if not self.speeds or min(self.speeds) <= 0:
            raise ValueError(f"TimeDomainSpecAugment: speeds = {list(speeds)} must be positive percentages")
        for name, lo, hi in (("drop_freq_count", drop_freq_count_low, drop_freq_count_high), ("drop_chunk_count", drop_chunk_count_low, drop_chunk_count_high),
                             ("drop_chunk_length", drop_chunk_length_low, drop_chunk_length_high)):
            if not 0 <= int(lo) <= int(hi):
                raise ValueError(f"TimeDomainSpecAugment: {name}_low = {lo}, {name}_high = {hi} must satisfy 0 <= low <= high")
        self.perturb_prob, self.drop_freq_prob, self.drop_chunk_prob = float(perturb_prob), float(drop_freq_prob), float(drop_chunk_prob)
        self.sample_rate, self.seed = int(sample_rate), int(seed)
        self.freq_count = (int(drop_freq_count_low), int(drop_freq_count_high))
        self.chunk_count = (int(drop_chunk_count_low), int(drop_chunk_count_high))
        self.chunk_length = (int(drop_chunk_length_low), int(drop_chunk_length_high))
        self.max_chunks = max(1, self.chunk_count[1])
        self._plans, self._tables = {}, {}

    def _plan(self, speed: int) -> Tuple[int, int, int]:
        """(orig_r, new_r, filter taps per phase) of sample_rate -> sample_rate * speed // 100 (host arithmetic)."""
        if speed not in self._plans:
            o, n, w, t = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            hip.check(hip.lib.ssak_resample_plan(self.sample_rate, self.sample_rate * speed // 100, C.byref(o), C.byref(n), C.byref(w), C.byref(t)))
            self._plans[speed] = (o.value, n.value, t.value)
        return self._plans[speed]

    def _table(self, speed: int, device) -> torch.Tensor:
        """The resampler's filter table of one speed on the device, built once (``ssak_resample_table``)."""
        key = (speed, str(device))
        if key not in self._tables:
            _, n, t = self._plan(speed)
            host = torch.empty(n * t, dtype=torch.float32)
            hip.check(hip.lib.ssak_resample_table(self.sample_rate, self.sample_rate * speed // 100, C.c_void_p(host.data_ptr())))
            self._tables[key] = host.to(device)
        return self._tables[key]

    def draw(self, step: int, positions: Sequence[int], lengths: Sequence[int]) -> TdsaTable:
        seed = self.seed % (1 << 63)
        rng = np.random.default_rng([seed, int(step)])
        t = TdsaTable()
        u_speed, i = float(rng.random()), int(rng.integers(len(self.speeds)))
        u_freq, count = float(rng.random()), int(rng.integers(self.freq_count[0], self.freq_count[1] + 1))
        freqs = rng.random(count) * (1.0 - 1e-14) + 1e-14
        u_chunk = float(rng.random())
        t.speed_index = None if u_speed > self.perturb_prob else i
        t.speed = 100 if t.speed_index is None else self.speeds[i]
        t.freqs = freqs if u_freq <= self.drop_freq_prob else freqs[:0]
        t.taps = compose_notches(t.freqs).astype(np.float32) if len(t.freqs) else None
        t.lens = np.asarray(lengths, dtype=np.int64)
        t.ratio = (1, 1) if t.speed == 100 else self._plan(t.speed)[:2]
        t.out_lens = -(-(t.lens * t.ratio[1]) // t.ratio[0])
        t.chunks = np.zeros((len(t.lens), self.max_chunks, 2), dtype=np.int32)
        t.counts = np.zeros(len(t.lens), dtype=np.int32)
        for b, (pos, L) in enumerate(zip(positions, t.out_lens)):
            r = np.random.default_rng([seed, int(step), int(pos)])
            n = int(r.integers(self.chunk_count[0], self.chunk_count[1] + 1))
            if n == 0:
                continue
            length = r.integers(self.chunk_length[0], self.chunk_length[1] + 1, size=n)
            start = r.integers(0, max(0, int(L) - int(length.max())) + 1, size=n)
            if u_chunk <= self.drop_chunk_prob:
                t.counts[b] = n
                t.chunks[b, :n, 0], t.chunks[b, :n, 1] = start, start + length
        t.lens, t.out_lens = t.lens.astype(np.int32), t.out_lens.astype(np.int32)
        return t

    def apply(self, waves: torch.Tensor, lens: torch.Tensor, table: TdsaTable):
        """(waves [B, T] fp32 zero padded, lens [B] int32 on the device) -> (augmented waves [B, T'], lens' [B] int32)."""
        B, T = waves.shape
        assert waves.is_cuda and waves.dtype == torch.float32 and waves.is_contiguous() and len(table.lens) == B
        if table.speed != 100:
            o, n = table.ratio
            T2 = -(-(T * n) // o)
            y = torch.empty((B, T2), dtype=torch.float32, device=waves.device)
            lens = lens.to(device=waves.device, dtype=torch.int32).contiguous()
            lens2 = torch.empty(B, dtype=torch.int32, device=waves.device)
            sr = self.sample_rate
            hip.check(hip.lib.ssak_resample_sinc(hip.ptr(waves), hip.ptr(lens), B, T, sr, sr * table.speed // 100,
                                                 hip.ptr(self._table(table.speed, waves.device)), hip.ptr(y), T2, hip.ptr(lens2), hip.stream()))
            waves, lens = y, lens2
        any_chunk = bool(table.counts.any())
        if table.taps is None and not any_chunk:
            return waves, lens
        taps = None if table.taps is None else torch.from_numpy(table.taps).to(waves.device)
        if any_chunk:
            chunks, counts = torch.from_numpy(table.chunks).to(waves.device), torch.from_numpy(table.counts).to(waves.device)
            return hip.augment_fir_drop(waves, taps, chunks, counts, table.counts), lens
        return hip.augment_fir_drop(waves, taps), lens
