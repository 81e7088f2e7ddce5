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
