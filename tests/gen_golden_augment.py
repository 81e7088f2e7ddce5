"""Generate tests/golden/augment_reverb.npz: the reference's own ``Reverberation._reverberate`` on float32 inputs.

Run once on the CPU with the reference checkout at hand:  python tests/gen_golden_augment.py /path/to/reference

Only ``ssak/utils/augment_reverberation.py`` is loaded, by file path, in a child process, with stand-ins for the modules it
imports at the top (``audiomentations``, ``torchaudio``, ``ssak.utils.monitoring``) that its convolution does not use;
``__init__`` (which reads RIR lists) is bypassed.  Nothing of the reference stays imported in this process.

Inputs: ``tests/golden/bonjour.wav`` (19 226 samples) with the first RIR of each of the reference's test rooms
(tests/data/rirs/{small,medium,large}room: 8 000, 16 000 and 32 000 taps -- the large one is longer than the utterance, so it is
truncated), plus its first second with the 32 000-tap RIR.  RIRs are stored as their int16 PCM samples (value / 32768).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOMS = ("smallroom", "mediumroom", "largeroom")

_CHILD = r"""
import importlib.util, json, sys, types
import numpy as np, torch
args = json.loads(sys.argv[1])
class _Base:
    def __init__(self, p=0.5):
        self.p = p
au = types.ModuleType("audiomentations"); core = types.ModuleType("audiomentations.core")
ti = types.ModuleType("audiomentations.core.transforms_interface"); ti.BaseWaveformTransform = _Base
ta = types.ModuleType("torchaudio")
ssak = types.ModuleType("ssak"); su = types.ModuleType("ssak.utils"); mon = types.ModuleType("ssak.utils.monitoring")
import logging; mon.logger = logging.getLogger("stand-in")
sys.modules.update({"audiomentations": au, "audiomentations.core": core, "audiomentations.core.transforms_interface": ti,
                    "torchaudio": ta, "ssak": ssak, "ssak.utils": su, "ssak.utils.monitoring": mon})
spec = importlib.util.spec_from_file_location("reference_augment_reverberation", args["module"])
mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
rv = mod.Reverberation.__new__(mod.Reverberation)
data = np.load(args["inputs"])
out = {}
for name in args["cases"]:
    x = torch.from_numpy(data[name + "_x"].astype(np.float32))
    h = torch.from_numpy(data[name + "_h"].astype(np.float32))
    out[name] = rv._reverberate(x, h, rescale_amp="avg").numpy().astype(np.float32)
np.savez(args["output"], **out)
"""


def read_pcm16(path):
    with wave.open(path) as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 1 and w.getframerate() == 16000
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").copy()


def main(reference: str):
    module = os.path.join(reference, "ssak", "utils", "augment_reverberation.py")
    assert os.path.isfile(module), module
    x = (read_pcm16(os.path.join(HERE, "golden", "bonjour.wav")).astype(np.float32) / 32768.0).astype(np.float32)
    rirs = {room: read_pcm16(os.path.join(reference, "tests", "data", "rirs", room, "Room001", "Room001-00001.wav")) for room in ROOMS}
    cases = {room: (x, rirs[room]) for room in ROOMS}
    cases["truncated"] = (x[:16000], rirs["largeroom"])
    with tempfile.TemporaryDirectory() as tmp:
        inp, outp = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
        np.savez(inp, **{f"{k}_x": v[0] for k, v in cases.items()}, **{f"{k}_h": v[1].astype(np.float32) / 32768.0 for k, v in cases.items()})
        subprocess.run([sys.executable, "-c", _CHILD, json.dumps({"module": module, "inputs": inp, "output": outp, "cases": list(cases)})],
                       check=True, cwd=tmp)
        got = dict(np.load(outp))
    np.savez_compressed(os.path.join(HERE, "golden", "augment_reverb.npz"), x=x, truncated_len=np.int32(16000),
                        **{f"rir_{room}": rirs[room] for room in ROOMS},
                        **{f"y_{k}": got[k] for k in cases})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SSAK_REFERENCE", "../reference"))
