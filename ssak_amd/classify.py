"""Utterance-level classification on the acoustic encoder: pooling over time, a two-Linear head, softmax / cross-entropy.

The reference ships one consumer of this shape, ``ssak/utils/gender.py``: ``Wav2Vec2ForSpeechClassification`` /
``HubertForSpeechClassification`` (:51-133, :155-237) behind ``predict_gender`` (:242-301).  The model is the encoder's last
hidden state, pooled over time (``merged_strategy``: mean, sum or max), then ``dropout -> Linear(H, H) -> tanh -> dropout ->
Linear(H, num_labels)`` (the ``ClassificationHead``), then softmax for prediction or ``CrossEntropyLoss`` for fine-tuning.
Language and emotion tagging have the same shape.

Here the encoder is the HIP engine of :mod:`ssak_amd.model`, stopped at ``ssak_w2v2_forward_hidden`` and re-entered at
``ssak_w2v2_backward_hidden``; everything between the hidden state and the loss runs in ``ssak_amd/csrc/classify.hip``
(``ssak_pool_*``, ``ssak_cls_head_*``, ``ssak_cls_softmax_ce``).  HuBERT checkpoints (parameters prefixed ``hubert.``) have the
graph of wav2vec2 with the feature projection's LayerNorm on and no batch-norm positional convolution: the prefix is mapped,
other variants are refused.

No timing of this path has been measured.

Command line, like the reference's ``__main__``::

    python -m ssak_amd.classify AUDIO... --model DIR [--start S --end E]
"""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import hip
from .config import Wav2Vec2Config
from .model import Wav2Vec2ForCTC, conv_out_lengths

POOLING_MODES = ("mean", "sum", "max")
HEAD_PARAMS = ("classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight", "classifier.out_proj.bias")
_ENCODER_PREFIXES = ("wav2vec2.", "hubert.")
_LEGACY = {"wav2vec2.encoder.pos_conv_embed.conv.weight_g": "wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original0",
           "wav2vec2.encoder.pos_conv_embed.conv.weight_v": "wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original1"}


@dataclasses.dataclass
class SpeechClassifierConfig(Wav2Vec2Config):
    """The encoder's configuration plus what the classification models of ssak/utils/gender.py read from theirs:
    ``pooling_mode``, ``num_labels`` / ``id2label`` and ``final_dropout`` (the head's dropout; the encoder applies none when it
    stops at the hidden state).  ``model_type`` is the checkpoint's encoder prefix (``wav2vec2`` or ``hubert``)."""
    pooling_mode: str = "mean"
    num_labels: int = 2
    id2label: Optional[Dict[int, str]] = None
    problem_type: Optional[str] = None
    model_type: str = "wav2vec2"

    def __post_init__(self):
        if self.pooling_mode not in POOLING_MODES:
            raise ValueError(f"pooling_mode {self.pooling_mode!r}: one of {POOLING_MODES}")
        if self.id2label is not None:
            self.id2label = {int(k): str(v) for k, v in self.id2label.items()}
            self.num_labels = len(self.id2label)
        if self.model_type not in ("wav2vec2", "hubert"):
            raise ValueError(f"model_type {self.model_type!r}: wav2vec2 or hubert")

    @classmethod
    def from_hf_dict(cls, d: dict) -> "SpeechClassifierConfig":
        # HuBERT variants whose graph is not wav2vec2's
        if d.get("feat_proj_layer_norm", True) is False:
            raise ValueError("feat_proj_layer_norm = false: the feature projection without its LayerNorm is not built")
        if d.get("conv_pos_batch_norm", False):
            raise ValueError("conv_pos_batch_norm = true: the batch-norm positional convolution is not built")
        names = {f.name for f in dataclasses.fields(cls)}
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in d.items() if k in names}
        return cls(**kw)

    def to_dict(self) -> dict:
        d = super().to_dict()
        d["model_type"] = self.model_type
        d["architectures"] = ["HubertForSpeechClassification" if self.model_type == "hubert" else "Wav2Vec2ForSpeechClassification"]
        labels = self.id2label or {i: f"LABEL_{i}" for i in range(self.num_labels)}
        d["id2label"] = {str(k): v for k, v in labels.items()}
        d["label2id"] = {v: k for k, v in labels.items()}
        if self.model_type == "hubert":
            d["feat_proj_layer_norm"], d["conv_pos_batch_norm"] = True, False
        return d


class SpeechClassifierOutput:
    __slots__ = ("loss", "logits", "probs", "frame_lens")

    def __init__(self, loss, logits, probs, frame_lens=None):
        self.loss, self.logits, self.probs, self.frame_lens = loss, logits, probs, frame_lens


class SpeechClassifier:
    """Encoder engine + pooling + classification head.  ``forward`` returns ``.logits`` [B, num_labels], ``.probs`` and (with
    labels) ``.loss``; ``backward`` leaves the head's gradients in ``head_grads`` and the encoder's in ``encoder.grads``.

    ``exact``: the engine's fp32-exact verification mode (float hidden state, fp32 products); the head is fp32 either way."""

    def __init__(self, config: SpeechClassifierConfig, device: str = "cuda:0", exact: bool = False, freeze_feature_encoder: bool = True,
                 seed: int = 69):
        if config.problem_type not in (None, "single_label_classification"):
            raise NotImplementedError(f"problem_type {config.problem_type!r}: only single-label classification is built")
        if config.num_labels < 2:
            raise NotImplementedError("num_labels = 1 is regression in the reference (MSELoss): only single-label classification is built")
        self.config = config
        self.device = torch.device(device)
        self.exact = bool(exact)
        self.training = False
        # the encoder: driven only through forward_hidden / backward_hidden; its lm_head stays at zero and is never run
        self.encoder = Wav2Vec2ForCTC(config, device=device, freeze_feature_encoder=freeze_feature_encoder, seed=seed, exact=self.exact)
        H, Cn = config.hidden_size, config.num_labels
        if H % 8:
            raise ValueError(f"hidden_size {H} must be a multiple of 8")
        self.head_layout: Dict[str, tuple] = {}
        off = 0
        for name, shape in zip(HEAD_PARAMS, ((H, H), (H,), (Cn, H), (Cn,))):
            n = int(np.prod(shape))
            self.head_layout[name] = (off, n, shape)
            off += (n + 3) // 4 * 4  # every tensor starts on a 16-byte boundary
        with torch.cuda.device(self.device):
            self.head_params = torch.zeros(off, dtype=torch.float32, device=self.device)
            self.head_grads = torch.zeros(off, dtype=torch.float32, device=self.device)
        g = torch.Generator().manual_seed(int(seed))
        for name in HEAD_PARAMS:  # nn.Linear weights as Wav2Vec2PreTrainedModel._init_weights draws them, biases zero
            if name.endswith("weight"):
                self.head_param(name).copy_(torch.randn(self.head_layout[name][2], generator=g) * 0.02)
        self._saved = None

    # ------------------------------------------------------------------ parameters
    def head_param(self, name: str) -> torch.Tensor:
        off, n, shape = self.head_layout[name]
        return self.head_params[off:off + n].view(shape)

    def head_grad(self, name: str) -> torch.Tensor:
        off, n, shape = self.head_layout[name]
        return self.head_grads[off:off + n].view(shape)

    def grad(self, name: str) -> torch.Tensor:
        """Gradient by state-dict name (``classifier.*`` or an encoder parameter under its ``wav2vec2.`` name)."""
        return self.head_grad(name) if name in self.head_layout else self.encoder.grad(name)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Encoder parameters under ``wav2vec2.*`` names (the unused lm_head left out) and the head's ``classifier.*``."""
        sd = {n: t for n, t in self.encoder.state_dict().items() if not n.startswith("lm_head.")}
        sd.update({n: self.head_param(n).detach().cpu().clone() for n in HEAD_PARAMS})
        return sd

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        enc = {n: t for n, t in sd.items() if n in self.encoder.layout}
        missing = [n for n in list(self.encoder.layout) + list(HEAD_PARAMS) if n not in sd and not n.startswith("lm_head.")]
        extra = [n for n in sd if n not in self.encoder.layout and n not in self.head_layout]
        if strict and (missing or extra):
            raise RuntimeError(f"state_dict mismatch: missing {missing[:4]} unexpected {extra[:4]}")
        self.encoder.load_state_dict(enc, strict=False)
        for n in HEAD_PARAMS:
            if n in sd:
                t = torch.as_tensor(sd[n]).to(torch.float32)
                if tuple(t.shape) != self.head_layout[n][2]:
                    raise RuntimeError(f"size mismatch for {n}: {tuple(t.shape)} vs {self.head_layout[n][2]}")
                self.head_param(n).copy_(t.to(self.device))
        return self

    def train(self, mode: bool = True):
        self.training = bool(mode)
        self.encoder.train(mode)
        return self

    def eval(self):
        return self.train(False)

    # ------------------------------------------------------------------ forward / backward
    def __call__(self, input_values, lengths=None, labels=None):
        return self.forward(input_values, lengths, labels)

    def forward(self, input_values: torch.Tensor, lengths=None, labels=None) -> SpeechClassifierOutput:
        """``input_values`` [B, T] normalised waveforms.  ``lengths`` = None pools all frames, padding included -- the
        reference's ``torch.mean(hidden, dim=1)``; with ``lengths`` [B] (samples, host values) the encoder masks the padding and
        only the valid frames are pooled.  ``labels`` [B] class ids (host values)."""
        cfg = self.config
        frame_lens = None
        if lengths is not None:
            lengths = torch.as_tensor(lengths).cpu().numpy() if not isinstance(lengths, np.ndarray) else lengths
            frame_lens = conv_out_lengths(cfg, lengths).astype(np.int32)
        hidden, flens = self.encoder.forward_hidden(input_values, lengths=lengths)
        seed = self.encoder._used_seed  # the step's dropout seed: the head's two sites draw under it like the encoder's
        with torch.cuda.device(self.device):
            pooled, argmax = hip.pool_fwd(hidden, frame_lens, cfg.pooling_mode)
            W1, b1, W2, b2 = (self.head_param(n) for n in HEAD_PARAMS)
            logits, act = hip.cls_head_fwd(pooled, W1, b1, W2, b2, cfg.final_dropout, seed, self.training)
            probs, loss, dlogits = hip.cls_softmax_ce(logits, labels, 1.0, want_grad=self.training)
        self._saved = (dlogits, pooled, act, argmax, frame_lens, hidden.shape[1], hidden.dtype, seed) if self.training and dlogits is not None else None
        return SpeechClassifierOutput(loss, logits, probs, flens)

    def backward(self, grad_scale: float = 1.0):
        """d loss / d parameters: head backward, pooling backward, then the encoder from d loss / d hidden."""
        if self._saved is None:
            raise RuntimeError("backward() needs a training-mode forward with labels")
        dlogits, pooled, act, argmax, frame_lens, F, dtype, seed = self._saved
        if grad_scale != 1.0:
            dlogits = dlogits * grad_scale
        with torch.cuda.device(self.device):
            grads = [self.head_grad(n) for n in HEAD_PARAMS]
            dpooled = hip.cls_head_bwd(dlogits, pooled, act, self.head_param(HEAD_PARAMS[0]), self.head_param(HEAD_PARAMS[2]), *grads,
                                       drop_p=self.config.final_dropout, seed=seed, training=True)
            dhidden = hip.pool_bwd(dpooled, argmax, frame_lens, F, self.config.pooling_mode, dtype)
        self._saved = None
        self.encoder.backward_hidden(dhidden)

    def named_grads(self):
        g = {n: t for n, t in self.encoder.named_grads().items() if not n.startswith("lm_head.")}
        g.update({n: self.head_grad(n) for n in HEAD_PARAMS})
        return g


# ---------------------------------------------------------------------------------------------------------- model folders
def _read_state_dict(folder: str) -> Dict[str, torch.Tensor]:
    st = os.path.join(folder, "model.safetensors")
    if os.path.isfile(st):
        from safetensors.torch import load_file
        return load_file(st)
    return torch.load(os.path.join(folder, "pytorch_model.bin"), map_location="cpu", weights_only=True)


def load_classifier(folder: str, device: str = "cuda:0", exact: bool = False, freeze_feature_encoder: bool = True) -> SpeechClassifier:
    """A model folder in the HuggingFace layout (``config.json`` + ``model.safetensors`` / ``pytorch_model.bin``) whose encoder
    parameters are prefixed ``wav2vec2.`` or ``hubert.`` -> :class:`SpeechClassifier` in eval mode.  Parameters absent from the
    checkpoint (``masked_spec_embed`` of a model saved without SpecAugment) keep their initial value."""
    with open(os.path.join(folder, "config.json")) as f:
        d = json.load(f)
    raw = _read_state_dict(folder)
    prefix = next((p for p in _ENCODER_PREFIXES if any(k.startswith(p) for k in raw)), None)
    if prefix is None:
        raise ValueError(f"{folder}: no parameter is prefixed {' or '.join(_ENCODER_PREFIXES)}")
    d = dict(d, model_type=prefix[:-1])
    cfg = SpeechClassifierConfig.from_hf_dict(d)
    model = SpeechClassifier(cfg, device=device, exact=exact, freeze_feature_encoder=freeze_feature_encoder)
    sd = {}
    for k, v in raw.items():
        if k.startswith(prefix):
            k = "wav2vec2." + k[len(prefix):]
        sd[_LEGACY.get(k, k)] = v
    known = set(model.encoder.layout) | set(HEAD_PARAMS)
    model.load_state_dict({k: v for k, v in sd.items() if k in known}, strict=False)
    absent = [n for n in HEAD_PARAMS if n not in sd]
    if absent:
        raise ValueError(f"{folder}: the checkpoint has no {absent[0]} (not a speech-classification model)")
    return model.eval()


def save_classifier(model: SpeechClassifier, folder: str):
    """Write the folder back, encoder parameters under the prefix the model was read with (``config.model_type``)."""
    os.makedirs(folder, exist_ok=True)
    prefix = model.config.model_type + "."
    with open(os.path.join(folder, "config.json"), "w") as f:
        json.dump(model.config.to_dict(), f, indent=1)
    from safetensors.torch import save_file
    sd = {(prefix + k[len("wav2vec2."):] if k.startswith("wav2vec2.") else k): v.contiguous() for k, v in model.state_dict().items()}
    save_file(sd, os.path.join(folder, "model.safetensors"))
    with open(os.path.join(folder, "preprocessor_config.json"), "w") as f:
        json.dump({"do_normalize": True, "feature_size": 1, "padding_value": 0.0, "sampling_rate": 16000,
                   "return_attention_mask": model.config.feat_extract_norm == "layer"}, f, indent=1)


# ---------------------------------------------------------------------------------------------------------- predict_gender
DEFAULT_GENDER_MODEL = "m3hrdadfi/hubert-base-persian-speech-gender-recognition"  # the reference's default (a hub id)
_OUTPUT_TYPES = ("best", "scores")
_gender_models: Dict[tuple, tuple] = {}  # (folder, device) -> (SpeechClassifier, {class id: "m" | "f"})


def _resample(x: torch.Tensor, orig_sr: int, new_sr: int) -> torch.Tensor:
    """[1, T] fp32 on the device -> [1, ceil(new * T / orig)] through ``ssak_resample_sinc`` (torchaudio's windowed-sinc formula)."""
    import ctypes as C
    o, n, w, taps = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    hip.check(hip.lib.ssak_resample_plan(orig_sr, new_sr, C.byref(o), C.byref(n), C.byref(w), C.byref(taps)))
    host = torch.empty(n.value * taps.value, dtype=torch.float32)
    hip.check(hip.lib.ssak_resample_table(orig_sr, new_sr, C.c_void_p(host.data_ptr())))
    table = host.to(x.device)
    B, T = x.shape
    Tout = -(-(n.value * T) // o.value)
    out = torch.empty((B, Tout), dtype=torch.float32, device=x.device)
    hip.check(hip.lib.ssak_resample_sinc(hip.ptr(x), None, B, T, orig_sr, new_sr, hip.ptr(table), hip.ptr(out), Tout, None, hip.stream()))
    return out


def _gender_model(folder: str, device: str):
    """The classifier of ``folder`` on ``device`` and its class names in lower case, loaded once per (folder, device)."""
    key = (folder, str(device))
    if key not in _gender_models:
        if not os.path.isdir(folder):
            raise FileNotFoundError(f"{folder}: not a model folder (nothing is downloaded: pass a local folder in the HuggingFace layout)")
        net = load_classifier(folder, device=device)
        names = {i: name.lower() for i, name in sorted((net.config.id2label or {}).items())}
        # a gender model has the two classes "m" and "f" (any case) and no third: the asserts the reference makes
        assert len(names) == 2, f"{folder}: a gender model has two labels, id2label has {len(names)}: {names}"
        for wanted, meaning in (("f", "female"), ("m", "male")):
            assert wanted in names.values(), f"{folder}: no label {wanted!r} ({meaning}) in id2label {names}"
        _gender_models[key] = (net, names)
    return _gender_models[key]


def predict_gender(waveform, sample_rate: int = 16_000, device: str = "cuda:0", model: str = DEFAULT_GENDER_MODEL, output_type: str = "best"):
    """The gender of the one speaker of ``waveform``, with the call and the answers of the reference's ``predict_gender``
    (ssak/utils/gender.py:242-301).

    ``waveform``: 1-D samples at ``sample_rate`` (anything but 16 kHz is resampled on the device).  ``model``: a local model
    FOLDER in the HuggingFace layout -- the reference's default is a hub id, and this library downloads nothing.
    ``output_type``: ``"best"`` returns ``"m"`` or ``"f"``; ``"scores"`` returns both probabilities, ``{"f": 0.1, "m": 0.9}``,
    in class order."""
    if output_type not in _OUTPUT_TYPES:
        raise ValueError(f"output_type {output_type!r}: one of {_OUTPUT_TYPES}")
    net, names = _gender_model(model, device)
    x = torch.as_tensor(np.asarray(waveform, dtype=np.float32)).reshape(1, -1).to(net.device).contiguous()
    with torch.cuda.device(net.device):
        if sample_rate != 16_000:
            x = _resample(x, int(sample_rate), 16_000)
        x = hip.wave_normalize(x)  # Wav2Vec2FeatureExtractor(do_normalize=True): zero mean, unit variance
    probs = net(x).probs[0].tolist()
    scores = {names[i]: p for i, p in enumerate(probs)}
    return scores if output_type == "scores" else max(scores, key=scores.get)


def main(argv=None):
    """``python -m ssak_amd.classify AUDIO... --model DIR [--start S --end E]``: one JSON object of scores per file."""
    import argparse

    from .data import load_audio
    ap = argparse.ArgumentParser(prog="python -m ssak_amd.classify", description="Score each audio file as male / female speech.")
    ap.add_argument("audio", nargs="+", metavar="AUDIO", help="16 kHz PCM WAV file(s)")
    ap.add_argument("--model", required=True, metavar="DIR", help="speech-classification model folder (HuggingFace layout)")
    ap.add_argument("--start", type=float, metavar="S", help="score the file from this second on")
    ap.add_argument("--end", type=float, metavar="E", help="score the file up to this second")
    ap.add_argument("--device", default="cuda:0", help="GPU to run on")
    args = ap.parse_args(argv)
    for path in args.audio:
        samples = load_audio(path, start=args.start, end=args.end)
        print(json.dumps(predict_gender(samples, device=args.device, model=args.model, output_type="scores"), indent=2))


if __name__ == "__main__":
    main()
