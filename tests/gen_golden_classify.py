"""Generate tests/golden/classify_tiny.npz: a tiny HuBERT speech-classification model and what it computes, in fp32 on the CPU.

Run once on the CPU, where ``transformers`` is installed:  python tests/gen_golden_classify.py
(``python tests/gen_golden_classify.py --folder DIR`` instead writes the stored model as a HuggingFace-layout folder, which is
what ``ssak_amd.classify.load_classifier`` and ``python -m ssak_amd.classify --model DIR`` read; it needs no ``transformers``.)

The encoder is ``transformers.HubertModel`` with the shapes of ``oracle.w2v2_ref.W2V2Config.tiny()`` and every regulariser off,
its weights the seeded ones of ``oracle.w2v2_ref.init_params`` under HuBERT names.  The classification model of the reference
(ssak/utils/gender.py, ``HubertForSpeechClassification``) is not part of ``transformers``; its head is restated here from its
description: the last hidden state, mean over time (all frames), ``Linear(H, H) -> tanh -> Linear(H, num_labels)`` (dropout
off), softmax, mean cross-entropy.  Stored: the weights (``w/<HuBERT state-dict name>``), the configuration (JSON), a
2-utterance input (raw and normalised), labels, logits, probs, loss, and the gradients of the head and of the last encoder
layer (``g/<name>``).
"""
from __future__ import annotations

import dataclasses
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(HERE, "golden", "classify_tiny.npz")
SEED, NUM_LABELS, SAMPLES = 69, 2, 8000
ID2LABEL = {0: "F", 1: "M"}
HEAD = ("classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight", "classifier.out_proj.bias")


def write_folder(npz, folder: str) -> str:
    """The model stored in the golden file as a HuggingFace-layout folder (config.json + model.safetensors)."""
    import torch
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "config.json"), "w") as f:
        f.write(str(npz["config_json"]))
    save_file({k[2:]: torch.from_numpy(np.array(npz[k])) for k in npz.files if k.startswith("w/")}, os.path.join(folder, "model.safetensors"))
    return folder


def main():
    import torch
    from transformers import HubertConfig, HubertModel

    from oracle import w2v2_ref as R
    torch.manual_seed(0)
    oc = R.W2V2Config.tiny().deterministic()
    H = oc.hidden_size
    kw = {k: v for k, v in oc.to_hf_kwargs().items() if k not in ("initializer_range",)}
    hf_cfg = HubertConfig(**kw, feat_proj_layer_norm=True, conv_pos_batch_norm=False, num_labels=NUM_LABELS)
    model = HubertModel(hf_cfg).eval().to(torch.float32)

    p = R.init_params(oc, SEED)
    enc = {k[len("wav2vec2."):]: v for k, v in p.items() if k.startswith("wav2vec2.")}
    if "masked_spec_embed" not in model.state_dict():
        enc.pop("masked_spec_embed")  # HubertModel has none with SpecAugment off
    model.load_state_dict(enc, strict=True)
    rng = np.random.default_rng(SEED)
    head = {HEAD[0]: rng.standard_normal((H, H)) / np.sqrt(H), HEAD[1]: 0.1 * rng.standard_normal(H),
            HEAD[2]: rng.standard_normal((NUM_LABELS, H)) / np.sqrt(H), HEAD[3]: 0.1 * rng.standard_normal(NUM_LABELS)}
    head = {k: torch.tensor(v, dtype=torch.float32, requires_grad=True) for k, v in head.items()}

    wave = (0.1 * rng.standard_normal((2, SAMPLES))).astype(np.float32) + np.float32(0.01)
    x = R.zero_mean_unit_var_norm(list(wave))
    labels = np.array([1, 0], dtype=np.int64)
    for q in model.parameters():
        q.requires_grad_(True)
    hidden = model(torch.from_numpy(x)).last_hidden_state
    pooled = hidden.mean(dim=1)
    act = torch.tanh(torch.nn.functional.linear(pooled, head[HEAD[0]], head[HEAD[1]]))
    logits = torch.nn.functional.linear(act, head[HEAD[2]], head[HEAD[3]])
    loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(labels))
    loss.backward()
    probs = torch.softmax(logits, dim=1)

    last = f"encoder.layers.{oc.num_hidden_layers - 1}."
    grads = {"hubert." + n: q.grad for n, q in model.named_parameters() if n.startswith(last)}
    grads.update({k: v.grad for k, v in head.items()})
    cfg_json = dict(dataclasses.asdict(oc), model_type="hubert", architectures=["HubertForSpeechClassification"],
                    pooling_mode="mean", num_labels=NUM_LABELS, id2label={str(k): v for k, v in ID2LABEL.items()},
                    label2id={v: k for k, v in ID2LABEL.items()}, feat_proj_layer_norm=True, conv_pos_batch_norm=False)
    for k in ("conv_dim", "conv_kernel", "conv_stride"):
        cfg_json[k] = list(cfg_json[k])
    out = {"w/hubert." + k: v.detach().numpy() for k, v in model.state_dict().items()}
    out.update({"w/" + k: v.detach().numpy() for k, v in head.items()})
    out.update({"g/" + k: v.numpy() for k, v in grads.items()})
    np.savez_compressed(GOLDEN, config_json=np.array(json.dumps(cfg_json)), wave=wave, x=x, labels=labels,
                        logits=logits.detach().numpy(), probs=probs.detach().numpy(), loss=np.float32(loss.item()),
                        hidden=hidden.detach().numpy(), **out)
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes; logits {logits.detach().numpy().tolist()} probs {probs.detach().numpy().tolist()} "
          f"loss {loss.item():.6f}; {len(grads)} gradient tensors")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--folder":
        write_folder(np.load(GOLDEN, allow_pickle=False), sys.argv[2])
    else:
        main()
