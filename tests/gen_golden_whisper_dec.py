"""Generate tests/golden/whisper_dec_tiny.npz: a tiny Whisper text decoder and what ``transformers`` computes with it, in float64
on the CPU, offline.

Run once on the CPU, where ``transformers`` is installed:  python tests/gen_golden_whisper_dec.py
(``write_folder(npz, DIR)`` below writes the stored decoder plus seeded random encoder weights as the HuggingFace-layout folder
``ssak_amd.whisper_seq2seq.WhisperSeq2Seq.from_pretrained`` reads; it needs no ``transformers``.)

The model is ``transformers.WhisperForConditionalGeneration`` with d_model 128, 2 heads of 64, 2 decoder layers, ffn 256, a
vocabulary of 127 tokens (not a multiple of 8) of which 6 are language tokens, 32 target positions and 50 encoder frames.  Only
the DECODER's weights are stored, rounded to bf16 and kept as uint16 bit patterns: that halves the file and takes the weight
rounding out of the GPU tests' bars (``w/<transformers name>``).  Stored with them: an encoder output ``enc`` [3, 50, 128] (bf16
bit patterns too), tokens [3, 12] with lengths (12, 2, 7), encoder lengths (50, 50, 23), transformers' logits of every position
and its cross-entropy (``.loss``) per utterance and over the batch, and the language probabilities of
``whisper.decoding.detect_language``'s rule (one position after ``<|startoftranscript|>``, non-language tokens masked).
transformers' Whisper decoder takes no encoder mask (its encoder always fills 30 s), so each utterance runs alone on the first
``enc_lens[b]`` frames of its encoder output -- the same function as masking the other keys.

The generator ASSERTS that, for every utterance, the top language probability leads the second by at least 0.2: the seed below
is the first for which it does (the language rows of the embedding are scaled up so that the language softmax is not flat).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import whisper_decoder_ref as WR  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "whisper_dec_tiny.npz")
D, NH, LAYERS, FFN, V, MAX_POS, S, MELS = 128, 2, 2, 256, 127, 32, 50, 80
EOT, SOT, LANG0 = 100, 101, 102
LANGS = ("en", "fr", "de", "es", "it", "pt")
TRANSLATE, TRANSCRIBE, NO_TIMESTAMPS = 108, 109, 110
B, L = 3, 12
LENS, ENC_LENS = (12, 2, 7), (50, 50, 23)
MARGIN = 0.2
LANG_ROW_SCALE = 4.0


def config_dict(max_source_positions: int = S, encoder_layers: int = 1) -> dict:
    return {"architectures": ["WhisperForConditionalGeneration"], "model_type": "whisper", "vocab_size": V, "num_mel_bins": MELS, "d_model": D,
            "encoder_layers": encoder_layers, "encoder_attention_heads": NH, "encoder_ffn_dim": FFN, "decoder_layers": LAYERS,
            "decoder_attention_heads": NH, "decoder_ffn_dim": FFN, "max_source_positions": max_source_positions,
            "max_target_positions": MAX_POS, "activation_function": "gelu", "scale_embedding": False, "tie_word_embeddings": True,
            "dropout": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0, "encoder_layerdrop": 0.0, "decoder_layerdrop": 0.0,
            "pad_token_id": EOT, "bos_token_id": EOT, "eos_token_id": EOT, "decoder_start_token_id": SOT, "is_encoder_decoder": True}


def generation_config_dict() -> dict:
    return {"decoder_start_token_id": SOT, "eos_token_id": EOT, "pad_token_id": EOT, "is_multilingual": True,
            "lang_to_id": {f"<|{c}|>": LANG0 + i for i, c in enumerate(LANGS)},
            "task_to_id": {"translate": TRANSLATE, "transcribe": TRANSCRIBE}, "no_timestamps_token_id": NO_TIMESTAMPS}


def decoder_param_shapes() -> dict:
    sh = {"embed_tokens.weight": (V, D), "embed_positions.weight": (MAX_POS, D), "layer_norm.weight": (D,), "layer_norm.bias": (D,)}
    for l in range(LAYERS):
        p = f"layers.{l}."
        for attn in ("self_attn", "encoder_attn"):
            for proj in ("q_proj", "k_proj", "v_proj", "out_proj"):
                sh[p + f"{attn}.{proj}.weight"] = (D, D)
                if proj != "k_proj":
                    sh[p + f"{attn}.{proj}.bias"] = (D,)
            sh[p + f"{attn}_layer_norm.weight"] = (D,)
            sh[p + f"{attn}_layer_norm.bias"] = (D,)
        sh.update({p + "fc1.weight": (FFN, D), p + "fc1.bias": (FFN,), p + "fc2.weight": (D, FFN), p + "fc2.bias": (D,),
                   p + "final_layer_norm.weight": (D,), p + "final_layer_norm.bias": (D,)})
    return {"model.decoder." + k: v for k, v in sh.items()}


def encoder_param_shapes(max_source_positions: int, encoder_layers: int) -> dict:
    sh = {"conv1.weight": (D, MELS, 3), "conv1.bias": (D,), "conv2.weight": (D, D, 3), "conv2.bias": (D,),
          "embed_positions.weight": (max_source_positions, D), "layer_norm.weight": (D,), "layer_norm.bias": (D,)}
    for l in range(encoder_layers):
        p = f"layers.{l}."
        for proj in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sh[p + f"self_attn.{proj}.weight"] = (D, D)
            if proj != "k_proj":
                sh[p + f"self_attn.{proj}.bias"] = (D,)
        sh.update({p + "self_attn_layer_norm.weight": (D,), p + "self_attn_layer_norm.bias": (D,), p + "fc1.weight": (FFN, D),
                   p + "fc1.bias": (FFN,), p + "fc2.weight": (D, FFN), p + "fc2.bias": (D,), p + "final_layer_norm.weight": (D,),
                   p + "final_layer_norm.bias": (D,)})
    return {"model.encoder." + k: v for k, v in sh.items()}


def draw(shapes: dict, rng) -> dict:
    """Seeded weights: matrices N(0, 0.08^2) (large enough that attention and the softmax over the vocabulary are not flat),
    LayerNorm scales around 1, biases and LayerNorm shifts N(0, 0.05^2); rounded to bf16."""
    out = {}
    for name, shape in shapes.items():
        if "layer_norm.weight" in name:
            w = 1.0 + 0.1 * rng.standard_normal(shape)
        elif name.endswith(".bias"):
            w = 0.05 * rng.standard_normal(shape)
        else:
            w = 0.08 * rng.standard_normal(shape)
        out[name] = WR.bf16_round(w)
    return out


def make_model(seed: int):
    rng = np.random.default_rng(seed)
    w = draw(decoder_param_shapes(), rng)
    E = w["model.decoder.embed_tokens.weight"]
    E[LANG0:LANG0 + len(LANGS)] = WR.bf16_round(E[LANG0:LANG0 + len(LANGS)] * LANG_ROW_SCALE)
    enc = WR.bf16_round(rng.standard_normal((B, S, D)))
    tokens = rng.integers(0, EOT, size=(B, L))
    tokens[:, 0] = SOT
    for b, n in enumerate(LENS):  # <|startoftranscript|> text ... <|endoftext|>, then padding
        if n > 1:
            tokens[b, n - 1] = EOT
        tokens[b, n:] = EOT
    return w, enc, tokens


def language_margin(w, enc):
    lang_ids = [LANG0 + i for i in range(len(LANGS))]
    probs = np.zeros((B, len(LANGS)))
    for b in range(B):
        lg = WR.decoder_logits(w, NH, LAYERS, enc[b:b + 1, :ENC_LENS[b]], np.array([[SOT]]))
        probs[b] = WR.language_probs(lg[:, 0], lang_ids)[1][0]
    top = np.sort(probs, -1)
    return probs, float((top[:, -1] - top[:, -2]).min())


def write_folder(npz, folder: str, max_source_positions: int = S, encoder_layers: int = 1, encoder_seed: int = 7, config_overrides=None,
                 extra_tensors=None) -> str:
    """The decoder stored in the golden file plus seeded random ENCODER weights as a HuggingFace-layout folder: config.json,
    generation_config.json, model.safetensors (fp32).  ``config_overrides`` / ``extra_tensors`` let a test write a folder that
    the loader must refuse."""
    import torch
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    cfg = dict(config_dict(max_source_positions, encoder_layers), **(config_overrides or {}))
    with open(os.path.join(folder, "config.json"), "w") as f:
        json.dump(cfg, f, indent=1)
    with open(os.path.join(folder, "generation_config.json"), "w") as f:
        f.write(str(npz["generation_config_json"]))
    sd = {k[2:]: torch.from_numpy(WR.bf16_from_bits(npz[k]).astype(np.float32)) for k in npz.files if k.startswith("w/")}
    enc = draw(encoder_param_shapes(max_source_positions, encoder_layers), np.random.default_rng(encoder_seed))
    sd.update({k: torch.from_numpy(v.astype(np.float32)) for k, v in enc.items()})
    sd.update(extra_tensors or {})
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(folder, "model.safetensors"))
    return folder


def hf_model(w):
    """transformers.WhisperForConditionalGeneration in float64 carrying the decoder weights ``w``."""
    import torch
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    cfg = {k: v for k, v in config_dict().items() if k not in ("architectures", "model_type")}
    model = WhisperForConditionalGeneration(WhisperConfig(**cfg)).double().eval()
    sd = model.state_dict()
    for k, v in w.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float64))
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    model.load_state_dict(sd)
    return model


def hf_forward(model, enc, tokens, labels):
    """(logits [B, L, V], loss) of transformers on decoder_input_ids = tokens with the encoder output given."""
    import torch
    with torch.no_grad():
        out = model(encoder_outputs=(torch.from_numpy(np.asarray(enc, dtype=np.float64)),), decoder_input_ids=torch.from_numpy(np.asarray(tokens)),
                    labels=torch.from_numpy(np.asarray(labels)), use_cache=False)
    return out.logits.numpy(), float(out.loss)


def main():
    seed = 0
    while True:
        w, enc, tokens = make_model(seed)
        lang_probs, margin = language_margin(w, enc)
        if margin >= MARGIN:
            break
        seed += 1
    assert margin >= MARGIN, margin  # the GPU test demands the arg-max for all utterances
    model = hf_model(w)
    labels = WR.shifted_targets(tokens, LENS)
    logits = np.zeros((B, L, V))
    loss = np.zeros(B)
    for b in range(B):
        logits[b], loss[b] = hf_forward(model, enc[b:b + 1, :ENC_LENS[b]], tokens[b:b + 1], labels[b:b + 1])
    n = (labels >= 0).sum(-1)
    hf_lang = WR.language_probs(logits[:, 0], [LANG0 + i for i in range(len(LANGS))])[1]  # tokens[:, 0] is <|startoftranscript|>
    assert np.abs(hf_lang - lang_probs).max() < 1e-10
    lang_probs = hf_lang
    out = {"w/" + k: WR.bf16_bits(v) for k, v in w.items()}
    out.update(config_json=json.dumps(config_dict()), generation_config_json=json.dumps(generation_config_dict()), seed=seed,
               enc=WR.bf16_bits(enc), tokens=tokens.astype(np.int32), lens=np.array(LENS, dtype=np.int32),
               enc_lens=np.array(ENC_LENS, dtype=np.int32), hf_logits=logits, hf_loss=loss, hf_batch_loss=float((loss * n).sum() / n.sum()),
               lang_ids=np.array([LANG0 + i for i in range(len(LANGS))], dtype=np.int32), lang_codes=np.array(LANGS), lang_probs=lang_probs)
    np.savez_compressed(GOLDEN, **out)
    print(f"seed {seed}: language margin {margin:.3f}, probabilities\n{np.round(lang_probs, 3)}\nloss {loss}, batch {out['hf_batch_loss']:.6f}; "
          f"{os.path.getsize(GOLDEN)} bytes -> {GOLDEN}")


if __name__ == "__main__":
    main()
