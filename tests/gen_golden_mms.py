"""Generate tests/golden/mms_tiny.npz: a tiny MMS-style wav2vec2 CTC model (language adapters, nested vocabulary) and what
``transformers`` computes with it, in fp32 on the CPU, offline, from local folders only.

Run once on the CPU, where ``transformers`` is installed:  python tests/gen_golden_mms.py
(``write_folder(npz, DIR)`` below writes the stored model as the HuggingFace-layout folder ``ssak_amd.checkpoint.load_pretrained``
and ``python -m ssak_amd.infer --model DIR --language X`` read; it needs no ``transformers``.)

The model is ``transformers.Wav2Vec2ForCTC`` with the shapes of the tiny XLSR fixture (hidden 64, 2 layers, 2 heads, layer-norm
feature encoder, stable LayerNorm), ``adapter_attn_dim = 16`` and every regulariser off; its weights are the seeded ones of
``oracle.w2v2_ref.init_params``, the adapter tensors and the two heads seeded here.  Two languages: ``eng`` (16 tokens, the
default: what model.safetensors and ``target_lang`` of tokenizer_config.json hold) and ``fra`` (21 tokens: another head size, and
not a multiple of 8).  The heads' biases push ``<s>``, ``</s>`` and ``<unk>`` far down so that no frame decodes to them: the
engine's tokenizer drops such tokens and ``Wav2Vec2CTCTokenizer`` prints them, which is not what this fixture is about.

Stored: the configuration and the nested vocabulary (JSON), every weight of the default load (``w/<name>``), each language's
adapter file (``a/<lang>/<name>``), two raw waveforms of different lengths (so that the attention mask matters; their values are
ones 16-bit PCM holds exactly, so a test can hand them over as .wav files), the normalised padded input, HF's fp32 logits for
the no-language load and after ``load_adapter`` of each language, and ``Wav2Vec2CTCTokenizer``'s greedy transcripts of each utterance's VALID frames (the engine's inference path decodes the frames
of the utterance, not those of the padding).
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(HERE, "golden", "mms_tiny.npz")
SEED, ADAPTER_DIM = 69, 16
SPECIALS = ["<pad>", "<s>", "</s>", "<unk>", "|"]
LANGS = {"eng": SPECIALS + list("abcdefghijk"), "fra": SPECIALS + list("abcdefghijklmé") + ["à", "ç"]}
DEFAULT_LANG = "eng"
SAMPLES = (4000, 3250)


def write_folder(npz, folder: str, bin_for=()) -> str:
    """The model stored in the golden file as a HuggingFace-layout folder: config.json, vocab.json (nested),
    tokenizer_config.json (target_lang), preprocessor_config.json, model.safetensors and one adapter.<lang>.safetensors per
    language -- ``adapter.<lang>.bin`` (torch.save) instead for the languages in ``bin_for``."""
    import torch
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    for name, key in (("config.json", "config_json"), ("vocab.json", "vocab_json"), ("tokenizer_config.json", "tokenizer_config_json"),
                      ("preprocessor_config.json", "preprocessor_config_json")):
        with open(os.path.join(folder, name), "w") as f:
            f.write(str(npz[key]))
    save_file({k[2:]: torch.from_numpy(np.array(npz[k])) for k in npz.files if k.startswith("w/")}, os.path.join(folder, "model.safetensors"))
    for lang in json.loads(str(npz["vocab_json"])):
        sd = {k.split("/", 2)[2]: torch.from_numpy(np.array(npz[k])) for k in npz.files if k.startswith(f"a/{lang}/")}
        if lang in bin_for:
            torch.save(sd, os.path.join(folder, f"adapter.{lang}.bin"))
        else:
            save_file(sd, os.path.join(folder, f"adapter.{lang}.safetensors"))
    return folder


def main():
    import torch
    from transformers import Wav2Vec2Config, Wav2Vec2CTCTokenizer, Wav2Vec2ForCTC

    from oracle import w2v2_ref as R
    torch.manual_seed(0)
    V0 = len(LANGS[DEFAULT_LANG])
    oc = R.W2V2Config.tiny(num_attention_heads=2, feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True,
                           vocab_size=V0).deterministic()
    H, L = oc.hidden_size, oc.num_hidden_layers
    kw = {k: v for k, v in oc.to_hf_kwargs().items() if k not in ("initializer_range",)}
    hf_cfg = Wav2Vec2Config(**kw, adapter_attn_dim=ADAPTER_DIM)
    model = Wav2Vec2ForCTC(hf_cfg).eval().to(torch.float32)
    base = R.init_params(oc, SEED)

    rng = np.random.default_rng(SEED)
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    adapters = {}
    for lang, toks in LANGS.items():
        sd = {}
        for l in range(L):
            p = f"wav2vec2.encoder.layers.{l}.adapter_layer."
            sd[p + "norm.weight"] = f32(1.0 + 0.2 * rng.standard_normal(H))
            sd[p + "norm.bias"] = f32(0.1 * rng.standard_normal(H))
            sd[p + "linear_1.weight"] = f32(rng.standard_normal((ADAPTER_DIM, H)) / np.sqrt(H))
            sd[p + "linear_1.bias"] = f32(0.3 * rng.standard_normal(ADAPTER_DIM))
            sd[p + "linear_2.weight"] = f32(rng.standard_normal((H, ADAPTER_DIM)) / np.sqrt(ADAPTER_DIM))
            sd[p + "linear_2.bias"] = f32(0.1 * rng.standard_normal(H))
        sd["lm_head.weight"] = f32(rng.standard_normal((len(toks), H)) / np.sqrt(H))
        bias = 0.1 * rng.standard_normal(len(toks))
        bias[1:4] = -20.0  # <s>, </s>, <unk> never win a frame (see the module docstring)
        sd["lm_head.bias"] = f32(bias)
        adapters[lang] = sd
    full = dict(base)
    full.update(adapters[DEFAULT_LANG])
    if "wav2vec2.masked_spec_embed" not in model.state_dict():
        full.pop("wav2vec2.masked_spec_embed")
    model.load_state_dict(full, strict=True)

    vocab = {lang: {t: i for i, t in enumerate(toks)} for lang, toks in LANGS.items()}
    # (values 16-bit PCM holds exactly, so that the waveforms survive a .wav file unchanged: the inference entry points read files)
    waves = [(np.round((0.1 * rng.standard_normal(n) + 0.01) * 32768.0) / 32768.0).astype(np.float32) for n in SAMPLES]
    lens = np.array(SAMPLES, dtype=np.int32)
    x = R.zero_mean_unit_var_norm(waves)
    mask = (np.arange(x.shape[1])[None, :] < lens[:, None]).astype(np.int64)
    pre_cfg = {"do_normalize": True, "feature_size": 1, "padding_value": 0.0, "sampling_rate": 16000, "return_attention_mask": True,
               "feature_extractor_type": "Wav2Vec2FeatureExtractor"}

    with tempfile.TemporaryDirectory() as tmp:
        # the folder as transformers itself writes it, then read back: everything below comes from local files
        from safetensors.torch import save_file
        model.save_pretrained(tmp, safe_serialization=True)
        with open(os.path.join(tmp, "vocab_in.json"), "w") as f:
            json.dump(vocab, f, ensure_ascii=False)
        tok = Wav2Vec2CTCTokenizer(os.path.join(tmp, "vocab_in.json"), target_lang=DEFAULT_LANG)
        tok.save_pretrained(tmp)
        for lang, sd in adapters.items():
            save_file(sd, os.path.join(tmp, f"adapter.{lang}.safetensors"))
        with open(os.path.join(tmp, "tokenizer_config.json")) as f:
            assert json.load(f).get("target_lang") == DEFAULT_LANG
        tok = Wav2Vec2CTCTokenizer.from_pretrained(tmp)
        assert tok.target_lang == DEFAULT_LANG
        hf = Wav2Vec2ForCTC.from_pretrained(tmp).eval()
        xt, mt = torch.from_numpy(x), torch.from_numpy(mask)
        flens = hf._get_feat_extract_output_lengths(torch.from_numpy(lens.astype(np.int64))).numpy().astype(np.int32)
        logits, texts = {}, {}
        with torch.no_grad():
            logits["default"] = hf(xt, attention_mask=mt).logits.numpy()
            for lang in ("fra", "eng"):  # another head size first, then back
                hf.load_adapter(lang)
                tok.set_target_lang(lang)
                lg = hf(xt, attention_mask=mt).logits
                assert lg.shape[-1] == len(LANGS[lang])
                logits[lang] = lg.numpy()
                ids = lg.argmax(-1)
                texts[lang] = [tok.decode(ids[b, :int(flens[b])]) for b in range(len(waves))]
        assert np.abs(logits["default"] - logits[DEFAULT_LANG]).max() < 1e-6  # the default load IS the default language
        sd_file = {k: v for k, v in hf.state_dict().items()}
    weights = {k: v.numpy() for k, v in full.items()}
    if "wav2vec2.masked_spec_embed" not in weights:
        weights["wav2vec2.masked_spec_embed"] = base["wav2vec2.masked_spec_embed"].numpy()
    del sd_file
    cfg_json = hf_cfg.to_dict()
    keep = set(kw) | {"adapter_attn_dim", "model_type", "architectures", "pad_token_id"}
    cfg_json = {k: v for k, v in cfg_json.items() if k in keep}
    cfg_json["architectures"] = ["Wav2Vec2ForCTC"]
    out = {"w/" + k: np.asarray(v, dtype=np.float32) for k, v in weights.items()}
    for lang, sd in adapters.items():
        out.update({f"a/{lang}/{k}": v.numpy() for k, v in sd.items()})
    np.savez_compressed(GOLDEN, config_json=np.array(json.dumps(cfg_json)), vocab_json=np.array(json.dumps(vocab, ensure_ascii=False)),
                        tokenizer_config_json=np.array(json.dumps({"target_lang": DEFAULT_LANG, "pad_token": "<pad>", "unk_token": "<unk>",
                                                                   "word_delimiter_token": "|", "tokenizer_class": "Wav2Vec2CTCTokenizer"})),
                        preprocessor_config_json=np.array(json.dumps(pre_cfg)), default_lang=np.array(DEFAULT_LANG),
                        wave0=waves[0], wave1=waves[1], x=x, lens=lens, frame_lens=flens,
                        logits_default=logits["default"], logits_eng=logits["eng"], logits_fra=logits["fra"],
                        texts_json=np.array(json.dumps(texts, ensure_ascii=False)), **out)
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes; frames {flens.tolist()}; transcripts {texts}")


if __name__ == "__main__":
    main()
