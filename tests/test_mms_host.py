"""CPU: the host side of MMS language adapters -- the nested vocabulary of ``CharTokenizer``, ``--language`` resolution, the
configuration field and the key-set check of an adapter file (``Wav2Vec2ForCTC.load_adapter`` reads through it); no GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_mms as GM  # noqa: E402

from ssak_amd.checkpoint import adapter_file, adapter_param_names, read_adapter_state  # noqa: E402
from ssak_amd.config import Wav2Vec2Config  # noqa: E402
from ssak_amd.data import CharTokenizer  # noqa: E402
from ssak_amd.infer import resolve_language  # noqa: E402

NESTED = {"eng": {"<pad>": 0, "<unk>": 1, "|": 2, "a": 3, "b": 4}, "fra": {"<pad>": 0, "<unk>": 1, "|": 2, "a": 3, "é": 4, "ç": 5},
          "fro": {"<pad>": 0, "<unk>": 1, "|": 2, "z": 3}}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "mms_tiny.npz"), allow_pickle=False)


def _write(tmp_path, vocab, tok_cfg=None):
    (tmp_path / "vocab.json").write_text(json.dumps(vocab, ensure_ascii=False))
    if tok_cfg is not None:
        (tmp_path / "tokenizer_config.json").write_text(json.dumps(tok_cfg))
    return str(tmp_path / "vocab.json")


def test_nested_vocabulary(tmp_path):
    tok = CharTokenizer.from_vocab_json(_write(tmp_path, NESTED, {"target_lang": "fra", "pad_token": "<pad>"}))
    assert tok.languages == ["eng", "fra", "fro"] and tok.target_lang == "fra"
    assert tok.vocab == ["<pad>", "<unk>", "|", "a", "é", "ç"] and len(tok) == 6 and tok.pad_token_id == 0
    assert tok.decode([3, 3, 0, 4, 2, 5]) == "aé ç" and tok.encode("é a") == [4, 2, 3]
    tok.set_target_lang("eng")
    assert tok.target_lang == "eng" and tok.vocab == ["<pad>", "<unk>", "|", "a", "b"] and tok.encode("é") == [1]
    with pytest.raises(ValueError, match="deu does not exist. Choose one of eng, fra, fro."):
        tok.set_target_lang("deu")
    assert tok.target_lang == "eng"
    # save writes back what it read: the nested table and the language in use
    out = tmp_path / "saved"
    out.mkdir()
    tok.save(str(out))
    assert json.loads((out / "vocab.json").read_text()) == NESTED
    again = CharTokenizer.from_vocab_json(str(out / "vocab.json"))
    assert again.target_lang == "eng" and again.vocab == tok.vocab


def test_nested_vocabulary_without_tokenizer_config_uses_the_first_language(tmp_path):
    tok = CharTokenizer.from_vocab_json(_write(tmp_path, NESTED))
    assert tok.target_lang == "eng"


def test_flat_vocabulary_is_what_it_was(tmp_path):
    flat = {"<pad>": 0, "<unk>": 1, "|": 2, "b": 4, "a": 3}
    tok = CharTokenizer.from_vocab_json(_write(tmp_path, flat))
    assert tok.vocab == ["<pad>", "<unk>", "|", "a", "b"] and tok.languages == [] and tok.target_lang is None
    with pytest.raises(ValueError, match="is not a multi-lingual"):
        tok.set_target_lang("eng")
    out = tmp_path / "saved"
    out.mkdir()
    tok.save(str(out))
    assert json.loads((out / "vocab.json").read_text()) == tok.index and not (out / "tokenizer_config.json").exists()


def test_language_resolution():
    tok = CharTokenizer(NESTED)
    assert resolve_language(tok, "fra") == "fra"          # exact (also a prefix of nothing else)
    assert resolve_language(tok, "e") == "eng"            # unique prefix
    assert resolve_language(tok, None) is None
    with pytest.raises(ValueError, match=r"Language fr not in .*\nCould it be one of \['fra', 'fro'\]\?"):
        resolve_language(tok, "fr")                        # ambiguous
    with pytest.raises(ValueError, match=r"Language deu not in \['eng', 'fra', 'fro'\]$"):
        resolve_language(tok, "deu")                       # absent
    flat = CharTokenizer(["<pad>", "a"])
    assert resolve_language(flat, "anything") == "anything"  # not a nested vocabulary: left alone, ignored later


def test_config_reads_and_writes_adapter_attn_dim(golden):
    d = json.loads(str(golden["config_json"]))
    cfg = Wav2Vec2Config.from_hf_dict(d)
    assert cfg.adapter_attn_dim == 16 and cfg.to_dict()["adapter_attn_dim"] == 16
    assert Wav2Vec2Config().adapter_attn_dim is None and Wav2Vec2Config().to_dict()["adapter_attn_dim"] is None
    assert Wav2Vec2Config.from_hf_dict(dict(d, adapter_attn_dim=None)).adapter_attn_dim is None
    with pytest.raises(ValueError, match="add_adapter"):
        Wav2Vec2Config.from_hf_dict(dict(d, add_adapter=True))


def test_adapter_file_key_set(golden, tmp_path):
    folder = GM.write_folder(golden, str(tmp_path / "m"))
    names = adapter_param_names(2)
    assert len(names) == 2 * 6 + 2 and "wav2vec2.encoder.layers.1.adapter_layer.linear_2.bias" in names
    sd = read_adapter_state(folder, "fra", names)
    assert set(sd) == set(names) and tuple(sd["lm_head.weight"].shape) == (21, 64)
    # safetensors is preferred over .bin; .bin is read when it is all there is
    torch.save({k: v + 1 for k, v in sd.items()}, os.path.join(folder, "adapter.fra.bin"))
    assert adapter_file(folder, "fra").endswith("adapter.fra.safetensors")
    os.remove(os.path.join(folder, "adapter.fra.safetensors"))
    sd_bin = read_adapter_state(folder, "fra", names)
    assert all(torch.equal(sd_bin[k], sd[k] + 1) for k in names)
    with pytest.raises(FileNotFoundError, match="adapter.deu.safetensors"):
        read_adapter_state(folder, "deu", names)
    # the two ValueErrors of load_adapter: unexpected keys first, then missing ones
    torch.save(dict(sd, extra=torch.zeros(1)), os.path.join(folder, "adapter.xx.bin"))
    with pytest.raises(ValueError, match="has unexpected keys: extra"):
        read_adapter_state(folder, "xx", names)
    torch.save({k: v for k, v in sd.items() if k != "lm_head.bias"}, os.path.join(folder, "adapter.yy.bin"))
    with pytest.raises(ValueError, match="has missing keys: lm_head.bias"):
        read_adapter_state(folder, "yy", names)
    with pytest.raises(ValueError, match="has unexpected keys"):
        read_adapter_state(folder, "eng", adapter_param_names(1))  # a model with fewer layers
