"""CPU: the float64 restatement of the LoRA decoder (tests/whisper_lora_ref.py) against the existing restatement with merged weights
and against transformers with hand-written LoRA modules; the adapter file format, the loader's refusals, the command line, and the
C entries' refusals (decided on the host, nothing launched)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_decoder_ref as WR  # noqa: E402
import whisper_lora_ref as LR  # noqa: E402
import whisper_train_ref as TR  # noqa: E402

R_, ALPHA = 8, 16.0
SCALING = ALPHA / R_


@pytest.fixture(scope="module")
def golden():
    g = np.load(G.GOLDEN)
    w = {k[2:]: WR.bf16_from_bits(g[k]) for k in g.files if k.startswith("w/")}
    return g, w, WR.bf16_from_bits(g["enc"]), WR.shifted_targets(g["tokens"], g["lens"])


@pytest.fixture(scope="module")
def lora():
    return LR.random_lora(G.LAYERS, G.D, R_, seed=5)


@pytest.fixture(scope="module")
def restated(golden, lora):
    g, w, enc, labels = golden
    return LR.decoder_loss_and_lora_grads(w, lora, G.NH, G.LAYERS, enc, labels, g["enc_lens"], G.EOT, G.SOT, scaling=SCALING)


def test_restatement_equals_the_existing_one_on_merged_weights(golden, lora, restated):
    """W = W0 + s B A built from leaf A, B handed to whisper_train_ref.decoder_loss_and_grads: the same function of A and B."""
    import torch
    g, w, enc, labels = golden
    leaves = {k: torch.tensor(v, requires_grad=True) for k, v in lora.items()}
    W = {k: torch.tensor(np.asarray(v, dtype=np.float64)) for k, v in w.items()}
    for n in leaves:
        if n.endswith(".lora_A.weight"):
            mod = n[:-len(".lora_A.weight")]
            W[mod + ".weight"] = W[mod + ".weight"] + SCALING * (leaves[mod + ".lora_B.weight"] @ leaves[n])
    loss, _ = TR.decoder_loss_and_grads(None, G.NH, G.LAYERS, enc, labels, g["enc_lens"], G.EOT, G.SOT, params=W)
    loss.backward()
    got_loss, grads = restated
    assert abs(got_loss - float(loss.detach())) <= 1e-12 * abs(got_loss)
    assert set(grads) == set(LR.names(G.LAYERS))
    for n, gr in grads.items():
        assert np.abs(gr).max() > 0, n
        assert TR.rel_l2(gr, leaves[n].grad.numpy()) <= 1e-12, n


def test_restatement_equals_transformers_with_lora_modules(golden, lora, restated):
    """transformers' decoder in float64, its eight target nn.Linear s wrapped by the LoRA module below (p = 0).  transformers takes
    no encoder mask: each utterance runs on its own frames, weighted by its token count (as tests/test_whisper_train_ref.py does)."""
    pytest.importorskip("transformers")
    import torch
    g, w, enc, labels = golden

    class Lora(torch.nn.Module):
        def __init__(self, base, A, B):
            super().__init__()
            self.base = base
            self.lora_A = torch.nn.Parameter(torch.tensor(A))
            self.lora_B = torch.nn.Parameter(torch.tensor(B))

        def forward(self, x):
            return self.base(x) + SCALING * ((x @ self.lora_A.T) @ self.lora_B.T)

    model = G.hf_model(w)
    wrapped = {}
    for l, layer in enumerate(model.model.decoder.layers):
        for attn, proj in LR.TARGETS:
            name = f"model.decoder.layers.{l}.{attn}.{proj}"
            mod = Lora(getattr(getattr(layer, attn), proj), lora[name + ".lora_A.weight"], lora[name + ".lora_B.weight"])
            setattr(getattr(layer, attn), proj, mod)
            wrapped[name] = mod
    ids = TR.shift_tokens_right(labels, G.EOT, G.SOT)
    n_all = int((labels >= 0).sum())
    total = 0.0
    for b in range(G.B):
        n_b = int((labels[b] >= 0).sum())
        e = torch.tensor(enc[b:b + 1, :g["enc_lens"][b]])
        out = model(encoder_outputs=(e,), decoder_input_ids=torch.from_numpy(ids[b:b + 1].astype(np.int64)),
                    labels=torch.from_numpy(labels[b:b + 1].astype(np.int64)))
        part = out.loss * n_b / n_all
        part.backward()
        total += float(part.detach())
    loss, grads = restated
    assert abs(total - loss) <= 1e-10 * abs(loss)
    for name, mod in wrapped.items():
        assert TR.rel_l2(grads[name + ".lora_A.weight"], mod.lora_A.grad.numpy()) <= 1e-10, name
        assert TR.rel_l2(grads[name + ".lora_B.weight"], mod.lora_B.grad.numpy()) <= 1e-10, name


def test_dropout_mask_enters_the_restatement(golden, lora, restated):
    """An all-ones mask with scale 1 is the p = 0 function; a real mask changes the loss."""
    g, w, enc, labels = golden
    rows = {0: G.B * G.L, 1: G.B * G.L, 2: G.B * G.L, 3: G.B * G.S}
    ones = {(l, k): np.ones((rows[k], G.D)) for l in range(G.LAYERS) for k in range(4)}
    a = LR.decoder_loss_and_lora_grads(w, lora, G.NH, G.LAYERS, enc, labels, g["enc_lens"], G.EOT, G.SOT, scaling=SCALING, masks=ones)
    assert a[0] == restated[0]
    rng = np.random.default_rng(0)
    half = {k: (rng.random(v.shape) < 0.5).astype(np.float64) for k, v in ones.items()}
    b = LR.decoder_loss_and_lora_grads(w, lora, G.NH, G.LAYERS, enc, labels, g["enc_lens"], G.EOT, G.SOT, scaling=SCALING, masks=half, mask_scale=2.0)
    assert b[0] != restated[0]
    assert LR.drop_scale(0.5) == 2.0 and LR.drop_scale(0.0) == 1.0 and abs(LR.drop_scale(0.05) - 65536 / (65536 - 3277)) < 1e-15


# ---------------------------------------------------------------------------------------------------------------- files
def _tensors(lora):
    import torch
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in lora.items()}


def test_adapter_file_round_trip(lora, tmp_path):
    import torch
    from safetensors.torch import load_file
    from ssak_amd import whisper_lora as WL
    folder = WL.write_adapter(str(tmp_path / "out" / "adapter_model"), _tensors(lora), WL.adapter_config(R_, ALPHA, 0.05, "/some/base"))
    with open(os.path.join(folder, "adapter_config.json")) as f:
        cfg = json.load(f)
    assert cfg["peft_type"] == "LORA" and cfg["r"] == R_ and cfg["lora_alpha"] == ALPHA and cfg["lora_dropout"] == 0.05 and cfg["bias"] == "none"
    assert cfg["target_modules"] == ".*decoder.*(self_attn|encoder_attn).*(q_proj|v_proj)$" == WL.TARGET_REGEX
    assert cfg["base_model_name_or_path"] == "/some/base" and cfg["fan_in_fan_out"] is False and cfg["inference_mode"] is True
    sd = load_file(os.path.join(folder, "adapter_model.safetensors"))
    assert set(sd) == {"base_model.model." + n for n in LR.names(G.LAYERS)}
    for n, v in lora.items():
        t = sd["base_model.model." + n]
        assert t.dtype == torch.float32 and tuple(t.shape) == v.shape and np.array_equal(t.numpy().view(np.int32), v.astype(np.float32).view(np.int32)), n
    # the walk of the reference's inference: the folder itself, or the first below it
    assert WL.find_adapter_config(folder) == folder and WL.find_adapter_config(str(tmp_path / "out")) == folder
    assert WL.find_adapter_config(str(tmp_path / "nothing")) is None
    cfg2, pairs = WL.read_adapter(folder)
    assert cfg2 == cfg and set(pairs) == {n[:-len(".lora_A.weight")] for n in lora if n.endswith(".lora_A.weight")}
    for mod, (A, B) in pairs.items():
        assert np.array_equal(A.numpy().view(np.int32), lora[mod + ".lora_A.weight"].astype(np.float32).view(np.int32))
        assert np.array_equal(B.numpy().view(np.int32), lora[mod + ".lora_B.weight"].astype(np.float32).view(np.int32))
    # PEFT's other spellings: an adapter name inside the key, a pickle instead of safetensors, a list of suffixes
    alt = str(tmp_path / "alt")
    os.makedirs(alt)
    torch.save({"base_model.model." + n.replace(".weight", ".default.weight"): v for n, v in _tensors(lora).items()}, os.path.join(alt, "adapter_model.bin"))
    with open(os.path.join(alt, "adapter_config.json"), "w") as f:
        json.dump(dict(cfg, target_modules=["q_proj", "v_proj"]), f)
    assert set(WL.read_adapter(alt)[1]) == set(pairs)
    assert WL.module_is_target("model.decoder.layers.1.encoder_attn.v_proj", WL.TARGET_REGEX)
    assert not WL.module_is_target("model.decoder.layers.1.encoder_attn.k_proj", WL.TARGET_REGEX)
    assert not WL.module_is_target("model.encoder.layers.1.self_attn.q_proj", WL.TARGET_REGEX)
    assert WL.module_is_target("model.decoder.layers.1.fc1", ["fc1"]) and not WL.module_is_target("model.decoder.layers.1.fc1", ["c1"])


def test_adapter_loader_refusals(lora, tmp_path):
    import torch
    from ssak_amd import whisper_lora as WL
    base = WL.adapter_config(R_, ALPHA, 0.05, "/some/base")

    def folder(name, tensors=None, **over):
        return WL.write_adapter(str(tmp_path / name), _tensors(lora) if tensors is None else tensors, dict(base, **over))

    for name, over, word in (("bias", {"bias": "all"}, "bias"), ("mts", {"modules_to_save": ["proj_out"]}, "modules_to_save"),
                             ("rank", {"rank_pattern": {"q_proj": 4}}, "rank_pattern"), ("alpha", {"alpha_pattern": {"q_proj": 4}}, "alpha_pattern"),
                             ("dora", {"use_dora": True}, "use_dora"), ("rs", {"use_rslora": True}, "use_rslora"),
                             ("type", {"peft_type": "IA3"}, "peft_type")):
        with pytest.raises(ValueError, match=word):
            WL.read_adapter(folder(name, **over))
    enc = {"model.encoder.layers.0.self_attn.q_proj.lora_A.weight": torch.zeros(R_, G.D), "model.encoder.layers.0.self_attn.q_proj.lora_B.weight": torch.zeros(G.D, R_)}
    with pytest.raises(ValueError, match="encoder adapters"):
        WL.read_adapter(folder("enc", enc, target_modules=["q_proj"]))
    with pytest.raises(ValueError, match="does not name"):
        WL.read_adapter(folder("unnamed", target_modules=["k_proj"]))
    with pytest.raises(ValueError, match="rank r = 16"):
        WL.read_adapter(folder("rank16", r=16))
    empty = str(tmp_path / "empty")
    os.makedirs(empty)
    with open(os.path.join(empty, "adapter_config.json"), "w") as f:
        json.dump(base, f)
    with pytest.raises(FileNotFoundError, match="adapter_model"):
        WL.read_adapter(empty)
    # the base must be a local folder: nothing is downloaded, and the error names the path
    with pytest.raises(FileNotFoundError, match="/some/base"):
        WL.load_adapter_folder(None, folder("ok"), folder("ok"), "cuda:0", False)


def test_layout_and_step_seeds():
    from ssak_amd import whisper_lora as WL
    layout, total = WL.lora_layout(G.LAYERS, G.D, R_)
    assert list(layout) == LR.names(G.LAYERS) and total == G.LAYERS * 4 * 2 * R_ * G.D
    assert layout[LR.names(G.LAYERS)[1]] == (R_ * G.D, R_ * G.D, (G.D, R_))
    # whisper-small at the reference's settings: 2.36 M trainable parameters
    assert WL.lora_layout(12, 768, 32)[1] == 2359296
    seeds = {WL.lora_step_seed(42, i) for i in range(100)} | {WL.lora_step_seed(43, i) for i in range(100)}
    assert len(seeds) == 200 and all(0 <= s < 1 << 64 for s in seeds)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_command_line(capsys):
    from ssak_amd.train_whisper import parse_args
    base = ["train_dir", "valid_dir", "--base_model", "model_dir"]
    a = parse_args(base)
    assert a.lora is False
    a = parse_args(base + ["--lora"])
    assert a.lora is True and (a.lora_r, a.lora_alpha, a.lora_dropout) == (32, 64, 0.05)
    a = parse_args(base + ["--lora", "--lora_r", "8", "--lora_alpha", "32", "--lora_dropout", "0"])
    assert (a.lora_r, a.lora_alpha, a.lora_dropout) == (8, 32, 0.0)
    for flags, words in ((["--lora", "--int4"], ["--int4"]), (["--peft"], ["--peft", "--lora"]), (["--lora", "--peft"], ["--peft", "--lora"]),
                         (["--lora", "--lora_r", "12"], ["--lora_r"]), (["--lora", "--gradient_accumulation_steps", "16"], ["gradient accumulation"])):
        with pytest.raises(SystemExit):
            parse_args(base + flags)
        err = capsys.readouterr().err
        assert all(word in err for word in words), (flags, err)


# ---------------------------------------------------------------------------------------------------------------- C entries
def test_lora_entries_reject_bad_arguments_before_any_launch():
    """SSAK_ERR_INVALID, decided on the host: every call here lacks an operand or names a shape no kernel is built for (the pointer
    is never dereferenced)."""
    import ssak_amd.hip as h
    L = h.lib
    assert L.ssak_version() == h.ABI_VERSION == 660  # the entries are additive

    def last():
        return L.ssak_last_error().decode()

    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)
    fwd = lambda x=one, ldx=128, A=one, B=one, y=one, ldy=128, t=one, M=4, Din=128, Dout=128, r=8, p=0.0: \
        L.ssak_lora_fwd(x, ldx, A, B, y, ldy, t, M, Din, Dout, r, 1.0, 1, 2, p, None)
    bwi = lambda dy=one, lddy=128, A=one, B=one, dt=one, dx=one, lddx=128, M=4, Din=128, Dout=128, r=8, p=0.0: \
        L.ssak_lora_bwd_input(dy, lddy, A, B, dt, dx, lddx, 1, M, Din, Dout, r, 1.0, 1, 2, p, None)
    bww = lambda dy=one, lddy=128, t=one, dt=one, x=one, ldx=128, dB=one, dA=one, M=4, Din=128, Dout=128, r=8, p=0.0, ws=one, nbytes=1 << 20: \
        L.ssak_lora_bwd_weights(dy, lddy, t, dt, x, ldx, dB, dA, M, Din, Dout, r, 1.0, 1, 2, p, ws, nbytes, None)
    mrg = lambda w=one, A=one, B=one, out=one, Din=128, Dout=128, r=8: L.ssak_lora_merge(w, A, B, out, None, Din, Dout, r, 1.0, None)
    for fn in (fwd, bwi, bww):
        for kw, word in ((dict(r=12), "r = 12"), (dict(r=128), "r = 128"), (dict(Din=96), "D_in = 96"), (dict(Dout=1344), "D_out = 1344"),
                         (dict(Din=0), "D_in = 0"), (dict(M=0), "M = 0"), (dict(p=1.0), "drop_p"), (dict(p=-0.5), "drop_p")):
            assert fn(**kw) == h.SSAK_ERR_INVALID and word in last(), (kw, last())
    for kw in (dict(x=None), dict(A=None), dict(B=None), dict(y=None)):
        assert fwd(**kw) == h.SSAK_ERR_INVALID and "null" in last(), kw
    for kw in (dict(dy=None), dict(A=None), dict(B=None), dict(dt=None)):
        assert bwi(**kw) == h.SSAK_ERR_INVALID and "null" in last(), kw
    for kw in (dict(dy=None), dict(t=None), dict(dt=None), dict(x=None), dict(dB=None), dict(dA=None), dict(ws=None)):
        assert bww(**kw) == h.SSAK_ERR_INVALID and "null" in last(), kw
    for kw in (dict(w=None), dict(A=None), dict(B=None), dict(out=None)):
        assert mrg(**kw) == h.SSAK_ERR_INVALID and "null" in last(), kw
    assert fwd(ldx=64) == h.SSAK_ERR_INVALID and "strides" in last()
    assert fwd(ldy=132) == h.SSAK_ERR_INVALID and "strides" in last()
    assert fwd(y=odd) == h.SSAK_ERR_INVALID and "aligned" in last()
    assert bwi(lddy=64) == h.SSAK_ERR_INVALID and "strides" in last()
    assert bwi(lddx=64) == h.SSAK_ERR_INVALID and "strides" in last()
    assert bww(ldx=64) == h.SSAK_ERR_INVALID and "strides" in last()
    need = L.ssak_lora_bwd_weights_workspace_bytes(1025, 128, 256, 8)
    assert need == 3 * 8 * (128 + 256) * 4  # three 512-row ranges
    assert bww(M=1025, Dout=256, lddy=256, nbytes=need - 1) == h.SSAK_ERR_INVALID and "workspace" in last()
    assert mrg(r=12) == h.SSAK_ERR_INVALID and "r = 12" in last()
    assert mrg(Din=96) == h.SSAK_ERR_INVALID and "D_in = 96" in last()
    assert mrg(Dout=5184) == h.SSAK_ERR_INVALID and "D_out = 5184" in last()
