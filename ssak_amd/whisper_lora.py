"""LoRA on the Whisper decoder (the reference's PEFT recipe, ssak/train/transformers/whisper_train.py:374-429, on a bf16 base) and
PEFT adapter folders (ssak/infer/whisper_infer.py:123-170): the adapter half of :class:`ssak_amd.whisper_seq2seq.WhisperSeq2Seq`.

:class:`WhisperLoraMixin` gives the model ``add_lora`` (adapters on ``q_proj`` / ``v_proj`` of the decoder's ``self_attn`` and
``encoder_attn``: three flat buffers ``lora_params`` fp32 / ``lora_shadow`` bf16 / ``lora_grads`` fp32 under PEFT's names; everything
else frozen), the forward hook of ``_decoder_hidden`` (``ssak_lora_fwd`` on the column blocks of the packed products), the
frozen-base ``backward`` (input gradients only, ``ssak_lora_bwd_input`` / ``ssak_lora_bwd_weights`` per adapter),
``merge_lora`` / ``unmerge_lora`` / ``lora_merged`` (``ssak_lora_merge`` into the bf16 shadow; unmerging recasts the untouched fp32
masters, which is exact) and ``save_adapter``.  The file half needs no GPU: :func:`write_adapter`, :func:`find_adapter_config`,
:func:`read_adapter`, :func:`check_adapter_config`, :func:`adapter_targets`.  Kernels: ssak_amd/csrc/whisper_lora.hip.

Not built: int8 / nf4 quantisation of the base (the reference's ``--peft`` / ``--int4`` as it spells them), gradient accumulation,
data parallelism, training adapters on other targets than the reference's, encoder adapters, DoRA, rsLoRA, ``generate`` on unmerged
adapters (it merges for the call).  ``peft`` itself is not a dependency and parity with it is not pinned by a test.
"""
from __future__ import annotations

import contextlib
import json
import math
import os
import re
from typing import Dict, Optional

import numpy as np
import torch

from . import hip

# the reference's LoraConfig.target_modules
TARGET_REGEX = ".*decoder.*(self_attn|encoder_attn).*(q_proj|v_proj)$"
_TRAIN_TARGETS = ("q_proj", "v_proj")
_ATTNS = ("self_attn", "encoder_attn")
_WHICH = {("self_attn", "q_proj"): 0, ("self_attn", "v_proj"): 1, ("encoder_attn", "q_proj"): 2, ("encoder_attn", "v_proj"): 3}
_MERGE_LEAVES = ("q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2")
_KEY_PREFIX = "base_model.model."
_REFUSED_LISTS = ("modules_to_save", "rank_pattern", "alpha_pattern")
_REFUSED_FLAGS = ("use_dora", "use_rslora")


def lora_layout(n_layers: int, d_model: int, r: int):
    """name -> (offset, numel, shape) in the flat adapter buffers, PEFT's names: per layer and target ``lora_A.weight`` [r, D] then
    ``lora_B.weight`` [D, r]."""
    layout, off = {}, 0
    for l in range(n_layers):
        for attn in _ATTNS:
            for proj in _TRAIN_TARGETS:
                for leaf, shape in (("lora_A", (r, d_model)), ("lora_B", (d_model, r))):
                    layout[f"model.decoder.layers.{l}.{attn}.{proj}.{leaf}.weight"] = (off, r * d_model, shape)
                    off += r * d_model
    return layout, off


def lora_step_seed(seed: int, step: int) -> int:
    """The 64-bit dropout seed of train step ``step`` under the model's LoRA ``seed`` (host-derived: every step a fresh mask)."""
    return int(np.random.SeedSequence([int(seed), int(step)]).generate_state(1, dtype=np.uint64)[0])


# ---------------------------------------------------------------------------------------------------------------- adapter files
def adapter_config(r: int, alpha: float, dropout: float, base_model_name_or_path: Optional[str]) -> dict:
    return {"peft_type": "LORA", "task_type": None, "r": int(r), "lora_alpha": alpha, "lora_dropout": float(dropout), "target_modules": TARGET_REGEX,
            "bias": "none", "base_model_name_or_path": base_model_name_or_path, "fan_in_fan_out": False, "inference_mode": True}


def write_adapter(folder: str, tensors: Dict[str, torch.Tensor], config: dict) -> str:
    """``adapter_config.json`` and ``adapter_model.safetensors`` (fp32, keys ``base_model.model.<name>``) -> folder."""
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "adapter_config.json"), "w") as f:
        json.dump(config, f, indent=1)
    save_file({_KEY_PREFIX + k: torch.as_tensor(v).detach().to(torch.float32).cpu().contiguous() for k, v in tensors.items()},
              os.path.join(folder, "adapter_model.safetensors"), metadata={"format": "pt"})
    return folder


def find_adapter_config(folder: str) -> Optional[str]:
    """The folder, ``folder`` itself or the first below it in ``os.walk`` order, that holds an ``adapter_config.json`` (as the
    reference's inference looks for one); None: not a PEFT folder."""
    if not os.path.isdir(folder):
        return None
    for root, _, files in os.walk(folder):
        if "adapter_config.json" in files:
            return root
    return None


def check_adapter_config(cfg: dict) -> dict:
    """Refuses, by name, what the merge does not implement -> the configuration."""
    if str(cfg.get("peft_type", "LORA")).upper() != "LORA":
        raise ValueError(f"peft_type {cfg.get('peft_type')!r}: only LORA adapters are built")
    if cfg.get("bias", "none") != "none":
        raise ValueError(f"bias = {cfg['bias']!r}: only bias = \"none\" is built")
    for key in _REFUSED_LISTS:
        if cfg.get(key):
            raise ValueError(f"{key} = {cfg[key]!r}: a non-empty {key} is not built")
    for key in _REFUSED_FLAGS:
        if cfg.get(key):
            raise ValueError(f"{key} = true: {key[4:] if key != 'use_dora' else 'DoRA'} adapters are not built ({key})")
    if cfg.get("fan_in_fan_out"):
        raise ValueError("fan_in_fan_out = true: Whisper's projections are nn.Linear (fan_in_fan_out false)")
    if not isinstance(cfg.get("r"), int) or cfg["r"] < 1:
        raise ValueError(f"r = {cfg.get('r')!r}: a positive integer rank is expected")
    return cfg


def module_is_target(module: str, target_modules) -> bool:
    """PEFT's rule: a string is a regex for ``re.fullmatch`` on the module name, a list holds suffixes."""
    if isinstance(target_modules, str):
        return re.fullmatch(target_modules, module) is not None
    return any(module == t or module.endswith("." + t) for t in target_modules)


def read_adapter(folder: str):
    """-> (config, {module name: (A [r, D_in], B [D_out, r])} fp32 on the host) of the adapter folder ``folder``
    (``adapter_model.safetensors`` or ``adapter_model.bin``), module names as transformers has them (``model.decoder.layers.0...``).
    Refused by name: what :func:`check_adapter_config` refuses, encoder targets, a target that is no decoder projection."""
    with open(os.path.join(folder, "adapter_config.json")) as f:
        cfg = check_adapter_config(json.load(f))
    st, pt = os.path.join(folder, "adapter_model.safetensors"), os.path.join(folder, "adapter_model.bin")
    if os.path.isfile(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    elif os.path.isfile(pt):
        sd = torch.load(pt, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"{folder}: adapter_config.json without adapter_model.safetensors or adapter_model.bin")
    pairs: Dict[str, dict] = {}
    for key, v in sd.items():
        m = re.fullmatch(r"(?:base_model\.model\.)?(.+)\.(lora_[AB])(?:\.[^.]+)?\.weight", key)
        if m is None:
            raise ValueError(f"{folder}: tensor {key} is not a LoRA weight (lora_A / lora_B)")
        pairs.setdefault(m.group(1), {})[m.group(2)] = v.to(torch.float32).contiguous()
    out = {}
    for module, ab in pairs.items():
        if ".encoder." in module or module.startswith("encoder."):
            raise ValueError(f"{folder}: adapter on {module}: encoder adapters are not built")
        if not module_is_target(module, cfg.get("target_modules") or []):
            raise ValueError(f"{folder}: adapter on {module}, which target_modules = {cfg.get('target_modules')!r} does not name")
        if re.fullmatch(r"model\.decoder\.layers\.\d+\.((self_attn|encoder_attn)\.(q_proj|k_proj|v_proj|out_proj)|fc1|fc2)", module) is None:
            raise ValueError(f"{folder}: adapter on {module}: only the decoder's q_proj, k_proj, v_proj, out_proj, fc1 and fc2 can be merged")
        if set(ab) != {"lora_A", "lora_B"}:
            raise ValueError(f"{folder}: {module} has {sorted(ab)}: both lora_A and lora_B are needed")
        A, B = ab["lora_A"], ab["lora_B"]
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != cfg["r"] or B.shape[1] != cfg["r"]:
            raise ValueError(f"{folder}: {module}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} do not have rank r = {cfg['r']}")
        out[module] = (A, B)
    if not out:
        raise ValueError(f"{folder}: the adapter file holds no LoRA weight")
    return cfg, out


# ---------------------------------------------------------------------------------------------------------------- the model half
class WhisperLoraMixin:
    """The adapter methods of :class:`ssak_amd.whisper_seq2seq.WhisperSeq2Seq`."""

    _lora: Optional[dict] = None      # r, alpha, dropout, seed, scaling, layout
    _lora_merged: bool = False
    _lora_train_pass: bool = False    # set by forward_train(keep_graph=True) around its decoder pass: dropout on, t kept
    lora_step: int = 0                # train forwards so far: the step counter the dropout seed is derived from
    lora_params: Optional[torch.Tensor] = None
    lora_shadow: Optional[torch.Tensor] = None
    lora_grads: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ construction
    def add_lora(self, r: int = 32, alpha: float = 64, dropout: float = 0.05, seed: int = 42, target_modules=None):
        """Adapters on the reference's targets, initialised as PEFT does (A ~ U(+-1/sqrt(D_in)) = kaiming_uniform(a = sqrt 5) from
        ``seed``, B = 0); everything else is frozen (``freeze_encoder`` included)."""
        if self._lora is not None:
            raise RuntimeError("add_lora(): the model already has adapters")
        if target_modules is not None and target_modules != TARGET_REGEX and sorted(target_modules) != sorted(_TRAIN_TARGETS):
            raise ValueError(f"target_modules = {target_modules!r}: training adapters on other targets than the reference's "
                             f"({TARGET_REGEX!r}) is not built")
        if r not in (8, 16, 32, 64):
            raise ValueError(f"r = {r}: the ranks built are 8, 16, 32 and 64")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"lora_dropout = {dropout}: a probability in [0, 1) is expected")
        cfg = self.config
        D = cfg.d_model
        if D % 64 or D > 1280:
            raise ValueError(f"d_model {D}: the adapter kernels take multiples of 64 up to 1280")
        layout, total = lora_layout(cfg.decoder_layers, D, r)
        self._lora = dict(r=int(r), alpha=alpha, dropout=float(dropout), seed=int(seed), scaling=float(alpha) / r, layout=layout)
        gen = torch.Generator().manual_seed(int(seed))
        host = torch.zeros(total, dtype=torch.float32)
        bound = 1.0 / math.sqrt(D)
        for name, (off, n, _) in layout.items():
            if ".lora_A." in name:
                host[off:off + n] = (torch.rand(n, generator=gen, dtype=torch.float32) * 2 - 1) * bound
        with torch.cuda.device(self.device):
            self.lora_params = host.to(self.device)
            self.lora_shadow = torch.empty(total, dtype=torch.bfloat16, device=self.device)
            self.lora_grads = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.sync_lora_shadow()
        self.freeze_encoder = True
        self.lora_step = 0
        return self

    def sync_lora_shadow(self):
        with torch.cuda.device(self.device):
            hip.check(hip.lib.ssak_cast_f32_bf16(hip.ptr(self.lora_params), hip.ptr(self.lora_shadow), self.lora_params.numel(), hip.stream()))

    def _lora_view(self, buf: torch.Tensor, name: str) -> torch.Tensor:
        off, n, shape = self._lora["layout"][name]
        return buf[off:off + n].view(shape)

    def lora_param(self, name: str) -> torch.Tensor:
        return self._lora_view(self.lora_params, name)

    def lora_grad(self, name: str) -> torch.Tensor:
        return self._lora_view(self.lora_grads, name)

    def load_lora_state_dict(self, sd: Dict[str, torch.Tensor]):
        """fp32 tensors under the layout's names (every one of them) into the masters; the shadow follows."""
        for name, (off, n, shape) in self._lora["layout"].items():
            t = torch.as_tensor(sd[name]).to(torch.float32)
            if tuple(t.shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {name}: {tuple(t.shape)} vs {tuple(shape)}")
            self.lora_params[off:off + n].copy_(t.reshape(-1).to(self.device))
        self.sync_lora_shadow()
        return self

    @staticmethod
    def lora_site(layer: int, which: int) -> int:
        """The dropout site of an adapter's input: ``which`` = 0 self q_proj, 1 self v_proj, 2 cross q_proj, 3 cross v_proj."""
        return hip.LORA_SITE_BASE + 4 * int(layer) + int(which)

    @property
    def lora_drop_seed(self) -> int:
        """The dropout seed of the last (or running) train forward: ``lora_step_seed(seed, lora_step)``."""
        return lora_step_seed(self._lora["seed"], self.lora_step)

    # ------------------------------------------------------------------ forward
    def _lora_active(self) -> bool:
        return self._lora is not None and not self._lora_merged

    def _lora_fwd(self, layer: int, attn: str, proj: str, x: torch.Tensor, y: torch.Tensor, saved: dict):
        """The adapter of ``layers.{layer}.{attn}.{proj}`` on ``y`` (the column block of the base product that is its output), in
        place.  In a train pass the dropout is on and ``t`` goes into ``saved`` under ``t{which}``."""
        lo = self._lora
        which = _WHICH[(attn, proj)]
        p = f"model.decoder.layers.{layer}.{attn}.{proj}."
        t = None
        train = self._lora_train_pass
        if train:
            t = saved[f"t{which}"] = torch.empty((x.shape[0], lo["r"]), dtype=torch.bfloat16, device=self.device)
        hip.lora_fwd(x, self._lora_view(self.lora_shadow, p + "lora_A.weight"), self._lora_view(self.lora_shadow, p + "lora_B.weight"), y,
                     lo["scaling"], t=t, seed=self.lora_drop_seed if train else 0, site=self.lora_site(layer, which),
                     drop_p=lo["dropout"] if train else 0.0)

    # ------------------------------------------------------------------ backward (frozen base)
    def _backward_lora(self, s: dict, grad_scale: float):
        """``backward()`` with adapters: the base does its input gradients only (no weight gradient, no bias sum, no embedding
        scatter, no ``d_enc``, nothing above layer 0's attention), each adapter its two weight gradients into ``lora_grads``."""
        cfg, lo = self.config, self._lora
        B, L, S, enc2 = s["B"], s["L"], s["S"], s["enc2"]
        D, nh, N, V = cfg.d_model, cfg.decoder_attention_heads, B * L, cfg.vocab_size
        dev = self.device
        r, sc, p_drop, seed = lo["r"], lo["scaling"], lo["dropout"], s["lora_seed"]
        bf = lambda *sh: torch.empty(sh, dtype=torch.bfloat16, device=dev)
        with torch.cuda.device(dev):
            ln_ws = hip._ws(hip.lib.ssak_layernorm_bwd_workspace_bytes(D), dev)
            ln_scratch = torch.zeros((2, D), dtype=torch.float32, device=dev)  # the frozen LayerNorms' dgamma / dbeta: never read
            lw_ws = hip._ws(hip.lib.ssak_lora_bwd_weights_workspace_bytes(max(N, B * S), D, D, r), dev)

            def norm_bwd(g1, ln, name, g_res):
                dr = bf(N, D)
                hip.layernorm_bwd(g1, None, ln[0], ln[2], ln[3], self._f(name + ".weight"), g_res, dr, ln_scratch[0], ln_scratch[1], workspace=ln_ws)
                return dr

            def adapter_bwd(layer, attn, proj, dy, x, t, dx):
                """dt, then dx += (when anything upstream needs it), then the adapter's dA / dB"""
                which = _WHICH[(attn, proj)]
                name = f"model.decoder.layers.{layer}.{attn}.{proj}."
                A, Bm = self._lora_view(self.lora_shadow, name + "lora_A.weight"), self._lora_view(self.lora_shadow, name + "lora_B.weight")
                site = self.lora_site(layer, which)
                dt = bf(dy.shape[0], r)
                hip.lora_bwd_input(dy, A, Bm, dt, sc, dx=dx, accumulate=True, seed=seed, site=site, drop_p=p_drop)
                hip.lora_bwd_weights(dy, t, dt, x, self.lora_grad(name + "lora_A.weight"), self.lora_grad(name + "lora_B.weight"), sc, seed=seed,
                                     site=site, drop_p=p_drop, workspace=lw_ws)

            xf = s["ln_f"][1]
            E = self._w("embed_tokens.weight")
            dx = bf(N, D)
            dl_ws = bf(min(self.row_chunk, N), E.shape[0])
            for r0, n, logits in self._project_chunks(xf):
                dl = dl_ws[:n]
                hip.dec_ce_bwd(logits, V, s["targets"][r0:r0 + n], grad_scale / s["n_scored"], dlogits=dl, want_loss=False)
                self._dgrad(dl, E, out=dx[r0:r0 + n])
            dh = norm_bwd(dx, s["ln_f"], "layer_norm", None)
            for l in reversed(range(cfg.decoder_layers)):
                p = f"layers.{l}."
                sv = s["layers"][l]
                dpre = self._dgrad(dh, self._w(p + "fc2.weight"), epilogue=hip.EPI_MUL_GELU_GRAD, aux_in=sv["pre"])
                dh = norm_bwd(self._dgrad(dpre, self._w(p + "fc1.weight")), sv["ln3"], p + "final_layer_norm", dh)
                # cross-attention: the encoder is frozen, so the k|v product has no input gradient to form
                a = p + "encoder_attn."
                dctx = self._dgrad(dh, self._w(a + "out_proj.weight"))
                dq, dkv = bf(N, D), bf(B * S, 2 * D)
                kv = sv["kv_c"]
                hip.dec_attention_bwd(sv["q_c"], kv[:, :D], kv[:, D:], sv["ctx_c"], sv["lse_c"], dctx, dq, dkv[:, :D], dkv[:, D:], B, L, S, nh,
                                      klens=s["enc_lens"])
                adapter_bwd(l, "encoder_attn", "v_proj", dkv[:, D:], enc2, sv["t3"], None)
                dxq = self._dgrad(dq, self._w(a + "q_proj.weight"))
                adapter_bwd(l, "encoder_attn", "q_proj", dq, sv["ln2"][1], sv["t2"], dxq)
                dh = norm_bwd(dxq, sv["ln2"], p + "encoder_attn_layer_norm", dh)
                # causal self-attention; nothing trainable is upstream of layer 0's
                a = p + "self_attn."
                dctx = self._dgrad(dh, self._w(a + "out_proj.weight"))
                dqkv = bf(N, 3 * D)
                qkv = sv["qkv"]
                hip.dec_attention_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], sv["ctx_s"], sv["lse_s"], dctx, dqkv[:, :D], dqkv[:, D:2 * D],
                                      dqkv[:, 2 * D:], B, L, L, nh, causal=True)
                dx1 = self._dgrad(dqkv, self._w(a + "q_proj.weight", 3)) if l > 0 else None
                adapter_bwd(l, "self_attn", "q_proj", dqkv[:, :D], sv["ln1"][1], sv["t0"], dx1)
                adapter_bwd(l, "self_attn", "v_proj", dqkv[:, 2 * D:], sv["ln1"][1], sv["t1"], dx1)
                if l > 0:
                    dh = norm_bwd(dx1, sv["ln1"], p + "self_attn_layer_norm", dh)
            self.encoder_grads_ready = False
        return None

    # ------------------------------------------------------------------ merging
    def _lora_targets(self):
        """(weight name in the decoder layout, A name, B name) per adapter"""
        for name in self._lora["layout"]:
            if name.endswith(".lora_A.weight"):
                module = name[:-len(".lora_A.weight")]
                yield module + ".weight", name, module + ".lora_B.weight"

    def merge_lora(self):
        """``dec_shadow`` of every target = bf16(W + scaling * B A) from the fp32 masters (``ssak_lora_merge``); the masters stay."""
        if self._lora is None:
            raise RuntimeError("merge_lora(): the model has no adapters")
        if self._lora_merged:
            return self
        with torch.cuda.device(self.device):
            for w, a, b in self._lora_targets():
                off, n, shape = self.layout[w]
                hip.lora_merge(self.dec_param(w), self.lora_param(a), self.lora_param(b), self.dec_shadow[off:off + n].view(shape), self._lora["scaling"])
        self._lora_merged = True
        return self

    def unmerge_lora(self):
        """The targets' shadow recast from the untouched fp32 masters: bit for bit what it was."""
        if not self._lora_merged:
            return self
        with torch.cuda.device(self.device):
            for w, _, _ in self._lora_targets():
                off, n, _ = self.layout[w]
                hip.check(hip.lib.ssak_cast_f32_bf16(hip.ptr(self.dec_params[off:]), hip.ptr(self.dec_shadow[off:]), n, hip.stream()))
        self._lora_merged = False
        return self

    @contextlib.contextmanager
    def lora_merged(self):
        """The model with its adapters merged into the shadow for the block (``generate`` / ``transcribe`` run this way)."""
        was = self._lora_merged
        self.merge_lora()
        try:
            yield self
        finally:
            if not was:
                self.unmerge_lora()

    def merge_adapter_tensors(self, pairs: Dict[str, tuple], scaling: float):
        """An adapter read from a folder (:func:`read_adapter`), merged for good: masters and shadow of every target become
        W + scaling * B A (PEFT's ``merge_and_unload``)."""
        with torch.cuda.device(self.device):
            for module, (A, Bm) in pairs.items():
                w = module + ".weight"
                if w not in self.layout:
                    raise ValueError(f"adapter on {module}: the decoder has no such projection")
                off, n, shape = self.layout[w]
                if A.shape[1] != shape[1] or Bm.shape[0] != shape[0]:
                    raise ValueError(f"adapter on {module}: lora_A {tuple(A.shape)} / lora_B {tuple(Bm.shape)} against a weight of shape {tuple(shape)}")
                master = self.dec_param(w)
                hip.lora_merge(master, A.to(self.device).contiguous(), Bm.to(self.device).contiguous(), self.dec_shadow[off:off + n].view(shape),
                               scaling, w_out_f32=master)
        return self

    # ------------------------------------------------------------------ files
    def lora_state_dict(self) -> Dict[str, torch.Tensor]:
        torch.cuda.synchronize(self.device)
        return {name: self.lora_param(name).detach().cpu().clone() for name in self._lora["layout"]}

    def save_adapter(self, folder: str, base_model_name_or_path: Optional[str] = None) -> str:
        """``adapter_config.json`` + ``adapter_model.safetensors`` as PEFT writes them; :meth:`from_pretrained` reads the folder
        back (``base_model_name_or_path``: by default the folder this model was loaded from)."""
        lo = self._lora
        if lo is None:
            raise RuntimeError("save_adapter(): the model has no adapters")
        base = base_model_name_or_path if base_model_name_or_path is not None else self.name_or_path
        return write_adapter(folder, self.lora_state_dict(), adapter_config(lo["r"], lo["alpha"], lo["dropout"], base))


def load_adapter_folder(cls, folder: str, adapter_dir: str, device: str, freeze_encoder: bool):
    """``from_pretrained`` of a PEFT folder: the base named by ``base_model_name_or_path`` (a local folder: nothing is downloaded)
    with the adapter merged into it."""
    cfg, pairs = read_adapter(adapter_dir)
    base = cfg.get("base_model_name_or_path")
    if not base or not os.path.isdir(base) or not os.path.isfile(os.path.join(base, "config.json")):
        raise FileNotFoundError(f"{adapter_dir}: base_model_name_or_path = {base!r} is not a local model folder (nothing is downloaded: "
                                f"put the base model there, or edit adapter_config.json)")
    if find_adapter_config(base) is not None:
        raise ValueError(f"{adapter_dir}: base_model_name_or_path = {base!r} is itself an adapter folder")
    model = cls.from_pretrained(base, device=device, freeze_encoder=freeze_encoder)
    model.merge_adapter_tensors(pairs, float(cfg.get("lora_alpha", cfg["r"])) / cfg["r"])
    model.name_or_path = folder if os.path.isfile(os.path.join(folder, "config.json")) else base  # (where the tokenizer files are)
    return model
