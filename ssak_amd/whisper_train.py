"""Full fine-tuning of ``WhisperForConditionalGeneration`` (the reference's non-PEFT branch,
ssak/train/transformers/whisper_train.py:432,464-507,531) on one MI355X: the training half of :class:`ssak_amd.whisper_seq2seq.WhisperSeq2Seq`.

:class:`WhisperTrainMixin` gives the model ``forward_train`` (``_decoder_hidden(keep=)``, the model's one teacher-forced pass keeping
what the backward reads -- its docstring lists that -- and HF's ``.loss`` on the device), ``backward`` (the vocabulary projection
per ``row_chunk`` rows, the layers in reverse, the tied embedding's two gradients, the cross k|v gradients into one fp32 ``d_enc``
handed to the encoder engine's ``backward_hidden``) and ``save_pretrained``.  :class:`WhisperAdamW` clips the encoder's and the decoder's gradient buffers by one
global norm and steps both.  Kernels: ssak_amd/csrc/whisper_train.hip (ABI 650) for the attention, cross-entropy and embedding
backward, ``ssak_layernorm_fwd_stats`` / ``ssak_layernorm_bwd``, and ``ssak_gemm_bf16`` for every product (dgrad; wgrad with both
operands K-major, ``accumulate`` and a library-sized split; the GELU pair of fc1 / fc2), ``ssak_colsum_bf16`` for the bias sums.
Every sum has a fixed order: two steps from the same state give the same bits.

Not built: decoder dropout / layerdrop (refused by name; every published Whisper config has them at
0), gradient checkpointing, gradient accumulation, int8 / int4 quantisation of the base, data parallelism.  LoRA on the bf16 base:
ssak_amd/whisper_lora.py (``add_lora``; ``backward`` and :class:`WhisperAdamW` then take their frozen-base branches).
"""
from __future__ import annotations

import json
import os
import shutil
from typing import Optional

import numpy as np
import torch

from . import hip
from .trainer import decay_ranges, hf_decays, linear_warmup_lr

# Rows of the vocabulary projection in flight in a train step (``model.row_chunk``, which run_training raises to this): the step runs
# three products per chunk against the [51 872, 768] embedding and adds to its fp32 gradient once per chunk, so the 256 rows that
# bound the inference workspace leave the step on small-M products (tools/bench_whisper_train.py times both); 2048 rows are 425 MB
# of fp32 logits and 212 MB of bf16 dlogits.
TRAIN_ROW_CHUNK = 2048
_QKV = ("q_proj", "k_proj", "v_proj")  # the order in which the layout packs an attention's projections
_REGULARISERS = ("dropout", "attention_dropout", "activation_dropout", "decoder_layerdrop", "encoder_layerdrop")
# what from_pretrained() takes from generation_config.json
_GENERATION_KEYS = ("lang_to_id", "decoder_start_token_id", "eos_token_id", "pad_token_id", "suppress_tokens", "begin_suppress_tokens",
                    "task_to_id", "no_timestamps_token_id", "max_initial_timestamp_index", "no_speech_token_id")
_TOKENIZER_FILES = ("generation_config.json", "tokenizer.json", "tokenizer_config.json", "vocab.json", "merges.txt", "normalizer.json",
                    "added_tokens.json", "special_tokens_map.json", "preprocessor_config.json")


def shift_tokens_right(labels, pad_token_id: int, decoder_start_token_id: int) -> np.ndarray:
    """transformers' ``shift_tokens_right``: labels [B, L] (-100 = ignored) -> decoder_input_ids [B, L]."""
    labels = np.asarray(labels)
    out = np.empty_like(labels)
    out[:, 1:] = labels[:, :-1]
    out[:, 0] = decoder_start_token_id
    out[out == -100] = pad_token_id
    return out


def decoder_decay_ranges(model):
    """[(offset, count, decays)] covering the decoder's flat buffers (HF Trainer's two weight-decay groups, by parameter name:
    :func:`ssak_amd.trainer.hf_decays`), adjacent parameters of one group merged; the alignment gaps go with the parameter before."""
    items = sorted((off, name) for name, (off, _, _) in model.layout.items())
    total = model.dec_params.numel()
    out = []
    for i, (off, name) in enumerate(items):
        end = items[i + 1][0] if i + 1 < len(items) else total
        d = hf_decays(name, model.config)
        if out and out[-1][2] == d:
            out[-1] = (out[-1][0], end - out[-1][0], d)
        else:
            out.append((off, end - off, d))
    return out


class WhisperTrainMixin:
    """The training methods of :class:`ssak_amd.whisper_seq2seq.WhisperSeq2Seq`."""

    freeze_encoder: bool = False
    # whether the last backward() filled encoder.grads: WhisperAdamW steps the encoder only then (a step on an encoder output the
    # caller computed leaves the encoder out of the clip norm and untouched -- no decay, no moment update on stale gradients)
    encoder_grads_ready: bool = False
    _dec_grads: Optional[torch.Tensor] = None
    _train: Optional[dict] = None

    # ------------------------------------------------------------------ gradients
    @property
    def dec_grads(self) -> torch.Tensor:
        """The decoder's gradients: a flat fp32 buffer with the layout of ``dec_params`` (allocated on first use)."""
        if self._dec_grads is None:
            self._dec_grads = torch.zeros_like(self.dec_params)
        return self._dec_grads

    def dec_grad(self, name: str) -> torch.Tensor:
        off, n, shape = self.layout[name]
        return self.dec_grads[off:off + n].view(shape)

    def _g(self, name: str, rows: int = 1) -> torch.Tensor:
        """Gradient of a weight (``rows`` adjacent tensors as one matrix / vector, as :meth:`_w` / :meth:`_f` take them)."""
        off, n, shape = self.layout["model.decoder." + name]
        return self.dec_grads[off:off + rows * n].view(rows * shape[0], *shape[1:])

    # ------------------------------------------------------------------ forward
    def forward_train(self, x, labels, enc_lens=None, keep_graph: bool = True) -> torch.Tensor:
        """``x``: waveforms [B, T], input features [B, mels, frames] or an encoder output [B, S, D] bf16 (then, or with
        ``freeze_encoder``, the encoder gets no gradient); ``labels`` [B, L] with -100 padding, as the reference's collator makes
        them: ``decoder_input_ids = shift_tokens_right(labels)``.  -> HF's ``.loss`` (the mean cross-entropy over the scored
        tokens), fp32 [1] on the device.  ``keep_graph=False`` (validation) keeps nothing for :meth:`backward`."""
        cfg = self.config
        for name in _REGULARISERS:
            if float(getattr(cfg, name, 0.0) or 0.0) > 0.0:
                raise ValueError(f"{name} = {getattr(cfg, name)}: training with {name} > 0 is not built (every published Whisper "
                                 f"configuration has it at 0)")
        lab = self._ids(labels, "labels")
        B, L = lab.shape
        if L > cfg.max_target_positions:
            raise ValueError(f"{L} label positions, the decoder has {cfg.max_target_positions}")
        if lab.max() >= cfg.vocab_size:
            raise ValueError(f"label {int(lab.max())} outside the vocabulary of {cfg.vocab_size}")
        n_scored = int((lab >= 0).sum())
        if n_scored == 0:
            raise ValueError("the batch has no scored token (every label is -100)")
        lab = np.where(lab < 0, -100, lab)
        pad = cfg.pad_token_id if cfg.pad_token_id is not None else (cfg.eos_token_id if cfg.eos_token_id is not None else 0)
        ids = shift_tokens_right(lab, pad, cfg.decoder_start_token_id)

        x = torch.as_tensor(x)
        train_encoder = keep_graph and not (x.dim() == 3 and x.dtype == torch.bfloat16) and not self.freeze_encoder
        self.encoder.train(train_encoder)  # training mode keeps the encoder's activations for backward_hidden
        try:
            enc = self._as_enc(x)
        finally:
            self.encoder.training = False
        Bx, S, D = enc.shape
        if Bx != B:
            raise ValueError(f"{B} label sequences for {Bx} encoder outputs")
        lens_host = self._enc_lens(enc_lens, B, S)

        layers = []  # (validation runs the keeping entries too and drops what they kept)
        lora_train = keep_graph and self._lora_active()  # adapters: dropout under this step's seed, each t kept
        if keep_graph and self._lora is not None and self._lora_merged:
            raise RuntimeError("forward_train(): the adapters are merged into the shadow; unmerge_lora() before a train step")
        if lora_train:
            self.lora_step += 1
        self._lora_train_pass = lora_train
        try:
            ln_f = self._decoder_hidden(enc, ids, lens_host, keep=layers)
        finally:
            self._lora_train_pass = False
        targets = np.ascontiguousarray(lab.reshape(-1), dtype=np.int32)
        with torch.cuda.device(self.device):
            parts = [hip.token_logprobs(logits, cfg.vocab_size, targets[r0:r0 + n])[1] for r0, n, logits in self._project_chunks(ln_f[1])]
            lp = parts[0] if len(parts) == 1 else torch.cat(parts)
            loss = -(lp.sum(dtype=torch.float32) / n_scored).reshape(1)
        self._train = None if not keep_graph else dict(B=B, L=L, S=S, enc2=enc.reshape(B * S, D), enc_lens=lens_host, ids=ids, targets=targets,
                                                       n_scored=n_scored, layers=layers, ln_f=ln_f, train_encoder=train_encoder,
                                                       lora_seed=self.lora_drop_seed if lora_train else None)
        return loss

    # ------------------------------------------------------------------ backward
    def _dgrad(self, dy: torch.Tensor, w: torch.Tensor, out=None, **kw) -> torch.Tensor:
        """dX [M, K] = dY [M, N] W [N, K] (an nn.Linear's input gradient); ``dy`` may be a column slice."""
        M, No = dy.shape
        Ki = w.shape[1]
        out = torch.empty((M, Ki), dtype=torch.bfloat16, device=self.device) if out is None else out
        return hip.gemm(dy, w, out, M, Ki, No, b_kmajor=True, lda=dy.stride(0), ldb=Ki, ldc=Ki, **kw)

    def _wgrad(self, dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor):
        """dW [N, K] += dY^T X: both operands K-major (the contraction runs over their rows), fp32 accumulate, library-sized split."""
        M, No = dy.shape
        Ki = x.shape[1]
        hip.gemm(dy, x, dw, No, Ki, M, a_kmajor=True, b_kmajor=True, lda=dy.stride(0), ldb=x.stride(0), ldc=Ki, accumulate=True, split_k=0)

    def _bgrad(self, dy: torch.Tensor, db: torch.Tensor):
        """db [N] = the column sums of dY [M, N]."""
        M, No = dy.shape
        ws = hip._ws(hip.lib.ssak_colsum_workspace_bytes(No), self.device)
        hip.check(hip.lib.ssak_colsum_bf16(hip.ptr(dy), dy.stride(0), M, No, hip.ptr(db), hip.ptr(ws), ws.numel(), hip.stream()))

    def _linear_bwd(self, dy: torch.Tensor, x: torch.Tensor, name: str, rows: int = 1, **dgrad):
        """The three gradients of nn.Linear ``name`` (y = x W^T + b) from ``dy``: dW += dY^T X, db = colsum(dY), -> dX = dY W
        (``dgrad``: what the input-gradient product takes on top -- ``out``, ``accumulate``, an epilogue).  ``rows`` = 3 / 2: the packed
        q|k|v / k|v product whose first projection ``name`` is -- one weight gradient and one input gradient over the packed matrix,
        the bias sums per column block.  Whisper's k_proj has no bias: its synthetic slot gets no gradient."""
        self._wgrad(dy, x, self._g(name + ".weight", rows))
        attn, _, proj = name.rpartition(".")
        blocks = [name] if rows == 1 else [f"{attn}.{q}" for q in _QKV[_QKV.index(proj):][:rows]]
        n = dy.shape[1] // rows
        for i, block in enumerate(blocks):
            if not block.endswith("k_proj"):
                self._bgrad(dy[:, i * n:(i + 1) * n], self._g(block + ".bias"))
        return self._dgrad(dy, self._w(name + ".weight", rows), **dgrad)

    def backward(self, grad_scale: float = 1.0):
        """d (grad_scale * loss) / d parameters of the last :meth:`forward_train`: the decoder's into ``dec_grads`` (overwritten), the
        encoder's into ``encoder.grads`` (unless the forward was given an encoder output or ``freeze_encoder`` is set).  Returns
        ``d_enc`` [B, S, D] fp32, the gradient of the encoder output.  With LoRA adapters (``add_lora``) the base is frozen: the
        adapters' gradients go into ``lora_grads``, ``dec_grads`` is never allocated and None is returned."""
        s = self._train
        if s is None:
            raise RuntimeError("backward() needs a forward_train()")
        self._train = None
        if self._lora is not None:  # frozen base: ssak_amd/whisper_lora.py
            return self._backward_lora(s, grad_scale)
        cfg = self.config
        B, L, S, enc2 = s["B"], s["L"], s["S"], s["enc2"]
        D, nh, N, V = cfg.d_model, cfg.decoder_attention_heads, B * L, cfg.vocab_size
        dev = self.device
        bf = lambda *sh: torch.empty(sh, dtype=torch.bfloat16, device=dev)
        with torch.cuda.device(dev):
            self.dec_grads.zero_()
            ln_ws = hip._ws(hip.lib.ssak_layernorm_bwd_workspace_bytes(D), dev)

            def norm_bwd(g1, ln, name, g_res):
                """through LayerNorm ``name`` (saved ``ln`` = (r, out, mean, rstd)): the gradient of r, + ``g_res``"""
                dr = bf(N, D)
                hip.layernorm_bwd(g1, None, ln[0], ln[2], ln[3], self._f(name + ".weight"), g_res, dr, self._g(name + ".weight"),
                                  self._g(name + ".bias"), workspace=ln_ws)
                return dr

            # ---- the vocabulary projection, row_chunk rows at a time: logits -> dlogits -> dX, dE
            xf = s["ln_f"][1]
            E, dE = self._w("embed_tokens.weight"), self._g("embed_tokens.weight")
            Vp = E.shape[0]
            dx = bf(N, D)
            dl_ws = bf(min(self.row_chunk, N), Vp)
            for r0, n, logits in self._project_chunks(xf):
                dl = dl_ws[:n]
                hip.dec_ce_bwd(logits, V, s["targets"][r0:r0 + n], grad_scale / s["n_scored"], dlogits=dl, want_loss=False)  # (the forward has the loss)
                self._dgrad(dl, E, out=dx[r0:r0 + n])
                self._wgrad(dl, xf[r0:r0 + n], dE)
            nl = cfg.decoder_layers
            dh = norm_bwd(dx, s["ln_f"], "layer_norm", None)
            d_enc = torch.zeros((B * S, D), dtype=torch.float32, device=dev)
            for l in reversed(range(nl)):
                p = f"layers.{l}."
                sv = s["layers"][l]
                # feed-forward: dh is the gradient of fc2's output; its input gradient takes GELU's on the way
                dpre = self._linear_bwd(dh, sv["f"], p + "fc2", epilogue=hip.EPI_MUL_GELU_GRAD, aux_in=sv["pre"])
                dh = norm_bwd(self._linear_bwd(dpre, sv["ln3"][1], p + "fc1"), sv["ln3"], p + "final_layer_norm", dh)
                # cross-attention: the k|v product's input gradient adds to d_enc
                a = p + "encoder_attn."
                dctx = self._linear_bwd(dh, sv["ctx_c"], a + "out_proj")
                dq, dkv = bf(N, D), bf(B * S, 2 * D)
                kv = sv["kv_c"]
                hip.dec_attention_bwd(sv["q_c"], kv[:, :D], kv[:, D:], sv["ctx_c"], sv["lse_c"], dctx, dq, dkv[:, :D], dkv[:, D:], B, L, S, nh,
                                      klens=s["enc_lens"])
                self._linear_bwd(dkv, enc2, a + "k_proj", 2, out=d_enc, accumulate=True)
                dh = norm_bwd(self._linear_bwd(dq, sv["ln2"][1], a + "q_proj"), sv["ln2"], p + "encoder_attn_layer_norm", dh)
                # causal self-attention
                a = p + "self_attn."
                dctx = self._linear_bwd(dh, sv["ctx_s"], a + "out_proj")
                dqkv = bf(N, 3 * D)
                qkv = sv["qkv"]
                hip.dec_attention_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], sv["ctx_s"], sv["lse_s"], dctx, dqkv[:, :D], dqkv[:, D:2 * D],
                                      dqkv[:, 2 * D:], B, L, L, nh, causal=True)
                dh = norm_bwd(self._linear_bwd(dqkv, sv["ln1"][1], a + "q_proj", 3), sv["ln1"], p + "self_attn_layer_norm", dh)
            # ---- the embedding's other use: the rows gathered per token, the positions summed over the batch
            hip.dec_embed_bwd(dh, s["ids"], dE, self._g("embed_positions.weight"), 0)
            self.encoder_grads_ready = bool(s["train_encoder"])
            if s["train_encoder"]:
                d_enc_bf = bf(B, S, D)
                hip.check(hip.lib.ssak_cast_f32_bf16(hip.ptr(d_enc), hip.ptr(d_enc_bf), d_enc.numel(), hip.stream()))
                self.encoder.backward_hidden(d_enc_bf)
        return d_enc.view(B, S, D)

    # ------------------------------------------------------------------ checkpoint
    def state_dict_hf(self):
        """fp32 tensors under transformers' names: ``model.encoder.*``, ``model.decoder.*`` and the tied ``proj_out.weight``; no
        synthetic k_proj bias slots, no CTC head, the vocabulary's padding rows dropped."""
        torch.cuda.synchronize(self.device)
        V = self.config.vocab_size
        sd = {"model." + k: v for k, v in self.encoder.state_dict().items() if not k.startswith("ctc_head.")}
        for name in self.layout:
            if name.endswith("k_proj.bias"):
                continue
            t = self.dec_param(name).detach().cpu().clone()
            sd[name] = t[:V].contiguous() if name.endswith("embed_tokens.weight") else t
        sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"].clone()
        return sd

    def save_pretrained(self, folder: str):
        """``model.safetensors`` (:meth:`state_dict_hf`) plus ``config.json``, ``generation_config.json`` and the tokenizer files of
        the folder the model was loaded from; :meth:`from_pretrained` reads the result back bit for bit."""
        from safetensors.torch import save_file
        os.makedirs(folder, exist_ok=True)
        save_file({k: v.contiguous() for k, v in self.state_dict_hf().items()}, os.path.join(folder, "model.safetensors"), metadata={"format": "pt"})
        src = self.name_or_path
        if src is not None and os.path.isfile(os.path.join(src, "config.json")):
            if os.path.abspath(src) != os.path.abspath(folder):
                shutil.copyfile(os.path.join(src, "config.json"), os.path.join(folder, "config.json"))
                for name in _TOKENIZER_FILES:
                    if os.path.isfile(os.path.join(src, name)):
                        shutil.copyfile(os.path.join(src, name), os.path.join(folder, name))
        else:
            # a model built from a configuration object: both files are written from it, split the way from_pretrained() reads them
            import dataclasses
            d = dataclasses.asdict(self.config)
            gen = {k: d.pop(k) for k in _GENERATION_KEYS}
            gen["lang_to_id"] = {f"<|{c}|>": i for c, i in (gen["lang_to_id"] or {}).items()}
            with open(os.path.join(folder, "config.json"), "w") as f:
                json.dump(dict(d, architectures=["WhisperForConditionalGeneration"], model_type="whisper", eos_token_id=gen["eos_token_id"],
                               pad_token_id=gen["pad_token_id"], decoder_start_token_id=gen["decoder_start_token_id"]), f, indent=1)
            with open(os.path.join(folder, "generation_config.json"), "w") as f:
                json.dump({k: v for k, v in gen.items() if v is not None}, f, indent=1)
        return folder


class WhisperAdamW:
    """AdamW over the encoder's and the decoder's flat buffers (``ssak_adamw_step``, bf16 shadows refreshed in the same sweep) under
    ONE global-norm clip (``ssak_grad_sumsq`` on the encoder's gradients, ``ssak_grad_sumsq_add`` on the decoder's), HF Trainer's two
    weight-decay groups and its linear warm-up and decay: ``optim="adamw_torch"`` of whisper_train.py:464-497.  With
    ``model.freeze_encoder`` the encoder's buffers are left alone; so they are in a step whose backward did not fill the encoder's
    gradients (``model.encoder_grads_ready``: the forward was given an encoder output), and the encoder's bias correction counts the
    steps it took (torch keeps ``step`` per parameter)."""

    def __init__(self, model, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=1.0, warmup_steps=0,
                 total_steps=100000):
        self.model = model
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm, self.warmup_steps, self.total_steps = max_grad_norm, warmup_steps, total_steps
        dev = model.device
        enc = model.encoder
        self.train_encoder = not model.freeze_encoder
        # (buffer of parameters, of gradients, of the shadow, count, ranges) per half
        self.halves = []
        if getattr(model, "_lora", None) is not None:
            # adapters: the one half; HF's rule decays every LoRA weight (no name holds "bias" or a LayerNorm), the clip norm runs
            # over the adapter gradients alone and the base gets neither moments nor a gradient buffer
            self.train_encoder = False
            n = model.lora_params.numel()
            self.halves.append((model.lora_params, model.lora_grads, model.lora_shadow, n, [(0, n, True)]))
        else:
            if self.train_encoder:
                self.halves.append((enc.params, enc.grads, enc.shadow, enc.num_trainable, decay_ranges(enc)))
            self.halves.append((model.dec_params, model.dec_grads, model.dec_shadow, model.dec_params.numel(), decoder_decay_ranges(model)))
        self.exp_avg = [torch.zeros(n, dtype=torch.float32, device=dev) for _, _, _, n, _ in self.halves]
        self.exp_avg_sq = [torch.zeros(n, dtype=torch.float32, device=dev) for _, _, _, n, _ in self.halves]
        self.gnorm_sq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._sumsq_ws = torch.empty(1024, dtype=torch.float32, device=dev)
        self.step_count = 0
        self.half_steps = [0] * len(self.halves)  # optimizer steps each half has taken

    def current_lr(self) -> float:
        return linear_warmup_lr(self.lr, self.step_count, self.warmup_steps, self.total_steps)

    def step(self, grad_scale: float = 1.0):
        lr = self.current_lr()
        self.step_count += 1
        with torch.cuda.device(self.model.device):
            st = hip.stream()
            step_encoder = self.train_encoder and self.model.encoder_grads_ready
            active = [i for i in range(len(self.halves)) if step_encoder or not (self.train_encoder and i == 0)]
            for j, i in enumerate(active):
                _, g, _, n, _ = self.halves[i]
                fn = hip.lib.ssak_grad_sumsq if j == 0 else hip.lib.ssak_grad_sumsq_add
                hip.check(fn(hip.ptr(g), n, hip.ptr(self.gnorm_sq), hip.ptr(self._sumsq_ws), self._sumsq_ws.numel() * 4, st))
            for i in active:
                (p, g, sh, n, ranges), m, v = self.halves[i], self.exp_avg[i], self.exp_avg_sq[i]
                self.half_steps[i] += 1
                todo = [(0, n, 0.0)] if self.weight_decay == 0.0 else [(off, cnt, self.weight_decay if d else 0.0) for off, cnt, d in ranges]
                for off, cnt, wd in todo:
                    hip.check(hip.lib.ssak_adamw_step(hip.ptr(p[off:]), hip.ptr(g[off:]), hip.ptr(m[off:]), hip.ptr(v[off:]), hip.ptr(sh[off:]), cnt,
                                                      hip.ptr(self.gnorm_sq), self.max_grad_norm, grad_scale, lr, self.betas[0], self.betas[1],
                                                      self.eps, wd, self.half_steps[i], st))
        if step_encoder:
            self.model.encoder.sync_weights(full=False)

    def grad_norm(self, grad_scale: float = 1.0) -> float:
        return float(self.gnorm_sq.sqrt().item()) * grad_scale
