"""float64 restatement of the LoRA arithmetic (ssak_amd/csrc/whisper_lora.hip and its host composition in
ssak_amd/whisper_lora.py), written from the definitions.

Per-kernel references (NumPy), each a function of the kernel's OWN inputs -- the device's bf16 operands as float64 and a given
``keep`` array -- returning the exact value and the magnitude sum the GPU tests' bars scale with: :func:`lora_fwd`,
:func:`lora_bwd_input`, :func:`lora_bwd_weights`, :func:`lora_merge`.

The whole decoder with adapters on q_proj / v_proj of both attentions: :func:`decoder_loss_and_lora_grads`, the decoder of
tests/whisper_train_ref.py (same formulas, same storage roundings) with the adapter path in its four linears.
"""
import math

import numpy as np

import whisper_train_ref as TR

HEAD_DIM = TR.HEAD_DIM
U8, U = TR.U8, TR.U
TARGETS = (("self_attn", "q_proj"), ("self_attn", "v_proj"), ("encoder_attn", "q_proj"), ("encoder_attn", "v_proj"))  # ``which`` 0 .. 3


def names(n_layers):
    """PEFT's names of the adapter tensors, in the order of the engine's flat buffers."""
    return [f"model.decoder.layers.{l}.{attn}.{proj}.{leaf}.weight" for l in range(n_layers) for attn, proj in TARGETS
            for leaf in ("lora_A", "lora_B")]


def drop_scale(p):
    """1 / (1 - p) with the engine's 16-bit threshold: the realised drop probability is round(p * 65536) / 65536."""
    return 1.0 if p <= 0 else 1.0 / (1.0 - min(65535.0, float(np.round(np.float32(p) * np.float32(65536.0)))) / 65536.0)


def _xd(x, keep, scale):
    return x if keep is None else x * np.asarray(keep, dtype=np.float64) * scale


# ---------------------------------------------------------------------------------------------------------------- per kernel
def lora_fwd_t(x, A, keep=None, scale=1.0):
    """t = xd A^T (before its rounding to bf16) and sum |xd| |A|."""
    xd = _xd(x, keep, scale)
    return xd @ A.T, np.abs(xd) @ np.abs(A).T


def lora_fwd_y(y, t, B, s):
    """y + s t B^T from the ROUNDED t, and |y| + s |t| |B|^T."""
    return y + s * (t @ B.T), np.abs(y) + abs(s) * (np.abs(t) @ np.abs(B).T)


def lora_bwd_dt(dy, B, s):
    return s * (dy @ B), abs(s) * (np.abs(dy) @ np.abs(B))


def lora_bwd_dx(dt, A, keep=None, scale=1.0, dx=None):
    """(dx +) keep (dt A) scale from the ROUNDED dt, and its magnitude."""
    k = 1.0 if keep is None else np.asarray(keep, dtype=np.float64)
    val, mag = k * (dt @ A) * scale, k * (np.abs(dt) @ np.abs(A)) * scale
    return (val, mag) if dx is None else (dx + val, np.abs(dx) + mag)


def lora_bwd_weights(dy, t, dt, x, s, keep=None, scale=1.0):
    """dB = s dy^T t, dA = dt^T xd, and their magnitude sums."""
    xd = _xd(x, keep, scale)
    return s * (dy.T @ t), dt.T @ xd, abs(s) * (np.abs(dy).T @ np.abs(t)), np.abs(dt).T @ np.abs(xd)


def lora_merge(W, A, B, s):
    return W + s * (B @ A), np.abs(W) + abs(s) * (np.abs(B) @ np.abs(A))


# ---------------------------------------------------------------------------------------------------------------- the whole decoder
def decoder_loss_and_lora_grads(w, lora, nh, n_layers, enc, labels, enc_lens=None, pad_token_id=0, decoder_start_token_id=0, scaling=1.0,
                                masks=None, mask_scale=1.0, storage=False, round_lora=False, params=None, prefix="model.decoder.",
                                want_logits=False):
    """HF's seq2seq loss of the decoder with LoRA adapters on q_proj / v_proj of self_attn and encoder_attn, and the gradients of
    the adapters: y = x W^T + b + scaling * (dropout(x) A^T) B^T.  ``w``: the frozen float64 weights under transformers' names;
    ``lora``: float64 arrays under PEFT's names (:func:`names`); ``masks``: {(layer, which): keep [rows, D]} with
    ``mask_scale`` = 1 / (1 - p), None = no dropout.
    ``storage``: the device's bf16 stores, forward and backward, as ``whisper_train_ref.decoder_loss_and_grads(storage=True)`` has
    them, plus the adapter's own: t, dt, the second store of y (base product, then + adapter) and the second / third store of dx
    (the base's input gradient, then + each adapter's, q before v).
    ``round_lora``: the products read A / B rounded to bf16 (the engine's shadow), the gradient goes to the master.
    ``params``: torch leaf tensors for the adapters (an optimizer's); then the loss tensor is returned.
    ``want_logits``: return the logits [B, L, V] (NumPy) and nothing else.
    -> (loss, {name: gradient})."""
    import torch
    rnd = TR._make_round()
    R = (lambda x: rnd(x, True, True)) if storage else (lambda x: x)
    Rg = (lambda x: rnd(x, False, True)) if storage else (lambda x: x)
    W = {k: torch.tensor(np.asarray(v, dtype=np.float64)) for k, v in w.items() if k.startswith(prefix)}
    Lw = params if params is not None else {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in lora.items()}
    g = lambda n: W[prefix + n]
    ab = (lambda n: rnd(Lw[prefix + n], True, False)) if round_lora else (lambda n: Lw[prefix + n])
    labels = np.asarray(labels)
    B, L = labels.shape
    ids = torch.from_numpy(TR.shift_tokens_right(labels, pad_token_id, decoder_start_token_id).astype(np.int64))
    enc_t = torch.tensor(np.asarray(enc, dtype=np.float64))
    S = enc_t.shape[1]
    enc_lens = [S] * B if enc_lens is None else list(enc_lens)
    lin = lambda x, n, bias=True: x @ g(n + ".weight").T + (g(n + ".bias") if bias else 0.0)

    def adapted(x_base, x_lora, n, layer, which):
        """nn.Linear ``n`` with its adapter: the base product stored, then the adapter added to it and stored again"""
        y = R(lin(x_base, n))
        xd = x_lora
        if masks is not None:
            keep = torch.from_numpy(np.asarray(masks[(layer, which)], dtype=np.float64)).reshape(x_lora.shape)
            xd = x_lora * keep * mask_scale
        t = R(xd @ ab(n + ".lora_A.weight").T)
        return R(y + scaling * (t @ ab(n + ".lora_B.weight").T))

    def layer_norm(x, n, eps=1e-5):
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return (x - mu) / torch.sqrt(var + eps) * g(n + ".weight") + g(n + ".bias")

    def attention(q, k, v, klens, causal):
        Lq, Lk = q.shape[1], k.shape[1]
        out = []
        for b in range(B):
            vis = torch.from_numpy(np.array(TR._visible(Lq, Lk, klens[b], causal, 0)))
            heads = []
            for h in range(nh):
                sl = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
                s = (q[b, :, sl] * 0.125) @ k[b, :, sl].T
                P = torch.softmax(s.masked_fill(~vis, -math.inf), -1)
                heads.append(R(P) @ v[b, :, sl])
            out.append(torch.cat(heads, -1))
        return torch.stack(out)

    E = g("embed_tokens.weight")
    encr = R(enc_t)
    h = R(E[ids] + g("embed_positions.weight")[:L][None])
    for l in range(n_layers):
        Ln = f"layers.{l}."
        # the input gradient of x is stored three times: the packed base product's, + the q adapter's, + the v adapter's
        x_v = Rg(R(layer_norm(h, Ln + "self_attn_layer_norm")))
        x_q = Rg(x_v)
        x_b = Rg(x_q)
        q = adapted(x_b, x_q, Ln + "self_attn.q_proj", l, 0)
        k = R(lin(x_b, Ln + "self_attn.k_proj", False))
        v = adapted(x_b, x_v, Ln + "self_attn.v_proj", l, 1)
        a = R(attention(q, k, v, [L] * B, True))
        h = R(h + R(lin(a, Ln + "self_attn.out_proj")))
        x_q = Rg(R(layer_norm(h, Ln + "encoder_attn_layer_norm")))
        x_b = Rg(x_q)
        q = adapted(x_b, x_q, Ln + "encoder_attn.q_proj", l, 2)
        k = R(lin(encr, Ln + "encoder_attn.k_proj", False))
        v = adapted(encr, encr, Ln + "encoder_attn.v_proj", l, 3)
        a = R(attention(q, k, v, enc_lens, False))
        h = R(h + R(lin(a, Ln + "encoder_attn.out_proj")))
        x = R(layer_norm(h, Ln + "final_layer_norm"))
        f = R(torch.nn.functional.gelu(R(lin(x, Ln + "fc1"))))
        h = R(h + R(lin(f, Ln + "fc2")))
    x = R(layer_norm(h, "layer_norm"))
    logits = Rg(x @ E.T)
    if want_logits:
        return logits.detach().numpy()
    loss = torch.nn.functional.cross_entropy(logits.reshape(B * L, -1), torch.from_numpy(labels.astype(np.int64)).reshape(-1), ignore_index=-100)
    if params is not None:
        return loss
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in Lw.items()}


def random_lora(n_layers, d_model, r, seed, b_scale=0.05):
    """Seeded, bf16-representable adapters with a nonzero B -> {name: float64 array}."""
    import torch
    rng = np.random.default_rng(seed)
    out = {}
    for n in names(n_layers):
        shape = (r, d_model) if ".lora_A." in n else (d_model, r)
        a = rng.uniform(-1, 1, shape) * (1.0 / math.sqrt(d_model) if ".lora_A." in n else b_scale)
        out[n] = torch.from_numpy(a).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
    return out
