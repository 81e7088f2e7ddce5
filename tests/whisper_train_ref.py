"""float64 restatement of the Whisper decoder's training arithmetic (ssak_amd/csrc/whisper_train.hip and its host composition),
written from the definitions and from tests/whisper_decoder_ref.py.

Per-op references (NumPy), each a function of the kernel's OWN inputs, with the magnitude companions the GPU tests' bars need:
:func:`attention_lse`, :func:`attention_bwd`, :func:`ce_bwd`, :func:`embed_bwd`.

The whole decoder (torch float64 autograd over the formulas of whisper_decoder_ref.py: embedding, attention with ``klens`` /
causal, LayerNorm, GELU, tied projection, HF's cross-entropy with -100): :func:`decoder_loss_and_grads` returns the loss, the
gradient of every decoder parameter (the tied embedding's covers both of its uses) and the gradient of ``enc``.
"""
import math

import numpy as np

import whisper_decoder_ref as WR

HEAD_DIM = WR.HEAD_DIM
U8, U = 2.0 ** -8, 2.0 ** -24


def shift_tokens_right(labels, pad_token_id, decoder_start_token_id):
    """transformers.models.whisper.modeling_whisper.shift_tokens_right: labels [B, L] -> decoder_input_ids [B, L]."""
    labels = np.asarray(labels)
    out = np.empty_like(labels)
    out[:, 1:] = labels[:, :-1]
    out[:, 0] = decoder_start_token_id
    out[out == -100] = pad_token_id
    return out


def _visible(Lq, Lk, klen, causal, q_offset):
    j = np.arange(Lk)[None, :]
    i = np.arange(Lq)[:, None]
    vis = j < klen
    if causal:
        vis = vis & (j <= q_offset + i)
    return np.broadcast_to(vis, (Lq, Lk))


def attention_lse(q, k, nh, klens=None, causal=False, q_offset=0):
    """lse [B, nh, Lq] = log sum over the visible keys of exp(q k^T / 8)."""
    B, Lq, D = q.shape
    Lk = k.shape[1]
    klens = [Lk] * B if klens is None else list(klens)
    out = np.zeros((B, nh, Lq))
    for b in range(B):
        vis = _visible(Lq, Lk, klens[b], causal, q_offset)
        for h in range(nh):
            sl = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
            s = np.where(vis, (q[b, :, sl] * 0.125) @ k[b, :, sl].T, -np.inf)
            m = s.max(-1)
            out[b, h] = m + np.log(np.exp(s - m[:, None]).sum(-1))
    return out


def attention_bwd(q, k, v, ctx, lse, dctx, nh, klens=None, causal=False, q_offset=0, n_q_tiles=None, n_k_tiles=None):
    """ssak_dec_attention_bwd as a function of its inputs: q [B, Lq, D], k / v [B, Lk, D], ctx / dctx [B, Lq, D], lse [B, nh, Lq].
    P = exp(q k^T / 8 - lse) on the visible keys, delta = rowsum(dctx ctx), dP = dctx v^T, dS = P (dP - delta), dq = dS k / 8,
    dk = dS^T q / 8, dv = P^T dctx.  Returns dict(dq, dk, dv, delta) and dict(bar_dq, bar_dk, bar_dv, bar_delta): the
    per-element error bounds of the kernel's roundings (derivation: tests/test_gpu_whisper_train_kernels.py)."""
    B, Lq, D = q.shape
    Lk = k.shape[1]
    klens = [Lk] * B if klens is None else list(klens)
    Tk = math.ceil(Lk / 32) if n_k_tiles is None else n_k_tiles
    Tq = math.ceil(Lq / 32) if n_q_tiles is None else n_q_tiles
    dq, dk, dv = np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    bq, bk, bv = np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    delta = np.zeros((B, nh, Lq))
    bdelta = np.zeros((B, nh, Lq))
    for b in range(B):
        vis = _visible(Lq, Lk, klens[b], causal, q_offset)
        for h in range(nh):
            sl = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
            qs, kk, vv, do, o = q[b, :, sl] * 0.125, k[b, :, sl], v[b, :, sl], dctx[b, :, sl], ctx[b, :, sl]
            kz, vz = np.where(vis.any(0)[:, None], kk, 0.0), np.where(vis.any(0)[:, None], vv, 0.0)  # never-visible keys may be poisoned
            s = qs @ kz.T
            amag = np.abs(qs) @ np.abs(kz).T  # sum_d |q k| / 8 per (i, j)
            P = np.where(vis, np.exp(s - lse[b, h][:, None]), 0.0)
            dl = (do * o).sum(-1)
            dmag = (np.abs(do) * np.abs(o)).sum(-1)
            dP = do @ vz.T
            dpmag = np.abs(do) @ np.abs(vz).T
            dS = P * (dP - dl[:, None])
            dq[b, :, sl], dk[b, :, sl], dv[b, :, sl] = 0.125 * (dS @ kz), dS.T @ qs, P.T @ do
            delta[b, h] = dl
            # ---- bars
            bd = 12 * U * dmag
            bdelta[b, h] = bd
            # relative error of a recomputed probability: score sum (2 roundings against amag), * log2 e, lse * log2 e, the
            # subtraction, v_exp_f32
            epsP = U * (2 * amag + 2 * np.abs(s) + 3 * np.abs(lse[b, h])[:, None] + 4)
            EdS = P * ((epsP + 3 * U) * np.abs(dP - dl[:, None]) + 2 * U * dpmag + bd[:, None] + U * (np.abs(dP) + np.abs(dl)[:, None])) + U8 * np.abs(dS)
            EP = P * (epsP + U8)
            bq[b, :, sl] = 0.125 * (EdS @ np.abs(kz) + (Tk + 8) * U * (np.abs(dS) @ np.abs(kz))) + U8 * np.abs(dq[b, :, sl])
            bk[b, :, sl] = EdS.T @ np.abs(qs) + (Tq + 8) * U * (np.abs(dS).T @ np.abs(qs)) + U8 * np.abs(dk[b, :, sl])
            bv[b, :, sl] = EP.T @ np.abs(do) + (Tq + 8) * U * (P.T @ np.abs(do)) + U8 * np.abs(dv[b, :, sl])
    return dict(dq=dq, dk=dk, dv=dv, delta=delta), dict(dq=bq, dk=bk, dv=bv, delta=bdelta)


def ce_bwd(logits, targets, grad_scale=1.0):
    """logits [R, V] float64, targets [R] (negative: ignored) -> dict(dlogits [R, V], row_loss [R], loss_sum, lse [R])."""
    x = np.asarray(logits, dtype=np.float64)
    t = np.asarray(targets)
    r = WR.token_logprobs(x, t)
    p = np.exp(x - r["lse"][:, None])
    onehot = np.zeros_like(x)
    sc = t >= 0
    onehot[np.nonzero(sc)[0], t[sc]] = 1.0
    d = np.where(sc[:, None], (p - onehot) * grad_scale, 0.0)
    return dict(dlogits=d, row_loss=-r["logprob"], loss_sum=-r["logprob"].sum(), lse=r["lse"], p=p)


def embed_bwd(dh, ids, Vp, max_pos, pos_offset=0):
    """dh [B, L, D], ids [B, L] -> (d_embed_tokens [Vp, D], d_embed_positions [max_pos, D]) and the sums of |terms| of each."""
    ids = np.asarray(ids)
    B, L, D = dh.shape
    dt, dp = np.zeros((Vp, D)), np.zeros((max_pos, D))
    at, ap = np.zeros((Vp, D)), np.zeros((max_pos, D))
    np.add.at(dt, ids.reshape(-1), dh.reshape(B * L, D))
    np.add.at(at, ids.reshape(-1), np.abs(dh).reshape(B * L, D))
    dp[pos_offset:pos_offset + L] = dh.sum(0)
    ap[pos_offset:pos_offset + L] = np.abs(dh).sum(0)
    return dt, dp, at, ap


# ---------------------------------------------------------------------------------------------------------------- the whole decoder
def _torch():
    import torch
    return torch


def _bf16(x):
    torch = _torch()
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _make_round():
    """round(x, fwd, bwd): the value rounded to bf16 on the way forward (``fwd``) and / or its gradient on the way back (``bwd``):
    where the device stores an activation in bf16 it stores that activation's gradient in bf16 too."""
    torch = _torch()

    class Round(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, fwd, bwd):
            ctx.bwd = bwd
            return _bf16(x) if fwd else x.clone()

        @staticmethod
        def backward(ctx, g):
            return (_bf16(g) if ctx.bwd else g), None, None

    return Round.apply


def decoder_loss_and_grads(p, nh, n_layers, enc, labels, enc_lens=None, pad_token_id=0, decoder_start_token_id=0, storage=False,
                           round_weights=False, prefix="model.decoder.", params=None):
    """HF's seq2seq loss of the decoder and its gradients, torch float64 autograd over the formulas of whisper_decoder_ref.py.
    p: float64 arrays under transformers' names; enc [B, S, D]; labels [B, L] (-100 ignored), the inputs being
    ``shift_tokens_right(labels)``; enc_lens [B]: the encoder frames cross-attention sees.
    ``storage``: every tensor the device stores in bf16 is rounded where it is stored -- activations, the residual stream, P into
    its products -- and so is its gradient on the way back (dS, dlogits and the activation gradients).
    ``round_weights``: the products read the weights rounded to bf16 (the engine's shadow), the gradient goes to the master.
    ``params``: torch leaf tensors to use instead of ``p`` (an optimizer's).
    -> (loss, {name: gradient}, d_enc [B, S, D]) as float / NumPy arrays."""
    torch = _torch()
    rnd = _make_round()
    R = (lambda x: rnd(x, True, True)) if storage else (lambda x: x)
    Rg = (lambda x: rnd(x, False, True)) if storage else (lambda x: x)
    W = params if params is not None else {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in p.items()
                                           if k.startswith(prefix)}
    g = (lambda n: rnd(W[prefix + n], True, False)) if round_weights else (lambda n: W[prefix + n])
    lin = lambda x, n, bias=True: x @ g(n + ".weight").T + (g(n + ".bias") if bias else 0.0)
    labels = np.asarray(labels)
    B, L = labels.shape
    ids = torch.from_numpy(shift_tokens_right(labels, pad_token_id, decoder_start_token_id).astype(np.int64))
    enc_t = torch.tensor(np.asarray(enc, dtype=np.float64), requires_grad=True)
    S = enc_t.shape[1]
    enc_lens = [S] * B if enc_lens is None else list(enc_lens)

    def layer_norm(x, n, eps=1e-5):
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return (x - mu) / torch.sqrt(var + eps) * g(n + ".weight") + g(n + ".bias")

    def attention(q, k, v, klens, causal):
        Lq, Lk = q.shape[1], k.shape[1]
        out = []
        for b in range(B):
            vis = torch.from_numpy(np.array(_visible(Lq, Lk, klens[b], causal, 0)))
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
        x = R(layer_norm(h, Ln + "self_attn_layer_norm"))
        q, k, v = R(lin(x, Ln + "self_attn.q_proj")), R(lin(x, Ln + "self_attn.k_proj", False)), R(lin(x, Ln + "self_attn.v_proj"))
        a = R(attention(q, k, v, [L] * B, True))
        h = R(h + R(lin(a, Ln + "self_attn.out_proj")))
        x = R(layer_norm(h, Ln + "encoder_attn_layer_norm"))
        q = R(lin(x, Ln + "encoder_attn.q_proj"))
        k, v = R(lin(encr, Ln + "encoder_attn.k_proj", False)), R(lin(encr, Ln + "encoder_attn.v_proj"))
        a = R(attention(q, k, v, enc_lens, False))
        h = R(h + R(lin(a, Ln + "encoder_attn.out_proj")))
        x = R(layer_norm(h, Ln + "final_layer_norm"))
        f = R(torch.nn.functional.gelu(R(lin(x, Ln + "fc1"))))
        h = R(h + R(lin(f, Ln + "fc2")))
    x = R(layer_norm(h, "layer_norm"))
    logits = Rg(x @ E.T)
    loss = torch.nn.functional.cross_entropy(logits.reshape(B * L, -1), torch.from_numpy(labels.astype(np.int64)).reshape(-1), ignore_index=-100)
    if params is not None:
        return loss, enc_t
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in W.items()}, enc_t.grad.numpy()


def rel_l2(a, b):
    """|a - b| / |b| over the whole tensor."""
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300))
