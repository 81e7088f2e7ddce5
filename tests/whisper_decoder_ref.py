"""float64 NumPy restatement of the Whisper text decoder as ssak_amd/whisper_seq2seq.py runs it: the embedding, the attention
(causal, ``q_offset``, ``klens``), the per-row log-softmax statistics (with and without an ``allowed`` list), the whole decoder
stack of transformers' ``WhisperForConditionalGeneration`` (pre-LN layers: self-attention, cross-attention, feed-forward; final
LayerNorm; vocabulary projection against the tied embedding), the three transcript scores and ``whisper.decoding``'s language
softmax.  tests/test_whisper_decoder_ref.py holds it to transformers in float64; the GPU tests hold the kernels to it.

``rnd``: every function that models a stored tensor takes a rounding function applied where the device stores one (identity =
the exact float64 value; :func:`bf16_round` = the device's storage roundings, which is how the GPU tests' bars are measured).
"""
import math

import numpy as np

HEAD_DIM = 64
_erf = np.vectorize(math.erf, otypes=[np.float64])


def identity(x):
    return x


def bf16_round(x):
    """Round to the nearest bf16 (ties to even), returned as float64."""
    f = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))
    u = f.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def bf16_bits(x):
    """float array (exactly representable in bf16) -> uint16 bit patterns."""
    f = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    return (f.view(np.uint32) >> 16).astype(np.uint16).reshape(f.shape)


def bf16_from_bits(u):
    return (np.asarray(u, dtype=np.uint32) << 16).view(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- pieces
def embed(embed_tokens, embed_positions, ids, pos_offset=0, rnd=identity):
    """out[b, i] = embed_tokens[ids[b, i]] + embed_positions[pos_offset + i]"""
    ids = np.asarray(ids)
    L = ids.shape[1]
    return rnd(embed_tokens[ids] + embed_positions[pos_offset:pos_offset + L][None])


def attention(q, k, v, nh, klens=None, causal=False, q_offset=0, rnd=identity, stats=False):
    """q [B, Lq, D], k / v [B, Lk, D] -> ctx [B, Lq, D] = softmax(q k^T * 64^-1/2 + mask) v per head.  Key j is visible to query i
    iff j < klens[b] and, when causal, j <= q_offset + i.  ``rnd`` rounds P into the second product (the row sum is that of the
    unrounded P) and the stored ctx.  ``stats``: also ctx_mag = sum_j P |v|, amax = max_j sum_d |q k| / 8 and smax = max |score|
    per (b, h, query), the terms of the GPU test's bar."""
    B, Lq, D = q.shape
    Lk = k.shape[1]
    assert D == nh * HEAD_DIM
    klens = [Lk] * B if klens is None else list(klens)
    ctx = np.zeros((B, Lq, D))
    ctx_mag = np.zeros((B, Lq, D))
    amax = np.zeros((B, nh, Lq))
    smax = np.zeros((B, nh, Lq))
    j = np.arange(Lk)[None, :]
    i = np.arange(Lq)[:, None]
    for b in range(B):
        vis = j < klens[b]
        if causal:
            vis = vis & (j <= q_offset + i)
        vis = np.broadcast_to(vis, (Lq, Lk))
        assert vis.any(-1).all(), "a fully masked query row"
        for h in range(nh):
            sl = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
            qs = q[b, :, sl] * 0.125
            s = qs @ k[b, :, sl].T
            s = np.where(vis, s, -np.inf)
            m = s.max(-1, keepdims=True)
            e = np.exp(s - m)
            den = e.sum(-1, keepdims=True)
            ctx[b, :, sl] = (rnd(e) @ v[b, :, sl]) / den
            if stats:
                p = e / den
                ctx_mag[b, :, sl] = p @ np.abs(v[b, :, sl])
                a = np.abs(qs) @ np.abs(k[b, :, sl]).T
                amax[b, h] = np.where(vis, a, 0).max(-1)
                smax[b, h] = np.where(vis, np.abs(s), 0).max(-1)
    ctx = rnd(ctx)
    return (ctx, dict(ctx_mag=ctx_mag, amax=amax, smax=smax)) if stats else ctx


def token_logprobs(logits, targets=None, allowed=None):
    """logits [R, V] -> dict(lse [R], logprob [R] (0 where target < 0), argmax [R] (lowest id on ties), probs [R, n_allowed] | None);
    with ``allowed`` the softmax runs over those columns only."""
    logits = np.asarray(logits, dtype=np.float64)
    R = logits.shape[0]
    cols = np.arange(logits.shape[1]) if allowed is None else np.asarray(allowed)
    x = logits[:, cols]
    m = x.max(-1, keepdims=True)
    e = np.exp(x - m)
    lse = (m + np.log(e.sum(-1, keepdims=True)))[:, 0]
    out = dict(lse=lse, argmax=cols[np.argmax(x, -1)], probs=None if allowed is None else e / e.sum(-1, keepdims=True), logprob=None)
    if targets is not None:
        t = np.asarray(targets)
        out["logprob"] = np.where(t >= 0, logits[np.arange(R), np.maximum(t, 0)] - lse, 0.0)
    return out


def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


# ---------------------------------------------------------------------------------------------------------------- the stack
def decoder_logits(p, nh, n_layers, enc, tokens, enc_lens=None, pos_offset=0, rnd=identity, prefix="model.decoder."):
    """p: float64 arrays under transformers' names (``model.decoder.*``; ``proj_out`` tied to ``embed_tokens``); enc [B, S, D];
    tokens [B, L] -> logits [B, L, V] of every position (teacher forcing).  ``rnd`` as in the module docstring: applied to every
    tensor the device stores in bf16 (the logits stay fp32)."""
    g = lambda n: np.asarray(p[prefix + n], dtype=np.float64)
    lin = lambda x, n, bias=True: x @ g(n + ".weight").T + (g(n + ".bias") if bias else 0.0)
    enc = rnd(np.asarray(enc, dtype=np.float64))
    E = g("embed_tokens.weight")
    h = embed(E, g("embed_positions.weight"), tokens, pos_offset, rnd)
    for l in range(n_layers):
        L = f"layers.{l}."
        x = rnd(layer_norm(h, g(L + "self_attn_layer_norm.weight"), g(L + "self_attn_layer_norm.bias")))
        q, k, v = rnd(lin(x, L + "self_attn.q_proj")), rnd(lin(x, L + "self_attn.k_proj", False)), rnd(lin(x, L + "self_attn.v_proj"))
        a = attention(q, k, v, nh, None, True, 0, rnd)
        h = rnd(h + rnd(lin(a, L + "self_attn.out_proj")))
        x = rnd(layer_norm(h, g(L + "encoder_attn_layer_norm.weight"), g(L + "encoder_attn_layer_norm.bias")))
        q = rnd(lin(x, L + "encoder_attn.q_proj"))
        k, v = rnd(lin(enc, L + "encoder_attn.k_proj", False)), rnd(lin(enc, L + "encoder_attn.v_proj"))
        a = attention(q, k, v, nh, enc_lens, False, 0, rnd)
        h = rnd(h + rnd(lin(a, L + "encoder_attn.out_proj")))
        x = rnd(layer_norm(h, g(L + "final_layer_norm.weight"), g(L + "final_layer_norm.bias")))
        f = rnd(gelu(lin(x, L + "fc1")))
        h = rnd(h + rnd(lin(f, L + "fc2")))
    x = rnd(layer_norm(h, g("layer_norm.weight"), g("layer_norm.bias")))
    return x @ E.T


# ---------------------------------------------------------------------------------------------------------------- scores
def shifted_targets(tokens, lens=None):
    """labels [B, L]: labels[b, i] = tokens[b, i + 1] for i + 1 < lens[b], else -100 (HF's ignore index)."""
    tokens = np.asarray(tokens)
    B, L = tokens.shape
    lens = [L] * B if lens is None else lens
    lab = np.full((B, L), -100, dtype=np.int64)
    for b in range(B):
        lab[b, :lens[b] - 1] = tokens[b, 1:lens[b]]
    return lab


def scores(logits, tokens, lens=None):
    """logits [B, L, V] of the teacher-forced pass on ``tokens`` -> dict(logprobs [B, L - 1], sum_logprob [B], avg_logprob [B] =
    sum / (n_scored + 1) (whisper/decoding.py), loss [B] = the utterance's mean cross-entropy, batch_loss = HF's ``.loss``: the
    mean over every label other than -100 of the batch)."""
    B, L, V = logits.shape
    lab = shifted_targets(tokens, lens)
    lp = token_logprobs(logits.reshape(B * L, V), lab.reshape(-1))["logprob"].reshape(B, L)[:, :L - 1]
    n = (lab >= 0).sum(-1)
    s = lp.sum(-1)
    return dict(logprobs=lp, sum_logprob=s, avg_logprob=s / (n + 1), loss=-s / np.maximum(n, 1), batch_loss=-s.sum() / n.sum(), n_scored=n)


def language_probs(logits_row, lang_ids):
    """whisper.decoding.detect_language on the logits [B, V] of the position after <|startoftranscript|>: every non-language
    token masked to -inf, softmax, arg-max -> (ids [B] token ids, probs [B, n_lang] in the order of ``lang_ids``)."""
    r = token_logprobs(logits_row, None, lang_ids)
    return r["argmax"], r["probs"]
