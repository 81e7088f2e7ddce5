"""float64 NumPy restatement of Whisper's greedy generation as ssak_amd/whisper_seq2seq.py (``generate``) runs it, on
tests/whisper_decoder_ref.py: the two suppress masks (transformers' ``SuppressTokensLogitsProcessor`` /
``SuppressTokensAtBeginLogitsProcessor``, whisper's ``SuppressTokens`` / ``SuppressBlank``), the arg-max with the lowest id on a
tie, the log-softmax of the PROCESSED row (whisper/decoding.py: filters first, ``log_softmax`` after), eos / pad / finished
handling, and the split-and-combine softmax of ``ssak_dec_attention_step``.  tests/test_whisper_generate_ref.py holds it to
transformers in float64; the GPU tests hold the kernels and the loop to it.  The whole prefix is recomputed at every step (no
cache): at the fixture's sizes that is cheap, and it is what makes the restatement a check of the cache.
"""
import numpy as np

import whisper_decoder_ref as WR


def process(logits, suppress=None, begin_suppress=None, first=False):
    """logits [R, V] -> a copy with the suppressed columns at -inf (``begin_suppress`` only when ``first``)."""
    x = np.array(logits, dtype=np.float64)
    for ids in (suppress, begin_suppress if first else None):
        if ids is not None and len(ids):
            x[:, np.asarray(ids)] = -np.inf
    return x


def log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def greedy_step(logits, finished, eos, pad, suppress=None, begin_suppress=None, first=False):
    """One ``ssak_dec_greedy_step``: logits [B, V], finished [B] bool -> (tokens [B], logprobs [B], finished after the step).  A row
    that was finished emits ``pad`` with log-probability 0; a row that emits ``eos`` becomes finished."""
    lsm = log_softmax(process(logits, suppress, begin_suppress, first))
    tok = lsm.argmax(-1)  # (numpy: the first, i.e. lowest, index of the maximum)
    lp = lsm[np.arange(len(tok)), tok]
    finished = np.asarray(finished, dtype=bool)
    tok = np.where(finished, pad, tok)
    lp = np.where(finished, 0.0, lp)
    return tok, lp, finished | (tok == eos)


def generate(p, nh, n_layers, enc, prompt, max_new_tokens, eos, pad, suppress=None, begin_suppress=None, enc_lens=None, rnd=WR.identity):
    """Greedy decoding of a lock-step batch: prompt [B, P] -> dict(tokens [B, n], logprobs [B, n], lens [B]) with n =
    ``max_new_tokens`` (no early stop: finished rows pad); ``lens[b]`` counts utterance b's tokens up to and including its eos."""
    prompt = np.asarray(prompt)
    B, P = prompt.shape
    seq = prompt.copy()
    finished = np.zeros(B, dtype=bool)
    toks, lps = [], []
    for i in range(max_new_tokens):
        logits = WR.decoder_logits(p, nh, n_layers, enc, seq, enc_lens, rnd=rnd)[:, -1]
        tok, lp, finished = greedy_step(logits, finished, eos, pad, suppress, begin_suppress, first=i == 0)
        toks.append(tok)
        lps.append(lp)
        seq = np.concatenate([seq, tok[:, None]], 1)
    toks, lps = np.stack(toks, 1), np.stack(lps, 1)
    lens = np.array([int(np.argmax(r == eos)) + 1 if (r == eos).any() else max_new_tokens for r in toks])
    return dict(tokens=toks, logprobs=lps, lens=lens)


def split_attention(q, k, v, nh, n_keys, n_split, klens=None):
    """``ssak_dec_attention_step`` as it is organised: q [B, D], k / v [B, cap, D] (rows >= n_keys are never touched) -> ctx [B, D].
    The keys [0, n_keys) are cut into ``n_split`` pieces of ceil(n_keys / n_split); each piece gives (max, sum, O) over its VISIBLE
    keys (j < klens[b]) -- (-inf, 0, 0) when it has none -- and the pieces are combined in order with factor 0 for an empty one."""
    B, D = q.shape
    chunk = -(-n_keys // n_split)
    ctx = np.zeros((B, D))
    for b in range(B):
        klen = n_keys if klens is None else min(max(int(klens[b]), 1), n_keys)
        for h in range(nh):
            sl = slice(h * WR.HEAD_DIM, (h + 1) * WR.HEAD_DIM)
            parts = []
            for s in range(n_split):
                k0, k1 = s * chunk, min((s + 1) * chunk, n_keys, klen)
                if k1 <= k0:
                    parts.append((-np.inf, 0.0, np.zeros(WR.HEAD_DIM)))
                    continue
                sc = k[b, k0:k1, sl] @ (q[b, sl] * 0.125)
                m = sc.max()
                e = np.exp(sc - m)
                parts.append((m, e.sum(), e @ v[b, k0:k1, sl]))
            M = max(m for m, _, _ in parts)
            L, O = 0.0, np.zeros(WR.HEAD_DIM)
            for m, l, o in parts:
                f = 0.0 if m == -np.inf else np.exp(m - M)
                L += f * l
                O += f * o
            ctx[b, sl] = O / L
    return ctx
