"""float64 NumPy restatement of one ``ssak_dec_timestamp_step`` (include/ssak_hip.h "Whisper timestamps"): whisper's
``ApplyTimestampRules`` in the interval form the kernel uses, the decision between the timestamps' mass and the likeliest text
token, the arg-max with the lowest id on a tie and the log-softmax of the FINAL processed row.  tests/test_whisper_timestamps_ref.py
holds it to ``transformers.generation.logits_process.WhisperTimeStampLogitsProcessor`` followed by arg-max and ``log_softmax`` in
float64; the GPU tests hold the kernel, ``generate(timestamps=True)`` and ``transcribe`` to it.
"""
import numpy as np


def last_timestamp(history, ts_begin):
    """The most recent timestamp id of ``history`` or -1: what the kernel keeps in ``ts_last``."""
    ts = [int(t) for t in history if t >= ts_begin]
    return ts[-1] if ts else -1


def allowed_columns(V, history, ts_begin, no_timestamps, eos, max_initial=None, suppress=None, begin_suppress=None):
    """bool [V]: the columns the rules leave before the mass decision.  ``history``: the row's sampled tokens (n = len)."""
    n = len(history)
    last = n >= 1 and history[-1] >= ts_begin
    pen = n < 2 or history[-2] >= ts_begin
    ok = np.ones(V, dtype=bool)
    for ids in (suppress, begin_suppress if n == 0 else None):
        if ids is not None and len(ids):
            ok[np.asarray(ids)] = False
    ok[no_timestamps] = False
    if last and pen:
        ok[ts_begin:] = False
    if last and not pen:
        ok[:eos] = False
    ts_last = last_timestamp(history, ts_begin)
    if ts_last >= 0:
        floor = ts_last if (last and not pen) else ts_last + 1
        ok[ts_begin:max(floor, ts_begin)] = False
    if n == 0:
        ok[:ts_begin] = False
        if max_initial is not None and max_initial >= 0:
            ok[ts_begin + max_initial + 1:] = False
    return ok


def timestamp_step_row(x, history, ts_begin, no_timestamps, eos, max_initial=None, suppress=None, begin_suppress=None):
    """One unfinished row: logits x [V] -> dict(mask = the FINAL allowed columns, token, logprob, margin = |log S_ts - (m_text - M)|
    (inf where one side is empty), gap = the final row's top-two distance (inf with one column), ts_last after the step).  A row
    with no allowed column gives token None."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    ok = allowed_columns(V, history, ts_begin, no_timestamps, eos, max_initial, suppress, begin_suppress)
    ts_last = last_timestamp(history, ts_begin)
    if not ok.any():
        return dict(mask=ok, token=None, logprob=0.0, margin=np.inf, gap=np.inf, ts_last=ts_last)
    M = x[ok].max()
    text, ts = ok.copy(), ok.copy()
    text[ts_begin:] = False
    ts[:ts_begin] = False
    S_text, S_ts = np.exp(x[text] - M).sum(), np.exp(x[ts] - M).sum()
    m_text = x[text].max() if text.any() else -np.inf
    margin = np.inf
    if S_ts > 0 and text.any():
        margin = abs(np.log(S_ts) - (m_text - M))
    if S_ts > 0 and np.log(S_ts) > m_text - M:
        ok = ts
        S = S_ts
    else:
        S = S_text + S_ts
    xs = np.where(ok, x, -np.inf)
    tok = int(xs.argmax())  # (numpy: the lowest index of the maximum)
    top = np.sort(xs[ok])
    gap = float(top[-1] - top[-2]) if top.size > 1 else np.inf
    return dict(mask=ok, token=tok, logprob=float((x[tok] - M) - np.log(S)), margin=float(margin), gap=gap,
                ts_last=tok if tok >= ts_begin else ts_last)


def timestamp_step(logits, histories, finished, eos, pad, ts_begin, no_timestamps, max_initial=None, suppress=None, begin_suppress=None):
    """One ``ssak_dec_timestamp_step`` over a batch: logits [B, V], one history per row, finished [B] bool -> (tokens, logprobs,
    finished after, rows = the per-row dicts, None for a finished row).  A finished row emits ``pad`` with log-probability 0."""
    toks, lps, rows = [], [], []
    for b, h in enumerate(histories):
        if finished[b]:
            toks.append(pad), lps.append(0.0), rows.append(None)
            continue
        r = timestamp_step_row(logits[b], list(h), ts_begin, no_timestamps, eos, max_initial, suppress, begin_suppress)
        toks.append(pad if r["token"] is None else r["token"]), lps.append(r["logprob"]), rows.append(r)
    toks = np.array(toks)
    return toks, np.array(lps), np.asarray(finished, dtype=bool) | (toks == eos), rows


def check_grammar(tokens, ts_begin, eos, no_timestamps, max_initial=None):
    """What ApplyTimestampRules guarantees of a window's sampled tokens (``tokens`` ends at its eos if it reached one): raises
    AssertionError naming the rule."""
    body = [t for t in tokens if t != eos]
    assert eos not in tokens[:-1], "eos ends the window"
    assert no_timestamps not in tokens, "<|notimestamps|> is never emitted"
    assert tokens and tokens[0] >= ts_begin, "the first token is a timestamp"
    if max_initial is not None:
        assert tokens[0] <= ts_begin + max_initial, "the first timestamp is at most max_initial"
    ts = [t for t in body if t >= ts_begin]
    assert all(a <= b for a, b in zip(ts, ts[1:])), "timestamps never decrease"
    flags = [t >= ts_begin for t in body]
    assert not any(a and b and c for a, b, c in zip(flags, flags[1:], flags[2:])), "never three timestamps in a row"
    for i in range(1, len(tokens) - 1):
        if tokens[i - 1] < ts_begin and tokens[i] >= ts_begin:
            assert tokens[i + 1] >= ts_begin or tokens[i + 1] == eos, "after text -> timestamp comes a timestamp or eos"


def generate(p, nh, n_layers, enc, prompt, max_new_tokens, eos, pad, ts_begin, no_timestamps, max_initial=None, suppress=None,
             begin_suppress=None, enc_lens=None):
    """Greedy decoding under the timestamp rules on tests/whisper_decoder_ref.py, the whole prefix recomputed at every step ->
    dict(tokens [B, n], logprobs [B, n], lens [B], margins [B, n], gaps [B, n]); margins / gaps are inf for finished rows."""
    import whisper_decoder_ref as WR
    prompt = np.asarray(prompt)
    B = prompt.shape[0]
    seq = prompt.copy()
    finished = np.zeros(B, dtype=bool)
    hist = [[] for _ in range(B)]
    toks, lps, margins, gaps = [], [], [], []
    for _ in range(max_new_tokens):
        logits = WR.decoder_logits(p, nh, n_layers, enc, seq, enc_lens)[:, -1]
        tok, lp, finished, rows = timestamp_step(logits, hist, finished, eos, pad, ts_begin, no_timestamps, max_initial, suppress, begin_suppress)
        for b in range(B):
            hist[b].append(int(tok[b]))
        toks.append(tok), lps.append(lp)
        margins.append([np.inf if r is None else r["margin"] for r in rows])
        gaps.append([np.inf if r is None else r["gap"] for r in rows])
        seq = np.concatenate([seq, tok[:, None]], 1)
    toks, lps = np.stack(toks, 1), np.stack(lps, 1)
    lens = np.array([int(np.argmax(r == eos)) + 1 if (r == eos).any() else max_new_tokens for r in toks])
    return dict(tokens=toks, logprobs=lps, lens=lens, margins=np.array(margins).T, gaps=np.array(gaps).T)
