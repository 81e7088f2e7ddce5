"""Float64 restatements of whisper's beam search (whisper/decoding.py: BeamSearchDecoder.update / finalize, MaximumLikelihoodRanker),
the contract of ssak_dec_beam_topk / ssak_dec_beam_select and of ``WhisperSeq2Seq.generate(beam_size=...)``.  Two forms of the update:

* :func:`update_dict` -- whisper's own: a dict keyed by the candidate SEQUENCE, filled beam by beam and rank by rank, walked through
  Python's stable ``sorted(..., reverse=True)``; the finished sequences in a dict per audio.
* :func:`update_array` -- what the kernels implement: candidates (beam, rank) ordered by (score descending, beam, rank), sources as
  row indices, the finished store as a list, a done audio frozen.

Both take the K = nb + 1 best of each row from :func:`topk_stable` (log-prob descending, a tie to the lowest column; columns at -inf
are not offered), so ties are defined.  A beam whose sum is -inf offers nothing: a call starts with sums [0, -inf, ...], which is
whisper's first step (all beams hold the same prefix, and its dict keeps one copy of each sequence).  No patience, ``max_candidates
= nb``.  numpy only.
"""
import numpy as np


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = np.max(np.where(np.isfinite(x), x, -np.inf), axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def topk_stable(logprob, K):
    """-> [(column, logprob)] of the K largest, highest first, a tie to the lowest column; -inf columns are not offered."""
    lp = np.asarray(logprob, dtype=np.float64)
    order = np.lexsort((np.arange(lp.size), -lp))[:K]
    return [(int(c), float(lp[c])) for c in order if lp[c] > -np.inf]


def update_dict(prefixes, sums, logprobs, nb, eos, finished):
    """whisper's update for ONE audio.  prefixes: nb token lists; sums [nb]; logprobs [nb, V] (the processed rows' log-softmax);
    finished: the audio's dict sequence -> score, updated in place.  -> (next prefixes, sources, next sums, completed)."""
    scores, sources = {}, {}
    for j in range(nb):
        if sums[j] == -np.inf:
            continue
        for token, lp in topk_stable(logprobs[j], nb + 1):
            seq = tuple(prefixes[j]) + (token,)
            if seq not in scores:  # (the first step of whisper: every beam offers the same sequences, the dict keeps one)
                sources[seq] = j
            scores[seq] = sums[j] + lp
    nxt, src, new_sums, newly = [], [], [], {}
    for seq in sorted(scores, key=scores.get, reverse=True):
        if seq[-1] == eos:
            newly[seq] = scores[seq]
        else:
            nxt.append(list(seq)), src.append(sources[seq]), new_sums.append(scores[seq])
            if len(nxt) == nb:
                break
    for seq in sorted(newly, key=newly.get, reverse=True):
        if len(finished) >= nb:
            break
        finished[seq] = newly[seq]
    return nxt, src, new_sums, len(finished) >= nb


def update_array(hist, sums, cands, nb, eos, pad, fin, done):
    """The kernels' update for ONE audio.  hist: nb token lists of equal length; sums [nb]; cands: per beam the list of (token,
    logprob) :func:`topk_stable` gave; fin: the audio's list of (tokens with eos, score), appended in place; done: was the audio
    done on entry.  -> (tokens [nb], sources [nb], sums [nb], logprobs [nb], done)."""
    if done:
        return [pad] * nb, list(range(nb)), list(sums), [0.0] * nb, True
    K = nb + 1
    flat = []
    for j in range(nb):
        if sums[j] == -np.inf:
            continue
        for r, (token, lp) in enumerate(cands[j][:K]):
            flat.append((-(sums[j] + lp), j, r, token, lp))
    flat.sort(key=lambda c: c[:3])
    tok, src, new, lps = [], [], [], []
    for neg, j, r, token, lp in flat:
        if token == eos:
            if len(fin) < nb:
                fin.append((list(hist[j]) + [eos], -neg))
        else:
            tok.append(token), src.append(j), new.append(-neg), lps.append(lp)
            if len(tok) == nb:
                break
    for s in range(len(tok), nb):
        tok.append(pad), src.append(s), new.append(-np.inf), lps.append(0.0)
    return tok, src, new, lps, len(fin) >= nb


def finalize(hist, sums, fin, nb):
    """-> the nb candidates [(tokens, sum, finished?)]: the finished in the order they finished, then the live hypotheses by
    ``list(np.argsort(sums))[::-1]``, skipping -inf, without eos."""
    out = [(list(t), float(s), True) for t, s in fin]
    for j in list(np.argsort(np.asarray(sums, dtype=np.float64)))[::-1]:
        if len(out) >= nb:
            break
        if sums[j] > -np.inf:
            out.append((list(hist[j]), float(sums[j]), False))
    return out


def rank(cands, length_penalty=None):
    """MaximumLikelihoodRanker: sum / length (the tokens before eos), or sum / ((5 + length) / 6) ** a; length 0 -> -inf; np.argmax."""
    scores = []
    for toks, s, finished in cands:
        n = len(toks) - 1 if finished else len(toks)
        scores.append(-np.inf if n == 0 else s / (n if length_penalty is None else ((5 + n) / 6) ** length_penalty))
    return int(np.argmax(scores))


def search_dict(logprob_fn, nb, eos, max_new, length_penalty=None):
    """whisper's loop for one audio: ``logprob_fn(prefix) -> [V]``.  -> (candidates as :func:`finalize` gives them, winner)."""
    prefixes, sums, finished = [[] for _ in range(nb)], [0.0] + [-np.inf] * (nb - 1), {}
    for _ in range(max_new):
        lps = [logprob_fn(p) if s > -np.inf else None for p, s in zip(prefixes, sums)]
        prefixes, src, sums, completed = update_dict(prefixes, sums, lps, nb, eos, finished)
        while len(prefixes) < nb:  # (the candidates ran out: no live hypothesis in this slot)
            prefixes.append([]), sums.append(-np.inf)
        if completed:
            break
    cands = [(list(seq), float(s), True) for seq, s in finished.items()]
    for j in list(np.argsort(np.asarray(sums)))[::-1]:  # (whisper appends eos here without an eos term; the length is the same)
        if len(cands) >= nb:
            break
        if sums[j] > -np.inf:
            cands.append((list(prefixes[j]), float(sums[j]), False))
    return cands, rank(cands, length_penalty)


def search_array(logprob_fns, nb, eos, pad, max_new, length_penalty=None):
    """The kernels' loop over a lock-step batch (one ``logprob_fn`` per audio): done audios are frozen, the loop ends when every
    audio is done or after ``max_new`` steps.  -> per audio (candidates, winner), and the steps taken."""
    B = len(logprob_fns)
    hist = [[[] for _ in range(nb)] for _ in range(B)]
    sums = [[0.0] + [-np.inf] * (nb - 1) for _ in range(B)]
    fin, done, steps = [[] for _ in range(B)], [False] * B, 0
    for _ in range(max_new):
        for b in range(B):
            cands = [topk_stable(logprob_fns[b](hist[b][j]), nb + 1) if (not done[b] and sums[b][j] > -np.inf) else [] for j in range(nb)]
            tok, src, new, _, d = update_array(hist[b], sums[b], cands, nb, eos, pad, fin[b], done[b])
            hist[b] = [list(hist[b][s]) + [t] for s, t in zip(src, tok)]
            sums[b], done[b] = new, d
        steps += 1
        if all(done):
            break
    out = []
    for b in range(B):
        cands = finalize(hist[b], sums[b], fin[b], nb)
        out.append((cands, rank(cands, length_penalty)))
    return out, steps


def greedy(logprob_fn, eos, max_new):
    """The arg-max loop (the lowest column on a tie) -> (tokens ending at eos if reached, sum)."""
    toks, s = [], 0.0
    for _ in range(max_new):
        (token, lp), = topk_stable(logprob_fn(toks), 1)
        toks.append(token)
        s += lp
        if token == eos:
            break
    return toks, s
