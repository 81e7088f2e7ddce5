"""CPU restatement of the LM beam search contract of ssak_amd/lm.py (numpy, the same merge order and tie rule as the device
kernel; float32 by default, float64 with ``dtype=np.float64``), plus the exact objective it approximates:
log P_ctc(y | x) + LM(y).

``beam_decode(..., return_margin=True)`` also returns the run's smallest decision margin (how far the closest decision of
the search was from going the other way), and :func:`analyse` runs both precisions and compares them: a case whose
float64 margin is at least ``DECISIVE_FACTOR`` times its fp32 noise has one right transcript, whatever the rounding."""
import itertools
import math
import time

import numpy as np

from ssak_amd.lm import CLASS_CHAR, CLASS_DELIM, LN10

f32 = np.float32
LP_FLOOR = f32(np.log(1e-15))
NEG = f32(-np.inf)
DECISIVE_FACTOR = 32.0  # margin >= 32 x fp32 noise: headroom for the device's expf / logf against numpy's (unmeasured)


def log_probs(logits, n_labels, dtype=np.float32):
    x = np.asarray(logits, dtype=dtype)[:, :n_labels]
    m = x.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=1, keepdims=True, dtype=dtype))
    return np.maximum(x - lse, dtype(LP_FLOOR)).astype(dtype)


def lse_fixed(*xs, ft=f32):
    xs = [ft(x) for x in xs if x is not None and x != NEG]
    if not xs:
        return ft(NEG)
    m = max(xs)
    s = ft(0)
    for x in xs:
        s = ft(s + np.exp(ft(x - m)))
    return ft(m + np.log(s))


def log10p_f64(lm, ctx, w):
    """``NgramLM.log10p`` with the additions in float64 (the table values are the file's float32 numbers either way)."""
    hl = 0
    while hl < min(len(ctx), lm.order - 1) and ctx[len(ctx) - 1 - hl] >= 0:
        hl += 1
    acc = 0.0
    for k in range(hl, 0, -1):
        h = list(ctx[len(ctx) - k:])
        hit, _ = lm.probe_ngram(h + [w])
        if hit is not None:
            return np.float64(acc + float(hit[0]))
        hb, _ = lm.probe_ngram(h)
        if hb is not None:
            acc += float(hb[1])
    return np.float64(acc + float(lm.uni[w, 0]))


class Scorer:
    """Prefix LM state (lm, partial, trie node, context) and its updates.  The parameters are the float32 numbers the
    device receives; ``dtype`` is the precision of the arithmetic on them."""

    def __init__(self, lm, cls, alpha, beta, unk_score_offset, dtype=np.float32):
        self.lm, self.cls = lm, cls
        self.ft = ft = np.float64 if dtype == np.float64 else np.float32
        self.ln10 = ft(math.log(10.0)) if ft is np.float64 else LN10
        self.alpha, self.beta, self.unk = ft(f32(alpha)), ft(f32(beta)), ft(f32(unk_score_offset))
        self._trie, self._p = {}, {}

    def initial(self):
        return (self.ft(0), self.ft(0), 0, (-1,) * 4 + (self.lm.bos,))

    def _child(self, trie, v):
        r = self._trie.get((trie, v))
        if r is None:
            r = self._trie[(trie, v)] = self.lm.probe_trie(trie, v)[0]
        return r

    def _log10p(self, ctx, word):
        r = self._p.get((ctx, word))
        if r is None:
            r = self.lm.log10p(list(ctx), word) if self.ft is f32 else log10p_f64(self.lm, list(ctx), word)
            self._p[(ctx, word)] = r
        return r

    def _word(self, lm_, trie, ctx):
        ft = self.ft
        wd = self.lm.word_of_node(trie) if trie > 0 else -1
        oov = wd < 0
        word = self.lm.unk if oov else wd
        L = ft(self.ln10 * self._log10p(ctx, word))
        lm2 = ft(lm_ + ft(ft(self.alpha * ft(L + (ft(self.ln10 * self.unk) if oov else ft(0)))) + self.beta))
        return lm2, ctx[1:] + (word,)

    def extend(self, state, v):
        ft = self.ft
        lm_, part, trie, ctx = state
        c = self.cls[v]
        if c == CLASS_CHAR:
            t2 = self._child(trie, v) if trie >= 0 else -1
            return (lm_, ft(0) if t2 >= 0 else ft(self.alpha * ft(self.ln10 * self.unk)), t2, ctx)
        if c == CLASS_DELIM and trie != 0:
            lm2, ctx2 = self._word(lm_, trie, ctx)
            return (lm2, ft(0), 0, ctx2)
        return state

    def final(self, state):
        ft = self.ft
        lm_, part, trie, ctx = state
        if trie != 0:
            lm_, ctx = self._word(lm_, trie, ctx)
        return ft(lm_ + ft(self.alpha * ft(self.ln10 * self._log10p(ctx, self.lm.eos))))

    def of_labels(self, ids):
        st = self.initial()
        for v in ids:
            st = self.extend(st, v)
        return st


def _min_gap(tots, upto, ties):
    """Smallest gap that decides the order of the descending ``tots[:upto + 1]``; with ``ties`` exact ties are decided
    by the enumeration index (by construction of the case), so only the gaps between distinct values count."""
    g = math.inf
    for k in range(min(upto, len(tots) - 1)):
        d = float(tots[k]) - float(tots[k + 1])
        if d > 0 or not ties:
            g = min(g, d)
    return g


def beam_decode(logits, length, lm, cls, blank, alpha=0.5, beta=1.0, beam_width=100, beam_prune_logp=-10.0,
                token_min_logp=-5.0, unk_score_offset=-10.0, dtype=np.float32, return_margin=False, ties=False, trace=None,
                tie_sign=1):
    """-> (label ids of the winner, its total score), or with ``return_margin`` -> (ids, score, margin).

    ``margin``: the minimum over the frames of (a) total[W-1] - total[W] of the sorted candidates when more than W exist,
    (b) |total - (best + beam_prune_logp)| over the top-W candidates, (c) |lp[t, v] - token_min_logp| over the labels,
    and at the end (d) the best final total minus the second best.  Rank swaps among kept beams only change enumeration
    indices, which matter in exact ties only; a case built on exact ties sets ``ties``: then the order of kept beams
    counts too, and in (a) and (d) only gaps between distinct values count (equal values are decided by the index).
    ``trace``: a dict that receives ``frames`` (per frame {(prefix hash, last): total} of the kept beams, the final
    totals last), ``max_kept`` and ``tie_cutoffs`` (frames in which total[W-1] == total[W]).  ``tie_sign=-1`` is the WRONG
    tie rule (the larger enumeration index wins): for tests that show that a case would notice it."""
    ft = np.float64 if dtype == np.float64 else np.float32
    n_labels = len(cls)
    lp = log_probs(np.asarray(logits)[:length], n_labels, ft)
    sc = Scorer(lm, cls, alpha, beta, unk_score_offset, ft)
    tmin, prune = ft(f32(token_min_logp)), ft(f32(beam_prune_logp))
    # prefixes are interned: node -> (parent, label), LM state and an order-independent hash of the label sequence
    par, lab, hk, states, child = [-1], [-1], [0], [sc.initial()], {}
    beams = [(0, -1, ft(0))]  # (prefix node, last (-1 = blank), acoustic) in rank order
    margin, frames, max_kept, tie_cutoffs = math.inf, [], 1, 0
    for t in range(length):
        row = lp[t]
        amax = int(np.argmax(row))
        S = [v for v in range(n_labels) if row[v] >= tmin or v == amax]
        if tmin > -np.inf:
            margin = min(margin, float(np.abs(row - tmin).min()))
        cands = {}
        for i, (P, last, ac) in enumerate(beams):
            for j, v in enumerate(S):
                e = i * len(S) + j
                s = ft(ac + row[v])
                if v == blank:
                    key, role = (P, -1), (0 if last < 0 else 1)
                elif v == last:
                    key, role = (P, v), 0
                else:
                    Q = child.get((P, v))
                    if Q is None:
                        Q = child[(P, v)] = len(par)
                        par.append(P)
                        lab.append(v)
                        hk.append(hash((hk[P], v)))
                        states.append(sc.extend(states[P], v))
                    key, role = (Q, v), (1 if last < 0 else 2)
                ent = cands.setdefault(key, [{}, e])
                ent[0][role] = s
                ent[1] = min(ent[1], e)
        scored = []
        for (P, last), (src, e) in cands.items():
            ac = lse_fixed(src.get(0), src.get(1), src.get(2), ft=ft)
            lm_, part = states[P][0], states[P][1]
            scored.append((ft(ft(ac + lm_) + part), e, P, last, ac))
        scored.sort(key=lambda r: (-r[0], tie_sign * r[1]))
        tots = [r[0] for r in scored]
        if len(scored) > beam_width:
            tie_cutoffs += tots[beam_width - 1] == tots[beam_width]
            if ties:  # the order of the kept beams and the first distinct value below the cutoff
                k = beam_width
                while k < len(tots) - 1 and tots[k] == tots[beam_width - 1]:
                    k += 1
                margin = min(margin, _min_gap(tots, k, True))
            else:
                margin = min(margin, float(tots[beam_width - 1]) - float(tots[beam_width]))
        elif ties:
            margin = min(margin, _min_gap(tots, len(tots) - 1, True))
        scored = scored[:beam_width]
        floor = ft(scored[0][0] + prune)
        if prune > -np.inf:
            margin = min(margin, min(abs(float(r[0]) - float(floor)) for r in scored))
        beams = [(P, last, ac) for tot, e, P, last, ac in scored if tot >= floor]
        max_kept = max(max_kept, len(beams))
        if trace is not None:
            frames.append({(hk[P], last): float(tot) for tot, e, P, last, ac in scored if tot >= floor})
    finals = {}
    for i, (P, last, ac) in enumerate(beams):
        ent = finals.setdefault(P, [{}, i])
        ent[0][0 if last < 0 else 1] = ac
    best, ftots = None, {}
    for P, (src, rank) in finals.items():
        tot = ft(lse_fixed(src.get(0), src.get(1), ft=ft) + sc.final(states[P]))
        ftots[(hk[P], "final")] = float(tot)
        if best is None or tot > best[0] or (tot == best[0] and rank < best[1]):
            best = (tot, rank, P)
    margin = min(margin, _min_gap(sorted(ftots.values(), reverse=True), len(ftots) - 1 if ties else 1, ties))
    if trace is not None:
        trace.update(frames=frames + [ftots], max_kept=max_kept, tie_cutoffs=int(tie_cutoffs))
    ids, P = [], best[2]
    while P > 0:
        ids.append(lab[P])
        P = par[P]
    ids.reverse()
    return (ids, float(best[0]), margin) if return_margin else (ids, float(best[0]))


def fp32_noise(frames32, frames64):
    """Largest |total_f32 - total_f64| over the beams kept in both runs, frame by frame, while the two runs keep the same
    set -> (noise, the first frame whose kept sets differ or None)."""
    noise = 0.0
    for t, (a, b) in enumerate(zip(frames32, frames64)):
        if a.keys() != b.keys():
            return noise, t
        noise = max(noise, max(abs(a[k] - b[k]) for k in a))
    return noise, None


def analyse(logits, length, lm, cls, blank, **kw):
    """Both precisions of :func:`beam_decode` on one utterance -> dict(ids, score (float64 run), ids32, score32, margin
    (float64 run), noise, split (first frame at which the kept sets differ, or None), decisive, max_kept, tie_cutoffs, seconds (of the two runs))."""
    t32, t64 = {}, {}
    t0 = time.perf_counter()
    ids32, s32 = beam_decode(logits, length, lm, cls, blank, dtype=np.float32, trace=t32, **kw)
    t1 = time.perf_counter()
    ids, s64, margin = beam_decode(logits, length, lm, cls, blank, dtype=np.float64, trace=t64, return_margin=True, **kw)
    t2 = time.perf_counter()
    noise, split = fp32_noise(t32["frames"], t64["frames"])
    return dict(ids=ids, score=s64, ids32=ids32, score32=s32, margin=margin, noise=noise, split=split,
                decisive=bool(split is None and margin >= DECISIVE_FACTOR * noise), max_kept=t64["max_kept"],
                tie_cutoffs=t64["tie_cutoffs"], seconds=(t1 - t0, t2 - t1))


def objective(logits, length, ids, lm, cls, blank, alpha, beta, unk_score_offset=-10.0):
    """log P_ctc(ids | x) (oracle/ctc_ref.ctc_single, float64) + the contract's LM score of the label sequence."""
    from oracle.ctc_ref import ctc_single
    nll, _ = ctc_single(np.asarray(logits, dtype=np.float64)[:, :len(cls)], np.array(ids, dtype=np.int64), length, blank=blank)
    sc = Scorer(lm, cls, alpha, beta, unk_score_offset)
    return -nll + float(sc.final(sc.of_labels(ids)))


def exhaustive(logits, length, lm, cls, blank, alpha, beta, unk_score_offset=-10.0):
    """argmax over every label sequence of length <= length of objective()."""
    labels = [v for v in range(len(cls)) if v != blank]
    best = (-np.inf, None)
    for L in range(length + 1):
        for y in itertools.product(labels, repeat=L):
            o = objective(logits, length, list(y), lm, cls, blank, alpha, beta, unk_score_offset)
            if o > best[0]:
                best = (o, list(y))
    return best[1], best[0]


def greedy(logits, length, blank):
    a = np.argmax(np.asarray(logits)[:length], axis=1)
    out, prev = [], -1
    for v in a:
        if v != prev and v != blank:
            out.append(int(v))
        prev = v
    return out
