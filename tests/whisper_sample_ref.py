"""float64 NumPy restatement of one ``ssak_dec_sample_step`` (include/ssak_hip.h "Whisper sampling"): the counter-based uniform in
numpy integer arithmetic, the Gumbel variate, the scores ``x / T + g`` and the log-softmax in float64.  The processed row is not
restated here: with the timestamp rules it is ``row["mask"]`` of tests/whisper_timestamps_ref.py (``timestamp_step_row``: the final
candidate set, the mass decision included), without them the suppress masks of tests/whisper_generate_ref.py (``process``).
tests/test_whisper_sample_ref.py holds the draw to ``softmax(x / T)`` by chi-square; the GPU tests hold the kernel and
``generate(temperature=...)`` to it.

The accept set.  The kernel forms, in fp32 (u = 2^-24),

    score_c = fl(fl(x_c * fl(1 / T)) + g_c),   g_c = -logf(-logf(u_c)),

and a column's fp32 score differs from its float64 score by at most

    delta_c = u (4 |x_c / T| + 7 |g_c| + 6):

* the product: fl(1 / T) carries one rounding and the product one more, (2 u + u^2) |x_c / T| <= 3 u |x_c / T| (a contraction of the
  product into the add only removes a rounding);
* the two logarithms: u_c itself is exact.  logf is taken at 3 ulp = 6 u relative (OpenCL's bound for log, which the device library
  is built to; HIP states less).  The inner l = -logf(u_c) is off by 6 u relative, which moves log(l) by at most 6 u absolutely;
  the outer logf adds 6 u |g_c|: 6 u (1 + |g_c|);
* the add: one rounding of a sum of magnitude at most |x_c / T| + |g_c|: u (|x_c / T| + |g_c|), the second-order terms being covered
  by the slack of the two lines above.

A column other than the float64 arg-max can therefore be the kernel's arg-max only if its float64 score is within
delta_c + delta_argmax of the maximum: those columns are the accept set.  A column at -inf is never in it.
"""
import numpy as np

import whisper_generate_ref as GR
import whisper_timestamps_ref as TR

DS_SAMPLE = 0x5A0  # whisper_step.h
U = 2.0 ** -24
_M32 = np.uint64(0xFFFFFFFF)


def _mul32(a, c):
    return (a * np.uint64(c)) & _M32


def hash_u32(seed, stream, idx):
    """common.h ``hash_u32`` with ``seed`` AND ``idx`` arrays (uint64, broadcast against each other) -> uint64 arrays holding
    32-bit values.  (oracle.dropout_hash.hash_u32 takes one seed; the CPU tests hold the two to each other.)"""
    seed = np.asarray(seed, dtype=np.uint64)
    idx = np.asarray(idx, dtype=np.uint64)
    sh = np.uint64(32)
    key = (seed & _M32) ^ _mul32(seed >> sh, 0x9E3779B1) ^ np.uint64((int(stream) * 0x85EBCA77) & 0xFFFFFFFF) ^ _mul32(idx >> sh, 0xC2B2AE3D)
    h = (idx & _M32) ^ key
    h = h ^ (h >> np.uint64(16))
    h = _mul32(h, 0x7FEB352D)
    h = h ^ (h >> np.uint64(15))
    h = _mul32(h, 0x846CA68B)
    return h ^ (h >> np.uint64(16))


def noise_words(seed, t, rows, n_cols):
    """The 32-bit words of step ``t``: rows [R] (row indices) x columns 0 .. n_cols - 1 -> uint64 [R, n_cols].
    k = hash_u32(seed, DS_SAMPLE, (t << 32) | row);  w = hash_u32(seed ^ (k << 32), DS_SAMPLE + 1, c)."""
    seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    rows = np.asarray(rows, dtype=np.uint64)
    t = np.broadcast_to(np.asarray(t, dtype=np.uint64), rows.shape)
    k = hash_u32(seed, DS_SAMPLE, (t << np.uint64(32)) | rows)
    rowseed = seed ^ (k << np.uint64(32))
    return hash_u32(rowseed[:, None], DS_SAMPLE + 1, np.arange(n_cols, dtype=np.uint64)[None, :])


def uniforms(seed, t, rows, n_cols):
    """u = ((w >> 9) + 0.5) 2^-23: an odd multiple of 2^-24, strictly inside (0, 1), exact in fp32 (and in float64)."""
    return ((noise_words(seed, t, rows, n_cols) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(seed, t, rows, n_cols):
    """g = -log(-log(u)), float64 [R, n_cols]; the 23 bits keep it inside [-log(24 log 2), 24 log 2] = [-2.812, 16.636]."""
    return -np.log(-np.log(uniforms(seed, t, rows, n_cols)))


def draw(x, ok, g, temperature):
    """One row: logits x [V], candidate set ok [V] bool, Gumbel variates g [V] -> dict(token, logprob, gap, accept).  ``gap``: the
    top-two distance of the float64 scores (inf with one finite candidate); ``accept``: the columns the kernel's fp32 arithmetic
    may return (module docstring).  No candidate with a finite logit: token None, log-prob 0."""
    x = np.asarray(x, dtype=np.float64)
    cand = ok & (x > -np.inf)
    if not cand.any():
        return dict(token=None, logprob=0.0, gap=np.inf, accept=np.zeros(0, dtype=np.int64))
    a = x / temperature
    score = np.where(cand, a + g, -np.inf)
    tok = int(score.argmax())  # (the lowest index of the maximum)
    delta = U * (4 * np.abs(np.where(cand, a, 0.0)) + 7 * np.abs(g) + 6)
    accept = np.flatnonzero(cand & (score[tok] - score <= delta + delta[tok]))
    top = np.sort(score[cand])
    gap = float(top[-1] - top[-2]) if top.size > 1 else np.inf
    xs = x[cand]
    m = xs.max()
    return dict(token=tok, logprob=float(x[tok] - (m + np.log(np.exp(xs - m).sum()))), gap=gap, accept=accept)


def sample_step(logits, finished, eos, pad, temperature, seed, t, histories=None, ts_begin=None, no_timestamps=None, max_initial=None,
                suppress=None, begin_suppress=None, first=None, row0=0):
    """One ``ssak_dec_sample_step`` over a batch: logits [R, V] (row r is the kernel's row ``row0 + r``), finished [R] bool.
    ``histories`` (one token list per row, each of length t): the timestamp rules of tests/whisper_timestamps_ref.py hold and fix the
    candidate set; None: no rules, the suppress masks alone (``first``, by default t == 0, applies ``begin_suppress``).
    -> (tokens [R], logprobs [R], finished after, rows): per unfinished row the dict of :func:`draw` plus ``mask`` (the candidate
    set) and, with rules, ``ts_last`` after the step; None for a finished row, which emits ``pad`` with log-probability 0, as does a
    row without a candidate."""
    logits = np.asarray(logits, dtype=np.float64)
    R, V = logits.shape
    first = t == 0 if first is None else first
    g = gumbel(seed, t, row0 + np.arange(R), V)
    toks, lps, rows = [], [], []
    for r in range(R):
        if finished[r]:
            toks.append(pad), lps.append(0.0), rows.append(None)
            continue
        if histories is None:
            ok = GR.process(np.zeros((1, V)), suppress, begin_suppress, first)[0] == 0.0  # (the columns no mask hits, whatever they hold)
        else:
            ok = TR.timestamp_step_row(logits[r], list(histories[r]), ts_begin, no_timestamps, eos, max_initial, suppress, begin_suppress)["mask"]
        d = draw(logits[r], ok, g[r], temperature)
        d["mask"] = ok
        if histories is not None:
            prev = TR.last_timestamp(histories[r], ts_begin)
            d["ts_last"] = d["token"] if d["token"] is not None and d["token"] >= ts_begin else prev
        toks.append(pad if d["token"] is None else d["token"]), lps.append(d["logprob"]), rows.append(d)
    toks = np.array(toks)
    return toks, np.array(lps), np.asarray(finished, dtype=bool) | (toks == eos), rows


def generate(p, nh, n_layers, enc, prompt, max_new_tokens, eos, pad, temperature, seed, n=1, timestamps=None, suppress=None,
             begin_suppress=None, enc_lens=None):
    """``generate(temperature=T, best_of=n)`` on tests/whisper_decoder_ref.py, the whole prefix recomputed at every step: prompt [B, P]
    -> dict(tokens [B * n, steps], logprobs, lens [B * n], gaps [B * n, steps]) for the B * n rows in the kernel's row order (audio
    b's candidates are rows b n .. b n + n - 1); ``seed`` is the kernel's (``sample_call_seed`` of the call's).  ``timestamps``: None
    or dict(ts_begin, no_timestamps, max_initial).  gaps are inf for finished rows."""
    import whisper_decoder_ref as WR
    prompt = np.repeat(np.asarray(prompt), n, axis=0)
    enc = np.repeat(np.asarray(enc), n, axis=0)
    enc_lens = None if enc_lens is None else np.repeat(np.asarray(enc_lens), n)
    R = prompt.shape[0]
    seq = prompt.copy()
    finished = np.zeros(R, dtype=bool)
    hist = [[] for _ in range(R)]
    toks, lps, gaps = [], [], []
    for i in range(max_new_tokens):
        logits = WR.decoder_logits(p, nh, n_layers, enc, seq, enc_lens)[:, -1]
        tok, lp, finished, rows = sample_step(logits, finished, eos, pad, temperature, seed, i, hist if timestamps else None,
                                              suppress=suppress, begin_suppress=begin_suppress, **(timestamps or {}))
        for r in range(R):
            hist[r].append(int(tok[r]))
        toks.append(tok), lps.append(lp)
        gaps.append([np.inf if d is None else d["gap"] for d in rows])
        seq = np.concatenate([seq, tok[:, None]], 1)
        if finished.all():
            break
    toks, lps = np.stack(toks, 1), np.stack(lps, 1)
    lens = np.array([int(np.argmax(r == eos)) + 1 if (r == eos).any() else toks.shape[1] for r in toks])
    return dict(tokens=toks, logprobs=lps, lens=lens, gaps=np.array(gaps).T)


# ---- the inputs the CPU and the GPU tests share --------------------------------------------------------------------------------------
CHI2_7_999 = 24.322  # the 99.9 % point of chi-square with 7 degrees of freedom
CHI_N = 65536
CHI_SEED = 20240611  # chosen once, run in tests/test_whisper_sample_ref.py, kept
CHI_P = np.array([0.5, 0.25, 0.12, 0.06, 0.035, 0.02, 0.01, 0.005])


def chi_logits():
    """The 8-column row of the distribution tests, fp32: log of probabilities from 0.5 down to 0.005."""
    return np.log(CHI_P).astype(np.float32)


def chi_square(tokens, x, temperature):
    """Pearson's chi-square of the token counts against softmax(x / T) -> (statistic, counts)."""
    a = np.asarray(x, dtype=np.float64) / temperature
    p = np.exp(a - a.max())
    p /= p.sum()
    counts = np.bincount(np.asarray(tokens), minlength=len(p)).astype(np.float64)
    e = p * counts.sum()
    return float(((counts - e) ** 2 / e).sum()), counts


def draw_rows(x, temperature, seed, t, rows):
    """The draws of one fp32 logits row ``x`` [V] repeated over ``rows`` (row indices; ``t`` a scalar or one step per row), every
    column a candidate, vectorised -> (tokens [R], single [R] bool: the accept set holds one column)."""
    a = np.asarray(x, dtype=np.float64)[None, :] / temperature
    g = gumbel(seed, t, rows, a.shape[1])
    score = a + g
    tok = score.argmax(-1)
    delta = U * (4 * np.abs(a) + 7 * np.abs(g) + 6)
    best = np.take_along_axis(score, tok[:, None], 1)
    n_acc = (best - score <= delta + np.take_along_axis(delta, tok[:, None], 1)).sum(-1)
    return tok, n_acc == 1


RANDOM_ROWS, RANDOM_V, RANDOM_SEED, RANDOM_T = 65, 127, 52, 0.8


def random_rows(ldv=RANDOM_V):
    """The random-rows case: 65 rows x V = 127 of 2 N(0, 1) logits in an [R, ldv] fp32 buffer (+1e30 in the columns past V)."""
    x = np.full((RANDOM_ROWS, ldv), 1e30, dtype=np.float32)
    x[:, :RANDOM_V] = (2.0 * np.random.default_rng(RANDOM_SEED).standard_normal((RANDOM_ROWS, RANDOM_V))).astype(np.float32)
    return x


# generate(temperature = GEN_T, best_of = GEN_N, seed = GEN_SEED) on tests/golden/whisper_dec_tiny.npz: GEN_SEED is chosen so that the
# float64 decoder restatement alone leaves at most an eighth of its steps with a top-two score gap below GEN_BAR (asserted in
# tests/test_whisper_sample_ref.py); 7.76e-2 is the logits bar of DESIGN.md "Whisper decoder", carried through the division by T
GEN_T, GEN_N, GEN_SEED, GEN_NEW = 0.7, 3, 82, 8
GEN_BAR = 2 * 7.76e-2 / GEN_T
GEN_LANGS = ["en", "fr", "de"]


def gen_case(golden, timestamps):
    """What the generate tests share -> (prompt [3, P], suppress list, the rules as :func:`generate` takes them or None)."""
    import gen_golden_whisper_dec as G
    nots = G.NO_TIMESTAMPS
    prompt = np.array([[G.SOT, G.LANG0 + G.LANGS.index(c), G.TRANSCRIBE] + ([] if timestamps else [nots]) for c in GEN_LANGS])
    rules = dict(ts_begin=nots + 1, no_timestamps=nots, max_initial=5) if timestamps else None
    return prompt, list(range(G.SOT, nots + 1)), rules
