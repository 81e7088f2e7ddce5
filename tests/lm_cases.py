"""The LM beam search cases shared by tests/test_lm_host.py (CPU: the restatement in float32 against float64) and
tests/test_gpu_lm_decode.py (the device against the float64 restatement).  A case is a dict; :func:`build` turns it into
a tokenizer, an ARPA file under ``tmp_path``, its host tables and the logits, all from the case's seed.

A case is DECISIVE when its float64 decision margin (lm_beam_ref.beam_decode) is at least 32 x its fp32 noise: then the
device must return the float64 transcript exactly.  The others fall back to the equivalence check (score within 1e-3,
a different transcript as good under the exact objective).  Margin and noise as the CPU test reproduces them (the worst
utterance of the case; ``ties``: exact ties by construction, decided by the enumeration index, are not counted):

    case            labels  V     W    F     order  margin    noise     margin/noise  decisive
    strip5          5       5     8    12    3      4.16e-03  8.67e-07  4799          yes
    strip64         64      64    8    12    3      7.22e-04  2.29e-06  315           yes
    strip65         65      65    8    12    3      3.22e-03  2.07e-06  1556          yes
    strip256        256     256   8    10    3      4.28e-03  1.92e-06  2227          yes
    strip257        257     257   8    10    3      2.40e-03  1.86e-06  1287          yes
    strip300        300     300   8    10    3      2.58e-03  1.81e-06  1427          yes
    strip1024       1024    1024  8    8     3      1.43e-02  2.95e-06  4869          yes
    strip1024_all   1024    1024  8    8     3      1.43e-02  2.95e-06  4869          yes
    extra33         33      40    8    12    3      3.38e-02  2.98e-06  11363         yes
    extra1024       1024    1032  8    8     3      2.76e-04  1.91e-06  145           yes
    keys4096        16      16    256  6     3      3.82e-04  3.10e-06  123           yes
    keys4097        17      17    241  6     3      2.76e-03  3.51e-06  788           yes
    keys9600        300     300   32   6     3      5.38e-02  3.79e-06  14188         yes
    width2          32      32    2    30    3      1.67e-03  1.99e-06  842           yes
    width63         32      32    63   30    3      1.67e-03  4.44e-06  377           yes
    width64         32      32    64   30    3      1.67e-03  5.04e-06  332           yes
    width65         32      32    65   30    3      1.00e-03  5.04e-06  198           yes
    width255        32      32    255  30    3      9.30e-04  8.16e-06  114           yes
    width256        32      32    256  30    3      6.37e-04  6.21e-06  103           yes
    tie3            12      12    3    4     3      5.35e-02  7.86e-07  68117         yes  (ties)
    tie5            12      12    5    4     3      1.54e-02  7.45e-07  20729         yes  (ties)
    tie3_empty      12      12    3    4     3      1.62e-01  1.74e-07  936206        yes  (ties)
    tie5_empty      12      12    5    4     3      5.35e-02  7.86e-07  68117         yes  (ties)
    order1          32      32    16   126   1      9.44e-01  3.81e-06  247762        yes
    order2          32      32    16   126   2      8.78e-02  6.38e-06  13763         yes
    order3          32      32    16   126   3      6.96e-02  5.73e-06  12146         yes
    order6          32      32    16   126   6      3.95e-01  4.13e-06  95527         yes
    order2t         32      32    16   126   2      3.94e-01  4.23e-06  93211         yes
    long            32      32    16   1500  3      3.32e-02  9.85e-05  337           yes
    masked          32      32    8    20    3      1.22e-03  2.54e-06  480           yes
"""
import os
import types

import numpy as np

from ssak_amd import synth
from ssak_amd.data import CharTokenizer
from ssak_amd.lm import NgramLM, label_classes

import lm_beam_ref as R

INF = float("inf")
TOK = CharTokenizer(synth.VOCAB)


def _case(name, kind, seed, n_labels, W, F, V=None, order=3, token_min_logp=-5.0, beam_prune_logp=-10.0, decisive=True, **kw):
    return dict(name=name, kind=kind, seed=seed, n_labels=n_labels, V=V or n_labels, W=W, F=F, order=order,
                token_min_logp=token_min_logp, beam_prune_logp=beam_prune_logp, decisive=decisive, **kw)


WIDE = dict(token_min_logp=-8.5, beam_prune_logp=-40.0)
CASES = [
    # strip-mined labels: S_t compaction, log-softmax and argmax over 1..4 strips of 256 labels
    _case("strip5", "random", 0, 5, 8, 12),
    _case("strip64", "random", 0, 64, 8, 12),
    _case("strip65", "random", 0, 65, 8, 12),
    _case("strip256", "random", 0, 256, 8, 10),
    _case("strip257", "random", 0, 257, 8, 10),
    _case("strip300", "random", 0, 300, 8, 10),
    _case("strip1024", "random", 0, 1024, 8, 8),
    _case("strip1024_all", "random", 0, 1024, 8, 8, token_min_logp=-INF),
    # n_labels < V: the surplus columns hold +50
    _case("extra33", "random", 1, 33, 8, 12, V=40),
    _case("extra1024", "random", 0, 1024, 8, 8, V=1032),
    # candidate keys in LDS (W * n_labels <= 4096) or in the workspace; no pruning, so every beam x label is a candidate
    _case("keys4096", "random", 0, 16, 256, 6, token_min_logp=-INF, beam_prune_logp=-INF),
    _case("keys4097", "random", 0, 17, 241, 6, token_min_logp=-INF, beam_prune_logp=-INF),
    _case("keys9600", "random", 0, 300, 32, 6, token_min_logp=-INF, beam_prune_logp=-INF),
    # beam widths at the wave edges, on peaked posteriors with a confusable second label in most frames; under the default
    # pruning these keep two beams, so the token floor lets a few more labels in and the prune floor is far: the beam fills
    _case("width2", "width", 5, 32, 2, 30, **WIDE),
    _case("width63", "width", 5, 32, 63, 30, **WIDE),
    _case("width64", "width", 5, 32, 64, 30, **WIDE),
    _case("width65", "width", 5, 32, 65, 30, **WIDE),
    _case("width255", "width", 5, 32, 255, 30, **WIDE),
    _case("width256", "width", 14, 32, 256, 30, **WIDE),
    # exact ties across the cutoff, by construction; seeds at which the opposite tie rule gives another transcript
    _case("tie3", "tie", 1, 12, 3, 4),
    _case("tie5", "tie", 0, 12, 5, 4),
    _case("tie3_empty", "tie_empty", 0, 12, 3, 4),
    _case("tie5_empty", "tie_empty", 1, 12, 5, 4),
    # LM orders; one set of acoustics (F is whatever the sentence takes); order2t = the order-6 file cut to its bigrams
    _case("order1", "order", 0, 32, 16, None, order=1),
    _case("order2", "order", 0, 32, 16, None, order=2),
    _case("order3", "order", 0, 32, 16, None, order=3),
    _case("order6", "order", 0, 32, 16, None, order=6),
    _case("order2t", "order", 0, 32, 16, None, order=2, truncated=True),
    # node store, prefix hash and read-back over a long utterance (two of them, the second shorter than F)
    _case("long", "long", 0, 32, 16, 1500, lens=(1500, 1371)),
    # -inf logits: a third of the non-blank columns in every frame, every column but the blank in one frame
    _case("masked", "masked", 0, 32, 8, 20),
]
BY_NAME = {c["name"]: c for c in CASES}


def vocabulary(n):
    """n labels: the project's 32, those plus one, or <pad>, | and n - 2 characters (a-z, then consecutive CJK code points)."""
    if n == 32:
        return list(synth.VOCAB)
    if n == 33:
        return list(synth.VOCAB) + [chr(0x4E00)]
    chars = [chr(ord("a") + i) for i in range(26)] + [chr(0x4E00 + i) for i in range(n)]
    return ["<pad>", "|"] + chars[:n - 2]


def random_words(rng, chars, n):
    """Up to ``n`` distinct words of 1-3 random characters."""
    out = []
    for _ in range(4 * n):
        w = "".join(chars[int(k)] for k in rng.integers(0, len(chars), int(rng.integers(1, 4))))
        if w not in out:
            out.append(w)
        if len(out) == n:
            break
    return out


def peaked(rng, text, conf=0.3, F=None, tok=TOK, frames=None):
    """Posteriors of a label sequence: each label held 1-2 frames then blank, a confusable second label in some frames.
    ``frames``: a list that receives the first frame of every label."""
    labs = tok.encode(text)
    rows = []
    for l in labs:
        if frames is not None:
            frames.append(len(rows))
        for _ in range(int(rng.integers(1, 3))):
            r = rng.standard_normal(len(tok)).astype(np.float32) * 0.5
            r[l] += 9.0
            if rng.random() < conf:
                r[int(rng.integers(5, 31))] += 7.5
            rows.append(r)
        r = rng.standard_normal(len(tok)).astype(np.float32) * 0.5
        r[tok.pad_token_id] += 8.0
        rows.append(r)
    x = np.stack(rows)
    if F is not None:
        x = np.concatenate([x, np.zeros((F - len(x), len(tok)), np.float32)])
    return x


def truncate_arpa(src, dst, order):
    """The ARPA file ``src`` cut to its first ``order`` sections (same low-order probabilities and backoffs)."""
    lines = open(src, encoding="utf-8").read().split("\n")
    out, keep = [], True
    for ln in lines:
        if ln.startswith("ngram "):
            keep = int(ln[6:].split("=")[0]) <= order
        elif ln.startswith("\\") and ln.endswith("-grams:"):
            keep = int(ln[1:].split("-")[0]) <= order
        elif ln == "\\end\\":
            keep = True
        if keep:
            out.append(ln)
    with open(dst, "w", encoding="utf-8") as f:
        f.write("\n".join(out))


def _order_words(rng):
    """24 pairs of words that differ in one letter, so that one ambiguous frame decides between two LM words."""
    words = []
    for w in synth.synth_words(rng, 24, 3, 5):
        k = int(rng.integers(len(w)))
        c = chr(ord("a") + (ord(w[k]) - ord("a") + 1 + int(rng.integers(25))) % 26)
        sib = w[:k] + c + w[k + 1:]
        if w not in words and sib not in words:
            words += [w, sib]
    return words


def _order_acoustics(rng, words, tmp_path, seed):
    """A sentence c1 .. c5 A w7 w8 w9 <OOV word> along a stored 6-gram (c1 .. c5, A) of the order-6 file; the frames of the
    one letter in which A differs from its pair B slightly prefer B.  Chosen so that the order-6 LM scores A far above B in
    that context and the bigrams of the same file score B above A: the long context decides."""
    p6, p2 = os.path.join(tmp_path, "design6.arpa"), os.path.join(tmp_path, "design2.arpa")
    synth.write_arpa(p6, words, [150] * 5, seed=seed)
    truncate_arpa(p6, p2, 2)
    lm6, lm2 = NgramLM(p6, TOK), NgramLM(p2, TOK)
    pair = {w: words[i ^ 1] for i, w in enumerate(words)}
    best = None
    keys = lm6.ng_keys[4]
    for g in keys[keys[:, 0] >= 0]:
        names = [lm6.words[i] for i in g]
        if any(n not in pair for n in names):
            continue
        a, b = lm6.word_id[names[5]], lm6.word_id[pair[names[5]]]
        d6 = float(lm6.log10p(list(g[:5]), a)) - float(lm6.log10p(list(g[:5]), b))
        d2 = float(lm2.log10p([int(g[4])], b)) - float(lm2.log10p([int(g[4])], a))
        if best is None or min(d6, d2 + 0.7) > best[0]:
            best = (min(d6, d2 + 0.7), names)
    assert best is not None and best[0] >= 1.2, "no 6-gram of this seed separates the orders"
    names = best[1]
    A, B = names[5], pair[names[5]]
    rest = [w for w in words if w not in names and w != B]
    tail = [rest[int(k)] for k in rng.choice(len(rest), 3, replace=False)]
    text = " ".join(names + tail + ["zzqx"])
    frames = []
    x = peaked(rng, text, conf=0.3, frames=frames)
    k = next(i for i in range(len(A)) if A[i] != B[i])
    pos = len(" ".join(names[:5])) + 1 + k
    end = frames[pos + 1] - 1  # the blank frame after the label
    for t in range(frames[pos], end):
        x[t] = rng.standard_normal(len(TOK)).astype(np.float32) * 0.5
        x[t, TOK.index[A[k]]] += 8.0
        x[t, TOK.index[B[k]]] += 8.2
    return x, A, B


def build(case, tmp_path):
    """-> namespace(case, tok, cls, blank, arpa, lm (host tables), x [B, F, V] float32, lens, kw (the decode arguments),
    ties)."""
    tmp_path = str(tmp_path)
    rng = np.random.default_rng(case["seed"])
    kind, NL, V, F = case["kind"], case["n_labels"], case["V"], case["F"]
    vocab = vocabulary(NL)
    if kind == "tie":  # words over i, j only: a .. h begin no LM word
        vocab = ["<pad>", "|"] + list("abcdefghij")
    elif kind == "tie_empty":  # the same with two labels without text
        vocab = ["<pad>", "<s>", "</s>", "|"] + list("abcdefgh")
    tok = CharTokenizer(vocab)
    cls = label_classes(tok)
    blank = tok.pad_token_id
    chars = [t for i, t in enumerate(vocab) if cls[i] == 0]
    arpa = os.path.join(tmp_path, case["name"] + ".arpa")
    lens = None
    if kind == "order":
        words = _order_words(rng)
        x, A, B = _order_acoustics(rng, words, tmp_path, case["seed"])
        if case.get("truncated"):
            truncate_arpa(os.path.join(tmp_path, "design6.arpa"), arpa, case["order"])
        else:
            synth.write_arpa(arpa, words, [150] * (case["order"] - 1), seed=case["seed"])
        x = x[None]
    else:
        if kind in ("tie", "tie_empty"):
            words = random_words(rng, chars[-2:], 10)
        elif NL == 32:
            words = synth.synth_words(rng, 60, 2, 5)
        else:
            words = random_words(rng, chars, 200)
        n = 4 * len(words)
        synth.write_arpa(arpa, words, [n] * (case["order"] - 1), seed=case["seed"])
    if kind == "random":
        x = (rng.standard_normal((1, F, V)) * 3.5).astype(np.float32)
        x[:, :, NL:] = 50.0
    elif kind == "masked":
        x = (rng.standard_normal((1, F, V)) * 3.5).astype(np.float32)
        others = np.array([v for v in range(NL) if v != blank])
        for t in range(F):
            x[0, t, rng.choice(others, len(others) // 3, replace=False)] = -np.inf
        x[0, F // 2, others] = -np.inf
    elif kind in ("tie", "tie_empty"):
        x = np.empty((1, F, V), np.float32)
        for t in range(F):
            x[0, t, :] = np.float32(rng.standard_normal())
            x[0, t, blank] = np.float32(rng.standard_normal() + 1.0)
    elif kind == "width":
        text = " ".join(words[int(k)] for k in rng.integers(0, len(words), 6))
        x = peaked(rng, text, conf=0.6)[None, :F]
        assert x.shape[1] == F
    elif kind == "long":
        lens = list(case["lens"])
        xs = []
        for L in lens:
            text = " ".join(words[int(k)] for k in rng.integers(0, len(words), 160))
            a = peaked(rng, text, conf=0.3)[:L]
            assert len(a) == L
            xs.append(np.concatenate([a, rng.standard_normal((F - L, V)).astype(np.float32)]))
        x = np.stack(xs)
    x = np.ascontiguousarray(x, dtype=np.float32)
    kw = dict(alpha=0.5, beta=1.0, beam_width=case["W"], beam_prune_logp=case["beam_prune_logp"],
              token_min_logp=case["token_min_logp"])
    return types.SimpleNamespace(case=case, tok=tok, cls=cls, blank=blank, arpa=arpa, lm=NgramLM(arpa, tok), x=x,
                                 lens=lens or [x.shape[1]] * len(x), kw=kw, ties=kind in ("tie", "tie_empty"))


def analyse(built, b=0):
    """lm_beam_ref.analyse of utterance ``b`` of a built case."""
    return R.analyse(built.x[b], built.lens[b], built.lm, built.cls, built.blank, ties=built.ties, **built.kw)


def table_row(name):
    """(margin, noise, decisive) of a case as the table at the top of this module records them."""
    for ln in __doc__.splitlines():
        f = ln.split()
        if f and f[0] == name:
            return float(f[6]), float(f[7]), f[9] == "yes"
    raise KeyError(name)


def worst(runs):
    """The utterance of a case with the smallest margin / noise."""
    return min(runs, key=lambda a: a["margin"] / max(a["noise"], 1e-30))
