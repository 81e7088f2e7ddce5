"""ARPA n-gram language model for CTC beam search on the device (``--arpa`` of ssak/infer/transformers_infer.py:97-133).

The reference decodes with pyctcdecode + KenLM (``build_ctcdecoder(labels, arpa, alpha=0.5, beta=1.0)``,
transformers_infer.py:272-295).  Neither is available to this project, so the search below is a contract of its own,
MODELLED ON pyctcdecode's defaults as the reference calls them; equality with pyctcdecode is not claimed
(pyctcdecode parity unpinned).  For one utterance of ``len`` frames:

* Input: ``lp[t, v] = max(log_softmax(logits[t])[v], ln 1e-15)`` over the first ``len(tokenizer)`` columns.
* Label classes (:func:`label_classes`): the pad token is the CTC blank, ``|`` the word delimiter, other ``<...>`` tokens
  are ordinary CTC labels with empty text (they break repeats and add nothing to a word, as ``CharTokenizer.decode``),
  everything else is a character.
* A beam is ``(prefix, last)``: the collapsed label sequence and blank or the final label of the prefix.  The search
  starts from the empty prefix, ``last`` = blank, acoustic score 0, LM context ``<s>``.
* Per frame the token set is ``S_t = {v : lp[t,v] >= token_min_logp} | {argmax_v lp[t,v]}``; every beam is extended by
  every ``v`` in ``S_t``: blank gives ``(prefix, blank)``, ``v == last`` gives ``(prefix, v)``, any other ``v`` gives
  ``(prefix+v, v)``.  Candidates with the same ``(prefix, last)`` are merged by logsumexp of their acoustic scores in the
  fixed source order (repeat, extension from the blank-ending parent, extension from the label-ending parent; for a
  blank-ending target: from the blank-ending beam, from the label-ending beam).  Candidates are ranked by
  ``total = acoustic + lm + partial``; ties go to the smaller enumeration index (parent beam rank, then token id; a merged
  candidate takes the smallest of its sources).  The top ``beam_width`` are kept, then every candidate with
  ``total < best + beam_prune_logp`` is dropped.
* LM terms, with ``L(w | h) = ln(10) * log10 P_arpa(w | h)`` under standard ARPA backoff: emitting ``|`` after a
  non-empty partial word ``w`` adds ``alpha * (L(w'|h) + ln(10) * unk_score_offset * [w OOV]) + beta`` (``w'`` is ``w``
  or ``<unk>``, ``h`` the last ``order-1`` words); a non-empty partial word that is not a prefix of any LM unigram
  carries ``partial = alpha * ln(10) * unk_score_offset``, otherwise ``partial = 0``.
* End of utterance: each beam's partial word is completed as a word, ``alpha * L(</s> | h)`` is added, beams with the
  same prefix are merged by logsumexp of their acoustic scores ([blank-ending, label-ending]), and the best total wins
  (ties: the smaller beam rank).
* Output: the winner's label ids (``[B, F]`` ids / ``[B]`` counts, as ``ssak_ctc_greedy_decode`` writes them) and its
  total; the text is ``tok.decode(ids[:n], group_tokens=False)``.
* Defaults (pyctcdecode's, to our reading): ``beam_width=100``, ``beam_prune_logp=-10``, ``token_min_logp=-5``,
  ``unk_score_offset=-10``; ``alpha=0.5``, ``beta=1.0`` as the reference.  Limits: ``beam_width <= 256``, ``V <= 1024``.

Device tables (``include/ssak_hip.h``, ``ssak_ngram_lm``): a unigram trie over LABEL ids as an open-addressing hash
``(node, label) -> child`` (root = node 0, ``node_word[node]`` = word id or -1), unigram (log10 p, log10 backoff) by word
id, and one open-addressing hash per order >= 2 keyed by the full word-id tuple (exact keys, no fingerprints).  All
tables use linear probing from ``lm_hash(ids)`` below; every probe loop on the device is bounded by the table size.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_ORDER = 6
MAX_BEAM = 256
MAX_LABELS = 1024
LN10 = np.float32(math.log(10.0))
CLASS_CHAR, CLASS_DELIM, CLASS_EMPTY = 0, 1, 2
UNK_LOG10P = np.float32(-100.0)  # <unk> absent from the ARPA file: KenLM's convention


# ------------------------------------------------------------------------------------------------- ARPA text
def read_arpa(path: str):
    """-> (order, counts[order], [per order: (list of word tuples, log10 prob float32[n], log10 backoff float32[n])]).
    Plain-text ARPA only: ``\\data\\``, ``ngram N=count`` lines, the ``\\N-grams:`` sections (N <= 6) and ``\\end\\``."""
    with open(path, "rb") as f:
        raw = f.read()
    if b"\0" in raw[:4096] or raw.startswith(b"mmap lm"):
        raise ValueError(f"{path}: not an ARPA text file (KenLM binary LMs are not supported)")
    try:
        text = raw.decode("utf-8")
    except UnicodeDecodeError as e:
        raise ValueError(f"{path}: not an ARPA text file ({e})") from None
    lines = text.splitlines()
    i, n = 0, len(lines)

    def skip_blank():
        nonlocal i
        while i < n and not lines[i].strip():
            i += 1

    skip_blank()
    if i >= n or lines[i].strip() != "\\data\\":
        raise ValueError(f"{path}: not an ARPA file (expected '\\data\\' first, got {lines[i][:40]!r})" if i < n
                         else f"{path}: empty file, not an ARPA file")
    i += 1
    counts: Dict[int, int] = {}
    while i < n and lines[i].strip().startswith("ngram "):
        k, _, c = lines[i].strip()[6:].partition("=")
        try:
            counts[int(k)] = int(c)
        except ValueError:
            raise ValueError(f"{path}:{i + 1}: bad count line {lines[i]!r}") from None
        i += 1
    order = len(counts)
    if order == 0 or sorted(counts) != list(range(1, order + 1)):
        raise ValueError(f"{path}: bad \\data\\ section (orders {sorted(counts)})")
    if order > MAX_ORDER:
        raise ValueError(f"{path}: order {order} > {MAX_ORDER} is not supported")
    sections = []
    for k in range(1, order + 1):
        skip_blank()
        if i >= n or lines[i].strip() != f"\\{k}-grams:":
            raise ValueError(f"{path}:{i + 1}: expected '\\{k}-grams:'")
        i += 1
        body = lines[i:i + counts[k]]
        i += counts[k]
        words, prob, bo = [], np.zeros(len(body), np.float32), np.zeros(len(body), np.float32)
        for j, line in enumerate(body):
            parts = line.split()
            if len(parts) not in (k + 1, k + 2):
                raise ValueError(f"{path}: {k}-gram line {j + 1}: {line!r}")
            try:
                prob[j] = float(parts[0])
                if len(parts) == k + 2:
                    bo[j] = float(parts[-1])
            except ValueError:
                raise ValueError(f"{path}: {k}-gram line {j + 1}: {line!r}") from None
            words.append(tuple(parts[1:k + 1]))
        sections.append((words, prob, bo))
    skip_blank()
    if i >= n or lines[i].strip() != "\\end\\":
        raise ValueError(f"{path}: expected '\\end\\' after the {order}-grams (section counts disagree with \\data\\?)")
    return order, [counts[k] for k in range(1, order + 1)], sections


# ------------------------------------------------------------------------------------------------- hashing
def lm_hash(cols: Sequence[np.ndarray]) -> np.ndarray:
    """FNV-1a over int32 ids then a 32-bit finaliser; the device computes the same (lm_decode.hip: lm_hash)."""
    h = np.full(len(cols[0]), 2166136261, dtype=np.uint32)
    for c in cols:
        h = (h ^ np.asarray(c).astype(np.int64).astype(np.uint32)) * np.uint32(16777619)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x2C1B3C6D)
    h ^= h >> np.uint32(12)
    return h


def _capacity(n: int, max_load: float) -> int:
    cap = 1
    while cap <= n or cap * max_load < n:
        cap *= 2
    return cap


def _place(h: np.ndarray, cap: int) -> np.ndarray:
    """Linear-probing positions of keys with hashes ``h`` in a table of ``cap`` slots (insertion in rounds: at each round
    the lowest-indexed key claiming a free slot takes it, the others move one slot on).  Every slot between a key's home
    and its position is occupied, which is all that a probing lookup needs."""
    n = len(h)
    pos = np.full(n, -1, dtype=np.int64)
    slot = (h & np.uint32(cap - 1)).astype(np.int64)
    taken = np.zeros(cap, dtype=bool)
    pending = np.arange(n)
    while pending.size:
        s = slot[pending]
        free = ~taken[s]
        u, first = np.unique(s[free], return_index=True)
        win = pending[free][first]
        pos[win] = u
        taken[u] = True
        lost = np.setdiff1d(pending, win, assume_unique=True)
        slot[lost] = (slot[lost] + 1) & (cap - 1)
        pending = lost
    return pos


def label_classes(tok) -> np.ndarray:
    """uint8[len(tok)]: 0 character, 1 word delimiter, 2 label without text (pad / blank and the other ``<...>`` tokens)."""
    cls = np.zeros(len(tok), dtype=np.uint8)
    for i, t in enumerate(tok.vocab):
        if t == tok.delim:
            cls[i] = CLASS_DELIM
        elif i == tok.pad_token_id or t in tok.special:
            cls[i] = CLASS_EMPTY
    return cls


# ------------------------------------------------------------------------------------------------- the LM
class NgramLM:
    """Host tables of an ARPA LM mapped onto a tokenizer's labels (+ their device copies once :meth:`to` ran).

    ``skipped[k-1]``: k-grams dropped because a word cannot be spelled with the tokenizer's character labels."""

    def __init__(self, arpa_path: str, tok, max_load: float = 0.5):
        order, counts, sections = read_arpa(arpa_path)
        self.order, self.counts = order, counts
        cls = label_classes(tok)
        char_id = {t: i for i, t in enumerate(tok.vocab) if cls[i] == CLASS_CHAR and i != tok.pad_token_id}
        # words: the unigrams; <s>, </s>, <unk> are words without spelling
        uw, uprob, ubo = sections[0]
        spell: Dict[str, Optional[List[int]]] = {}
        words: List[str] = []
        keep = []
        for j, (w,) in enumerate(uw):
            if w in ("<s>", "</s>", "<unk>"):
                labs = []
            else:
                labs = [char_id.get(c) for c in w]
                if not labs or any(l is None for l in labs):
                    continue
            spell[w] = labs
            words.append(w)
            keep.append(j)
        self.words = words
        self.word_id = {w: i for i, w in enumerate(words)}
        for need in ("<s>", "</s>"):
            if need not in self.word_id:
                raise ValueError(f"{arpa_path}: the unigrams lack {need}")
        uni = np.stack([uprob[keep], ubo[keep]], axis=1).astype(np.float32)
        if "<unk>" not in self.word_id:
            self.word_id["<unk>"] = len(words)
            words.append("<unk>")
            uni = np.concatenate([uni, np.array([[UNK_LOG10P, 0.0]], np.float32)])
        self.uni = np.ascontiguousarray(uni)
        self.bos, self.eos, self.unk = self.word_id["<s>"], self.word_id["</s>"], self.word_id["<unk>"]
        self.skipped = [len(uw) - len(keep)]
        # trie over label ids
        parent, label, child = [], [], []
        kids: Dict[Tuple[int, int], int] = {}
        node_word = [-1]
        for w in words:
            labs = spell.get(w) or []
            node = 0
            for l in labs:
                nxt = kids.get((node, l))
                if nxt is None:
                    nxt = len(node_word)
                    kids[(node, l)] = nxt
                    node_word.append(-1)
                    parent.append(node)
                    label.append(l)
                    child.append(nxt)
                node = nxt
            if labs:
                node_word[node] = self.word_id[w]
        self.node_word = np.array(node_word, dtype=np.int32)
        parent, label, child = (np.array(a, dtype=np.int32) for a in (parent, label, child))
        cap = _capacity(len(parent), max_load)
        self.trie = np.full((cap, 3), -1, dtype=np.int32)
        if len(parent):
            pos = _place(lm_hash([parent, label]), cap)
            self.trie[pos] = np.stack([parent, label, child], axis=1)
        # one hash per order >= 2
        self.ng_keys, self.ng_val = [], []
        for k in range(2, order + 1):
            kw, kp, kb = sections[k - 1]
            ids = np.array([[self.word_id.get(w, -1) for w in t] for t in kw], dtype=np.int32).reshape(-1, k)
            ok = (ids >= 0).all(axis=1)
            self.skipped.append(int((~ok).sum()))
            ids, kp, kb = ids[ok], kp[ok], kb[ok]
            cap = _capacity(len(ids), max_load)
            keys = np.full((cap, k), -1, dtype=np.int32)
            val = np.zeros((cap, 2), dtype=np.float32)
            if len(ids):
                pos = _place(lm_hash([ids[:, c] for c in range(k)]), cap)
                keys[pos], val[pos, 0], val[pos, 1] = ids, kp, kb
            self.ng_keys.append(keys)
            self.ng_val.append(val)
        self.device = None
        self._dev = None

    # ---- host lookups with the device's probing (tests; the CPU restatement of the decode)
    def probe_trie(self, node: int, label: int) -> Tuple[int, int]:
        """-> (child or -1, slots probed)."""
        cap = len(self.trie)
        s = int(lm_hash([np.array([node]), np.array([label])])[0]) & (cap - 1)
        for p in range(cap):
            e = self.trie[s]
            if e[0] == -1:
                return -1, p + 1
            if e[0] == node and e[1] == label:
                return int(e[2]), p + 1
            s = (s + 1) & (cap - 1)
        return -1, cap

    def probe_ngram(self, ids: Sequence[int]) -> Tuple[Optional[np.ndarray], int]:
        """-> ((log10 p, log10 backoff) or None, slots probed) for a word-id tuple of length 1..order."""
        k = len(ids)
        if k == 1:
            return self.uni[ids[0]], 1
        keys, val = self.ng_keys[k - 2], self.ng_val[k - 2]
        cap = len(keys)
        s = int(lm_hash([np.array([i]) for i in ids])[0]) & (cap - 1)
        for p in range(cap):
            if keys[s, 0] == -1:
                return None, p + 1
            if (keys[s] == ids).all():
                return val[s], p + 1
            s = (s + 1) & (cap - 1)
        return None, cap

    def log10p(self, ctx: Sequence[int], w: int) -> np.float32:
        """log10 P(w | ctx) with ARPA backoff, in the device's fp32 order.  ``ctx``: word ids, most recent last; only the
        trailing run of ids >= 0, at most order-1 of them, is used."""
        hl = 0
        while hl < min(len(ctx), self.order - 1) and ctx[len(ctx) - 1 - hl] >= 0:
            hl += 1
        acc = np.float32(0.0)
        for k in range(hl, 0, -1):
            h = list(ctx[len(ctx) - k:])
            hit, _ = self.probe_ngram(h + [w])
            if hit is not None:
                return np.float32(acc + hit[0])
            hb, _ = self.probe_ngram(h)
            if hb is not None:
                acc = np.float32(acc + hb[1])
        return np.float32(acc + self.uni[w, 0])

    def word_of_node(self, node: int) -> int:
        """Word id completed at a trie node (-1: OOV; node -1 is an OOV prefix)."""
        return int(self.node_word[node]) if node >= 0 else -1

    # ---- device copies
    def to(self, device):
        """Upload the tables; builds the ``ssak_ngram_lm`` descriptor the decode kernels take."""
        import torch
        from . import hip
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        dev = dict(trie=t(self.trie), node_word=t(self.node_word), uni=t(self.uni),
                   keys=[t(k) for k in self.ng_keys], val=[t(v) for v in self.ng_val])
        d = hip.NgramLMDesc()
        d.order, d.n_words, d.bos, d.eos, d.unk = self.order, len(self.words), self.bos, self.eos, self.unk
        d.trie_cap, d.n_nodes = len(self.trie), len(self.node_word)
        d.trie, d.node_word, d.uni = dev["trie"].data_ptr(), dev["node_word"].data_ptr(), dev["uni"].data_ptr()
        for k in range(2, self.order + 1):
            d.ng_keys[k - 1] = dev["keys"][k - 2].data_ptr()
            d.ng_val[k - 1] = dev["val"][k - 2].data_ptr()
            d.ng_cap[k - 1] = len(self.ng_keys[k - 2])
        self.device, self._dev, self.desc = torch.device(device), dev, d
        return self

    def nbytes(self) -> int:
        return sum(a.nbytes for a in [self.trie, self.node_word, self.uni] + self.ng_keys + self.ng_val)


def load_arpa(path: str, tokenizer, device="cuda:0") -> NgramLM:
    """ARPA text file -> :class:`NgramLM` with its tables on ``device``."""
    lm = NgramLM(path, tokenizer)
    return lm.to(device) if device is not None else lm


def decode(logits, lens, lm: NgramLM, tokenizer, alpha: float = 0.5, beta: float = 1.0, beam_width: int = 100,
           beam_prune_logp: float = -10.0, token_min_logp: float = -5.0, unk_score_offset: float = -10.0):
    """CTC beam search with ``lm`` over device logits [B, F, V] fp32 (raw) -> (ids [B, F] int32, n [B] int32, score [B] fp32),
    on the device, under the contract of this module's docstring."""
    from . import hip
    cls = getattr(lm, "_cls", None)
    if cls is None or cls.device != lm.device or cls.numel() != len(tokenizer):
        import torch
        cls = torch.from_numpy(label_classes(tokenizer)).to(lm.device)
        lm._cls = cls
    return hip.ctc_lm_beam_decode(logits, lens, lm.desc, n_labels=len(tokenizer), blank=tokenizer.pad_token_id,
                                  label_class=cls, alpha=alpha, beta=beta, beam_width=beam_width,
                                  beam_prune_logp=beam_prune_logp, token_min_logp=token_min_logp,
                                  unk_score_offset=unk_score_offset)
