// CTC beam search with an ARPA n-gram LM (the --arpa path of ssak/infer/transformers_infer.py:97-133).  gfx950.
//
// Contract (scores, merges, tie rule, LM terms): ssak_amd/lm.py; pyctcdecode parity unpinned.
//
// One 256-thread workgroup per utterance runs the whole frame loop.  Beams (<= 256) live in LDS as structure-of-arrays,
// double-buffered; a beam is (prefix node, last) plus its acoustic score and the prefix's LM state (completed-word score,
// partial-word score, word-trie node, last 5 words).  Per frame:
//   1. log_softmax of the row (fixed-order wave + workgroup reductions), floor at ln 1e-15, argmax (first maximum), and
//      the ordered compaction of S_t;
//   2. a small LDS hash live prefix node -> (blank-ending beam, label-ending beam), so that every beam knows its sibling
//      (same prefix, other `last`) and the beams on its parent prefix;
//   3. candidates = (beam rank i, token j), enumeration index e = i * |S_t| + j.  All sources of a (prefix, last) target use
//      the same token, so the target is emitted by its lowest-ranked source only, which gathers the <= 3 sources' scores
//      itself (no general hash, no float atomics).  Each candidate leaves one sortable 32-bit key (0 = not emitted);
//   4. radix select of the W-th largest key (4 byte-digit histogram passes, integer LDS atomics), collection in
//      enumeration order (ties at the cutoff go to the smaller e), rank-by-count sort of the <= 256 survivors, pruning;
//   5. survivors re-evaluate their candidate and build the next beams; new prefix nodes are numbered in rank order and
//      entered in a per-utterance hash (parent node, label) -> node in the workspace, so a prefix has ONE node for the
//      whole utterance (the identity the merges rely on); the node store (parent, label) is read back at the end.
// Everything is integer or fixed-order fp32 arithmetic: results are bit-reproducible and do not depend on the batch.
#include <math.h>

#include "kernels.h"

namespace {

constexpr int LMD_THREADS = 256;
constexpr int LMD_WAVES = LMD_THREADS / 64;
constexpr int LMD_MAXW = SSAK_LM_MAX_BEAM;
constexpr int LMD_MAXV = SSAK_LM_MAX_LABELS;
constexpr int LMD_CTX = SSAK_LM_MAX_ORDER - 1;
constexpr int LMD_LDS_CAND = 4096;  // candidate keys kept in LDS up to this count, beyond it in the workspace
constexpr int LMD_LIVE = 2 * LMD_MAXW;
constexpr float LMD_LN10 = 2.302585093f;
constexpr float LMD_LP_FLOOR = -34.538776394910684f;  // ln(1e-15)

__device__ __forceinline__ uint32_t hmix(uint32_t h, int x) { return (h ^ (uint32_t)x) * 16777619u; }
__device__ __forceinline__ uint32_t hfin(uint32_t h) {
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  return h;
}

// ---- LM tables (ssak_amd/lm.py builds them with the same hash and probing)
__device__ int trie_child(const ssak_ngram_lm& lm, int node, int label) {
  const uint32_t mask = (uint32_t)lm.trie_cap - 1u;
  uint32_t s = hfin(hmix(hmix(2166136261u, node), label)) & mask;
  for (int p = 0; p < lm.trie_cap; ++p) {
    const int32_t* e = lm.trie + 3 * (size_t)s;
    const int k0 = e[0];
    if (k0 == -1) return -1;
    if (k0 == node && e[1] == label) return e[2];
    s = (s + 1u) & mask;
  }
  return -1;
}

// The k-gram (tail[-k+1 .. -1] of a context ending at ctx_end, then w when with_w) -> its (log10 p, log10 backoff) slot.
// k counts the words looked up.  Returns the value pointer or null.
__device__ const float* ngram_find(const ssak_ngram_lm& lm, const int32_t* ctx_end, int nctx, int w, bool with_w) {
  const int k = nctx + (with_w ? 1 : 0);
  if (k == 1) return lm.uni + 2 * (size_t)(with_w ? w : ctx_end[-1]);
  uint32_t h = 2166136261u;
  for (int j = 0; j < nctx; ++j) h = hmix(h, ctx_end[j - nctx]);
  if (with_w) h = hmix(h, w);
  const int cap = lm.ng_cap[k - 1];
  const int32_t* keys = lm.ng_keys[k - 1];
  if (cap <= 0 || !keys) return nullptr;
  const uint32_t mask = (uint32_t)cap - 1u;
  uint32_t s = hfin(h) & mask;
  for (int p = 0; p < cap; ++p) {
    const int32_t* e = keys + (size_t)s * k;
    if (e[0] == -1) return nullptr;
    bool eq = true;
    for (int j = 0; j < nctx; ++j) eq = eq && e[j] == ctx_end[j - nctx];
    if (with_w) eq = eq && e[nctx] == w;
    if (eq) return lm.ng_val[k - 1] + 2 * (size_t)s;
    s = (s + 1u) & mask;
  }
  return nullptr;
}

// log10 P(w | context) with ARPA backoff; context = the trailing run of ids >= 0 before ctx_end (at most order-1 of them).
// fp32 additions in a fixed order: backoffs from the longest context down, then the hit.
__device__ float lm_log10p(const ssak_ngram_lm& lm, const int32_t* ctx_end, int nctx, int w) {
  const int lim = min(nctx, lm.order - 1);
  int hl = 0;
  while (hl < lim && ctx_end[-1 - hl] >= 0) ++hl;
  float acc = 0.f;
  for (int k = hl; k >= 1; --k) {
    const float* hit = ngram_find(lm, ctx_end, k, w, true);
    if (hit) return acc + hit[0];
    const float* hb = ngram_find(lm, ctx_end, k, 0, false);
    if (hb) acc += hb[1];
  }
  return acc + lm.uni[2 * (size_t)w];
}

__device__ __forceinline__ float lse_fixed(float a, float b, float c) {  // -INFINITY = absent source; order a, b, c
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == -INFINITY) return -INFINITY;
  float s = 0.f;
  if (a != -INFINITY) s += expf(a - m);
  if (b != -INFINITY) s += expf(b - m);
  if (c != -INFINITY) s += expf(c - m);
  return m + logf(s);
}

__device__ __forceinline__ uint32_t sortable(float x) {  // larger float -> larger key; NaN -> 0 (never kept)
  if (x != x) return 0u;
  const uint32_t u = __float_as_uint(x);
  const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return k == 0u ? 1u : k;
}
__device__ __forceinline__ float unsortable(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// ---- per-utterance prefix store in the workspace: node -> (parent, label), hash (parent << 11 | label) -> node
struct PrefixStore {
  int32_t* nodes;                // [2 * max_nodes]
  unsigned long long* hkeys;     // [cap], ~0 = empty
  int32_t* hval;                 // [cap]
  uint32_t* cand;                // overflow candidate keys or null
  int max_nodes;
  int cap;
};

__device__ __forceinline__ uint32_t phash(unsigned long long key) {
  return hfin(hmix(hmix(2166136261u, (int)(key >> 11)), (int)(key & 2047ull)));
}
__device__ int prefix_child(const PrefixStore& ps, int parent, int label) {
  const unsigned long long key = ((unsigned long long)parent << 11) | (unsigned long long)label;
  const uint32_t mask = (uint32_t)ps.cap - 1u;
  uint32_t s = phash(key) & mask;
  for (int p = 0; p < ps.cap; ++p) {
    const unsigned long long k = ps.hkeys[s];
    if (k == ~0ull) return -1;
    if (k == key) return ps.hval[s];
    s = (s + 1u) & mask;
  }
  return -1;
}
__device__ bool prefix_insert(const PrefixStore& ps, int parent, int label, int node) {
  const unsigned long long key = ((unsigned long long)parent << 11) | (unsigned long long)label;
  const uint32_t mask = (uint32_t)ps.cap - 1u;
  uint32_t s = phash(key) & mask;
  for (int p = 0; p < ps.cap; ++p) {
    const unsigned long long old = atomicCAS(ps.hkeys + s, ~0ull, key);
    if (old == ~0ull || old == key) {
      ps.hval[s] = node;
      return true;
    }
    s = (s + 1u) & mask;
  }
  return false;
}

struct Beams {  // structure-of-arrays in LDS
  int node[LMD_MAXW], par[LMD_MAXW], nlab[LMD_MAXW], last[LMD_MAXW], trie[LMD_MAXW], dep[LMD_MAXW];
  int ctx[LMD_MAXW][LMD_CTX];
  float ac[LMD_MAXW], lm[LMD_MAXW], part[LMD_MAXW];
};

struct Shared {
  float lp[LMD_MAXV];
  short stok[LMD_MAXV];
  Beams bm[2];
  int sib[LMD_MAXW], pb[LMD_MAXW], pl[LMD_MAXW];
  int lkey[LMD_LIVE], lb[LMD_LIVE], ll[LMD_LIVE];
  uint32_t ck[LMD_LDS_CAND];
  uint32_t su[LMD_MAXW], se[LMD_MAXW];
  int hist[256];
  float redf[LMD_WAVES];
  int redi[LMD_WAVES], redi2[LMD_WAVES];
  int sel_bin, sel_above, fail;
};

__device__ __forceinline__ float wave_max_f(float v) {
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Workgroup reductions: every wave reduces, wave totals meet in LDS and are combined in wave order by every thread.
__device__ float block_max(Shared& S, float v) {
  v = wave_max_f(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) S.redf[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = S.redf[0];
  for (int w = 1; w < LMD_WAVES; ++w) r = fmaxf(r, S.redf[w]);
  return r;
}
__device__ float block_sum(Shared& S, float v) {
  v = wave_sum_f(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) S.redf[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = S.redf[0];
  for (int w = 1; w < LMD_WAVES; ++w) r += S.redf[w];
  return r;
}
__device__ int block_sum_i(Shared& S, int v) {
  v = wave_sum_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) S.redi[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
  for (int w = 0; w < LMD_WAVES; ++w) r += S.redi[w];
  return r;
}
// Exclusive prefix count of `flag` over the workgroup in thread order; *total = the count.
__device__ int block_scan_flag(Shared& S, bool flag, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int below = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) S.redi2[wv] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < LMD_WAVES; ++w) {
    if (w < wv) off += S.redi2[w];
    tot += S.redi2[w];
  }
  *total = tot;
  return off + below;
}

__device__ int live_find(const Shared& S, int node) {
  uint32_t s = hfin(hmix(2166136261u, node)) & (LMD_LIVE - 1);
  for (int p = 0; p < LMD_LIVE; ++p) {
    const int k = S.lkey[s];
    if (k == -1) return -1;
    if (k == node) return (int)s;
    s = (s + 1u) & (LMD_LIVE - 1);
  }
  return -1;
}

struct Cand {
  bool ext;     // the target prefix is the parent's prefix + v (else: the beam's own prefix)
  int child;    // ext: the target's prefix node when it already exists, else -1
  int word;     // ext: word appended to the LM context (-1: none)
  int trie;
  float ac, lm, part;
};

struct Params {
  ssak_ngram_lm lm;
  ssak_lm_beam_params p;
};

// Candidate (beam i, token v): true when this source emits the target; fills c (acoustic, LM state of the target).
__device__ __forceinline__ bool eval_cand(const Shared& S, const Beams& B, const Params& P, const PrefixStore& ps, int i, int v, float lpv,
                          const uint8_t* __restrict__ cls, Cand& c) {
  const int blank = P.p.blank;
  const float NEG = -INFINITY;
  c.ext = false;
  c.child = -1;
  c.word = -1;
  c.trie = B.trie[i];
  c.lm = B.lm[i];
  c.part = B.part[i];
  if (v == blank) {  // (P, blank): sources [blank-ending beam, label-ending beam]
    const int sb = S.sib[i];
    if (sb >= 0 && sb < i) return false;
    const bool iblank = B.last[i] < 0;
    const float a = B.ac[i] + lpv;
    const float o = sb >= 0 ? B.ac[sb] + lpv : NEG;
    c.ac = iblank ? lse_fixed(a, o, NEG) : lse_fixed(o, a, NEG);
    return true;
  }
  if (v == B.last[i]) {  // repeat: (P, v); sources [repeat, blank-ending parent beam, label-ending parent beam]
    const int qb = S.pb[i];
    int ql = S.pl[i];
    if (ql >= 0 && B.nlab[ql] == v) ql = -1;  // that beam's v is a repeat onto the parent
    if ((qb >= 0 && qb < i) || (ql >= 0 && ql < i)) return false;
    c.ac = lse_fixed(B.ac[i] + lpv, qb >= 0 ? B.ac[qb] + lpv : NEG, ql >= 0 ? B.ac[ql] + lpv : NEG);
    return true;
  }
  // extension (P + v, v): sources [repeat of the child's label-ending beam, blank-ending beam on P, label-ending beam on P]
  const int sb = S.sib[i];
  int eb = B.last[i] < 0 ? i : sb, el = B.last[i] < 0 ? sb : i;
  if (el >= 0 && B.last[el] == v) el = -1;  // (only when el == sib: i itself is not label-ending with last v here)
  if ((eb >= 0 && eb < i) || (el >= 0 && el < i)) return false;
  const int child = prefix_child(ps, B.node[i], v);
  int rq = -1;
  if (child >= 0) {
    const int s = live_find(S, child);
    if (s >= 0) rq = S.ll[s];
  }
  if (rq >= 0 && rq < i) return false;
  c.ext = true;
  c.child = child;
  c.ac = lse_fixed(rq >= 0 ? B.ac[rq] + lpv : NEG, eb >= 0 ? B.ac[eb] + lpv : NEG, el >= 0 ? B.ac[el] + lpv : NEG);
  const int k = cls[v];
  const float unk_part = P.p.alpha * (LMD_LN10 * P.p.unk_score_offset);
  if (k == 0) {  // character
    c.trie = B.trie[i] >= 0 ? trie_child(P.lm, B.trie[i], v) : -1;
    c.part = c.trie >= 0 ? 0.f : unk_part;
  } else if (k == 1 && B.trie[i] != 0) {  // delimiter after a non-empty partial word
    const int t = B.trie[i];
    const int wd = t > 0 && t < P.lm.n_nodes ? P.lm.node_word[t] : -1;
    const bool oov = wd < 0;
    c.word = oov ? P.lm.unk : wd;
    const float L = LMD_LN10 * lm_log10p(P.lm, B.ctx[i] + LMD_CTX, LMD_CTX, c.word);
    c.lm = B.lm[i] + (P.p.alpha * (L + (oov ? LMD_LN10 * P.p.unk_score_offset : 0.f)) + P.p.beta);
    c.trie = 0;
    c.part = 0.f;
  }
  return true;
}

__global__ __launch_bounds__(LMD_THREADS) void lm_beam_kernel(const float* __restrict__ logits, const int32_t* __restrict__ in_lens,
                                                              int F, int V, Params P, char* __restrict__ ws, size_t ws_per_utt,
                                                              int max_nodes, int pcap, int32_t* __restrict__ ids,
                                                              int32_t* __restrict__ out_n, float* __restrict__ out_score) {
  __shared__ Shared S;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int W = P.p.beam_width, NL = P.p.n_labels;
  const uint8_t* cls = P.p.label_class;
  const int T = in_lens ? min(max(in_lens[b], 0), F) : F;
  char* base = ws + (size_t)b * ws_per_utt;
  PrefixStore ps;
  ps.nodes = (int32_t*)base;
  ps.hkeys = (unsigned long long*)(base + (((size_t)max_nodes * 8 + 255) & ~(size_t)255));
  ps.hval = (int32_t*)((char*)ps.hkeys + (size_t)pcap * 8);
  ps.cand = (size_t)W * NL > (size_t)LMD_LDS_CAND ? (uint32_t*)((char*)ps.hval + (((size_t)pcap * 4 + 255) & ~(size_t)255)) : nullptr;
  ps.max_nodes = max_nodes;
  ps.cap = pcap;
  uint32_t* ck = ps.cand ? ps.cand : S.ck;

  int cur = 0, nb = 1, ncount = 1;
  if (tid == 0) {
    Beams& B = S.bm[0];
    B.node[0] = 0;
    B.par[0] = -1;
    B.nlab[0] = -1;
    B.last[0] = -1;
    B.trie[0] = 0;
    B.dep[0] = 0;
    for (int j = 0; j < LMD_CTX; ++j) B.ctx[0][j] = -1;
    B.ctx[0][LMD_CTX - 1] = P.lm.bos;
    B.ac[0] = 0.f;
    B.lm[0] = 0.f;
    B.part[0] = 0.f;
    ps.nodes[0] = -1;
    ps.nodes[1] = -1;
    S.fail = 0;
  }
  __syncthreads();

  for (int t = 0;; ++t) {
    Beams& B = S.bm[cur];
    // ---- 2. live prefix nodes -> (blank-ending beam, label-ending beam); sibling and parent beams
    for (int s = tid; s < LMD_LIVE; s += LMD_THREADS) {
      S.lkey[s] = -1;
      S.lb[s] = -1;
      S.ll[s] = -1;
    }
    __syncthreads();
    if (tid < nb) {
      uint32_t s = hfin(hmix(2166136261u, B.node[tid])) & (LMD_LIVE - 1);
      for (int p = 0; p < LMD_LIVE; ++p) {
        const int old = atomicCAS(&S.lkey[s], -1, B.node[tid]);
        if (old == -1 || old == B.node[tid]) break;
        s = (s + 1u) & (LMD_LIVE - 1);
      }
      if (B.last[tid] < 0) S.lb[s] = tid; else S.ll[s] = tid;
    }
    __syncthreads();
    if (tid < nb) {
      const int s = live_find(S, B.node[tid]);
      S.sib[tid] = B.last[tid] < 0 ? S.ll[s] : S.lb[s];
      const int sp = B.par[tid] >= 0 ? live_find(S, B.par[tid]) : -1;
      S.pb[tid] = sp >= 0 ? S.lb[sp] : -1;
      S.pl[tid] = sp >= 0 ? S.ll[sp] : -1;
    }
    __syncthreads();
    if (t == T) break;

    // ---- 1. log_softmax of the row, S_t
    const float* row = logits + ((size_t)b * F + t) * V;
    float mx = -INFINITY;
    for (int v = tid; v < NL; v += LMD_THREADS) {
      const float x = row[v];
      S.lp[v] = x;
      mx = fmaxf(mx, x);
    }
    mx = block_max(S, mx);
    float se = 0.f;
    for (int v = tid; v < NL; v += LMD_THREADS) se += expf(S.lp[v] - mx);
    const float lse = mx + logf(block_sum(S, se));
    float bestv = -INFINITY;
    for (int v = tid; v < NL; v += LMD_THREADS) {
      const float l = fmaxf(S.lp[v] - lse, LMD_LP_FLOOR);
      S.lp[v] = l;
      bestv = fmaxf(bestv, l);
    }
    bestv = block_max(S, bestv);  // (barriers inside: lp complete)
    int amax = NL;
    for (int v = tid; v < NL; v += LMD_THREADS)
      if (S.lp[v] == bestv) amax = min(amax, v);
    for (int o = 32; o >= 1; o >>= 1) amax = min(amax, __shfl_xor(amax, o, 64));
    __syncthreads();
    if ((tid & 63) == 0) S.redi[tid >> 6] = amax;
    __syncthreads();
    for (int w = 0; w < LMD_WAVES; ++w) amax = min(amax, S.redi[w]);
    int ns = 0;
    for (int v0 = 0; v0 < NL; v0 += LMD_THREADS) {
      const int v = v0 + tid;
      const bool in = v < NL && (S.lp[v] >= P.p.token_min_logp || v == amax);
      int tot;
      const int pos = block_scan_flag(S, in, &tot);
      if (in) S.stok[ns + pos] = (short)v;
      ns += tot;
    }
    __syncthreads();

    // ---- 3. candidates
    const int N = nb * ns;
    int nvalid = 0;
    for (int e = tid; e < N; e += LMD_THREADS) {
      const int i = e / ns, v = S.stok[e - i * ns];
      Cand c;
      uint32_t key = 0u;
      if (eval_cand(S, B, P, ps, i, v, S.lp[v], cls, c)) key = sortable((c.ac + c.lm) + c.part);
      ck[e] = key;
      nvalid += key != 0u;
    }
    nvalid = block_sum_i(S, nvalid);  // (barriers inside: keys complete)
    const int take = min(W, nvalid);

    // ---- 4. selection: threshold key T (the take-th largest) and how many keys equal to T are kept
    uint32_t Tk = 0u;
    int keq = 0;
    if (take < nvalid) {
      uint32_t prefix = 0u;
      int need = take;
      for (int shift = 24; shift >= 0; shift -= 8) {
        S.hist[tid] = 0;
        __syncthreads();
        const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int e = tid; e < N; e += LMD_THREADS) {
          const uint32_t u = ck[e];
          if (u != 0u && (u & himask) == prefix) atomicAdd(&S.hist[(u >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid < 64) {  // wave 0: lane l holds bins 255-4l .. 252-4l; inclusive scan from the top bin down
          const int c0 = S.hist[255 - 4 * tid], c1 = S.hist[254 - 4 * tid], c2 = S.hist[253 - 4 * tid], c3 = S.hist[252 - 4 * tid];
          const int sum = c0 + c1 + c2 + c3;
          int inc = sum;
          for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(inc, o, 64);
            if (tid >= o) inc += y;
          }
          const int exc = inc - sum;
          if (exc < need && inc >= need) {
            int a = exc, bin;
            if (a + c0 >= need) bin = 255 - 4 * tid;
            else if ((a += c0) + c1 >= need) bin = 254 - 4 * tid;
            else if ((a += c1) + c2 >= need) bin = 253 - 4 * tid;
            else { a += c2; bin = 252 - 4 * tid; }
            S.sel_bin = bin;
            S.sel_above = a;
          }
        }
        __syncthreads();
        prefix |= (uint32_t)S.sel_bin << shift;
        need -= S.sel_above;
      }
      Tk = prefix;
      keq = need;
    }
    // collection in enumeration order
    int run_eq = 0, run_sel = 0;
    for (int e0 = 0; e0 < N; e0 += LMD_THREADS) {
      const int e = e0 + tid;
      const uint32_t u = e < N ? ck[e] : 0u;
      const bool eq = u != 0u && u == Tk;
      int teq, tsel;
      const int eqrank = run_eq + block_scan_flag(S, eq, &teq);
      const bool sel = u > Tk || (eq && eqrank < keq);
      const int pos = run_sel + block_scan_flag(S, sel, &tsel);
      if (sel && pos < LMD_MAXW) {
        S.su[pos] = u;
        S.se[pos] = (uint32_t)e;
      }
      run_eq += teq;
      run_sel += tsel;
    }
    __syncthreads();
    // rank-by-count sort (key desc, e asc) and pruning
    uint32_t my_u = 0u, my_e = 0u;
    int rank = -1;
    if (tid < take) {
      my_u = S.su[tid];
      my_e = S.se[tid];
      rank = 0;
      for (int k = 0; k < take; ++k) {
        const uint32_t u = S.su[k], e = S.se[k];
        rank += (u > my_u) || (u == my_u && e < my_e);
      }
    }
    __syncthreads();
    if (rank >= 0) {
      S.su[rank] = my_u;
      S.se[rank] = my_e;
    }
    __syncthreads();
    const float floor_total = unsortable(S.su[0]) + P.p.beam_prune_logp;
    const bool keep = tid < take && unsortable(S.su[tid]) >= floor_total;
    const int nkeep = block_sum_i(S, keep ? 1 : 0);  // kept ranks are a prefix of the sorted order

    // ---- 5. survivors -> next beams
    Beams& NB = S.bm[cur ^ 1];
    Cand c;
    int i = 0, v = 0;
    bool fresh = false;
    if (tid < nkeep) {
      const int e = (int)S.se[tid];
      i = e / ns;
      v = S.stok[e - i * ns];
      eval_cand(S, B, P, ps, i, v, S.lp[v], cls, c);
      fresh = c.ext && c.child < 0;
    }
    int nfresh;
    const int fpos = block_scan_flag(S, fresh, &nfresh);
    if (tid < nkeep) {
      int node = B.node[i], par = B.par[i], nlab = B.nlab[i], dep = B.dep[i];
      if (c.ext) {
        par = B.node[i];
        nlab = v;
        dep = B.dep[i] + 1;
        node = c.child;
        if (fresh) {
          node = ncount + fpos;
          if (node < ps.max_nodes) {
            ps.nodes[2 * (size_t)node] = par;
            ps.nodes[2 * (size_t)node + 1] = v;
            if (!prefix_insert(ps, par, v, node)) S.fail = 1;
          } else {
            S.fail = 1;
          }
        }
      }
      NB.node[tid] = node;
      NB.par[tid] = par;
      NB.nlab[tid] = nlab;
      NB.dep[tid] = dep;
      NB.last[tid] = v == P.p.blank ? -1 : v;
      NB.trie[tid] = c.trie;
      NB.ac[tid] = c.ac;
      NB.lm[tid] = c.lm;
      NB.part[tid] = c.part;
      if (c.word >= 0) {
        for (int j = 0; j < LMD_CTX - 1; ++j) NB.ctx[tid][j] = B.ctx[i][j + 1];
        NB.ctx[tid][LMD_CTX - 1] = c.word;
      } else {
        for (int j = 0; j < LMD_CTX; ++j) NB.ctx[tid][j] = B.ctx[i][j];
      }
    }
    ncount += nfresh;
    nb = nkeep;
    cur ^= 1;
    __syncthreads();
    if (S.fail) break;
  }

  // ---- end of utterance: complete the partial word, </s>, merge the two beams of a prefix, best total
  Beams& B = S.bm[cur];
  Beams& X = S.bm[cur ^ 1];  // scratch: the completed contexts
  float total = -INFINITY;
  if (tid < nb && !S.fail) {
    float lmf = B.lm[tid];
    int word = -1;
    bool oov = false;
    if (B.trie[tid] != 0) {
      const int t = B.trie[tid];
      const int wd = t > 0 && t < P.lm.n_nodes ? P.lm.node_word[t] : -1;
      oov = wd < 0;
      word = oov ? P.lm.unk : wd;
      const float L = LMD_LN10 * lm_log10p(P.lm, B.ctx[tid] + LMD_CTX, LMD_CTX, word);
      lmf = lmf + (P.p.alpha * (L + (oov ? LMD_LN10 * P.p.unk_score_offset : 0.f)) + P.p.beta);
    }
    for (int j = 0; j < LMD_CTX; ++j) X.ctx[tid][j] = word >= 0 ? (j < LMD_CTX - 1 ? B.ctx[tid][j + 1] : word) : B.ctx[tid][j];
    lmf = lmf + P.p.alpha * (LMD_LN10 * lm_log10p(P.lm, X.ctx[tid] + LMD_CTX, LMD_CTX, P.lm.eos));
    const int sb = S.sib[tid];
    if (sb < 0 || tid < sb) {
      const float o = sb >= 0 ? B.ac[sb] : -INFINITY;
      const float ac = B.last[tid] < 0 ? lse_fixed(B.ac[tid], o, -INFINITY) : lse_fixed(o, B.ac[tid], -INFINITY);
      total = ac + lmf;
    }
  }
  // argmax (total desc, rank asc)
  float bt = total;
  int bi = total == -INFINITY ? LMD_THREADS : tid;
  for (int o = 32; o >= 1; o >>= 1) {
    const float ot = __shfl_xor(bt, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ot > bt || (ot == bt && oi < bi)) {
      bt = ot;
      bi = oi;
    }
  }
  __syncthreads();
  if ((tid & 63) == 0) {
    S.redf[tid >> 6] = bt;
    S.redi[tid >> 6] = bi;
  }
  __syncthreads();
  bt = S.redf[0];
  bi = S.redi[0];
  for (int w = 1; w < LMD_WAVES; ++w)
    if (S.redf[w] > bt || (S.redf[w] == bt && S.redi[w] < bi)) {
      bt = S.redf[w];
      bi = S.redi[w];
    }
  const bool ok = !S.fail && bi < nb;
  const int len = ok ? B.dep[bi] : 0;
  int32_t* out = ids + (size_t)b * F;
  for (int k = len + tid; k < F; k += LMD_THREADS) out[k] = -1;
  if (tid == 0) {
    int node = ok ? B.node[bi] : 0;
    for (int k = len - 1; k >= 0 && node > 0; --k) {
      out[k] = ps.nodes[2 * (size_t)node + 1];
      node = ps.nodes[2 * (size_t)node];
    }
    out_n[b] = ok ? len : -1;
    out_score[b] = ok ? bt : NAN;
  }
}

__global__ void lm_query_kernel(ssak_ngram_lm lm, const int32_t* __restrict__ ctx, const int32_t* __restrict__ words, int Q,
                                float* __restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  const int nc = lm.order - 1;
  const int32_t* c = ctx + (size_t)q * nc;
  bool ok = words[q] >= 0 && words[q] < lm.n_words;
  for (int j = 0; j < nc; ++j) ok = ok && c[j] < lm.n_words;
  out[q] = ok ? lm_log10p(lm, c + nc, nc, words[q]) : NAN;  // ids out of range: NaN, never a read outside the tables
}

struct Layout {
  int max_nodes, pcap;
  size_t per_utt;
};
Layout lm_layout(int F, int V, int W) {
  Layout L;
  const long nodes = 1 + (long)F * W;
  long cap = 1;
  while (cap < 2 * nodes) cap *= 2;
  L.max_nodes = (int)nodes;
  L.pcap = (int)cap;
  const size_t a = ((size_t)nodes * 8 + 255) & ~(size_t)255;
  const size_t h = (size_t)cap * 8 + (((size_t)cap * 4 + 255) & ~(size_t)255);
  const size_t nl = (size_t)min(V, LMD_MAXV);
  const size_t c = (size_t)W * nl > (size_t)LMD_LDS_CAND ? (((size_t)W * nl * 4 + 255) & ~(size_t)255) : 0;
  L.per_utt = (a + h + c + 255) & ~(size_t)255;
  return L;
}

int check_lm(const ssak_ngram_lm* lm) {
  SSAK_REQUIRE(lm && lm->order >= 1 && lm->order <= SSAK_LM_MAX_ORDER, "lm: order must be 1..%d", SSAK_LM_MAX_ORDER);
  SSAK_REQUIRE(lm->uni && lm->trie && lm->node_word && lm->n_words > 0 && lm->n_nodes > 0, "lm: null table");
  SSAK_REQUIRE(lm->trie_cap > 0 && (lm->trie_cap & (lm->trie_cap - 1)) == 0, "lm: trie_cap must be a power of two");
  SSAK_REQUIRE(lm->bos >= 0 && lm->bos < lm->n_words && lm->eos >= 0 && lm->eos < lm->n_words && lm->unk >= 0 &&
                   lm->unk < lm->n_words, "lm: <s> / </s> / <unk> ids out of range");
  for (int k = 2; k <= lm->order; ++k)
    SSAK_REQUIRE(lm->ng_keys[k - 1] && lm->ng_val[k - 1] && lm->ng_cap[k - 1] > 0 && (lm->ng_cap[k - 1] & (lm->ng_cap[k - 1] - 1)) == 0,
                 "lm: order-%d table missing or its capacity not a power of two", k);
  return SSAK_OK;
}

}  // namespace

extern "C" size_t ssak_ctc_lm_beam_workspace_bytes(int B, int F, int V, int beam_width) {
  if (B <= 0 || F < 0 || V <= 0 || beam_width <= 0 || beam_width > SSAK_LM_MAX_BEAM) return 0;
  return (size_t)B * lm_layout(F, V, beam_width).per_utt;
}

extern "C" int ssak_ctc_lm_beam_decode(const float* logits, const int32_t* in_lens, int B, int F, int V, const ssak_ngram_lm* lm,
                                       const ssak_lm_beam_params* params, int32_t* ids, int32_t* n, float* score, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  SSAK_REQUIRE(logits && ids && n && score && workspace && params, "lm beam: null pointer");
  SSAK_REQUIRE(B > 0 && F > 0 && V > 0, "lm beam: bad shape B=%d F=%d V=%d", B, F, V);
  const int rc = check_lm(lm);
  if (rc != SSAK_OK) return rc;
  const ssak_lm_beam_params& p = *params;
  SSAK_REQUIRE(p.beam_width >= 1 && p.beam_width <= SSAK_LM_MAX_BEAM, "lm beam: beam_width %d not in 1..%d", p.beam_width,
               SSAK_LM_MAX_BEAM);
  SSAK_REQUIRE(p.n_labels >= 1 && p.n_labels <= V && p.n_labels <= SSAK_LM_MAX_LABELS,
               "lm beam: n_labels %d not in 1..min(V=%d, %d)", p.n_labels, V, SSAK_LM_MAX_LABELS);
  SSAK_REQUIRE(p.blank >= 0 && p.blank < p.n_labels, "lm beam: blank %d not a label", p.blank);
  SSAK_REQUIRE(p.label_class, "lm beam: null label_class");
  SSAK_REQUIRE(!(p.alpha != p.alpha) && !(p.beta != p.beta) && !(p.token_min_logp != p.token_min_logp) &&
                   !(p.beam_prune_logp != p.beam_prune_logp) && !(p.unk_score_offset != p.unk_score_offset),
               "lm beam: NaN parameter");
  const Layout L = lm_layout(F, V, p.beam_width);
  SSAK_REQUIRE(workspace_bytes >= (size_t)B * L.per_utt, "lm beam: workspace %zu bytes < %zu", workspace_bytes,
               (size_t)B * L.per_utt);
  hipStream_t st = (hipStream_t)stream;
  SSAK_HIP(hipMemsetAsync(workspace, 0xFF, (size_t)B * L.per_utt, st));
  Params P;
  P.lm = *lm;
  P.p = p;
  lm_beam_kernel<<<B, LMD_THREADS, 0, st>>>(logits, in_lens, F, V, P, (char*)workspace, L.per_utt, L.max_nodes, L.pcap, ids, n,
                                            score);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" int ssak_lm_query(const ssak_ngram_lm* lm, const int32_t* ctx_ids, const int32_t* words, int Q, float* log10p,
                             void* stream) {
  const int rc = check_lm(lm);
  if (rc != SSAK_OK) return rc;
  SSAK_REQUIRE(Q >= 0 && words && log10p && (ctx_ids || lm->order == 1 || Q == 0), "lm query: null pointer");
  if (Q == 0) return SSAK_OK;
  lm_query_kernel<<<ssak_cdiv(Q, 256), 256, 0, (hipStream_t)stream>>>(*lm, ctx_ids, words, Q, log10p);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}
