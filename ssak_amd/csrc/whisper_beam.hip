// Whisper beam search (ABI 630): the three kernels that turn the greedy token step of whisper_generate.hip into a step that keeps
// nb hypotheses per audio (whisper/decoding.py BeamSearchDecoder; the rules are restated in DESIGN.md "Whisper beam search").  As
// in ABI 610 / 620 no entry takes a host mirror of a device array or reads anything back, sums are fp32 in a fixed order and the
// only atomics are integer ones.
//
// dec_beam_topk_kernel.  One workgroup per row of logits [B * nb, ldv].  The column predicate is the token step's (whisper_step.h:
// ts_rules, ts_mass_wins; without timestamps: the suppress masks alone), evaluated on the row's own history.  Pass one and two are
// dec_token_step_kernel's, on the same scan_allowed: the text and the timestamp maximum with their lowest columns, then the two
// sums of exp(x - M) in column order.  The mass decision fixes the candidate set (the timestamps alone, or every allowed
// column) and the log-sum.  Pass one also keeps, per
// thread, the L >= K best text columns and the L best timestamp columns in two sorted register lists (compile-time indices only;
// equal values stay in column order); K rounds of block_argmax over the threads' better heads then give the candidates in the
// order (value descending, column ascending), the owner of each dropping it from its list.  The row is read twice, as before.
//
// dec_beam_select_kernel.  One workgroup per audio.  The nb * K candidates get their fp32 score sum + logprob, each thread counts
// the candidates ordered before its own (score descending, beam ascending, rank ascending: a permutation, no sort network), thread
// 0 walks the order as whisper walks its sorted dict, and then the whole workgroup rewrites the two histories from a copy in LDS
// (every row of t entries is read before any is written: src may repeat a source or form a cycle), stores the newly finished
// sequences and forms the next input rows.
//
// dec_kv_reorder_kernel.  A thread owns one 16-byte chunk of one (layer, audio, key) across the audio's nb beams: it loads the beams
// whose source is another beam, then stores them.  No other thread reads or writes those bytes, so the gather is in place.
#include <type_traits>

#include "kernels.h"
#include "whisper_step.h"

namespace {
constexpr int BM_MAX_NB = 8;
constexpr int BM_MAX_K = BM_MAX_NB + 1;
constexpr int BM_MAX_CAND = BM_MAX_NB * BM_MAX_K;
constexpr int BM_MAX_T = 448;  // history entries per beam the select kernel holds in LDS (Whisper's max_target_positions)

// ---- ssak_dec_beam_topk ------------------------------------------------------------------------------------------------------
struct TkParams {
  const float* logits;
  const uint8_t* suppress;
  const uint8_t* begin_suppress;  // NULL unless this is the first step
  const int32_t* tokens;
  const int32_t* ts_last;
  const uint8_t* done;
  int32_t* cand_token;
  float* cand_logprob;
  long ldv, ldt;
  int V, nb, K, t, eos_id, timestamps, ts_begin, no_timestamps_id, max_initial;
};

// A thread's L best (value, column) pairs of one kind, highest first, in registers: every index below is a compile-time constant.
template <int L>
struct TopList {
  float v[L];
  int32_t c[L];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < L; ++k) v[k] = -INFINITY, c[k] = INT_MAX;
  }
  // the thread's columns come in increasing order, so a value equal to a kept one goes behind it: strict comparisons throughout
  __device__ __forceinline__ void offer(float cv, int32_t cc) {
    if (!(cv > v[L - 1])) return;
    bool sw = false;  // once the new pair has found its slot, everything behind it moves down one, equal values included
#pragma unroll
    for (int k = 0; k < L; ++k) {
      sw = sw || cv > v[k];
      const float tv = sw ? v[k] : cv;
      const int32_t tc = sw ? c[k] : cc;
      v[k] = sw ? cv : v[k];
      c[k] = sw ? cc : c[k];
      cv = tv, cc = tc;
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int k = 0; k + 1 < L; ++k) v[k] = v[k + 1], c[k] = c[k + 1];
    v[L - 1] = -INFINITY, c[L - 1] = INT_MAX;
  }
};

template <bool VEC, int L>
__global__ __launch_bounds__(GS_THREADS) void dec_beam_topk_kernel(const TkParams p) {
  __shared__ float red[16];
  __shared__ int32_t ired[16];
  const int tid = threadIdx.x, row = blockIdx.x;
  if (p.done[row / p.nb]) return;  // (uniform over the workgroup) a done audio's candidates stay as they are
  const float* x = p.logits + (long)row * p.ldv;
  const uint8_t* const s0 = p.suppress;
  const uint8_t* const s1 = p.begin_suppress;
  const int V = p.V, n = p.t, K = p.K;
  TsRules rules = no_rules(V);
  if (p.timestamps)
    rules = ts_rules(p.tokens + (long)row * p.ldt, n, n == 0 ? -1 : p.ts_last[row], V, p.ts_begin, p.eos_id, p.no_timestamps_id, p.max_initial);
  const int tsb = rules.tsb;
  int32_t* const out_t = p.cand_token + (long)row * K;
  float* const out_l = p.cand_logprob + (long)row * K;

  // pass one: the thread's L best text and L best timestamp columns; their heads are dec_token_step_kernel's four running statistics
  TopList<L> lt, ls;
  lt.clear(), ls.clear();
  scan_allowed<VEC>(x, s0, s1, V, rules, [&](int c, float v) {
    if (c < tsb)
      lt.offer(v, c);
    else
      ls.offer(v, c);
  });
  float mt = lt.v[0], ms = ls.v[0];  // the text maximum, the timestamp maximum, each with its lowest column
  int32_t it = lt.c[0], is = ls.c[0];
  block_argmax(mt, it, red, ired);
  block_argmax(ms, is, red, ired);
  int filled = 0;
  if (it < V || is < V) {
    const float M = fmaxf(mt, ms);
    float st = 0.f, ss = 0.f;  // pass two: sums of exp(x - M) over the allowed text / timestamp columns
    scan_allowed<VEC>(x, s0, s1, V, rules, [&](int c, float v) {
      const float ex = expf(v - M);
      st += c < tsb ? ex : 0.f;
      ss += c < tsb ? 0.f : ex;
    });
    st = block_sum(st, red);
    ss = block_sum(ss, red);
    const bool ts_only = ts_mass_wins(ss, mt, M);  // the candidates: the timestamps alone, or every allowed column
    const float lse = logf(ts_only ? ss : st + ss);
    // K rounds: every thread offers the better of its two heads (a tie to the text side: text ids lie below the timestamps), the
    // workgroup's arg-max with the lowest column is the next candidate, its owner drops it
    for (; filled < K; ++filled) {
      const bool text = !ts_only && (lt.v[0] > ls.v[0] || (lt.v[0] == ls.v[0] && lt.c[0] < ls.c[0]));
      float best = text ? lt.v[0] : ls.v[0];
      int32_t bi = text ? lt.c[0] : ls.c[0];
      block_argmax(best, bi, red, ired);
      if (bi >= V) break;  // (uniform) fewer than K candidates
      if (tid == 0) {
        out_t[filled] = bi;
        out_l[filled] = (best - M) - lse;
      }
      if (lt.c[0] == bi) lt.pop();
      if (ls.c[0] == bi) ls.pop();
    }
  }
  if (tid == 0)
    for (int k = filled; k < K; ++k) {
      out_t[k] = -1;
      out_l[k] = -INFINITY;
    }
}

// ---- ssak_dec_beam_select ----------------------------------------------------------------------------------------------------
struct SlParams {
  const int32_t* cand_token;
  const float* cand_logprob;
  float* sum_logprob;
  int32_t* src;
  int32_t* tokens;
  float* logprobs;
  int32_t* ts_last;  // NULL: no timestamps
  int32_t* fin_tokens;
  float* fin_logprobs;
  int32_t* fin_len;
  float* fin_sum;
  int32_t* n_fin;
  uint8_t* done;
  int32_t* n_unfinished;
  const bf16* embed_tokens;
  const bf16* embed_positions;
  bf16* h_next;
  long ldt;
  int nb, K, V, D, t, next_pos, eos_id, pad_id, ts_begin;
};

__global__ __launch_bounds__(GS_THREADS) void dec_beam_select_kernel(const SlParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // the audio's two histories: nb * t tokens, nb * t log-probs
  __shared__ float c_score[BM_MAX_CAND], c_lp[BM_MAX_CAND];
  __shared__ int32_t c_tok[BM_MAX_CAND], c_order[BM_MAX_CAND];  // c_tok < 0: the candidate does not exist
  __shared__ int32_t l_src[BM_MAX_NB], l_tok[BM_MAX_NB], f_src[BM_MAX_NB], f_slot[BM_MAX_NB], n_store;
  __shared__ float l_lp[BM_MAX_NB], l_sum[BM_MAX_NB], f_lp[BM_MAX_NB];
  const int tid = threadIdx.x, b = blockIdx.x, nb = p.nb, K = p.K, t = p.t, nc = nb * K;
  const long row0 = (long)b * nb;
  int32_t* const hT = reinterpret_cast<int32_t*>(smem);
  float* const hL = reinterpret_cast<float*>(smem) + (long)nb * t;
  const bool was_done = p.done[b] != 0;  // (read by every thread before thread 0 writes it, behind the barriers below)
  if (was_done) {  // (uniform) a done audio emits pad, keeps identity sources and changes nothing else
    if (tid < nb) {
      p.tokens[(row0 + tid) * p.ldt + t] = p.pad_id;
      p.logprobs[(row0 + tid) * p.ldt + t] = 0.f;
      p.src[row0 + tid] = (int32_t)(row0 + tid);
    }
    if (p.h_next)
      for (int i = 0; i < nb; ++i) form_h_next(p.h_next + (row0 + i) * p.D, p.embed_tokens, p.embed_positions, p.pad_id, p.V, p.D, p.next_pos);
    return;
  }
  for (int idx = tid; idx < nb * t; idx += GS_THREADS) {
    const long g = (row0 + idx / t) * p.ldt + idx % t;
    hT[idx] = p.tokens[g];
    hL[idx] = p.logprobs[g];
  }
  if (tid < nc) {
    const int j = tid / K;
    const float s = p.sum_logprob[row0 + j];
    const int32_t tk = p.cand_token[row0 * K + tid];
    const float lp = p.cand_logprob[row0 * K + tid];
    const bool ok = s != -INFINITY && tk >= 0 && tk < p.V;  // a beam whose sum is -inf offers nothing
    c_tok[tid] = ok ? tk : -1;
    c_lp[tid] = lp;
    c_score[tid] = ok ? s + lp : -INFINITY;  // one fp32 add, the sum first
  }
  __syncthreads();
  if (tid < nc) {  // the position of candidate tid = (beam, rank): score descending, then beam, then rank; the missing ones last
    const bool ok = c_tok[tid] >= 0;
    const float sc = c_score[tid];
    int before = 0;
    for (int m = 0; m < nc; ++m) {
      const bool okm = c_tok[m] >= 0;
      const float sm = c_score[m];
      before += ok ? (okm && (sm > sc || (sm == sc && m < tid))) : (okm || m < tid);
    }
    c_order[before] = tid;
  }
  __syncthreads();
  if (tid == 0) {
    int32_t tl[BM_MAX_NB];
#pragma unroll
    for (int i = 0; i < BM_MAX_NB; ++i) tl[i] = (p.ts_last && i < nb) ? p.ts_last[row0 + i] : -1;  // every source's value before any is written
    int nf = p.n_fin[b], saved = 0, stored = 0;
    for (int pos = 0; pos < nc && saved < nb; ++pos) {
      const int i = c_order[pos];
      const int32_t tk = c_tok[i];
      if (tk < 0) break;  // the candidates ran out
      if (tk == p.eos_id) {
        if (nf < nb) {
          f_src[stored] = i / K, f_lp[stored] = c_lp[i], f_slot[stored] = nf;
          p.fin_len[row0 + nf] = t + 1;
          p.fin_sum[row0 + nf] = c_score[i];
          ++stored, ++nf;
        }
      } else {
        l_src[saved] = i / K, l_tok[saved] = tk, l_lp[saved] = c_lp[i], l_sum[saved] = c_score[i];
        ++saved;
      }
    }
    for (; saved < nb; ++saved) l_src[saved] = saved, l_tok[saved] = p.pad_id, l_lp[saved] = 0.f, l_sum[saved] = -INFINITY;
    n_store = stored;
    for (int i = 0; i < nb; ++i) {
      p.sum_logprob[row0 + i] = l_sum[i];
      p.src[row0 + i] = (int32_t)(row0 + l_src[i]);
      if (p.ts_last) {
        int32_t v = -1;
#pragma unroll
        for (int s = 0; s < BM_MAX_NB; ++s) v = s == l_src[i] ? tl[s] : v;
        p.ts_last[row0 + i] = l_tok[i] >= p.ts_begin ? l_tok[i] : v;
      }
    }
    p.n_fin[b] = nf;
    p.done[b] = nf >= nb ? 1 : 0;
    if (nf < nb) atomicAdd(p.n_unfinished, 1);  // (an integer count on the word the entry zeroed: order-free)
  }
  __syncthreads();
  // the histories follow the hypotheses, from the copy in LDS; the finished take their source's history plus eos
  for (int idx = tid; idx < nb * t; idx += GS_THREADS) {
    const int i = idx / t, c = idx % t, s = l_src[i];
    if (s != i) {
      const long g = (row0 + i) * p.ldt + c;
      p.tokens[g] = hT[s * t + c];
      p.logprobs[g] = hL[s * t + c];
    }
  }
  if (tid < nb) {
    p.tokens[(row0 + tid) * p.ldt + t] = l_tok[tid];
    p.logprobs[(row0 + tid) * p.ldt + t] = l_lp[tid];
  }
  for (int f = 0; f < n_store; ++f) {
    const long g = (row0 + f_slot[f]) * p.ldt;
    const int s = f_src[f];
    for (int c = tid; c < t; c += GS_THREADS) {
      p.fin_tokens[g + c] = hT[s * t + c];
      p.fin_logprobs[g + c] = hL[s * t + c];
    }
    if (tid == 0) {
      p.fin_tokens[g + t] = p.eos_id;
      p.fin_logprobs[g + t] = f_lp[f];
    }
  }
  if (p.h_next)
    for (int i = 0; i < nb; ++i) form_h_next(p.h_next + (row0 + i) * p.D, p.embed_tokens, p.embed_positions, l_tok[i], p.V, p.D, p.next_pos);
}

// ---- ssak_dec_kv_reorder -----------------------------------------------------------------------------------------------------
constexpr int KR_THREADS = 256;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
struct KrParams {
  bf16* cache;
  const int32_t* src;
  long s_layer, s_row, s_key;
  int row_lo, n_keys, chunks;
};

// grid: (ceil(n_keys * chunks / 256), B, layers); NB = the beams per audio at compile time, so that the sources and the chunks
// in flight sit in registers
// f(integral_constant<0>), ..., f(integral_constant<N - 1>): a loop the compiler cannot leave rolled
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

template <int NB>
__global__ __launch_bounds__(KR_THREADS) void dec_kv_reorder_kernel(const KrParams p) {
  const int b = blockIdx.y, l = blockIdx.z;
  int ls[NB];
  bool any = false;
  static_for<0, NB>([&](auto i) {
    const int s = p.src[b * NB + i] - b * NB;
    ls[i] = (s >= 0 && s < NB) ? s : (int)i;  // (a source outside the audio's own beams is the caller's error: the beam keeps its bytes)
    any |= ls[i] != i;
  });
  if (!any) return;  // (uniform over the workgroup)
  const long idx = (long)blockIdx.x * KR_THREADS + threadIdx.x;
  if (idx >= (long)p.n_keys * p.chunks) return;
  const int key = p.row_lo + (int)(idx / p.chunks), c = (int)(idx % p.chunks);
  bf16* const base = p.cache + l * p.s_layer + (long)b * NB * p.s_row + key * p.s_key + c * 8;
  u32x4 v[NB];  // (a native vector: the struct type of uint4 kept the array in memory)
  static_for<0, NB>([&](auto i) {
    if (ls[i] != i) v[i] = *reinterpret_cast<const u32x4*>(base + ls[i] * p.s_row);
  });
  static_for<0, NB>([&](auto i) {
    if (ls[i] != i) *reinterpret_cast<u32x4*>(base + i * p.s_row) = v[i];
  });
}
}  // namespace

extern "C" int ssak_dec_beam_topk(const float* logits, long ldv, int B, int nb, int V, const uint8_t* suppress, const uint8_t* begin_suppress,
                                  int first, int timestamps, int ts_begin, int no_timestamps_id, int max_initial, int eos_id,
                                  const int32_t* tokens, long ldt, int t, const int32_t* ts_last, const uint8_t* done, int K,
                                  int32_t* cand_token, float* cand_logprob, void* stream) {
  SSAK_REQUIRE(logits && done && cand_token && cand_logprob, "dec_beam_topk: null pointer");
  SSAK_REQUIRE(nb >= 1 && nb <= BM_MAX_NB, "dec_beam_topk: nb=%d outside [1, %d]", nb, BM_MAX_NB);
  SSAK_REQUIRE(K == nb + 1, "dec_beam_topk: K=%d, the candidate buffers hold nb + 1 = %d per row", K, nb + 1);
  SSAK_REQUIRE(B > 0 && (long)B * nb <= 65535 && V > 0 && ldv >= V, "dec_beam_topk: bad shape B=%d nb=%d V=%d ldv=%ld", B, nb, V, ldv);
  SSAK_REQUIRE(eos_id >= 0 && eos_id < V, "dec_beam_topk: eos_id=%d outside [0, %d)", eos_id, V);
  if (timestamps) {
    SSAK_REQUIRE(tokens && ts_last, "dec_beam_topk: the timestamp rules read tokens and ts_last");
    SSAK_REQUIRE(t >= 0 && t < ldt, "dec_beam_topk: step t=%d outside the token buffer's %ld columns", t, ldt);
    SSAK_REQUIRE(ts_begin > eos_id && ts_begin < V, "dec_beam_topk: ts_begin=%d must lie in (eos_id=%d, V=%d)", ts_begin, eos_id, V);
    SSAK_REQUIRE(no_timestamps_id >= 0 && no_timestamps_id < V, "dec_beam_topk: no_timestamps_id=%d outside [0, %d)", no_timestamps_id, V);
  }
  TkParams p;
  p.logits = logits, p.suppress = suppress, p.begin_suppress = first ? begin_suppress : nullptr, p.tokens = tokens, p.ts_last = ts_last;
  p.done = done, p.cand_token = cand_token, p.cand_logprob = cand_logprob, p.ldv = ldv, p.ldt = ldt;
  p.V = V, p.nb = nb, p.K = K, p.t = t, p.eos_id = eos_id, p.timestamps = timestamps ? 1 : 0, p.ts_begin = ts_begin;
  p.no_timestamps_id = no_timestamps_id, p.max_initial = max_initial < 0 ? -1 : max_initial;
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = scan_vec(logits, ldv, p.suppress, p.begin_suppress);
  // (the lists are 6 deep up to nb = 5, whisper's default and the reference's --accurate, and 9 deep beyond)
  if (vec && K <= 6)
    dec_beam_topk_kernel<true, 6><<<B * nb, GS_THREADS, 0, st>>>(p);
  else if (vec)
    dec_beam_topk_kernel<true, BM_MAX_K><<<B * nb, GS_THREADS, 0, st>>>(p);
  else if (K <= 6)
    dec_beam_topk_kernel<false, 6><<<B * nb, GS_THREADS, 0, st>>>(p);
  else
    dec_beam_topk_kernel<false, BM_MAX_K><<<B * nb, GS_THREADS, 0, st>>>(p);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" int ssak_dec_beam_select(const int32_t* cand_token, const float* cand_logprob, int B, int nb, int K, int V, float* sum_logprob,
                                    int32_t* src, int32_t* tokens, float* logprobs, long ldt, int t, int32_t* ts_last, int ts_begin,
                                    int32_t* fin_tokens, float* fin_logprobs, int32_t* fin_len, float* fin_sum, int32_t* n_fin, uint8_t* done,
                                    int32_t* n_unfinished, const void* embed_tokens, const void* embed_positions, int D, int max_positions,
                                    int next_pos, int eos_id, int pad_id, void* h_next, void* stream) {
  SSAK_REQUIRE(cand_token && cand_logprob && sum_logprob && src && tokens && logprobs && fin_tokens && fin_logprobs && fin_len && fin_sum &&
                   n_fin && done && n_unfinished,
               "dec_beam_select: null pointer");
  SSAK_REQUIRE(nb >= 1 && nb <= BM_MAX_NB, "dec_beam_select: nb=%d outside [1, %d]", nb, BM_MAX_NB);
  SSAK_REQUIRE(K == nb + 1, "dec_beam_select: K=%d, the candidate buffers hold nb + 1 = %d per row", K, nb + 1);
  SSAK_REQUIRE(B > 0 && (long)B * nb <= 65535 && V > 0, "dec_beam_select: bad shape B=%d nb=%d V=%d", B, nb, V);
  SSAK_REQUIRE(eos_id >= 0 && eos_id < V && pad_id >= 0 && pad_id < V, "dec_beam_select: eos_id=%d / pad_id=%d outside [0, %d)", eos_id, pad_id, V);
  SSAK_REQUIRE(t >= 0 && t < ldt, "dec_beam_select: step t=%d outside the token buffer's %ld columns", t, ldt);
  SSAK_REQUIRE(t <= BM_MAX_T, "dec_beam_select: step t=%d, the histories of at most %d entries per beam fit the kernel", t, BM_MAX_T);
  if (ts_last) SSAK_REQUIRE(ts_begin > eos_id && ts_begin < V, "dec_beam_select: ts_begin=%d must lie in (eos_id=%d, V=%d)", ts_begin, eos_id, V);
  if (const int rc = check_h_next("dec_beam_select", embed_tokens, embed_positions, D, max_positions, next_pos, h_next)) return rc;
  SlParams p;
  p.cand_token = cand_token, p.cand_logprob = cand_logprob, p.sum_logprob = sum_logprob, p.src = src, p.tokens = tokens, p.logprobs = logprobs;
  p.ts_last = ts_last, p.fin_tokens = fin_tokens, p.fin_logprobs = fin_logprobs, p.fin_len = fin_len, p.fin_sum = fin_sum, p.n_fin = n_fin;
  p.done = done, p.n_unfinished = n_unfinished, p.embed_tokens = (const bf16*)embed_tokens, p.embed_positions = (const bf16*)embed_positions;
  p.h_next = (bf16*)h_next, p.ldt = ldt, p.nb = nb, p.K = K, p.V = V, p.D = D, p.t = t, p.next_pos = next_pos, p.eos_id = eos_id, p.pad_id = pad_id;
  p.ts_begin = ts_begin;
  const hipStream_t st = (hipStream_t)stream;
  SSAK_HIP(hipMemsetAsync(n_unfinished, 0, sizeof(int32_t), st));
  const size_t lds = (size_t)nb * t * 8 + 16;  // at nb = 8, t = 447: 28 KB
  dec_beam_select_kernel<<<B, GS_THREADS, lds, st>>>(p);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" int ssak_dec_kv_reorder(void* cache, const int32_t* src, int layers, int B, int nb, int cap, int width, long layer_stride,
                                   long row_stride, long key_stride, int row_lo, int row_hi, void* stream) {
  SSAK_REQUIRE(cache && src, "dec_kv_reorder: null pointer");
  SSAK_REQUIRE(nb >= 1 && nb <= BM_MAX_NB, "dec_kv_reorder: nb=%d outside [1, %d]", nb, BM_MAX_NB);
  SSAK_REQUIRE(layers > 0 && layers <= 65535 && B > 0 && B <= 65535 && cap > 0 && width > 0 && width % 8 == 0,
               "dec_kv_reorder: bad shape layers=%d B=%d cap=%d width=%d (width a multiple of 8)", layers, B, cap, width);
  SSAK_REQUIRE(row_lo >= 0 && row_lo <= row_hi && row_hi <= cap, "dec_kv_reorder: rows [%d, %d) outside the cache's %d", row_lo, row_hi, cap);
  const long row_span = (long)(cap - 1) * key_stride + width, layer_span = ((long)B * nb - 1) * row_stride + row_span;
  SSAK_REQUIRE(key_stride >= width && row_stride >= row_span && layer_stride >= layer_span && key_stride % 8 == 0 && row_stride % 8 == 0 &&
                   layer_stride % 8 == 0,
               "dec_kv_reorder: strides layer=%ld row=%ld key=%ld must be multiples of 8 and nest (key >= %d, row >= %ld, layer >= %ld)",
               layer_stride, row_stride, key_stride, width, row_span, layer_span);
  SSAK_REQUIRE(aligned16(cache), "dec_kv_reorder: the cache is not 16-byte aligned");
  if (row_lo == row_hi) return SSAK_OK;
  KrParams p;
  p.cache = (bf16*)cache, p.src = src, p.s_layer = layer_stride, p.s_row = row_stride, p.s_key = key_stride;
  p.row_lo = row_lo, p.n_keys = row_hi - row_lo, p.chunks = width / 8;
  const long per = (long)p.n_keys * p.chunks;
  const dim3 grid((unsigned)((per + KR_THREADS - 1) / KR_THREADS), B, layers);
  const hipStream_t st = (hipStream_t)stream;
  switch (nb) {
    case 1: break;  // (one beam per audio: its source is itself)
    case 2: dec_kv_reorder_kernel<2><<<grid, KR_THREADS, 0, st>>>(p); break;
    case 3: dec_kv_reorder_kernel<3><<<grid, KR_THREADS, 0, st>>>(p); break;
    case 4: dec_kv_reorder_kernel<4><<<grid, KR_THREADS, 0, st>>>(p); break;
    case 5: dec_kv_reorder_kernel<5><<<grid, KR_THREADS, 0, st>>>(p); break;
    case 6: dec_kv_reorder_kernel<6><<<grid, KR_THREADS, 0, st>>>(p); break;
    case 7: dec_kv_reorder_kernel<7><<<grid, KR_THREADS, 0, st>>>(p); break;
    default: dec_kv_reorder_kernel<8><<<grid, KR_THREADS, 0, st>>>(p); break;
  }
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}
