// The Whisper generation loop's own kernels (ABI 610, 620): the attention of ONE query per (utterance, head) against a key / value
// cache, and the token selection that closes a step and forms the next step's input row.  Neither entry takes a host copy of a
// device array: the loop of ssak_amd/whisper_seq2seq.py (`generate`) stays on the device between tokens.
//
// dec_attn_step_kernel.  The work per key is one 64-long dot product and one 64-wide axpy: memory-bound, so the kernel is
// built around 16-byte loads of whole rows and bytes in flight, not around the MFMA (dec_attn_kernel's 16-query tile would carry
// one live row).  A 64-element bf16 head row is 128 bytes = 8 lanes x 16 bytes; a wave instruction fetches 8 keys, lane
// (g = lane / 8, c = lane % 8) holding elements [8 c, 8 c + 8) of key g.  A wave takes 32-key tiles (4 K loads and 4 V loads
// issued together: 128 bytes per lane, 8 KB per wave in flight), the four waves of a workgroup take the tiles w, w + 4, ... of the
// workgroup's key range, and n_split workgroups share the keys of one (utterance, head).  Scores: the lane's 8 products
// (fp32 FMA, q scaled by 64^-1/2) summed over the 8 lanes of the key by three DPP steps (fixed order), times log2 e.  Each lane
// group g keeps an online softmax of its own keys -- running maximum, row sum and O[8 c .. 8 c + 8) in fp32; P IS KEPT IN FP32
// into the second product and the row sum is the sum of the same unrounded P.  The 32 (wave, group) partials of a workgroup
// meet in LDS in (wave, group) order; with n_split > 1 the workgroup's (max, sum, O[64]) go to the workspace in fp32 and
// dec_attn_combine_kernel merges the splits in split order.  A partial that saw no key has maximum -inf and sum 0: its factor is
// taken as 0, never exp2(-inf - -inf).  No float atomics, no arrival order: two runs give the same bits.  With `group` > 1 (ABI 630,
// ssak_dec_attention_step_grouped) query row b reads the keys and klens of utterance b / group: the beams of an audio share its
// cross k|v buffer.
//
// dec_token_step_kernel<VEC, TS, SAMPLE>.  One workgroup per row, the two-pass shape of token_logprobs_kernel with the suppress masks applied
// as the columns are read (whisper_step.h: scan_allowed, the loop dec_beam_topk_kernel runs).  Without TS it is the greedy step
// (ABI 610): one running maximum with its lowest column, one sum; the rules' type is NoRules and nothing of them is compiled in.
// With TS (ABI 620) whisper's ApplyTimestampRules are folded into the column predicate.  The rules of a row reduce to uniform
// scalars read before the loop -- the two tokens the kernel itself wrote at columns t - 1 and t - 2, and ts_last[b] -- that give
// one text interval [text_lo, ts_begin) and one timestamp interval [ts_lo, ts_hi]; a column is allowed when no mask byte hits it,
// it is not <|notimestamps|> and it lies in one of the two.  No per-row mask exists in memory.  Pass one carries four running
// statistics per thread (the text and the timestamp maximum, each with its lowest column), pass two the two sums of exp(x - M)
// in column order; lanes, then waves, in a fixed order.  With SAMPLE (ABI 640, ssak_dec_sample_step; with or without TS) passes one
// and two are the same and the mass decision fixes the candidate set instead of the token -- the timestamp columns alone when the
// mass wins, else every allowed column; a third scan takes the arg-max of x_c / T + g_c over that set, g_c = -log(-log(u_c)) a
// Gumbel variate of the counter-based uniform sample_uniform (whisper_step.h), which is one exact draw from softmax(x / T) over
// the set with no prefix sum in it; the log-probability is the drawn column's under the UNTEMPERED processed row.
#include <limits.h>

#include <algorithm>
#include <type_traits>

#include "kernels.h"
#include "whisper_step.h"

namespace {
// ---- ssak_dec_attention_step -------------------------------------------------------------------------------------------------
constexpr int AS_HD = 64;
constexpr int AS_WAVES = 4;
constexpr int AS_THREADS = 64 * AS_WAVES;
constexpr int AS_KT = 32;          // keys per wave tile: 4 loads of 8 keys
constexpr int AS_PARTS = 8 * AS_WAVES;
constexpr int AS_MAX_AUTO_SPLIT = 16;
constexpr int AS_MAX_SPLIT = 64;
constexpr float AS_LOG2E = 1.4426950408889634f;

struct AsParams {
  const bf16* q;
  const bf16* k;
  const bf16* v;
  bf16* ctx;
  const int32_t* klens;
  float* ws_m;  // [B * nh * n_split]
  float* ws_l;  // [B * nh * n_split]
  float* ws_o;  // [B * nh * n_split, 64]
  long ldq, ldk, ldv, k_batch_stride, v_batch_stride;
  int n_keys, nh, n_split, chunk;
  int group;  // query row b reads the keys of utterance b / group (the beams of an audio share its cross k|v)
};

// the sum over the 8 lanes of a key (lanes 8 g .. 8 g + 7): quad swaps, then the mirror of the 8-lane half row
__device__ __forceinline__ float sum8(float v) {
  v += dpp_f<0xB1, 0xf>(0.f, v);
  v += dpp_f<0x4E, 0xf>(0.f, v);
  v += dpp_f<0x141, 0xf>(0.f, v);
  return v;
}

__global__ __launch_bounds__(AS_THREADS) void dec_attn_step_kernel(const AsParams p) {
  __shared__ __attribute__((aligned(16))) float po[AS_PARTS][AS_HD];
  __shared__ float pm[AS_PARTS], pl[AS_PARTS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 3, c = lane & 7;
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  // klens is validated once by the caller that uploaded it; the clamp keeps any value inside the cache
  const int bk = b / p.group;  // the utterance whose keys this query row reads
  const int klen = p.klens ? min(max(p.klens[bk], 1), p.n_keys) : p.n_keys;
  const int k0 = s * p.chunk, k1 = min(min(k0 + p.chunk, p.n_keys), klen);  // this workgroup's visible keys: [k0, k1), maybe empty

  float qf[8];
  chunk_to_f(ld8<bf16>(p.q + (long)b * p.ldq + h * AS_HD + 8 * c), qf);
#pragma unroll
  for (int e = 0; e < 8; ++e) qf[e] *= 0.125f;  // (exact)
  const bf16* const kb = p.k + (long)bk * p.k_batch_stride + h * AS_HD + 8 * c;
  const bf16* const vb = p.v + (long)bk * p.v_batch_stride + h * AS_HD + 8 * c;

  float m = -INFINITY, l = 0.f, o[8];  // log2-domain running maximum, row sum and O of this lane group's keys
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;

  for (int base = k0 + w * AS_KT; base < k1; base += AS_WAVES * AS_KT) {
    Chunk8<bf16> kc[4], vc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = base + 8 * i + g;
      kc[i].q = make_uint4(0, 0, 0, 0);
      vc[i].q = make_uint4(0, 0, 0, 0);  // a masked key's probability is 0: its V must not be NaN
      if (key < k1) {
        kc[i] = ld8<bf16>(kb + (long)key * p.ldk);
        vc[i] = ld8<bf16>(vb + (long)key * p.ldv);
      }
    }
    float sc[4], mx = m;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float kf[8], d = 0.f;
      chunk_to_f(kc[i], kf);
#pragma unroll
      for (int e = 0; e < 8; ++e) d = fmaf(qf[e], kf[e], d);
      d = sum8(d) * AS_LOG2E;
      sc[i] = base + 8 * i + g < k1 ? d : -INFINITY;
      mx = fmaxf(mx, sc[i]);
    }
    const float m_safe = mx == -INFINITY ? 0.f : mx;  // a lane group that has seen no key yet
    const float alpha = __builtin_amdgcn_exp2f(m - m_safe);
    m = mx;
    l *= alpha;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] *= alpha;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float pr = __builtin_amdgcn_exp2f(sc[i] - m_safe);
      float vf[8];
      chunk_to_f(vc[i], vf);
      l += pr;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaf(pr, vf[e], o[e]);
    }
  }
  const int part = w * 8 + g;
  if (c == 0) {
    pm[part] = m;
    pl[part] = l;
  }
  *reinterpret_cast<float4*>(&po[part][8 * c]) = make_float4(o[0], o[1], o[2], o[3]);
  *reinterpret_cast<float4*>(&po[part][8 * c + 4]) = make_float4(o[4], o[5], o[6], o[7]);
  __syncthreads();
  // ---- the 32 partials meet, wave 0 group 0 first: one thread per output element
  if (tid < AS_HD) {
    float M = -INFINITY;
#pragma unroll
    for (int i = 0; i < AS_PARTS; ++i) M = fmaxf(M, pm[i]);
    float L = 0.f, acc = 0.f;
#pragma unroll
    for (int i = 0; i < AS_PARTS; ++i) {
      const float mi = pm[i];
      const float f = mi == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mi - M);
      L += f * pl[i];
      acc += f * po[i][tid];
    }
    const long bh = (long)b * p.nh + h;
    if (p.n_split == 1) {
      p.ctx[bh * AS_HD + tid] = (bf16)(L > 0.f ? acc / L : 0.f);
    } else {
      const long slot = bh * p.n_split + s;
      p.ws_o[slot * AS_HD + tid] = acc;
      if (tid == 0) {
        p.ws_m[slot] = M;  // -inf for a split with no visible key; its sum and O are 0
        p.ws_l[slot] = L;
      }
    }
  }
}

// One 64-thread workgroup per (utterance, head): the splits' partials in split order.
__global__ __launch_bounds__(64) void dec_attn_combine_kernel(const float* __restrict__ ws_m, const float* __restrict__ ws_l,
                                                              const float* __restrict__ ws_o, int n_split, bf16* __restrict__ ctx) {
  const long bh = blockIdx.x;
  const int d = threadIdx.x;
  float M = -INFINITY;
  for (int s = 0; s < n_split; ++s) M = fmaxf(M, ws_m[bh * n_split + s]);
  float L = 0.f, acc = 0.f;
  for (int s = 0; s < n_split; ++s) {
    const float ms = ws_m[bh * n_split + s];
    const float f = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - M);
    L += f * ws_l[bh * n_split + s];
    acc += f * ws_o[(bh * n_split + s) * AS_HD + d];
  }
  ctx[bh * AS_HD + d] = (bf16)(L > 0.f ? acc / L : 0.f);
}

// The split the library chooses: enough workgroups to cover the 256 CUs twice where the keys allow it (at least 128 keys, one
// tile per wave, for every split), ranges cut at multiples of the wave tile.
void choose_split(int bh, int n_keys, int n_split, int* ns, int* chunk) {
  if (n_split > 0) {
    *ns = n_split;
    *chunk = ssak_cdiv(n_keys, n_split);
    return;
  }
  int s = std::min(std::min(ssak_cdiv(512, bh), std::max(1, n_keys / 128)), AS_MAX_AUTO_SPLIT);
  const int ch = ssak_cdiv(ssak_cdiv(n_keys, s), AS_KT) * AS_KT;
  *chunk = ch;
  *ns = ssak_cdiv(n_keys, ch);
}

// ---- ssak_dec_greedy_step, ssak_dec_timestamp_step ---------------------------------------------------------------------------
// (GS_THREADS, the timestamp rules, scan_allowed, block_argmax and form_h_next: whisper_step.h, shared with whisper_beam.hip)
struct GsParams {
  const float* logits;
  const uint8_t* suppress;
  const uint8_t* begin_suppress;  // NULL unless this is the first step
  const bf16* embed_tokens;
  const bf16* embed_positions;
  uint8_t* finished;
  int32_t* n_unfinished;
  int32_t* tokens;
  float* logprobs;
  bf16* h_next;
  long ldv, ldt;
  int V, D, t, next_pos, eos_id, pad_id;
  int32_t* ts_last;  // (this line and the next: read with TS only)
  int ts_begin, no_timestamps_id, max_initial;
  float inv_temperature;  // (this line and the next: read with SAMPLE only)
  uint64_t seed;
};

template <bool VEC, bool TS, bool SAMPLE = false>
__global__ __launch_bounds__(GS_THREADS) void dec_token_step_kernel(const GsParams p) {
  __shared__ float red[16];
  __shared__ int32_t ired[16];
  const int tid = threadIdx.x, row = blockIdx.x;
  const float* x = p.logits + (long)row * p.ldv;
  const bool was_finished = p.finished[row] != 0;  // (read by every thread before thread 0 writes it, behind the barriers below)
  int token = p.pad_id;
  float logprob = 0.f;
  int ts_new = -1;  // what ts_last[row] becomes; only an unfinished row writes it
  if (!was_finished) {  // (uniform over the workgroup)
    const int V = p.V, tsb = TS ? p.ts_begin : V;  // without TS every column is a text column and none is tested
    if constexpr (TS) ts_new = p.t == 0 ? -1 : p.ts_last[row];  // (every thread reads it before thread 0 writes it, behind the barriers below)
    const auto rules = [&] {
      if constexpr (TS)
        return ts_rules(p.tokens + (long)row * p.ldt, p.t, ts_new, V, tsb, p.eos_id, p.no_timestamps_id, p.max_initial);
      else
        return NoRules{};
    }();
    // pass one: the text and the timestamp maximum, each with its lowest column (ms, is, ss keep their initial values without TS)
    float mt = -INFINITY, ms = -INFINITY;
    int32_t it = INT_MAX, is = INT_MAX;
    scan_allowed<VEC>(x, p.suppress, p.begin_suppress, V, rules, [&](int c, float v) {
      // strict: within a thread's increasing columns the first maximum stays.  (Selects, not `if text .. else ..` around two
      // like updates: the compiler merged those into one update through a selected pointer, which put the four in scratch.)
      const bool text = !TS || c < tsb, bt = text && v > mt, bs = !text && v > ms;
      mt = bt ? v : mt, it = bt ? c : it;
      if constexpr (TS) ms = bs ? v : ms, is = bs ? c : is;
    });
    block_argmax(mt, it, red, ired);
    if constexpr (TS) block_argmax(ms, is, red, ired);
    if (it < V || is < V) {  // (a row with no allowed column, the caller's error, emits pad_id with log-prob 0)
      const float M = TS ? fmaxf(mt, ms) : mt;
      float st = 0.f, ss = 0.f;  // pass two: sums of exp(x - M) over the allowed text / timestamp columns, in column order
      scan_allowed<VEC>(x, p.suppress, p.begin_suppress, V, rules, [&](int c, float v) {
        const float ex = expf(v - M);
        st += (!TS || c < tsb) ? ex : 0.f;
        if constexpr (TS) ss += c < tsb ? 0.f : ex;
      });
      st = block_sum(st, red);
      if constexpr (TS) ss = block_sum(ss, red);
      if constexpr (SAMPLE) {
        // pass three: the arg-max of x / T + Gumbel noise over the candidate set the mass decision fixed (a -inf column's score
        // is -inf and never beats the initial -inf; the lowest column on a tie)
        const bool only_ts = TS && ts_mass_wins(ss, mt, M);
        const uint64_t rowseed = sample_rowseed(p.seed, p.t, row);
        const float inv_t = p.inv_temperature;
        float best = -INFINITY;
        int32_t bi = INT_MAX;
        scan_allowed<VEC>(x, p.suppress, p.begin_suppress, V, rules, [&](int c, float v) {
          const float sc = v * inv_t - logf(-logf(sample_uniform(rowseed, c)));
          const bool b = (!TS || !only_ts || c >= tsb) && sc > best;
          best = b ? sc : best, bi = b ? c : bi;
        });
        block_argmax(best, bi, red, ired);
        if (bi < V) {
          token = bi;
          logprob = (x[bi] - M) - logf(only_ts ? ss : st + ss);
        }
      } else if (TS && ts_mass_wins(ss, mt, M)) {
        token = is;
        logprob = (ms - M) - logf(ss);
      } else {
        token = (it < V && mt >= ms) ? it : is;  // (text ids lie below the timestamps: the lowest id on a tie)
        logprob = -logf(st + ss);                // x[token] = M; without TS ss is +0: -log of the one sum, to the bit
      }
      if (TS && token >= tsb) ts_new = token;
    }
  }
  if (tid == 0) {
    p.tokens[(long)row * p.ldt + p.t] = token;
    p.logprobs[(long)row * p.ldt + p.t] = logprob;
    const bool now_finished = was_finished || token == p.eos_id;
    p.finished[row] = now_finished ? 1 : 0;
    if (TS && !was_finished) p.ts_last[row] = ts_new;
    if (!now_finished) atomicAdd(p.n_unfinished, 1);  // (an integer count on the word the entry zeroed: order-free)
  }
  if (p.h_next) form_h_next(p.h_next + (long)row * p.D, p.embed_tokens, p.embed_positions, token, p.V, p.D, p.next_pos);
}
}  // namespace

extern "C" size_t ssak_dec_attention_step_workspace_bytes(int B, int nh, int n_split) {
  if (B <= 0 || nh <= 0 || n_split < 0) return 0;
  const size_t ns = n_split == 0 ? AS_MAX_AUTO_SPLIT : (size_t)n_split;
  return (size_t)B * nh * ns * (AS_HD + 2) * sizeof(float);
}

extern "C" int ssak_dec_attention_step_grouped(const void* q, long ldq, const void* k, long ldk, long k_batch_stride, const void* v, long ldv,
                                               long v_batch_stride, int n_keys, const int32_t* klens, int B, int nh, int head_dim, int n_split,
                                               int group, void* workspace, size_t workspace_bytes, void* ctx, void* stream) {
  SSAK_REQUIRE(q && k && v && ctx, "dec_attention_step: null pointer");
  SSAK_REQUIRE(head_dim == AS_HD, "dec_attention_step: head_dim=%d; the supported head dimension is %d", head_dim, AS_HD);
  SSAK_REQUIRE(B > 0 && B <= 65535 && nh > 0 && nh <= 65535, "dec_attention_step: bad shape B=%d nh=%d", B, nh);
  SSAK_REQUIRE(group >= 1 && B % group == 0, "dec_attention_step: group=%d does not divide the %d query rows", group, B);
  SSAK_REQUIRE(n_keys >= 1, "dec_attention_step: n_keys=%d, at least one key is needed", n_keys);
  SSAK_REQUIRE(n_split >= 0 && n_split <= AS_MAX_SPLIT, "dec_attention_step: n_split=%d outside [0, %d] (0 = the library chooses)", n_split,
               AS_MAX_SPLIT);
  const long D = (long)nh * AS_HD;
  const long strides[5] = {ldq, ldk, ldv, k_batch_stride, v_batch_stride};
  for (long s : strides)
    SSAK_REQUIRE(s >= D && s % 8 == 0,
                 "dec_attention_step: strides ldq=%ld ldk=%ld ldv=%ld k_batch_stride=%ld v_batch_stride=%ld must be multiples of 8 and >= nh * "
                 "%d = %ld",
                 ldq, ldk, ldv, k_batch_stride, v_batch_stride, AS_HD, D);
  SSAK_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(ctx), "dec_attention_step: a buffer is not 16-byte aligned");
  int ns, chunk;
  choose_split(B * nh, n_keys, n_split, &ns, &chunk);
  AsParams p;
  p.q = (const bf16*)q, p.k = (const bf16*)k, p.v = (const bf16*)v, p.ctx = (bf16*)ctx, p.klens = klens;
  p.ws_m = p.ws_l = p.ws_o = nullptr;
  if (ns > 1) {
    const size_t slots = (size_t)B * nh * ns;
    SSAK_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= slots * (AS_HD + 2) * sizeof(float),
                 "dec_attention_step: %d splits need a 16-byte aligned workspace of ssak_dec_attention_step_workspace_bytes = %zu bytes", ns,
                 slots * (AS_HD + 2) * sizeof(float));
    p.ws_o = (float*)workspace;
    p.ws_m = p.ws_o + slots * AS_HD;
    p.ws_l = p.ws_m + slots;
  }
  p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.k_batch_stride = k_batch_stride, p.v_batch_stride = v_batch_stride;
  p.n_keys = n_keys, p.nh = nh, p.n_split = ns, p.chunk = chunk, p.group = group;
  const hipStream_t st = (hipStream_t)stream;
  dec_attn_step_kernel<<<dim3(ns, nh, B), AS_THREADS, 0, st>>>(p);
  SSAK_LAUNCH_CHECK();
  if (ns > 1) {
    dec_attn_combine_kernel<<<B * nh, 64, 0, st>>>(p.ws_m, p.ws_l, p.ws_o, ns, p.ctx);
    SSAK_LAUNCH_CHECK();
  }
  return SSAK_OK;
}

extern "C" int ssak_dec_attention_step(const void* q, long ldq, const void* k, long ldk, long k_batch_stride, const void* v, long ldv,
                                       long v_batch_stride, int n_keys, const int32_t* klens, int B, int nh, int head_dim, int n_split,
                                       void* workspace, size_t workspace_bytes, void* ctx, void* stream) {
  return ssak_dec_attention_step_grouped(q, ldq, k, ldk, k_batch_stride, v, ldv, v_batch_stride, n_keys, klens, B, nh, head_dim, n_split, 1,
                                         workspace, workspace_bytes, ctx, stream);
}

namespace {
// what ssak_dec_greedy_step, ssak_dec_timestamp_step and ssak_dec_sample_step refuse alike; fills the shared parameters
int greedy_params(const char* who, const float* logits, long ldv, int B, int V, const uint8_t* suppress, const uint8_t* begin_suppress, int first,
                  const void* embed_tokens, const void* embed_positions, int D, int max_positions, int next_pos, int eos_id, int pad_id,
                  uint8_t* finished, int32_t* n_unfinished, int32_t* tokens, float* logprobs, long ldt, int t, void* h_next, GsParams* out) {
  SSAK_REQUIRE(logits && finished && n_unfinished && tokens && logprobs, "%s: null pointer", who);
  SSAK_REQUIRE(B > 0 && V > 0 && ldv >= V, "%s: bad shape B=%d V=%d ldv=%ld", who, B, V, ldv);
  SSAK_REQUIRE(eos_id >= 0 && eos_id < V && pad_id >= 0 && pad_id < V, "%s: eos_id=%d / pad_id=%d outside [0, %d)", who, eos_id, pad_id, V);
  SSAK_REQUIRE(t >= 0 && t < ldt, "%s: step t=%d outside the token buffer's %ld columns", who, t, ldt);
  if (const int rc = check_h_next(who, embed_tokens, embed_positions, D, max_positions, next_pos, h_next)) return rc;
  GsParams& p = *out;
  p.logits = logits, p.suppress = suppress, p.begin_suppress = first ? begin_suppress : nullptr;
  p.embed_tokens = (const bf16*)embed_tokens, p.embed_positions = (const bf16*)embed_positions;
  p.finished = finished, p.n_unfinished = n_unfinished, p.tokens = tokens, p.logprobs = logprobs, p.h_next = (bf16*)h_next;
  p.ldv = ldv, p.ldt = ldt, p.V = V, p.D = D, p.t = t, p.next_pos = next_pos, p.eos_id = eos_id, p.pad_id = pad_id;
  p.ts_last = nullptr, p.ts_begin = p.no_timestamps_id = 0, p.max_initial = -1;
  p.inv_temperature = 0.f, p.seed = 0;
  return SSAK_OK;
}
// what the entries that apply the timestamp rules refuse alike; fills the rules' parameters
int ts_params(const char* who, int ts_begin, int no_timestamps_id, int max_initial, int eos_id, int V, int32_t* ts_last, GsParams* out) {
  SSAK_REQUIRE(ts_last, "%s: ts_last is NULL", who);
  SSAK_REQUIRE(ts_begin > eos_id && ts_begin < V, "%s: ts_begin=%d must lie in (eos_id=%d, V=%d)", who, ts_begin, eos_id, V);
  SSAK_REQUIRE(no_timestamps_id >= 0 && no_timestamps_id < V, "%s: no_timestamps_id=%d outside [0, %d)", who, no_timestamps_id, V);
  GsParams& p = *out;
  p.ts_last = ts_last, p.ts_begin = ts_begin, p.no_timestamps_id = no_timestamps_id, p.max_initial = max_initial < 0 ? -1 : max_initial;
  return SSAK_OK;
}
// the count zeroed, then the one kernel on B rows
template <bool TS, bool SAMPLE = false>
int launch_token_step(const GsParams& p, int B, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  SSAK_HIP(hipMemsetAsync(p.n_unfinished, 0, sizeof(int32_t), st));
  if (scan_vec(p.logits, p.ldv, p.suppress, p.begin_suppress))
    dec_token_step_kernel<true, TS, SAMPLE><<<B, GS_THREADS, 0, st>>>(p);
  else
    dec_token_step_kernel<false, TS, SAMPLE><<<B, GS_THREADS, 0, st>>>(p);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}
}  // namespace

extern "C" int ssak_dec_greedy_step(const float* logits, long ldv, int B, int V, const uint8_t* suppress, const uint8_t* begin_suppress,
                                    int first, const void* embed_tokens, const void* embed_positions, int D, int max_positions, int next_pos,
                                    int eos_id, int pad_id, uint8_t* finished, int32_t* n_unfinished, int32_t* tokens, float* logprobs,
                                    long ldt, int t, void* h_next, void* stream) {
  GsParams p;
  const int rc = greedy_params("dec_greedy_step", logits, ldv, B, V, suppress, begin_suppress, first, embed_tokens, embed_positions, D, max_positions,
                               next_pos, eos_id, pad_id, finished, n_unfinished, tokens, logprobs, ldt, t, h_next, &p);
  return rc != SSAK_OK ? rc : launch_token_step<false>(p, B, stream);
}

extern "C" int ssak_dec_timestamp_step(const float* logits, long ldv, int B, int V, const uint8_t* suppress, const uint8_t* begin_suppress,
                                       int first, int ts_begin, int no_timestamps_id, int max_initial, const void* embed_tokens,
                                       const void* embed_positions, int D, int max_positions, int next_pos, int eos_id, int pad_id,
                                       uint8_t* finished, int32_t* n_unfinished, int32_t* tokens, float* logprobs, long ldt, int t,
                                       int32_t* ts_last, void* h_next, void* stream) {
  GsParams p;
  const int rc = greedy_params("dec_timestamp_step", logits, ldv, B, V, suppress, begin_suppress, first, embed_tokens, embed_positions, D,
                               max_positions, next_pos, eos_id, pad_id, finished, n_unfinished, tokens, logprobs, ldt, t, h_next, &p);
  if (rc != SSAK_OK) return rc;
  if (const int rt = ts_params("dec_timestamp_step", ts_begin, no_timestamps_id, max_initial, eos_id, V, ts_last, &p)) return rt;
  return launch_token_step<true>(p, B, stream);
}

extern "C" int ssak_dec_sample_step(const float* logits, long ldv, int B, int V, const uint8_t* suppress, const uint8_t* begin_suppress, int first,
                                    int ts_begin, int no_timestamps_id, int max_initial, const void* embed_tokens, const void* embed_positions,
                                    int D, int max_positions, int next_pos, int eos_id, int pad_id, uint8_t* finished, int32_t* n_unfinished,
                                    int32_t* tokens, float* logprobs, long ldt, int t, int32_t* ts_last, void* h_next, float temperature,
                                    uint64_t seed, void* stream) {
  GsParams p;
  const int rc = greedy_params("dec_sample_step", logits, ldv, B, V, suppress, begin_suppress, first, embed_tokens, embed_positions, D, max_positions,
                               next_pos, eos_id, pad_id, finished, n_unfinished, tokens, logprobs, ldt, t, h_next, &p);
  if (rc != SSAK_OK) return rc;
  // (NaN fails the first comparison; a temperature whose reciprocal overflows fp32 would turn every score into inf)
  SSAK_REQUIRE(temperature > 0.f && 1.f / temperature < INFINITY,
               "dec_sample_step: temperature=%g must be positive with a finite reciprocal (temperature 0 is ssak_dec_greedy_step / "
               "ssak_dec_timestamp_step)",
               (double)temperature);
  p.inv_temperature = 1.f / temperature, p.seed = seed;
  if (!ts_last) return launch_token_step<false, true>(p, B, stream);  // no rules: the timestamp arguments are not read
  if (const int rt = ts_params("dec_sample_step", ts_begin, no_timestamps_id, max_initial, eos_id, V, ts_last, &p)) return rt;
  return launch_token_step<true, true>(p, B, stream);
}
