// What the token-selection kernels of the Whisper generation loop share (whisper_generate.hip: dec_token_step_kernel; whisper_beam.hip:
// dec_beam_topk_kernel): the column predicate of whisper's ApplyTimestampRules, the masked scan of a logits row, its mass rule, the
// workgroup arg-max, the next input row, and the host checks the two files' entries have in common.  One statement of each, so that
// the beam's candidates are filtered, reduced and scored exactly as the greedy token is.
#pragma once
#include <limits.h>

#include "common.h"

constexpr int GS_THREADS = 256;  // one workgroup per logits row

// The rules of a row as uniform scalars: one text interval [text_lo, tsb) and one timestamp interval [ts_lo, ts_hi]; a column is
// allowed when it is not <|notimestamps|> and lies in one of the two (the suppress masks come on top, as the columns are read).
struct TsRules {
  int tsb, text_lo, ts_lo, ts_hi, nots;
  __device__ __forceinline__ bool allowed(int c) const { return c != nots && ((c >= text_lo && c < tsb) || (c >= ts_lo && c <= ts_hi)); }
};

// hist: the row's n tokens so far (of these the last two are read); ts_prev: the row's most recent timestamp id or -1 (-1 at n == 0)
__device__ __forceinline__ TsRules ts_rules(const int32_t* hist, int n, int ts_prev, int V, int tsb, int eos_id, int nots, int max_initial) {
  const bool last = n >= 1 && hist[n - 1] >= tsb;
  const bool pen = n < 2 || hist[n - 2] >= tsb;
  TsRules r;
  r.tsb = tsb, r.nots = nots;
  r.text_lo = n == 0 ? tsb : (last && !pen ? eos_id : 0);
  r.ts_lo = tsb, r.ts_hi = V - 1;
  if (ts_prev >= 0) r.ts_lo = max(r.ts_lo, last && !pen ? ts_prev : ts_prev + 1);
  if (n == 0 && max_initial >= 0) r.ts_hi = min((long)r.ts_hi, (long)tsb + max_initial);
  if (last && pen) r.ts_hi = -1;
  return r;
}

// no rules: every column is a text column (the greedy step's predicate is the suppress masks alone)
__device__ __forceinline__ TsRules no_rules(int V) { return TsRules{V, 0, V, -1, -1}; }
// the same as a type: a kernel instantiated on it carries no per-column test
struct NoRules {
  __device__ __forceinline__ bool allowed(int) const { return true; }
};

// f(column, value) on every column of the row that no mask byte hits and the rules allow; a thread's columns come in increasing order
template <bool VEC, typename R, typename F>
__device__ __forceinline__ void scan_allowed(const float* x, const uint8_t* s0, const uint8_t* s1, int V, const R& rules, F f) {
  const int tid = threadIdx.x;
  const int n4 = VEC ? (V & ~3) : 0;
  for (int i = tid * 4; i < n4; i += GS_THREADS * 4) {
    const float4 q = *reinterpret_cast<const float4*>(x + i);
    uint32_t mk = s0 ? *reinterpret_cast<const uint32_t*>(s0 + i) : 0u;
    if (s1) mk |= *reinterpret_cast<const uint32_t*>(s1 + i);
    const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (!((mk >> (8 * e)) & 0xffu) && rules.allowed(i + e)) f(i + e, v[e]);
  }
  for (int i = n4 + tid; i < V; i += GS_THREADS) {
    const bool sup = (s0 && s0[i]) || (s1 && s1[i]);
    if (!sup && rules.allowed(i)) f(i, x[i]);
  }
}
// whether scan_allowed may take its vector loop: 16-byte logits rows, 4-byte mask words
inline bool scan_vec(const float* logits, long ldv, const uint8_t* s0, const uint8_t* s1) {
  return aligned16(logits) && ldv % 4 == 0 && ((uintptr_t)s0 & 3) == 0 && ((uintptr_t)s1 & 3) == 0;
}

// the timestamps' mass against the likeliest text token: log S_ts - log S > m_text - M - log S, with ss = S_ts / exp(M)
__device__ __forceinline__ bool ts_mass_wins(float ss, float mt, float M) { return ss > 0.f && logf(ss) > mt - M; }

// The uniform of the sampling step (ssak_dec_sample_step), from hash_u32 alone: a key per (seed, step t, row), a word per column
// under a seed whose high half carries that key, and the word's top 23 bits at the centre of their cell: u = (2 k + 1) 2^-24 with
// k in [0, 2^23), strictly inside (0, 1) and exact in fp32.  (Not the rank-one rowkey * colmul word of the dropout masks: there
// two rows' words are multiples of each other.)
constexpr uint32_t DS_SAMPLE = 0x5A0u;
__device__ __forceinline__ uint64_t sample_rowseed(uint64_t seed, int t, int row) {
  const uint32_t k = hash_u32(seed, DS_SAMPLE, ((uint64_t)(uint32_t)t << 32) | (uint32_t)row);
  return seed ^ ((uint64_t)k << 32);
}
__device__ __forceinline__ float sample_uniform(uint64_t rowseed, int c) {
  return ((float)(hash_u32(rowseed, DS_SAMPLE + 1, (uint64_t)(uint32_t)c) >> 9) + 0.5f) * 0x1p-23f;
}

// (value, lowest column) of the maximum over the workgroup: lanes, then waves; every thread returns the same pair
__device__ __forceinline__ void block_argmax(float& best, int32_t& bi, float* red, int32_t* ired) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ov = __shfl_xor(best, o);
    const int32_t oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = best;
    ired[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
#pragma unroll
  for (int ww = 0; ww < GS_THREADS / 64; ++ww) {
    const float ov = red[ww];
    const int32_t oi = ired[ww];
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
}

// the next step's input row: bf16(fp32(embed_tokens[token]) + fp32(embed_positions[next_pos])), by the whole workgroup
__device__ __forceinline__ void form_h_next(bf16* h_row, const bf16* embed_tokens, const bf16* embed_positions, int token, int V, int D,
                                            int next_pos) {
  const int id = min(max(token, 0), V - 1);
  for (int ch = threadIdx.x; ch < (D >> 3); ch += blockDim.x) {
    float e[8], r[8];
    chunk_to_f(ld8<bf16>(embed_tokens + (long)id * D + ch * 8), e);
    chunk_to_f(ld8<bf16>(embed_positions + (long)next_pos * D + ch * 8), r);
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] += r[k];
    st8<bf16>(h_row + ch * 8, f_to_chunk8<bf16>(e));
  }
}
// what an entry that forms h_next refuses (`who`: the entry's name in the message)
inline int check_h_next(const char* who, const void* embed_tokens, const void* embed_positions, int D, int max_positions, int next_pos,
                        const void* h_next) {
  if (!h_next) return SSAK_OK;
  SSAK_REQUIRE(embed_tokens && embed_positions, "%s: h_next needs the two embedding tables", who);
  SSAK_REQUIRE(D > 0 && D % 8 == 0 && max_positions > 0, "%s: bad shape D=%d max_positions=%d", who, D, max_positions);
  SSAK_REQUIRE(next_pos >= 0 && next_pos < max_positions, "%s: next_pos=%d overruns the position table of %d", who, next_pos, max_positions);
  SSAK_REQUIRE(aligned16(embed_tokens) && aligned16(embed_positions) && aligned16(h_next), "%s: a buffer is not 16-byte aligned", who);
  return SSAK_OK;
}
