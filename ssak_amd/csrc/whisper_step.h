// What the token-selection kernels of the Whisper generation loop share (whisper_generate.hip: dec_timestamp_kernel; whisper_beam.hip:
// dec_beam_topk_kernel): the column predicate of whisper's ApplyTimestampRules, its mass rule, and the workgroup arg-max.  One
// statement of the rules, so that the beam's candidates are filtered exactly as the greedy token is.
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

// the timestamps' mass against the likeliest text token: log S_ts - log S > m_text - M - log S, with ss = S_ts / exp(M)
__device__ __forceinline__ bool ts_mass_wins(float ss, float mt, float M) { return ss > 0.f && logf(ss) > mt - M; }

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
