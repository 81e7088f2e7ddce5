// The Whisper text decoder's own kernels (ABI 600): token + position embedding, the attention both decoder attentions run
// (causal self-attention over a packed q|k|v buffer, cross-attention over the encoder-side k|v buffer) and the per-row
// log-softmax statistics of the vocabulary projection.  Everything else of a decoder layer is ssak_gemm_bf16 with its bias /
// GELU epilogues and the residual + LayerNorm row kernel of norm_act.hip (ssak_layernorm_fwd); the sequencing is Python
// (ssak_amd/whisper_seq2seq.py).  bf16 storage, fp32 accumulation.  The backward is whisper_train.hip (ABI 650); what it reads of this
// file's forward is the attention's log-sum-exp (ssak_dec_attention_fwd_lse).
//
// dec_attn_kernel.  One workgroup per (utterance, head, 16 queries), 16 being the M of v_mfma_f32_16x16x32_bf16; decoder
// shapes are 1 .. 448 queries against up to 1500 keys, so the key range, not the query range, is what the four waves split:
// wave w takes the 32-key tiles w, w + 4, ... with an online softmax of its own, and the four partial (max, sum, O) meet in LDS
// in wave order.  Scores are computed transposed, S^T = K Q^T: the K rows are the A operand as they sit in memory (one 16-byte
// load per lane), the query is the accumulator's column, i.e. the lane, so a row maximum is 8 registers and two lane exchanges.
// A lane ends up with the probabilities of keys 4g + r and 16 + 4g + r (g = lane / 16) of the tile: taken in that order they are
// the B operand of O^T += V^T P^T with the tile's keys permuted, and V^T is written to LDS (per wave, no workgroup barrier in
// the loop) under the same permutation, so its A operand is one 16-byte LDS read.  Tiles that cross klens or the causal
// diagonal compare key indices; the others do not.  No float atomics; every sum has a fixed order.
#include <limits.h>

#include <algorithm>

#include "kernels.h"

namespace {
// ---- ssak_dec_embed ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dec_embed_kernel(const bf16* __restrict__ tok, const bf16* __restrict__ pos,
                                                        const int32_t* __restrict__ ids, long rows, int L, int D, int V, int pos_offset,
                                                        bf16* __restrict__ out) {
  const int nch = D >> 3;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * nch) return;
  const long row = i / nch;
  const int ch = (int)(i - row * nch);
  // the launcher has validated the host copy of the ids; the clamp keeps a device copy that disagrees inside the table
  const int id = min(max(ids[row], 0), V - 1);
  const int pp = pos_offset + (int)(row % L);
  float e[8], q[8];
  chunk_to_f(ld8<bf16>(tok + (long)id * D + ch * 8), e);
  chunk_to_f(ld8<bf16>(pos + (long)pp * D + ch * 8), q);
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] += q[k];
  st8<bf16>(out + row * D + ch * 8, f_to_chunk8<bf16>(e));
}

// ---- ssak_dec_attention_fwd --------------------------------------------------------------------------------------------------
constexpr int DA_HD = 64;       // the head dimension of every Whisper size
constexpr int DA_QT = 16;       // queries per workgroup
constexpr int DA_KT = 32;       // keys per tile = K of the P V product's instruction
constexpr int DA_WAVES = 4;
constexpr int DA_THREADS = 64 * DA_WAVES;
constexpr int DA_VP = DA_KT + 8;  // bf16 pitch of the V^T image: 80-byte rows keep the 16-byte reads aligned and off one bank group
constexpr int DA_OP = DA_HD + 4;  // fp32 pitch of a wave's partial O
constexpr float DA_LOG2E = 1.4426950408889634f;
constexpr float DA_LN2 = 0.6931471805599453f;

struct DaParams {
  const bf16* q;
  const bf16* k;
  const bf16* v;
  bf16* ctx;
  float* lse;  // [B, nh, Lq] natural-log log-sum-exp of the scaled, masked scores, or null (ssak_dec_attention_fwd_lse)
  const int32_t* klens;
  long ldq, ldk, ldv;
  int Lq, Lk, nh, causal, q_offset;
};

__device__ __forceinline__ bf16x8 ld_bf16x8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

__global__ __launch_bounds__(DA_THREADS) void dec_attn_kernel(const DaParams p) {
  __shared__ __attribute__((aligned(16))) bf16 vt[DA_WAVES][DA_HD][DA_VP];
  __shared__ __attribute__((aligned(16))) float osum[DA_WAVES][DA_QT][DA_OP];
  __shared__ float ms[DA_WAVES][DA_QT], ls[DA_WAVES][DA_QT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * DA_QT, h = blockIdx.y, b = blockIdx.z;
  const int D = p.nh * DA_HD;
  // the launcher has validated the host copy of klens; the clamp keeps a device copy that disagrees inside the buffers
  const int klen = p.klens ? min(max(p.klens[b], 0), p.Lk) : p.Lk;
  const int qlast = min(q0 + DA_QT - 1, p.Lq - 1);
  const int kend = p.causal ? min(klen, p.q_offset + qlast + 1) : klen;  // no query of this tile sees a key >= kend
  const int ntiles = (kend + DA_KT - 1) / DA_KT;

  // Q^T, the B operand of S^T = K Q^T: lane (lr, g) holds q[q0 + lr][8 g + j] and [32 + 8 g + j], scaled by 64^-1/2 (exact in bf16)
  const int qi = q0 + lr;
  bf16x8 qf[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[hh][j] = (bf16)0.f;
  if (qi < p.Lq) {
    const bf16* qp = p.q + ((long)b * p.Lq + qi) * p.ldq + h * DA_HD + 8 * g;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const bf16x8 t = ld_bf16x8(qp + 32 * hh);
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[hh][j] = (bf16)((float)t[j] * 0.125f);
    }
  }
  const int lim = p.causal ? p.q_offset + qi : INT_MAX;  // the last key this lane's query sees

  const bf16* const kb = p.k + (long)b * p.Lk * p.ldk + h * DA_HD + 8 * g;
  const bf16* const vb = p.v + (long)b * p.Lk * p.ldv + h * DA_HD + 8 * (lane & 7);
  float m = -INFINITY, lpart = 0.f;  // log2-domain running maximum of the lane's query; the lane's share of its row sum
  f32x4 oacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) oacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int t = w; t < ntiles; t += DA_WAVES) {
    const int base = t * DA_KT;
    const bool full = base + DA_KT <= klen && (!p.causal || base + DA_KT - 1 <= p.q_offset + q0);  // (wave-uniform)
    // ---- V tile -> LDS, transposed, key kk of the tile at slot 8 ((kk & 15) >> 2) + 4 (kk >> 4) + (kk & 3)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int kk = (lane >> 3) + 8 * n, key = base + kk;
      bf16x8 x;
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = (bf16)0.f;  // a masked key's probability is 0: its V must not be NaN
      if (key < klen) x = ld_bf16x8(vb + (long)key * p.ldv);
      const int slot = 8 * ((kk & 15) >> 2) + 4 * (kk >> 4) + (kk & 3);
#pragma unroll
      for (int j = 0; j < 8; ++j) vt[w][8 * (lane & 7) + j][slot] = x[j];
    }
    // ---- S^T for the tile's two 16-key halves
    f32x4 sc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int key = base + 16 * s + lr;
      bf16x8 ka[2];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int j = 0; j < 8; ++j) ka[hh][j] = (bf16)0.f;
      if (key < klen) {
        ka[0] = ld_bf16x8(kb + (long)key * p.ldk);
        ka[1] = ld_bf16x8(kb + (long)key * p.ldk + 32);
      }
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[0], qf[0], a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[1], qf[1], a, 0, 0, 0);
      sc[s] = a;  // a[r] = score of (query lr, key base + 16 s + 4 g + r)
    }
    float x[2][4];
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = sc[s][r] * DA_LOG2E;
        if (!full) {
          const int key = base + 16 * s + 4 * g + r;
          if (key >= klen || key > lim) v = -INFINITY;
        }
        x[s][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);
    const float m_safe = m_new == -INFINITY ? 0.f : m_new;  // a query that has seen no key yet (below the causal diagonal)
    const float alpha = __builtin_amdgcn_exp2f(m - m_safe);
    m = m_new;
    bf16x8 pb;
    float psum = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = __builtin_amdgcn_exp2f(x[s][r] - m_safe);
        psum += pr;
        pb[4 * s + r] = (bf16)pr;
      }
    lpart = lpart * alpha + psum;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's V^T image is complete (LDS runs a wave's accesses in order)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf16x8 va = *reinterpret_cast<const bf16x8*>(&vt[w][16 * i + lr][8 * g]);  // A[row d = 16 i + lr][slot 8 g + j]
#pragma unroll
      for (int r = 0; r < 4; ++r) oacc[i][r] *= alpha;
      oacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, oacc[i], 0, 0, 0);  // O^T[d = 16 i + 4 g + r][query lr]
    }
  }
  float l = lpart;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (g == 0) {
    ms[w][lr] = m;
    ls[w][lr] = l;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&osum[w][lr][16 * i + 4 * g]) = make_float4(oacc[i][0], oacc[i][1], oacc[i][2], oacc[i][3]);
  __syncthreads();
  // ---- the four partials meet, wave 0 first
  if (tid < DA_QT * 8) {
    const int qq = tid >> 3, ch = tid & 7;
    if (q0 + qq < p.Lq) {
      float M = ms[0][qq];
#pragma unroll
      for (int ww = 1; ww < DA_WAVES; ++ww) M = fmaxf(M, ms[ww][qq]);
      float L = 0.f, o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
      for (int ww = 0; ww < DA_WAVES; ++ww) {
        const float mw = ms[ww][qq];
        const float f = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - M);
        L += f * ls[ww][qq];
        const float4 a = *reinterpret_cast<const float4*>(&osum[ww][qq][8 * ch]), c = *reinterpret_cast<const float4*>(&osum[ww][qq][8 * ch + 4]);
        const float av[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += f * av[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = L > 0.f ? o[e] / L : 0.f;
      st8<bf16>(p.ctx + ((long)b * p.Lq + q0 + qq) * D + h * DA_HD + 8 * ch, f_to_chunk8<bf16>(o));
      if (p.lse && ch == 0) p.lse[((long)b * p.nh + h) * p.Lq + q0 + qq] = (M + log2f(L)) * DA_LN2;
    }
  }
}

// ---- ssak_token_logprobs -----------------------------------------------------------------------------------------------------
constexpr int TL_THREADS = 256;

__device__ __forceinline__ float tl_ld(const float* p) { return *p; }
__device__ __forceinline__ float tl_ld(const bf16* p) { return (float)*p; }
__device__ __forceinline__ void tl_ld4(const float* p, float* v) { *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void tl_ld4(const bf16* p, float* v) { chunk_to_f(ld4<bf16>(p), v); }

// One workgroup per row.  Columns: all of [0, V), or the ids of `allowed`.  Two passes over the row (maximum and arg-max, then
// the sum of exp): per-thread partials in index order, then a fixed-order second stage.  Columns >= V are never read.
template <typename T, bool VEC>
__global__ __launch_bounds__(TL_THREADS) void token_logprobs_kernel(const T* __restrict__ logits, long ldv, int V,
                                                                    const int32_t* __restrict__ targets,
                                                                    const int32_t* __restrict__ allowed, int n_allowed,
                                                                    float* __restrict__ lse, float* __restrict__ logprob,
                                                                    int32_t* __restrict__ argmax, float* __restrict__ probs) {
  __shared__ float red[16];
  __shared__ int32_t ired[16];
  const int tid = threadIdx.x, row = blockIdx.x;
  const T* x = logits + (long)row * ldv;
  const int n = allowed ? n_allowed : V;
  const int n4 = (VEC && !allowed) ? (V & ~3) : 0;  // the vector main loop's extent; the rest goes one column at a time
  float best = -INFINITY;
  int32_t bi = INT_MAX;
  for (int i = tid * 4; i < n4; i += TL_THREADS * 4) {
    float v[4];
    tl_ld4(x + i, v);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (v[e] > best) {  // strict: within a thread's increasing columns the first maximum stays
        best = v[e];
        bi = i + e;
      }
  }
  for (int i = n4 + tid; i < n; i += TL_THREADS) {
    const int col = allowed ? min(max(allowed[i], 0), V - 1) : i;
    const float v = tl_ld(x + col);
    if (v > best || (v == best && col < bi)) {
      best = v;
      bi = col;
    }
  }
  // the lowest id that attains the maximum: lanes, then waves
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ov = __shfl_xor(best, o);
    const int32_t oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = best;
    ired[tid >> 6] = bi;
  }
  __syncthreads();
#pragma unroll
  for (int ww = 0; ww < TL_THREADS / 64; ++ww) {
    const float ov = red[ww];
    const int32_t oi = ired[ww];
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  float s = 0.f;
  for (int i = tid * 4; i < n4; i += TL_THREADS * 4) {
    float v[4];
    tl_ld4(x + i, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) s += expf(v[e] - best);
  }
  for (int i = n4 + tid; i < n; i += TL_THREADS) {
    const int col = allowed ? min(max(allowed[i], 0), V - 1) : i;
    s += expf(tl_ld(x + col) - best);
  }
  s = block_sum(s, red);
  const float lz = best + logf(s);
  if (probs)
    for (int i = tid; i < n_allowed; i += TL_THREADS) {
      const int col = min(max(allowed[i], 0), V - 1);
      probs[(long)row * n_allowed + i] = expf(tl_ld(x + col) - best) / s;
    }
  if (tid == 0) {
    if (lse) lse[row] = lz;
    if (argmax) argmax[row] = bi;
    if (logprob) {
      const int tg = targets ? targets[row] : -1;
      logprob[row] = tg >= 0 ? tl_ld(x + min(tg, V - 1)) - lz : 0.f;  // a negative target (HF's -100) is not scored
    }
  }
}

template <typename T>
int token_logprobs_launch(const T* logits, bool vec, int R, int V, long ldv, const int32_t* targets, const int32_t* allowed, int n_allowed,
                          float* lse, float* logprob, int32_t* argmax, float* probs, hipStream_t st) {
  if (vec)
    token_logprobs_kernel<T, true><<<R, TL_THREADS, 0, st>>>(logits, ldv, V, targets, allowed, n_allowed, lse, logprob, argmax, probs);
  else
    token_logprobs_kernel<T, false><<<R, TL_THREADS, 0, st>>>(logits, ldv, V, targets, allowed, n_allowed, lse, logprob, argmax, probs);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}
}  // namespace

extern "C" int ssak_dec_embed(const void* embed_tokens, const void* embed_positions, const int32_t* ids, const int32_t* ids_host, int B,
                              int L, int D, int V, int max_positions, int pos_offset, void* out, void* stream) {
  SSAK_REQUIRE(embed_tokens && embed_positions && ids && ids_host && out, "dec_embed: null pointer");
  SSAK_REQUIRE(B > 0 && L > 0 && D > 0 && V > 0 && max_positions > 0, "dec_embed: bad shape B=%d L=%d D=%d V=%d max_positions=%d", B, L, D, V,
               max_positions);
  SSAK_REQUIRE(D % 8 == 0, "dec_embed: D=%d is not a multiple of 8", D);
  SSAK_REQUIRE(pos_offset >= 0 && (long)pos_offset + L <= max_positions, "dec_embed: positions [%d, %ld) overrun the table of %d", pos_offset,
               (long)pos_offset + L, max_positions);
  SSAK_REQUIRE(aligned16(embed_tokens) && aligned16(embed_positions) && aligned16(out), "dec_embed: a buffer is not 16-byte aligned");
  const long rows = (long)B * L;
  for (long i = 0; i < rows; ++i)
    SSAK_REQUIRE(ids_host[i] >= 0 && ids_host[i] < V, "dec_embed: id[%ld] = %d outside [0, %d)", i, ids_host[i], V);
  const long total = rows * (D >> 3);
  SSAK_REQUIRE((total + 255) / 256 <= INT_MAX, "dec_embed: too many elements");
  dec_embed_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>((const bf16*)embed_tokens, (const bf16*)embed_positions, ids,
                                                                                       rows, L, D, V, pos_offset, (bf16*)out);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" int ssak_dec_attention_fwd_lse(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, int Lk, const int32_t* klens,
                                          const int32_t* klens_host, int B, int Lq, int nh, int head_dim, int causal, int q_offset, void* ctx,
                                          float* lse, void* stream) {
  SSAK_REQUIRE(q && k && v && ctx, "dec_attention_fwd: null pointer");
  SSAK_REQUIRE(head_dim == DA_HD, "dec_attention_fwd: head_dim=%d; the supported head dimension is %d", head_dim, DA_HD);
  SSAK_REQUIRE(B > 0 && B <= 65535 && Lq > 0 && Lk > 0 && nh > 0 && nh <= 65535, "dec_attention_fwd: bad shape B=%d Lq=%d Lk=%d nh=%d", B, Lq, Lk, nh);
  const long D = (long)nh * DA_HD;
  SSAK_REQUIRE(ldq >= D && ldk >= D && ldv >= D && ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0,
               "dec_attention_fwd: row strides ldq=%ld ldk=%ld ldv=%ld must be multiples of 8 and >= nh * %d = %ld", ldq, ldk, ldv, DA_HD, D);
  SSAK_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(ctx), "dec_attention_fwd: a buffer is not 16-byte aligned");
  SSAK_REQUIRE(q_offset >= 0 && (long)q_offset + Lq <= INT_MAX / 2, "dec_attention_fwd: q_offset=%d", q_offset);
  SSAK_REQUIRE((klens == nullptr) == (klens_host == nullptr),
               "dec_attention_fwd: klens and klens_host come together (the same values on the device and on the host)");
  if (klens_host)
    for (int b = 0; b < B; ++b)
      SSAK_REQUIRE(klens_host[b] >= 1 && klens_host[b] <= Lk, "dec_attention_fwd: klens[%d] = %d outside [1, %d]", b, klens_host[b], Lk);
  DaParams p;
  p.q = (const bf16*)q, p.k = (const bf16*)k, p.v = (const bf16*)v, p.ctx = (bf16*)ctx, p.lse = lse, p.klens = klens;
  p.ldq = ldq, p.ldk = ldk, p.ldv = ldv;
  p.Lq = Lq, p.Lk = Lk, p.nh = nh, p.causal = causal != 0, p.q_offset = q_offset;
  dec_attn_kernel<<<dim3(ssak_cdiv(Lq, DA_QT), nh, B), DA_THREADS, 0, (hipStream_t)stream>>>(p);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

// the same launch without the statistics
extern "C" int ssak_dec_attention_fwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, int Lk, const int32_t* klens,
                                      const int32_t* klens_host, int B, int Lq, int nh, int head_dim, int causal, int q_offset, void* ctx,
                                      void* stream) {
  return ssak_dec_attention_fwd_lse(q, ldq, k, ldk, v, ldv, Lk, klens, klens_host, B, Lq, nh, head_dim, causal, q_offset, ctx, nullptr, stream);
}

extern "C" int ssak_token_logprobs(const void* logits, int dtype, int R, int V, long ldv, const int32_t* targets, const int32_t* targets_host,
                                   const int32_t* allowed, const int32_t* allowed_host, int n_allowed, float* lse, float* logprob,
                                   int32_t* argmax, float* probs, void* stream) {
  SSAK_REQUIRE(logits, "token_logprobs: null pointer");
  SSAK_REQUIRE(dtype == 0 || dtype == 1, "token_logprobs: dtype %d (0 = bf16, 1 = fp32)", dtype);
  SSAK_REQUIRE(R > 0 && V > 0 && ldv >= V, "token_logprobs: bad shape R=%d V=%d ldv=%ld", R, V, ldv);
  SSAK_REQUIRE((targets == nullptr) == (targets_host == nullptr),
               "token_logprobs: targets and targets_host come together (the same values on the device and on the host)");
  SSAK_REQUIRE(targets || !logprob, "token_logprobs: logprob needs targets");
  SSAK_REQUIRE((allowed == nullptr) == (allowed_host == nullptr) && (allowed != nullptr) == (n_allowed > 0),
               "token_logprobs: allowed, allowed_host and n_allowed > 0 come together");
  SSAK_REQUIRE(!probs || allowed, "token_logprobs: probs [R, n_allowed] needs the allowed list");
  if (targets_host)
    for (int r = 0; r < R; ++r) SSAK_REQUIRE(targets_host[r] < V, "token_logprobs: target[%d] = %d outside [0, %d)", r, targets_host[r], V);
  for (int i = 0; i < n_allowed; ++i)
    SSAK_REQUIRE(allowed_host[i] >= 0 && allowed_host[i] < V, "token_logprobs: allowed[%d] = %d outside [0, %d)", i, allowed_host[i], V);
  const bool vec = aligned16(logits) && ldv % 4 == 0;
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == 1)
    return token_logprobs_launch<float>((const float*)logits, vec, R, V, ldv, targets, allowed, n_allowed, lse, logprob, argmax, probs, st);
  return token_logprobs_launch<bf16>((const bf16*)logits, vec, R, V, ldv, targets, allowed, n_allowed, lse, logprob, argmax, probs, st);
}
