// Whisper fine-tuning (ABI 650): the backward kernels of the text decoder.  The forward's own kernels are whisper_decoder.hip; every
// projection, bias sum and the feed-forward's GELU pair are ssak_gemm_bf16.  bf16 storage, fp32 accumulation, no float atomics: every
// sum has a fixed order and two runs give the same bits.
//
// ssak_dec_attention_bwd, two kernels in the shape of the forward's (one 16-wide MFMA edge per workgroup, four waves over the long
// edge, the four partials meeting in LDS in wave order).  P is recomputed from the forward's lse; masking is the forward's.
//   dab_dq_kernel   one workgroup per (utterance, head, 16 queries).  delta = rowsum(dO * O) first (written out for the second kernel),
//                   then per 32-key tile S^T = K Q^T and dP^T = V dO^T (K / V rows are the A operand as they sit in memory),
//                   dS = P (dP - delta) in the lane that owns (query, key), and dq^T += K^T dS^T with K^T in LDS under the key
//                   permutation that makes the lane's eight dS values the B operand (the forward's P V product with K for V).
//   dab_dkv_kernel  one workgroup per (utterance, head, 16 keys), the same thing with the roles swapped: the waves walk 32-query
//                   tiles, S = Q K^T and dP = dO V^T (Q / dO rows are the A operand, the block's K / V rows stay in registers), and
//                   dv^T += dO^T P, dk^T += Q^T dS with Q^T (scaled) and dO^T in LDS.  Keys >= klens[b] have P = 0 in every lane,
//                   so their rows of dk / dv are written as zeros.
// ssak_dec_ce_bwd: one workgroup per row, three passes (maximum, sum of exp, dlogits) in ssak_token_logprobs' order; the row losses
// are summed by one workgroup in row order.  ssak_dec_embed_bwd: one workgroup per unique token walks its rows in the CSR's order;
// one per position walks the batch in order.
#include <limits.h>

#include <vector>

#include "kernels.h"

namespace {
constexpr int DB_HD = 64;                    // the head dimension of every Whisper size
constexpr int DB_ET = 16;                    // the workgroup's edge: 16 queries (dq) or 16 keys (dk, dv)
constexpr int DB_RT = 32;                    // the reduction tile: K of the second product's instruction
constexpr int DB_WAVES = 4;
constexpr int DB_THREADS = 64 * DB_WAVES;
constexpr int DB_TP = DB_RT + 8;             // bf16 pitch of a transposed image (80-byte rows: aligned 16-byte reads)
constexpr int DB_OP = DB_HD + 4;             // fp32 pitch of a wave's partial
constexpr float DB_LOG2E = 1.4426950408889634f;

struct DabParams {
  const bf16 *q, *k, *v, *ctx, *dctx;
  const float* lse;
  float* delta;
  bf16 *dq, *dk, *dv;
  const int32_t* klens;
  long ldq, ldk, ldv, lddq, lddk, lddv;
  int Lq, Lk, nh, causal, q_offset;
};

__device__ __forceinline__ bf16x8 db_ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ bf16x8 db_zero8() {
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (bf16)0.f;
  return z;
}
__device__ __forceinline__ bf16x8 db_eighth(const bf16x8 t) {  // the forward's scaling of q: exact in bf16
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (bf16)((float)t[j] * 0.125f);
  return r;
}
// row rr (0 .. 31) of a reduction tile sits at this slot of the transposed image: the lane that owns rows 4 g + r and 16 + 4 g + r
// of the tile holds them as elements 4 s + r of its B operand, i.e. as slots 8 g + 4 s + r
__device__ __forceinline__ int db_slot(int rr) { return 8 * ((rr & 15) >> 2) + 4 * (rr >> 4) + (rr & 3); }

__global__ __launch_bounds__(DB_THREADS) void dab_dq_kernel(const DabParams p) {
  __shared__ __attribute__((aligned(16))) bf16 kt[DB_WAVES][DB_HD][DB_TP];
  __shared__ __attribute__((aligned(16))) float osum[DB_WAVES][DB_ET][DB_OP];
  __shared__ float dl[DB_ET];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * DB_ET, h = blockIdx.y, b = blockIdx.z;
  const int D = p.nh * DB_HD;
  const int klen = p.klens ? min(max(p.klens[b], 0), p.Lk) : p.Lk;
  const int qlast = min(q0 + DB_ET - 1, p.Lq - 1);
  const int kend = p.causal ? min(klen, p.q_offset + qlast + 1) : klen;  // no query of this tile sees a key >= kend
  const int ntiles = (kend + DB_RT - 1) / DB_RT;
  const long stat0 = ((long)b * p.nh + h) * p.Lq;

  // ---- delta[query] = sum_d dO O: eight lanes per query, eight products each in column order, then three exchanges
  if (tid < DB_ET * 8) {
    const int qq = tid >> 3, ch = tid & 7;
    float s = 0.f;
    if (q0 + qq < p.Lq) {
      const long off = ((long)b * p.Lq + q0 + qq) * D + h * DB_HD + 8 * ch;
      const bf16x8 o = db_ld8(p.ctx + off), d = db_ld8(p.dctx + off);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += (float)o[j] * (float)d[j];
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    if (ch == 0) {
      dl[qq] = s;
      if (q0 + qq < p.Lq) p.delta[stat0 + q0 + qq] = s;
    }
  }
  __syncthreads();

  // Q^T (scaled) and dO^T, the B operands of S^T = K Q^T and dP^T = V dO^T: lane (lr, g) holds columns 8 g + j and 32 + 8 g + j
  const int qi = q0 + lr;
  bf16x8 qf[2] = {db_zero8(), db_zero8()}, dof[2] = {db_zero8(), db_zero8()};
  float lse2 = 0.f;
  if (qi < p.Lq) {
    const bf16* qp = p.q + ((long)b * p.Lq + qi) * p.ldq + h * DB_HD + 8 * g;
    const bf16* dp = p.dctx + ((long)b * p.Lq + qi) * D + h * DB_HD + 8 * g;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      qf[hh] = db_eighth(db_ld8(qp + 32 * hh));
      dof[hh] = db_ld8(dp + 32 * hh);
    }
    lse2 = p.lse[stat0 + qi] * DB_LOG2E;
  }
  const float dlt = dl[lr];
  const int lim = p.causal ? p.q_offset + qi : INT_MAX;  // the last key this lane's query sees

  const bf16* const kb = p.k + (long)b * p.Lk * p.ldk + h * DB_HD;
  const bf16* const vb = p.v + (long)b * p.Lk * p.ldv + h * DB_HD;
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int t = w; t < ntiles; t += DB_WAVES) {
    const int base = t * DB_RT;
    const bool full = base + DB_RT <= klen && (!p.causal || base + DB_RT - 1 <= p.q_offset + q0);  // (wave-uniform)
    // ---- K tile -> LDS, transposed and permuted (a masked key's dS is 0: its K must not be NaN)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int kk = (lane >> 3) + 8 * n, key = base + kk;
      bf16x8 x = db_zero8();
      if (key < klen) x = db_ld8(kb + (long)key * p.ldk + 8 * (lane & 7));
      const int slot = db_slot(kk);
#pragma unroll
      for (int j = 0; j < 8; ++j) kt[w][8 * (lane & 7) + j][slot] = x[j];
    }
    bf16x8 dsb;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int key = base + 16 * s + lr;
      bf16x8 ka[2] = {db_zero8(), db_zero8()}, va[2] = {db_zero8(), db_zero8()};
      if (key < klen) {
        ka[0] = db_ld8(kb + (long)key * p.ldk + 8 * g);
        ka[1] = db_ld8(kb + (long)key * p.ldk + 8 * g + 32);
        va[0] = db_ld8(vb + (long)key * p.ldv + 8 * g);
        va[1] = db_ld8(vb + (long)key * p.ldv + 8 * g + 32);
      }
      f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
      sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[0], qf[0], sc, 0, 0, 0);
      sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[1], qf[1], sc, 0, 0, 0);  // sc[r]: (query lr, key base + 16 s + 4 g + r)
      dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[0], dof[0], dp, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[1], dof[1], dp, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pr = __builtin_amdgcn_exp2f(sc[r] * DB_LOG2E - lse2);
        if (!full) {
          const int kx = base + 16 * s + 4 * g + r;
          if (kx >= klen || kx > lim) pr = 0.f;
        }
        dsb[4 * s + r] = (bf16)(pr * (dp[r] - dlt));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's K^T image is complete (LDS runs a wave's accesses in order)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(&kt[w][16 * i + lr][8 * g]);
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, dsb, acc[i], 0, 0, 0);  // dq^T[d = 16 i + 4 g + r][query lr]
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&osum[w][lr][16 * i + 4 * g]) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
  __syncthreads();
  // ---- the four partials meet, wave 0 first
  if (tid < DB_ET * 8) {
    const int qq = tid >> 3, ch = tid & 7;
    if (q0 + qq < p.Lq) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
      for (int ww = 0; ww < DB_WAVES; ++ww) {
        const float4 a = *reinterpret_cast<const float4*>(&osum[ww][qq][8 * ch]), c = *reinterpret_cast<const float4*>(&osum[ww][qq][8 * ch + 4]);
        const float av[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += av[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] *= 0.125f;
      st8<bf16>(p.dq + ((long)b * p.Lq + q0 + qq) * p.lddq + h * DB_HD + 8 * ch, f_to_chunk8<bf16>(o));
    }
  }
}

constexpr int DB_IMG_BYTES = DB_WAVES * DB_HD * DB_TP * 2;          // one transposed image set: 20 480 bytes
constexpr int DB_SUM_BYTES = DB_WAVES * DB_ET * DB_OP * 4;          // one set of partials: 17 408 bytes
constexpr int DB_KV_LDS = 2 * (DB_IMG_BYTES > DB_SUM_BYTES ? DB_IMG_BYTES : DB_SUM_BYTES);

__global__ __launch_bounds__(DB_THREADS) void dab_dkv_kernel(const DabParams p) {
  // the loop's images (Q^T, dO^T per wave) and, after it, the waves' partials (dk, dv) share the same bytes
  __shared__ __attribute__((aligned(16))) unsigned char smem[DB_KV_LDS];
  typedef bf16 (*Img)[DB_HD][DB_TP];
  typedef float (*Sum)[DB_ET][DB_OP];
  const Img qt = reinterpret_cast<Img>(smem), dot = reinterpret_cast<Img>(smem + DB_IMG_BYTES);
  const Sum sumk = reinterpret_cast<Sum>(smem), sumv = reinterpret_cast<Sum>(smem + DB_SUM_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int k0 = blockIdx.x * DB_ET, h = blockIdx.y, b = blockIdx.z;
  const int D = p.nh * DB_HD;
  const int klen = p.klens ? min(max(p.klens[b], 0), p.Lk) : p.Lk;
  const long stat0 = ((long)b * p.nh + h) * p.Lq;
  const int key = k0 + lr;
  const bool kvalid = key < klen;

  // K and V rows of the block, the B operands of S = Q K^T and dP = dO V^T
  bf16x8 kf[2] = {db_zero8(), db_zero8()}, vf[2] = {db_zero8(), db_zero8()};
  if (kvalid) {
    const bf16* kp = p.k + ((long)b * p.Lk + key) * p.ldk + h * DB_HD + 8 * g;
    const bf16* vp = p.v + ((long)b * p.Lk + key) * p.ldv + h * DB_HD + 8 * g;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      kf[hh] = db_ld8(kp + 32 * hh);
      vf[hh] = db_ld8(vp + 32 * hh);
    }
  }
  const bf16* const qb = p.q + (long)b * p.Lq * p.ldq + h * DB_HD;
  const bf16* const db = p.dctx + (long)b * p.Lq * D + h * DB_HD;
  f32x4 ak[4], av[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) ak[i] = av[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // query i sees key j iff j <= q_offset + i: the tiles before query k0 - q_offset see none of the block's keys
  const int t0 = p.causal ? max(k0 - p.q_offset, 0) / DB_RT : 0;
  const int ntiles = k0 < klen ? (p.Lq + DB_RT - 1) / DB_RT : 0;
  for (int t = t0 + w; t < ntiles; t += DB_WAVES) {
    const int base = t * DB_RT;
    // ---- Q (scaled) and dO tiles -> LDS, transposed and permuted; rows >= Lq are zeros
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int rr = (lane >> 3) + 8 * n, qx = base + rr;
      bf16x8 x = db_zero8(), y = db_zero8();
      if (qx < p.Lq) {
        x = db_eighth(db_ld8(qb + (long)qx * p.ldq + 8 * (lane & 7)));
        y = db_ld8(db + (long)qx * D + 8 * (lane & 7));
      }
      const int slot = db_slot(rr);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        qt[w][8 * (lane & 7) + j][slot] = x[j];
        dot[w][8 * (lane & 7) + j][slot] = y[j];
      }
    }
    bf16x8 pb, dsb;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int qx = base + 16 * s + lr;
      bf16x8 qa[2] = {db_zero8(), db_zero8()}, da[2] = {db_zero8(), db_zero8()};
      if (qx < p.Lq) {
        qa[0] = db_eighth(db_ld8(qb + (long)qx * p.ldq + 8 * g));
        qa[1] = db_eighth(db_ld8(qb + (long)qx * p.ldq + 8 * g + 32));
        da[0] = db_ld8(db + (long)qx * D + 8 * g);
        da[1] = db_ld8(db + (long)qx * D + 8 * g + 32);
      }
      f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
      sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[0], kf[0], sc, 0, 0, 0);
      sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[1], kf[1], sc, 0, 0, 0);  // sc[r]: (query base + 16 s + 4 g + r, key k0 + lr)
      dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[0], vf[0], dp, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[1], vf[1], dp, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qr = base + 16 * s + 4 * g + r;
        float pr = 0.f, ds = 0.f;
        if (kvalid && qr < p.Lq && (!p.causal || key <= p.q_offset + qr)) {
          pr = __builtin_amdgcn_exp2f(sc[r] * DB_LOG2E - p.lse[stat0 + qr] * DB_LOG2E);
          ds = pr * (dp[r] - p.delta[stat0 + qr]);
        }
        pb[4 * s + r] = (bf16)pr;
        dsb[4 * s + r] = (bf16)ds;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's images are complete (LDS runs a wave's accesses in order)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(&qt[w][16 * i + lr][8 * g]);
      const bf16x8 c = *reinterpret_cast<const bf16x8*>(&dot[w][16 * i + lr][8 * g]);
      ak[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, dsb, ak[i], 0, 0, 0);  // dk^T[d = 16 i + 4 g + r][key lr]
      av[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c, pb, av[i], 0, 0, 0);   // dv^T
    }
  }
  __syncthreads();  // every wave is done with its images: the partials take their place
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    *reinterpret_cast<float4*>(&sumk[w][lr][16 * i + 4 * g]) = make_float4(ak[i][0], ak[i][1], ak[i][2], ak[i][3]);
    *reinterpret_cast<float4*>(&sumv[w][lr][16 * i + 4 * g]) = make_float4(av[i][0], av[i][1], av[i][2], av[i][3]);
  }
  __syncthreads();
  // ---- the four partials meet, wave 0 first: threads 0 .. 127 write dk, 128 .. 255 dv
  {
    const int which = tid >> 7, kk = (tid & 127) >> 3, ch = tid & 7;
    if (k0 + kk < p.Lk) {
      const Sum sum = which ? sumv : sumk;
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
      for (int ww = 0; ww < DB_WAVES; ++ww) {
        const float4 a = *reinterpret_cast<const float4*>(&sum[ww][kk][8 * ch]);
        const float4 c = *reinterpret_cast<const float4*>(&sum[ww][kk][8 * ch + 4]);
        const float x[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += x[e];
      }
      bf16* const out = which ? p.dv + ((long)b * p.Lk + k0 + kk) * p.lddv : p.dk + ((long)b * p.Lk + k0 + kk) * p.lddk;
      st8<bf16>(out + h * DB_HD + 8 * ch, f_to_chunk8<bf16>(o));
    }
  }
}

// ---- ssak_dec_ce_bwd ---------------------------------------------------------------------------------------------------------
constexpr int CE_THREADS = 256;

// One workgroup per row.  An ignored row (target < 0) is all zeros.  A scored row: the maximum, then the sum of exp as per-thread
// partials in column order and a fixed-order second stage (ssak_token_logprobs' statistics), then the gradient.
template <bool VEC>
__global__ __launch_bounds__(CE_THREADS) void ce_bwd_kernel(const float* __restrict__ logits, long ldv, int V, const int32_t* __restrict__ targets,
                                                            float grad_scale, bf16* __restrict__ dlogits, long ldd, float* __restrict__ row_loss) {
  __shared__ float red[16];
  const int tid = threadIdx.x, row = blockIdx.x;
  const float* x = logits + (long)row * ldv;
  bf16* d = dlogits + (long)row * ldd;
  // the launcher has validated the host copy of the targets; the clamp keeps a device copy that disagrees inside the row
  const int tg = min(targets[row], V - 1);
  if (tg < 0) {
    for (long i = tid; i < ldd; i += CE_THREADS) d[i] = (bf16)0.f;
    if (tid == 0 && row_loss) row_loss[row] = 0.f;
    return;
  }
  const int n4 = VEC ? (V & ~3) : 0;  // the vector loops' extent; the rest goes one column at a time
  float best = -INFINITY;
  for (int i = tid * 4; i < n4; i += CE_THREADS * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    best = fmaxf(fmaxf(fmaxf(best, v.x), fmaxf(v.y, v.z)), v.w);
  }
  for (int i = n4 + tid; i < V; i += CE_THREADS) best = fmaxf(best, x[i]);
  best = block_max(best, red);
  float s = 0.f;
  for (int i = tid * 4; i < n4; i += CE_THREADS * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    s += expf(v.x - best);
    s += expf(v.y - best);
    s += expf(v.z - best);
    s += expf(v.w - best);
  }
  for (int i = n4 + tid; i < V; i += CE_THREADS) s += expf(x[i] - best);
  s = block_sum(s, red);
  const float lz = best + logf(s);
  for (int i = tid * 4; i < n4; i += CE_THREADS * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    const float e[4] = {v.x, v.y, v.z, v.w};
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (bf16)((expf(e[j] - lz) - (i + j == tg ? 1.f : 0.f)) * grad_scale);
    *reinterpret_cast<bf16x4*>(d + i) = o;
  }
  for (int i = n4 + tid; i < V; i += CE_THREADS) d[i] = (bf16)((expf(x[i] - lz) - (i == tg ? 1.f : 0.f)) * grad_scale);
  for (long i = V + tid; i < ldd; i += CE_THREADS) d[i] = (bf16)0.f;
  if (tid == 0 && row_loss) row_loss[row] = lz - x[tg];
}

// loss_sum[0] += the row losses: per-thread partials in row order, then the fixed-order second stage
__global__ __launch_bounds__(CE_THREADS) void ce_loss_sum_kernel(const float* __restrict__ row_loss, int R, float* __restrict__ loss_sum) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < R; i += CE_THREADS) s += row_loss[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) loss_sum[0] += s;
}

// ---- ssak_dec_embed_bwd ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_bwd_tokens_kernel(const bf16* __restrict__ dh, long N, int D, int Vp, const int32_t* __restrict__ uniq,
                                                               const int32_t* __restrict__ offs, const int32_t* __restrict__ rows,
                                                               float* __restrict__ d_tok) {
  const int u = blockIdx.x;
  // the launcher has validated the host copies; the clamps keep device copies that disagree inside the buffers
  const int id = min(max(uniq[u], 0), Vp - 1);
  const long lo = min(max((long)offs[u], 0L), N), hi = min(max((long)offs[u + 1], lo), N);
  for (int c = threadIdx.x; c < D; c += 256) {
    float s = 0.f;
    for (long j = lo; j < hi; ++j) {
      const long r = min(max((long)rows[j], 0L), N - 1);
      s += (float)dh[r * D + c];
    }
    d_tok[(long)id * D + c] += s;
  }
}

__global__ __launch_bounds__(256) void embed_bwd_positions_kernel(const bf16* __restrict__ dh, int B, int L, int D, int pos_offset,
                                                                  float* __restrict__ d_pos) {
  const int i = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += 256) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += (float)dh[((long)b * L + i) * D + c];
    d_pos[(long)(pos_offset + i) * D + c] += s;
  }
}
}  // namespace

extern "C" int ssak_dec_attention_bwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, int Lk, const int32_t* klens,
                                      const int32_t* klens_host, int B, int Lq, int nh, int head_dim, int causal, int q_offset,
                                      const void* ctx, const float* lse, const void* dctx, void* dq, long lddq, void* dk, long lddk, void* dv,
                                      long lddv, float* delta, void* stream) {
  SSAK_REQUIRE(q && k && v && ctx && lse && dctx && dq && dk && dv && delta, "dec_attention_bwd: null pointer");
  SSAK_REQUIRE(head_dim == DB_HD, "dec_attention_bwd: head_dim=%d; the supported head dimension is %d", head_dim, DB_HD);
  SSAK_REQUIRE(B > 0 && B <= 65535 && Lq > 0 && Lk > 0 && nh > 0 && nh <= 65535, "dec_attention_bwd: bad shape B=%d Lq=%d Lk=%d nh=%d", B, Lq, Lk, nh);
  const long D = (long)nh * DB_HD;
  const long lds[6] = {ldq, ldk, ldv, lddq, lddk, lddv};
  for (int i = 0; i < 6; ++i)
    SSAK_REQUIRE(lds[i] >= D && lds[i] % 8 == 0,
                 "dec_attention_bwd: row strides ldq=%ld ldk=%ld ldv=%ld lddq=%ld lddk=%ld lddv=%ld must be multiples of 8 and >= nh * %d = %ld", ldq,
                 ldk, ldv, lddq, lddk, lddv, DB_HD, D);
  SSAK_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(ctx) && aligned16(dctx) && aligned16(dq) && aligned16(dk) && aligned16(dv),
               "dec_attention_bwd: a buffer is not 16-byte aligned");
  SSAK_REQUIRE(q_offset >= 0 && (long)q_offset + Lq <= INT_MAX / 2, "dec_attention_bwd: q_offset=%d", q_offset);
  SSAK_REQUIRE((klens == nullptr) == (klens_host == nullptr),
               "dec_attention_bwd: klens and klens_host come together (the same values on the device and on the host)");
  if (klens_host)
    for (int b = 0; b < B; ++b)
      SSAK_REQUIRE(klens_host[b] >= 1 && klens_host[b] <= Lk, "dec_attention_bwd: klens[%d] = %d outside [1, %d]", b, klens_host[b], Lk);
  DabParams p;
  p.q = (const bf16*)q, p.k = (const bf16*)k, p.v = (const bf16*)v, p.ctx = (const bf16*)ctx, p.dctx = (const bf16*)dctx;
  p.lse = lse, p.delta = delta, p.dq = (bf16*)dq, p.dk = (bf16*)dk, p.dv = (bf16*)dv, p.klens = klens;
  p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.lddq = lddq, p.lddk = lddk, p.lddv = lddv;
  p.Lq = Lq, p.Lk = Lk, p.nh = nh, p.causal = causal != 0, p.q_offset = q_offset;
  const hipStream_t st = (hipStream_t)stream;
  dab_dq_kernel<<<dim3(ssak_cdiv(Lq, DB_ET), nh, B), DB_THREADS, 0, st>>>(p);
  SSAK_LAUNCH_CHECK();
  dab_dkv_kernel<<<dim3(ssak_cdiv(Lk, DB_ET), nh, B), DB_THREADS, 0, st>>>(p);  // reads the delta the first kernel wrote
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" int ssak_dec_ce_bwd(const float* logits, int R, int V, long ldv, const int32_t* targets, const int32_t* targets_host, float grad_scale,
                               void* dlogits, long ldd, float* row_loss, float* loss_sum, void* stream) {
  SSAK_REQUIRE(logits && targets && targets_host && dlogits, "dec_ce_bwd: null pointer");
  SSAK_REQUIRE(row_loss || !loss_sum, "dec_ce_bwd: loss_sum is the sum of row_loss, which is NULL");
  SSAK_REQUIRE(R > 0 && V > 0 && ldv >= V && ldd >= V, "dec_ce_bwd: bad shape R=%d V=%d ldv=%ld ldd=%ld", R, V, ldv, ldd);
  for (int r = 0; r < R; ++r) SSAK_REQUIRE(targets_host[r] < V, "dec_ce_bwd: target[%d] = %d outside [0, %d)", r, targets_host[r], V);
  const bool vec = aligned16(logits) && ldv % 4 == 0 && ((uintptr_t)dlogits & 7) == 0 && ldd % 4 == 0;
  const hipStream_t st = (hipStream_t)stream;
  if (vec) ce_bwd_kernel<true><<<R, CE_THREADS, 0, st>>>(logits, ldv, V, targets, grad_scale, (bf16*)dlogits, ldd, row_loss);
  else ce_bwd_kernel<false><<<R, CE_THREADS, 0, st>>>(logits, ldv, V, targets, grad_scale, (bf16*)dlogits, ldd, row_loss);
  SSAK_LAUNCH_CHECK();
  if (loss_sum) {
    ce_loss_sum_kernel<<<1, CE_THREADS, 0, st>>>(row_loss, R, loss_sum);
    SSAK_LAUNCH_CHECK();
  }
  return SSAK_OK;
}

extern "C" int ssak_dec_embed_bwd(const void* dh, int B, int L, int D, int Vp, int max_positions, int pos_offset, const int32_t* uniq,
                                  const int32_t* offsets, const int32_t* rows, const int32_t* uniq_host, const int32_t* offsets_host,
                                  const int32_t* rows_host, int n_unique, float* d_embed_tokens, float* d_embed_positions, void* stream) {
  SSAK_REQUIRE(dh && uniq && offsets && rows && uniq_host && offsets_host && rows_host && d_embed_tokens && d_embed_positions,
               "dec_embed_bwd: null pointer");
  SSAK_REQUIRE(B > 0 && L > 0 && D > 0 && Vp > 0 && max_positions > 0 && (long)B * L <= INT_MAX, "dec_embed_bwd: bad shape B=%d L=%d D=%d Vp=%d max_positions=%d",
               B, L, D, Vp, max_positions);
  SSAK_REQUIRE(pos_offset >= 0 && (long)pos_offset + L <= max_positions, "dec_embed_bwd: positions [%d, %ld) overrun the table of %d", pos_offset,
               (long)pos_offset + L, max_positions);
  const int N = B * L;
  SSAK_REQUIRE(n_unique > 0 && n_unique <= N, "dec_embed_bwd: n_unique=%d outside [1, %d]", n_unique, N);
  SSAK_REQUIRE(offsets_host[0] == 0 && offsets_host[n_unique] == N, "dec_embed_bwd: offsets must run from 0 to B * L = %d", N);
  std::vector<char> seen((size_t)N, 0);
  for (int u = 0; u < n_unique; ++u) {
    SSAK_REQUIRE(uniq_host[u] >= 0 && uniq_host[u] < Vp && (u == 0 || uniq_host[u] > uniq_host[u - 1]),
                 "dec_embed_bwd: uniq[%d] = %d outside [0, %d) or not ascending", u, uniq_host[u], Vp);
    SSAK_REQUIRE(offsets_host[u + 1] > offsets_host[u] && offsets_host[u + 1] <= N, "dec_embed_bwd: offsets[%d] = %d is not ascending", u + 1, offsets_host[u + 1]);
    for (int j = offsets_host[u]; j < offsets_host[u + 1]; ++j) {
      const int r = rows_host[j];
      SSAK_REQUIRE(r >= 0 && r < N && !seen[r] && (j == offsets_host[u] || r > rows_host[j - 1]),
                   "dec_embed_bwd: rows[%d] = %d outside [0, %d), repeated or not ascending within its token", j, r, N);
      seen[r] = 1;
    }
  }
  const hipStream_t st = (hipStream_t)stream;
  embed_bwd_tokens_kernel<<<n_unique, 256, 0, st>>>((const bf16*)dh, N, D, Vp, uniq, offsets, rows, d_embed_tokens);
  SSAK_LAUNCH_CHECK();
  embed_bwd_positions_kernel<<<L, 256, 0, st>>>((const bf16*)dh, B, L, D, pos_offset, d_embed_positions);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

// ---- the LayerNorm row kernels as product entries: the templates the engine and the ssak_debug_layernorm_* entries call, without
// dropout sites
extern "C" int ssak_layernorm_fwd_stats(const void* y, const void* res, const float* gamma, const float* beta, void* r_out, void* out, float* mean,
                                        float* rstd, int M, int C, float eps, int dtype, void* stream) {
  SSAK_REQUIRE(dtype == 0 || dtype == 1, "layernorm_fwd_stats: dtype %d (0 bf16, 1 fp32)", dtype);
  SSAK_REQUIRE(M > 0 && C > 0 && (C & 7) == 0 && C <= 1536, "layernorm_fwd_stats: M=%d C=%d (C a multiple of 8, <= 1536)", M, C);
  SSAK_REQUIRE(y || res, "layernorm_fwd_stats: neither y nor res");
  SSAK_REQUIRE(out && gamma && beta && mean && rstd, "layernorm_fwd_stats: out, gamma, beta, mean and rstd are required");
  const DropSpec none;
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    return k_layernorm_fwd_t<bf16>((const bf16*)y, (const bf16*)res, gamma, beta, (bf16*)r_out, (bf16*)out, mean, rstd, M, C, eps, none, none, st);
  return k_layernorm_fwd_t<float>((const float*)y, (const float*)res, gamma, beta, (float*)r_out, (float*)out, mean, rstd, M, C, eps, none, none, st);
}

extern "C" size_t ssak_layernorm_bwd_workspace_bytes(int C) { return C > 0 ? (size_t)LN_BWD_BLOCKS * 3 * C * sizeof(float) : 0; }

extern "C" int ssak_layernorm_bwd(const void* g1, const void* g2, const void* r, const float* mean, const float* rstd, const float* gamma,
                                  const void* g_res, void* dr, float* dgamma, float* dbeta, int M, int C, int dtype, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  SSAK_REQUIRE(dtype == 0 || dtype == 1, "layernorm_bwd: dtype %d (0 bf16, 1 fp32)", dtype);
  SSAK_REQUIRE(M > 0 && C > 0 && (C & 7) == 0 && C <= 1536, "layernorm_bwd: M=%d C=%d (C a multiple of 8, <= 1536)", M, C);
  SSAK_REQUIRE(g1 && r && mean && rstd && gamma && dr && dgamma && dbeta, "layernorm_bwd: null operand");
  SSAK_REQUIRE(workspace && workspace_bytes >= ssak_layernorm_bwd_workspace_bytes(C), "layernorm_bwd: workspace too small");
  const DropSpec none;
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    return k_layernorm_bwd_t<bf16>((const bf16*)g1, (const bf16*)g2, (const bf16*)r, mean, rstd, gamma, (const bf16*)g_res, (bf16*)dr, nullptr,
                                   dgamma, dbeta, (float*)workspace, M, C, none, none, st);
  return k_layernorm_bwd_t<float>((const float*)g1, (const float*)g2, (const float*)r, mean, rstd, gamma, (const float*)g_res, (float*)dr, nullptr,
                                  dgamma, dbeta, (float*)workspace, M, C, none, none, st);
}
