// Whisper LoRA fine-tuning: the adapter's own arithmetic around the decoder's frozen q_proj / v_proj products (the reference's
// PEFT recipe, ssak/train/transformers/whisper_train.py:374-429).  x [M, D_in] bf16, A [r, D_in] and B [D_out, r] (bf16 shadows of
// fp32 masters), s = lora_alpha / r, keep = the dropout site's bits at (row, col) of x (common.h keep_bit; scale 1 / (1 - p)).
// bf16 storage, fp32 accumulation, no atomics: every sum has a fixed order and two runs give the same bits.
//
// Every kernel is one wave per workgroup on one 16-row tile and streams its [M, D] operand once; A and B (49 KB each at whisper-small,
// r = 32) are read through the cache by every wave.  The products are 16x16x32 bf16 MFMAs in their transposed form, so that a lane
// ends up with four ADJACENT columns of one row (8-byte stores) and the [16, r] intermediate goes from the first product's result
// layout to the second product's operand layout through a 2 KB LDS image.
//   lora_fwd_kernel        t^T = A xd^T (A's and x's rows are the operands as they sit in memory), t = bf16(scale * .) -> LDS and
//                          memory; then y^T += s B t^T per 16 output columns (B's rows are the operand as they sit in memory).
//   lora_bwd_input_kernel  dt^T = B^T dy^T (B^T gathered: eight 2-byte loads per operand), dt = bf16(s * .); then per 16 input
//                          columns dx^T (+)= keep (A^T dt^T) scale (A^T gathered).
//   lora_bwd_weights_kernel  grid (64-column tiles of dB then of dA, LR_PART_ROWS-row ranges): dB = dy^T t and dA = dt^T xd contract
//                          over the rows, so both operands are gathered (2-byte loads down a column); a wave walks its row range
//                          32 rows at a time and writes its fp32 partial; lora_bwd_weights_sum_kernel adds the partials ascending.
//   lora_merge_kernel      one thread per element of W, fp32 FMAs in ascending r.
#include "kernels.h"

SSAK_DEFINE_DROP_TABLE

namespace {
constexpr int LR_ROWS = 16;          // rows of x / y / dy per workgroup (one wave)
constexpr int LR_MAX_R = 64;
constexpr int LR_MAX_D = 1280;       // Whisper large's d_model
constexpr int LR_MERGE_MAX_D = 5120; // its feed-forward width (the merge also serves fc1 / fc2 of a loaded adapter)
constexpr int LR_PART_ROWS = 512;    // rows per first-stage partial of the weight gradients
constexpr int LR_TP = LR_MAX_R + 8;  // bf16 pitch of the [16, r] image (144-byte rows: aligned 16-byte reads)

struct LoraDrop {
  uint64_t seed;
  uint32_t site, thi;  // thi = thresh16 << 16; 0: no mask
  float scale;
};

uint32_t lora_thresh(float p) { return p <= 0.f ? 0u : (uint32_t)fminf(65535.f, roundf(p * 65536.f)); }  // norm_act.hip thresh_of
LoraDrop lora_drop(uint64_t seed, uint32_t site, float p) {
  const uint32_t th = lora_thresh(p);
  return LoraDrop{seed, site, th << 16, th ? 1.f / (1.f - (float)th / 65536.f) : 1.f};
}

__device__ __forceinline__ bf16x8 lr_ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ bf16x8 lr_zero8() {
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (bf16)0.f;
  return z;
}
// keep (.) x on the eight columns c0 .. c0 + 7 (c0 a multiple of 8) of the row whose key is rk
__device__ __forceinline__ bf16x8 lr_mask8(bf16x8 x, uint32_t rk, int c0, uint32_t thi) {
  const uint4 m0 = *reinterpret_cast<const uint4*>(&g_drop_colmul.v[c0]);
  const uint4 m1 = *reinterpret_cast<const uint4*>(&g_drop_colmul.v[c0 + 4]);
  const uint32_t cm[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (!drop_keep(rk, cm[j], thi)) x[j] = (bf16)0.f;
  return x;
}
// the [16, r] image as the second product's B operand: lane (lr, g) holds row lr, columns 32 ks + 8 g .. + 7 (zero past 16 RT)
template <int RT>
__device__ __forceinline__ void lr_image_operand(const bf16 (*tl)[LR_TP], int lr, int g, bf16x8 (&tb)[(RT + 1) / 2]) {
#pragma unroll
  for (int ks = 0; ks < (RT + 1) / 2; ++ks) {
    const int k = 32 * ks + 8 * g;
    tb[ks] = k < 16 * RT ? *reinterpret_cast<const bf16x8*>(&tl[lr][k]) : lr_zero8();
  }
}

struct LoraFwdParams {
  const bf16 *x, *A, *B;
  bf16 *y, *t;
  long ldx, ldy;
  int M, Din, Dout, r;
  float s;
  LoraDrop d;
};

// RT = the 16-wide tiles of r (r = 8 runs as 16 with A's rows 8 .. 15 read as zeros)
template <int RT>
__global__ __launch_bounds__(64) void lora_fwd_kernel(const LoraFwdParams p) {
  __shared__ __attribute__((aligned(16))) bf16 tl[LR_ROWS][LR_TP];
  const int lane = threadIdx.x, lr = lane & 15, g = lane >> 4;
  const long m = (long)blockIdx.x * LR_ROWS + lr;
  const bool live = m < p.M;
  const uint32_t rk = p.d.thi ? drop_rowkey(p.d.seed, p.d.site, (uint64_t)m) : 0u;
  f32x4 acc[RT];
#pragma unroll
  for (int jt = 0; jt < RT; ++jt) acc[jt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < p.Din; k0 += 32) {
    bf16x8 xb = lr_zero8();
    if (live) {
      xb = lr_ld8(p.x + m * p.ldx + k0 + 8 * g);
      if (p.d.thi) xb = lr_mask8(xb, rk, k0 + 8 * g, p.d.thi);
    }
#pragma unroll
    for (int jt = 0; jt < RT; ++jt) {
      const int j = 16 * jt + lr;
      bf16x8 a = lr_zero8();
      if (j < p.r) a = lr_ld8(p.A + (long)j * p.Din + k0 + 8 * g);
      acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xb, acc[jt], 0, 0, 0);  // acc[jt][i]: (row lr, j = 16 jt + 4 g + i)
    }
  }
#pragma unroll
  for (int jt = 0; jt < RT; ++jt) {
    bf16x4 tv;
#pragma unroll
    for (int i = 0; i < 4; ++i) tv[i] = (bf16)(acc[jt][i] * p.d.scale);
    const int j0 = 16 * jt + 4 * g;
    *reinterpret_cast<bf16x4*>(&tl[lr][j0]) = tv;
    if (live && p.t && j0 < p.r) *reinterpret_cast<bf16x4*>(p.t + m * p.r + j0) = tv;
  }
  __syncthreads();
  bf16x8 tb[(RT + 1) / 2];
  lr_image_operand<RT>(tl, lr, g, tb);
  for (int n0 = 0; n0 < p.Dout; n0 += 16) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < (RT + 1) / 2; ++ks) {
      const int k = 32 * ks + 8 * g;
      bf16x8 b = lr_zero8();
      if (k < p.r) b = lr_ld8(p.B + (long)(n0 + lr) * p.r + k);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, tb[ks], c, 0, 0, 0);  // c[i]: (column n0 + 4 g + i, row lr)
    }
    if (live) {
      bf16* yp = p.y + m * p.ldy + n0 + 4 * g;
      bf16x4 v = *reinterpret_cast<const bf16x4*>(yp);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (bf16)((float)v[i] + p.s * c[i]);
      *reinterpret_cast<bf16x4*>(yp) = v;
    }
  }
}

struct LoraBwdInParams {
  const bf16 *dy, *A, *B;
  bf16 *dt, *dx;
  long lddy, lddx;
  int M, Din, Dout, r, accumulate;
  float s;
  LoraDrop d;
};

template <int RT>
__global__ __launch_bounds__(64) void lora_bwd_input_kernel(const LoraBwdInParams p) {
  __shared__ __attribute__((aligned(16))) bf16 tl[LR_ROWS][LR_TP];
  const int lane = threadIdx.x, lr = lane & 15, g = lane >> 4;
  const long m = (long)blockIdx.x * LR_ROWS + lr;
  const bool live = m < p.M;
  f32x4 acc[RT];
#pragma unroll
  for (int jt = 0; jt < RT; ++jt) acc[jt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // dt^T = B^T dy^T: the A operand is B^T, gathered (lane: j = 16 jt + lr, output columns k0 + 8 g + e)
  for (int k0 = 0; k0 < p.Dout; k0 += 32) {
    bf16x8 db = lr_zero8();
    if (live) db = lr_ld8(p.dy + m * p.lddy + k0 + 8 * g);
#pragma unroll
    for (int jt = 0; jt < RT; ++jt) {
      const int j = 16 * jt + lr;
      bf16x8 a = lr_zero8();
      if (j < p.r) {
        const bf16* bp = p.B + (long)(k0 + 8 * g) * p.r + j;
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = bp[(long)e * p.r];
      }
      acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, db, acc[jt], 0, 0, 0);  // acc[jt][i]: (row lr, j = 16 jt + 4 g + i)
    }
  }
#pragma unroll
  for (int jt = 0; jt < RT; ++jt) {
    bf16x4 tv;
#pragma unroll
    for (int i = 0; i < 4; ++i) tv[i] = (bf16)(acc[jt][i] * p.s);
    const int j0 = 16 * jt + 4 * g;
    *reinterpret_cast<bf16x4*>(&tl[lr][j0]) = tv;
    if (live && j0 < p.r) *reinterpret_cast<bf16x4*>(p.dt + m * p.r + j0) = tv;
  }
  if (!p.dx) return;  // (the whole grid: nothing upstream needs this gradient)
  __syncthreads();
  bf16x8 tb[(RT + 1) / 2];
  lr_image_operand<RT>(tl, lr, g, tb);
  const uint32_t rk = p.d.thi ? drop_rowkey(p.d.seed, p.d.site, (uint64_t)m) : 0u;
  // dx^T = A^T dt^T per 16 input columns: the A operand is A^T, gathered (lane: column c0 + lr, j = 32 ks + 8 g + e)
  for (int c0 = 0; c0 < p.Din; c0 += 16) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < (RT + 1) / 2; ++ks) {
      const int j0 = 32 * ks + 8 * g;
      bf16x8 a = lr_zero8();
      if (j0 < p.r) {
        const bf16* ap = p.A + (long)j0 * p.Din + c0 + lr;
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = ap[(long)e * p.Din];
      }
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, tb[ks], c, 0, 0, 0);  // c[i]: (column c0 + 4 g + i, row lr)
    }
    if (live) {
      const int col = c0 + 4 * g;
      bf16* xp = p.dx + m * p.lddx + col;
      float v[4] = {c[0] * p.d.scale, c[1] * p.d.scale, c[2] * p.d.scale, c[3] * p.d.scale};
      if (p.d.thi) {
        const uint4 cm4 = *reinterpret_cast<const uint4*>(&g_drop_colmul.v[col]);
        const uint32_t cm[4] = {cm4.x, cm4.y, cm4.z, cm4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (!drop_keep(rk, cm[i], p.d.thi)) v[i] = 0.f;
      }
      bf16x4 o;
      if (p.accumulate) {
        const bf16x4 old = *reinterpret_cast<const bf16x4*>(xp);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16)((float)old[i] + v[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16)v[i];
      }
      *reinterpret_cast<bf16x4*>(xp) = o;
    }
  }
}

struct LoraBwdWParams {
  const bf16 *dy, *t, *dt, *x;
  float* ws;
  long lddy, ldx;
  int M, Din, Dout, r;
  LoraDrop d;
};

// blockIdx.x: the 64-column tiles of dy (dB) and then of x (dA); blockIdx.y: the row range.  Partial layout per range:
// dB [D_out, r] then dA [r, D_in], unscaled.
template <int RT>
__global__ __launch_bounds__(64) void lora_bwd_weights_kernel(const LoraBwdWParams p) {
  const int lane = threadIdx.x, lr = lane & 15, g = lane >> 4;
  const int nb = p.Dout / 64;
  const bool is_b = (int)blockIdx.x < nb;
  const int col0 = 64 * (is_b ? (int)blockIdx.x : (int)blockIdx.x - nb);
  const long m_lo = (long)blockIdx.y * LR_PART_ROWS;
  const long m_hi = m_lo + LR_PART_ROWS < p.M ? m_lo + LR_PART_ROWS : (long)p.M;
  const bf16* const big = (is_b ? p.dy : p.x) + col0 + lr;
  const long ldb = is_b ? p.lddy : p.ldx;
  const bf16* const small = is_b ? p.t : p.dt;
  const bool masked = !is_b && p.d.thi;
  uint32_t cm[4] = {0u, 0u, 0u, 0u};
  if (masked) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) cm[ct] = g_drop_colmul.v[col0 + 16 * ct + lr];
  }
  f32x4 acc[4][RT];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int jt = 0; jt < RT; ++jt) acc[ct][jt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (long m0 = m_lo; m0 < m_hi; m0 += 32) {
    // the contraction runs over rows: lane (lr, g) holds rows m0 + 8 g + e of one column of each operand
    bf16x8 sm[RT], bg[4];
#pragma unroll
    for (int jt = 0; jt < RT; ++jt) sm[jt] = lr_zero8();
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) bg[ct] = lr_zero8();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const long row = m0 + 8 * g + e;
      if (row < m_hi) {
#pragma unroll
        for (int jt = 0; jt < RT; ++jt)
          if (16 * jt + lr < p.r) sm[jt][e] = small[row * p.r + 16 * jt + lr];
        const uint32_t rk = masked ? drop_rowkey(p.d.seed, p.d.site, (uint64_t)row) : 0u;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const bf16 v = big[row * ldb + 16 * ct];
          bg[ct][e] = (masked && !drop_keep(rk, cm[ct], p.d.thi)) ? (bf16)0.f : v;
        }
      }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int jt = 0; jt < RT; ++jt) {
        if (is_b)  // dB = dy^T t: acc[i] = (output column col0 + 16 ct + 4 g + i, j = 16 jt + lr)
          acc[ct][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bg[ct], sm[jt], acc[ct][jt], 0, 0, 0);
        else       // dA = dt^T xd: acc[i] = (j = 16 jt + 4 g + i, input column col0 + 16 ct + lr)
          acc[ct][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sm[jt], bg[ct], acc[ct][jt], 0, 0, 0);
      }
  }
  float* const part = p.ws + (long)blockIdx.y * p.r * (p.Dout + p.Din);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int jt = 0; jt < RT; ++jt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (is_b) {
          const int o = col0 + 16 * ct + 4 * g + i, j = 16 * jt + lr;
          if (j < p.r) part[(long)o * p.r + j] = acc[ct][jt][i];
        } else {
          const int j = 16 * jt + 4 * g + i, c = col0 + 16 * ct + lr;
          if (j < p.r) part[(long)p.Dout * p.r + (long)j * p.Din + c] = acc[ct][jt][i];
        }
      }
}

// dB = s * (the partials added in ascending range order), dA = scale * (the same)
__global__ void lora_bwd_weights_sum_kernel(const float* ws, int parts, long n_b, long n_a, float s, float scale, float* dB, float* dA) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_b + n_a) return;
  float sum = 0.f;
  for (int k = 0; k < parts; ++k) sum += ws[(long)k * (n_b + n_a) + i];
  if (i < n_b)
    dB[i] = s * sum;
  else
    dA[i - n_b] = scale * sum;
}

__global__ void lora_merge_kernel(const float* w, const float* A, const float* B, bf16* out, float* out_f32, int Din, int Dout, int r, float s) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)Din * Dout) return;
  const int o = (int)(i / Din), c = (int)(i % Din);
  float acc = 0.f;
  for (int j = 0; j < r; ++j) acc = fmaf(B[(long)o * r + j], A[(long)j * Din + c], acc);
  const float v = fmaf(s, acc, w[i]);
  out[i] = (bf16)v;
  if (out_f32) out_f32[i] = v;
}

bool lora_rank_ok(int r) { return r == 8 || r == 16 || r == 32 || r == 64; }
bool lora_dim_ok(int d, int cap) { return d >= 64 && d <= cap && d % 64 == 0; }
}  // namespace

#define LORA_SHAPE_CHECKS(what)                                                                                                      \
  SSAK_REQUIRE(lora_rank_ok(r), what ": r = %d, the ranks built are 8, 16, 32 and 64", r);                                           \
  SSAK_REQUIRE(lora_dim_ok(D_in, LR_MAX_D) && lora_dim_ok(D_out, LR_MAX_D),                                                          \
               what ": D_in = %d, D_out = %d: multiples of 64 up to %d are built", D_in, D_out, LR_MAX_D);                           \
  SSAK_REQUIRE(M >= 1, what ": M = %d rows", M);                                                                                     \
  SSAK_REQUIRE(drop_p >= 0.f && drop_p < 1.f, what ": drop_p = %g outside [0, 1)", (double)drop_p);                                  \
  SSAK_REQUIRE(!(drop_p > 0.f) || D_in <= DROP_TABLE_N, what ": dropout sites are built for at most %d columns", DROP_TABLE_N)

#define LORA_DISPATCH(kernel, grid, st, p)                         \
  do {                                                             \
    if (r <= 16)                                                   \
      kernel<1><<<grid, 64, 0, st>>>(p);                           \
    else if (r == 32)                                              \
      kernel<2><<<grid, 64, 0, st>>>(p);                           \
    else                                                           \
      kernel<4><<<grid, 64, 0, st>>>(p);                           \
  } while (0)

extern "C" int ssak_lora_fwd(const void* x, long ldx, const void* A, const void* B, void* y, long ldy, void* t, int M, int D_in, int D_out,
                             int r, float scaling, uint64_t seed, uint32_t site, float drop_p, void* stream) {
  SSAK_REQUIRE(x && A && B && y, "lora_fwd: null operand");
  LORA_SHAPE_CHECKS("lora_fwd");
  SSAK_REQUIRE(ldx >= D_in && ldy >= D_out && ldx % 8 == 0 && ldy % 8 == 0, "lora_fwd: row strides %ld / %ld for widths %d / %d (multiples of 8, at least the width)",
               ldx, ldy, D_in, D_out);
  SSAK_REQUIRE(aligned16(x) && aligned16(A) && aligned16(B) && aligned16(y) && aligned16(t), "lora_fwd: operands must be 16-byte aligned");
  LoraFwdParams p{(const bf16*)x, (const bf16*)A, (const bf16*)B, (bf16*)y, (bf16*)t, ldx, ldy, M, D_in, D_out, r, scaling, lora_drop(seed, site, drop_p)};
  LORA_DISPATCH(lora_fwd_kernel, ssak_cdiv(M, LR_ROWS), (hipStream_t)stream, p);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" int ssak_lora_bwd_input(const void* dy, long lddy, const void* A, const void* B, void* dt, void* dx, long lddx, int accumulate, int M,
                                   int D_in, int D_out, int r, float scaling, uint64_t seed, uint32_t site, float drop_p, void* stream) {
  SSAK_REQUIRE(dy && A && B && dt, "lora_bwd_input: null operand");
  LORA_SHAPE_CHECKS("lora_bwd_input");
  SSAK_REQUIRE(lddy >= D_out && lddy % 8 == 0 && (!dx || (lddx >= D_in && lddx % 8 == 0)),
               "lora_bwd_input: row strides %ld / %ld for widths %d / %d (multiples of 8, at least the width)", lddy, lddx, D_out, D_in);
  SSAK_REQUIRE(aligned16(dy) && aligned16(A) && aligned16(B) && aligned16(dt) && aligned16(dx), "lora_bwd_input: operands must be 16-byte aligned");
  LoraBwdInParams p{(const bf16*)dy, (const bf16*)A, (const bf16*)B, (bf16*)dt, (bf16*)dx, lddy, lddx, M, D_in, D_out, r, accumulate ? 1 : 0, scaling,
                    lora_drop(seed, site, drop_p)};
  LORA_DISPATCH(lora_bwd_input_kernel, ssak_cdiv(M, LR_ROWS), (hipStream_t)stream, p);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" size_t ssak_lora_bwd_weights_workspace_bytes(int M, int D_in, int D_out, int r) {
  if (M < 1 || D_in < 1 || D_out < 1 || r < 1) return 0;
  return (size_t)ssak_cdiv(M, LR_PART_ROWS) * (size_t)r * ((size_t)D_in + (size_t)D_out) * sizeof(float);
}

extern "C" int ssak_lora_bwd_weights(const void* dy, long lddy, const void* t, const void* dt, const void* x, long ldx, float* dB, float* dA, int M,
                                     int D_in, int D_out, int r, float scaling, uint64_t seed, uint32_t site, float drop_p, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  SSAK_REQUIRE(dy && t && dt && x && dB && dA && workspace, "lora_bwd_weights: null operand");
  LORA_SHAPE_CHECKS("lora_bwd_weights");
  SSAK_REQUIRE(lddy >= D_out && ldx >= D_in, "lora_bwd_weights: row strides %ld / %ld for widths %d / %d", lddy, ldx, D_out, D_in);
  SSAK_REQUIRE(workspace_bytes >= ssak_lora_bwd_weights_workspace_bytes(M, D_in, D_out, r) && aligned16(workspace),
               "lora_bwd_weights: workspace of %zu bytes, %zu needed (16-byte aligned)", workspace_bytes,
               ssak_lora_bwd_weights_workspace_bytes(M, D_in, D_out, r));
  const hipStream_t st = (hipStream_t)stream;
  const int parts = ssak_cdiv(M, LR_PART_ROWS);
  const LoraDrop d = lora_drop(seed, site, drop_p);
  LoraBwdWParams p{(const bf16*)dy, (const bf16*)t, (const bf16*)dt, (const bf16*)x, (float*)workspace, lddy, ldx, M, D_in, D_out, r, d};
  const dim3 grid((D_out + D_in) / 64, parts);
  LORA_DISPATCH(lora_bwd_weights_kernel, grid, st, p);
  SSAK_LAUNCH_CHECK();
  const long n_b = (long)D_out * r, n_a = (long)r * D_in;
  lora_bwd_weights_sum_kernel<<<ssak_cdiv(n_b + n_a, 256), 256, 0, st>>>((const float*)workspace, parts, n_b, n_a, scaling, d.scale, dB, dA);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" int ssak_lora_merge(const float* w_master, const float* A, const float* B, void* w_out, float* w_out_f32, int D_in, int D_out, int r,
                               float scaling, void* stream) {
  SSAK_REQUIRE(w_master && A && B && w_out, "lora_merge: null operand");
  SSAK_REQUIRE(lora_rank_ok(r), "lora_merge: r = %d, the ranks built are 8, 16, 32 and 64", r);
  SSAK_REQUIRE(lora_dim_ok(D_in, LR_MERGE_MAX_D) && lora_dim_ok(D_out, LR_MERGE_MAX_D), "lora_merge: D_in = %d, D_out = %d: multiples of 64 up to %d are built",
               D_in, D_out, LR_MERGE_MAX_D);
  lora_merge_kernel<<<ssak_cdiv((long)D_in * D_out, 256), 256, 0, (hipStream_t)stream>>>(w_master, A, B, (bf16*)w_out, w_out_f32, D_in, D_out, r, scaling);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}
