// The closing row kernel of a stable-LN encoder layer that carries an MMS language adapter (transformers
// modeling_wav2vec2.py: Wav2Vec2AttnAdapterLayer :930-952, applied after the feed-forward residual :644-647).  gfx950.
//
//   r2  = res + y                                           (fp32, never stored)
//   r2' = r2 + W2 relu(W1 LN_a(r2) + b1) + b2               LN_a: the adapter's own gamma / beta, eps_a (HF: 1e-5)
//   out = LN_next(r2')                                      the next layer's LayerNorm (or the encoder's), eps_n
//
// One launch per layer.  A workgroup of 8 waves owns 16 rows, the M of one MFMA tile:
//   1. row phase: a wave reads its 2 rows (16-byte chunks, one wave per row as in norm_act.hip), LayerNorm statistics in fp32,
//      and writes LN_a(r2) into an LDS image [16][H + pad] in the storage type; r2 stays in registers;
//   2. down-projection t [16, A] = LN_a(r2) W1^T: K = H is dealt over the 8 waves in steps of 32, each wave reads its W1
//      fragments (16 bytes per lane, straight from the [A, H] matrix) exactly once per workgroup; the 8 partial tiles are
//      summed through LDS, + b1, ReLU, rounded to bf16 into a [16][32] image whose columns A .. 31 are zero (the instruction's
//      K is 32, the adapter's is 16);
//   3. up-projection d [16, H] = t W2^T: the 16-column tiles of H are dealt over the waves, W2 fragments again read once per
//      workgroup; d goes to LDS as fp32 over the image of phase 1 (dead by then);
//   4. row phase: r2' = r2 + d + b2, rounded to the storage type and stored (the value the next LayerNorm sees), then the
//      next LayerNorm of the stored r2' as k_layernorm_fwd_t does it.
// T = float (the fp32-exact mode): the same four phases with both products as fp32 FMA chains, nothing rounded below fp32.
// Traffic per row: 2 reads + 2 writes of H elements, the class of bytes the plain closing LayerNorm launch moves; the
// products are 4 H A flops per row, ~10 flop / byte at A = 16: HBM-bound.
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int AA_ROWS = 16;                 // rows of a workgroup = M of mfma_f32_16x16x32_bf16
constexpr int AA_WAVES = 8;                 // 2 rows per wave in the row phases
constexpr int AA_THREADS = 64 * AA_WAVES;
constexpr int AA_A = 16;                    // adapter_attn_dim the kernel is built for (MMS)
constexpr int AA_RPW = AA_ROWS / AA_WAVES;

template <typename T>
struct AaParams {
  const T* y;        // [M,H] feed-forward output (may be null: r2 = res)
  const T* res;      // [M,H] residual stream before the feed-forward (or r2 itself)
  const float* ga;   // adapter LayerNorm
  const float* ba;
  const T* w1;       // [A,H]  linear_1.weight
  const float* b1;   // [A]
  const T* w2;       // [H,A]  linear_2.weight
  const float* b2;   // [H]
  const float* gn;   // the LayerNorm that follows the layer
  const float* bn;
  T* r_out;          // [M,H] r2' (may alias res or y)
  T* out;            // [M,H] LN_next(r2')
  float* mean;       // [M] statistics of LN_next (both or neither)
  float* rstd;
  int M, H;
  float eps_a, eps_n;
};

inline size_t aa_lds_bytes(int H) {
  // [16][H + 4] fp32 (the LN_a image of phase 1, then d of phase 3) | partial tiles [8][16][16] fp32 | t [16][32] bf16 / [16][16] fp32
  return (size_t)AA_ROWS * (H + 4) * sizeof(float) + (size_t)AA_WAVES * AA_ROWS * AA_A * sizeof(float) + AA_ROWS * 32 * sizeof(bf16);
}

template <typename T, int NCH>
__global__ __launch_bounds__(AA_THREADS) void attn_adapter_fwd_kernel(const AaParams<T> p) {
  constexpr bool BF = std::is_same<T, bf16>::value;
  extern __shared__ __attribute__((aligned(16))) unsigned char aa_smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = p.H, nch = H >> 3;
  const int row0 = blockIdx.x * AA_ROWS;
  const int dp = H + 4;                       // fp32 pitch of d (and of the fp32 LN_a image)
  const int xp = BF ? H + 8 : H + 4;          // pitch of the LN_a image in elements of T
  float* const D = reinterpret_cast<float*>(aa_smem);
  T* const Xn = reinterpret_cast<T*>(aa_smem);
  float* const red = reinterpret_cast<float*>(aa_smem + (size_t)AA_ROWS * dp * sizeof(float));
  unsigned char* const tt = reinterpret_cast<unsigned char*>(red + AA_WAVES * AA_ROWS * AA_A);
  const float inv_h = 1.f / (float)H;

  // ---- 1. r2 = res + y, LN_a(r2) -> LDS
  float v[AA_RPW][NCH][8];
#pragma unroll
  for (int rr = 0; rr < AA_RPW; ++rr) {
    const int lrow = w * AA_RPW + rr, row = row0 + lrow;
    const bool valid = row < p.M;  // (wave-uniform)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = lane + 64 * i;
#pragma unroll
      for (int k = 0; k < 8; ++k) v[rr][i][k] = 0.f;
      if (valid && ch < nch) {
        const size_t o = (size_t)row * H + ch * 8;
        chunk_to_f(ld8<T>(p.res + o), v[rr][i]);
        if (p.y) {
          float t[8];
          chunk_to_f(ld8<T>(p.y + o), t);
#pragma unroll
          for (int k = 0; k < 8; ++k) v[rr][i][k] += t[k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[rr][i][k];
      }
    }
    const float mean = wave_sum(s) * inv_h;
    float q2 = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (lane + 64 * i < nch) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d = v[rr][i][k] - mean;
          q2 += d * d;
        }
      }
    const float rstd = rsqrtf(wave_sum(q2) * inv_h + p.eps_a);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = lane + 64 * i;
      if (ch < nch) {
        float g[8], b[8], n[8];
        *reinterpret_cast<float4*>(g) = *reinterpret_cast<const float4*>(p.ga + ch * 8);
        *reinterpret_cast<float4*>(g + 4) = *reinterpret_cast<const float4*>(p.ga + ch * 8 + 4);
        *reinterpret_cast<float4*>(b) = *reinterpret_cast<const float4*>(p.ba + ch * 8);
        *reinterpret_cast<float4*>(b + 4) = *reinterpret_cast<const float4*>(p.ba + ch * 8 + 4);
#pragma unroll
        for (int k = 0; k < 8; ++k) n[k] = valid ? (v[rr][i][k] - mean) * rstd * g[k] + b[k] : 0.f;  // rows past M: zeros
        st8<T>(Xn + (size_t)lrow * xp + ch * 8, f_to_chunk8<T>(n));
      }
    }
  }
  __syncthreads();

  // ---- 2. t = relu(LN_a(r2) W1^T + b1)   [16, A]
  if constexpr (BF) {
    const int lr = lane & 15, lq = lane >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 32 * w; k0 < H; k0 += 32 * AA_WAVES) {
      const int kk = k0 + 8 * lq;
      bf16x8 fa = {0, 0, 0, 0, 0, 0, 0, 0}, fb = {0, 0, 0, 0, 0, 0, 0, 0};
      if (kk < H) {  // (H is a multiple of 8: a lane's 8 k are inside or outside together)
        fa = *reinterpret_cast<const bf16x8*>(Xn + (size_t)lr * xp + kk);        // A[row lr][k]
        fb = *reinterpret_cast<const bf16x8*>(p.w1 + (size_t)lr * H + kk);       // B[k][col lr] = W1[lr][k]
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(w * AA_ROWS + lq * 4 + r) * AA_A + lr] = acc[r];  // D[row 4 lq + r][col lr]
    __syncthreads();
    bf16* const Tt = reinterpret_cast<bf16*>(tt);
    if (tid < AA_ROWS * AA_A) {
      const int a = tid & 15, row = tid >> 4;
      float t = p.b1[a];
#pragma unroll
      for (int ww = 0; ww < AA_WAVES; ++ww) t += red[(ww * AA_ROWS + row) * AA_A + a];
      Tt[row * 32 + a] = (bf16)fmaxf(t, 0.f);
      Tt[row * 32 + 16 + a] = (bf16)0.f;  // K of the instruction is 32: the upper half multiplies zeros
    }
    __syncthreads();
    // ---- 3. d = t W2^T   [16, H] fp32 -> LDS (over the LN_a image: every read of it is behind the two barriers above)
    const bf16x8 ft = *reinterpret_cast<const bf16x8*>(Tt + lr * 32 + 8 * lq);  // A[row lr][k = 8 lq + j]
    for (int h0 = 16 * w; h0 < H; h0 += 16 * AA_WAVES) {
      const int col = h0 + lr;
      bf16x8 fb = {0, 0, 0, 0, 0, 0, 0, 0};
      if (lq < 2 && col < H) fb = *reinterpret_cast<const bf16x8*>(p.w2 + (size_t)col * AA_A + 8 * lq);  // B[k][col] = W2[col][k]
      f32x4 d = {0.f, 0.f, 0.f, 0.f};
      d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ft, fb, d, 0, 0, 0);
      if (col < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) D[(size_t)(lq * 4 + r) * dp + col] = d[r];
      }
    }
  } else {
    // fp32-exact mode: FMA chains.  Thread -> (row, a) and one half of K; the halves meet in LDS.
    const int o = tid & 255, a = o & 15, row = o >> 4, half = tid >> 8;
    const int ksplit = (nch >> 1) * 8, lo = half ? ksplit : 0, hi = half ? H : ksplit;
    float t = 0.f;
    for (int k = lo; k < hi; k += 4) {
      const float4 x = *reinterpret_cast<const float4*>(Xn + (size_t)row * xp + k);
      const float4 ww = *reinterpret_cast<const float4*>(p.w1 + (size_t)a * H + k);
      t = fmaf(x.x, ww.x, t);
      t = fmaf(x.y, ww.y, t);
      t = fmaf(x.z, ww.z, t);
      t = fmaf(x.w, ww.w, t);
    }
    red[half * 256 + o] = t;
    __syncthreads();
    float* const Tt = reinterpret_cast<float*>(tt);
    if (tid < 256) Tt[o] = fmaxf(red[o] + red[256 + o] + p.b1[a], 0.f);
    __syncthreads();
    for (int idx = tid; idx < AA_ROWS * H; idx += AA_THREADS) {
      const int r = idx / H, h = idx - r * H;
      float d = 0.f;
#pragma unroll
      for (int a4 = 0; a4 < AA_A; a4 += 4) {
        const float4 tv = *reinterpret_cast<const float4*>(Tt + r * AA_A + a4);
        const float4 ww = *reinterpret_cast<const float4*>(p.w2 + (size_t)h * AA_A + a4);
        d = fmaf(tv.x, ww.x, d);
        d = fmaf(tv.y, ww.y, d);
        d = fmaf(tv.z, ww.z, d);
        d = fmaf(tv.w, ww.w, d);
      }
      D[(size_t)r * dp + h] = d;
    }
  }
  __syncthreads();

  // ---- 4. r2' = r2 + d + b2 (stored), out = LN_next(r2')
#pragma unroll
  for (int rr = 0; rr < AA_RPW; ++rr) {
    const int lrow = w * AA_RPW + rr, row = row0 + lrow;
    if (row >= p.M) continue;  // (wave-uniform; no barrier follows)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = lane + 64 * i;
      if (ch < nch) {
        float d[8], b[8];
        *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(D + (size_t)lrow * dp + ch * 8);
        *reinterpret_cast<float4*>(d + 4) = *reinterpret_cast<const float4*>(D + (size_t)lrow * dp + ch * 8 + 4);
        *reinterpret_cast<float4*>(b) = *reinterpret_cast<const float4*>(p.b2 + ch * 8);
        *reinterpret_cast<float4*>(b + 4) = *reinterpret_cast<const float4*>(p.b2 + ch * 8 + 4);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[rr][i][k] += d[k] + b[k];
        // round through the storage type: the LayerNorm below (and whatever reads r2' later) sees the stored values
        const Chunk8<T> q = f_to_chunk8<T>(v[rr][i]);
        st8<T>(p.r_out + (size_t)row * H + ch * 8, q);
        chunk_to_f(q, v[rr][i]);
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[rr][i][k];
      }
    }
    const float mean = wave_sum(s) * inv_h;
    float q2 = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (lane + 64 * i < nch) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d = v[rr][i][k] - mean;
          q2 += d * d;
        }
      }
    const float rstd = rsqrtf(wave_sum(q2) * inv_h + p.eps_n);
    if (lane == 0 && p.mean) {
      p.mean[row] = mean;
      p.rstd[row] = rstd;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = lane + 64 * i;
      if (ch < nch) {
        float g[8], b[8], o8[8];
        *reinterpret_cast<float4*>(g) = *reinterpret_cast<const float4*>(p.gn + ch * 8);
        *reinterpret_cast<float4*>(g + 4) = *reinterpret_cast<const float4*>(p.gn + ch * 8 + 4);
        *reinterpret_cast<float4*>(b) = *reinterpret_cast<const float4*>(p.bn + ch * 8);
        *reinterpret_cast<float4*>(b + 4) = *reinterpret_cast<const float4*>(p.bn + ch * 8 + 4);
#pragma unroll
        for (int k = 0; k < 8; ++k) o8[k] = (v[rr][i][k] - mean) * rstd * g[k] + b[k];
        st8<T>(p.out + (size_t)row * H + ch * 8, f_to_chunk8<T>(o8));
      }
    }
  }
}

template <typename T, int NCH>
int aa_launch(const AaParams<T>& p, hipStream_t st) {
  const size_t lds = aa_lds_bytes(p.H);
  static bool attr_done = false;
  if (!attr_done) {
    SSAK_HIP(hipFuncSetAttribute((const void*)attn_adapter_fwd_kernel<T, NCH>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_done = true;
  }
  attn_adapter_fwd_kernel<T, NCH><<<ssak_cdiv(p.M, AA_ROWS), AA_THREADS, lds, st>>>(p);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

}  // namespace

bool k_attn_adapter_supported(int H, int A) { return A == AA_A && H > 0 && (H & 7) == 0 && H <= 1536; }

template <typename T>
int k_attn_adapter_fwd_t(const T* y, const T* res, const float* ln_g, const float* ln_b, const T* w1, const float* b1, const T* w2,
                         const float* b2, const float* next_g, const float* next_b, T* r_out, T* out, float* mean, float* rstd, int M,
                         int H, int A, float eps_adapter, float eps_next, hipStream_t st) {
  SSAK_REQUIRE(A == AA_A, "attn_adapter: adapter_attn_dim %d (supported: 16)", A);
  SSAK_REQUIRE(M > 0 && H > 0 && (H & 7) == 0 && H <= 1536, "attn_adapter: M=%d H=%d (H a multiple of 8, <= 1536)", M, H);
  SSAK_REQUIRE(res && ln_g && ln_b && w1 && b1 && w2 && b2 && next_g && next_b && r_out && out, "attn_adapter: null operand");
  SSAK_REQUIRE(!mean == !rstd, "attn_adapter: mean and rstd go together");
  const AaParams<T> p{y, res, ln_g, ln_b, w1, b1, w2, b2, next_g, next_b, r_out, out, mean, rstd, M, H, eps_adapter, eps_next};
  const int nch = ssak_cdiv(H / 8, 64);
  if (nch == 1) return aa_launch<T, 1>(p, st);
  if (nch == 2) return aa_launch<T, 2>(p, st);
  return aa_launch<T, 3>(p, st);
}
template int k_attn_adapter_fwd_t<bf16>(const bf16*, const bf16*, const float*, const float*, const bf16*, const float*, const bf16*,
                                        const float*, const float*, const float*, bf16*, bf16*, float*, float*, int, int, int, float,
                                        float, hipStream_t);
template int k_attn_adapter_fwd_t<float>(const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                                         const float*, const float*, const float*, float*, float*, float*, float*, int, int, int, float,
                                         float, hipStream_t);

// ---- test-only: one launch into the caller's buffers (tests/test_gpu_mms.py holds it to tests/attn_adapter_ref.py).
// dtype 0 = bf16 (activations and W1 / W2 bf16), 1 = fp32 (everything float).  Nothing on the hot path calls this.
extern "C" int ssak_test_attn_adapter_fwd(const void* y, const void* res, const float* ln_g, const float* ln_b, const void* w1,
                                          const float* b1, const void* w2, const float* b2, const float* next_g, const float* next_b,
                                          void* r_out, void* out, float* mean, float* rstd, int M, int H, int A, float eps_adapter,
                                          float eps_next, int dtype, void* stream) {
  SSAK_REQUIRE(dtype == 0 || dtype == 1, "test_attn_adapter_fwd: dtype %d (0 bf16, 1 fp32)", dtype);
  if (dtype == 0)
    return k_attn_adapter_fwd_t<bf16>((const bf16*)y, (const bf16*)res, ln_g, ln_b, (const bf16*)w1, b1, (const bf16*)w2, b2, next_g,
                                      next_b, (bf16*)r_out, (bf16*)out, mean, rstd, M, H, A, eps_adapter, eps_next, (hipStream_t)stream);
  return k_attn_adapter_fwd_t<float>((const float*)y, (const float*)res, ln_g, ln_b, (const float*)w1, b1, (const float*)w2, b2, next_g,
                                     next_b, (float*)r_out, (float*)out, mean, rstd, M, H, A, eps_adapter, eps_next, (hipStream_t)stream);
}
