// Utterance classification on the encoder's last hidden state: pooling over time, the two-Linear head and softmax +
// cross-entropy, forward and backward -- what ssak/utils/gender.py's Wav2Vec2ForSpeechClassification / HubertForSpeechClassification
// run after the encoder (merged_strategy, the ClassificationHead, CrossEntropyLoss).  Host-side composition: ssak_amd/classify.py.
//
// Only the pooling passes touch a large tensor ([B, F, H]: 24 MB at 32 x 499 x 768 bf16); they stream it with 16-byte accesses.
// The head works on [B, H] with B small: its kernels stream the fp32 weights once per 8 utterances and never use the matrix cores.
// Every sum runs in a fixed order (per-thread partials in index order, then a fixed-order second stage in LDS): results are
// bit-reproducible, and there are no float atomics.
#include <limits.h>

#include <algorithm>

#include "kernels.h"

namespace {
// ---- pooling ---------------------------------------------------------------------------------------------------------
// One workgroup per (utterance, 128 columns): POOL_CW lanes side by side cover the columns with one 16-byte (bf16) chunk each,
// POOL_R groups of them take the frames r, r + POOL_R, ...; the POOL_R partial rows meet in LDS.
constexpr int POOL_CW = 16;
constexpr int POOL_R = 16;
constexpr int POOL_THREADS = POOL_CW * POOL_R;
constexpr int POOL_COLS = POOL_CW * 8;
static_assert(POOL_COLS <= POOL_THREADS, "the second stage takes one thread per column");

__device__ __forceinline__ int valid_frames(const int32_t* lens, int b, int F) {
  // the launcher has validated the host copy of the lengths; the clamp keeps a device copy that disagrees inside the tensor
  return lens ? min(max(lens[b], 0), F) : F;
}

template <typename T, int MODE>
__global__ __launch_bounds__(POOL_THREADS) void pool_fwd_kernel(const T* __restrict__ hidden, const int32_t* __restrict__ lens, int F,
                                                                int H, float* __restrict__ pooled, int32_t* __restrict__ argmax) {
  constexpr bool MAX = MODE == SSAK_POOL_MAX;
  __shared__ float red[POOL_R][POOL_COLS];
  __shared__ int32_t ired[MAX ? POOL_R : 1][POOL_COLS];
  const int b = blockIdx.y, cw = threadIdx.x % POOL_CW, r = threadIdx.x / POOL_CW;
  const int chunk = blockIdx.x * POOL_CW + cw;
  const int n = valid_frames(lens, b, F);
  float acc[8];
  int32_t idx[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    acc[e] = MAX ? -INFINITY : 0.f;
    idx[e] = INT_MAX;
  }
  auto take = [&](const float* v, int f) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if constexpr (MAX) {
        if (v[e] > acc[e]) {  // strict: within a thread's increasing frames the first maximum stays
          acc[e] = v[e];
          idx[e] = f;
        }
      } else {
        acc[e] += v[e];
      }
    }
  };
  if (chunk < (H >> 3)) {
    const T* p = hidden + (long)b * F * H + (long)chunk * 8;
    int f = r;
    for (; f + 3 * POOL_R < n; f += 4 * POOL_R) {  // four rows in flight per thread
      const Chunk8<T> c0 = ld8<T>(p + (long)f * H), c1 = ld8<T>(p + (long)(f + POOL_R) * H);
      const Chunk8<T> c2 = ld8<T>(p + (long)(f + 2 * POOL_R) * H), c3 = ld8<T>(p + (long)(f + 3 * POOL_R) * H);
      float v[8];
      chunk_to_f(c0, v);
      take(v, f);
      chunk_to_f(c1, v);
      take(v, f + POOL_R);
      chunk_to_f(c2, v);
      take(v, f + 2 * POOL_R);
      chunk_to_f(c3, v);
      take(v, f + 3 * POOL_R);
    }
    for (; f < n; f += POOL_R) {
      float v[8];
      chunk_to_f(ld8<T>(p + (long)f * H), v);
      take(v, f);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[r][cw * 8 + e] = acc[e];
    if constexpr (MAX) ired[r][cw * 8 + e] = idx[e];
  }
  __syncthreads();
  const int col = threadIdx.x, gcol = blockIdx.x * POOL_COLS + col;
  if (col < POOL_COLS && gcol < H) {
    float s = red[0][col];
    int32_t si = MAX ? ired[0][col] : 0;
    for (int q = 1; q < POOL_R; ++q) {
      const float v = red[q][col];
      if constexpr (MAX) {
        const int32_t vi = ired[q][col];
        if (v > s || (v == s && vi < si)) {  // the lowest frame that attains the maximum
          s = v;
          si = vi;
        }
      } else {
        s += v;
      }
    }
    if constexpr (MODE == SSAK_POOL_MEAN) s = n > 0 ? s / (float)n : 0.f;
    pooled[(long)b * H + gcol] = s;
    if constexpr (MAX) argmax[(long)b * H + gcol] = si == INT_MAX ? 0 : si;
  }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ dpooled, const int32_t* __restrict__ argmax,
                                                       const int32_t* __restrict__ lens, int B, int F, int H, T* __restrict__ dhidden) {
  const int nch = H >> 3;
  const long total = (long)B * F * nch;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % nch);
    const long bf = i / nch;
    const int f = (int)(bf % F), b = (int)(bf / F);
    const int n = valid_frames(lens, b, F);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (f < n) {
      const long o = (long)b * H + (long)ch * 8;
      const float4 g0 = *reinterpret_cast<const float4*>(dpooled + o), g1 = *reinterpret_cast<const float4*>(dpooled + o + 4);
      const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      if constexpr (MODE == SSAK_POOL_MAX) {
        const int4 a0 = *reinterpret_cast<const int4*>(argmax + o), a1 = *reinterpret_cast<const int4*>(argmax + o + 4);
        const int a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = a[e] == f ? g[e] : 0.f;
      } else if constexpr (MODE == SSAK_POOL_MEAN) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = g[e] / (float)n;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = g[e];
      }
    }
    st8<T>(dhidden + i * 8, f_to_chunk8<T>(v));
  }
}

// ---- the head's three products ------------------------------------------------------------------------------------------
// A dropout site of the head: keep(seed, site, row = utterance, col = feature) of common.h; thi = 0 turns it off.
struct HeadDrop {
  uint64_t seed;
  uint32_t site;
  uint32_t thi;  // thresh16 << 16
  float scale;
};
__device__ __forceinline__ float head_drop(float x, uint32_t rowkey, uint32_t colmul, const HeadDrop& d) {
  return drop_keep(rowkey, colmul, d.thi) ? x * d.scale : 0.f;
}

constexpr int HEAD_BT = 8;  // utterances per pass over a weight row

// out[b, j] = act(sum_k drop(in[b, k]) W[j, k] + bias[j]): one wave per output feature j streams its weight row once per
// HEAD_BT utterances; lanes take float4 slices of the row, the wave total is the fixed-order DPP sum.
template <int TANH>
__global__ __launch_bounds__(256) void linear_fwd_kernel(const float* __restrict__ in, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ out, int B, int K, int N,
                                                         HeadDrop d) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= N) return;  // whole waves leave; there is no barrier below
  const float* wrow = W + (long)j * K;
  for (int b0 = 0; b0 < B; b0 += HEAD_BT) {
    float acc[HEAD_BT];
    uint32_t rk[HEAD_BT];
#pragma unroll
    for (int bb = 0; bb < HEAD_BT; ++bb) {
      acc[bb] = 0.f;
      rk[bb] = d.thi ? drop_rowkey(d.seed, d.site, (uint64_t)(b0 + bb)) : 1u;
    }
    for (int k = lane * 4; k < K; k += 256) {
      const float4 w4 = *reinterpret_cast<const float4*>(wrow + k);
      const float w[4] = {w4.x, w4.y, w4.z, w4.w};
      uint32_t cm[4] = {1u, 1u, 1u, 1u};
      if (d.thi) {
#pragma unroll
        for (int e = 0; e < 4; ++e) cm[e] = drop_colmul((uint32_t)(k + e));
      }
#pragma unroll
      for (int bb = 0; bb < HEAD_BT; ++bb) {
        if (b0 + bb < B) {
          const float4 x4 = *reinterpret_cast<const float4*>(in + (long)(b0 + bb) * K + k);
          const float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[bb] = fmaf(d.thi ? head_drop(x[e], rk[bb], cm[e], d) : x[e], w[e], acc[bb]);
        }
      }
    }
#pragma unroll
    for (int bb = 0; bb < HEAD_BT; ++bb) {
      const float s = wave_sum(acc[bb]) + bias[j];
      if (lane == 0 && b0 + bb < B) out[(long)(b0 + bb) * N + j] = TANH ? tanhf(s) : s;
    }
  }
}

// out[b, k] = epilogue(sum_j g[b, j] W[j, k]): the input gradient of the same Linear.  A workgroup owns 32 columns k and HEAD_BT
// utterances; its 8 row groups take j = q, q + 8, ... (128-byte row segments) and meet in LDS in the order q = 0 .. 7.
// MODE 0: out = drop'(v) (the gradient through the dropout in front of the Linear);  MODE 1: out = drop'(v) * (1 - a^2), the
// tanh in front of that dropout as well.
template <int MODE>
__global__ __launch_bounds__(256) void linear_dinput_kernel(const float* __restrict__ g, const float* __restrict__ W,
                                                            const float* __restrict__ a, float* __restrict__ out, int B, int K, int N,
                                                            HeadDrop d) {
  static_assert(HEAD_BT == 8, "the second stage maps the 8 row groups onto the HEAD_BT utterances");
  __shared__ float red[8][HEAD_BT][32];
  const int kl = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int k = blockIdx.x * 32 + kl, b0 = blockIdx.y * HEAD_BT;
  float acc[HEAD_BT];
#pragma unroll
  for (int bb = 0; bb < HEAD_BT; ++bb) acc[bb] = 0.f;
  if (k < K) {
    for (int j = q; j < N; j += 8) {
      const float w = W[(long)j * K + k];
#pragma unroll
      for (int bb = 0; bb < HEAD_BT; ++bb)
        if (b0 + bb < B) acc[bb] = fmaf(g[(long)(b0 + bb) * N + j], w, acc[bb]);
    }
  }
#pragma unroll
  for (int bb = 0; bb < HEAD_BT; ++bb) red[q][bb][kl] = acc[bb];
  __syncthreads();
  const int bb = q, b = b0 + bb;  // second stage: thread (bb, kl)
  if (b < B && k < K) {
    float s = red[0][bb][kl];
    for (int t = 1; t < 8; ++t) s += red[t][bb][kl];
    if (d.thi) s = head_drop(s, drop_rowkey(d.seed, d.site, (uint64_t)b), drop_colmul((uint32_t)k), d);
    if constexpr (MODE == 1) {
      const float av = a[(long)b * K + k];
      s *= 1.f - av * av;
    }
    out[(long)b * K + k] = s;
  }
}

// dW[j, k] = sum_b g[b, j] drop(in[b, k]), db[j] = sum_b g[b, j] (b = 0 .. B-1 in that order): one thread per float4 of dW.
__global__ __launch_bounds__(256) void linear_dweight_kernel(const float* __restrict__ g, const float* __restrict__ in,
                                                             float* __restrict__ dW, float* __restrict__ db, int B, int K, int N,
                                                             HeadDrop d) {
  const int kq = K >> 2;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * kq) return;
  const int j = (int)(i / kq), k = (int)(i % kq) * 4;
  uint32_t cm[4] = {1u, 1u, 1u, 1u};
  if (d.thi) {
#pragma unroll
    for (int e = 0; e < 4; ++e) cm[e] = drop_colmul((uint32_t)(k + e));
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, sb = 0.f;
  for (int b = 0; b < B; ++b) {
    const float gv = g[(long)b * N + j];
    const float4 x4 = *reinterpret_cast<const float4*>(in + (long)b * K + k);
    const float x[4] = {x4.x, x4.y, x4.z, x4.w};
    const uint32_t rk = d.thi ? drop_rowkey(d.seed, d.site, (uint64_t)b) : 1u;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = fmaf(gv, d.thi ? head_drop(x[e], rk, cm[e], d) : x[e], acc[e]);
    sb += gv;
  }
  *reinterpret_cast<float4*>(dW + (long)j * K + k) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  if (k == 0) db[j] = sb;
}

// ---- softmax + cross-entropy: one workgroup; thread t takes the utterances t, t + 256, ...; the loss is the fixed-order sum
// of the 256 per-thread partials.
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, int B, int C,
                                                         float gscale, float* __restrict__ probs, float* __restrict__ loss,
                                                         float* __restrict__ dlogits) {
  __shared__ float part[256];
  float acc = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float* row = logits + (long)b * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, row[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(row[c] - m);
    const int lab = labels ? labels[b] : -1;
    for (int c = 0; c < C; ++c) {
      const float p = expf(row[c] - m) / s;
      probs[(long)b * C + c] = p;
      if (dlogits) dlogits[(long)b * C + c] = (p - (c == lab ? 1.f : 0.f)) * gscale;
    }
    // (the launcher has validated the host copy of the labels; a device copy that disagrees gives NaN, never an access)
    if (labels) acc += (lab >= 0 && lab < C) ? (logf(s) + m - row[lab]) : NAN;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0 && loss) {
    float t = 0.f;
    for (int i = 0; i < 256; ++i) t += part[i];
    loss[0] = t / (float)B;
  }
}

uint32_t head_thresh(float p) { return p <= 0.f ? 0u : (uint32_t)fminf(65535.f, roundf(p * 65536.f)); }  // norm_act.hip thresh_of
HeadDrop head_site(uint64_t seed, uint32_t site, float p, int training) {
  const uint32_t t = training ? head_thresh(p) : 0u;
  return HeadDrop{seed, site, t << 16, t ? 1.f / (1.f - (float)t / 65536.f) : 1.f};
}

bool pool_args_ok(const char* who, const void* hidden, const int32_t* lens, const int32_t* lens_host, int B, int F, int H, int mode,
                  int dtype) {
  if (!hidden) return ssak_set_error("%s: null pointer", who), false;
  if (B <= 0 || B > 65535 || F <= 0 || H <= 0) return ssak_set_error("%s: bad shape B=%d F=%d H=%d", who, B, F, H), false;
  if (H % 8) return ssak_set_error("%s: H=%d is not a multiple of 8", who, H), false;
  if (mode != SSAK_POOL_MEAN && mode != SSAK_POOL_SUM && mode != SSAK_POOL_MAX) return ssak_set_error("%s: unknown mode %d", who, mode), false;
  if (dtype != 0 && dtype != 1) return ssak_set_error("%s: dtype %d (0 = bf16, 1 = fp32)", who, dtype), false;
  if ((lens == nullptr) != (lens_host == nullptr))
    return ssak_set_error("%s: frame_lens and frame_lens_host come together (the same values on the device and on the host)", who), false;
  if (lens_host)
    for (int b = 0; b < B; ++b)
      if (lens_host[b] < 1 || lens_host[b] > F)
        return ssak_set_error("%s: frame_lens[%d] = %d outside [1, %d]", who, b, lens_host[b], F), false;
  return true;
}

template <typename T>
int pool_fwd_launch(const T* hidden, const int32_t* lens, int B, int F, int H, int mode, float* pooled, int32_t* argmax, hipStream_t st) {
  const dim3 grid(ssak_cdiv(H, POOL_COLS), B);
  if (mode == SSAK_POOL_MEAN)
    pool_fwd_kernel<T, SSAK_POOL_MEAN><<<grid, POOL_THREADS, 0, st>>>(hidden, lens, F, H, pooled, argmax);
  else if (mode == SSAK_POOL_SUM)
    pool_fwd_kernel<T, SSAK_POOL_SUM><<<grid, POOL_THREADS, 0, st>>>(hidden, lens, F, H, pooled, argmax);
  else
    pool_fwd_kernel<T, SSAK_POOL_MAX><<<grid, POOL_THREADS, 0, st>>>(hidden, lens, F, H, pooled, argmax);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

template <typename T>
int pool_bwd_launch(const float* dpooled, const int32_t* argmax, const int32_t* lens, int B, int F, int H, int mode, T* dhidden,
                    hipStream_t st) {
  const long total = (long)B * F * (H >> 3);
  const unsigned grid = (unsigned)std::min<long>((total + 255) / 256, 2048);
  if (mode == SSAK_POOL_MEAN)
    pool_bwd_kernel<T, SSAK_POOL_MEAN><<<grid, 256, 0, st>>>(dpooled, argmax, lens, B, F, H, dhidden);
  else if (mode == SSAK_POOL_SUM)
    pool_bwd_kernel<T, SSAK_POOL_SUM><<<grid, 256, 0, st>>>(dpooled, argmax, lens, B, F, H, dhidden);
  else
    pool_bwd_kernel<T, SSAK_POOL_MAX><<<grid, 256, 0, st>>>(dpooled, argmax, lens, B, F, H, dhidden);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

bool head_shape_ok(const char* who, int B, int H, int C, float p) {
  if (B <= 0 || B > 65535 * HEAD_BT || H <= 0 || C <= 0) return ssak_set_error("%s: bad shape B=%d H=%d C=%d", who, B, H, C), false;
  if (H % 4) return ssak_set_error("%s: H=%d is not a multiple of 4", who, H), false;
  if (!(p >= 0.f && p < 1.f)) return ssak_set_error("%s: dropout probability %g outside [0, 1)", who, (double)p), false;
  return true;
}
}  // namespace

extern "C" int ssak_pool_fwd(const void* hidden, const int32_t* frame_lens, const int32_t* frame_lens_host, int B, int F, int H, int mode,
                             int dtype, float* pooled, int32_t* argmax, void* stream) {
  if (!pool_args_ok("pool_fwd", hidden, frame_lens, frame_lens_host, B, F, H, mode, dtype)) return SSAK_ERR_INVALID;
  SSAK_REQUIRE(pooled && (mode != SSAK_POOL_MAX || argmax), "pool_fwd: null output pointer");
  SSAK_REQUIRE(aligned16(hidden), "pool_fwd: hidden is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1) return pool_fwd_launch<float>((const float*)hidden, frame_lens, B, F, H, mode, pooled, argmax, st);
  return pool_fwd_launch<bf16>((const bf16*)hidden, frame_lens, B, F, H, mode, pooled, argmax, st);
}

extern "C" int ssak_pool_bwd(const float* dpooled, const int32_t* argmax, const int32_t* frame_lens, const int32_t* frame_lens_host, int B,
                             int F, int H, int mode, int dtype, void* dhidden, void* stream) {
  if (!pool_args_ok("pool_bwd", dhidden, frame_lens, frame_lens_host, B, F, H, mode, dtype)) return SSAK_ERR_INVALID;
  SSAK_REQUIRE(dpooled && (mode != SSAK_POOL_MAX || argmax), "pool_bwd: null input pointer");
  SSAK_REQUIRE(aligned16(dhidden) && aligned16(dpooled) && aligned16(argmax), "pool_bwd: a buffer is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1) return pool_bwd_launch<float>(dpooled, argmax, frame_lens, B, F, H, mode, (float*)dhidden, st);
  return pool_bwd_launch<bf16>(dpooled, argmax, frame_lens, B, F, H, mode, (bf16*)dhidden, st);
}

extern "C" int ssak_cls_head_fwd(const float* pooled, const float* W1, const float* b1, const float* W2, const float* b2, int B, int H,
                                 int C, float drop_p, uint64_t seed, int training, float* act, float* logits, void* stream) {
  SSAK_REQUIRE(pooled && W1 && b1 && W2 && b2 && act && logits, "cls_head_fwd: null pointer");
  if (!head_shape_ok("cls_head_fwd", B, H, C, drop_p)) return SSAK_ERR_INVALID;
  SSAK_REQUIRE(aligned16(pooled) && aligned16(W1) && aligned16(W2) && aligned16(act), "cls_head_fwd: a buffer is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  linear_fwd_kernel<1><<<ssak_cdiv(H, 4), 256, 0, st>>>(pooled, W1, b1, act, B, H, H, head_site(seed, SSAK_CLS_SITE_INPUT, drop_p, training));
  SSAK_LAUNCH_CHECK();
  linear_fwd_kernel<0><<<ssak_cdiv(C, 4), 256, 0, st>>>(act, W2, b2, logits, B, H, C, head_site(seed, SSAK_CLS_SITE_HIDDEN, drop_p, training));
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" size_t ssak_cls_head_bwd_workspace_bytes(int B, int H, int C) {
  (void)C;
  return B > 0 && H > 0 ? (size_t)B * H * sizeof(float) : 0;  // dz [B, H]
}

extern "C" int ssak_cls_head_bwd(const float* dlogits, const float* pooled, const float* act, const float* W1, const float* W2, int B,
                                 int H, int C, float drop_p, uint64_t seed, int training, float* dW1, float* db1, float* dW2, float* db2,
                                 float* dpooled, void* workspace, size_t workspace_bytes, void* stream) {
  SSAK_REQUIRE(dlogits && pooled && act && W1 && W2 && dW1 && db1 && dW2 && db2 && dpooled && workspace, "cls_head_bwd: null pointer");
  if (!head_shape_ok("cls_head_bwd", B, H, C, drop_p)) return SSAK_ERR_INVALID;
  SSAK_REQUIRE(workspace_bytes >= ssak_cls_head_bwd_workspace_bytes(B, H, C), "cls_head_bwd: workspace too small");
  SSAK_REQUIRE(aligned16(workspace) && aligned16(pooled) && aligned16(act) && aligned16(dW1) && aligned16(dW2),
               "cls_head_bwd: a buffer is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const HeadDrop in_site = head_site(seed, SSAK_CLS_SITE_INPUT, drop_p, training), hid_site = head_site(seed, SSAK_CLS_SITE_HIDDEN, drop_p, training);
  float* dz = (float*)workspace;
  const dim3 gin(ssak_cdiv(H, 32), ssak_cdiv(B, HEAD_BT));
  // out_proj: dW2 = dlogits^T drop(a), db2;  dz = drop'(dlogits W2) * (1 - a^2)
  linear_dweight_kernel<<<ssak_cdiv((long)C * (H >> 2), 256), 256, 0, st>>>(dlogits, act, dW2, db2, B, H, C, hid_site);
  SSAK_LAUNCH_CHECK();
  linear_dinput_kernel<1><<<gin, 256, 0, st>>>(dlogits, W2, act, dz, B, H, C, hid_site);
  SSAK_LAUNCH_CHECK();
  // dense: dW1 = dz^T drop(pooled), db1;  dpooled = drop'(dz W1)
  linear_dweight_kernel<<<ssak_cdiv((long)H * (H >> 2), 256), 256, 0, st>>>(dz, pooled, dW1, db1, B, H, H, in_site);
  SSAK_LAUNCH_CHECK();
  linear_dinput_kernel<0><<<gin, 256, 0, st>>>(dz, W1, nullptr, dpooled, B, H, H, in_site);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" int ssak_cls_softmax_ce(const float* logits, const int32_t* labels, const int32_t* labels_host, int B, int C, float grad_scale,
                                   float* probs, float* loss, float* dlogits, void* stream) {
  SSAK_REQUIRE(logits && probs, "cls_softmax_ce: null pointer");
  SSAK_REQUIRE(B > 0 && C > 0, "cls_softmax_ce: bad shape B=%d C=%d", B, C);
  SSAK_REQUIRE((labels == nullptr) == (labels_host == nullptr),
               "cls_softmax_ce: labels and labels_host come together (the same values on the device and on the host)");
  SSAK_REQUIRE(labels || (!loss && !dlogits), "cls_softmax_ce: loss / dlogits need labels");
  if (labels_host)
    for (int b = 0; b < B; ++b)
      SSAK_REQUIRE(labels_host[b] >= 0 && labels_host[b] < C, "cls_softmax_ce: label[%d] = %d outside [0, %d)", b, labels_host[b], C);
  softmax_ce_kernel<<<1, 256, 0, (hipStream_t)stream>>>(logits, labels, B, C, grad_scale / (float)B, probs, loss, dlogits);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}
