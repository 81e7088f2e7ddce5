// Training-data augmentation on the device (ssak_amd/augment.py; the reference's SpeechAugment of ssak/utils/augment.py with
// wav2vec_train.py:258-273's arguments): gain, background noise, reverberation and time stretch, between the resample and the
// normalisation of DeviceIngest, on the ingest stream.
//
// Every parameter is drawn on the host and arrives as one fp64 row per utterance (SSAK_AUG_* columns, ssak_hip.h).  Results
// depend on an utterance's own samples and row only: sums are fixed-order fp64 trees over fixed 8192-sample chunks, FFT sizes
// follow from the utterance's own lengths, and there are no atomics -- an utterance alone gives the bits it gives in a batch.
//
// FFT: one radix-2 Stockham routine in LDS (n <= 4096 points per workgroup, ping-pong buffers), used directly for the 2048-point
// frames of the time stretch and as both steps of a four-step FFT (N = N1 * N2, twiddles in between) for the reverberation's
// linear convolution of up to 2^24 points.  Twiddles are sincospi of exact binary fractions.
#include <cfloat>
#include <cmath>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int AUG_CHUNK = 8192;  // samples per partial-sum block (fixed: the sums do not depend on the batch)
constexpr int AUG_THREADS = 256;
constexpr int FFT_MAX_LOG = 12;  // one workgroup's FFT: <= 4096 points
constexpr int TS_NFFT = 2048, TS_HOP = 512, TS_BINS = 1025;
constexpr int RV_MAX_LOG = 24;

__device__ __forceinline__ double block_sum_d(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// radix-2 Stockham FFT of a[0..n) (n = 2^logn <= 4096) in LDS; sgn -1 forward, +1 inverse (unscaled).  Returns the buffer that
// holds the result (a or b).  Ends with a barrier.
__device__ float2* lds_fft(float2* a, float2* b, int n, float sgn) {
  const int half = n >> 1;
  for (int ns = 1; ns < n; ns <<= 1) {
    for (int j = threadIdx.x; j < half; j += blockDim.x) {
      const int k = j & (ns - 1);
      const float2 u = a[j], v = a[j + half];
      float s, c;
      sincospif(sgn * (float)k / (float)ns, &s, &c);
      const float2 t = make_float2(v.x * c - v.y * s, v.x * s + v.y * c);
      const int o = ((j - k) << 1) + k;
      b[o] = make_float2(u.x + t.x, u.y + t.y);
      b[o + ns] = make_float2(u.x - t.x, u.y - t.y);
    }
    __syncthreads();
    float2* t = a;
    a = b;
    b = t;
  }
  return a;
}

__device__ __forceinline__ const double* row(const double* params, int b) { return params + (size_t)b * SSAK_AUG_NCOL; }
__device__ __forceinline__ int clamp_len(const int32_t* lens, int b, int T) { return lens ? min(max(lens[b], 0), T) : T; }

// ------------------------------------------------------------------------------------------------ gain and background noise
// segment of the noise file: start, S = min(L, N) samples; the noise sample at output t is seg[t % S] (the tiling)
struct NoiseSeg {
  const float* seg;
  int S;
};
__device__ __forceinline__ NoiseSeg noise_seg(const double* p, const ssak_audio_bank& nb, int L) {
  const int f = (int)p[SSAK_AUG_NOISE];
  const int N = nb.length[f];
  const int S = min(L, N);
  const long st = min(max((long)p[SSAK_AUG_NOISE_START], 0L), (long)(N - S));
  return NoiseSeg{nb.data + nb.offset[f] + st, S};
}

__global__ __launch_bounds__(AUG_THREADS) void gn_partial_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int T,
                                                                 const double* __restrict__ params, ssak_audio_bank nb,
                                                                 double* __restrict__ part, int nch) {
  __shared__ double red[16];
  const int b = blockIdx.y, c = blockIdx.x;
  const double* p = row(params, b);
  if ((int)p[SSAK_AUG_KIND] != SSAK_AUG_NOISE_MIX) return;
  const int L = clamp_len(lens, b, T);
  const int t0 = c * AUG_CHUNK;
  if (t0 >= L) return;
  const int t1 = min(L, t0 + AUG_CHUNK);
  const NoiseSeg ns = noise_seg(p, nb, L);
  const float* xb = x + (size_t)b * T;
  double sx = 0.0, sn = 0.0;
  for (int t = t0 + threadIdx.x; t < t1; t += AUG_THREADS) {
    const double v = xb[t];
    sx += v * v;
    if (t < ns.S) {
      const double n = ns.seg[t];
      sn += n * n;
    }
  }
  sx = block_sum_d(sx, red);
  sn = block_sum_d(sn, red);
  if (threadIdx.x == 0) {
    part[((size_t)b * nch + c) * 2] = sx;
    part[((size_t)b * nch + c) * 2 + 1] = sn;
  }
}

__global__ __launch_bounds__(AUG_THREADS) void gn_apply_kernel(const float* x, const int32_t* __restrict__ lens, int T,
                                                               const double* __restrict__ params, ssak_audio_bank nb,
                                                               const double* __restrict__ part, int nch, float* y) {
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * AUG_CHUNK;
  if (t0 >= T) return;
  const int t1 = min(T, t0 + AUG_CHUNK);
  const double* p = row(params, b);
  const int kind = (int)p[SSAK_AUG_KIND];
  const int L = clamp_len(lens, b, T);
  const float* xb = x + (size_t)b * T;
  float* yb = y + (size_t)b * T;
  if (kind == SSAK_AUG_GAIN) {
    const float g = (float)p[SSAK_AUG_GAIN_LIN];
    for (int t = t0 + threadIdx.x; t < t1; t += AUG_THREADS) yb[t] = t < L ? xb[t] * g : xb[t];
    return;
  }
  float f = 0.f;
  NoiseSeg ns{nullptr, 0};
  if (kind == SSAK_AUG_NOISE_MIX && L > 0) {
    ns = noise_seg(p, nb, L);
    double sx = 0.0, sn = 0.0;  // (every thread sums the same partials in the same order)
    for (int c = 0, n = (L + AUG_CHUNK - 1) / AUG_CHUNK; c < n; ++c) {
      sx += part[((size_t)b * nch + c) * 2];
      sn += part[((size_t)b * nch + c) * 2 + 1];
    }
    const double noise_rms = ns.S > 0 ? sqrt(sn / ns.S) : 0.0;
    if (noise_rms >= 1e-9) f = (float)((sqrt(sx / L) / p[SSAK_AUG_SNR_AMP]) / noise_rms);
  }
  if (f != 0.f) {
    for (int t = t0 + threadIdx.x; t < t1; t += AUG_THREADS) yb[t] = t < L ? xb[t] + ns.seg[t % ns.S] * f : xb[t];
  } else if (y != x) {
    for (int t = t0 + threadIdx.x; t < t1; t += AUG_THREADS) yb[t] = xb[t];
  }
}

// ------------------------------------------------------------------------------------------------ reverberation
// per utterance: log2 of the linear-convolution FFT size (-1: not reverberated)
struct RvGeom {
  int L, Lt, d, logn;
};
__device__ __forceinline__ RvGeom rv_geom(const double* params, const int32_t* lens, int T, const ssak_audio_bank& rb, int b) {
  const double* p = row(params, b);
  RvGeom g{0, 0, 0, -1};
  if ((int)p[SSAK_AUG_KIND] != SSAK_AUG_REVERB) return g;
  g.L = clamp_len(lens, b, T);
  if (g.L <= 0) return g;
  const int r = (int)p[SSAK_AUG_RIR];
  g.Lt = min(rb.length[r], g.L);
  const int d = (int)p[SSAK_AUG_RIR_PEAK];
  g.d = d < g.L ? d : 0;  // a peak past the truncation: h[:L] unrotated (augment_reverberation.py:291-303)
  const int need = g.L + g.Lt - 1;
  int k = 0;
  while ((1 << k) < need) ++k;
  g.logn = max(k, 1);
  return g;
}

// partial sums of x^2 and h^2 per chunk: the packed FFT carries h scaled by a power of two 2^e that brings its energy to x's
// (X and H are separated by conjugate symmetry, so each inherits rounding relative to |Z|: an h far quieter than x would lose
// digits).  What equal energies do not cover is an impulsive h: a few taps carry all of its energy, scaled they stand at about
// sqrt(L) times x's level, and in the first passes of the forward FFT their twiddle products round at that level into the real
// part, that is into the samples of x at the tap's position plus multiples of n / 2, n / 4, ...  The relative L2 error stays
// that of two separate transforms; isolated output samples are off by up to 20 times as much (5e-6 of max|y| for L = 2^23 and
// 3 taps, against 2e-7; tests/test_gpu_augment_edges.py).
__global__ __launch_bounds__(AUG_THREADS) void rv_energy_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int T,
                                                                const double* __restrict__ params, ssak_audio_bank rb,
                                                                double* __restrict__ part, int nch) {
  __shared__ double red[16];
  const int b = blockIdx.y, c = blockIdx.x;
  const RvGeom g = rv_geom(params, lens, T, rb, b);
  if (g.logn < 0) return;
  const int t0 = c * AUG_CHUNK;
  if (t0 >= g.L) return;
  const int t1 = min(g.L, t0 + AUG_CHUNK);
  const float* xb = x + (size_t)b * T;
  const float* h = rb.data + rb.offset[(int)row(params, b)[SSAK_AUG_RIR]];
  double sx = 0.0, sh = 0.0;
  for (int t = t0 + threadIdx.x; t < t1; t += AUG_THREADS) {
    const double v = xb[t];
    sx += v * v;
    if (t < g.Lt) {
      const double u = h[t];
      sh += u * u;
    }
  }
  sx = block_sum_d(sx, red);
  sh = block_sum_d(sh, red);
  if (threadIdx.x == 0) {
    part[((size_t)b * nch + c) * 2] = sx;
    part[((size_t)b * nch + c) * 2 + 1] = sh;
  }
}

// `silent` (if asked for): x or h[:L] is all zero.  Their product is then exactly zero, which the packed transform does not give
// by itself: the four-step FFT of a real signal is conjugate-symmetric only to rounding, so the H separated from FFT(x + i 0)
// is that rounding, and the rescale to mean|x| would bring it up to x's level.
__device__ __forceinline__ int rv_scale_exp(const double* part, int nch, int b, int L, bool* silent = nullptr) {
  double sx = 0.0, sh = 0.0;
  for (int c = 0, n = (L + AUG_CHUNK - 1) / AUG_CHUNK; c < n; ++c) {
    sx += part[((size_t)b * nch + c) * 2];
    sh += part[((size_t)b * nch + c) * 2 + 1];
  }
  const bool none = !(sx > 0.0) || !(sh > 0.0);
  if (silent) *silent = none;
  if (none) return 0;
  return max(-60, min(60, (int)rint(0.5 * log2(sx / sh))));
}

__global__ __launch_bounds__(AUG_THREADS) void rv_pack_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int T,
                                                              const double* __restrict__ params, ssak_audio_bank rb,
                                                              const double* __restrict__ part, int nch, float2* __restrict__ z, long nmax) {
  const int b = blockIdx.y;
  const RvGeom g = rv_geom(params, lens, T, rb, b);
  if (g.logn < 0) return;
  const long n = 1L << g.logn;
  const float s = ldexpf(1.f, rv_scale_exp(part, nch, b, g.L));
  const float* xb = x + (size_t)b * T;
  const float* h = rb.data + rb.offset[(int)row(params, b)[SSAK_AUG_RIR]];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    z[b * nmax + i] = make_float2(i < g.L ? xb[i] : 0.f, i < g.Lt ? h[i] * s : 0.f);
}

// one step of the four-step FFT of each utterance's n = 2^logn points (n1 = 2^ceil(logn/2) rows of n2 = 2^floor(logn/2)):
//   step 0: column q < n2: FFT over n1 of in[i * n2 + q], times w_n^(q k1), -> out[k1 * n2 + q]
//   step 1: row q < n1: FFT over n2 of in[q * n2 + i] -> out[q + n1 * k2]   (natural order)
__global__ __launch_bounds__(AUG_THREADS) void rv_fft_step_kernel(const float2* __restrict__ in, float2* __restrict__ out, long nmax,
                                                                  const int32_t* __restrict__ x_lens, int T, const double* __restrict__ params,
                                                                  ssak_audio_bank rb, int step, float sgn) {
  __shared__ float2 buf_a[1 << FFT_MAX_LOG], buf_b[1 << FFT_MAX_LOG];
  const int b = blockIdx.y, q = blockIdx.x;
  const RvGeom g = rv_geom(params, x_lens, T, rb, b);
  if (g.logn < 0) return;
  const int l1 = (g.logn + 1) / 2, l2 = g.logn / 2;
  const int n1 = 1 << l1, n2 = 1 << l2;
  const int m = step == 0 ? n1 : n2;
  if (q >= (step == 0 ? n2 : n1)) return;
  const float2* src = in + b * nmax;
  float2* dst = out + b * nmax;
  for (int i = threadIdx.x; i < m; i += blockDim.x) buf_a[i] = step == 0 ? src[(long)i * n2 + q] : src[(long)q * n2 + i];
  __syncthreads();
  const float2* r = lds_fft(buf_a, buf_b, m, sgn);
  if (step == 0) {
    const float inv = 2.f / (float)(1 << g.logn);  // sincospi(2 m / n): exact binary fractions
    for (int k = threadIdx.x; k < m; k += blockDim.x) {
      float s, c;
      sincospif(sgn * (float)(q * k) * inv, &s, &c);
      dst[(long)k * n2 + q] = cmul(r[k], make_float2(c, s));
    }
  } else {
    for (int k = threadIdx.x; k < m; k += blockDim.x) dst[q + (long)n1 * k] = r[k];
  }
}

// Z = FFT(x + i h) -> P = X H with X = (Z_k + conj Z_-k) / 2, H = (Z_k - conj Z_-k) / 2i
__global__ __launch_bounds__(AUG_THREADS) void rv_mul_kernel(const float2* __restrict__ z, float2* __restrict__ pr, long nmax,
                                                             const int32_t* __restrict__ lens, int T, const double* __restrict__ params,
                                                             ssak_audio_bank rb, const double* __restrict__ part, int nch) {
  const int b = blockIdx.y;
  const RvGeom g = rv_geom(params, lens, T, rb, b);
  if (g.logn < 0) return;
  const long n = 1L << g.logn;
  bool silent;
  const float hs = 0.5f * ldexpf(1.f, -rv_scale_exp(part, nch, b, g.L, &silent));  // (undoes the power-of-two scale of h exactly)
  const float2* zb = z + b * nmax;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x) {
    if (silent) {
      pr[b * nmax + k] = make_float2(0.f, 0.f);
      continue;
    }
    const float2 a = zb[k], c = zb[(n - k) & (n - 1)];
    const float2 X = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));
    const float2 H = make_float2(hs * (a.y + c.y), -hs * (a.x - c.x));
    pr[b * nmax + k] = cmul(X, H);
  }
}

// circular product of length L from the linear one c (length L + Lt - 1, real part / n), rotated by d:
//   w[t] = c[m] + c[m + L] (m + L < L + Lt - 1), m = (t + d) mod L;  partial sums of |x| and |w| per chunk
__global__ __launch_bounds__(AUG_THREADS) void rv_fold_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int T,
                                                              const double* __restrict__ params, ssak_audio_bank rb,
                                                              const float2* __restrict__ c, long nmax, float* __restrict__ w,
                                                              double* __restrict__ part, int nch) {
  __shared__ double red[16];
  const int b = blockIdx.y, ch = blockIdx.x;
  const RvGeom g = rv_geom(params, lens, T, rb, b);
  if (g.logn < 0) return;
  const int t0 = ch * AUG_CHUNK;
  if (t0 >= g.L) return;
  const int t1 = min(g.L, t0 + AUG_CHUNK);
  const float inv_n = 1.f / (float)(1L << g.logn);
  const float2* cb = c + b * nmax;
  const float* xb = x + (size_t)b * T;
  double sx = 0.0, sw = 0.0;
  for (int t = t0 + threadIdx.x; t < t1; t += AUG_THREADS) {
    int m = t + g.d;
    if (m >= g.L) m -= g.L;
    float v = cb[m].x;
    if (m < g.Lt - 1) v += cb[m + g.L].x;
    v *= inv_n;
    w[(size_t)b * nmax * 2 + t] = v;
    sx += fabs((double)xb[t]);
    sw += fabs((double)v);
  }
  sx = block_sum_d(sx, red);
  sw = block_sum_d(sw, red);
  if (threadIdx.x == 0) {
    part[((size_t)b * nch + ch) * 2] = sx;
    part[((size_t)b * nch + ch) * 2 + 1] = sw;
  }
}

// y = w / (mean|w| + 1e-14) * mean|x| (augment_reverberation.py _rescale "avg"); other utterances untouched
__global__ __launch_bounds__(AUG_THREADS) void rv_apply_kernel(const int32_t* __restrict__ lens, int T, const double* __restrict__ params,
                                                               ssak_audio_bank rb, const float* __restrict__ w, long nmax,
                                                               const double* __restrict__ part, int nch, float* y) {
  const int b = blockIdx.y;
  const RvGeom g = rv_geom(params, lens, T, rb, b);
  if (g.logn < 0) return;
  const int t0 = blockIdx.x * AUG_CHUNK;
  if (t0 >= g.L) return;
  const int t1 = min(g.L, t0 + AUG_CHUNK);
  double sx = 0.0, sw = 0.0;
  for (int c = 0, n = (g.L + AUG_CHUNK - 1) / AUG_CHUNK; c < n; ++c) {
    sx += part[((size_t)b * nch + c) * 2];
    sw += part[((size_t)b * nch + c) * 2 + 1];
  }
  const float s = (float)((sx / g.L) / (sw / g.L + 1e-14));
  const float* wb = w + (size_t)b * nmax * 2;
  for (int t = t0 + threadIdx.x; t < t1; t += AUG_THREADS) y[(size_t)b * T + t] = wb[t] * s;
}

// ------------------------------------------------------------------------------------------------ time stretch
struct TsGeom {
  int L, F, n_use, len_out;
  double rate;
};
__device__ __host__ __forceinline__ TsGeom ts_geom(int L, double rate) {
  TsGeom g;
  g.L = L;
  g.rate = rate;
  g.F = 1 + L / TS_HOP;
  const int n_out = (int)ceil((double)g.F / rate);  // len(np.arange(0, F, rate))
  g.len_out = (int)nearbyint((double)L / rate);     // round(L / rate), half to even
  g.n_use = min(n_out, (g.len_out + 2 * (TS_NFFT / 2) + TS_HOP - 1) / TS_HOP);
  return g;
}
__device__ __forceinline__ float hann(int t) { return 0.5f - 0.5f * cospif((float)t / (float)(TS_NFFT / 2)); }

// frame f: periodic-Hann-windowed x[512 f - 1024 + t] (zeros outside) -> 1025 bins of its 2048-point FFT
__global__ __launch_bounds__(AUG_THREADS) void ts_stft_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int T,
                                                              const double* __restrict__ params, float2* __restrict__ S, int fmax) {
  __shared__ float2 buf_a[TS_NFFT], buf_b[TS_NFFT];
  const int b = blockIdx.y, f = blockIdx.x;
  const TsGeom g = ts_geom(clamp_len(lens, b, T), row(params, b)[SSAK_AUG_RATE]);
  if (f >= g.F) return;
  const float* xb = x + (size_t)b * T;
  for (int t = threadIdx.x; t < TS_NFFT; t += blockDim.x) {
    const long i = (long)f * TS_HOP - TS_NFFT / 2 + t;
    buf_a[t] = make_float2(i >= 0 && i < g.L ? xb[i] * hann(t) : 0.f, 0.f);
  }
  __syncthreads();
  const float2* r = lds_fft(buf_a, buf_b, TS_NFFT, -1.f);
  float2* dst = S + ((size_t)b * fmax + f) * TS_BINS;
  for (int k = threadIdx.x; k < TS_BINS; k += blockDim.x) dst[k] = r[k];
}

// librosa.phase_vocoder(hop 512): one thread per (utterance, bin), a scan over the output frames; the phase accumulator in fp64
__global__ __launch_bounds__(AUG_THREADS) void ts_vocoder_kernel(const float2* __restrict__ S, int fmax, const int32_t* __restrict__ lens,
                                                                 int T, const double* __restrict__ params, float2* __restrict__ D, int omax) {
  const int b = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= TS_BINS) return;
  const TsGeom g = ts_geom(clamp_len(lens, b, T), row(params, b)[SSAK_AUG_RATE]);
  const float2* Sb = S + (size_t)b * fmax * TS_BINS + k;
  float2* Db = D + (size_t)b * omax * TS_BINS + k;
  const double two_pi = 6.283185307179586, phi = (double)k * (3.141592653589793 / 2.0);
  const float2 s0 = Sb[0];
  double acc = atan2f(s0.y, s0.x);
  for (int j = 0; j < g.n_use; ++j) {
    const double st = (double)j * g.rate;
    const int kf = (int)floor(st);
    const double a = st - kf;
    const float2 c0 = kf < g.F ? Sb[(size_t)kf * TS_BINS] : make_float2(0.f, 0.f);
    const float2 c1 = kf + 1 < g.F ? Sb[(size_t)(kf + 1) * TS_BINS] : make_float2(0.f, 0.f);
    const double mag = (1.0 - a) * (double)sqrtf(c0.x * c0.x + c0.y * c0.y) + a * (double)sqrtf(c1.x * c1.x + c1.y * c1.y);
    const double red = acc - two_pi * rint(acc / two_pi);
    float sn, cs;
    sincosf((float)red, &sn, &cs);
    Db[(size_t)j * TS_BINS] = make_float2((float)(mag * cs), (float)(mag * sn));
    double dp = (double)atan2f(c1.y, c1.x) - (double)atan2f(c0.y, c0.x) - phi;
    dp -= two_pi * rint(dp / two_pi);
    acc += phi + dp;
  }
}

// output frame j: irfft(2048) (imaginary parts of bins 0 and 1024 ignored) times the window
__global__ __launch_bounds__(AUG_THREADS) void ts_istft_kernel(const float2* __restrict__ D, int omax, const int32_t* __restrict__ lens,
                                                               int T, const double* __restrict__ params, float* __restrict__ Y) {
  __shared__ float2 buf_a[TS_NFFT], buf_b[TS_NFFT];
  const int b = blockIdx.y, j = blockIdx.x;
  const TsGeom g = ts_geom(clamp_len(lens, b, T), row(params, b)[SSAK_AUG_RATE]);
  if (j >= g.n_use) return;
  const float2* src = D + ((size_t)b * omax + j) * TS_BINS;
  for (int k = threadIdx.x; k < TS_NFFT; k += blockDim.x) {
    float2 v;
    if (k == 0 || k == TS_NFFT / 2)
      v = make_float2(src[k].x, 0.f);
    else if (k < TS_NFFT / 2)
      v = src[k];
    else {
      const float2 m = src[TS_NFFT - k];
      v = make_float2(m.x, -m.y);
    }
    buf_a[k] = v;
  }
  __syncthreads();
  const float2* r = lds_fft(buf_a, buf_b, TS_NFFT, 1.f);
  float* dst = Y + ((size_t)b * omax + j) * TS_NFFT;
  for (int t = threadIdx.x; t < TS_NFFT; t += blockDim.x) dst[t] = r[t].x * (1.f / TS_NFFT) * hann(t);
}

// overlap-add as a gather: output t sums its <= 4 frames at p = t + 1024 and divides by the window sum-square
__global__ __launch_bounds__(AUG_THREADS) void ts_ola_kernel(const float* __restrict__ Y, int omax, const int32_t* __restrict__ lens, int T,
                                                             const double* __restrict__ params, float* __restrict__ y, int Tout,
                                                             int32_t* __restrict__ out_lens) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const TsGeom g = ts_geom(clamp_len(lens, b, T), row(params, b)[SSAK_AUG_RATE]);
  if (t == 0 && out_lens) out_lens[b] = g.len_out;
  if (t >= Tout) return;
  float v = 0.f;
  if (t < g.len_out) {
    const int p = t + TS_NFFT / 2;
    const int f_hi = min(g.n_use - 1, p / TS_HOP);
    const int f_lo = p >= TS_NFFT ? (p - TS_NFFT + TS_HOP) / TS_HOP : 0;
    float sum = 0.f, wss = 0.f;
    const float* Yb = Y + (size_t)b * omax * TS_NFFT;
    for (int f = f_lo; f <= f_hi; ++f) {
      const int o = p - f * TS_HOP;
      const float w = hann(o);
      sum += Yb[(size_t)f * TS_NFFT + o];
      wss += w * w;
    }
    v = wss > FLT_MIN ? sum / wss : sum;
  }
  y[(size_t)b * Tout + t] = v;
}

size_t align256(size_t n) { return (n + 255) / 256 * 256; }

int check_lens_host(const int32_t* lens_host, int B, int T, const char* who) {
  SSAK_REQUIRE(lens_host, "%s: null lens_host", who);
  for (int b = 0; b < B; ++b) SSAK_REQUIRE(lens_host[b] >= 0 && lens_host[b] <= T, "%s: lens[%d] = %d outside [0, %d]", who, b, lens_host[b], T);
  return SSAK_OK;
}

int check_bank(const ssak_audio_bank* bk, const char* who) {
  SSAK_REQUIRE(bk && bk->n > 0, "%s: empty bank", who);
  SSAK_REQUIRE(bk->data && bk->offset && bk->length && bk->offset_host && bk->length_host, "%s: null bank pointer", who);
  for (int i = 0; i < bk->n; ++i) SSAK_REQUIRE(bk->length_host[i] > 0 && bk->offset_host[i] >= 0, "%s: bank entry %d is empty", who, i);
  return SSAK_OK;
}

long rv_nmax(int T, int max_rir_len) {
  const long need = (long)T + std::min(max_rir_len, T) - 1;
  long n = 2;
  while (n < need) n <<= 1;
  return n;
}

}  // namespace

extern "C" size_t ssak_augment_gain_noise_workspace_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  return align256((size_t)B * ssak_cdiv(T, AUG_CHUNK) * 2 * sizeof(double));
}

extern "C" int ssak_augment_gain_noise(const float* x, const int32_t* lens, const int32_t* lens_host, int B, int T, const double* params,
                                       const double* params_host, const ssak_audio_bank* noise, float* y, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  SSAK_REQUIRE(x && lens && params && params_host && y, "augment_gain_noise: null pointer");
  SSAK_REQUIRE(B > 0 && T > 0, "augment_gain_noise: bad shape B=%d T=%d", B, T);
  if (int rc = check_lens_host(lens_host, B, T, "augment_gain_noise")) return rc;
  bool any_noise = false;
  for (int b = 0; b < B; ++b) {
    const double* p = params_host + (size_t)b * SSAK_AUG_NCOL;
    const int kind = (int)p[SSAK_AUG_KIND];
    SSAK_REQUIRE(kind >= SSAK_AUG_NONE && kind <= SSAK_AUG_REVERB, "augment_gain_noise: row %d has kind %d", b, kind);
    if (kind == SSAK_AUG_GAIN) SSAK_REQUIRE(std::isfinite(p[SSAK_AUG_GAIN_LIN]), "augment_gain_noise: row %d gain is not finite", b);
    if (kind == SSAK_AUG_NOISE_MIX) {
      if (!any_noise) {
        if (int rc = check_bank(noise, "augment_gain_noise: noise bank")) return rc;
        any_noise = true;
      }
      const int f = (int)p[SSAK_AUG_NOISE];
      SSAK_REQUIRE(f >= 0 && f < noise->n, "augment_gain_noise: row %d noise file %d outside [0, %d)", b, f, noise->n);
      const long N = noise->length_host[f], S = std::min<long>(lens_host[b], N), st = (long)p[SSAK_AUG_NOISE_START];
      SSAK_REQUIRE(st >= 0 && st + S <= N, "augment_gain_noise: row %d noise start %ld outside [0, %ld]", b, st, N - S);
      SSAK_REQUIRE(p[SSAK_AUG_SNR_AMP] > 0.0 && std::isfinite(p[SSAK_AUG_SNR_AMP]), "augment_gain_noise: row %d snr amplitude", b);
    }
  }
  const int nch = ssak_cdiv(T, AUG_CHUNK);
  SSAK_REQUIRE(workspace && workspace_bytes >= ssak_augment_gain_noise_workspace_bytes(B, T), "augment_gain_noise: workspace too small");
  ssak_audio_bank nb{};
  if (any_noise) nb = *noise;
  double* part = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (any_noise) {
    gn_partial_kernel<<<dim3(nch, B), AUG_THREADS, 0, st>>>(x, lens, T, params, nb, part, nch);
    SSAK_LAUNCH_CHECK();
  }
  gn_apply_kernel<<<dim3(nch, B), AUG_THREADS, 0, st>>>(x, lens, T, params, nb, part, nch, y);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

extern "C" size_t ssak_augment_reverb_workspace_bytes(int B, int T, int max_rir_len) {
  if (B <= 0 || T <= 0 || max_rir_len <= 0) return 0;
  const long nmax = rv_nmax(T, max_rir_len);
  return 2 * align256((size_t)B * nmax * sizeof(float2)) + align256((size_t)B * ssak_cdiv(T, AUG_CHUNK) * 2 * sizeof(double));
}

extern "C" int ssak_augment_reverb(const float* x, const int32_t* lens, const int32_t* lens_host, int B, int T, const double* params,
                                   const double* params_host, const ssak_audio_bank* rirs, float* y, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  SSAK_REQUIRE(x && lens && params && params_host && y, "augment_reverb: null pointer");
  SSAK_REQUIRE(B > 0 && T > 0, "augment_reverb: bad shape B=%d T=%d", B, T);
  if (int rc = check_lens_host(lens_host, B, T, "augment_reverb")) return rc;
  int max_rir = 0, max_log = -1;
  for (int b = 0; b < B; ++b) {
    const double* p = params_host + (size_t)b * SSAK_AUG_NCOL;
    if ((int)p[SSAK_AUG_KIND] != SSAK_AUG_REVERB) continue;
    if (max_rir == 0)
      if (int rc = check_bank(rirs, "augment_reverb: RIR bank")) return rc;
    const int r = (int)p[SSAK_AUG_RIR];
    SSAK_REQUIRE(r >= 0 && r < rirs->n, "augment_reverb: row %d RIR %d outside [0, %d)", b, r, rirs->n);
    const int Lh = rirs->length_host[r], d = (int)p[SSAK_AUG_RIR_PEAK];
    SSAK_REQUIRE(d >= 0 && d < Lh, "augment_reverb: row %d RIR peak %d outside [0, %d)", b, d, Lh);
    max_rir = std::max(max_rir, Lh);
    if (lens_host[b] > 0) {
      const long need = (long)lens_host[b] + std::min(Lh, lens_host[b]) - 1;
      int k = 1;
      while ((1L << k) < need) ++k;
      SSAK_REQUIRE(k <= RV_MAX_LOG, "augment_reverb: row %d needs a 2^%d-point FFT (at most 2^%d)", b, k, RV_MAX_LOG);
      max_log = std::max(max_log, k);
    }
  }
  if (y != x)
    SSAK_HIP(hipMemcpyAsync(y, x, (size_t)B * T * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (max_log < 0) return SSAK_OK;  // nothing reverberated
  const long nmax = rv_nmax(T, max_rir);
  SSAK_REQUIRE(workspace && workspace_bytes >= ssak_augment_reverb_workspace_bytes(B, T, max_rir), "augment_reverb: workspace too small");
  const int nch = ssak_cdiv(T, AUG_CHUNK);
  char* w = (char*)workspace;
  float2* buf0 = (float2*)w;
  float2* buf1 = (float2*)(w + align256((size_t)B * nmax * sizeof(float2)));
  double* part = (double*)(w + 2 * align256((size_t)B * nmax * sizeof(float2)));
  const ssak_audio_bank rb = *rirs;
  hipStream_t st = (hipStream_t)stream;
  const int n1max = 1 << ((max_log + 1) / 2), n2max = 1 << (max_log / 2);
  const int gx = std::min<long>(ssak_cdiv(1L << max_log, AUG_THREADS * 4), 4096);
  rv_energy_kernel<<<dim3(nch, B), AUG_THREADS, 0, st>>>(x, lens, T, params, rb, part, nch);
  SSAK_LAUNCH_CHECK();
  rv_pack_kernel<<<dim3(gx, B), AUG_THREADS, 0, st>>>(x, lens, T, params, rb, part, nch, buf0, nmax);
  SSAK_LAUNCH_CHECK();
  rv_fft_step_kernel<<<dim3(n2max, B), AUG_THREADS, 0, st>>>(buf0, buf1, nmax, lens, T, params, rb, 0, -1.f);
  SSAK_LAUNCH_CHECK();
  rv_fft_step_kernel<<<dim3(n1max, B), AUG_THREADS, 0, st>>>(buf1, buf0, nmax, lens, T, params, rb, 1, -1.f);
  SSAK_LAUNCH_CHECK();
  rv_mul_kernel<<<dim3(gx, B), AUG_THREADS, 0, st>>>(buf0, buf1, nmax, lens, T, params, rb, part, nch);
  SSAK_LAUNCH_CHECK();
  rv_fft_step_kernel<<<dim3(n2max, B), AUG_THREADS, 0, st>>>(buf1, buf0, nmax, lens, T, params, rb, 0, 1.f);
  SSAK_LAUNCH_CHECK();
  rv_fft_step_kernel<<<dim3(n1max, B), AUG_THREADS, 0, st>>>(buf0, buf1, nmax, lens, T, params, rb, 1, 1.f);
  SSAK_LAUNCH_CHECK();
  // the folded product goes to buf0 viewed as floats ([B][2 nmax]; it needs L <= nmax of them)
  rv_fold_kernel<<<dim3(nch, B), AUG_THREADS, 0, st>>>(x, lens, T, params, rb, buf1, nmax, (float*)buf0, part, nch);
  SSAK_LAUNCH_CHECK();
  rv_apply_kernel<<<dim3(nch, B), AUG_THREADS, 0, st>>>(lens, T, params, rb, (const float*)buf0, nmax, part, nch, y);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

namespace {
// ------------------------------------------------------------------------------------------------ FIR + chunk drop
// TimeDomainSpecAugment's DropFreq (one 101-tap notch product for the batch) and DropChunk in one read and one write of the
// batch.  A workgroup makes FIR_TILE consecutive outputs of one row: the tile and its halo go to LDS once (16-byte loads
// where the row allows them), each thread then makes two groups of 4 consecutive outputs from sliding register windows, so
// that a step of 4 taps costs two 16-byte LDS reads of samples and one (broadcast) of taps for 32 FMAs.
//
// Alignment: rows start at b * T floats, which is 16-byte aligned for no T in particular, so the tiles of row b start at
// t0 = tile * FIR_TILE - m with m = (b * T) mod 4: the flat index of every fourth sample of a tile, and of every thread's first
// output, is then a multiple of 4.  The window is read from LDS at offsets that are multiples of 4 as well: LDS index j holds
// row sample t0 - lead + j with lead = ntaps / 2 rounded up to 4, and the taps are stored behind s = lead - ntaps / 2 zeros.
constexpr int FIR_TILE = SSAK_AUG_FIR_TILE, FIR_THREADS = 256, FIR_SUB = FIR_TILE / (4 * FIR_THREADS);
constexpr int FIR_KP_MAX = (SSAK_AUG_FIR_MAX_TAPS + 3 + 3) / 4 * 4;  // taps behind <= 3 zeros, rounded up to 4: 260
static_assert(FIR_SUB == 2, "fir_drop_kernel is written for two groups of 4 outputs per thread");

// One 16-byte LDS read that stays one: left to itself the compiler fetches the window's odd pairs (the operands of its packed
// FMAs) with separate 8-byte reads at odd offsets, 4 lanes to a bank.
typedef float fir_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ fir_f4 lds16(const float4* p) {  // p points into LDS
  return *(const volatile __attribute__((address_space(3))) fir_f4*)p;
}

// 4 samples of a row from sample r on (r + the row's base is a multiple of 4 when `wide`), zeros outside [0, T)
__device__ __forceinline__ float4 load4(const float* __restrict__ xb, int r, int T, bool wide) {
  if (wide && r >= 0 && r + 3 < T) return *(const float4*)(xb + r);
  float4 v;
  v.x = r >= 0 && r < T ? xb[r] : 0.f;
  v.y = r + 1 >= 0 && r + 1 < T ? xb[r + 1] : 0.f;
  v.z = r + 2 >= 0 && r + 2 < T ? xb[r + 2] : 0.f;
  v.w = r + 3 >= 0 && r + 3 < T ? xb[r + 3] : 0.f;
  return v;
}

// Thread i makes outputs 4 i .. 4 i + 3 of each half of the tile: consecutive lanes read consecutive 16-byte slots of LDS (no
// bank conflict for 16-byte reads; 8 consecutive outputs per thread would put the lanes 32 bytes apart, 2 lanes per slot) and
// store consecutive 16 bytes.
__global__ __launch_bounds__(FIR_THREADS) void fir_drop_kernel(const float* __restrict__ x, int T, const float* __restrict__ taps, int ntaps,
                                                               const int32_t* __restrict__ chunks, const int32_t* __restrict__ counts,
                                                               int max_chunks, float* __restrict__ out, int wide) {
  __shared__ float4 xs[(FIR_TILE + FIR_KP_MAX) / 4];
  __shared__ float4 ts[FIR_KP_MAX / 4];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * T;
  const int m = wide ? (int)(base & 3) : 0;
  const int t0 = blockIdx.x * FIR_TILE - m;
  if (t0 >= T) return;
  const float* xb = x + base;
  float* ob = out + base;
  const int32_t* ch = chunks ? chunks + (size_t)b * max_chunks * 2 : nullptr;
  const int nch = chunks ? min(max(counts[b], 0), max_chunks) : 0;
  float4 acc[FIR_SUB];
  if (ntaps == 0) {  // no filter: a copy
#pragma unroll
    for (int h = 0; h < FIR_SUB; ++h) acc[h] = load4(xb, t0 + (h * FIR_THREADS + threadIdx.x) * 4, T, wide);
  } else {
    const int half = ntaps >> 1, lead = (half + 3) & ~3, s = lead - half;
    const int kp = (s + ntaps + 3) & ~3;
    for (int j = threadIdx.x; j < kp; j += FIR_THREADS) ((float*)ts)[j] = j >= s && j - s < ntaps ? taps[j - s] : 0.f;
    for (int j4 = threadIdx.x; j4 < (FIR_TILE + kp) / 4; j4 += FIR_THREADS) xs[j4] = load4(xb, t0 - lead + 4 * j4, T, wide);
    __syncthreads();
    const float4* win0 = xs + threadIdx.x;
    const float4* win1 = xs + FIR_THREADS + threadIdx.x;
    fir_f4 a0 = lds16(win0), b0 = lds16(win1);
    float ya[4] = {0.f, 0.f, 0.f, 0.f}, yb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int k4 = 0; k4 < kp / 4; ++k4) {
      const fir_f4 a1 = lds16(win0 + k4 + 1), b1 = lds16(win1 + k4 + 1);
      const fir_f4 g = lds16(ts + k4);
      const float wa[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const float wb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      const float gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ya[i] = fmaf(gg[j], wa[i + j], ya[i]);
          yb[i] = fmaf(gg[j], wb[i + j], yb[i]);
        }
      a0 = a1;
      b0 = b1;
    }
    acc[0] = make_float4(ya[0], ya[1], ya[2], ya[3]);
    acc[1] = make_float4(yb[0], yb[1], yb[2], yb[3]);
  }
  float y[FIR_SUB][4] = {{acc[0].x, acc[0].y, acc[0].z, acc[0].w}, {acc[1].x, acc[1].y, acc[1].z, acc[1].w}};
  for (int c = 0; c < nch; ++c) {
    const int cs = ch[2 * c], ce = ch[2 * c + 1];
    if (ce <= t0 || cs >= t0 + FIR_TILE) continue;  // (uniform: most tiles meet no chunk)
#pragma unroll
    for (int h = 0; h < FIR_SUB; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = t0 + (h * FIR_THREADS + threadIdx.x) * 4 + i;
        if (t >= cs && t < ce) y[h][i] = 0.f;
      }
  }
#pragma unroll
  for (int h = 0; h < FIR_SUB; ++h) {
    const int t = t0 + (h * FIR_THREADS + threadIdx.x) * 4;  // this thread's first output of this half
    if (wide && t >= 0 && t + 4 <= T) {
      *(float4*)(ob + t) = make_float4(y[h][0], y[h][1], y[h][2], y[h][3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (t + i >= 0 && t + i < T) ob[t + i] = y[h][i];
    }
  }
}

}  // namespace

extern "C" int ssak_augment_fir_drop(const float* x, int B, int T, const float* taps, int ntaps, const int32_t* chunks,
                                     const int32_t* chunk_counts, const int32_t* chunk_counts_host, int max_chunks, float* out, void* stream) {
  SSAK_REQUIRE(x && out, "augment_fir_drop: null pointer");
  SSAK_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= (1 << 30), "augment_fir_drop: bad shape B=%d T=%d", B, T);
  SSAK_REQUIRE(out + (size_t)B * T <= x || x + (size_t)B * T <= out, "augment_fir_drop: out must not overlap x");
  if (taps) {
    SSAK_REQUIRE(ntaps > 0 && (ntaps & 1) && ntaps <= SSAK_AUG_FIR_MAX_TAPS, "augment_fir_drop: ntaps = %d must be odd and at most %d", ntaps,
                 SSAK_AUG_FIR_MAX_TAPS);
  } else {
    SSAK_REQUIRE(ntaps == 0, "augment_fir_drop: null taps with ntaps = %d", ntaps);
  }
  if (chunks) {
    SSAK_REQUIRE(chunk_counts && chunk_counts_host, "augment_fir_drop: chunks without their counts");
    SSAK_REQUIRE(max_chunks > 0, "augment_fir_drop: max_chunks = %d", max_chunks);
    for (int b = 0; b < B; ++b)
      SSAK_REQUIRE(chunk_counts_host[b] >= 0 && chunk_counts_host[b] <= max_chunks, "augment_fir_drop: row %d has %d chunks, outside [0, %d]", b,
                   chunk_counts_host[b], max_chunks);
  }
  const int wide = (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  fir_drop_kernel<<<dim3(ssak_cdiv((long)T + 3, FIR_TILE), B), FIR_THREADS, 0, (hipStream_t)stream>>>(x, T, taps, ntaps, chunks, chunk_counts,
                                                                                                      max_chunks, out, wide);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}

namespace {
void ts_sizes(int T, int T_out, int* fmax, int* omax) {
  *fmax = 1 + T / TS_HOP;
  *omax = (T_out + TS_NFFT + TS_HOP - 1) / TS_HOP;
}
}  // namespace

extern "C" size_t ssak_augment_time_stretch_workspace_bytes(int B, int T, int T_out) {
  if (B <= 0 || T <= 0 || T_out <= 0) return 0;
  int fmax, omax;
  ts_sizes(T, T_out, &fmax, &omax);
  return align256((size_t)B * fmax * TS_BINS * sizeof(float2)) + align256((size_t)B * omax * TS_BINS * sizeof(float2)) +
         align256((size_t)B * omax * TS_NFFT * sizeof(float));
}

extern "C" int ssak_augment_time_stretch(const float* x, const int32_t* lens, const int32_t* lens_host, int B, int T, const double* params,
                                         const double* params_host, float* y, int32_t* out_lens, int T_out, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  SSAK_REQUIRE(x && lens && params && params_host && y, "augment_time_stretch: null pointer");
  SSAK_REQUIRE(y != x, "augment_time_stretch: y must not alias x");
  SSAK_REQUIRE(B > 0 && T > 0 && T_out > 0, "augment_time_stretch: bad shape B=%d T=%d T_out=%d", B, T, T_out);
  if (int rc = check_lens_host(lens_host, B, T, "augment_time_stretch")) return rc;
  int max_f = 1, max_use = 1;
  for (int b = 0; b < B; ++b) {
    const double rate = params_host[(size_t)b * SSAK_AUG_NCOL + SSAK_AUG_RATE];
    SSAK_REQUIRE(rate >= 0.5 && rate <= 2.0, "augment_time_stretch: row %d rate %g outside [0.5, 2]", b, rate);
    const TsGeom g = ts_geom(lens_host[b], rate);
    SSAK_REQUIRE(g.len_out <= T_out, "augment_time_stretch: row %d needs %d output samples, T_out = %d", b, g.len_out, T_out);
    max_f = std::max(max_f, g.F);
    max_use = std::max(max_use, g.n_use);
  }
  SSAK_REQUIRE(workspace && workspace_bytes >= ssak_augment_time_stretch_workspace_bytes(B, T, T_out), "augment_time_stretch: workspace too small");
  int fmax, omax;
  ts_sizes(T, T_out, &fmax, &omax);
  char* w = (char*)workspace;
  float2* S = (float2*)w;
  float2* D = (float2*)(w + align256((size_t)B * fmax * TS_BINS * sizeof(float2)));
  float* Y = (float*)((char*)D + align256((size_t)B * omax * TS_BINS * sizeof(float2)));
  hipStream_t st = (hipStream_t)stream;
  ts_stft_kernel<<<dim3(max_f, B), AUG_THREADS, 0, st>>>(x, lens, T, params, S, fmax);
  SSAK_LAUNCH_CHECK();
  ts_vocoder_kernel<<<dim3(ssak_cdiv(TS_BINS, 64), B), 64, 0, st>>>(S, fmax, lens, T, params, D, omax);
  SSAK_LAUNCH_CHECK();
  ts_istft_kernel<<<dim3(max_use, B), AUG_THREADS, 0, st>>>(D, omax, lens, T, params, Y);
  SSAK_LAUNCH_CHECK();
  ts_ola_kernel<<<dim3(ssak_cdiv(T_out, AUG_THREADS), B), AUG_THREADS, 0, st>>>(Y, omax, lens, T, params, y, T_out, out_lens);
  SSAK_LAUNCH_CHECK();
  return SSAK_OK;
}
