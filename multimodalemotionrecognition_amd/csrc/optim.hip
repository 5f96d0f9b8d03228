// The optimizer's per-step passes over FusedAdam's flat fp32 buffers (optim.py) beyond the bare Adam recurrence of
// csrc/head.hip: the global gradient norm (mer_grad_sqnorm + mer_clip_finalize) and the Adam step that takes the clip
// coefficient from device memory and keeps an exponential moving average of the weights (mer_adam_step_ex).
//
// Everything here is HBM-bound and bitwise reproducible: no floating-point atomics, every sum in a fixed order that
// depends on neither the grid size nor the order in which workgroups run.
#include "common.h"
#include "mer.h"

#include <math.h>

// ---------------------------------------------------------------------------------------
// Sum of squares over a table of segments.  A segment is cut into chunks of MER_NORM_CHUNK floats counted from the
// SEGMENT's start (the last chunk of a segment is short); chunk c of the launch is chunk c - first_chunk[s] of the
// segment s that holds it.  One workgroup reduces one chunk at a time:
//   thread t squares (in fp64) and adds the float4s t, t + 256, t + 512, t + 768 of the chunk, x y z w in turn;
//   the 64 lanes of a wave are folded by the xor tree 32, 16, 8, 4, 2, 1;
//   the four wave sums are added as ((w0 + w1) + w2) + w3 and stored to partials[c].
// Which workgroup takes which chunk changes nothing: partials[c] has a single writer and a fixed summation order.
// ---------------------------------------------------------------------------------------
static_assert(MER_NORM_CHUNK % 1024 == 0, "a chunk is a whole number of 256-thread float4 passes");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ((w0 + w1) + w2) + w3 of the four waves' sums, valid in thread 0; `red` is reusable after the trailing barrier
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(int nseg, const long* __restrict__ segs, long nchunks,
                                                          double* __restrict__ partials) {
  __shared__ double red[4];
  constexpr int PASSES = MER_NORM_CHUNK / 1024;
  for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    int lo = 0, hi = nseg - 1;  // the last segment whose first chunk is <= c
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[3 * mid + 2] <= c) lo = mid; else hi = mid - 1;
    }
    const long first = (c - segs[3 * lo + 2]) * MER_NORM_CHUNK;
    const long left = segs[3 * lo + 1] - first;  // <= 0 only for a table that does not cover chunk c: nothing is read
    const int n4 = (int)((left < MER_NORM_CHUNK ? (left > 0 ? left : 0) : MER_NORM_CHUNK) / 4);
    const float4* x = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(segs[3 * lo]) + first);
    float4 q[PASSES];
#pragma unroll
    for (int j = 0; j < PASSES; ++j) {
      const int i = threadIdx.x + 256 * j;
      q[j] = i < n4 ? x[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < PASSES; ++j) {
      acc += (double)q[j].x * (double)q[j].x;
      acc += (double)q[j].y * (double)q[j].y;
      acc += (double)q[j].z * (double)q[j].z;
      acc += (double)q[j].w * (double)q[j].w;
    }
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) partials[c] = s;
  }
}

MER_API int mer_grad_sqnorm(int nseg, const long* segs, long nchunks, double* partials, void* stream) {
  if (nseg <= 0 || nchunks <= 0 || !segs || !partials) return (int)hipErrorInvalidValue;
  if (((uintptr_t)segs | (uintptr_t)partials) & 7) return (int)hipErrorInvalidValue;
  const int grid = (int)(nchunks < 2048 ? nchunks : 2048);
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, nseg, segs, nchunks, partials);
  MER_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------
// One workgroup: the partials in index order (thread t adds t, t + 256, ...; then the same tree), the norm, the
// clip coefficient and the running telemetry of the record documented in mer.h.
// ---------------------------------------------------------------------------------------
static_assert(MER_CLIP_THREADS == 256, "block_sum_f64 folds four waves");

__global__ __launch_bounds__(MER_CLIP_THREADS) void clip_finalize_kernel(long nchunks, const double* __restrict__ partials,
                                                                         float grad_scale, float max_norm,
                                                                         float* __restrict__ rec) {
  __shared__ double red[4];
  double acc = 0.0;
  for (long i = threadIdx.x; i < nchunks; i += MER_CLIP_THREADS) acc += partials[i];
  const double sum = block_sum_f64(acc, red);
  if (threadIdx.x == 0) {
    const float total = (float)((double)grad_scale * sqrt(sum));
    const float c = max_norm / (total + 1e-6f);
    const float coef = c > 1.f ? 1.f : c;  // min(1, c) that keeps a NaN, as torch's clamp(max=1) does
    rec[MER_CLIP_TOTAL_NORM] = total;
    rec[MER_CLIP_COEF] = coef;
    rec[MER_CLIP_STEPS] = rec[MER_CLIP_STEPS] + 1.f;
    if (isfinite(total)) {
      rec[MER_CLIP_NORM_SUM] = rec[MER_CLIP_NORM_SUM] + total;
      rec[MER_CLIP_NORM_MAX] = fmaxf(rec[MER_CLIP_NORM_MAX], total);
    } else {
      rec[MER_CLIP_NONFINITE] = rec[MER_CLIP_NONFINITE] + 1.f;
    }
  }
}

MER_API int mer_clip_finalize(long nchunks, const double* partials, float grad_scale, float max_norm, float* rec,
                              void* stream) {
  if (nchunks <= 0 || !partials || !rec) return (int)hipErrorInvalidValue;
  if (((uintptr_t)partials & 7) || ((uintptr_t)rec & 3)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(MER_CLIP_THREADS), 0, (hipStream_t)stream, nchunks, partials,
                     grad_scale, max_norm, rec);
  MER_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------
// adam_kernel of csrc/head.hip with the gradient scale multiplied by a device-resident clip coefficient and an
// optional EMA plane.  ADAM1 and the scalar tail restate adam_kernel's character for character (there `gscale` is a
// kernel argument, here grad_scale * *coef formed once per thread), so with *coef == 1 and no EMA the two kernels
// compute the same bits (tests/test_optim_kernels_gpu.py compares them).
//   e += (1 - d) * (p_new - e)  after the parameter update.
// HBM-bound: 16 B read + 12 B written per parameter, + 4 B read and 4 B written with the EMA.
// ---------------------------------------------------------------------------------------
template <bool EMA>
__global__ __launch_bounds__(256) void adam_ex_kernel(long n, float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v, float lr, float b1,
                                                      float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                                      float grad_scale, const float* __restrict__ coef,
                                                      float* __restrict__ ema, float ema_decay) {
  const long n4 = n / 4;
  const float step = lr / bc1;
  const float gscale = coef ? grad_scale * *coef : grad_scale;
  const float ema_w = 1.f - ema_decay;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n4; e += (long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[e];
    const float4 gg = reinterpret_cast<const float4*>(g)[e];
    float4 mm = reinterpret_cast<float4*>(m)[e];
    float4 vv = reinterpret_cast<float4*>(v)[e];
    float4 ee;
    if constexpr (EMA) ee = reinterpret_cast<float4*>(ema)[e];
#define ADAM1(c)                                                  \
  {                                                               \
    const float gr = gscale * gg.c + wd * pp.c;                   \
    mm.c = b1 * mm.c + (1.f - b1) * gr;                           \
    vv.c = b2 * vv.c + (1.f - b2) * gr * gr;                      \
    pp.c -= step * mm.c / (sqrtf(vv.c) / bc2_sqrt + eps);         \
  }
    ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
    reinterpret_cast<float4*>(p)[e] = pp;
    reinterpret_cast<float4*>(m)[e] = mm;
    reinterpret_cast<float4*>(v)[e] = vv;
    if constexpr (EMA) {
      ee.x += ema_w * (pp.x - ee.x);
      ee.y += ema_w * (pp.y - ee.y);
      ee.z += ema_w * (pp.z - ee.z);
      ee.w += ema_w * (pp.w - ee.w);
      reinterpret_cast<float4*>(ema)[e] = ee;
    }
  }
  for (long e = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const float gr = gscale * g[e] + wd * p[e];
    m[e] = b1 * m[e] + (1.f - b1) * gr;
    v[e] = b2 * v[e] + (1.f - b2) * gr * gr;
    p[e] -= step * m[e] / (sqrtf(v[e]) / bc2_sqrt + eps);
    if constexpr (EMA) ema[e] += ema_w * (p[e] - ema[e]);
  }
}

MER_API int mer_adam_step_ex(long n, float* p, const float* g, float* m, float* v, float lr, float b1, float b2,
                             float eps, float wd, int step, float grad_scale, const float* coef, float* ema,
                             float ema_decay, void* stream) {
  if (n <= 0) return 0;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) return (int)hipErrorInvalidValue;
  if ((uintptr_t)coef & 3) return (int)hipErrorInvalidValue;
  const float bc1 = 1.f - powf(b1, (float)step);
  const float bc2s = sqrtf(1.f - powf(b2, (float)step));
  const long n4 = (n + 3) / 4;
  const int grid = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
  if (ema)
    hipLaunchKernelGGL(adam_ex_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, p, g, m, v, lr, b1, b2,
                       eps, wd, bc1, bc2s, grad_scale, coef, ema, ema_decay);
  else
    hipLaunchKernelGGL(adam_ex_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, p, g, m, v, lr, b1, b2,
                       eps, wd, bc1, bc2s, grad_scale, coef, ema, ema_decay);
  MER_LAUNCH_CHECK();
}
