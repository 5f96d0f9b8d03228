// Emotion timeline over a long recording (timeline.py): the device-side assembly of overlapping windows whose
// frames are encoded once.
//   * frames_gather_resize_normalize: the preprocessing of csrc/clips.hip reading source frame idx[n] of the decoded
//     recording for output n -- the recording's unique sampled frames in one launch, no gathered uint8 copy;
//   * rows_gather: out[r] = src[idx[r]] for fp32 rows -- the [U, 512] frame features to the [Nw * T, 512] window slots;
//   * timeline_smooth: centred moving average of the per-window probabilities + the per-window argmax.
// The audio windows need no kernel of their own: mer_wav_pad_crop already reads (offset, length) rows of one packed
// buffer, and overlapping windows are offsets into the one recording.
// Every index array is validated on the host by the Python wrappers; the kernels also clamp each index into range, so
// no launch can read outside its source whatever the array holds.
#include "common.h"
#include "frame_resize.h"
#include "mer.h"

namespace {

__device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__global__ __launch_bounds__(256) void frames_gather_resize_normalize_kernel(
    int n_src, int H0, int W0, int S, const uint8_t* __restrict__ src, long frame_stride, const int* __restrict__ idx,
    int n0, double scale_y, double scale_x, FrameNorm nm, float* __restrict__ dst) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = n0 + blockIdx.z;
  if (x >= S) return;
  const int f = clamp_index(idx[n], n_src);
  resize_normalize_pixel(src + (long)f * frame_stride, (long)W0 * 3, H0, W0, S, x, y, n, scale_y, scale_x, nm, dst);
}

// one thread per 16 bytes of the output
__global__ __launch_bounds__(256) void rows_gather_vec4_kernel(long total, int n_src, int d4,
                                                               const float4* __restrict__ src,
                                                               const int* __restrict__ idx, float4* __restrict__ out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long r = t / d4;
  const int c = (int)(t - r * d4);
  out[t] = src[(long)clamp_index(idx[r], n_src) * d4 + c];
}

__global__ __launch_bounds__(256) void rows_gather_scalar_kernel(long total, int n_src, int D,
                                                                 const float* __restrict__ src,
                                                                 const int* __restrict__ idx, float* __restrict__ out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long r = t / D;
  const int c = (int)(t - r * D);
  out[t] = src[(long)clamp_index(idx[r], n_src) * D + c];
}

// One thread per window: class by class, the sum over windows [w - r, w + r] clipped to [0, Nw) in ascending window
// order (a fixed order: the result does not depend on the launch shape), divided by the number of windows summed.
// The running best keeps the lowest class index on ties.  r = 0: the sum is the one value, the divisor 1.
__global__ __launch_bounds__(256) void timeline_smooth_kernel(int Nw, int C, int radius, const float* __restrict__ probs,
                                                              float* __restrict__ smoothed, int* __restrict__ top1) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= Nw) return;
  const int lo = w - radius < 0 ? 0 : w - radius;
  const int hi = radius >= Nw - 1 - w ? Nw - 1 : w + radius;  // (w + radius cannot overflow: only taken when small)
  const float cnt = (float)(hi - lo + 1);
  float best = 0.f;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    float s = probs[(long)lo * C + c];
    for (int k = lo + 1; k <= hi; ++k) s += probs[(long)k * C + c];
    s = s / cnt;
    smoothed[(long)w * C + c] = s;
    if (c == 0 || s > best) {
      best = s;
      arg = c;
    }
  }
  top1[w] = arg;
}

}  // namespace

MER_API int mer_frames_gather_resize_normalize(int n_src, int H0, int W0, const void* frames, long frame_stride,
                                               int n_out, const int* idx, int S, float mean0, float mean1, float mean2,
                                               float std0, float std1, float std2, float* out, void* stream) {
  if (n_out <= 0) return 0;
  if (n_src <= 0 || H0 <= 0 || W0 <= 0 || S <= 0 || frame_stride < (long)H0 * W0 * 3 || !frames || !idx || !out)
    return (int)hipErrorInvalidValue;
  const double sy = 1.0 / ((double)S / H0), sx = 1.0 / ((double)S / W0);  // cv::resize: 1 / inv_scale
  const FrameNorm nm{mean0, mean1, mean2, std0, std1, std2};
  for (int n0 = 0; n0 < n_out; n0 += 65535) {  // grid z holds at most 65535 frames: one launch up to there
    const int nz = n_out - n0 < 65535 ? n_out - n0 : 65535;
    hipLaunchKernelGGL(frames_gather_resize_normalize_kernel, dim3((S + 255) / 256, S, nz), dim3(256), 0,
                       (hipStream_t)stream, n_src, H0, W0, S, (const uint8_t*)frames, frame_stride, idx, n0, sy, sx, nm,
                       out);
  }
  MER_LAUNCH_CHECK();
}

MER_API int mer_rows_gather(int n_src, int n_out, int D, const float* src, const int* idx, float* out, void* stream) {
  if (n_out <= 0 || D == 0) return 0;
  if (n_src <= 0 || D < 0 || !src || !idx || !out) return (int)hipErrorInvalidValue;
  const bool vec = D % 4 == 0 && ((uintptr_t)src | (uintptr_t)out) % 16 == 0;
  const long total = (long)n_out * (vec ? D / 4 : D);
  const long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (vec)
    hipLaunchKernelGGL(rows_gather_vec4_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total, n_src,
                       D / 4, (const float4*)src, idx, (float4*)out);
  else
    hipLaunchKernelGGL(rows_gather_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total,
                       n_src, D, src, idx, out);
  MER_LAUNCH_CHECK();
}

MER_API int mer_timeline_smooth(int Nw, int C, int radius, const float* probs, float* smoothed, int* top1,
                                void* stream) {
  if (Nw <= 0) return 0;
  if (C <= 0 || radius < 0 || !probs || !smoothed || !top1 || probs == smoothed) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(timeline_smooth_kernel, dim3((Nw + 255) / 256), dim3(256), 0, (hipStream_t)stream, Nw, C, radius,
                     probs, smoothed, top1);
  MER_LAUNCH_CHECK();
}
