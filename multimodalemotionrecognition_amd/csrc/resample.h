// The polyphase resampler's per-output arithmetic, shared by the streaming kernel (stream.hip) and the batched
// whole-clip kernel (audio_clips.hip): both call rs_output, so a stream and a clip give the same bits by construction.
#pragma once
#include <hip/hip_runtime.h>

constexpr int RS_BLOCK = 256;            // outputs per workgroup, one thread each
constexpr long RS_MAX_SPAN = 12288;      // floats of LDS one workgroup may stage (48 KB)

__host__ __device__ __forceinline__ long rs_half(long up, long down) { return 10 * (up > down ? up : down); }
// inputs one workgroup stages: the newest inputs of RS_BLOCK consecutive outputs, plus kmax - 1 older ones
__host__ __device__ __forceinline__ long rs_span(long up, long down, long kmax) {
  return (long)(RS_BLOCK - 1) * down / up + 1 + kmax;
}
// first input a workgroup whose first output is o0 stages
__device__ __forceinline__ long rs_lo(long o0, int up, int down, int kmax) {
  return (o0 * down + rs_half(up, down)) / up - (kmax - 1);
}

// Output o: m = o * down + half is its centre in the upsampled signal, phase p = m % up, newest input x = m / up;
// acc = sum over t < taps(p) of table[p][t] * input[x - t], t ascending (newest input first), one fmaf per tap, from
// 0.f: the order and the operands depend on o alone.  lds holds the inputs [lo, lo + span), zeros where the signal
// has none.
__device__ __forceinline__ float rs_output(long o, int up, int down, int kmax, const float* __restrict__ table,
                                           const float* lds, long lo, int span) {
  const long half = rs_half(up, down);
  const long m = o * down + half;
  const long x = m / up;
  const int p = (int)(m - x * up);
  const int taps = (int)((2 * half - p) / up) + 1;  // taps k = p + t * up <= 2 * half
  const float* __restrict__ h = table + (long)p * kmax;
  int at = (int)(x - lo);  // < span: x <= the block's last output's newest input
  float acc = 0.f;
  for (int t = 0; t < taps && t < kmax; ++t, --at) acc = fmaf(h[t], at >= 0 && at < span ? lds[at] : 0.f, acc);
  return acc;
}
