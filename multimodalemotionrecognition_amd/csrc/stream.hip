// Live streaming sessions (streaming.py): per-session device rings that are written once and read by every window.
//   * resample_stream: a rational polyphase resampler (scipy resample_poly's filter, host/mer_io.cpp mer_resample)
//     that carries its state across chunks and writes its outputs straight into the session's audio ring;
//   * ring_windows: the last min(count, target) samples of B rings, in time order across the wrap, zero-padded at the
//     end (the reference's crop-from-the-end / pad-at-the-end, preprocess.py:319-323), one launch for B sessions;
//   * rows_scatter: dst[idx[r]] = src[r] for fp32 rows -- freshly encoded frame features into the feature ring.
// Every descriptor is validated on the host (here for the scalar arguments, in the Python wrappers for the device
// arrays); the kernels also clamp, so no launch reads or writes outside its buffers whatever the arrays hold.
#include "common.h"
#include "mer.h"
#include "resample.h"

namespace {

// outputs a stream of n inputs has emitted: every o whose newest input floor((o * down + half) / up) has arrived
__host__ __device__ __forceinline__ long rs_emitted(long n, long up, long down) {
  if (up == 1 && down == 1) return n;
  const long a = n * up - rs_half(up, down) - 1;
  return a < 0 ? 0 : a / down + 1;
}

// The virtual input V = [hist | chunk]: V[j] is global input n_in - hist_len + j; before the stream start (kept as
// zeros in hist) and anywhere outside V it is 0.
__device__ __forceinline__ float rs_input(long g, long n_in, int hist_len, const float* __restrict__ hist,
                                          const float* __restrict__ chunk, long n_chunk) {
  const long j = g - (n_in - hist_len);
  if (j < 0) return 0.f;
  if (j < hist_len) return hist[j];
  return j - hist_len < n_chunk ? chunk[j - hist_len] : 0.f;
}

// Output o = out0 + i through rs_output (resample.h): its order and operands depend on o alone, so any chunking gives
// the same bits.  The workgroup's inputs [lo, lo + span) are staged in LDS.
__global__ __launch_bounds__(RS_BLOCK) void resample_stream_kernel(
    int up, int down, int kmax, const float* __restrict__ table, const float* __restrict__ chunk, long n_chunk,
    long n_in, long out0, long n_out, const float* __restrict__ hist, int hist_len, float* __restrict__ ring, long cap,
    int span) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const long i0 = (long)blockIdx.x * RS_BLOCK;
  const long lo = rs_lo(out0 + i0, up, down, kmax);
  for (int j = threadIdx.x; j < span; j += RS_BLOCK) rs_lds[j] = rs_input(lo + j, n_in, hist_len, hist, chunk, n_chunk);
  __syncthreads();
  const long i = i0 + threadIdx.x;
  if (i >= n_out) return;
  const float acc = rs_output(out0 + i, up, down, kmax, table, rs_lds, lo, span);
  if (i >= n_out - cap) ring[(out0 + i) % cap] = acc;  // a chunk longer than the ring keeps its last cap outputs
}

__global__ __launch_bounds__(256) void resample_copy_kernel(const float* __restrict__ chunk, long n_chunk, long out0,
                                                            float* __restrict__ ring, long cap) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_chunk && i >= n_chunk - cap) ring[(out0 + i) % cap] = chunk[i];
}

// The second, tiny launch: the last hist_len entries of V into the OTHER history buffer (the resampling launch and
// this one both read the old buffer, so neither orders against the other), and the two global counts.
__global__ __launch_bounds__(256) void resample_state_kernel(const float* __restrict__ chunk, long n_chunk, long n_in,
                                                             const float* __restrict__ hist, float* __restrict__ hist_new,
                                                             int hist_len, long n_out_after, long* __restrict__ counts) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0) {  // block 0's first thread alone
    counts[0] = n_in + n_chunk;
    counts[1] = n_out_after;
  }
  if (j < hist_len) hist_new[j] = rs_input(n_in + n_chunk - hist_len + j, n_in, hist_len, hist, chunk, n_chunk);
}

__device__ __forceinline__ long clamp_long(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void ring_windows_kernel(long target, const float* __restrict__ rings, int n_slots,
                                                           long cap, const long* __restrict__ slot,
                                                           const long* __restrict__ end, const long* __restrict__ count,
                                                           float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= target) return;
  const long s = clamp_long(slot[b], 0, n_slots - 1), e = clamp_long(end[b], 0, cap - 1);
  long n = clamp_long(count[b], 0, cap);
  n = n < target ? n : target;
  float v = 0.f;
  if (i < n) {
    long at = e - n + i;  // in (-cap, cap)
    if (at < 0) at += cap;
    v = rings[s * cap + at];
  }
  out[(long)b * target + i] = v;
}

__device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// one thread per 16 bytes of the source
__global__ __launch_bounds__(256) void rows_scatter_vec4_kernel(long total, int n_dst, int d4,
                                                                const float4* __restrict__ src,
                                                                const int* __restrict__ idx, float4* __restrict__ dst) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long r = t / d4;
  const int c = (int)(t - r * d4);
  dst[(long)clamp_index(idx[r], n_dst) * d4 + c] = src[t];
}

__global__ __launch_bounds__(256) void rows_scatter_scalar_kernel(long total, int n_dst, int D,
                                                                  const float* __restrict__ src,
                                                                  const int* __restrict__ idx, float* __restrict__ dst) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long r = t / D;
  const int c = (int)(t - r * D);
  dst[(long)clamp_index(idx[r], n_dst) * D + c] = src[t];
}

}  // namespace

MER_API int mer_resample_stream(int up, int down, int kmax, const float* table, const float* chunk, long n_chunk,
                                long n_in, const float* hist, float* hist_new, int hist_len, float* ring, long cap,
                                long* counts, void* stream) {
  if (n_chunk == 0) return 0;
  if (up <= 0 || down <= 0 || n_chunk < 0 || n_in < 0 || cap <= 0 || !chunk || !ring || !counts)
    return (int)hipErrorInvalidValue;
  if (n_in + n_chunk > (1L << 40) || up > (1 << 20) || down > (1 << 20)) return (int)hipErrorInvalidValue;  // (long products)
  const long out0 = rs_emitted(n_in, up, down), n_out = rs_emitted(n_in + n_chunk, up, down) - out0;
  if (up == 1 && down == 1) {
    const long blocks = (n_chunk + 255) / 256;
    if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, chunk, n_chunk,
                       out0, ring, cap);
    hipLaunchKernelGGL(resample_state_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, chunk, n_chunk, n_in,
                       (const float*)nullptr, (float*)nullptr, 0, out0 + n_out, counts);
    MER_LAUNCH_CHECK();
  }
  const long half = rs_half(up, down);
  // hist_len inputs reach back to the oldest input the next output can need: ceil(2 * half / up) <= kmax
  if (kmax != (int)(2 * half / up) + 1 || hist_len != kmax || !table || !hist || !hist_new || hist == hist_new)
    return (int)hipErrorInvalidValue;
  const long span = rs_span(up, down, kmax);
  if (span > RS_MAX_SPAN) return (int)hipErrorInvalidValue;
  if (n_out > 0) {
    const long blocks = (n_out + RS_BLOCK - 1) / RS_BLOCK;
    if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_stream_kernel, dim3((unsigned)blocks), dim3(RS_BLOCK), (size_t)span * sizeof(float),
                       (hipStream_t)stream, up, down, kmax, table, chunk, n_chunk, n_in, out0, n_out, hist, hist_len,
                       ring, cap, (int)span);
  }
  hipLaunchKernelGGL(resample_state_kernel, dim3((hist_len + 255) / 256), dim3(256), 0, (hipStream_t)stream, chunk,
                     n_chunk, n_in, hist, hist_new, hist_len, out0 + n_out, counts);
  MER_LAUNCH_CHECK();
}

MER_API int mer_ring_windows(int B, long target, const float* rings, int n_slots, long cap, const long* slot,
                             const long* end, const long* count, float* out, void* stream) {
  if (B <= 0 || target == 0) return 0;
  if (target < 0 || n_slots <= 0 || cap <= 0 || !rings || !slot || !end || !count || !out)
    return (int)hipErrorInvalidValue;
  const long bx = (target + 255) / 256;
  if (bx > 0x7fffffffL || B > 65535) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(ring_windows_kernel, dim3((unsigned)bx, B), dim3(256), 0, (hipStream_t)stream, target, rings,
                     n_slots, cap, slot, end, count, out);
  MER_LAUNCH_CHECK();
}

MER_API int mer_rows_scatter(int n_dst, int n_rows, int D, const float* src, const int* idx, float* dst, void* stream) {
  if (n_rows <= 0 || D == 0) return 0;
  if (n_dst <= 0 || D < 0 || !src || !idx || !dst) return (int)hipErrorInvalidValue;
  const bool vec = D % 4 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0;
  const long total = (long)n_rows * (vec ? D / 4 : D);
  const long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (vec)
    hipLaunchKernelGGL(rows_scatter_vec4_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total,
                       n_dst, D / 4, (const float4*)src, idx, (float4*)dst);
  else
    hipLaunchKernelGGL(rows_scatter_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total,
                       n_dst, D, src, idx, dst);
  MER_LAUNCH_CHECK();
}
