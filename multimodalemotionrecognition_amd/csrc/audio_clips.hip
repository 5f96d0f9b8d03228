// Audio clip assembly on the device (clips.assemble_waveforms): what load_audio_wav does after decoding the WAV.
//   * resample_clips: B ragged clips at one input rate -> [B][target] at the output rate, resampled (scipy
//     resample_poly's filter, host/mer_io.cpp mer_resample) and zero-padded / cropped in one launch.  The per-output
//     arithmetic is rs_output (resample.h), the streaming resampler's: a clip and a stream give the same bits.
//   * mix_noise_clips: the train-split noise mix (ravdess.py:539-576) of a [B][target] batch -- per-block fp64 power
//     partials, a fixed-order fold to one scale per clip, then clamp(wav + noise * scale).
// One thread per output, coalesced 4-byte loads and stores: the resampler does 2 * half / up + 1 LDS reads and fmafs
// per output (61 at 48 kHz), so it is bound by those, not by its one store; the mix passes stream 12 bytes per sample.
// Scalar arguments are checked here, the per-clip descriptor arrays by the Python wrapper on the host; the kernels
// clamp as well, so no launch reads or writes outside its buffers whatever the arrays hold.
#include "common.h"
#include "mer.h"
#include "resample.h"

namespace {

constexpr int MIX_BLOCK = 256;  // samples per power partial

__device__ __forceinline__ long clip_outputs(long len, long up, long down) { return (len * up + down - 1) / down; }

// Block (x, b): outputs [x * 256, x * 256 + 256) of clip b.  The staged span is read from THIS clip's
// [offset, offset + len) alone: everything else is zero, whatever lies next to the clip in the packed buffer.
__global__ __launch_bounds__(RS_BLOCK) void resample_clips_kernel(long target, int up, int down, int kmax,
                                                                  const float* __restrict__ table,
                                                                  const float* __restrict__ packed,
                                                                  const long* __restrict__ offsets,
                                                                  const long* __restrict__ lengths,
                                                                  float* __restrict__ out, int span) {
  extern __shared__ __attribute__((aligned(16))) float rc_lds[];
  const int b = blockIdx.y;
  const long len = lengths[b] > 0 ? lengths[b] : 0;
  const long nout = clip_outputs(len, up, down), keep = nout < target ? nout : target;
  const long i0 = (long)blockIdx.x * RS_BLOCK, i = i0 + threadIdx.x;
  float* __restrict__ row = out + (long)b * target;
  if (i0 >= keep) {  // the whole block lies in the pad (uniform over the block: no barrier is skipped by a part of it)
    if (i < target) row[i] = 0.f;
    return;
  }
  const float* __restrict__ src = packed + offsets[b];
  const long lo = rs_lo(i0, up, down, kmax);
  for (int j = threadIdx.x; j < span; j += RS_BLOCK) {
    const long g = lo + j;
    rc_lds[j] = g >= 0 && g < len ? src[g] : 0.f;
  }
  __syncthreads();
  if (i >= target) return;
  row[i] = i < keep ? rs_output(i, up, down, kmax, table, rc_lds, lo, span) : 0.f;
}

__global__ __launch_bounds__(256) void copy_clips_kernel(long target, const float* __restrict__ packed,
                                                         const long* __restrict__ offsets,
                                                         const long* __restrict__ lengths, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= target) return;
  out[(long)b * target + i] = i < lengths[b] ? packed[offsets[b] + i] : 0.f;
}

__device__ __forceinline__ long noise_at(long start, long i, long n_noise) {
  return (long)((unsigned long)((start > 0 ? start : 0) + i) % (unsigned long)n_noise);
}

// Pass A: parts[b][x] = (sum wav^2, sum v^2) over samples [x * 256, x * 256 + 256) of row b, in fp64; v is the noise
// sample the mix will add (mode 1), 0 otherwise.  The block's tree has a fixed shape, so the sums are reproducible.
__global__ __launch_bounds__(MIX_BLOCK) void mix_power_kernel(long target, const float* __restrict__ wav,
                                                              const int* __restrict__ mode,
                                                              const long* __restrict__ start,
                                                              const float* __restrict__ noise, long n_noise,
                                                              double* __restrict__ parts) {
  __shared__ double s_w[MIX_BLOCK], s_n[MIX_BLOCK];
  const int b = blockIdx.y, md = mode[b];
  const long i = (long)blockIdx.x * MIX_BLOCK + threadIdx.x;
  double w = 0.0, v = 0.0;
  if (md != 0 && i < target) {
    w = (double)wav[(long)b * target + i];
    if (md == 1 && n_noise > 0) v = (double)noise[noise_at(start[b], i, n_noise)];
  }
  s_w[threadIdx.x] = w * w;
  s_n[threadIdx.x] = v * v;
  __syncthreads();
  for (int s = MIX_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      s_w[threadIdx.x] += s_w[threadIdx.x + s];
      s_n[threadIdx.x] += s_n[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* o = parts + ((long)b * gridDim.x + blockIdx.x) * 2;
    o[0] = s_w[0];
    o[1] = s_n[0];
  }
}

// One thread per clip folds its partials in block order: ps, pn (means over target), then the host's rule
// (mer_mix_noise).  scale[b]: mode 1 the factor on the noise track, mode 2 the Gaussian sigma, mode 0 zero.
__global__ __launch_bounds__(256) void mix_scale_kernel(int B, long target, int nblk, const int* __restrict__ mode,
                                                        const float* __restrict__ snr_db,
                                                        const double* __restrict__ parts, float* __restrict__ scale) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double ps = 0.0, pn = 0.0;
  for (int x = 0; x < nblk; ++x) {
    ps += parts[((long)b * nblk + x) * 2];
    pn += parts[((long)b * nblk + x) * 2 + 1];
  }
  ps /= (double)target;
  pn /= (double)target;
  const double snr = pow(10.0, (double)snr_db[b] / 10.0);
  const double want = ps / (snr > 1e-8 ? snr : 1e-8);
  float s = 0.f;
  if (mode[b] == 1) s = pn > 1e-8 ? (float)sqrt(want / pn) : 1.f;
  else if (mode[b] == 2) s = (float)sqrt(want);
  scale[b] = s;
}

// Pass B.  Mode 1: clamp(fl(wav + fl(noise * scale)), -1, 1); mode 2: the same with noise = ztable[hash(seed, i) >> 16]
// (the video augmentation's 16-bit Gaussian) and scale = sigma; mode 0: a copy, NOT clamped.
__global__ __launch_bounds__(256) void mix_apply_kernel(long target, const float* __restrict__ wav,
                                                        const int* __restrict__ mode, const long* __restrict__ start,
                                                        const unsigned long long* __restrict__ seed,
                                                        const float* __restrict__ noise, long n_noise,
                                                        const float* __restrict__ ztable,
                                                        const float* __restrict__ scale, float* __restrict__ out) {
#pragma clang fp contract(off)  // fl(wav + fl(noise * scale)), never an fma (the host's and numpy's order)
  const int b = blockIdx.y, md = mode[b];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= target) return;
  float v = wav[(long)b * target + i];
  if (md == 1 || md == 2) {
    float nz = 0.f;
    if (md == 2) nz = ztable[mer_hash(seed[b], (uint64_t)i) >> 16];
    else if (n_noise > 0) nz = noise[noise_at(start[b], i, n_noise)];
    v = v + nz * scale[b];
    v = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
  }
  out[(long)b * target + i] = v;
}

}  // namespace

MER_API int mer_resample_clips(int B, long target, int up, int down, int kmax, const float* table, const float* packed,
                               const long* offsets, const long* lengths, float* out, void* stream) {
  if (B <= 0 || target == 0) return 0;
  if (target < 0 || up <= 0 || down <= 0 || !packed || !offsets || !lengths || !out) return (int)hipErrorInvalidValue;
  if (up > (1 << 20) || down > (1 << 20) || target > (1L << 40)) return (int)hipErrorInvalidValue;  // (long products)
  const long bx = (target + RS_BLOCK - 1) / RS_BLOCK;
  if (bx > 0x7fffffffL || B > 65535) return (int)hipErrorInvalidValue;
  if (up == 1 && down == 1) {
    hipLaunchKernelGGL(copy_clips_kernel, dim3((unsigned)bx, B), dim3(256), 0, (hipStream_t)stream, target, packed,
                       offsets, lengths, out);
    MER_LAUNCH_CHECK();
  }
  const long half = rs_half(up, down);
  if (kmax != (int)(2 * half / up) + 1 || !table) return (int)hipErrorInvalidValue;
  const long span = rs_span(up, down, kmax);
  if (span > RS_MAX_SPAN) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(resample_clips_kernel, dim3((unsigned)bx, B), dim3(RS_BLOCK), (size_t)span * sizeof(float),
                     (hipStream_t)stream, target, up, down, kmax, table, packed, offsets, lengths, out, (int)span);
  MER_LAUNCH_CHECK();
}

MER_API int mer_mix_noise_clips(int B, long target, const float* wav, const int* mode, const long* start,
                                const float* snr_db, const unsigned long long* seed, const float* noise, long n_noise,
                                const float* ztable, double* parts, float* scale, float* out, void* stream) {
  if (B <= 0 || target == 0) return 0;
  if (target < 0 || n_noise < 0 || !wav || !mode || !start || !snr_db || !seed || !ztable || !parts || !scale || !out ||
      (n_noise > 0 && !noise))
    return (int)hipErrorInvalidValue;
  const long bx = (target + MIX_BLOCK - 1) / MIX_BLOCK;
  if (bx > 0x7fffffffL || B > 65535) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(mix_power_kernel, dim3((unsigned)bx, B), dim3(MIX_BLOCK), 0, (hipStream_t)stream, target, wav,
                     mode, start, noise, n_noise, parts);
  hipLaunchKernelGGL(mix_scale_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, target, (int)bx,
                     mode, snr_db, parts, scale);
  hipLaunchKernelGGL(mix_apply_kernel, dim3((unsigned)bx, B), dim3(256), 0, (hipStream_t)stream, target, wav, mode,
                     start, seed, noise, n_noise, ztable, scale, out);
  MER_LAUNCH_CHECK();
}
