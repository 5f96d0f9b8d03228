// Packing kernels of the ResNet18 trunk: video frames and conv weights into the layouts conv.hip reads.
#include "common.h"
#include "mer.h"

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// ---------------------------------------------------------------------------------------
// Packing kernels
// ---------------------------------------------------------------------------------------
// video frames NCHW fp32 -> NHWC bf16 with channels zero-padded to Cp
// one frame per blockIdx.y; Cp == 8: one 16-byte store per pixel
__global__ void pack_input_kernel(int C, int HW, const float* __restrict__ x, bf16_t* __restrict__ y) {
  const int n = blockIdx.y;
  const float* xn = x + (long)n * C * HW;
  u32x4* yn = reinterpret_cast<u32x4*>(y + (long)n * HW * 8);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    u32x4 o = {0u, 0u, 0u, 0u};
    bf16_t* oh = reinterpret_cast<bf16_t*>(&o);
    for (int c = 0; c < C; ++c) oh[c] = f2bf(xn[(long)c * HW + p]);
    yn[p] = o;
  }
}
MER_API int mer_pack_input_nhwc(int N, int C, int H, int W, int Cp, const float* x, void* y, void* stream) {
  if (Cp != 8 || C > 8) return (int)hipErrorInvalidValue;
  const int HW = H * W;
  dim3 grid((HW + 255) / 256 < 64 ? (HW + 255) / 256 : 64, N);
  hipLaunchKernelGGL(pack_input_kernel, grid, dim3(256), 0, (hipStream_t)stream, C, HW, x, (bf16_t*)y);
  MER_LAUNCH_CHECK();
}

// Space-to-depth stem input (ResNet conv1: 7x7, stride 2, pad 3 on C <= 4 channels, H and W even):
// fp32 NCHW [N][C][H][W] -> bf16 [N][H/2+3][W/2+3][16], pixel (j, i) = 2x2 block (j-2, i-2) of the frame
// with channel (dy*2 + dx)*C + c (zero for the 2 leading / 1 trailing border rows and columns and for
// channels >= 4C).  The stride-2 7x7 conv then is a stride-1 4x4 conv with no padding on 16 channels
// (K = 256 instead of 7*7*8 = 392 for the 8-channel-padded direct form); weights: pack mode 2 below.
template <int C>  // compile-time channel count: the (dy, dx, c) -> s2d channel map unrolls to fixed registers
__global__ void pack_input_s2d_kernel(int N, int H, int W, const float* __restrict__ x, bf16_t* __restrict__ y) {
  const int Hs = H / 2 + 3, Ws = W / 2 + 3;
  const int total = N * Hs * Ws;  // (< 2^22, checked on the host: 32-bit index math, exact float-reciprocal divides --
                                  // the 64-bit divisions of a long index were most of this kernel's time)
  const float inv_Ws = 1.f / Ws, inv_Hs = 1.f / Hs;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
    const int q = fdiv(p, inv_Ws);
    const int i = p - q * Ws;
    const int n = fdiv(q, inv_Hs);
    const int j = q - n * Hs;
    uint32_t o[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const int jj = j - 2, ii = i - 2;
    if (jj >= 0 && jj < H / 2 && ii >= 0 && ii < W / 2) {
      // the 2x2 block's two rows of each channel as float2 loads (adjacent lanes read adjacent 8-byte pairs: one
      // coalesced 512-byte run per wave instruction)
      const float* xn = x + (long)n * C * H * W + (long)(2 * jj) * W + 2 * ii;
      float v[C][4];  // [c][dydx]
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
          const float2 q2 = *reinterpret_cast<const float2*>(xn + (long)c * H * W + dy * W);
          v[c][2 * dy] = q2.x;
          v[c][2 * dy + 1] = q2.y;
        }
#pragma unroll
      for (int ch = 0; ch < 4 * C; ++ch)
        o[ch >> 1] |= (uint32_t)f2bf(v[ch % C][ch / C]) << ((ch & 1) * 16);
    }
    u32x4* dst = reinterpret_cast<u32x4*>(y + (long)p * 16);
    dst[0] = u32x4{o[0], o[1], o[2], o[3]};
    dst[1] = u32x4{o[4], o[5], o[6], o[7]};
  }
}
MER_API int mer_pack_input_s2d(int N, int C, int H, int W, const float* x, void* y, void* stream) {
  if (C < 1 || C > 4 || (H & 1) || (W & 1) || ((uintptr_t)x & 7)) return (int)hipErrorInvalidValue;
  const long per_frame = (long)(H / 2 + 3) * (W / 2 + 3);
  if (N < 0 || per_frame >= (1L << 22)) return (int)hipErrorInvalidValue;
  // the kernel's fdiv index math holds below 2^22 pixels per launch: larger batches go in frame chunks
  const int chunk = (int)(((1L << 22) - 1) / per_frame);
  const hipStream_t st = (hipStream_t)stream;
  for (int n0 = 0; n0 < N; n0 += chunk) {
    const int nc = N - n0 < chunk ? N - n0 : chunk;
    const long total = (long)nc * per_frame;
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    const float* xc = x + (long)n0 * C * H * W;
    bf16_t* yc = (bf16_t*)y + n0 * per_frame * 16;
    if (C == 3) hipLaunchKernelGGL(pack_input_s2d_kernel<3>, dim3(grid), dim3(256), 0, st, nc, H, W, xc, yc);
    else if (C == 1) hipLaunchKernelGGL(pack_input_s2d_kernel<1>, dim3(grid), dim3(256), 0, st, nc, H, W, xc, yc);
    else if (C == 2) hipLaunchKernelGGL(pack_input_s2d_kernel<2>, dim3(grid), dim3(256), 0, st, nc, H, W, xc, yc);
    else hipLaunchKernelGGL(pack_input_s2d_kernel<4>, dim3(grid), dim3(256), 0, st, nc, H, W, xc, yc);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// PyTorch conv weight [K][C][R][S] fp32 -> fwd [K][R][S][Cp] (transpose=0) or dgrad [Cp][R][S][Kp] (transpose=1)
__global__ void pack_w_kernel(int K, int C, int R, int S, int Cp, int transpose, const float* __restrict__ w,
                              bf16_t* __restrict__ out) {
  const long total = (long)K * R * S * Cp;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int k, r, s, c;
    if (!transpose) {
      c = e % Cp; long q = e / Cp; s = q % S; q /= S; r = q % R; k = q / R;
    } else {
      k = e % K; long q = e / K; s = q % S; q /= S; r = q % R; c = q / R;
    }
    out[e] = c < C ? f2bf(w[(((long)k * C + c) * R + r) * S + s]) : (bf16_t)0;
  }
}
MER_API int mer_pack_conv_weight(int K, int C, int R, int S, int Cp, int transpose, const float* w, void* out,
                                 void* stream) {
  const long total = (long)K * R * S * Cp;
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(pack_w_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, K, C, R, S, Cp, transpose, w,
                     (bf16_t*)out);
  MER_LAUNCH_CHECK();
}

// All of a trunk's weight packs in ONE launch (the per-step re-pack in training is ~40 small layouts
// whose separate launches cost more than their bytes).  desc: n records of 9 int64 =
// {w, out, K, C, R, S, Cp, transpose (0, 1, or 2 = space-to-depth stem), first element (unused here)};
// grid.y = record.  Both layouts go
// through an LDS tile so global reads AND writes are contiguous runs:
//   transpose 0: block = one output channel k: w[k][c][rs] (C*RS contiguous floats) -> out[k][rs][c<Cp];
//   transpose 1: block = (input channel c, 64 output channels k0..): w[k][c][rs] (runs of RS) ->
//                out[c][rs][k0..k0+63].
// FLAT: one-dimensional grid over every record's blocks (column 8 = the record's first block): no idle blocks (the
// 2-D form launches 4,096 blocks per record, most of which only exit -- that dispatch was most of its time)
template <bool FLAT>
__global__ __launch_bounds__(256) void pack_w_batched_kernel(const long long* __restrict__ desc, int n) {
  __shared__ float tile[4608];  // max C*RS (512 * 9) or 64 * RS (RS <= 49 -> 3136)
  int rec = FLAT ? 0 : (int)blockIdx.y;
  if (FLAT)
    for (int i = 1; i < n; ++i)
      if (desc[i * 9 + 8] <= (long long)blockIdx.x) rec = i;
  const long long* r = desc + rec * 9;
  const int bx = FLAT ? (int)(blockIdx.x - r[8]) : (int)blockIdx.x;
  const float* w = reinterpret_cast<const float*>(r[0]);
  bf16_t* out = reinterpret_cast<bf16_t*>(r[1]);
  const int K = (int)r[2], C = (int)r[3], RS = (int)(r[4] * r[5]), Cp = (int)r[6];
  if (r[7] == 3) {  // transposed pack from the forward bf16 pack: src [K][RS][C] -> out [C][RS][K] (C, K % 64 == 0)
    // block = (tap, 64-channel tile, 64-output tile): 16-byte loads of 64 k-rows into LDS, 16-byte stores of 64 c-rows
    const uint16_t* src = reinterpret_cast<const uint16_t*>(r[0]);
    uint16_t* lds = reinterpret_cast<uint16_t*>(tile);  // [64 k][72] (row pad spreads the column gathers)
    const int kbn = K >> 6, cbn = C >> 6;
    const int rs = bx / (kbn * cbn), rem = bx - rs * kbn * cbn, cb = rem / kbn, kb = rem - cb * kbn;
    if (rs >= RS) return;
    const int k0 = kb * 64, c0 = cb * 64;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = threadIdx.x + 256 * j, kk = i >> 3, ch = (i & 7) * 8;
      const uint4 v = *reinterpret_cast<const uint4*>(src + ((long)(k0 + kk) * RS + rs) * C + c0 + ch);
      *reinterpret_cast<uint4*>(lds + kk * 72 + ch) = v;
    }
    __syncthreads();
    uint16_t* ob = reinterpret_cast<uint16_t*>(out);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = threadIdx.x + 256 * j, cc = i >> 3, kc = (i & 7) * 8;
      uint32_t pk[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        pk[e] = (uint32_t)lds[(kc + 2 * e) * 72 + cc] | ((uint32_t)lds[(kc + 2 * e + 1) * 72 + cc] << 16);
      *reinterpret_cast<uint4*>(ob + ((long)(c0 + cc) * RS + rs) * K + k0 + kc) = uint4{pk[0], pk[1], pk[2], pk[3]};
    }
    return;
  }
  if (r[7] == 2) {  // space-to-depth stem: out[k][ry][rx][ch], tap (r, s) = (2ry+dy-1, 2rx+dx-1), ch = (dy*2+dx)*C + c
    const int k = bx;
    const int R = (int)r[4], S = (int)r[5], Ro = (R + 2) / 2, So = (S + 2) / 2;
    if (k >= K) return;
    const float* src = w + (long)k * C * RS;
    for (int i = threadIdx.x; i < C * RS; i += 256) tile[i] = src[i];
    __syncthreads();
    bf16_t* dst = out + (long)k * Ro * So * Cp;
    for (int i = threadIdx.x; i < Ro * So * Cp; i += 256) {
      const int ch = i % Cp, q = i / Cp, rx = q % So, ry = q / So;
      const int dydx = ch / C, c = ch - dydx * C;
      const int rr = 2 * ry + (dydx >> 1) - 1, ss = 2 * rx + (dydx & 1) - 1;
      const bool ok = dydx < 4 && rr >= 0 && rr < R && ss >= 0 && ss < S;
      dst[i] = ok ? f2bf(tile[c * RS + rr * S + ss]) : (bf16_t)0;
    }
  } else if (!r[7]) {
    const int k = bx;
    if (k >= K) return;
    const float* src = w + (long)k * C * RS;
    const int n = C * RS;
    if ((n & 3) == 0 && (((uintptr_t)src) & 15) == 0) {
      for (int i = threadIdx.x; i < n / 4; i += 256)
        reinterpret_cast<f32x4*>(tile)[i] = reinterpret_cast<const f32x4*>(src)[i];  // [c][rs]
    } else {
      for (int i = threadIdx.x; i < n; i += 256) tile[i] = src[i];
    }
    __syncthreads();
    bf16_t* dst = out + (long)k * RS * Cp;
    // 8 consecutive channels of one tap per thread, one 16-byte store (Cp % 8 == 0); i / Cp by reciprocal
    const float inv_Cp = 1.f / Cp;
    for (int i = threadIdx.x; i < RS * Cp / 8; i += 256) {  // i*8 = rs*Cp + c0
      const int rs = fdiv(i * 8, inv_Cp), c0 = i * 8 - rs * Cp;
      uint32_t pk[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + 2 * e;
        const uint32_t lo = c < C ? f2bf(tile[c * RS + rs]) : 0u, hi = c + 1 < C ? f2bf(tile[(c + 1) * RS + rs]) : 0u;
        pk[e] = lo | (hi << 16);
      }
      *reinterpret_cast<uint4*>(dst + (long)i * 8) = uint4{pk[0], pk[1], pk[2], pk[3]};
    }
  } else {
    const int kb = (K + 63) / 64;
    const int c = bx / kb, k0 = (bx - c * kb) * 64;
    if (c >= Cp) return;
    const int nk = min(64, K - k0);
    const float inv_RS = 1.f / RS;
    for (int i = threadIdx.x; i < nk * RS; i += 256) {  // [kk][rs]
      const int kk = fdiv(i, inv_RS), rs = i - kk * RS;
      tile[i] = c < C ? w[((long)(k0 + kk) * C + c) * RS + rs] : 0.f;
    }
    __syncthreads();
    bf16_t* dst = out + (long)c * RS * K + k0;
    if (nk == 64 && (K & 7) == 0) {  // 8 consecutive output channels per thread, one 16-byte store
      for (int i = threadIdx.x; i < RS * 8; i += 256) {  // i = rs*8 + kk0/8
        const int rs = i >> 3, kk0 = (i & 7) * 8;
        uint32_t pk[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          pk[e] = (uint32_t)f2bf(tile[(kk0 + 2 * e) * RS + rs]) | ((uint32_t)f2bf(tile[(kk0 + 2 * e + 1) * RS + rs]) << 16);
        *reinterpret_cast<uint4*>(dst + (long)rs * K + kk0) = uint4{pk[0], pk[1], pk[2], pk[3]};
      }
    } else {
      for (int i = threadIdx.x; i < RS * nk; i += 256) {  // i = rs*nk + kk
        const int rs = i / nk, kk = i - rs * nk;
        dst[(long)rs * K + kk] = f2bf(tile[kk * RS + rs]);
      }
    }
  }
}
MER_API int mer_pack_conv_weights(int n, const long long* desc, long total, void* stream) {
  (void)total;
  if (n <= 0 || n > 64) return (int)hipErrorInvalidValue;
  // grid.x covers the largest record: 512 output channels (layout 0) or 512 x 8 (c, k-block) tiles
  hipLaunchKernelGGL(pack_w_batched_kernel<false>, dim3(512 * 8, n), dim3(256), 0, (hipStream_t)stream, desc, n);
  MER_LAUNCH_CHECK();
}
MER_API int mer_pack_conv_weights_flat(int n, const long long* desc, long total_blocks, void* stream) {
  if (n <= 0 || n > 64 || total_blocks <= 0 || total_blocks > (1L << 30)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_w_batched_kernel<true>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, desc,
                     n);
  MER_LAUNCH_CHECK();
}
