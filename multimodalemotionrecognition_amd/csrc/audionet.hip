// AudioCNN forward in eval mode (audio.py:122-154), fp32 throughout: the network is 94 MFLOP per clip and the
// reference's checkpoints are fp32, so bf16 would buy nothing.
//
// * conv_bn_relu(_pool): 3x3 / pad 1 convolution with bias, BatchNorm on running statistics (folded with the bias
//   into one scale / shift per channel at the start of every launch, from the live parameters), ReLU, and for the
//   first two layers MaxPool2d(2) (floor) in the epilogue -- the pre-pool activation is never stored.
//   Layer 1 (1 -> 16, K = 9) is a direct VALU kernel; layers 2 and 3 (K = 144 / 288, N = 32 / 64) are implicit
//   GEMMs on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) over an input tile with halo staged in LDS.
// * adaptive_avgpool_seq: AdaptiveAvgPool2d((1, bins)) + squeeze + transpose, [B, C, H, W] -> [B, bins, C]; also from
//   the frame trunk's NHWC bf16 activations (AudioResNet18, whose convolutions are the trunk's bf16 kernels).
// AudioCNN's activations are NCHW fp32, as the reference's.
#include "common.h"
#include "mer.h"

// scale = gamma / sqrt(var + eps), shift = (bias - mean) * scale + beta
__device__ __forceinline__ void bn_fold(int c, const float* bias, const float* gamma, const float* beta,
                                        const float* rmean, const float* rvar, float eps, float* sc, float* sh) {
  const float s = gamma[c] * (1.0f / sqrtf(rvar[c] + eps));
  sc[c] = s;
  sh[c] = ((bias ? bias[c] : 0.f) - rmean[c]) * s + beta[c];
}

// ---------------------------------------------------------------------------------------
// Layer 1: Conv2d(1, COUT, 3, pad 1) + BN + ReLU + MaxPool2d(2).  One thread per pooled pixel, all COUT channels:
// a 4x4 input patch in registers, weights / scale / shift in LDS (broadcast reads).  x [B][1][H][W],
// y [B][COUT][H/2][W/2]; lanes run along the pooled row, so every channel's store is contiguous.
// ---------------------------------------------------------------------------------------
template <int COUT>
__global__ __launch_bounds__(256) void conv1_bn_relu_pool_kernel(int H, int W, int blocks_per_img,
                                                                 const float* __restrict__ x,
                                                                 const float* __restrict__ w,
                                                                 const float* __restrict__ bias,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta,
                                                                 const float* __restrict__ rmean,
                                                                 const float* __restrict__ rvar, float eps,
                                                                 float* __restrict__ y) {
  __shared__ float ws[COUT * 9], sc[COUT], sh[COUT];
  const int tid = threadIdx.x;
  for (int e = tid; e < COUT * 9; e += 256) ws[e] = w[e];
  if (tid < COUT) bn_fold(tid, bias, gamma, beta, rmean, rvar, eps, sc, sh);
  __syncthreads();
  const int b = blockIdx.x / blocks_per_img, PH = H / 2, PW = W / 2;
  const int e = (blockIdx.x - b * blocks_per_img) * 256 + tid;
  if (e >= PH * PW) return;
  const int ph = e / PW, pw = e - ph * PW;
  const float* xb = x + (long)b * H * W;
  float p[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int gh = 2 * ph - 1 + r, gw = 2 * pw - 1 + c;
      p[r][c] = (gh >= 0 && gh < H && gw >= 0 && gw < W) ? xb[(long)gh * W + gw] : 0.f;
    }
  float* yb = y + (long)b * COUT * PH * PW + (long)ph * PW + pw;
#pragma unroll 4
  for (int co = 0; co < COUT; ++co) {
    float m = 0.f;  // ReLU outputs are >= 0
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        float a = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) a = fmaf(p[dy + kh][dx + kw], ws[co * 9 + kh * 3 + kw], a);
        m = fmaxf(m, a * sc[co] + sh[co]);
      }
    yb[(long)co * PH * PW] = m;
  }
}

// w [COUT][CIN][3][3] -> wp [tap][CIN][COUT]: the MFMA B operand (k = channel, n = output channel) then reads 16
// consecutive floats per k.  Runs in front of every conv launch (the live weights, nothing cached).
__global__ __launch_bounds__(256) void conv_pack_w_kernel(int CIN, int COUT, const float* __restrict__ w,
                                                          float* __restrict__ wp) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 9 * CIN * COUT) return;
  const int co = e % COUT, ci = (e / COUT) % CIN, tap = e / (COUT * CIN);
  wp[e] = w[((long)co * CIN + ci) * 9 + tap];
}

// ---------------------------------------------------------------------------------------
// Layers 2 / 3: implicit GEMM, M = pixels, N = COUT, K = 9 * CIN ordered (tap, channel).
// A workgroup takes an 8-row x 16-column tile of (pre-pool) output pixels of one image, all COUT channels; the input
// tile with halo ([CIN][10][18], channel stride 208 = 16 mod 32 so the four k lanes of an operand read use both
// halves of the banks) is staged in LDS.  Wave w owns rows 2w, 2w + 1: two row tiles of 16 pixels x COUT / 16 column
// tiles, so a 2x2 pooling window lies in one lane's accumulators (columns 2p, 2p + 1 of both rows).
// x [B][CIN][H][W]; y [B][COUT][H][W], or [B][COUT][H/2][W/2] with POOL.
// ---------------------------------------------------------------------------------------
constexpr int AC_TH = 8, AC_TW = 16, AC_RS = AC_TW + 2, AC_CS = 208;
static_assert((AC_TH + 2) * AC_RS <= AC_CS, "input tile rows fit the channel stride");

template <int CIN, int COUT, bool POOL>
__global__ __launch_bounds__(256) void conv3x3_bn_relu_mfma_kernel(int H, int W, int tiles_h, int tiles_w,
                                                                   const float* __restrict__ x,
                                                                   const float* __restrict__ wp,
                                                                   const float* __restrict__ bias,
                                                                   const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta,
                                                                   const float* __restrict__ rmean,
                                                                   const float* __restrict__ rvar, float eps,
                                                                   float* __restrict__ y) {
  static_assert(CIN % 4 == 0 && COUT % 16 == 0, "MFMA tiling");
  constexpr int NT = COUT / 16;
  __shared__ float Xs[CIN * AC_CS];
  __shared__ float sc[COUT], sh[COUT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lk = lane >> 4;
  int bid = blockIdx.x;
  const int tw = bid % tiles_w;
  bid /= tiles_w;
  const int th = bid % tiles_h, b = bid / tiles_h;
  const int h0 = th * AC_TH, w0 = tw * AC_TW;
  const float* xb = x + (long)b * CIN * H * W;
  if (tid < COUT) bn_fold(tid, bias, gamma, beta, rmean, rvar, eps, sc, sh);
  for (int e = tid; e < CIN * (AC_TH + 2) * AC_RS; e += 256) {
    const int ci = e / ((AC_TH + 2) * AC_RS), rem = e - ci * (AC_TH + 2) * AC_RS;
    const int r = rem / AC_RS, c = rem - r * AC_RS;
    const int gh = h0 - 1 + r, gw = w0 - 1 + c;
    Xs[ci * AC_CS + rem] = (gh >= 0 && gh < H && gw >= 0 && gw < W) ? xb[((long)ci * H + gh) * W + gw] : 0.f;
  }
  __syncthreads();

  f32x4 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int kh = tap / 3, kw = tap - kh * 3;
    const float* xa = Xs + (2 * wv + kh) * AC_RS + lr + kw;
    const float* wb = wp + (long)tap * CIN * COUT + lr;
#pragma unroll 4
    for (int c0 = 0; c0 < CIN; c0 += 4) {
      const int ci = c0 + lk;
      const float a0 = xa[ci * AC_CS], a1 = xa[ci * AC_CS + AC_RS];
      float bv[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) bv[j] = wb[ci * COUT + j * 16];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv[j], acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv[j], acc[1][j], 0, 0, 0);
      }
    }
  }

  // accumulator: row (pixel column) = lk * 4 + r, column (output channel) = j * 16 + lr; image row = h0 + 2 wv + i
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int co = j * 16 + lr;
    const float s = sc[co], t = sh[co];
    float v[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[i][r] = fmaxf(acc[i][j][r] * s + t, 0.f);
    if (POOL) {
      const int PH = H / 2, PW = W / 2, ph = (h0 >> 1) + wv;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int pw = (w0 >> 1) + lk * 2 + p;
        if (ph < PH && pw < PW)
          y[(((long)b * COUT + co) * PH + ph) * PW + pw] =
              fmaxf(fmaxf(v[0][2 * p], v[0][2 * p + 1]), fmaxf(v[1][2 * p], v[1][2 * p + 1]));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = h0 + 2 * wv + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int col = w0 + lk * 4 + r;
          if (row < H && col < W) y[(((long)b * COUT + co) * H + row) * W + col] = v[i][r];
        }
      }
    }
  }
}

template <int CIN, int COUT, bool POOL>
static int launch_conv_mfma(int B, int H, int W, const float* x, const float* w, const float* bias, const float* gamma,
                            const float* beta, const float* rmean, const float* rvar, float eps, float* wpack, float* y,
                            hipStream_t st) {
  const int tiles_h = (H + AC_TH - 1) / AC_TH, tiles_w = (W + AC_TW - 1) / AC_TW;
  if ((long)B * tiles_h * tiles_w > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(conv_pack_w_kernel, dim3((9 * CIN * COUT + 255) / 256), dim3(256), 0, st, CIN, COUT, w, wpack);
  hipLaunchKernelGGL((conv3x3_bn_relu_mfma_kernel<CIN, COUT, POOL>), dim3(B * tiles_h * tiles_w), dim3(256), 0, st, H, W,
                     tiles_h, tiles_w, x, wpack, bias, gamma, beta, rmean, rvar, eps, y);
  MER_LAUNCH_CHECK();
}

MER_API int mer_audiocnn_conv(int B, int H, int W, int Cin, int Cout, int pool, const float* x, const float* w,
                              const float* bias, const float* gamma, const float* beta, const float* rmean,
                              const float* rvar, float eps, float* wpack, float* y, void* stream) {
  if (B <= 0) return 0;
  if (H < 1 || W < 1 || !x || !w || !gamma || !beta || !rmean || !rvar || !y) return (int)hipErrorInvalidValue;
  if (pool && (H < 2 || W < 2)) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (Cin == 1 && Cout == 16 && pool) {
    const int bpi = ((H / 2) * (W / 2) + 255) / 256;
    if ((long)B * bpi > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(conv1_bn_relu_pool_kernel<16>, dim3(B * bpi), dim3(256), 0, st, H, W, bpi, x, w, bias, gamma, beta,
                       rmean, rvar, eps, y);
    MER_LAUNCH_CHECK();
  }
  if (!wpack) return (int)hipErrorInvalidValue;
  if (Cin == 16 && Cout == 32 && pool)
    return launch_conv_mfma<16, 32, true>(B, H, W, x, w, bias, gamma, beta, rmean, rvar, eps, wpack, y, st);
  if (Cin == 32 && Cout == 64 && !pool)
    return launch_conv_mfma<32, 64, false>(B, H, W, x, w, bias, gamma, beta, rmean, rvar, eps, wpack, y, st);
  return (int)hipErrorInvalidValue;  // only the three layers of AudioCNN are built
}

// ---------------------------------------------------------------------------------------
// AdaptiveAvgPool2d((1, bins)) + squeeze(2) + transpose(1, 2): y[b][i][c] = mean over all h and over
// w in [floor(i W / bins), ceil((i + 1) W / bins)) of x[b][c][h][w] (bins overlap when W < bins).
// One thread per output, bin index fastest (neighbouring lanes read neighbouring column ranges of one row).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adaptive_avgpool_seq_kernel(long total, int C, int H, int W, int bins,
                                                                   const float* __restrict__ x,
                                                                   float* __restrict__ y) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int i = (int)(e % bins);
  const long bc = e / bins;
  const int c = (int)(bc % C);
  const long b = bc / C;
  const int ws = (int)(((long)i * W) / bins), we = (int)((((long)i + 1) * W + bins - 1) / bins);
  const float* p = x + bc * H * W;
  float s = 0.f;
  for (int h = 0; h < H; ++h)
    for (int q = ws; q < we; ++q) s += p[(long)h * W + q];
  y[(b * bins + i) * C + c] = s / (float)(H * (we - ws));
}

MER_API int mer_adaptive_avgpool_seq(int B, int C, int H, int W, int bins, const float* x, float* y, void* stream) {
  if (B <= 0) return 0;
  if (C < 1 || H < 1 || W < 1 || bins < 1 || !x || !y) return (int)hipErrorInvalidValue;
  const long total = (long)B * C * bins;
  if ((total + 255) / 256 > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(adaptive_avgpool_seq_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, total, C, H, W, bins, x, y);
  MER_LAUNCH_CHECK();
}

// The same pooling of an NHWC bf16 map (AudioResNet18's layer4 output): x bf16 [B][H][W][C] -> y fp32 [B][bins][C];
// one thread per output, channel fastest (every load and the store are contiguous across lanes).
__global__ __launch_bounds__(256) void adaptive_avgpool_seq_nhwc_kernel(long total, int C, int H, int W, int bins,
                                                                        const bf16_t* __restrict__ x,
                                                                        float* __restrict__ y) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const long bi = e / C;
  const int i = (int)(bi % bins);
  const long b = bi / bins;
  const int ws = (int)(((long)i * W) / bins), we = (int)((((long)i + 1) * W + bins - 1) / bins);
  const bf16_t* p = x + b * H * W * C + c;
  float s = 0.f;
  for (int h = 0; h < H; ++h)
    for (int q = ws; q < we; ++q) s += bf2f(p[((long)h * W + q) * C]);
  y[e] = s / (float)(H * (we - ws));
}

MER_API int mer_adaptive_avgpool_seq_nhwc(int B, int H, int W, int C, int bins, const void* x, float* y, void* stream) {
  if (B <= 0) return 0;
  if (C < 1 || H < 1 || W < 1 || bins < 1 || !x || !y) return (int)hipErrorInvalidValue;
  const long total = (long)B * C * bins;
  if ((total + 255) / 256 > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(adaptive_avgpool_seq_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, total, C, H, W, bins, (const bf16_t*)x, y);
  MER_LAUNCH_CHECK();
}
