// AudioCNN in training mode (audio.py:122-154), fp32 NCHW throughout: forward on batch statistics with the running-stat
// update, and the whole backward.  The eval kernels of audionet.hip are not touched (tests/test_audionet_gpu.py pins
// their bits); the MFMA tiling here is theirs.
//
// Forward, per layer:  conv + bias -> z (stored: the backward needs it)
//                      per-(image, channel) plane (mean, M2), merged per channel by Chan's formula in a fixed order
//                      -> scale / shift / mean / invstd, running statistics, num_batches_tracked
//                      y = [maxpool2] relu(z * scale + shift)
// Backward, per layer: sum g and sum g * xhat per plane through the recomputed arg-max / ReLU mask, folded per channel
//                      -> dbeta, dgamma; dz = scale * (g - mean g - xhat * mean(g xhat)) over the whole map
//                      (layer 1 never stores dz: its nine weight-gradient taps and the bias sum are reduced in the
//                      same pass); conv weight gradient on the MFMA into per-workgroup rows folded in a fixed order;
//                      conv data gradient = the forward conv kernel on the flipped, transposed weights.
// No atomics: every reduction has a fixed order that depends on the shape alone.
#include "common.h"
#include "mer.h"

constexpr int AT_TH = 8, AT_TW = 16, AT_RS = AT_TW + 2, AT_CS = 208;
static_assert((AT_TH + 2) * AT_RS <= AT_CS, "input tile rows fit the channel stride");

__device__ __forceinline__ float bn_act(float z, float sc, float sh) { return fmaf(z, sc, sh); }

// Sum over the 256 threads of a block in a fixed order; red: 4 floats of LDS.  Every thread gets the result.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// First maximum of a 2x2 window in window order (00, 01, 10, 11), as torch's max_pool2d: strict comparisons.
__device__ __forceinline__ int window_argmax(const float a[4]) {
  int k = 0;
  float m = a[0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (a[i] > m) {
      m = a[i];
      k = i;
    }
  return k;
}

// ---------------------------------------------------------------------------------------
// Layer 1 forward: Conv2d(1, COUT, 3, pad 1) + bias, one thread per pixel, all COUT channels.
// ---------------------------------------------------------------------------------------
template <int COUT>
__global__ __launch_bounds__(256) void conv1_z_kernel(int H, int W, int blocks_per_img, const float* __restrict__ x,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ z) {
  __shared__ float ws[COUT * 9], bs[COUT];
  const int tid = threadIdx.x;
  for (int e = tid; e < COUT * 9; e += 256) ws[e] = w[e];
  if (tid < COUT) bs[tid] = bias ? bias[tid] : 0.f;
  __syncthreads();
  const int b = blockIdx.x / blocks_per_img;
  const int e = (blockIdx.x - b * blocks_per_img) * 256 + tid;
  if (e >= H * W) return;
  const int h = e / W, q = e - h * W;
  const float* xb = x + (long)b * H * W;
  float p[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int gh = h - 1 + r, gw = q - 1 + c;
      p[r][c] = (gh >= 0 && gh < H && gw >= 0 && gw < W) ? xb[(long)gh * W + gw] : 0.f;
    }
  float* zb = z + (long)b * COUT * H * W + e;
#pragma unroll 4
  for (int co = 0; co < COUT; ++co) {
    float a = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) a = fmaf(p[kh][kw], ws[co * 9 + kh * 3 + kw], a);
    zb[(long)co * H * W] = a + bs[co];
  }
}

// Forward: w [COUT][CIN][3][3] -> wp [tap][CIN][COUT].  Data gradient (transposed): w is the forward weight
// [CIN][COUT][3][3] (this conv's input channels are the forward's outputs) and wp[tap][ci][co] = w[ci][co][8 - tap].
__global__ __launch_bounds__(256) void conv_pack_wt_kernel(int CIN, int COUT, int transposed, const float* __restrict__ w,
                                                           float* __restrict__ wp) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 9 * CIN * COUT) return;
  const int co = e % COUT, ci = (e / COUT) % CIN, tap = e / (COUT * CIN);
  wp[e] = transposed ? w[((long)ci * COUT + co) * 9 + (8 - tap)] : w[((long)co * CIN + ci) * 9 + tap];
}

// ---------------------------------------------------------------------------------------
// 3x3 / pad 1 convolution as an implicit GEMM on the exact-fp32 MFMA, the tiling of audionet.hip: a workgroup takes
// an 8 x 16 pixel tile of one image and all COUT channels; wave w owns rows 2w, 2w + 1.  z = conv(x) (+ bias).
// ---------------------------------------------------------------------------------------
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void conv3x3_z_mfma_kernel(int H, int W, int tiles_h, int tiles_w,
                                                             const float* __restrict__ x, const float* __restrict__ wp,
                                                             const float* __restrict__ bias, float* __restrict__ z) {
  static_assert(CIN % 4 == 0 && COUT % 16 == 0, "MFMA tiling");
  constexpr int NT = COUT / 16;
  __shared__ float Xs[CIN * AT_CS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lk = lane >> 4;
  int bid = blockIdx.x;
  const int tw = bid % tiles_w;
  bid /= tiles_w;
  const int th = bid % tiles_h, b = bid / tiles_h;
  const int h0 = th * AT_TH, w0 = tw * AT_TW;
  const float* xb = x + (long)b * CIN * H * W;
  for (int e = tid; e < CIN * (AT_TH + 2) * AT_RS; e += 256) {
    const int ci = e / ((AT_TH + 2) * AT_RS), rem = e - ci * (AT_TH + 2) * AT_RS;
    const int r = rem / AT_RS, c = rem - r * AT_RS;
    const int gh = h0 - 1 + r, gw = w0 - 1 + c;
    Xs[ci * AT_CS + rem] = (gh >= 0 && gh < H && gw >= 0 && gw < W) ? xb[((long)ci * H + gh) * W + gw] : 0.f;
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
    const float* xa = Xs + (2 * wv + kh) * AT_RS + lr + kw;
    const float* wb = wp + (long)tap * CIN * COUT + lr;
#pragma unroll 4
    for (int c0 = 0; c0 < CIN; c0 += 4) {
      const int ci = c0 + lk;
      const float a0 = xa[ci * AT_CS], a1 = xa[ci * AT_CS + AT_RS];
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
    const float bs = bias ? bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = h0 + 2 * wv + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = w0 + lk * 4 + r;
        if (row < H && col < W) z[(((long)b * COUT + co) * H + row) * W + col] = acc[i][j][r] + bs;
      }
    }
  }
}

template <int CIN, int COUT>
static int launch_conv_z(int B, int H, int W, int transposed, const float* x, const float* w, const float* bias,
                         float* wpack, float* z, hipStream_t st) {
  const int tiles_h = (H + AT_TH - 1) / AT_TH, tiles_w = (W + AT_TW - 1) / AT_TW;
  if ((long)B * tiles_h * tiles_w > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(conv_pack_wt_kernel, dim3((9 * CIN * COUT + 255) / 256), dim3(256), 0, st, CIN, COUT, transposed, w,
                     wpack);
  hipLaunchKernelGGL((conv3x3_z_mfma_kernel<CIN, COUT>), dim3(B * tiles_h * tiles_w), dim3(256), 0, st, H, W, tiles_h,
                     tiles_w, x, wpack, bias, z);
  MER_LAUNCH_CHECK();
}

MER_API int mer_audiocnn_train_conv(int B, int H, int W, int Cin, int Cout, int transposed, const float* x,
                                    const float* w, const float* bias, float* wpack, float* z, void* stream) {
  if (B < 1 || H < 1 || W < 1 || !x || !w || !z) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (!transposed && Cin == 1 && Cout == 16) {
    const long bpi = ((long)H * W + 255) / 256;
    if ((long)H * W > 0x7fffffffL || (long)B * bpi > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(conv1_z_kernel<16>, dim3((unsigned)(B * bpi)), dim3(256), 0, st, H, W, (int)bpi, x, w, bias, z);
    MER_LAUNCH_CHECK();
  }
  if (!wpack) return (int)hipErrorInvalidValue;
  if (!transposed && Cin == 16 && Cout == 32) return launch_conv_z<16, 32>(B, H, W, 0, x, w, bias, wpack, z, st);
  if (!transposed && Cin == 32 && Cout == 64) return launch_conv_z<32, 64>(B, H, W, 0, x, w, bias, wpack, z, st);
  if (transposed && Cin == 64 && Cout == 32) return launch_conv_z<64, 32>(B, H, W, 1, x, w, bias, wpack, z, st);
  if (transposed && Cin == 32 && Cout == 16) return launch_conv_z<32, 16>(B, H, W, 1, x, w, bias, wpack, z, st);
  return (int)hipErrorInvalidValue;  // only AudioCNN's three layers and their two data gradients are built
}

// ---------------------------------------------------------------------------------------
// Batch statistics.  A plane (image, channel) is cut into S = ceil(HW / MER_BN_PLANE_CHUNK) chunks of CH values, one
// block each (a block per plane left the 39 MB layer-1 map to 512 blocks: 62 us).  Per chunk: the mean from a plain
// sum, corrected by the sum of the deviations from it, and M2 = sum (v - mean)^2 about that mean -- no sum of
// squares, so a map whose mean is far from zero (log-mel: -40 +- 15) keeps its variance.
// part [C][B * S][2] = (mean, M2); chunk s of a plane holds the values [s CH, min(HW, (s + 1) CH)).
// ---------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int chunk_count(int n, int ch, int s) {
  const long lo = (long)s * ch, hi = lo + ch < n ? lo + ch : n;
  return hi > lo ? (int)(hi - lo) : 0;
}

__global__ __launch_bounds__(256) void bn_plane_stats_kernel(int B, int C, int HW, int S, int CH,
                                                             const float* __restrict__ z, float* __restrict__ part) {
  __shared__ float red[4];
  const int plane = blockIdx.x / S, sc = blockIdx.x - plane * S;
  const int b = plane / C, c = plane - b * C, tid = threadIdx.x;
  const int n = chunk_count(HW, CH, sc);
  const float* p = z + (long)plane * HW + (long)sc * CH;
  float s = 0.f;
  for (int i = tid; i < n; i += 256) s += p[i];
  const float m0 = n ? block_sum(s, red) / (float)n : 0.f;
  float d1 = 0.f, d2 = 0.f;
  for (int i = tid; i < n; i += 256) {
    const float d = p[i] - m0;
    d1 += d;
    d2 = fmaf(d, d, d2);
  }
  d1 = block_sum(d1, red);
  d2 = block_sum(d2, red);
  if (tid == 0) {
    const float corr = n ? d1 / (float)n : 0.f;
    const long r = (((long)c * B + b) * S + sc) * 2;
    part[r] = m0 + corr;
    part[r + 1] = fmaxf(d2 - corr * d1, 0.f);
  }
}

// One wave per channel, in fp64: lane l merges the chunk records l, l + 64, ... in order (Chan et al.), then the 64
// lane results are merged down a fixed tree (one thread walking all B * S records cost 60 us of dependent loads).
// ss [C][4] = scale, shift, mean, invstd with scale = gamma * invstd, shift = beta - mean * scale.
__global__ __launch_bounds__(64) void bn_train_finalize_kernel(int B, int C, int HW, int S, int CH,
                                                               const float* __restrict__ part,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, float momentum,
                                                               float* __restrict__ ss, float* __restrict__ rmean,
                                                               float* __restrict__ rvar, long* __restrict__ nbt) {
  const int c = blockIdx.x, lane = threadIdx.x;
  if (c == 0 && lane == 0 && nbt) nbt[0] += 1;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int r = lane; r < B * S; r += 64) {
    const double nb = (double)chunk_count(HW, CH, r % S);
    if (nb == 0.0) continue;
    const double mb = part[((long)c * B * S + r) * 2], qb = part[((long)c * B * S + r) * 2 + 1];
    const double nt = n + nb, delta = mb - mean;
    mean += delta * (nb / nt);
    m2 += qb + delta * delta * (n * nb / nt);
    n = nt;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double nb = __shfl_down(n, o, 64), mb = __shfl_down(mean, o, 64), qb = __shfl_down(m2, o, 64);
    const double nt = n + nb, delta = mb - mean;
    if (nb > 0.0) {
      mean += delta * (nb / nt);
      m2 += qb + delta * delta * (n * nb / nt);
      n = nt;
    }
  }
  if (lane) return;
  const double var = m2 / n;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = gamma[c] * invstd, fm = (float)mean;
  ss[c * 4] = sc;
  ss[c * 4 + 1] = fmaf(-fm, sc, beta[c]);
  ss[c * 4 + 2] = fm;
  ss[c * 4 + 3] = invstd;
  if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * fm;
  if (rvar) rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)(m2 / (n - 1.0));
}

MER_API int mer_bn_train_stats(int B, int C, int HW, const float* z, const float* gamma, const float* beta, float eps,
                               float momentum, float* part, float* ss, float* running_mean, float* running_var,
                               long* num_batches_tracked, void* stream) {
  if (B < 1 || C < 1 || HW < 1 || (long)B * HW < 2 || !z || !gamma || !beta || !part || !ss)
    return (int)hipErrorInvalidValue;
  const int S = MER_BN_PLANE_CHUNKS(HW), CH = (HW + S - 1) / S;
  if ((long)B * C * S > 0x7fffffffL || !(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_plane_stats_kernel, dim3(B * C * S), dim3(256), 0, st, B, C, HW, S, CH, z, part);
  hipLaunchKernelGGL(bn_train_finalize_kernel, dim3(C), dim3(64), 0, st, B, C, HW, S, CH, part, gamma, beta,
                     eps, momentum, ss, running_mean, running_var, num_batches_tracked);
  MER_LAUNCH_CHECK();
}

// y = relu(z * scale + shift), or its 2x2 floor max-pool; one thread per output.
__global__ __launch_bounds__(256) void bn_relu_pool_fwd_kernel(long total, int C, int H, int W, int pool,
                                                               const float* __restrict__ z, const float* __restrict__ ss,
                                                               float* __restrict__ y) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  if (!pool) {
    const int c = (int)((e / ((long)H * W)) % C);
    y[e] = fmaxf(bn_act(z[e], ss[c * 4], ss[c * 4 + 1]), 0.f);
    return;
  }
  const int PH = H / 2, PW = W / 2;
  const int pw = (int)(e % PW);
  const long t = e / PW;
  const int ph = (int)(t % PH);
  const long bc = t / PH;
  const int c = (int)(bc % C);
  const float sc = ss[c * 4], sh = ss[c * 4 + 1];
  const float* p = z + (bc * H + 2 * ph) * W + 2 * pw;
  const float m = fmaxf(fmaxf(bn_act(p[0], sc, sh), bn_act(p[1], sc, sh)),
                        fmaxf(bn_act(p[W], sc, sh), bn_act(p[W + 1], sc, sh)));
  y[e] = fmaxf(m, 0.f);
}

MER_API int mer_bn_relu_pool_fwd(int B, int C, int H, int W, int pool, const float* z, const float* ss, float* y,
                                 void* stream) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || !z || !ss || !y) return (int)hipErrorInvalidValue;
  if (pool && (H < 2 || W < 2)) return (int)hipErrorInvalidValue;
  const long total = (long)B * C * (pool ? H / 2 : H) * (pool ? W / 2 : W);
  if ((total + 255) / 256 > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_relu_pool_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     total, C, H, W, pool, z, ss, y);
  MER_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------
// Backward of [maxpool2] relu(bn(z)).  g is the gradient of the layer's output ([B][C][H/2][W/2] with pool).
// Pass 1, one block per chunk of a plane (S chunks, as the statistics): sum g and sum g * xhat, g routed to the first
// maximum of its window and through the ReLU mask bn(z) > 0 (both recomputed from z).  red [C][B * S][2].
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_bwd_plane_reduce_kernel(int B, int C, int H, int W, int pool, int S,
                                                                  const float* __restrict__ z,
                                                                  const float* __restrict__ ss,
                                                                  const float* __restrict__ g, float* __restrict__ red,
                                                                  const float* __restrict__ x, float* __restrict__ xs) {
  __shared__ float rs[4];
  const int plane = blockIdx.x / S, cs = blockIdx.x - plane * S;
  const int b = plane / C, c = plane - b * C, tid = threadIdx.x;
  const float sc = ss[c * 4], sh = ss[c * 4 + 1], mean = ss[c * 4 + 2], invstd = ss[c * 4 + 3];
  const float* zp = z + (long)plane * H * W;
  float s1 = 0.f, s2 = 0.f;
  if (pool) {
    const int PH = H / 2, PW = W / 2, ch = (PH * PW + S - 1) / S;
    const int i0 = cs * ch, i1 = i0 + chunk_count(PH * PW, ch, cs);
    const float* gp = g + (long)plane * PH * PW;
    for (int i = i0 + tid; i < i1; i += 256) {
      const int ph = i / PW, pw = i - ph * PW;
      const float* p = zp + (long)(2 * ph) * W + 2 * pw;
      const float zz[4] = {p[0], p[1], p[W], p[W + 1]};
      const float a[4] = {bn_act(zz[0], sc, sh), bn_act(zz[1], sc, sh), bn_act(zz[2], sc, sh), bn_act(zz[3], sc, sh)};
      const int k = window_argmax(a);
      float am = a[0], zm = zz[0];
#pragma unroll
      for (int q = 1; q < 4; ++q)
        if (k == q) {
          am = a[q];
          zm = zz[q];
        }
      if (am > 0.f) {
        const float gv = gp[i];
        s1 += gv;
        s2 = fmaf(gv, (zm - mean) * invstd, s2);
      }
    }
  } else {
    const int ch = (H * W + S - 1) / S, i0 = cs * ch, i1 = i0 + chunk_count(H * W, ch, cs);
    const float* gp = g + (long)plane * H * W;
    for (int i = i0 + tid; i < i1; i += 256) {
      const float zv = zp[i];
      if (bn_act(zv, sc, sh) > 0.f) {
        const float gv = gp[i];
        s1 += gv;
        s2 = fmaf(gv, (zv - mean) * invstd, s2);
      }
    }
  }
  s1 = block_sum(s1, rs);
  s2 = block_sum(s2, rs);
  if (tid == 0) {
    red[(((long)c * B + b) * S + cs) * 2] = s1;
    red[(((long)c * B + b) * S + cs) * 2 + 1] = s2;
  }
  if (x && c == 0) {  // layer 1: the sums of the conv's input, for the centring constant of its weight gradient
    const int ch = (H * W + S - 1) / S, i0 = cs * ch, i1 = i0 + chunk_count(H * W, ch, cs);
    float sx = 0.f;
    for (int i = i0 + tid; i < i1; i += 256) sx += x[(long)b * H * W + i];
    sx = block_sum(sx, rs);
    if (tid == 0) xs[b * S + cs] = sx;
  }
}

// One wave per channel: lane l adds the chunk sums l, l + 64, ... of the R = B * S in order, then the lanes are added
// by the fixed butterfly of wave_sum; dbeta += sum g, dgamma += sum g xhat (either may be NULL),
// coef [C][2] = the two means over the n = B H W values of the channel; coef[2 C] = the mean of the layer-1 input.
__global__ __launch_bounds__(64) void bn_bwd_finalize_kernel(int R, int C, float inv_n, const float* __restrict__ red,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                             float* __restrict__ coef, const float* __restrict__ xs) {
  const int c = blockIdx.x, lane = threadIdx.x;
  if (c == 0 && xs) {
    float sx = 0.f;
    for (int r = lane; r < R; r += 64) sx += xs[r];
    sx = wave_sum(sx);
    if (lane == 0) coef[2 * C] = sx * inv_n;
  }
  float s1 = 0.f, s2 = 0.f;
  for (int r = lane; r < R; r += 64) {
    s1 += red[((long)c * R + r) * 2];
    s2 += red[((long)c * R + r) * 2 + 1];
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane) return;
  if (dbeta) dbeta[c] += s1;
  if (dgamma) dgamma[c] += s2;
  coef[c * 2] = s1 * inv_n;
  coef[c * 2 + 1] = s2 * inv_n;
}

// Pass 2, one block per chunk of a plane, every pixel of the map (also the rows / columns the floor pooling drops: they get no
// g but belong to the statistics): dz = scale * (g - mean g - xhat * mean(g xhat)).  The chunk's sum of dz goes to
// dbp [B * S][C].  WG1 (layer 1, one input channel): dz is not stored; its products with the nine shifted inputs are
// reduced here instead, dwp [B * S][C][9].  The input is centred first, x - xc with xc = its batch mean (the zero padding
// becomes -xc): sum dz is zero under batch statistics, so the constant drops out of the gradient, and without it a
// log-mel input (mean -40) multiplies every rounding of the cancelling dz sum by 40 -- fp32 torch is 1.5e-4 of max-abs
// off fp64 on the T = 301 golden for that reason.
template <bool WG1>
__global__ __launch_bounds__(256) void bn_bwd_dz_kernel(int B, int C, int H, int W, int pool, int S,
                                                        const float* __restrict__ z, const float* __restrict__ ss,
                                                        const float* __restrict__ coef, const float* __restrict__ g,
                                                        float* __restrict__ dz, const float* __restrict__ x,
                                                        float* __restrict__ dbp, float* __restrict__ dwp) {
  __shared__ float rs[4];
  const int plane = blockIdx.x / S, cs = blockIdx.x - plane * S;
  const int b = plane / C, c = plane - b * C, tid = threadIdx.x;
  const float sc = ss[c * 4], sh = ss[c * 4 + 1], mean = ss[c * 4 + 2], invstd = ss[c * 4 + 3];
  const float c1 = coef[c * 2], c2 = coef[c * 2 + 1];
  const int PH = H / 2, PW = W / 2;
  const int ch = (H * W + S - 1) / S, i0 = cs * ch, i1 = i0 + chunk_count(H * W, ch, cs);
  const float* zp = z + (long)plane * H * W;
  const float* gp = g + (long)plane * (pool ? PH * PW : H * W);
  const float* xb = WG1 ? x + (long)b * H * W : nullptr;
  const float xc = WG1 ? coef[2 * C] : 0.f;
  float sdz = 0.f, sw[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) sw[t] = 0.f;
  for (int i = i0 + tid; i < i1; i += 256) {
    const int h = i / W, q = i - h * W;
    const float zv = zp[i];
    float gv = 0.f;
    if (pool) {
      const int ph = h >> 1, pw = q >> 1;
      if (ph < PH && pw < PW) {
        const float* p = zp + (long)(2 * ph) * W + 2 * pw;
        const float a[4] = {bn_act(p[0], sc, sh), bn_act(p[1], sc, sh), bn_act(p[W], sc, sh), bn_act(p[W + 1], sc, sh)};
        if (window_argmax(a) == (h & 1) * 2 + (q & 1) && bn_act(zv, sc, sh) > 0.f) gv = gp[ph * PW + pw];
      }
    } else if (bn_act(zv, sc, sh) > 0.f) {
      gv = gp[i];
    }
    const float d = sc * (gv - c1 - (zv - mean) * invstd * c2);
    sdz += d;
    if (WG1) {
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int gh = h - 1 + kh, gw = q - 1 + kw;
          const float xv = (gh >= 0 && gh < H && gw >= 0 && gw < W) ? xb[(long)gh * W + gw] : 0.f;
          sw[kh * 3 + kw] = fmaf(d, xv - xc, sw[kh * 3 + kw]);
        }
    } else {
      dz[(long)plane * H * W + i] = d;
    }
  }
  sdz = block_sum(sdz, rs);
  if (tid == 0) dbp[((long)b * S + cs) * C + c] = sdz;
  if (WG1) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float v = block_sum(sw[t], rs);
      if (tid == 0) dwp[(((long)b * S + cs) * C + c) * 9 + t] = v;
    }
  }
}

// out[k] += sum over the rows p of part[p * n + k], in a fixed order: a block takes 64 columns, wave w adds the rows
// w, w + 4, ... and the four sums are added in wave order.
__global__ __launch_bounds__(256) void rows_sum_kernel(int rows, int n, const float* __restrict__ part,
                                                       float* __restrict__ out) {
  __shared__ float ps[4][64];
  const int col = threadIdx.x & 63, wv = threadIdx.x >> 6, k = blockIdx.x * 64 + col;
  float s = 0.f;
  if (k < n) {
#pragma unroll 8
    for (int p = wv; p < rows; p += 4) s += part[(long)p * n + k];
  }
  ps[wv][col] = s;
  __syncthreads();
  if (wv == 0 && k < n) out[k] += (ps[0][col] + ps[1][col]) + (ps[2][col] + ps[3][col]);
}

MER_API int mer_bn_relu_pool_bwd(int B, int C, int H, int W, int pool, const float* z, const float* ss, const float* g,
                                 float* part, float* dgamma, float* dbeta, float* dbias, float* dz, const float* x,
                                 float* dw1, void* stream) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || !z || !ss || !g || !part) return (int)hipErrorInvalidValue;
  if (pool && (H < 2 || W < 2)) return (int)hipErrorInvalidValue;
  if ((long)H * W > 0x7fffffffL || (long)B * H * W < 2) return (int)hipErrorInvalidValue;
  const int S = MER_BN_PLANE_CHUNKS(H * W);
  if ((long)B * C * S > 0x7fffffffL / 12) return (int)hipErrorInvalidValue;
  const int R = B * S;
  if ((x != nullptr) != (dw1 != nullptr) || (!dz && !x)) return (int)hipErrorInvalidValue;
  if (dz && x) return (int)hipErrorInvalidValue;  // layer 1 reduces its weight gradient and stores no dz
  hipStream_t st = (hipStream_t)stream;
  // part, with R = B * S: red [C][R][2] | coef [2 C + 1] | dbp [R][C] | dwp [R][C][9] | xs [R]
  //       = MER_BN_RELU_POOL_BWD_WS(B, C, HW) floats
  float *red = part, *coef = red + (long)2 * R * C, *dbp = coef + 2 * C + 1, *dwp = dbp + (long)R * C;
  float* xs = x ? dwp + (long)9 * R * C : nullptr;
  hipLaunchKernelGGL(bn_bwd_plane_reduce_kernel, dim3(R * C), dim3(256), 0, st, B, C, H, W, pool, S, z, ss, g, red, x, xs);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(64), 0, st, R, C,
                     (float)(1.0 / ((double)B * H * W)), red, dgamma, dbeta, coef, xs);
  if (x) {
    hipLaunchKernelGGL(bn_bwd_dz_kernel<true>, dim3(R * C), dim3(256), 0, st, B, C, H, W, pool, S, z, ss, coef, g, dz, x,
                       dbp, dwp);
    hipLaunchKernelGGL(rows_sum_kernel, dim3((C * 9 + 63) / 64), dim3(256), 0, st, R, C * 9, dwp, dw1);
  } else {
    hipLaunchKernelGGL(bn_bwd_dz_kernel<false>, dim3(R * C), dim3(256), 0, st, B, C, H, W, pool, S, z, ss, coef, g, dz, x,
                       dbp, dwp);
  }
  if (dbias) hipLaunchKernelGGL(rows_sum_kernel, dim3((C + 63) / 64), dim3(256), 0, st, R, C, dbp, dbias);
  MER_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------
// Conv weight gradient of layers 2 / 3: dw[co][ci][tap] = sum over pixels of dz[co][p] * x[ci][p + tap], a GEMM with
// M = COUT, N = 9 CIN, K = B H W on the exact-fp32 MFMA.  A workgroup walks the 4 x 16 pixel tiles
// blockIdx.x, blockIdx.x + gridDim.x, ... (a mapping of the shape alone) with the input tile (halo included) and the
// dz tile in LDS, pixel-major with the channel fastest (odd strides: conflict-free staging, ~2 lanes per bank on the
// operand reads).  Wave w owns output channels 16 (w % MT) .. + 16 and, when COUT = 32, rows 2 (w / MT), + 1 of the
// tile: all nine taps and every input channel, 9 CIN / 16 accumulator tiles.  Each (workgroup, row half) writes one
// row of part [gridDim.x * PS][COUT * CIN * 9]; rows_sum_kernel folds them in order.
// ---------------------------------------------------------------------------------------
constexpr int WG_TH = 4;

template <int CIN, int COUT>
__global__ __launch_bounds__(256) void conv3x3_wgrad_mfma_kernel(int H, int W, int tiles_h, int tiles_w, int ntiles,
                                                                 const float* __restrict__ x,
                                                                 const float* __restrict__ dz,
                                                                 float* __restrict__ part) {
  static_assert(CIN % 16 == 0 && (COUT == 32 || COUT == 64), "MFMA tiling");
  constexpr int MT = COUT / 16, PS = 4 / MT, NT = CIN / 16, RW = WG_TH / PS;
  constexpr int XS = CIN == 16 ? 17 : CIN + 17, DS = COUT + 17;  // = 17 mod 32
  constexpr int XP = (WG_TH + 2) * AT_RS, DP = WG_TH * AT_TW;
  __shared__ float Xs[XP * XS];
  __shared__ float Ds[DP * DS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const int mt = wv % MT, ps = wv / MT;
  f32x4 acc[NT][9];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int bid = tile;
    const int tw = bid % tiles_w;
    bid /= tiles_w;
    const int th = bid % tiles_h, b = bid / tiles_h;
    const int h0 = th * WG_TH, w0 = tw * AT_TW;
    const float* xb = x + (long)b * CIN * H * W;
    const float* db = dz + (long)b * COUT * H * W;
    __syncthreads();  // the previous tile's operand reads
    for (int e = tid; e < CIN * XP; e += 256) {
      const int ci = e / XP, rem = e - ci * XP;
      const int r = rem / AT_RS, c = rem - r * AT_RS;
      const int gh = h0 - 1 + r, gw = w0 - 1 + c;
      Xs[rem * XS + ci] = (gh >= 0 && gh < H && gw >= 0 && gw < W) ? xb[((long)ci * H + gh) * W + gw] : 0.f;
    }
    for (int e = tid; e < COUT * DP; e += 256) {
      const int co = e / DP, rem = e - co * DP;
      const int r = rem / AT_TW, c = rem - r * AT_TW;
      const int gh = h0 + r, gw = w0 + c;
      Ds[rem * DS + co] = (gh < H && gw < W) ? db[((long)co * H + gh) * W + gw] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
      const int row = ps * RW + rr;
#pragma unroll
      for (int c0 = 0; c0 < AT_TW; c0 += 4) {
        const float a = Ds[(row * AT_TW + c0 + lk) * DS + mt * 16 + lr];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int kh = t / 3, kw = t - kh * 3;
          const float* xp = Xs + ((row + kh) * AT_RS + c0 + lk + kw) * XS + lr;
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xp[j * 16], acc[j][t], 0, 0, 0);
        }
      }
    }
  }
  // accumulator: row (output channel) = mt * 16 + lk * 4 + r, column (input channel) = j * 16 + lr
  float* pr = part + ((long)blockIdx.x * PS + ps) * (COUT * CIN * 9);
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) pr[((mt * 16 + lk * 4 + r) * CIN + j * 16 + lr) * 9 + t] = acc[j][t][r];
}

template <int CIN, int COUT>
static int launch_wgrad(int B, int H, int W, const float* x, const float* dz, float* part, float* dw, hipStream_t st) {
  const int tiles_h = (H + WG_TH - 1) / WG_TH, tiles_w = (W + AT_TW - 1) / AT_TW;
  const long ntiles = (long)B * tiles_h * tiles_w;
  if (ntiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const int wgs = ntiles < MER_AUDIOCNN_WGRAD_WGS ? (int)ntiles : MER_AUDIOCNN_WGRAD_WGS;
  constexpr int PS = 4 / (COUT / 16), n = COUT * CIN * 9;
  hipLaunchKernelGGL((conv3x3_wgrad_mfma_kernel<CIN, COUT>), dim3(wgs), dim3(256), 0, st, H, W, tiles_h, tiles_w,
                     (int)ntiles, x, dz, part);
  hipLaunchKernelGGL(rows_sum_kernel, dim3((n + 63) / 64), dim3(256), 0, st, wgs * PS, n, part, dw);
  MER_LAUNCH_CHECK();
}

MER_API int mer_audiocnn_wgrad(int B, int H, int W, int Cin, int Cout, const float* x, const float* dz, float* part,
                               float* dw, void* stream) {
  if (B < 1 || H < 1 || W < 1 || !x || !dz || !part || !dw) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (Cin == 16 && Cout == 32) return launch_wgrad<16, 32>(B, H, W, x, dz, part, dw, st);
  if (Cin == 32 && Cout == 64) return launch_wgrad<32, 64>(B, H, W, x, dz, part, dw, st);
  return (int)hipErrorInvalidValue;  // layer 1's weight gradient is reduced by mer_bn_relu_pool_bwd
}

// ---------------------------------------------------------------------------------------
// Backward of mer_adaptive_avgpool_seq, a gather: dx[b][c][h][w] = sum over the bins i whose column range
// [floor(i W / bins), ceil((i + 1) W / bins)) holds w (several when W < bins) of g[b][i][c] / (H * range length).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adaptive_avgpool_seq_bwd_kernel(long total, int C, int H, int W, int bins,
                                                                       const float* __restrict__ g,
                                                                       float* __restrict__ dx) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int w = (int)(e % W);
  const long bc = e / ((long)H * W);
  const int c = (int)(bc % C);
  const long b = bc / C;
  long lo = ((long)w * bins) / W - 1, hi = (((long)w + 1) * bins) / W + 1;
  lo = lo < 0 ? 0 : lo;
  hi = hi > bins - 1 ? bins - 1 : hi;
  float s = 0.f;
  for (long i = lo; i <= hi; ++i) {
    const int ws = (int)((i * W) / bins), we = (int)(((i + 1) * W + bins - 1) / bins);
    if (w >= ws && w < we) s += g[(b * bins + i) * C + c] / (float)(H * (we - ws));
  }
  dx[e] = s;
}

MER_API int mer_adaptive_avgpool_seq_bwd(int B, int C, int H, int W, int bins, const float* g, float* dx, void* stream) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || bins < 1 || !g || !dx) return (int)hipErrorInvalidValue;
  const long total = (long)B * C * H * W;
  if ((total + 255) / 256 > 0x7fffffffL || (long)H * W > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(adaptive_avgpool_seq_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, total, C, H, W, bins, g, dx);
  MER_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------
// SpecAugment's masked copy: y = x with the drawn frequency rows and time columns zeroed, one mask for the whole
// batch.  The bands travel in the kernel arguments.
// ---------------------------------------------------------------------------------------
struct SpecBands {
  int n;
  int start[MER_SPEC_AUGMENT_MAX_BANDS], len[MER_SPEC_AUGMENT_MAX_BANDS];
};

__global__ __launch_bounds__(256) void spec_augment_mask_kernel(long total, int n_mels, int T, SpecBands fb, SpecBands tb,
                                                                const float* __restrict__ x, float* __restrict__ y) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int t = (int)(e % T), f = (int)((e / T) % n_mels);
  bool keep = true;
#pragma unroll
  for (int i = 0; i < MER_SPEC_AUGMENT_MAX_BANDS; ++i) {
    if (i < fb.n && f >= fb.start[i] && f < fb.start[i] + fb.len[i]) keep = false;
    if (i < tb.n && t >= tb.start[i] && t < tb.start[i] + tb.len[i]) keep = false;
  }
  y[e] = keep ? x[e] : 0.f;
}

static bool fill_bands(SpecBands& s, int n, const int* bands, int size) {
  if (n < 0 || n > MER_SPEC_AUGMENT_MAX_BANDS || (n > 0 && !bands)) return false;
  s.n = n;
  for (int i = 0; i < MER_SPEC_AUGMENT_MAX_BANDS; ++i) {
    s.start[i] = i < n ? bands[2 * i] : 0;
    s.len[i] = i < n ? bands[2 * i + 1] : 0;
    if (s.start[i] < 0 || s.len[i] < 0 || (long)s.start[i] + s.len[i] > size) return false;
  }
  return true;
}

MER_API int mer_spec_augment_mask(long planes, int n_mels, int T, const float* x, float* y, int n_freq,
                                  const int* freq_bands, int n_time, const int* time_bands, void* stream) {
  if (planes < 1 || n_mels < 1 || T < 1 || !x || !y || x == y) return (int)hipErrorInvalidValue;
  SpecBands fb, tb;
  if (!fill_bands(fb, n_freq, freq_bands, n_mels) || !fill_bands(tb, n_time, time_bands, T))
    return (int)hipErrorInvalidValue;
  if (planes > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const long total = planes * n_mels * T;
  if ((total + 255) / 256 > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(spec_augment_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     total, n_mels, T, fb, tb, x, y);
  MER_LAUNCH_CHECK();
}
