// BatchNorm (finalize / apply / backward, the folds of the conv epilogues' partial rows) and pooling of the ResNet18
// trunk, channel-last bf16.
#include "common.h"
#include "mer.h"

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// ---------------------------------------------------------------------------------------
// BatchNorm2d (train mode), channel-last.  stats[c] = (sum, sumsq) over M = N*H*W values.
// finalize: ms[c] = (mean, rstd); running_mean = (1-mom) rm + mom*mean; running_var uses the
// unbiased variance (torch semantics); num_batches_tracked += 1.
// ---------------------------------------------------------------------------------------
// Forward statistics layout (mer.h MER_BN_STAT_ROWS): one row per output row tile of the conv (<= ceil(M/64)
// rows, unused rows zero) followed by 64 scratch rows.  Rows are summed in a fixed order: stage 1 (when
// there are more than 64 rows) folds contiguous row groups into the 64 scratch rows, stage 2 folds <= 64
// rows per channel -- deterministic whatever the tile size and block schedule were.
// Latency: a block here is a short chain (one wave-row of loads, a sum, an LDS meet), so every load of a
// thread's rows is issued before the first add (batches of 16 from clamped addresses, zero-selected) -- the
// loop that added as it loaded waited one memory latency per two rows.  The sum order is unchanged: a0 takes
// the thread's rows 0, 2, 4, ... and a1 rows 1, 3, 5, ... (rows r0 + pg + 4 i).
__global__ __launch_bounds__(256) void bn_stat_rows_fold_kernel(int C2, int rows, int per, const float* __restrict__ in,
                                                                float* __restrict__ out) {
  __shared__ float part[4][64];
  const int el = threadIdx.x & 63, pg = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el, grp = blockIdx.y;
  const int r0 = grp * per, r1 = min(rows, r0 + per);
  const int ec = e < C2 ? e : C2 - 1;
  const int n = r1 - (r0 + pg) > 0 ? (r1 - (r0 + pg) + 3) / 4 : 0;  // this thread's rows
  float a0 = 0.f, a1 = 0.f;
  for (int i0 = 0; i0 < n; i0 += 16) {
    float x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = r0 + pg + 4 * (i0 + i);
      x[i] = in[(long)(r < r1 ? r : r1 - 1) * C2 + ec];
    }
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      if (i0 + i < n) a0 += x[i];
      if (i0 + i + 1 < n) a1 += x[i + 1];
    }
  }
  part[pg][el] = a0 + a1;
  __syncthreads();
  if (pg == 0 && e < C2) out[(long)grp * C2 + e] = (part[0][el] + part[1][el]) + (part[2][el] + part[3][el]);
}

// 64 channels per block; the 4 waves split the (<= 64) rows, then meet in LDS
__global__ __launch_bounds__(256) void bn_finalize_kernel(int C, long M, int rows, const float* __restrict__ stats,
                                                          float eps, float momentum, float* __restrict__ ms,
                                                          float* __restrict__ rmean, float* __restrict__ rvar,
                                                          long long* __restrict__ nbt) {
  __shared__ float part[4][64][2];
  const int cl = threadIdx.x & 63, pg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  if (!stats) {  // eval mode: normalise with the running statistics, no update
    if (pg == 0 && c < C) {
      ms[2 * c] = rmean[c];
      ms[2 * c + 1] = rsqrtf(rvar[c] + eps);
    }
    return;
  }
  float sum = 0.f, sq = 0.f;
  {  // rows <= 64: this wave's <= 16 rows all in flight before the first add (same order)
    const int cc = c < C ? c : C - 1;
    float xs[16], xq[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = pg + 4 * i, pc = p < rows ? p : rows - 1;
      xs[i] = stats[(long)pc * 2 * C + 2 * cc];
      xq[i] = stats[(long)pc * 2 * C + 2 * cc + 1];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (pg + 4 * i < rows) {
        sum += xs[i];
        sq += xq[i];
      }
  }
  part[pg][cl][0] = sum;
  part[pg][cl][1] = sq;
  __syncthreads();
  if (pg != 0 || c >= C) return;
  sum = part[0][cl][0] + part[1][cl][0] + part[2][cl][0] + part[3][cl][0];
  sq = part[0][cl][1] + part[1][cl][1] + part[2][cl][1] + part[3][cl][1];
  const float mean = sum / M;
  const float var = fmaxf(sq / M - mean * mean, 0.f);
  ms[2 * c] = mean;
  ms[2 * c + 1] = rsqrtf(var + eps);
  if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean;
  if (rvar) rvar[c] = (1.f - momentum) * rvar[c] + momentum * var * ((float)M / (float)(M > 1 ? M - 1 : 1));
  if (nbt && c == 0) *nbt += 1;
}
// 64 < rows <= BN_WIDE_ROWS: the fold and the finalize in ONE launch (round 6).  16 waves per block; wave w sums rows
// w, w + 16, ... of the block's 64 columns (lane = column), the 16 wave partials meet in LDS and wave 0 adds them in a
// fixed pairwise order -- deterministic, like the two-stage form it replaces for ResNet18 layer2 / layer3 (784 / 196
// rows at B = 32), one ~5 us launch less per BatchNorm.  Every load of a thread's rows (NB <= 64 of them) is issued
// before the first add: the batches-of-16 loop waited one memory latency per batch, 4 per pass at 784 rows, and the
// finalize ran its sums and its sums of squares as two such passes (13.4 us per launch in the step trace).  The
// forward finalize's columns are the interleaved (sum, sumsq) pairs of 32 channels, so one pass carries both and the
// grid has twice the blocks.  The per-element order (even-ordinal rows into a0, odd into a1, then the wave tree) is
// the batched loop's, so the results are bitwise those of the round-6 kernels.
constexpr int BN_WIDE_ROWS = 1024;

template <int N>
__device__ __forceinline__ float pair_tree(const float* v, int stride) {
  if constexpr (N == 1) {
    return v[0];
  } else {
    return pair_tree<N / 2>(v, stride) + pair_tree<N / 2>(v + (N / 2) * stride, stride);
  }
}

// per-(wave, element) partial over rows w, w + 16, ... (< rows <= 16 * NB): x[r * ld + e]
// (32-bit offsets from the column's base: rows * ld < 2^31 for every caller, and 64 loads in flight fit in 128 VGPRs)
template <int NB>
__device__ __forceinline__ float wide_rows_sum(const float* __restrict__ x, int rows, int ld, int e, int w) {
  float v[NB];
  const float* __restrict__ xe = x + e;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int r = w + 16 * i;
    v[i] = xe[(r < rows ? r : rows - 1) * ld];
  }
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int i = 0; i < NB; i += 2) {
    if (w + 16 * i < rows) a0 += v[i];
    if (w + 16 * (i + 1) < rows) a1 += v[i + 1];
  }
  return a0 + a1;
}

template <int NB>
__device__ __forceinline__ void bn_finalize_wide_body(int C, long M, int rows, const float* __restrict__ stats,
                                                      float eps, float momentum, float* __restrict__ ms,
                                                      float* __restrict__ rmean, float* __restrict__ rvar,
                                                      long long* __restrict__ nbt, float (*part)[64]) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + l;  // column of the [rows][C][2] layout: channel col / 2, sum (even) / sumsq (odd)
  if (blockIdx.x * 64 >= 2 * C) return;  // (block-uniform: the paired launch's grid covers the wider record)
  part[w][l] = wide_rows_sum<NB>(stats, rows, 2 * C, col < 2 * C ? col : 2 * C - 1, w);
  __syncthreads();
  if (w != 0) return;
  const float tot = pair_tree<16>(&part[0][l], 64);
  const float sq = __shfl_xor(tot, 1, 64);
  const int c = col >> 1;
  if ((l & 1) || c >= C) return;
  const float sum = tot;
  const float mean = sum / M;
  const float var = fmaxf(sq / M - mean * mean, 0.f);
  ms[2 * c] = mean;
  ms[2 * c + 1] = rsqrtf(var + eps);
  if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean;
  if (rvar) rvar[c] = (1.f - momentum) * rvar[c] + momentum * var * ((float)M / (float)(M > 1 ? M - 1 : 1));
  if (nbt && c == 0) *nbt += 1;
}

template <int NB>
__global__ __launch_bounds__(1024) void bn_finalize_wide_kernel(int C, long M, int rows, const float* __restrict__ stats,
                                                                float eps, float momentum, float* __restrict__ ms,
                                                                float* __restrict__ rmean, float* __restrict__ rvar,
                                                                long long* __restrict__ nbt) {
  __shared__ float part[16][64];
  bn_finalize_wide_body<NB>(C, M, rows, stats, eps, momentum, ms, rmean, rvar, nbt, part);
}

// Two BatchNorms' finalizes in one launch (blockIdx.y = record): a stride-2 BasicBlock's bn2 and downsample BN, whose
// convs both end before either BatchNorm is applied -- one ~4-7 us launch less on the trunk stream per such block.
struct BnFinRec {
  int C, rows;
  long M;
  const float* stats;
  float *ms, *rmean, *rvar;
  long long* nbt;
};
struct BnFinPair {
  BnFinRec r[2];
};
template <int NB>
__global__ __launch_bounds__(1024) void bn_finalize_wide2_kernel(BnFinPair t, float eps, float momentum) {
  __shared__ float part[16][64];
  const bool y = blockIdx.y != 0;  // (uniform selects: an indexed kernel-argument record cost scratch at NB = 64)
  bn_finalize_wide_body<NB>(y ? t.r[1].C : t.r[0].C, y ? t.r[1].M : t.r[0].M, y ? t.r[1].rows : t.r[0].rows,
                            y ? t.r[1].stats : t.r[0].stats, eps, momentum, y ? t.r[1].ms : t.r[0].ms,
                            y ? t.r[1].rmean : t.r[0].rmean, y ? t.r[1].rvar : t.r[0].rvar,
                            y ? t.r[1].nbt : t.r[0].nbt, part);
}

// out[e] = sum over parts rows of in[p][e], e < 2C, for 64 < parts <= BN_WIDE_ROWS (one launch; see above)
template <int NB>
__global__ __launch_bounds__(1024) void partials_sum_wide_kernel(int C2, int parts, const float* __restrict__ in,
                                                                 float* __restrict__ out) {
  __shared__ float part[16][64];
  const int el = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el, ec = e < C2 ? e : C2 - 1;
  part[w][el] = wide_rows_sum<NB>(in, parts, C2, ec, w);
  __syncthreads();
  if (w == 0 && e < C2) out[e] = pair_tree<16>(&part[0][el], 64);
}
// two buffers of the same shape in one launch (blockIdx.y): a stride-2 block's bn2 and downsample-BN backward sums,
// which one fused dgrad epilogue produced
template <int NB>
__global__ __launch_bounds__(1024) void partials_sum_wide2_kernel(int C2, int parts, const float* __restrict__ in0,
                                                                  float* __restrict__ out0,
                                                                  const float* __restrict__ in1,
                                                                  float* __restrict__ out1) {
  __shared__ float part[16][64];
  const float* in = blockIdx.y ? in1 : in0;
  float* out = blockIdx.y ? out1 : out0;
  const int el = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el, ec = e < C2 ? e : C2 - 1;
  part[w][el] = wide_rows_sum<NB>(in, parts, C2, ec, w);
  __syncthreads();
  if (w == 0 && e < C2) out[e] = pair_tree<16>(&part[0][el], 64);
}

// the wide launches by row count: NB = 16 / 32 / 64 loads per thread
template <class F16, class F32, class F64>
static inline void wide_pick(int rows, F16 f16, F32 f32, F64 f64) {
  if (rows <= 256) f16();
  else if (rows <= 512) f32();
  else f64();
}

MER_API int mer_bn_finalize(int C, long M, const float* stats, float eps, float momentum, float* ms, float* rmean,
                            float* rvar, long long* num_batches_tracked, void* stream) {
  return mer_bn_finalize_rows(C, M, (int)((M + 63) / 64), stats, eps, momentum, ms, rmean, rvar, num_batches_tracked,
                              stream);
}

MER_API int mer_bn_finalize_rows2(int C, long M, int data_rows, const float* stats, float* ms, float* rmean, float* rvar,
                                  long long* nbt, int C2, long M2, int data_rows2, const float* stats2, float* ms2,
                                  float* rmean2, float* rvar2, long long* nbt2, float eps, float momentum,
                                  void* stream) {
  if (!stats || !stats2 || C <= 0 || C2 <= 0 || data_rows <= 0 || data_rows > (M + 63) / 64 || data_rows2 <= 0 ||
      data_rows2 > (M2 + 63) / 64)
    return (int)hipErrorInvalidValue;
  const int rows = data_rows > data_rows2 ? data_rows : data_rows2;
  if (rows > BN_WIDE_ROWS) {  // the two-stage folds, one after the other
    const int rc = mer_bn_finalize_rows(C, M, data_rows, stats, eps, momentum, ms, rmean, rvar, nbt, stream);
    return rc ? rc : mer_bn_finalize_rows(C2, M2, data_rows2, stats2, eps, momentum, ms2, rmean2, rvar2, nbt2, stream);
  }
  BnFinPair t{};
  t.r[0] = BnFinRec{C, data_rows, M, stats, ms, rmean, rvar, nbt};
  t.r[1] = BnFinRec{C2, data_rows2, M2, stats2, ms2, rmean2, rvar2, nbt2};
  const int cmax = C > C2 ? C : C2;
  const dim3 grid((2 * cmax + 63) / 64, 2);
  hipStream_t st = (hipStream_t)stream;
#define MER_BN_FIN2(NB) [&] { hipLaunchKernelGGL(bn_finalize_wide2_kernel<NB>, grid, dim3(1024), 0, st, t, eps, momentum); }
  wide_pick(rows, MER_BN_FIN2(16), MER_BN_FIN2(32), MER_BN_FIN2(64));
#undef MER_BN_FIN2
  MER_LAUNCH_CHECK();
}

MER_API int mer_bn_finalize_rows(int C, long M, int data_rows, const float* stats, float eps, float momentum, float* ms,
                                 float* rmean, float* rvar, long long* num_batches_tracked, void* stream) {
  if (!stats && (!rmean || !rvar)) return (int)hipErrorInvalidValue;
  const int all_rows = (int)((M + 63) / 64);  // MER_BN_STAT_ROWS(M) - 64: the scratch rows follow them
  if (data_rows <= 0 || data_rows > all_rows) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = data_rows;
  const float* src = stats;
  int rows = tiles;
  if (stats && tiles > 64 && tiles <= BN_WIDE_ROWS) {
    const dim3 grid((2 * C + 63) / 64);
#define MER_BN_FIN_WIDE(NB)                                                                                          \
  [&] {                                                                                                              \
    hipLaunchKernelGGL(bn_finalize_wide_kernel<NB>, grid, dim3(1024), 0, st, C, M, tiles, stats, eps, momentum, ms, \
                       rmean, rvar, num_batches_tracked);                                                            \
  }
    wide_pick(tiles, MER_BN_FIN_WIDE(16), MER_BN_FIN_WIDE(32), MER_BN_FIN_WIDE(64));
#undef MER_BN_FIN_WIDE
    MER_LAUNCH_CHECK();
  }
  if (stats && tiles > 64) {
    float* scratch = const_cast<float*>(stats) + (long)all_rows * 2 * C;
    const int per = (tiles + 63) / 64;
    hipLaunchKernelGGL(bn_stat_rows_fold_kernel, dim3((2 * C + 63) / 64, 64), dim3(256), 0, st, 2 * C, tiles, per,
                       stats, scratch);
    src = scratch;
    rows = 64;
  }
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 63) / 64), dim3(256), 0, st, C, M, rows, src, eps, momentum, ms,
                     rmean, rvar, num_batches_tracked);
  MER_LAUNCH_CHECK();
}

// y = [relu]( bn(x) + (res_bn ? bn2(res) : res) ), 8 channels per thread (C % 8 == 0).
// ms = (mean, rstd) pairs; eval mode passes (running_mean, 1/sqrt(running_var+eps)) the same way.
// BN is folded into one (scale, shift) per channel, computed once per block into LDS (C <= 512); a
// thread always owns the same 8 channels (256 % (C/8) == 0 and the grid stride is a multiple of 256) and
// streams two 16-byte vectors per iteration so the loads of both are in flight together.
__global__ __launch_bounds__(256) void bn_apply_kernel(long M, int C, const bf16_t* __restrict__ x,
                                                       const float* __restrict__ ms, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const bf16_t* __restrict__ res,
                                                       const float* __restrict__ ms2, const float* __restrict__ gamma2,
                                                       const float* __restrict__ beta2, int relu,
                                                       bf16_t* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float coef[4][512];  // scale, shift, scale2, shift2
  for (int c = threadIdx.x; c < C; c += 256) {
    const float sc = ms[2 * c + 1] * gamma[c];
    coef[0][c] = sc;
    coef[1][c] = beta[c] - ms[2 * c] * sc;
    float sc2 = 1.f, sh2 = 0.f;
    if (ms2) {
      sc2 = ms2[2 * c + 1] * gamma2[c];
      sh2 = beta2[c] - ms2[2 * c] * sc2;
    }
    coef[2][c] = sc2;
    coef[3][c] = sh2;
  }
  __syncthreads();
  const long nvec = M * C / 8;
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int c0 = (int)(tid0 % (C / 8)) * 8;
  float sc[8], sh[8], sc2[8], sh2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sc[i] = coef[0][c0 + i];
    sh[i] = coef[1][c0 + i];
    sc2[i] = coef[2][c0 + i];
    sh2[i] = coef[3][c0 + i];
  }
  auto one = [&](const u32x4& xv, const u32x4& rv) -> u32x4 {
    const bf16_t* xh = reinterpret_cast<const bf16_t*>(&xv);
    const bf16_t* rh = reinterpret_cast<const bf16_t*>(&rv);
    u32x4 ov;
    bf16_t* oh = reinterpret_cast<bf16_t*>(&ov);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float v = bf2f(xh[i]) * sc[i] + sh[i];
      if (res) v += bf2f(rh[i]) * sc2[i] + sh2[i];
      if (relu) v = fmaxf(v, 0.f);
      oh[i] = f2bf(v);
    }
    return ov;
  };
  const u32x4 z = {0u, 0u, 0u, 0u};
  long e = tid0;
  for (; e + stride < nvec; e += 2 * stride) {
    const u32x4 x0 = *reinterpret_cast<const u32x4*>(x + e * 8);
    const u32x4 x1 = *reinterpret_cast<const u32x4*>(x + (e + stride) * 8);
    const u32x4 r0 = res ? *reinterpret_cast<const u32x4*>(res + e * 8) : z;
    const u32x4 r1 = res ? *reinterpret_cast<const u32x4*>(res + (e + stride) * 8) : z;
    *reinterpret_cast<u32x4*>(y + e * 8) = one(x0, r0);
    *reinterpret_cast<u32x4*>(y + (e + stride) * 8) = one(x1, r1);
  }
  if (e < nvec) {
    const u32x4 x0 = *reinterpret_cast<const u32x4*>(x + e * 8);
    const u32x4 r0 = res ? *reinterpret_cast<const u32x4*>(res + e * 8) : z;
    *reinterpret_cast<u32x4*>(y + e * 8) = one(x0, r0);
  }
}
static int bn_stream_grid(long nvec) {
  const long g = (nvec + 1023) / 1024;  // ~4 vectors per thread
  return (int)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}

MER_API int mer_bn_apply(long M, int C, const void* x, const float* ms, const float* gamma, const float* beta,
                         const void* res, const float* ms2, const float* gamma2, const float* beta2, int relu, void* y,
                         void* stream) {
  if (C % 8 || C > 512 || 256 % (C / 8)) return (int)hipErrorInvalidValue;
  const long nvec = M * C / 8;
  const int grid = bn_stream_grid(nvec);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, M, C, (const bf16_t*)x, ms,
                     gamma, beta, (const bf16_t*)res, ms2, gamma2, beta2, relu, (bf16_t*)y);
  MER_LAUNCH_CHECK();
}

// BatchNorm folded to (scale, shift) for channel c from ms = (mean, rstd) pairs
__device__ __forceinline__ void stem_bn_coef(int c, const float* ms, const float* gamma, const float* beta, float& sc,
                                             float& sh) {
  sc = ms[2 * c + 1] * gamma[c];
  sh = beta[c] - ms[2 * c] * sc;
}

// BN backward reduction: g = dy * (mask > 0) (mask = the ReLU output, or null), xhat from x and ms:
//   red[c] = (sum g, sum g*xhat), one partial row per block folded in block order.  C <= 512, C % 8 == 0.
// BNMASK: no mask tensor; the ReLU mask is recomputed as bf16(relu(x*scale + shift)) > 0 from (ms, mgamma,
// mbeta) -- the fused stem, whose activation is never stored.
template <bool BNMASK>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(long M, int C, const bf16_t* __restrict__ dy,
                                                            const bf16_t* __restrict__ mask,
                                                            const bf16_t* __restrict__ x, const float* __restrict__ ms,
                                                            const float* __restrict__ mgamma,
                                                            const float* __restrict__ mbeta,
                                                            float* __restrict__ rows, long rows_per_block) {
  // per-thread sums over this block's rows, then the rows_per_iter threads of a channel chunk meet in LDS in
  // thread order and the block STORES its partial row: no atomics, deterministic
  __shared__ float part[2][2048];  // [s1|s2][tr * C + c], rows_per_iter * C <= 2048
  const int cpr = C / 8;                     // 16B chunks per row
  const int rows_per_iter = 256 / cpr > 0 ? 256 / cpr : 1;
  const int tc = threadIdx.x % cpr, tr = threadIdx.x / cpr;
  const long r0 = blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
  float s1[8] = {0.f}, s2[8] = {0.f};
  if (tr < rows_per_iter) {
    float mean[8], rstd[8], msc[8], msh[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      mean[i] = ms[2 * (tc * 8 + i)];
      rstd[i] = ms[2 * (tc * 8 + i) + 1];
      if (BNMASK) stem_bn_coef(tc * 8 + i, ms, mgamma, mbeta, msc[i], msh[i]);
    }
    // 4 rows per iteration with every load issued first (unconditional, from clamped rows; a row past r1
    // contributes exact zeros), so a thread has 8-12 loads in flight instead of one row's 2-3: the same rows
    // in the same order as a one-row loop, bit-identical sums
    for (long rb = r0 + tr; rb < r1; rb += 4 * rows_per_iter) {
      u32x4 gv[4], xv[4], mv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long r = rb + u * rows_per_iter;
        const long off = (r < r1 ? r : r1 - 1) * C + tc * 8;
        gv[u] = *reinterpret_cast<const u32x4*>(dy + off);
        xv[u] = *reinterpret_cast<const u32x4*>(x + off);
        mv[u] = u32x4{1u, 1u, 1u, 1u};
        if (!BNMASK && mask) mv[u] = *reinterpret_cast<const u32x4*>(mask + off);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool rowok = rb + u * rows_per_iter < r1;
        const bf16_t* gh = reinterpret_cast<const bf16_t*>(&gv[u]);
        const bf16_t* xh = reinterpret_cast<const bf16_t*>(&xv[u]);
        const bf16_t* mh = reinterpret_cast<const bf16_t*>(&mv[u]);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const bool live = BNMASK ? bf2f(f2bf(fmaxf(bf2f(xh[i]) * msc[i] + msh[i], 0.f))) > 0.f
                                   : (!mask || bf2f(mh[i]) > 0.f);
          const float g = (live && rowok) ? bf2f(gh[i]) : 0.f;
          if (rowok) {  // (a select: the loads above are unconditional)
            s1[i] += g;
            s2[i] += g * (bf2f(xh[i]) - mean[i]) * rstd[i];
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      part[0][tr * C + tc * 8 + i] = s1[i];
      part[1][tr * C + tc * 8 + i] = s2[i];
    }
  }
  __syncthreads();
  float* out = rows + (long)blockIdx.x * C * 2;
  for (int c = threadIdx.x; c < C; c += 256) {
    float a = 0.f, b = 0.f;
    for (int q = 0; q < rows_per_iter; ++q) {
      a += part[0][q * C + c];
      b += part[1][q * C + c];
    }
    out[2 * c] = a;
    out[2 * c + 1] = b;
  }
}
// rows_per_block keeps the block count <= 512 (the workspace holds MER_BN_RED_WS_ROWS = 512 + 64 rows)
static long bn_bwd_reduce_rpb(long M) { return (M + 511) / 512 > 32 ? (M + 511) / 512 : 32; }
static int partials_fold(int C, int parts, float* in, float* out, hipStream_t st);
MER_API int mer_bn_bwd_reduce(long M, int C, const void* dy, const void* mask, const void* x, const float* ms,
                              float* red, float* workspace, void* stream) {
  if (C % 8 || C > 512) return (int)hipErrorInvalidValue;
  const long rpb = bn_bwd_reduce_rpb(M);
  const int blocks = (int)((M + rpb - 1) / rpb);
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, M, C,
                     (const bf16_t*)dy, (const bf16_t*)mask, (const bf16_t*)x, ms, (const float*)nullptr,
                     (const float*)nullptr, workspace, rpb);
  return partials_fold(C, blocks, workspace, red, (hipStream_t)stream);
}

// out[c] = sum_p in[p][c] over `parts` partial rows of (a, b) pairs (fused-epilogue reductions), in a fixed
// order; 64 entries per block, the 4 waves split the rows, then meet in LDS.  More than 64 rows are first
// folded (bn_stat_rows_fold_kernel) into the 64 scratch rows the caller provides after them.
__global__ __launch_bounds__(256) void partials_sum_kernel(int C, int parts, const float* __restrict__ in,
                                                           float* __restrict__ out) {
  __shared__ float part[4][64];
  const int el = threadIdx.x & 63, pg = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el;
  float acc = 0.f;
  {  // parts <= 64: this wave's <= 16 rows all in flight before the first add (same order)
    const int ec = e < 2 * C ? e : 2 * C - 1;
    float x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = pg + 4 * i;
      x[i] = in[(long)(p < parts ? p : parts - 1) * 2 * C + ec];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (pg + 4 * i < parts) acc += x[i];
  }
  part[pg][el] = acc;
  __syncthreads();
  if (pg == 0 && e < 2 * C) out[e] = part[0][el] + part[1][el] + part[2][el] + part[3][el];
}
static int partials_fold(int C, int parts, float* in, float* out, hipStream_t st) {
  const float* src = in;
  if (parts > 64 && parts <= BN_WIDE_ROWS) {
    const dim3 grid((2 * C + 63) / 64);
#define MER_PSUM_WIDE(NB) \
  [&] { hipLaunchKernelGGL(partials_sum_wide_kernel<NB>, grid, dim3(1024), 0, st, 2 * C, parts, in, out); }
    wide_pick(parts, MER_PSUM_WIDE(16), MER_PSUM_WIDE(32), MER_PSUM_WIDE(64));
#undef MER_PSUM_WIDE
    MER_LAUNCH_CHECK();
  }
  if (parts > 64) {
    float* scratch = in + (long)parts * 2 * C;
    const int per = (parts + 63) / 64;
    hipLaunchKernelGGL(bn_stat_rows_fold_kernel, dim3((2 * C + 63) / 64, 64), dim3(256), 0, st, 2 * C, parts, per, in,
                       scratch);
    src = scratch;
    parts = 64;
  }
  hipLaunchKernelGGL(partials_sum_kernel, dim3((2 * C + 63) / 64), dim3(256), 0, st, C, parts, src, out);
  MER_LAUNCH_CHECK();
}
MER_API int mer_partials_sum(int C, int parts, float* in, float* out, void* stream) {
  if (C <= 0 || parts <= 0) return (int)hipErrorInvalidValue;
  return partials_fold(C, parts, in, out, (hipStream_t)stream);
}

MER_API int mer_partials_sum2(int C, int parts, float* in, float* out, float* in2, float* out2, void* stream) {
  if (C <= 0 || parts <= 0 || !in || !out || !in2 || !out2) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (parts > BN_WIDE_ROWS) {  // the two-stage folds, one after the other
    const int rc = partials_fold(C, parts, in, out, st);
    return rc ? rc : partials_fold(C, parts, in2, out2, st);
  }
  const dim3 grid((2 * C + 63) / 64, 2);
#define MER_PSUM2(NB) \
  [&] { hipLaunchKernelGGL(partials_sum_wide2_kernel<NB>, grid, dim3(1024), 0, st, 2 * C, parts, in, out, in2, out2); }
  wide_pick(parts, MER_PSUM2(16), MER_PSUM2(32), MER_PSUM2(64));
#undef MER_PSUM2
  MER_LAUNCH_CHECK();
}

// dx = gamma*rstd*(g - s1/M - xhat*s2/M) (bf16), and (block 0) dgamma += s2, dbeta += s1.
// Affine in (g, x) once the sums are known: dx = k1*g + k2*x + k0 per channel, the constants computed once
// per block into LDS; same thread/channel ownership and 2-vector streaming as bn_apply_kernel.
// (BNMASK as in bn_bwd_reduce_kernel; dy and dx may alias: every element is read, then written, by one thread)
template <bool BNMASK>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(long M, int C, const bf16_t* dy,
                                                           const bf16_t* __restrict__ mask,
                                                           const bf16_t* __restrict__ x, const float* __restrict__ ms,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ mbeta,
                                                           const float* __restrict__ red, int batch_stats,
                                                           bf16_t* dx, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta) {
  __shared__ __attribute__((aligned(16))) float coef[5][512];
  const float invM = 1.f / (float)M;
  for (int c = threadIdx.x; c < C; c += 256) {
    if (blockIdx.x == 0) {
      if (dgamma) dgamma[c] += red[2 * c + 1];
      if (dbeta) dbeta[c] += red[2 * c];
    }
    const float mu = ms[2 * c], rs = ms[2 * c + 1], gr = gamma[c] * rs;
    // batch statistics (train): the mean/var terms carry gradient; running stats (eval): they do not
    const float a = batch_stats ? red[2 * c] * invM : 0.f;
    const float b = batch_stats ? red[2 * c + 1] * invM : 0.f;
    const float t = gr * b * rs;  // (explicit rounding steps, shared with bn_bwd_apply2_kernel)
    coef[0][c] = gr;
    coef[1][c] = -t;
    coef[2][c] = fmaf(-gr, a, t * mu);
    if (BNMASK) stem_bn_coef(c, ms, gamma, mbeta, coef[3][c], coef[4][c]);
  }
  __syncthreads();
  const long nvec = M * C / 8;
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int c0 = (int)(tid0 % (C / 8)) * 8;
  float k1[8], k2[8], k0[8], msc[8], msh[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    k1[i] = coef[0][c0 + i];
    k2[i] = coef[1][c0 + i];
    k0[i] = coef[2][c0 + i];
    msc[i] = BNMASK ? coef[3][c0 + i] : 0.f;
    msh[i] = BNMASK ? coef[4][c0 + i] : 0.f;
  }
  auto one = [&](const u32x4& gv, const u32x4& xv, const u32x4& mv) -> u32x4 {
    const bf16_t* gh = reinterpret_cast<const bf16_t*>(&gv);
    const bf16_t* xh = reinterpret_cast<const bf16_t*>(&xv);
    const bf16_t* mh = reinterpret_cast<const bf16_t*>(&mv);
    u32x4 ov;
    bf16_t* oh = reinterpret_cast<bf16_t*>(&ov);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool live = BNMASK ? bf2f(f2bf(fmaxf(bf2f(xh[i]) * msc[i] + msh[i], 0.f))) > 0.f
                               : (!mask || bf2f(mh[i]) > 0.f);
      const float g = live ? bf2f(gh[i]) : 0.f;
      oh[i] = f2bf(fmaf(k1[i], g, fmaf(k2[i], bf2f(xh[i]), k0[i])));  // explicit: apply2 rounds the same
    }
    return ov;
  };
  const u32x4 one16 = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};  // bf16 1.0 (no mask)
  long e = tid0;
  for (; e + stride < nvec; e += 2 * stride) {
    const long e1 = e + stride;
    const u32x4 g0 = *reinterpret_cast<const u32x4*>(dy + e * 8);
    const u32x4 g1 = *reinterpret_cast<const u32x4*>(dy + e1 * 8);
    const u32x4 x0 = *reinterpret_cast<const u32x4*>(x + e * 8);
    const u32x4 x1 = *reinterpret_cast<const u32x4*>(x + e1 * 8);
    const u32x4 m0 = (!BNMASK && mask) ? *reinterpret_cast<const u32x4*>(mask + e * 8) : one16;
    const u32x4 m1 = (!BNMASK && mask) ? *reinterpret_cast<const u32x4*>(mask + e1 * 8) : one16;
    *reinterpret_cast<u32x4*>(dx + e * 8) = one(g0, x0, m0);
    *reinterpret_cast<u32x4*>(dx + e1 * 8) = one(g1, x1, m1);
  }
  if (e < nvec) {
    const u32x4 g0 = *reinterpret_cast<const u32x4*>(dy + e * 8);
    const u32x4 x0 = *reinterpret_cast<const u32x4*>(x + e * 8);
    const u32x4 m0 = (!BNMASK && mask) ? *reinterpret_cast<const u32x4*>(mask + e * 8) : one16;
    *reinterpret_cast<u32x4*>(dx + e * 8) = one(g0, x0, m0);
  }
}
MER_API int mer_bn_bwd_apply(long M, int C, const void* dy, const void* mask, const void* x, const float* ms,
                             const float* gamma, const float* red, int batch_stats, void* dx, float* dgamma,
                             float* dbeta, void* stream) {
  if (C % 8 || C > 512 || 256 % (C / 8)) return (int)hipErrorInvalidValue;
  const long nvec = M * C / 8;
  const int grid = bn_stream_grid(nvec);
  hipLaunchKernelGGL((bn_bwd_apply_kernel<false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, M, C,
                     (const bf16_t*)dy, (const bf16_t*)mask, (const bf16_t*)x, ms, gamma, (const float*)nullptr, red,
                     batch_stats, (bf16_t*)dx, dgamma, dbeta);
  MER_LAUNCH_CHECK();
}

// Two BatchNorm backward applies that read the same gradient and ReLU mask: a stride-2 BasicBlock's bn2 and its
// downsample BN (the block output relu(bn2(c2) + bn_d(cd)) fans its gradient out to both).  One pass loads g and the
// mask once for both outputs -- 12 instead of 16 bytes per element and one launch less -- with each output's
// per-element arithmetic exactly bn_bwd_apply_kernel<false>'s (bit-identical to two launches).
__global__ __launch_bounds__(256) void bn_bwd_apply2_kernel(long M, int C, const bf16_t* __restrict__ dy,
                                                            const bf16_t* __restrict__ mask,
                                                            const bf16_t* __restrict__ x, const float* __restrict__ ms,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ red,
                                                            const bf16_t* __restrict__ x2,
                                                            const float* __restrict__ ms2,
                                                            const float* __restrict__ gamma2,
                                                            const float* __restrict__ red2, int batch_stats,
                                                            bf16_t* __restrict__ dx, bf16_t* __restrict__ dx2,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            float* __restrict__ dgamma2, float* __restrict__ dbeta2) {
  __shared__ __attribute__((aligned(16))) float coef[6][512];
  const float invM = 1.f / (float)M;
  for (int c = threadIdx.x; c < C; c += 256) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* rd = h ? red2 : red;
      const float* m = h ? ms2 : ms;
      if (blockIdx.x == 0) {
        float* dg = h ? dgamma2 : dgamma;
        float* db = h ? dbeta2 : dbeta;
        if (dg) dg[c] += rd[2 * c + 1];
        if (db) db[c] += rd[2 * c];
      }
      const float mu = m[2 * c], rs = m[2 * c + 1], gr = (h ? gamma2 : gamma)[c] * rs;
      const float a = batch_stats ? rd[2 * c] * invM : 0.f;
      const float b = batch_stats ? rd[2 * c + 1] * invM : 0.f;
      const float t = gr * b * rs;
      coef[3 * h + 0][c] = gr;
      coef[3 * h + 1][c] = -t;
      coef[3 * h + 2][c] = fmaf(-gr, a, t * mu);
    }
  }
  __syncthreads();
  const long nvec = M * C / 8;
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int c0 = (int)(tid0 % (C / 8)) * 8;
  float k[6][8];
#pragma unroll
  for (int j = 0; j < 6; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) k[j][i] = coef[j][c0 + i];
  for (long e = tid0; e < nvec; e += stride) {
    const u32x4 gv = *reinterpret_cast<const u32x4*>(dy + e * 8);
    const u32x4 mv = *reinterpret_cast<const u32x4*>(mask + e * 8);
    const u32x4 xv = *reinterpret_cast<const u32x4*>(x + e * 8);
    const u32x4 x2v = *reinterpret_cast<const u32x4*>(x2 + e * 8);
    const bf16_t* gh = reinterpret_cast<const bf16_t*>(&gv);
    const bf16_t* mh = reinterpret_cast<const bf16_t*>(&mv);
    const bf16_t* xh = reinterpret_cast<const bf16_t*>(&xv);
    const bf16_t* x2h = reinterpret_cast<const bf16_t*>(&x2v);
    u32x4 ov, o2v;
    bf16_t* oh = reinterpret_cast<bf16_t*>(&ov);
    bf16_t* o2h = reinterpret_cast<bf16_t*>(&o2v);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float g = bf2f(mh[i]) > 0.f ? bf2f(gh[i]) : 0.f;
      oh[i] = f2bf(fmaf(k[0][i], g, fmaf(k[1][i], bf2f(xh[i]), k[2][i])));
      o2h[i] = f2bf(fmaf(k[3][i], g, fmaf(k[4][i], bf2f(x2h[i]), k[5][i])));
    }
    *reinterpret_cast<u32x4*>(dx + e * 8) = ov;
    *reinterpret_cast<u32x4*>(dx2 + e * 8) = o2v;
  }
}
MER_API int mer_bn_bwd_apply2(long M, int C, const void* dy, const void* mask, const void* x, const float* ms,
                              const float* gamma, const float* red, const void* x2, const float* ms2,
                              const float* gamma2, const float* red2, int batch_stats, void* dx, void* dx2,
                              float* dgamma, float* dbeta, float* dgamma2, float* dbeta2, void* stream) {
  if (C % 8 || C > 512 || 256 % (C / 8) || !mask || !x2 || !dx2 || dx == dy || dx2 == dy)
    return (int)hipErrorInvalidValue;
  const long nvec = M * C / 8;
  const int grid = bn_stream_grid(nvec);
  hipLaunchKernelGGL(bn_bwd_apply2_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, M, C, (const bf16_t*)dy,
                     (const bf16_t*)mask, (const bf16_t*)x, ms, gamma, red, (const bf16_t*)x2, ms2, gamma2, red2,
                     batch_stats, (bf16_t*)dx, (bf16_t*)dx2, dgamma, dbeta, dgamma2, dbeta2);
  MER_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 1) (resnet stem) channel-last, with the argmax tap (0..8) saved for backward.
// ---------------------------------------------------------------------------------------
// 8 channels (16 B) per thread.  The 16-byte-chunk index e = pixel * C/8 + chunk runs to N*H*W*C/8 < 2^30, far past
// fdiv's exact range (common.h: it is first wrong at 2^23 + 7 for C/8 = 8), so the chunk split is an integer one -- a
// shift where C/8 is a power of two (every trunk shape), a 32-bit divide otherwise -- and fdiv only decomposes the
// pixel index, which the launchers keep below 2^22.
__device__ __forceinline__ int chunk_div(int e, int cpr, int cpr_shift) {
  return cpr_shift >= 0 ? e >> cpr_shift : e / cpr;
}
static int chunk_shift(int cpr) { return (cpr & (cpr - 1)) ? -1 : __builtin_ctz((unsigned)cpr); }
// what the pooling launchers admit: pixels < 2^22 (fdiv, common.h) and chunks < 2^30 (32-bit e plus one grid stride)
static bool pool_index_ok(int N, int H, int W, int C) {
  const long pixels = (long)N * H * W;
  return N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && pixels < (1L << 22) && pixels * (C / 8) < (1L << 30);
}

__global__ void maxpool_fwd_kernel(int N, int H, int W, int C, int Ho, int Wo, int cpr_shift,
                                   const bf16_t* __restrict__ x, bf16_t* __restrict__ y, uint8_t* __restrict__ arg) {
  const int cpr = C / 8;
  const int total = N * Ho * Wo * cpr;
  const float inv_Wo = 1.f / Wo, inv_Ho = 1.f / Ho;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int q = chunk_div(e, cpr, cpr_shift);  // output pixel, < N*H*W < 2^22: fdiv below is exact
    const int c0 = (e - q * cpr) * 8;
    const int q2 = fdiv(q, inv_Wo);
    const int ow = q - q2 * Wo;
    const int n = fdiv(q2, inv_Ho);
    const int oh = q2 - n * Ho;
    float best[8];
    int bi[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { best[i] = -INFINITY; bi[i] = 0; }
    for (int r = 0; r < 3; ++r)
      for (int s = 0; s < 3; ++s) {
        const int ih = oh * 2 - 1 + r, iw = ow * 2 - 1 + s;
        if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
        const u32x4 v = *reinterpret_cast<const u32x4*>(x + (((long)n * H + ih) * W + iw) * C + c0);
        const bf16_t* vh = reinterpret_cast<const bf16_t*>(&v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float f = bf2f(vh[i]);
          if (f > best[i]) { best[i] = f; bi[i] = r * 3 + s; }  // first max wins, like torch
        }
      }
    u32x4 o;
    bf16_t* oh8 = reinterpret_cast<bf16_t*>(&o);
    uint2 a;
    uint8_t* a8 = reinterpret_cast<uint8_t*>(&a);
#pragma unroll
    for (int i = 0; i < 8; ++i) { oh8[i] = f2bf(best[i]); a8[i] = (uint8_t)bi[i]; }
    *reinterpret_cast<u32x4*>(y + (long)q * C + c0) = o;
    *reinterpret_cast<uint2*>(arg + (long)q * C + c0) = a;
  }
}
MER_API int mer_maxpool_fwd(int N, int H, int W, int C, const void* x, void* y, void* argmax, void* stream) {
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  if (!pool_index_ok(N, H, W, C)) return (int)hipErrorInvalidValue;
  const long total = (long)N * Ho * Wo * C / 8;
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, N, H, W, C, Ho, Wo,
                     chunk_shift(C / 8), (const bf16_t*)x, (bf16_t*)y, (uint8_t*)argmax);
  MER_LAUNCH_CHECK();
}
// gather backward: dx[n,h,w,c] = sum of dy over the (<= 4) windows whose argmax is (h,w)
__global__ void maxpool_bwd_kernel(int N, int H, int W, int C, int Ho, int Wo, int cpr_shift,
                                   const bf16_t* __restrict__ dy, const uint8_t* __restrict__ arg,
                                   bf16_t* __restrict__ dx) {
  const int cpr = C / 8;
  const int total = N * H * W * cpr;
  const float inv_W = 1.f / W, inv_H = 1.f / H;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int q = chunk_div(e, cpr, cpr_shift);  // (pixel q < 2^22: fdiv below is exact)
    const int c0 = (e - q * cpr) * 8;
    const int q2 = fdiv(q, inv_W);
    const int w = q - q2 * W;
    const int n = fdiv(q2, inv_H);
    const int h = q2 - n * H;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // the (<= 4) candidate windows: every load unconditional from a clamped window, invalid ones masked by the
    // tap test (a load under a per-lane branch waits for itself: 4 dependent round trips per thread)
    u32x4 gq[2][2];
    uint2 aq[2][2];
    int tap[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int oh = (h + 1) / 2 - 1 + a, ow = (w + 1) / 2 - 1 + b;
        const int r = h - (oh * 2 - 1), s = w - (ow * 2 - 1);
        const bool ok = oh >= 0 && oh < Ho && ow >= 0 && ow < Wo && r >= 0 && r <= 2 && s >= 0 && s <= 2;
        const int ohc = oh < 0 ? 0 : (oh >= Ho ? Ho - 1 : oh), owc = ow < 0 ? 0 : (ow >= Wo ? Wo - 1 : ow);
        const long oi = (((long)n * Ho + ohc) * Wo + owc) * C + c0;
        gq[a][b] = *reinterpret_cast<const u32x4*>(dy + oi);
        aq[a][b] = *reinterpret_cast<const uint2*>(arg + oi);
        tap[a][b] = ok ? r * 3 + s : -1;  // -1 matches no argmax
      }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const bf16_t* gh = reinterpret_cast<const bf16_t*>(&gq[a][b]);
        const uint8_t* a8 = reinterpret_cast<const uint8_t*>(&aq[a][b]);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if ((int)a8[i] == tap[a][b]) acc[i] += bf2f(gh[i]);
      }
    u32x4 o;
    bf16_t* oh8 = reinterpret_cast<bf16_t*>(&o);
#pragma unroll
    for (int i = 0; i < 8; ++i) oh8[i] = f2bf(acc[i]);
    *reinterpret_cast<u32x4*>(dx + (long)q * C + c0) = o;
  }
}
MER_API int mer_maxpool_bwd(int N, int H, int W, int C, const void* dy, const void* argmax, void* dx, void* stream) {
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  if (!pool_index_ok(N, H, W, C)) return (int)hipErrorInvalidValue;
  const long total = (long)N * H * W * C / 8;
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, N, H, W, C, Ho, Wo,
                     chunk_shift(C / 8), (const bf16_t*)dy, (const uint8_t*)argmax, (bf16_t*)dx);
  MER_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------
// Fused ResNet stem tail (video.py:21-23 -> torchvision conv1/bn1/relu/maxpool), channel-last, C = 64:
//   forward:  p = maxpool3x3s2p1( a ),  a = bf16(relu(x * scale + shift))  -- a is never stored;
//   backward: da = maxpool gather of dp (materialised once by maxpool_bwd), g = da * (a > 0) with the ReLU
//             mask recomputed from (x, BN) in the BatchNorm reduction and apply passes, so a is never stored
//             (gathering dp inside both passes instead was measured 2x slower: DESIGN.md section 4e).
// Same roundings, tap order and tie rule as bn_apply -> maxpool_fwd / maxpool_bwd -> bn_bwd_*.
// ---------------------------------------------------------------------------------------

__global__ void stem_bnrelu_maxpool_kernel(int N, int H, int W, int C, int Ho, int Wo, int cpr_shift,
                                           const bf16_t* __restrict__ x, const float* __restrict__ ms,
                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                           bf16_t* __restrict__ y, uint8_t* __restrict__ arg) {
  const int cpr = C / 8;
  const int total = N * Ho * Wo * cpr;
  const float inv_Wo = 1.f / Wo, inv_Ho = 1.f / Ho;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int q = chunk_div(e, cpr, cpr_shift);  // (as maxpool_fwd_kernel)
    const int c0 = (e - q * cpr) * 8;
    const int q2 = fdiv(q, inv_Wo);
    const int ow = q - q2 * Wo;
    const int n = fdiv(q2, inv_Ho);
    const int oh = q2 - n * Ho;
    float sc[8], sh[8], best[8];
    int bi[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      stem_bn_coef(c0 + i, ms, gamma, beta, sc[i], sh[i]);
      best[i] = -INFINITY;
      bi[i] = 0;
    }
    // all 9 taps loaded first, unconditionally from clamped pixels (branch-free: the loads are in flight
    // together), out-of-frame taps masked to -inf so they never win; same tap order and first-max tie rule
    u32x4 v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ih = oh * 2 - 1 + t / 3, iw = ow * 2 - 1 + t % 3;
      const int ihc = ih < 0 ? 0 : (ih >= H ? H - 1 : ih), iwc = iw < 0 ? 0 : (iw >= W ? W - 1 : iw);
      v[t] = *reinterpret_cast<const u32x4*>(x + (((long)n * H + ihc) * W + iwc) * C + c0);
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ih = oh * 2 - 1 + t / 3, iw = ow * 2 - 1 + t % 3;
      const bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
      const bf16_t* vh = reinterpret_cast<const bf16_t*>(&v[t]);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float f = ok ? bf2f(f2bf(fmaxf(bf2f(vh[i]) * sc[i] + sh[i], 0.f))) : -INFINITY;
        if (f > best[i]) { best[i] = f; bi[i] = t; }
      }
    }
    u32x4 o;
    bf16_t* oh8 = reinterpret_cast<bf16_t*>(&o);
    uint2 a;
    uint8_t* a8 = reinterpret_cast<uint8_t*>(&a);
#pragma unroll
    for (int i = 0; i < 8; ++i) { oh8[i] = f2bf(best[i]); a8[i] = (uint8_t)bi[i]; }
    *reinterpret_cast<u32x4*>(y + (long)q * C + c0) = o;
    *reinterpret_cast<uint2*>(arg + (long)q * C + c0) = a;
  }
}

MER_API int mer_stem_bnrelu_maxpool_fwd(int N, int H, int W, int C, const void* x, const float* ms, const float* gamma,
                                        const float* beta, void* y, void* argmax, void* stream) {
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  if (C > 512 || !pool_index_ok(N, H, W, C)) return (int)hipErrorInvalidValue;
  const long total = (long)N * Ho * Wo * C / 8;
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(stem_bnrelu_maxpool_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, N, H, W, C, Ho, Wo,
                     chunk_shift(C / 8), (const bf16_t*)x, ms, gamma, beta, (bf16_t*)y, (uint8_t*)argmax);
  MER_LAUNCH_CHECK();
}

MER_API int mer_stem_pool_bn_bwd(int N, int H, int W, int C, const void* dy, const void* argmax, const void* x,
                                 const float* ms, const float* gamma, const float* beta, float* red, int batch_stats,
                                 void* dx, float* dgamma, float* dbeta, float* workspace, void* stream) {
  if (C > 512 || !pool_index_ok(N, H, W, C) || 256 % (C / 8)) return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)stream;
  const long M = (long)N * H * W;
  // 1) maxpool gather backward into dx (as the pre-BN gradient); 2) BN reduction with the ReLU mask
  // recomputed from (x, BN); 3) BN apply in place over dx (each element read, then written, by one thread)
  int rc = mer_maxpool_bwd(N, H, W, C, dy, argmax, dx, stream);
  if (rc) return rc;
  const long rpb = bn_bwd_reduce_rpb(M);
  const int blocks = (int)((M + rpb - 1) / rpb);
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, M, C, (const bf16_t*)dx,
                     (const bf16_t*)nullptr, (const bf16_t*)x, ms, gamma, beta, workspace, rpb);
  rc = partials_fold(C, blocks, workspace, red, st);
  if (rc) return rc;
  hipLaunchKernelGGL((bn_bwd_apply_kernel<true>), dim3(bn_stream_grid(M * C / 8)), dim3(256), 0, st, M, C,
                     (const bf16_t*)dx, (const bf16_t*)nullptr, (const bf16_t*)x, ms, gamma, beta, red, batch_stats,
                     (bf16_t*)dx, dgamma, dbeta);
  MER_LAUNCH_CHECK();
}

// global average pool (AdaptiveAvgPool2d(1)): NHWC bf16 -> [N, C] fp32; backward broadcasts dy/HW.
__global__ void avgpool_fwd_kernel(int N, int HW, int C, const bf16_t* __restrict__ x, float* __restrict__ y) {
  const int n = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int p = 0; p < HW; ++p) s += bf2f(x[((long)n * HW + p) * C + c]);
  y[(long)n * C + c] = s / HW;
}
__global__ void avgpool_bwd_kernel(int N, int HW, int C, const float* __restrict__ dy, bf16_t* __restrict__ dx) {
  const int n = blockIdx.y;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < HW * C; e += gridDim.x * blockDim.x) {
    const int c = e % C;
    dx[(long)n * HW * C + e] = f2bf(dy[(long)n * C + c] / HW);
  }
}
MER_API int mer_avgpool_fwd(int N, int HW, int C, const void* x, float* y, void* stream) {
  hipLaunchKernelGGL(avgpool_fwd_kernel, dim3((C + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, N, HW, C,
                     (const bf16_t*)x, y);
  MER_LAUNCH_CHECK();
}
MER_API int mer_avgpool_bwd(int N, int HW, int C, const float* dy, void* dx, void* stream) {
  dim3 grid((HW * C + 255) / 256, N);
  hipLaunchKernelGGL(avgpool_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, N, HW, C, dy, (bf16_t*)dx);
  MER_LAUNCH_CHECK();
}
