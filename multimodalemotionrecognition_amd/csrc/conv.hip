// ResNet18 frame trunk (VideoNet.backbone, video.py:21-23 -> torchvision resnet18) on MFMA.
//
// Activations are NHWC bf16 (channels padded to a multiple of 8 so every 16-byte chunk of an
// im2col row is 8 channels of ONE tap).  Convolutions are implicit GEMMs on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation:
//   fwd   : Y[m=(n,oh,ow)][k]      = sum_{r,s,c} X[n, oh*st-pad+r, ow*st-pad+s, c] W[k][r][s][c]
//   dgrad : dX[m=(n,h,w)][c]       = sum_{r,s,k} dY[n, (h+pad-r)/st, (w+pad-s)/st, k] W'[c][r][s][k]
//           (taps whose (h+pad-r) is not a multiple of st contribute zero)
//   wgrad : dW[k][(r,s,c)]         = sum_{p=(n,oh,ow)} dY[p][k] X[n, oh*st-pad+r, ow*st-pad+s, c]
// fwd/dgrad stage K-contiguous tiles (ds_read_b128 fragments); wgrad reduces over pixels, so both
// operands are staged [pixel][channel] and read with the gfx950 LDS transpose (ds_read_b64_tr_b16).
// BatchNorm (train mode: batch statistics, running-stat update with momentum 0.1 / unbiased var)
// is split into a stats reduction fused into the conv epilogue, a finalize, and an apply pass.
// This unit holds the forward / input-gradient kernels, the tile plan and their entry points; the weight gradients
// are in conv_wgrad.hip, the packing kernels in conv_pack.hip, BatchNorm and pooling in bn_pool.hip.
#include "conv_common.h"
#include "mer.h"

// timing build: the halo kernel's stamps (CT) and conv_pipe_kernel's (CTP, tools/pipe_phases.py)
MER_CT_BUFFER(mer_ct, 512 * 64)
MER_CT_BUFFER(mer_ctp, 4096 * 8)
#define CT(k) CT_AT(mer_ct_buf, k)
#define CTP(k) CTP_AT(mer_ctp_buf, k)

namespace {

template <bool DGRAD>
__device__ __forceinline__ u32x4 conv_a_chunk(const ConvGeom& g, int n, int oh, int ow, bool rowok, int kk, int tap,
                                              int c, int r, int s) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (!rowok || kk >= g.Kred) return v;
  int ih, iw;
  if (!DGRAD) {
    ih = oh * g.st - g.pad + r;
    iw = ow * g.st - g.pad + s;
  } else {
    const int th = oh + g.pad - r, tw = ow + g.pad - s;
    if (th < 0 || tw < 0) return v;
    if (g.st == 1) {
      ih = th;
      iw = tw;
    } else if (g.st == 2) {
      if ((th | tw) & 1) return v;
      ih = th >> 1;
      iw = tw >> 1;
    } else {
      if ((th % g.st) || (tw % g.st)) return v;
      ih = th / g.st;
      iw = tw / g.st;
    }
  }
  if (ih < 0 || ih >= g.IH || iw < 0 || iw >= g.IW) return v;
  return *reinterpret_cast<const u32x4*>(g.X + (((long)n * g.IH + ih) * g.IW + iw) * g.IC + c);
}

// fwd / dgrad implicit GEMM. BM_ x BN_ tile, 4 waves as 2x2.
template <bool DGRAD, int BM_, int BN_>
__global__ __launch_bounds__(256, 2) void conv_kernel(ConvGeom g) {
  constexpr int LDK = CBK + 8;
  constexpr int IT = BM_ / 32, JT = BN_ / 32;           // 16x16 tiles per wave
  constexpr int ACH = BM_ * 8 / 256, BCH = BN_ * 8 / 256;  // 16B chunks per thread per K step
  __shared__ __attribute__((aligned(16))) bf16_t lds[2][(BM_ + BN_) * LDK];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int M = g.N * g.OH * g.OW;
  const int nx = (g.Ncols + BN_ - 1) / BN_, ny = (M + BM_ - 1) / BM_;
  int tx, ty;
  xcd_tile(blockIdx.x, nx, nx * ny, tx, ty);
  const int m0 = ty * BM_, n0 = tx * BN_;
  const int wm = (w >> 1) * (BM_ / 2), wn = (w & 1) * (BN_ / 2);
  const int crow = t >> 3, ckc = t & 7;

  int an[ACH], aoh[ACH], aow[ACH];
  bool aok[ACH];
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    const int m = m0 + crow + 32 * i;
    aok[i] = m < M;
    const int mm = aok[i] ? m : 0;
    an[i] = mm / (g.OH * g.OW);
    const int rem = mm - an[i] * g.OH * g.OW;
    aoh[i] = rem / g.OW;
    aow[i] = rem - aoh[i] * g.OW;
  }
  u32x4 ra[ACH], rb[BCH];
  const float inv_IC = 1.f / g.IC, inv_S = 1.f / g.S;
  auto gload = [&](int k0) {
    const int kk = k0 + ckc * 8;
    const int tap = fdiv(kk, inv_IC), c = kk - tap * g.IC;
    const int r = fdiv(tap, inv_S), s = tap - r * g.S;
#pragma unroll
    for (int i = 0; i < ACH; ++i) ra[i] = conv_a_chunk<DGRAD>(g, an[i], aoh[i], aow[i], aok[i], kk, tap, c, r, s);
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      const int n = n0 + crow + 32 * i;
      rb[i] = (n < g.Ncols && kk < g.Kred) ? *reinterpret_cast<const u32x4*>(g.Wt + (long)n * g.Kred + kk)
                                            : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < ACH; ++i)
      *reinterpret_cast<u32x4*>(&lds[buf][(crow + 32 * i) * LDK + ckc * 8]) = ra[i];
#pragma unroll
    for (int i = 0; i < BCH; ++i)
      *reinterpret_cast<u32x4*>(&lds[buf][(BM_ + crow + 32 * i) * LDK + ckc * 8]) = rb[i];
  };
  f32x4 acc[IT][JT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (g.Kred + CBK - 1) / CBK;
  gload(0);
  lstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * CBK);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int kof = s * 32 + (lane >> 4) * 8;
      bf16x8 af[IT], bfr[JT];
#pragma unroll
      for (int i = 0; i < IT; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(&lds[cur][(wm + i * 16 + (lane & 15)) * LDK + kof]);
#pragma unroll
      for (int j = 0; j < JT; ++j)
        bfr[j] = *reinterpret_cast<const bf16x8*>(&lds[cur][(BM_ + wn + j * 16 + (lane & 15)) * LDK + kof]);
#pragma unroll
      for (int i = 0; i < IT; ++i)
#pragma unroll
        for (int j = 0; j < JT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) lstore(cur ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < JT; ++j) {
    const int col = n0 + wn + j * 16 + (lane & 15);
    float csum = 0.f, csq = 0.f;
#pragma unroll
    for (int i = 0; i < IT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
        if (row < M && col < g.Ncols) {
          float v = acc[i][j][r];
          if (g.R_) {
            const long ri = (long)row * g.ldy + col;
            if (!g.Rmask || bf2f(g.Rmask[ri]) > 0.f) v += bf2f(g.R_[ri]);
          }
          const bf16_t h = f2bf(v);
          g.Y[(long)row * g.ldy + col] = h;
          const float hv = bf2f(h);
          csum += hv;
          csq += hv * hv;
        }
      }
    if (g.stats) {
      csum += __shfl_xor(csum, 16, 64);
      csum += __shfl_xor(csum, 32, 64);
      csq += __shfl_xor(csq, 16, 64);
      csq += __shfl_xor(csq, 32, 64);
      if ((lane >> 4) == 0 && col < g.Ncols) {
        float* slab = g.stats + (long)ty * g.Ncols * 2;  // this row tile's own stats row (exactly 2 adds onto 0: order-free)
        atomicAdd(slab + 2 * col, csum);
        atomicAdd(slab + 2 * col + 1, csq);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Pipelined fwd / dgrad implicit GEMM: the im2col A tile and the weight tile are DMA'd straight into
// LDS with global_load_lds (16 B per lane), the next K-tile issued before the current one is consumed
// (cdna_hip_programming.md §5 "Minimum 2-phase").  Same XOR-swizzled [rows][64] LDS image as
// gemm_bf16.hip's pipelined kernel.  Zero padding (spatial borders, dgrad's stride holes, K tail,
// rows past M / N) is served by pointing the lane at a 16-byte zero chunk in global memory.
// ---------------------------------------------------------------------------------------

__device__ __forceinline__ int cswz(int row, int c) { return c ^ ((row >> 1) & 7); }
// K-step of CW 16-byte chunks per LDS row: 8 (64-wide, 128-byte rows) or 4 (32-wide, 64-byte rows; four rows share
// a 256-byte bank row, so the XOR takes row bits 2-3 -- the 16 rows one ds_read_b128 lane group reads then cover
// all 16 bank slots)
template <int CW>
__device__ __forceinline__ int cswz_k(int row, int c) {
  return CW == 8 ? (c ^ ((row >> 1) & 7)) : (c ^ ((row >> 2) & 3));
}

template <bool DGRAD>
__device__ __forceinline__ const bf16_t* conv_a_src(const ConvGeom& g, int n, int oh, int ow, bool rowok, int kk,
                                                    float inv_IC, float inv_S) {
  const bf16_t* zero = reinterpret_cast<const bf16_t*>(mer_conv_zero16);
  if (!rowok || kk >= g.Kred) return zero;
  const int tap = fdiv(kk, inv_IC), c = kk - tap * g.IC;
  const int r = fdiv(tap, inv_S), s = tap - r * g.S;
  int ih, iw;
  if (!DGRAD) {
    ih = oh * g.st - g.pad + r;
    iw = ow * g.st - g.pad + s;
  } else {
    const int th = oh + g.pad - r, tw = ow + g.pad - s;
    if (th < 0 || tw < 0) return zero;
    if (g.st == 1) {
      ih = th;
      iw = tw;
    } else {
      if ((th | tw) & 1) return zero;  // st == 2 (checked on the host)
      ih = th >> 1;
      iw = tw >> 1;
    }
  }
  if (ih < 0 || ih >= g.IH || iw < 0 || iw >= g.IW) return zero;
  return g.X + (((long)n * g.IH + ih) * g.IW + iw) * g.IC + c;
}

// Stride-2 dgrad, parity-decomposed (PAR): an input pixel (h, w) only receives taps with
// (h + pad - r) and (w + pad - s) even, so the 4 parity classes (h&1, w&1) (blockIdx.y) are 4 dense
// implicit GEMMs over just their taps -- 1/4 of the MFMA work of the masked 9-tap form for 3x3 and none
// of its zero staging.  Class c: rows (n, hh, ww) -> pixel (n, 2hh+ph, 2ww+pw); taps r = r0 + 2ri,
// s = s0 + 2si with r0 = (ph + pad) & 1; source row ih = hh + (ph + pad - r0)/2 - ri.
struct ParClass {
  int ph, pw, Hc, Wc, r0, s0, nr, ns, dh0, dw0;
};

// Parity class of this block: grid.y walks the classes longest first (3 = odd/odd: 4 taps of a 3x3, then 2, 2, 1)
// -- blocks dispatch y-major, so the long class-3 tiles start first and the short ones fill the tail.
__device__ __forceinline__ int par_cls() { return 3 - (int)blockIdx.y; }

__device__ __forceinline__ ParClass par_class(const ConvGeom& g, int cls) {
  ParClass c;
  c.ph = cls >> 1;
  c.pw = cls & 1;
  c.Hc = (g.OH - c.ph + 1) >> 1;
  c.Wc = (g.OW - c.pw + 1) >> 1;
  c.r0 = (c.ph + g.pad) & 1;
  c.s0 = (c.pw + g.pad) & 1;
  c.nr = (g.R - c.r0 + 1) >> 1;
  c.ns = (g.S - c.s0 + 1) >> 1;
  c.dh0 = (c.ph + g.pad - c.r0) >> 1;
  c.dw0 = (c.pw + g.pad - c.s0) >> 1;
  return c;
}

// Forward BatchNorm statistics of one output tile from the accumulator layout (column = lane & 15: two shuffles per
// value; acc holds the stored, bf16-rounded outputs).  The cross-wave exchanges here and in conv_epilogue_vec go
// through LDS only, so they use lds_barrier() (lgkmcnt(0) + s_barrier): a __syncthreads() would also drain every
// outstanding global store and DMA (vmcnt(0)), which the persistent halo kernel overlaps with its next tile.  The WM waves sharing a column meet in LDS (red: >= WM*WN*TN*2
// idle floats) in wave order; the block then STORES its per-column (sum, sumsq) into stats row stat_row -- every (row
// tile, column) has exactly one writer, so the statistics (and every BatchNorm output) are bitwise deterministic.
// the lane's partial (sum, sumsq) of its accumulator-layout columns j * 16 + (lane & 15) over its rows (< M)
template <int FM, int FN, int WM, int WN>
__device__ __forceinline__ void conv_tile_stats_lane(const ConvGeom& g, const f32x4 (&acc)[FM][FN], int w, int lane,
                                                     int m0, int n0, int M, float (&part)[FN][2]) {
  constexpr int TM = FM * 16, TN = FN * 16;
  const int wr = w / WN, wc = w % WN, fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int col = n0 + wc * TN + j * 16 + fr;
    float csum = 0.f, csq = 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wr * TM + i * 16 + fq * 4 + r;
        if (row < M && col < g.Ncols) {
          const float hv = acc[i][j][r];
          csum += hv;
          csq += hv * hv;
        }
      }
    part[j][0] = csum;
    part[j][1] = csq;
  }
}

// lane partials -> the block's per-column (sum, sumsq) row: two shuffles per value, the WM waves of a column meet in
// LDS (red) in wave order, one writer per element
template <int FN, int WM, int WN>
__device__ __forceinline__ void conv_stats_finish(const ConvGeom& g, float (&part)[FN][2], float* red, int w, int lane,
                                                  int n0, long stat_row) {
  constexpr int TN = FN * 16;
  const int wr = w / WN, wc = w % WN, fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int j = 0; j < FN; ++j)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      part[j][q] += __shfl_xor(part[j][q], 16, 64);
      part[j][q] += __shfl_xor(part[j][q], 32, 64);
    }
  lds_barrier();
  if (wr > 0 && fq == 0)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      red[((wr * WN + wc) * FN * 16 + j * 16 + fr) * 2] = part[j][0];
      red[((wr * WN + wc) * FN * 16 + j * 16 + fr) * 2 + 1] = part[j][1];
    }
  lds_barrier();
  if (wr == 0 && fq == 0) {
    float* slab = g.stats + stat_row * g.Ncols * 2;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int col = n0 + wc * TN + j * 16 + fr;
      float t0 = part[j][0], t1 = part[j][1];
#pragma unroll
      for (int q = 1; q < WM; ++q) {
        t0 += red[((q * WN + wc) * FN * 16 + j * 16 + fr) * 2];
        t1 += red[((q * WN + wc) * FN * 16 + j * 16 + fr) * 2 + 1];
      }
      if (col < g.Ncols) {
        slab[2 * col] = t0;
        slab[2 * col + 1] = t1;
      }
    }
  }
}

template <int FM, int FN, int WM, int WN>
__device__ __forceinline__ void conv_tile_stats(const ConvGeom& g, const f32x4 (&acc)[FM][FN], float* red, int w,
                                                int lane, int m0, int n0, int M, long stat_row) {
  float part[FN][2];
  conv_tile_stats_lane<FM, FN, WM, WN>(g, acc, w, lane, m0, n0, M, part);
  conv_stats_finish<FN, WM, WN>(g, part, red, w, lane, n0, stat_row);
}

// Running per-lane partial sums of a persistent workgroup's tiles (conv_halo_kernel): each tile's fused column
// reductions add into these -- every tile of a workgroup covers the same output columns -- and the cross-lane /
// cross-wave reduction and the partial-row store run ONCE per workgroup (conv_epilogue_acc_finish), not once per tile.
// (vector types rather than arrays: a float[8] member left in scratch once the finish's 16-byte stores were
// vectorised over it)
typedef __attribute__((ext_vector_type(8))) float f32x8;
template <int FN>
struct EpiAcc {
  f32x8 sA, sB, sC;  // dgrad: the BN-backward sums of the lane's 8 pass-layout columns
  float fs[FN][2];   // fwd: the BN statistics of the lane's accumulator-layout columns
  __device__ void zero() {
    sA = sB = sC = f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < FN; ++j) fs[j][0] = fs[j][1] = 0.f;
  }
};
struct EpiNoAcc {};

// The 16-byte conv epilogue: each wave stages fp32 accumulators of 16-row groups of its TM x TN sub-tile in its own
// slice (WAVE_FLOATS floats at smemf + w * WAVE_FLOATS, idle LDS), then every lane owns 8 consecutive columns of one
// row per pass: 16-byte residual / mask / BN-operand loads and one 16-byte bf16 store instead of 2-byte accesses per
// element.  The fused column reductions (forward BN statistics of the stored bf16 values into stats row stat_row; the
// dgrad's BN-backward sums into bnr_red row red_row_id) accumulate per lane over its rows, then meet across the lanes
// sharing the columns (xor tree) and across the WM waves of a column (LDS, wave order): one writer per partial-row
// element, fixed order.  out_row(row) = the output pixel of GEMM row `row`.  Called by every wave of the workgroup.
// The epilogue's pass geometry: each wave stages GI 16-row groups at a time; a pass moves RPP rows, one per lane
// group of LPR lanes (8 columns each)
template <int FM, int FN, int WAVE_FLOATS>
struct EpiGeo {
  static constexpr int TM = FM * 16, TN = FN * 16, LDT = TN + 4;
  static constexpr int GI0 = WAVE_FLOATS / (16 * LDT);
  static constexpr int GI = GI0 < FM ? GI0 : FM;
  static constexpr int LPR = TN / 8, RPP = 64 / LPR;
  static constexpr int PPG = (GI * 16 + RPP - 1) / RPP;  // passes per staged group
  static constexpr int NP = ((FM + GI - 1) / GI) * PPG;  // passes per tile
};

// The dgrad epilogue's global operands (residual, residual mask, BN mask, BN input(s), BN (mean, rstd) of its 8
// columns), loaded AHEAD of the epilogue -- conv_halo_kernel issues them before its K loop, so their latency hides
// under the MFMAs instead of stalling the epilogue's passes one after another.  Same addresses as the in-epilogue
// loads (rows past M clamped to row M - 1; those passes discard them).
template <int NP>
struct EpiPre {
  u32x4 r[NP], m[NP], bm[NP], x[NP], x2[NP];
  float mu[8], rs[8], mu2[8], rs2[8];
};
struct EpiNone {};

template <bool DGRAD, int FM, int FN, int WM, int WN, int WAVE_FLOATS, class OutRow, int NP, bool X2 = true>
__device__ __forceinline__ void conv_epilogue_prefetch(const ConvGeom& g, EpiPre<NP>& pre, int w, int lane, int m0,
                                                       int n0, int M, OutRow out_row) {
  using E = EpiGeo<FM, FN, WAVE_FLOATS>;
  static_assert(NP == E::NP, "prefetch pass count");
  const int wr = w / WN, wc = w % WN;
  const int lr = lane / E::LPR, lc = (lane % E::LPR) * 8;
  const int colv = n0 + wc * E::TN + lc;
  const bool cok = colv < g.Ncols;
  const bool do_bnr = DGRAD && g.bnr_red != nullptr;
  const bool has_x2 = X2 && do_bnr && g.bnr_x2 != nullptr;
  const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int col = cok ? colv + e : 0;
    pre.mu[e] = do_bnr ? g.bnr_ms[2 * col] : 0.f;
    pre.rs[e] = do_bnr ? g.bnr_ms[2 * col + 1] : 0.f;
    pre.mu2[e] = has_x2 ? g.bnr_ms2[2 * col] : 0.f;
    pre.rs2[e] = has_x2 ? g.bnr_ms2[2 * col + 1] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int i0 = (q / E::PPG) * E::GI, rr = (q % E::PPG) * E::RPP;
    int row = m0 + wr * E::TM + i0 * 16 + rr + lr;
    row = row < M ? row : M - 1;
    const long e0 = out_row(row) * g.ldy + (cok ? colv : 0);
    pre.r[q] = (DGRAD && g.R_) ? *reinterpret_cast<const u32x4*>(g.R_ + e0) : z;
    pre.m[q] = (DGRAD && g.R_ && g.Rmask) ? *reinterpret_cast<const u32x4*>(g.Rmask + e0) : z;
    pre.bm[q] = do_bnr ? *reinterpret_cast<const u32x4*>(g.bnr_mask + e0) : z;
    pre.x[q] = do_bnr ? *reinterpret_cast<const u32x4*>(g.bnr_x + e0) : z;
    pre.x2[q] = has_x2 ? *reinterpret_cast<const u32x4*>(g.bnr_x2 + e0) : z;
  }
}

template <bool DGRAD, int FM, int FN, int WM, int WN, int WAVE_FLOATS, class OutRow, class Pre = EpiNone,
          bool DEFER = false, bool X2 = true, class AccT = EpiNoAcc>
__device__ __forceinline__ void conv_epilogue_vec(const ConvGeom& g, f32x4 (&acc)[FM][FN], float* smemf, int w,
                                                  int lane, int m0, int n0, int M, long red_row_id, long stat_row,
                                                  OutRow out_row, const Pre* pre = nullptr, int ct_slot = -1,
                                                  AccT* accp = nullptr) {
  constexpr bool PREF = !std::is_same<Pre, EpiNone>::value;
  constexpr bool ACC = !std::is_same<AccT, EpiNoAcc>::value;  // add the reductions into *accp, store nothing
  using E = EpiGeo<FM, FN, WAVE_FLOATS>;
  constexpr int TM = FM * 16, TN = FN * 16;
  const int wr = w / WN, wc = w % WN, fr = lane & 15, fq = lane >> 4;
  constexpr int LDT = TN + 4;
  constexpr int GI = E::GI;
  static_assert(GI >= 1, "epilogue staging slice too small");
  constexpr int LPR = TN / 8, RPP = 64 / LPR;
  float* wl = smemf + w * WAVE_FLOATS;
  const int lr = lane / LPR, lc = (lane % LPR) * 8;
  const int colv = n0 + wc * TN + lc;
  const bool cok = colv < g.Ncols;
  const bool do_bnr = DGRAD && g.bnr_red != nullptr;
  const bool has_x2 = X2 && do_bnr && g.bnr_x2 != nullptr;  // X2 = false: compiled out (24 VGPRs)
  float mu[8], rs[8], mu2[8], rs2[8];
  float sA[8], sB[8], sC[8];
  // DEFER (the halo kernel): the 16-byte output stores are issued LAST, after the cross-wave reductions -- a wave
  // stalled issuing stores would otherwise hold every other wave at the reductions' barriers (the store queue
  // drains ~16 B/clk per CU).  The deferred stores hold ~40 VGPRs, which cost conv_pipe_kernel's 8-wave dgrad
  // tiles their second block per CU (127 -> 150 VGPRs: layer2's dgrads 37 -> 56 us), so it stores per pass.
  constexpr int NPS = DEFER ? E::NP : 1;
  u32x4 pend[NPS];
  long pend_at[NPS];
  bool pend_ok[NPS];
#pragma unroll
  for (int q = 0; q < NPS; ++q) pend_ok[q] = false;
  auto flush = [&]() {
#pragma unroll
    for (int q = 0; q < NPS; ++q)
      if (pend_ok[q]) *reinterpret_cast<u32x4*>(g.Y + pend_at[q]) = pend[q];
  };
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if constexpr (PREF) {
      mu[e] = pre->mu[e];
      rs[e] = pre->rs[e];
      mu2[e] = pre->mu2[e];
      rs2[e] = pre->rs2[e];
    } else {
      const int col = cok ? colv + e : 0;
      mu[e] = do_bnr ? g.bnr_ms[2 * col] : 0.f;
      rs[e] = do_bnr ? g.bnr_ms[2 * col + 1] : 0.f;
      mu2[e] = has_x2 ? g.bnr_ms2[2 * col] : 0.f;
      rs2[e] = has_x2 ? g.bnr_ms2[2 * col + 1] : 0.f;
    }
    sA[e] = sB[e] = sC[e] = 0.f;
  }
#pragma unroll
  for (int i0 = 0; i0 < FM; i0 += GI) {
#pragma unroll
    for (int ii = 0; ii < GI; ++ii) {
      if (i0 + ii >= FM) break;
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) wl[(ii * 16 + fq * 4 + r) * LDT + j * 16 + fr] = acc[i0 + ii][j][r];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int nrows = (FM - i0 < GI ? FM - i0 : GI) * 16;
#pragma unroll
    for (int rr = 0; rr < GI * 16; rr += RPP) {
      const int rl = rr + lr;
      const int row = m0 + wr * TM + i0 * 16 + rl;
      if (rl < nrows && row < M && cok) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(&wl[rl * LDT + lc]);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(&wl[rl * LDT + lc + 4]);
        float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        const long e0 = out_row(row) * g.ldy + colv;
        const int q = (i0 / GI) * E::PPG + rr / RPP;  // this pass's prefetch slot (static once the loops unroll)
        if (DGRAD && g.R_) {
          u32x4 rv, mv;
          if constexpr (PREF) {
            rv = pre->r[q];
            mv = g.Rmask ? pre->m[q] : u32x4{1u, 1u, 1u, 1u};
          } else {
            rv = *reinterpret_cast<const u32x4*>(g.R_ + e0);
            mv = g.Rmask ? *reinterpret_cast<const u32x4*>(g.Rmask + e0) : u32x4{1u, 1u, 1u, 1u};
          }
          const bf16_t* rh = reinterpret_cast<const bf16_t*>(&rv);
          const bf16_t* mh = reinterpret_cast<const bf16_t*>(&mv);
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (!g.Rmask || bf2f(mh[e]) > 0.f) v[e] += bf2f(rh[e]);
        }
        u32x4 ov;
        bf16_t* oh = reinterpret_cast<bf16_t*>(&ov);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          oh[e] = f2bf(v[e]);
          v[e] = bf2f(oh[e]);  // the stored value feeds the reductions
        }
        if constexpr (DEFER) {
          pend[q] = ov;
          pend_at[q] = e0;
          pend_ok[q] = true;
        } else {
          *reinterpret_cast<u32x4*>(g.Y + e0) = ov;
        }
        if (do_bnr) {
          u32x4 mv, xv, x2v;
          if constexpr (PREF) {
            mv = pre->bm[q];
            xv = pre->x[q];
            x2v = pre->x2[q];
          } else {
            mv = *reinterpret_cast<const u32x4*>(g.bnr_mask + e0);
            xv = *reinterpret_cast<const u32x4*>(g.bnr_x + e0);
            x2v = has_x2 ? *reinterpret_cast<const u32x4*>(g.bnr_x2 + e0) : u32x4{0u, 0u, 0u, 0u};
          }
          const bf16_t* mh = reinterpret_cast<const bf16_t*>(&mv);
          const bf16_t* xh = reinterpret_cast<const bf16_t*>(&xv);
          const bf16_t* x2h = reinterpret_cast<const bf16_t*>(&x2v);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float gv = bf2f(mh[e]) > 0.f ? v[e] : 0.f;
            sA[e] += gv;
            sB[e] += gv * (bf2f(xh[e]) - mu[e]) * rs[e];
            if (has_x2) sC[e] += gv * (bf2f(x2h[e]) - mu2[e]) * rs2[e];
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (ct_slot >= 0) CT(ct_slot);
  if constexpr (ACC) {
    if (do_bnr) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        accp->sA[e] += sA[e];
        accp->sB[e] += sB[e];
        accp->sC[e] += sC[e];
      }
      flush();
      return;
    }
  }
  if (do_bnr) {
  // lanes sharing this lane's 8 columns: lane % LPR equal -> xor over the row bits of the lane index
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sA[e] += __shfl_xor(sA[e], o, 64);
      sB[e] += __shfl_xor(sB[e], o, 64);
      if (has_x2) sC[e] += __shfl_xor(sC[e], o, 64);
    }
  if (ct_slot >= 0) CT(ct_slot + 3);
  // the WM waves of a column range meet in LDS: red[(wr*WN + wc)][TN][3]
  float* red = smemf;
  lds_barrier();  // every wave is past its staging slice
  if (ct_slot >= 0) CT(ct_slot + 4);
  if (wr > 0 && lane < LPR)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float* o = red + ((wr * WN + wc) * TN + lc + e) * 3;
      o[0] = sA[e];
      o[1] = sB[e];
      o[2] = sC[e];
    }
  lds_barrier();
  if (wr != 0 || lane >= LPR || !cok) {
    flush();
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int q = 1; q < WM; ++q) {
      const float* o = red + ((q * WN + wc) * TN + lc + e) * 3;
      sA[e] += o[0];
      sB[e] += o[1];
      sC[e] += o[2];
    }
  {
    const long slab = red_row_id * g.Ncols * 2 + 2 * colv;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      *reinterpret_cast<f32x4*>(g.bnr_red + slab + 2 * e) = f32x4{sA[e], sB[e], sA[e + 1], sB[e + 1]};
      if (g.bnr_red2)
        *reinterpret_cast<f32x4*>(g.bnr_red2 + slab + 2 * e) = f32x4{sA[e], sC[e], sA[e + 1], sC[e + 1]};
    }
  }
  if (ct_slot >= 0) CT(ct_slot + 1);
  flush();
  if (ct_slot >= 0) CT(ct_slot + 2);
  return;
  }  // do_bnr
  if (!g.stats) {
    flush();
    return;
  }
  // forward BN statistics from the accumulator layout (column = lane & 15: two shuffles per value, cheaper than
  // the 8-column lane reduction) over the stored, bf16-rounded values
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = bf2f(f2bf(acc[i][j][r]));
  if constexpr (ACC) {
    float part[FN][2];
    conv_tile_stats_lane<FM, FN, WM, WN>(g, acc, w, lane, m0, n0, M, part);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      accp->fs[j][0] += part[j][0];
      accp->fs[j][1] += part[j][1];
    }
    flush();
    return;
  }
  conv_tile_stats<FM, FN, WM, WN>(g, acc, smemf, w, lane, m0, n0, M, stat_row);
  if (ct_slot >= 0) CT(ct_slot + 1);
  flush();
  if (ct_slot >= 0) CT(ct_slot + 2);
}

// The workgroup's accumulated reductions (EpiAcc) -> its one partial row: the dgrad's BN-backward sums meet across the
// lanes sharing columns (xor tree) and the WM waves (LDS, wave order) as in conv_epilogue_vec; the forward statistics
// as in conv_stats_finish.  Called by every wave, with smemf free LDS.
template <bool DGRAD, int FM, int FN, int WM, int WN, int WAVE_FLOATS, bool X2 = true>
__device__ __forceinline__ void conv_epilogue_acc_finish(const ConvGeom& g, EpiAcc<FN>& a, float* smemf, int w,
                                                         int lane, int n0, long row_id) {
  if constexpr (DGRAD) {
    if (!g.bnr_red) return;
    using E = EpiGeo<FM, FN, WAVE_FLOATS>;
    constexpr int TN = FN * 16, LPR = E::LPR;
    const int wr = w / WN, wc = w % WN;
    const int lc = (lane % LPR) * 8;
    const int colv = n0 + wc * TN + lc;
    const bool cok = colv < g.Ncols;
    const bool has_x2 = X2 && g.bnr_x2 != nullptr;
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a.sA[e] += __shfl_xor(a.sA[e], o, 64);
        a.sB[e] += __shfl_xor(a.sB[e], o, 64);
        if (has_x2) a.sC[e] += __shfl_xor(a.sC[e], o, 64);
      }
    float* red = smemf;
    lds_barrier();
    if (wr > 0 && lane < LPR)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float* o = red + ((wr * WN + wc) * TN + lc + e) * 3;
        o[0] = a.sA[e];
        o[1] = a.sB[e];
        o[2] = a.sC[e];
      }
    lds_barrier();
    if (wr != 0 || lane >= LPR || !cok) return;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int q = 1; q < WM; ++q) {
        const float* o = red + ((q * WN + wc) * TN + lc + e) * 3;
        a.sA[e] += o[0];
        a.sB[e] += o[1];
        a.sC[e] += o[2];
      }
    const long slab = row_id * g.Ncols * 2 + 2 * colv;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      *reinterpret_cast<f32x4*>(g.bnr_red + slab + 2 * e) = f32x4{a.sA[e], a.sB[e], a.sA[e + 1], a.sB[e + 1]};
      if (g.bnr_red2)
        *reinterpret_cast<f32x4*>(g.bnr_red2 + slab + 2 * e) = f32x4{a.sA[e], a.sC[e], a.sA[e + 1], a.sC[e + 1]};
    }
  } else {
    if (!g.stats) return;
    conv_stats_finish<FN, WM, WN>(g, a.fs, smemf, w, lane, n0, row_id);
  }
}

// Minimum waves per SIMD of a conv_pipe_kernel block of nw waves: 16-wave blocks 1 per CU, 8-wave blocks 2 per CU --
// except the tiles that would spill at 128 VGPRs (the 256-row dgrad tiles and the 3-deep 128 x 128 dgrad ring, none of
// them a default pick), which keep one block per CU; 4-wave blocks 2 per CU.
// A block whose LDS leaves no room for a second one on the CU (160 KB) asks for nw / 4 (its own waves only).
constexpr int conv_pipe_wpe(int nw, int bm, int bn, int stages, bool dgrad, bool par, int lds_bytes = 0) {
  return (nw >= 16 || 2 * lds_bytes > 160 * 1024)
             ? (nw >= 4 ? nw / 4 : 1)
             : nw == 8 ? ((dgrad && (bm == 256 || (!par && bm == 128 && bn == 128 && stages == 3))) ? 2 : 4) : 2;
}
// dynamic LDS of a conv_pipe_kernel instantiation: KG rings, or the split-K tile exchange if larger
constexpr int conv_pipe_lds(int bm, int bn, int stages, int ks, int kg) {
  return kg * stages * (bm + bn) * ks * 2 > (kg > 1 ? kg * bm * (bn + 4) * 4 : 0)
             ? kg * stages * (bm + bn) * ks * 2
             : kg * bm * (bn + 4) * 4;
}

// The wave layout of the in-workgroup split-K reduction (KG > 1): WAVES * KG waves over the BM x BN tile, 4 wave
// rows when that leaves >= 16-row / 16-column sub-tiles.
template <int BM_, int BN_, int NW>
struct KgLayout {
  static constexpr int WM = (NW >= 4 && BM_ / 4 >= 16) ? 4 : (NW >= 2 ? 2 : 1);
  static constexpr int WN = NW / WM;
  static_assert(WM * WN == NW && BM_ % (16 * WM) == 0 && BN_ % (16 * WN) == 0, "split-K epilogue layout");
};

// STAGES-deep LDS ring (cdna_hip_programming.md "Pipelining across barriers"): tiles kt+1 .. kt+STAGES-2 stay
// in flight across the barrier that publishes tile kt (counted vmcnt, raw s_barrier); the barrier also retires
// every wave's reads of tile kt-1, whose buffer the DMA of tile kt+STAGES-1 then reuses.
//
// KG > 1: in-workgroup split-K.  The small-M layers (ResNet18 layer3 / layer4: 12,544 / 4,096 GEMM rows) have one
// 64 x 128 tile per CU, and one 8-wave tile per CU leaves the K loop latency-bound (0.15-0.18 of the MFMA peak).
// KG K-groups of WM x WN waves each own a ring of their own and a contiguous 1/KG of the K-steps, all groups stepping
// through the same barriers; at the end every group stores its fp32 tile to LDS and the WAVES * KG waves re-split the
// tile (KgLayout), each element summed over the groups in group order -- deterministic, no global partials, and the
// fused epilogue (BN statistics / BN-backward sums) runs unchanged on the summed tile.
//
// FAST: the scalar-walk staging (see there), picked by the launcher (`fast` in launch_conv_pipe_t) where the shape
// allows it.
template <bool DGRAD, bool PAR, int BM_, int BN_, int WM = 2, int WN = 2, int STAGES = 2, int KS = 64, bool X2 = true,
          int KG = 1, bool FAST = false>
// (__launch_bounds__'s second argument is amdgpu_waves_per_eu, a minimum of waves per SIMD: two 8-wave blocks per CU need
// 4, i.e. <= 128 VGPRs -- with 2, the parity-class dgrad tile took 131 VGPRs and ran one block per CU)
__global__ __launch_bounds__(64 * WM * WN * KG, conv_pipe_wpe(WM * WN * KG, BM_, BN_, STAGES, DGRAD, PAR,
                                                              conv_pipe_lds(BM_, BN_, STAGES, KS, KG))) void conv_pipe_kernel(ConvGeom g) {
  constexpr int WAVES = WM * WN;  // per K-group
  constexpr int CW = KS / 8, RPG = 64 / CW;  // 16-byte chunks per LDS row, rows per glds instruction
  constexpr int IA = BM_ / RPG / WAVES, IB = BN_ / RPG / WAVES;  // glds per wave per K-tile
  static_assert(IA * RPG * WAVES == BM_ && IB * RPG * WAVES == BN_, "tile rows must split into whole glds pieces");
  static_assert(KS == 64 || KS == 32, "K-tile");
  static_assert(KG == 1 || KG == 2 || KG == 4, "K-groups");
  constexpr int TM = BM_ / WM, TN = BN_ / WN, FM = TM / 16, FN = TN / 16;
  constexpr int BUF = (BM_ + BN_) * KS;
  extern __shared__ __attribute__((aligned(16))) bf16_t smem_all[];
  const int t = threadIdx.x, lane = t & 63, kg = (t >> 6) / WAVES, w = (t >> 6) % WAVES;
  bf16_t* const smem = smem_all + kg * STAGES * BUF;  // this K-group's ring
  ParClass pc{};
  int M, Kr, rowsH, rowsW;  // this launch's GEMM rows / reduction length, row -> (n, a, b) grid
  int Kr0 = 0;              // PAR: the 3x3 taps' share of Kr (the fused downsample segment follows it in class 0)
  if (PAR) {
    pc = par_class(g, par_cls());
    M = g.N * pc.Hc * pc.Wc;
    Kr0 = pc.nr * pc.ns * g.IC;
    Kr = Kr0 + ((g.X2 && pc.ph == 0 && pc.pw == 0) ? g.K2 : 0);
    rowsH = pc.Hc;
    rowsW = pc.Wc;
  } else {
    M = g.N * g.OH * g.OW;
    Kr = g.Kred;
    rowsH = g.OH;
    rowsW = g.OW;
  }
  const int nx = (g.Ncols + BN_ - 1) / BN_, ny = (M + BM_ - 1) / BM_;
  if ((int)blockIdx.x >= nx * ny) return;  // grid sized for the largest parity class
  CTP(0);
  int tx, ty;
  xcd_tile(blockIdx.x, nx, nx * ny, tx, ty);
  const int m0 = ty * BM_, n0 = tx * BN_;
  const int wr = w / WN, wc = w % WN;

  // LDS row of A-operand glds j -> its GEMM row's (n, a, b) and validity; the lane's (swizzled) channel chunk
  auto a_row = [&](int j, int& n, int& oh, int& ow, bool& ok) {
    const int m = m0 + (w * IA + j) * RPG + lane / CW;
    ok = m < M;
    const int mm = ok ? m : 0;
    n = mm / (rowsH * rowsW);
    const int rem = mm - n * rowsH * rowsW;
    oh = rem / rowsW;
    ow = rem - oh * rowsW;
  };
  int acl[IA];
#pragma unroll
  for (int j = 0; j < IA; ++j) acl[j] = cswz_k<CW>((w * IA + j) * RPG + lane / CW, lane % CW) * 8;
  int bcl[IB], bn[IB];
  bool bok[IB];
#pragma unroll
  for (int j = 0; j < IB; ++j) {
    const int r = (w * IB + j) * RPG + lane / CW;
    const int n = n0 + r;
    bok[j] = n < g.Ncols;
    bn[j] = bok[j] ? n : 0;
    bcl[j] = cswz_k<CW>(r, lane % CW) * 8;
  }
  const bf16_t* zero = reinterpret_cast<const bf16_t*>(mer_conv_zero16);

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  // this K-group's K-steps: [kb, kb + nk) of the tile's nk_all; every group runs the loop nkg times (the barriers are
  // workgroup-wide), a group with fewer steps idles through its last ones
  const int nk_all = (Kr + KS - 1) / KS;
  const int nkg = (nk_all + KG - 1) / KG, kb = __builtin_amdgcn_readfirstlane(kg * nkg);  // (kg is wave-uniform)
  const int nk = nk_all - kb < nkg ? (nk_all - kb > 0 ? nk_all - kb : 0) : nkg;
  const int kofs = kb * KS;
  constexpr int G = IA + IB;
  static_assert(STAGES >= 2 && STAGES <= 4, "ring depth");
  // The ring: stage(buf) issues the DMAs of the NEXT K-step (the steps are staged strictly in order, kofs first) into
  // slot buf.  Read and write slots advance as wrapping counters.
  auto k_loop = [&](auto&& stage) {
#pragma unroll
    for (int p = 0; p < STAGES - 1; ++p)
      if (p < nk) stage(p);
    int wslot = STAGES - 1, rslot = 0;
    CTP(1);
    for (int kt = 0; kt < nkg; ++kt) {
      const int left = nk - 1 - kt;
      const int ahead = left < (STAGES - 2) ? left : (STAGES - 2);
      wait_tiles_in_flight<G>(ahead);
      lds_barrier();
      if (kt + STAGES - 1 < nk) stage(wslot);
      wslot = wslot == STAGES - 1 ? 0 : wslot + 1;
      const bf16_t* la = smem + rslot * BUF;
      rslot = rslot == STAGES - 1 ? 0 : rslot + 1;
      if (KG > 1 && kt >= nk) continue;
      const bf16_t* lb = la + BM_ * KS;
#pragma unroll
      for (int s = 0; s < KS / 32; ++s) {
        bf16x8 af[FM], bfr[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int r = wr * TM + i * 16 + fr;
          af[i] = *reinterpret_cast<const bf16x8*>(la + r * KS + cswz_k<CW>(r, s * 4 + fq) * 8);
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int r = wc * TN + j * 16 + fr;
          bfr[j] = *reinterpret_cast<const bf16x8*>(lb + r * KS + cswz_k<CW>(r, s * 4 + fq) * 8);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
    }
  };

  // Fast address path: every channel count is a multiple of the K-step, so a K-step lies inside ONE tap -- the tap, its
  // element offset in the source window and the weight offset are wave-uniform and walk in scalar registers; a lane
  // keeps, per DMA, the pointer of its row's window origin (+ its channel chunk; it may lie outside the tensor and is
  // only ever an operand of a select) and one bit per tap, set where the tap's pixel is inside the frame.  Per K-step
  // and DMA that leaves a bit test, a 64-bit add of a scalar and a select against the zero chunk.  Same sources in the
  // same order as the generic staging below (kept for IC of 8 / 16, K tails, more than 32 taps -- a 7 x 7 forward; its
  // stride-2 input gradient has 16 taps per parity class and walks).
  // Two instantiations, not one kernel with both loops: the accumulators merging from two loops made the 128-VGPR
  // parity-class 128 x 128 tile spill in its epilogue.
  if constexpr (FAST) {
    const bool has_ds = PAR && Kr > Kr0;  // this class carries the fused downsample segment
    constexpr bool NEG = DGRAD || PAR;  // input gradients walk the window backwards
    const int nr = PAR ? pc.nr : g.R, ns = PAR ? pc.ns : g.S;
    const bf16_t* fa[IA];
    unsigned fm[IA];
#pragma unroll
    for (int j = 0; j < IA; ++j) {
      int n, oh, ow;
      bool ok;
      a_row(j, n, oh, ow, ok);
      // window origin: tap (ri, si) reads pixel (h0 + sg * ri, w0 + sg * si)
      const int h0 = PAR ? oh + pc.dh0 : DGRAD ? oh + g.pad : oh * g.st - g.pad;
      const int w0 = PAR ? ow + pc.dw0 : DGRAD ? ow + g.pad : ow * g.st - g.pad;
      unsigned cm = 0, m = 0;
      for (int si = 0; si < ns; ++si) cm |= (unsigned)((unsigned)(NEG ? w0 - si : w0 + si) < (unsigned)g.IW) << si;
      for (int ri = 0; ri < nr; ++ri)
        if ((unsigned)(NEG ? h0 - ri : h0 + ri) < (unsigned)g.IH) m |= cm << (ri * ns);
      fm[j] = ok ? m : 0u;
      fa[j] = g.X + ((((long)n * g.IH + h0) * g.IW + w0) * g.IC + acl[j]);
    }
    const bf16_t* fb[IB];
#pragma unroll
    for (int j = 0; j < IB; ++j) fb[j] = g.Wt + ((long)bn[j] * g.Kred + bcl[j]);
    // the scalar walk: tap (ri, si), channel base c inside it, the tap's A / weight element offsets
    int f_ic = g.IC, f_c, f_tap, f_ri, f_si, f_aoff, f_boff;
    bool f_ds = false;
    auto tap_offsets = [&]() {
      const int ao = (f_ri * g.IW + f_si) * g.IC;
      f_aoff = NEG ? -ao : ao;
      f_boff = PAR ? ((pc.r0 + 2 * f_ri) * g.S + pc.s0 + 2 * f_si) * g.IC : f_tap * g.IC;
    };
    // class 0's downsample segment: one tap, valid wherever the row is; its output pixel (hh, ww) is the input pixel
    auto enter_ds = [&]() {
      f_ds = true;
      f_ic = g.K2;
      f_c = f_tap = f_ri = f_si = f_aoff = f_boff = 0;
#pragma unroll
      for (int j = 0; j < IA; ++j) {
        int n, hh, ww;
        bool ok;
        a_row(j, n, hh, ww, ok);
        fm[j] = ok ? 1u : 0u;
        fa[j] = g.X2 + ((((long)n * g.IH + hh) * g.IW + ww) * g.K2 + acl[j]);
      }
#pragma unroll
      for (int j = 0; j < IB; ++j) fb[j] = g.Wt2 + ((long)bn[j] * g.K2 + bcl[j]);
    };
    if (has_ds && kofs >= Kr0) {
      enter_ds();
      f_c = kofs - Kr0;
    } else {
      f_tap = kofs / g.IC;
      f_c = kofs - f_tap * g.IC;
      f_ri = f_tap / (ns > 0 ? ns : 1);  // (a parity class of a 1 x 1 conv can be empty: no taps, no K-steps)
      f_si = f_tap - f_ri * ns;
      tap_offsets();
    }
    k_loop([&](int buf) {
      bf16_t* la = smem + buf * BUF;
      bf16_t* lb = la + BM_ * KS;
      const unsigned tbit = 1u << (f_tap & 31);
      const long ao = f_aoff + f_c, bo = f_boff + f_c;
#pragma unroll
      for (int j = 0; j < IA; ++j) glds16((fm[j] & tbit) ? fa[j] + ao : zero, la + (w * IA + j) * 512);
#pragma unroll
      for (int j = 0; j < IB; ++j) glds16(bok[j] ? fb[j] + bo : zero, lb + (w * IB + j) * 512);
      f_c += KS;
      if (f_c == f_ic) {  // (wave-uniform) next tap
        f_c = 0;
        ++f_tap;
        if (++f_si == ns) {
          f_si = 0;
          ++f_ri;
        }
        tap_offsets();
        if (has_ds && !f_ds && f_tap == nr * ns) enter_ds();
      }
    });
  } else {
    int an[IA], aoh[IA], aow[IA];
    bool aok[IA];
#pragma unroll
    for (int j = 0; j < IA; ++j) a_row(j, an[j], aoh[j], aow[j], aok[j]);
    const bf16_t* pb[IB];
    const bf16_t* pb2[IB];
#pragma unroll
    for (int j = 0; j < IB; ++j) {
      pb[j] = g.Wt + (long)bn[j] * g.Kred;
      pb2[j] = g.Wt2 + (long)bn[j] * g.K2;  // (unused unless the downsample segment is fused)
    }
    const float inv_IC = 1.f / g.IC, inv_S = 1.f / g.S, inv_ns = PAR ? 1.f / pc.ns : 1.f;
    // class-local reduction index kk -> (ri, si, c) -> source; the weight operand's offset of the same kk
    auto par_a_src = [&](int n, int hh, int ww, bool rowok, int kk) -> const bf16_t* {
      if (!rowok || kk >= Kr) return zero;
      if (kk >= Kr0)  // the fused downsample segment (class 0): its output pixel (hh, ww) is the input pixel (2hh, 2ww)
        return g.X2 + (((long)n * g.IH + hh) * g.IW + ww) * g.K2 + (kk - Kr0);
      const int tap = fdiv(kk, inv_IC), c = kk - tap * g.IC;
      const int ri = fdiv(tap, inv_ns), si = tap - ri * pc.ns;
      const int ih = hh + pc.dh0 - ri, iw = ww + pc.dw0 - si;
      if (ih < 0 || ih >= g.IH || iw < 0 || iw >= g.IW) return zero;
      return g.X + (((long)n * g.IH + ih) * g.IW + iw) * g.IC + c;
    };
    auto par_b_off = [&](int kk) -> int {
      const int tap = fdiv(kk, inv_IC), c = kk - tap * g.IC;
      const int ri = fdiv(tap, inv_ns), si = tap - ri * pc.ns;
      return ((pc.r0 + 2 * ri) * g.S + pc.s0 + 2 * si) * g.IC + c;
    };
    int k0 = kofs;
    k_loop([&](int buf) {
      bf16_t* la = smem + buf * BUF;
      bf16_t* lb = la + BM_ * KS;
#pragma unroll
      for (int j = 0; j < IA; ++j) {
        const bf16_t* src = PAR ? par_a_src(an[j], aoh[j], aow[j], aok[j], k0 + acl[j])
                                : conv_a_src<DGRAD>(g, an[j], aoh[j], aow[j], aok[j], k0 + acl[j], inv_IC, inv_S);
        glds16(src, la + (w * IA + j) * 512);
      }
#pragma unroll
      for (int j = 0; j < IB; ++j) {
        const int kk = k0 + bcl[j];
        const bool ok = bok[j] && kk < Kr;
        const bf16_t* src = !PAR ? pb[j] + kk : (kk >= Kr0 ? pb2[j] + (kk - Kr0) : pb[j] + par_b_off(kk));
        glds16(ok ? src : zero, lb + (w * IB + j) * 512);
      }
      k0 += KS;
    });
  }
  CTP(2);

  // output row -> element offset of the pixel in Y
  auto out_row = [&](int row) -> long {
    if (!PAR) return (long)row;
    const int n = row / (pc.Hc * pc.Wc);
    const int rem = row - n * pc.Hc * pc.Wc;
    const int hh = rem / pc.Wc, ww = rem - hh * pc.Wc;
    return ((long)n * g.OH + 2 * hh + pc.ph) * g.OW + 2 * ww + pc.pw;
  };
  // partial-row index of this tile for the fused reductions: ty, after the row tiles of the preceding parity
  // classes in the PAR (stride-2) form
  auto red_row = [&]() -> long {
    long row_id = ty;
    if (PAR)
      for (int c2 = 0; c2 < par_cls(); ++c2) {
        const ParClass q = par_class(g, c2);
        row_id += (g.N * q.Hc * q.Wc + BM_ - 1) / BM_;
      }
    return row_id;
  };
  // One-pass input-gradient epilogues load their operands (residual, its mask, the BN mask and input(s), BN (mean, rstd))
  // right after the K loop, so the latency hides under the barrier / split-K exchange.  (Loading every pass's operands
  // there for the multi-pass tiles needs 20 VGPRs per pass: the 128 x 128 tiles then spill.)
  constexpr int EWF = STAGES * BUF / 2 / WAVES;  // epilogue staging floats per wave
  const int ct_slot = 10;  // (timing build: stamps inside the epilogue, CT slots 10..12)
  if constexpr (KG > 1) {  // (the launcher takes KG > 1 only with the 16-byte epilogue)
    using L = KgLayout<BM_, BN_, WAVES * KG>;
    constexpr int LDR = BN_ + 4;  // padded fp32 rows: a fragment's 4 row quads fall on distinct bank groups
    constexpr int TM2 = BM_ / L::WM, TN2 = BN_ / L::WN, FM2 = TM2 / 16, FN2 = TN2 / 16;
    using E2 = EpiGeo<FM2, FN2, EWF>;
    const int w2 = t >> 6, wr2 = w2 / L::WN, wc2 = w2 % L::WN;
    constexpr bool PF = DGRAD && E2::NP == 1;
    EpiPre<E2::NP> pre;
    if constexpr (PF)
      conv_epilogue_prefetch<DGRAD, FM2, FN2, L::WM, L::WN, EWF, decltype(out_row), E2::NP, X2>(g, pre, w2, lane, m0,
                                                                                                n0, M, out_row);
    __syncthreads();  // every wave's last fragment reads are done before the exchange reuses the ring
    float* const part = reinterpret_cast<float*>(smem_all);
    {
      float* mine = part + kg * BM_ * LDR;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) mine[(wr * TM + i * 16 + fq * 4 + r) * LDR + wc * TN + j * 16 + fr] = acc[i][j][r];
    }
    lds_barrier();
    f32x4 acc2[FM2][FN2];
#pragma unroll
    for (int i = 0; i < FM2; ++i)
#pragma unroll
      for (int j = 0; j < FN2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = (wr2 * TM2 + i * 16 + fq * 4 + r) * LDR + wc2 * TN2 + j * 16 + fr;
          float s = part[e];
#pragma unroll
          for (int q = 1; q < KG; ++q) s += part[q * BM_ * LDR + e];  // group order: fixed
          acc2[i][j][r] = s;
        }
    lds_barrier();  // every wave holds its sums before the epilogue reuses the LDS
    CTP(3);
    if constexpr (PF)
      conv_epilogue_vec<DGRAD, FM2, FN2, L::WM, L::WN, EWF, decltype(out_row), decltype(pre), false, X2>(
          g, acc2, reinterpret_cast<float*>(smem_all), w2, lane, m0, n0, M, g.bnr_red ? red_row() : 0l, ty, out_row,
          &pre, ct_slot);
    else
      conv_epilogue_vec<DGRAD, FM2, FN2, L::WM, L::WN, EWF, decltype(out_row), EpiNone, false, X2>(
          g, acc2, reinterpret_cast<float*>(smem_all), w2, lane, m0, n0, M, (DGRAD && g.bnr_red) ? red_row() : 0l, ty,
          out_row, static_cast<const EpiNone*>(nullptr), ct_slot);
    CTP(4);
    return;
  }
  if (g.vec) {
    using E1 = EpiGeo<FM, FN, EWF>;
    if constexpr (DGRAD && E1::NP == 1) {
      EpiPre<E1::NP> pre;
      conv_epilogue_prefetch<DGRAD, FM, FN, WM, WN, EWF, decltype(out_row), E1::NP, X2>(g, pre, w, lane, m0, n0, M,
                                                                                         out_row);
      __syncthreads();  // every wave's last fragment reads are done before the epilogue reuses the ring
      CTP(3);
      conv_epilogue_vec<DGRAD, FM, FN, WM, WN, EWF, decltype(out_row), decltype(pre), false, X2>(
          g, acc, reinterpret_cast<float*>(smem), w, lane, m0, n0, M, g.bnr_red ? red_row() : 0l, ty, out_row, &pre,
          ct_slot);
    } else {
      __syncthreads();  // every wave's last fragment reads are done before the epilogue reuses the ring
      CTP(3);
      conv_epilogue_vec<DGRAD, FM, FN, WM, WN, EWF, decltype(out_row), EpiNone, false, X2>(
          g, acc, reinterpret_cast<float*>(smem), w, lane, m0, n0, M, (DGRAD && g.bnr_red) ? red_row() : 0l, ty,
          out_row, static_cast<const EpiNone*>(nullptr), ct_slot);
    }
    CTP(4);
    return;
  } else {
  __syncthreads();
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wr * TM + i * 16 + fq * 4 + r;
      if (row >= M) continue;
      const long orow = out_row(row) * g.ldy;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int col = n0 + wc * TN + j * 16 + fr;
        if (col >= g.Ncols) continue;
        float v = acc[i][j][r];
        if (g.R_) {
          const long ri = orow + col;
          if (!g.Rmask || bf2f(g.Rmask[ri]) > 0.f) v += bf2f(g.R_[ri]);
        }
        const bf16_t h = f2bf(v);
        g.Y[orow + col] = h;
        acc[i][j][r] = bf2f(h);  // the stored value feeds the BN statistics
      }
    }
  if (DGRAD && g.bnr_red) {
    // fused bn_bwd_reduce over this tile's stored gradient: 3 sums per column (g, g*xhat, g*xhat2)
    float ps[FN][3];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int col = n0 + wc * TN + j * 16 + fr;
      const bool cok = col < g.Ncols;
      const float mu = cok ? g.bnr_ms[2 * col] : 0.f, rs = cok ? g.bnr_ms[2 * col + 1] : 0.f;
      const float mu2 = (cok && g.bnr_x2) ? g.bnr_ms2[2 * col] : 0.f;
      const float rs2 = (cok && g.bnr_x2) ? g.bnr_ms2[2 * col + 1] : 0.f;
      float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wr * TM + i * 16 + fq * 4 + r;
          if (row < M && cok) {
            const long e = out_row(row) * g.ldy + col;
            const float gv = bf2f(g.bnr_mask[e]) > 0.f ? acc[i][j][r] : 0.f;
            s1 += gv;
            s2 += gv * (bf2f(g.bnr_x[e]) - mu) * rs;
            if (g.bnr_x2) s3 += gv * (bf2f(g.bnr_x2[e]) - mu2) * rs2;
          }
        }
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
        s3 += __shfl_xor(s3, o, 64);
      }
      ps[j][0] = s1;
      ps[j][1] = s2;
      ps[j][2] = s3;
    }
    // the WM waves sharing a column meet in LDS (staging buffers idle now): red[wr][col][3]
    float* red = reinterpret_cast<float*>(smem);
    __syncthreads();
    if (wr > 0 && fq == 0)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q) red[((wr * WN + wc) * FN * 16 + j * 16 + fr) * 3 + q] = ps[j][q];
    __syncthreads();
    if (wr == 0 && fq == 0) {
      // this block's own partial row (single writer per element -> deterministic after the fixed-order fold):
      // row = ty, after the row tiles of the preceding parity classes in the PAR (stride-2) form
      long row_id = ty;
      if (PAR)
        for (int c2 = 0; c2 < par_cls(); ++c2) {
          const ParClass q = par_class(g, c2);
          row_id += (g.N * q.Hc * q.Wc + BM_ - 1) / BM_;
        }
      const long slab = row_id * g.Ncols * 2;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int col = n0 + wc * TN + j * 16 + fr;
        float t0 = ps[j][0], t1 = ps[j][1], t2 = ps[j][2];
#pragma unroll
        for (int q = 1; q < WM; ++q) {
          const float* o = red + ((q * WN + wc) * FN * 16 + j * 16 + fr) * 3;
          t0 += o[0];
          t1 += o[1];
          t2 += o[2];
        }
        if (col < g.Ncols) {
          g.bnr_red[slab + 2 * col] = t0;
          g.bnr_red[slab + 2 * col + 1] = t1;
          if (g.bnr_red2) {
            g.bnr_red2[slab + 2 * col] = t0;
            g.bnr_red2[slab + 2 * col + 1] = t2;
          }
        }
      }
    }
  }
  }  // !g.vec
  if (g.stats) conv_tile_stats<FM, FN, WM, WN>(g, acc, reinterpret_cast<float*>(smem), w, lane, m0, n0, M, ty);
}

// ---------------------------------------------------------------------------------------
// The tile plan.  Which kernel a forward / input-gradient convolution runs, on which tile and grid, and how many
// partial rows (forward BN statistics, the dgrad's BN-backward sums: one row per row tile) that launch writes are
// resolved ONCE, by conv_plan() below, from the geometry and the requested variant.  The entry points launch from the
// plan and mer_conv_fwd_rows / mer_conv_dgrad_rows report from it: the trunk does not zero its statistics arenas, so
// a row count that disagreed with the launch would fold unwritten rows or drop a tile.
// ---------------------------------------------------------------------------------------
template <int BM_, int BN_, int WM_ = 2, int WN_ = 2, int STAGES_ = 2, int KS_ = 64, int KG_ = 1>
struct Tile {
  static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, STAGES = STAGES_, KS = KS_, KG = KG_;
};

enum ConvFamily { kConvNone, kConvHalo, kConvReg, kConvPipe };  // conv_halo_kernel / conv_kernel / conv_pipe_kernel

struct ConvPlan {
  int err;         // what the launch returns instead of launching (hipSuccess: launch)
  ConvFamily family;
  int halo;        // kConvHalo: halo_kind (1: layer1, 2: the stem)
  int variant;     // the resolved variant (-1 / 6 requests included)
  bool par;        // the stride-2 input gradient's parity-class form (grid_y = 4)
  int BM, BN, WM, WN, STAGES, KS, KG;
  bool x2, fast;   // the X2 / FAST instantiation switches of conv_pipe_kernel (x2: of conv_halo_kernel too)
  size_t lds;      // dynamic LDS bytes of a pipelined launch
  unsigned grid_x, grid_y;
  int rows;        // partial rows the launch writes
};

template <bool DGRAD, bool PAR, class T>
int launch_conv_pipe_t(ConvGeom& g, const ConvPlan& p, hipStream_t st) {
  // the tile this walk of the ladder arrived at is the one the plan sized the grid, the LDS and the rows for
  if (T::BM != p.BM || T::BN != p.BN || T::WM != p.WM || T::WN != p.WN || T::STAGES != p.STAGES || T::KS != p.KS ||
      T::KG != p.KG)
    return (int)hipErrorInvalidConfiguration;
  auto launch = [&](void (*kern)(ConvGeom)) -> int {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)p.lds) != hipSuccess)
      return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(kern, dim3(p.grid_x, p.grid_y), dim3(64 * T::WM * T::WN * T::KG), p.lds, st, g);
    return (int)hipGetLastError();
  };
  if constexpr (DGRAD && !PAR) {
    if (!p.x2)
      return p.fast ? launch(&conv_pipe_kernel<DGRAD, PAR, T::BM, T::BN, T::WM, T::WN, T::STAGES, T::KS, false, T::KG,
                                               true>)
                    : launch(&conv_pipe_kernel<DGRAD, PAR, T::BM, T::BN, T::WM, T::WN, T::STAGES, T::KS, false, T::KG,
                                               false>);
  }
  return p.fast
             ? launch(&conv_pipe_kernel<DGRAD, PAR, T::BM, T::BN, T::WM, T::WN, T::STAGES, T::KS, true, T::KG, true>)
             : launch(&conv_pipe_kernel<DGRAD, PAR, T::BM, T::BN, T::WM, T::WN, T::STAGES, T::KS, true, T::KG, false>);
}

inline int conv_bn(const ConvGeom& g) { return g.Ncols <= 64 ? 64 : 128; }
// below 384 128-row tiles, 64-row tiles (128-row tiles on the deep layers lose 3.5 % of the step); `par`: the four
// parity classes' tiles, a class taken as a quarter of the pixels
inline bool conv_small_m(const ConvGeom& g, bool par) {
  const long M = (long)g.N * g.OH * g.OW / (par ? 4 : 1);
  const int bn = conv_bn(g);
  return ((M + 127) / 128) * ((g.Ncols + bn - 1) / bn) * (par ? 4 : 1) < 384;
}

// The pipelined tile of a variant: calls f(Tile<...>{}) with the tile as a type and returns what f returns.  The one
// copy of the rule: conv_plan() records the tile through it, launch_conv_plan() instantiates the kernel through it.
// variant 1: 4-wave tiles; variant 2 (default): 8-wave tiles -- more waves per CU hide the DMA latency of
// the 2-deep pipeline (tools/bench_conv.py: 1.1-1.3x on every ResNet layer), cf. gemm_bf16.hip
// pick_variant; variant 3: 16-wave 256-row tiles on the large-M layers.
template <bool DGRAD, bool PAR, class F>
int conv_pipe_tile(const ConvGeom& g, int variant, F&& f) {
  const int bn = conv_bn(g);
  const bool small_m = conv_small_m(g, PAR);
  if (variant == 7) {  // in-workgroup split-K (two K-groups) on the 64-row tiles
    if (bn == 64) return PAR ? f(Tile<64, 64, 2, 2, 2, 64, 2>{}) : f(Tile<64, 64, 2, 2, 3, 64, 2>{});
    return PAR ? f(Tile<64, 128, 2, 4, 2, 64, 2>{}) : f(Tile<64, 128, 2, 4, 3, 64, 2>{});
  }
  if (variant == 3 && !small_m) {  // 256-row tiles (8 / 16 waves) for the large-M layers
    // (the 16-wave dgrad tile needs more than 128 VGPRs and would spill to scratch: 8-wave 256 x 64 tiles instead;
    // tools/check_scratch.py keeps every kernel of the library scratch-free)
    if constexpr (DGRAD) {
      return f(Tile<256, 64, 4, 2>{});
    } else {
      if (bn == 64) return f(Tile<256, 64, 4, 2>{});
      return f(Tile<256, 128, 4, 4>{});
    }
  }
  if (variant == 5) {  // 32-wide K-tiles on a 4-deep ring (three K-tiles in flight), 4-wave tiles
    if (bn == 64) return small_m ? f(Tile<64, 64, 2, 2, 4, 32>{}) : f(Tile<128, 64, 2, 2, 4, 32>{});
    return small_m ? f(Tile<64, 128, 2, 2, 4, 32>{}) : f(Tile<128, 128, 2, 4, 4, 32>{});
  }
  if (variant == 4) {  // variant-2 tiles on a 3-deep ring (two K-tiles in flight across each barrier)
    if (bn == 64) return small_m ? f(Tile<64, 64, 2, 2, 3>{}) : f(Tile<128, 64, 4, 2, 3>{});
    return small_m ? f(Tile<64, 128, 2, 4, 3>{}) : f(Tile<128, 128, 2, 4, 3>{});
  }
  if (variant >= 2) {
    // deep layers (small M, one 64-row tile per CU or fewer): a 3-deep ring keeps two K-tiles in flight
    // (tools/bench_conv.py: layer4 3x3 fwd 54.6 -> 44.8 us, dgrad 55.1 -> 47.1 us; the parity-class dgrad
    // and the large-M layers run best on the 2-deep ring at 2 blocks per CU)
    if (bn == 64)
      return small_m ? (PAR ? f(Tile<64, 64, 2, 2>{}) : f(Tile<64, 64, 2, 2, 3>{})) : f(Tile<128, 64, 4, 2>{});
    // (a stride-1 input gradient with a second BN-backward branch -- x2: the block-0 output of layers 2-4 -- used to
    // take the 64 x 128 tile because the 128 x 128 one needed 138 VGPRs; bounded to 128 (conv_pipe_wpe) it runs two
    // blocks per CU without spilling: layer2.1.conv1's dgrad 54.0 -> 39.4 us, profiles/r06/bench_conv_x2.txt)
    return small_m ? (PAR ? f(Tile<64, 128, 2, 4>{}) : f(Tile<64, 128, 2, 4, 3>{})) : f(Tile<128, 128, 2, 4>{});
  }
  if (bn == 64) return small_m ? f(Tile<64, 64>{}) : f(Tile<128, 64>{});
  return small_m ? f(Tile<64, 128>{}) : f(Tile<128, 128>{});
}

// the register-staged kernel (variant 0; input gradients of stride > 2)
template <bool DGRAD>
int launch_conv(ConvGeom& g, const ConvPlan& p, hipStream_t st) {
  auto launch = [&](void (*kern)(ConvGeom)) -> int {
    hipLaunchKernelGGL(kern, dim3(p.grid_x), dim3(256), 0, st, g);
    return (int)hipGetLastError();
  };
  if (p.BN == 64) return p.BM == 64 ? launch(&conv_kernel<DGRAD, 64, 64>) : launch(&conv_kernel<DGRAD, 128, 64>);
  return p.BM == 64 ? launch(&conv_kernel<DGRAD, 64, 128>) : launch(&conv_kernel<DGRAD, 128, 128>);
}

// ---------------------------------------------------------------------------------------
// Stride-1 convolutions of 64 output channels with the whole weight resident in LDS: ResNet18 layer1 (3x3, pad 1,
// 64 -> 64 channels on 28x28 maps at 112^2 frames; forward and input gradient) and the stem in its space-to-depth form
// (4x4, pad 0, 16 -> 64 channels: 59x59 -> 56x56).  conv_pipe_kernel re-fetches every input pixel from L2 once per
// tap and waits one DMA round trip per 64-deep K-step with ~8 MFMAs per wave behind it: latency-bound, layer1 ran at
// 200-380 TF/s and the stem at ~195.  Here persistent workgroups keep the packed weight [64][R*S*C] resident in LDS
// (layer1 73.7 KB, stem 32 KB) and stage, per 128-pixel output tile, the HALO its taps read -- the input rows the
// tile's output rows need, (W + R - 1) pixels wide with zero border columns -- double-buffered, so tile i+1's halo
// streams in while tile i computes.  The K loop is LDS -> MFMA only: no global load, no barrier.  The A fragment of
// tap (r, s) for output pixel (n, y, x) is halo pixel (n*IH + y + r - pad - base, x + s), the same 16 bytes
// conv_pipe_kernel gathers; K-steps run in the same (tap, channel) order on the same MFMA with the same wave layout
// and epilogue (conv_epilogue_vec), so outputs and BN statistics are bit-identical to conv_pipe_kernel's
// (tests/test_resnet_gpu.py).  Both LDS images are XOR-swizzled per 16-byte chunk so a fragment's 16 rows fall on 16
// distinct bank slots.
// ---------------------------------------------------------------------------------------
namespace halo {
constexpr int BM = 128;  // output pixels per tile
// C input channels, R x R taps, pad, W output width, IHX = IH - OH (input rows beyond the output rows: the stem's 3),
// ROWS halo rows: the image rows 128 consecutive output pixels span + R - 1, + IHX when a tile may straddle frames
template <int C_, int R_, int PAD_, int W_, int IHX_>
struct Geo {
  static constexpr int C = C_, R = R_, PAD = PAD_, W = W_, IHX = IHX_;
  static constexpr int KRED = R * R * C, WCH = KRED / 8;    // reduction, 16-byte chunks per weight row
  static constexpr int CPP = C / 8;                         // chunks per halo pixel
  static constexpr int HW = W + R - 1;                      // halo row width (pixels)
  static constexpr int ROWS = (W + BM - 2) / W + 1 + (R - 1) + IHX;
  static constexpr int CH = (ROWS * HW * CPP + 63) / 64 * 64;  // 16-byte chunks per halo buffer (whole glds pieces)
  static constexpr int ELEMS = CH * 8;                         // bf16 elements per halo buffer
  static constexpr int LDS_ELEMS = 64 * KRED + 2 * ELEMS + C;  // weights, two halo buffers, one zero pixel
  static constexpr int KSTEPS = KRED / 32;
  static constexpr int HSHIFT = CPP == 8 ? 1 : 3;  // halo swizzle: chunk c of pixel p at c ^ ((p >> HSHIFT) & (CPP-1))
  static_assert(CPP == 8 || CPP == 2, "halo layouts for 16 or 64 channels");
  static_assert(WCH % 16 == 0 || WCH % 16 == 8, "weight-row swizzle");
};
// physical chunk of logical weight chunk c in row n (16 consecutive rows at one c cover all 16 bank slots)
template <int WCH>
__device__ __forceinline__ int wchunk(int n, int c) {
  return WCH % 16 == 0 ? ((c & ~15) | ((c & 15) ^ (n & 15))) : ((c & ~7) | ((c & 7) ^ ((n >> 1) & 7)));
}
}  // namespace halo

// X2: the dgrad's second fused BN (bnr_x2) may be present (false: its sums and registers are compiled out)
template <bool DGRAD, class GE, int WM, int WN, int OCC, bool X2 = true>
__global__ __launch_bounds__(64 * WM * WN, OCC) void conv_halo_kernel(ConvGeom g) {
  constexpr int WAVES = WM * WN;
  constexpr int TM = halo::BM / WM, TN = 64 / WN, FM = TM / 16, FN = TN / 16;
  constexpr int HW = GE::HW, CPP = GE::CPP, C = GE::C, R = GE::R, PAD = GE::PAD, W_ = GE::W;
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  bf16_t* const wlds = smem;
  bf16_t* const hbuf = smem + 64 * GE::KRED;
  bf16_t* const zpix = hbuf + 2 * GE::ELEMS;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w / WN, wc = w % WN, fr = lane & 15, fq = lane >> 4;
  const int OH = g.OH, IH = g.IH, IW = g.IW, M = g.N * g.OH * W_, in_rows = g.N * g.IH;
  const int ntiles = (M + halo::BM - 1) / halo::BM;
  const bf16_t* zero = reinterpret_cast<const bf16_t*>(mer_conv_zero16);
  int tile = blockIdx.x;
  CT(0);
  // global input row of output row (frame n, row y) at tap row 0: n * IH + y - pad
  auto in_row0 = [&](int m) {
    const int go = m / W_, n = go / OH;
    return n * IH + (go - n * OH) - PAD;
  };
  // halo of tile `tl`: global input rows base .. base + ROWS - 1 (base = in_row0 of the tile's first pixel), input
  // columns -pad .. W + R - 2 - pad; chunk L of the buffer holds halo pixel L / CPP, logical channel chunk
  // (L % CPP) ^ ((pixel >> HSHIFT) & (CPP - 1))
  auto stage_halo = [&](bf16_t* hb, int tl) {
    const int base = in_row0(tl * halo::BM);
    for (int j = w; j < GE::CH / 64; j += WAVES) {
      const int L = j * 64 + lane;
      const int hp = L / CPP, c = (L % CPP) ^ ((hp >> GE::HSHIFT) & (CPP - 1));
      const int hr = hp / HW, x = hp - hr * HW - PAD, gr = base + hr;
      const bool ok = hr < GE::ROWS && gr >= 0 && gr < in_rows && x >= 0 && x < IW;
      glds16(ok ? g.X + ((long)gr * IW + x) * C + c * 8 : zero, hb + j * 512);
    }
  };
  // resident weights: row n (output column) x WCH chunks, swizzled by halo::wchunk
  for (int j = w; j < GE::WCH; j += WAVES) {  // 64 rows x WCH chunks = WCH glds pieces of 64 chunks
    const int L = j * 64 + lane;
    const int n = L / GE::WCH, pc = L - n * GE::WCH;
    glds16(g.Wt + (long)n * GE::KRED + halo::wchunk<GE::WCH>(n, pc) * 8, wlds + j * 512);  // (an involution)
  }
  stage_halo(hbuf, tile);
  if (t < CPP) *reinterpret_cast<u32x4*>(zpix + t * 8) = u32x4{0u, 0u, 0u, 0u};
  wait_vmcnt<0>();
  __syncthreads();
  CT(1);

  // Per tile: issue the next tile's halo DMA, run the K loop on this one, wait for that DMA (and the previous tile's
  // epilogue stores -- both had the whole K loop to land), then the epilogue (staged through this tile's halo buffer,
  // now free).  No vmcnt wait follows the epilogue: its stores drain under the next K loop.  The fused column
  // reductions (forward BN statistics, the dgrad's BN-backward sums) accumulate per lane over the workgroup's tiles --
  // all of them cover the same 64 output columns -- and are reduced and stored once, as partial row blockIdx.x, after
  // the loop (round 6: one cross-lane / cross-wave reduction per workgroup instead of per tile, and grid-size partial
  // rows instead of one per tile for the folds).
  EpiAcc<FN> eacc;
  eacc.zero();
  for (int cur = 0, it = 0; tile < ntiles; tile += gridDim.x, cur ^= 1, ++it) {
    bf16_t* const hb = hbuf + cur * GE::ELEMS;
    if (tile + (int)gridDim.x < ntiles) stage_halo(hbuf + (cur ^ 1) * GE::ELEMS, tile + gridDim.x);
    CT(it < 11 ? 2 + 5 * it : 63);
    const int m0 = tile * halo::BM, base = in_row0(m0);
    const auto out_row = [](int row) { return (long)row; };
    constexpr int EWF = GE::ELEMS / 2 / WAVES;  // epilogue staging floats per wave (this tile's halo buffer)
    EpiPre<EpiGeo<FM, FN, EWF>::NP> pre;
    if constexpr (DGRAD)
      conv_epilogue_prefetch<DGRAD, FM, FN, WM, WN, EWF, decltype(out_row), EpiGeo<FM, FN, EWF>::NP, X2>(
          g, pre, w, lane, m0, 0, M, out_row);
    int hpb[FM], yv[FM];  // per fragment row of this lane: halo pixel of tap (0, 0), input row of tap row 0
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      int m = m0 + wr * TM + i * 16 + fr;
      m = m < M ? m : M - 1;  // rows past M compute garbage that the epilogue discards
      const int go = m / W_, x = m - go * W_, n = go / OH, y = go - n * OH;
      yv[i] = y - PAD;
      hpb[i] = (n * IH + y - PAD - base) * HW + x;
    }
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // k-steps of 32 in the packed (tap, channel) order: the fragments of step u + 1 are read while step u's MFMAs run
    // (two register sets, static indices: the loop is fully unrolled)
    bf16x8 af[2][FM], bfr[2][FN];
    auto frags = [&](int u, bf16x8 (&a)[FM], bf16x8 (&b)[FN]) {
      const int kk = u * 32 + fq * 8;       // this lane's 8 reduction indices start here
      const int tap = kk / C, c = (kk % C) / 8;
      const int r = tap / R, s = tap - R * (tap / R);
      // dgrad: tap (r, s) of the packed transposed weight reads dy at (h + pad - r, w + pad - s): the halo row / col
      // of output (y, x) then sits at offset (R - 1 - r, R - 1 - s) from (y - pad, x - pad) when pad = (R - 1) / 2
      const int hr = DGRAD ? R - 1 - r : r, hs = DGRAD ? R - 1 - s : s;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int hp = hpb[i] + hr * HW + hs;
        const bool ok = (unsigned)(yv[i] + hr) < (unsigned)IH;  // rows outside the frame read the zero pixel
        a[i] = *reinterpret_cast<const bf16x8*>(
            ok ? hb + hp * C + ((c ^ ((hp >> GE::HSHIFT) & (CPP - 1))) << 3) : zpix);
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int n = wc * TN + j * 16 + fr, cb = u * 4 + fq;
        b[j] = *reinterpret_cast<const bf16x8*>(wlds + n * GE::KRED + (halo::wchunk<GE::WCH>(n, cb) << 3));
      }
    };
    frags(0, af[0], bfr[0]);
#pragma unroll
    for (int u = 0; u < GE::KSTEPS; ++u) {
      if (u + 1 < GE::KSTEPS) frags(u + 1, af[(u + 1) & 1], bfr[(u + 1) & 1]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u & 1][i], bfr[u & 1][j], acc[i][j], 0, 0, 0);
    }
    CT(it < 11 ? 3 + 5 * it : 63);
    wait_vmcnt<0>();  // this wave's share of the next halo (and the previous epilogue's stores) has landed
    lds_barrier();    // every wave's: the next halo is complete and no wave still reads hb
    CT(it < 11 ? 4 + 5 * it : 63);
    const int ct_slot = it == 1 ? 60 : -1;  // (timing build: stamps inside the second tile's epilogue)
    if constexpr (DGRAD)
      conv_epilogue_vec<DGRAD, FM, FN, WM, WN, EWF, decltype(out_row), decltype(pre), true, X2, EpiAcc<FN>>(
          g, acc, reinterpret_cast<float*>(hb), w, lane, m0, 0, M, (long)tile, (long)tile, out_row, &pre, ct_slot,
          &eacc);
    else
      conv_epilogue_vec<DGRAD, FM, FN, WM, WN, EWF, decltype(out_row), EpiNone, true, true, EpiAcc<FN>>(
          g, acc, reinterpret_cast<float*>(hb), w, lane, m0, 0, M, (long)tile, (long)tile, out_row,
          static_cast<const EpiNone*>(nullptr), ct_slot, &eacc);
    CT(it < 11 ? 5 + 5 * it : 63);
    lds_barrier();    // every wave is past its epilogue's use of hb before the DMA two tiles on refills it
    CT(it < 11 ? 6 + 5 * it : 63);
  }
  // (no DMA is in flight after the last tile: the halo buffers are free)
  conv_epilogue_acc_finish<DGRAD, FM, FN, WM, WN, GE::ELEMS / 2 / WAVES, X2>(g, eacc, reinterpret_cast<float*>(hbuf), w,
                                                                          lane, 0, (long)blockIdx.x);
}

using HaloL1 = halo::Geo<64, 3, 1, 28, 0>;    // layer1: 3x3 / pad 1, 64 -> 64, 28x28
using HaloStem = halo::Geo<16, 4, 0, 56, 3>;  // the stem's space-to-depth form: 4x4 / pad 0, 16 -> 64, 59x59 -> 56x56

// which halo kernel applies (0: none): 3x3 / stride 1 / pad 1, 64 -> 64 channels on 28-wide maps (fwd and dgrad), or
// 4x4 / stride 1 / pad 0, 16 -> 64 channels, 59 -> 56 (fwd); 64 output columns, 16-byte epilogue, no fused downsample
int halo_kind(const ConvGeom& g, bool dgrad) {
  if (g.st != 1 || g.Ncols != 64 || g.ldy != 64 || !g.vec || g.X2 != nullptr ||
      ((((uintptr_t)g.X) | ((uintptr_t)g.Wt)) & 15) != 0)
    return 0;
  if (g.R == 3 && g.S == 3 && g.pad == 1 && g.IC == 64 && g.IW == 28 && g.OW == 28 && g.IH == g.OH && g.Kred == 576)
    return 1;
  if (!dgrad && g.R == 4 && g.S == 4 && g.pad == 0 && g.IC == 16 && g.IW == 59 && g.OW == 56 && g.IH == 59 &&
      g.OH == 56 && g.Kred == 256)
    return 2;
  return 0;
}

template <bool DGRAD, class GE, int OCC, bool X2 = true>
int launch_halo_t(ConvGeom& g, const ConvPlan& p, hipStream_t st) {
  constexpr int WM = 4, WN = 2;  // 8 waves, 32 x 32 each: conv_pipe_kernel's 128 x 64 tile (variant 2)
  const size_t lds = GE::LDS_ELEMS * sizeof(bf16_t);
  static_assert(GE::LDS_ELEMS * 2 * OCC <= 160 * 1024, "LDS per CU");
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_halo_kernel<DGRAD, GE, WM, WN, OCC, X2>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL((conv_halo_kernel<DGRAD, GE, WM, WN, OCC, X2>), dim3(p.grid_x), dim3(64 * WM * WN), lds, st, g);
  return (int)hipGetLastError();
}

constexpr int halo_occ(int kind) { return kind == 1 ? 1 : 2; }  // workgroups per CU (the stem: 71 KB of LDS each)

template <bool DGRAD>
int launch_conv_halo(ConvGeom& g, const ConvPlan& p, hipStream_t st) {
  // (the dgrad without a second fused BN -- every layer1 dgrad of the train step -- drops its registers: the
  // per-workgroup accumulators otherwise spill)
  if constexpr (DGRAD)
    if (p.halo == 1 && !p.x2) return launch_halo_t<DGRAD, HaloL1, halo_occ(1), false>(g, p, st);
  if (p.halo == 1) return launch_halo_t<DGRAD, HaloL1, halo_occ(1)>(g, p, st);
  if constexpr (!DGRAD) return launch_halo_t<false, HaloStem, halo_occ(2)>(g, p, st);
  return (int)hipErrorInvalidValue;
}

// Default tile for a non-parity-class conv (forward, or stride-1 input gradient): the in-workgroup split-K form (7: 64-row
// tiles, two K-groups) when one such tile per CU covers the output (ResNet18 layer4: 256 tiles) and each K-group gets
// >= 4 K-steps; otherwise the one-group tiles (`fallback`).  Serialized trunk at B = 32 (profiles/r06/trunk_table_serial
// .txt vs r05): layer4 3x3 fwd 44 -> 36.5 us, dgrad 50-53 -> 41-46.5; layer4.0 stride-2 fwd 24.2 -> 22.1.  Measured and
// dropped: 128-row tiles with two K-groups for layer3 (196 tiles) won standalone with warm operands (34.1 -> 28.2 us)
// but not in the trunk (33.4 -> 34.0, dgrad 39 -> 42) nor in a same-box step A/B (205.17 vs 205.35 steps/s, 4 pairs);
// 64 x 64 per-wave sub-tiles with four / two K-groups lost on every layer (profiles/r06/bench_conv_v10_v11_lost.txt).
int conv_default_variant(const ConvGeom& g, int fallback) {
  if (!g.vec || g.Kred < 8 * CBK) return fallback;
  const long M = (long)g.N * g.OH * g.OW;
  const long nt = (g.Ncols + (g.Ncols <= 64 ? 63 : 127)) / (g.Ncols <= 64 ? 64 : 128);
  if (((M + 63) / 64) * nt <= cu_count()) return 7;
  return fallback;
}

template <class F>
int conv_pipe_tile_of(const ConvGeom& g, bool dgrad, bool par, int variant, F&& f) {
  if (!dgrad) return conv_pipe_tile<false, false>(g, variant, f);
  return par ? conv_pipe_tile<true, true>(g, variant, f) : conv_pipe_tile<true, false>(g, variant, f);
}

// `variant`: as the entry points take it (-1: the default; 6: the halo kernel or an error).  Default: the halo kernel
// where it applies (layer1, the stem), else the pipelined tiles -- 64-channel input gradients (layer1, the layer2.0
// input gradients) on 32-wide K-tiles on a 4-deep ring with 4-wave tiles (5; tools/bench_conv.py --fused: layer1
// 101 -> 65 us, layer2.0 s2 74 -> 51, downsample 48 -> 31), everything else on the 8-wave 64-wide 2-deep ring (2; the
// deep ring loses 10-50% there), either replaced by conv_default_variant's choice outside the parity-class form.
ConvPlan conv_plan(const ConvGeom& g, bool dgrad, int variant) {
  ConvPlan p{};
  const long M = (long)g.N * g.OH * g.OW;
  const long nx = (g.Ncols + conv_bn(g) - 1) / conv_bn(g);
  p.grid_y = 1;
  p.x2 = true;
  if (variant == -1 || variant == 6) {
    if (const int hk = halo_kind(g, dgrad)) {  // persistent workgroups, one partial row each
      const long ntiles = (M + halo::BM - 1) / halo::BM, slots = (long)halo_occ(hk) * cu_count();
      p.family = kConvHalo;
      p.halo = hk;
      p.variant = 6;
      p.BM = halo::BM; p.BN = 64; p.WM = 4; p.WN = 2;
      p.x2 = !(dgrad && hk == 1 && !g.bnr_x2);
      p.grid_x = (unsigned)(ntiles < slots ? ntiles : slots);
      p.rows = (int)p.grid_x;
      return p;
    }
    if (variant == 6) {
      p.err = (int)hipErrorInvalidValue;
      return p;
    }
    variant = dgrad ? (g.Ncols <= 64 ? 5 : 2) : 2;
    if (!dgrad || g.st == 1) variant = conv_default_variant(g, variant);
  }
  p.variant = variant;
  if (variant == 0 || (dgrad && g.st > 2)) {
    p.family = kConvReg;
    p.BM = conv_small_m(g, false) ? 64 : 128;  // deep layers (layer3/4): halve BM so the grid fills 256 CUs
    p.BN = conv_bn(g);
    p.WM = p.WN = 2;
    p.rows = (int)((M + p.BM - 1) / p.BM);
    p.grid_x = (unsigned)(nx * p.rows);
    return p;
  }
  p.family = kConvPipe;
  p.par = dgrad && g.st == 2;
  conv_pipe_tile_of(g, dgrad, p.par, variant, [&](auto t) {
    using T = decltype(t);
    p.BM = T::BM; p.BN = T::BN; p.WM = T::WM; p.WN = T::WN; p.STAGES = T::STAGES; p.KS = T::KS; p.KG = T::KG;
    return 0;
  });
  if (p.KG > 1 && !g.vec) p.err = (int)hipErrorInvalidValue;  // the split-K form has the 16-byte epilogue only
  const size_t ring = (size_t)p.KG * p.STAGES * (p.BM + p.BN) * p.KS * sizeof(bf16_t);
  const size_t kgred = p.KG > 1 ? (size_t)p.KG * p.BM * (p.BN + 4) * sizeof(float) : 0;  // the split-K tile exchange
  p.lds = ring > kgred ? ring : kgred;
  // a stride-1 input gradient whose BN-backward target has no second (downsample) branch runs the instantiation
  // without the x2 terms: 24 fewer VGPRs, which keeps the 8-wave tiles at 2 blocks per CU
  p.x2 = !(dgrad && !p.par && !g.bnr_x2);
  // every reduction segment a whole number of K-steps long and at most 32 taps (one validity bit each; PAR: the
  // taps of the largest parity class): the scalar-walk staging (FAST)
  p.fast = p.par ? (g.IC % p.KS == 0 && (!g.X2 || g.K2 % p.KS == 0) && ((g.R + 1) / 2) * ((g.S + 1) / 2) <= 32)
                 : (g.IC % p.KS == 0 && g.R * g.S <= 32 && (!dgrad || g.st == 1));
  const long nbn = (g.Ncols + p.BN - 1) / p.BN;
  if (!p.par) {
    p.rows = (int)((M + p.BM - 1) / p.BM);
    p.grid_x = (unsigned)(p.rows * nbn);
    return p;
  }
  // PAR: grid.x covers the largest parity class (ph = pw = 0), grid.y = the 4 classes; a class's row tiles store their
  // rows back to back (red_row)
  p.grid_y = 4;
  for (int cls = 0; cls < 4; ++cls) {
    const int ph = cls >> 1, pw = cls & 1;
    const long Mc = (long)g.N * ((g.OH - ph + 1) >> 1) * ((g.OW - pw + 1) >> 1);
    p.rows += (int)((Mc + p.BM - 1) / p.BM);
    if (cls == 0) p.grid_x = (unsigned)((Mc + p.BM - 1) / p.BM * nbn);
  }
  return p;
}

template <bool DGRAD>
int launch_conv_plan(ConvGeom& g, const ConvPlan& p, hipStream_t st) {
  if (p.err != (int)hipSuccess) return p.err;
  if (p.family == kConvHalo) return launch_conv_halo<DGRAD>(g, p, st);
  if (p.family == kConvReg) return launch_conv<DGRAD>(g, p, st);
  if constexpr (DGRAD)
    if (p.par)
      return conv_pipe_tile<true, true>(g, p.variant,
                                        [&](auto t) { return launch_conv_pipe_t<true, true, decltype(t)>(g, p, st); });
  return conv_pipe_tile<DGRAD, false>(g, p.variant,
                                      [&](auto t) { return launch_conv_pipe_t<DGRAD, false, decltype(t)>(g, p, st); });
}

// What mer_conv_fwd_rows / mer_conv_dgrad_rows report: the plan's count where the launch is the library's own choice
// (the halo kernel, the default pipelined tile); for any other request an upper bound -- rows past the tiles stay as
// the caller left them (zeroed) -- of one row per 64 GEMM rows plus the parity classes' tails (MER_BN_RED_ROWS(M) - 64)
int conv_plan_rows(const ConvGeom& g, bool dgrad, int variant) {
  const ConvPlan p = conv_plan(g, dgrad, variant);
  if (p.family == kConvHalo || (variant == -1 && p.family == kConvPipe)) return p.rows;
  return (int)(((long)g.N * g.OH * g.OW + 63) / 64 + (dgrad ? 4 : 0));
}

ConvGeom fwd_geom(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* x,
                  const void* w_packed, void* y, float* stats) {
  ConvGeom g{};
  g.N = N; g.IH = H; g.IW = W; g.IC = C;
  g.OH = (H + 2 * pad - R) / stride + 1; g.OW = (W + 2 * pad - S) / stride + 1;
  g.R = R; g.S = S; g.st = stride; g.pad = pad;
  g.Ncols = K; g.Kred = R * S * C;
  g.X = (const bf16_t*)x; g.Wt = (const bf16_t*)w_packed; g.Y = (bf16_t*)y; g.ldy = K; g.stats = stats;
  g.vec = conv_vec_ok(g);
  return g;
}

ConvGeom dgrad_geom(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* dy,
                    const void* wt_packed, const void* ds_dy) {
  ConvGeom g{};
  g.N = N; g.OH = H; g.OW = W;
  g.IH = (H + 2 * pad - R) / stride + 1; g.IW = (W + 2 * pad - S) / stride + 1; g.IC = K;
  g.R = R; g.S = S; g.st = stride; g.pad = pad;
  g.Ncols = C; g.Kred = R * S * K;
  g.X = (const bf16_t*)dy; g.Wt = (const bf16_t*)wt_packed; g.ldy = C; g.stats = nullptr;
  g.X2 = (const bf16_t*)ds_dy;
  g.vec = conv_vec_ok(g);
  return g;
}

}  // namespace

MER_API int mer_conv_fwd(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* x,
                         const void* w_packed, void* y, float* stats, void* stream) {
  return mer_conv_fwd_ex(N, H, W, C, K, R, S, stride, pad, x, w_packed, y, stats, -1, stream);
}

MER_API int mer_conv_fwd_rows(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* x,
                              const void* w_packed, int variant) {
  if (N <= 0 || C % 8 || variant < -1 || variant > 7) return -(int)hipErrorInvalidValue;
  return conv_plan_rows(fwd_geom(N, H, W, C, K, R, S, stride, pad, x, w_packed, nullptr, nullptr), false, variant);
}

MER_API int mer_conv_dgrad_rows(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* dy,
                                const void* wt_packed, const void* ds_dy, int variant) {
  if (N <= 0 || K % 8 || C % 8 || variant < -1 || variant > 7) return -(int)hipErrorInvalidValue;
  return conv_plan_rows(dgrad_geom(N, H, W, C, K, R, S, stride, pad, dy, wt_packed, ds_dy), true, variant);
}

MER_API int mer_conv_fwd_ex(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* x,
                            const void* w_packed, void* y, float* stats, int variant, void* stream) {
  if (C % 8 || variant < -1 || variant > 7) return (int)hipErrorInvalidValue;
  ConvGeom g = fwd_geom(N, H, W, C, K, R, S, stride, pad, x, w_packed, y, stats);
  return launch_conv_plan<false>(g, conv_plan(g, false, variant), (hipStream_t)stream);
}

MER_API int mer_conv_dgrad(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* dy,
                           const void* wt_packed, void* dx, const void* residual, const void* residual_mask,
                           void* stream) {
  return mer_conv_dgrad_ex(N, H, W, C, K, R, S, stride, pad, dy, wt_packed, dx, residual, residual_mask, -1, stream);
}

MER_API int mer_conv_dgrad_ex(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* dy,
                              const void* wt_packed, void* dx, const void* residual, const void* residual_mask,
                              int variant, void* stream) {
  return mer_conv_dgrad_bnr(N, H, W, C, K, R, S, stride, pad, dy, wt_packed, dx, residual, residual_mask, nullptr,
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, variant, stream);
}

MER_API int mer_conv_dgrad_bnr(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* dy,
                               const void* wt_packed, void* dx, const void* residual, const void* residual_mask,
                               const void* bn_mask, const void* bn_x, const float* bn_ms, float* bn_red,
                               const void* bn_x2, const float* bn_ms2, float* bn_red2, int variant, void* stream) {
  return mer_conv_dgrad_ds(N, H, W, C, K, R, S, stride, pad, dy, wt_packed, dx, residual, residual_mask, bn_mask, bn_x,
                           bn_ms, bn_red, bn_x2, bn_ms2, bn_red2, nullptr, nullptr, 0, variant, stream);
}

MER_API int mer_conv_dgrad_ds(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* dy,
                              const void* wt_packed, void* dx, const void* residual, const void* residual_mask,
                              const void* bn_mask, const void* bn_x, const float* bn_ms, float* bn_red,
                              const void* bn_x2, const float* bn_ms2, float* bn_red2, const void* ds_dy,
                              const void* ds_wt_packed, int ds_K, int variant, void* stream) {
  if (K % 8 || C % 8 || variant < -1 || variant > 7) return (int)hipErrorInvalidValue;
  // the fused downsample: a 1x1 / stride-2 / pad-0 conv of the same input with ds_K output channels, beside a
  // 3x3 / stride-2 / pad-1 conv (its taps land in parity class (0, 0) only, at pixel (2i, 2j)); K-tile aligned.
  // Only the pipelined kernels read the second K segment: not the register-staged variant 0 (the default never
  // resolves to it; the halo test refuses a second segment itself).
  if (ds_dy && (stride != 2 || R != 3 || S != 3 || pad != 1 || !ds_wt_packed || ds_K <= 0 || ds_K % 64 || K % 64 ||
                variant == 0))
    return (int)hipErrorInvalidValue;
  if (bn_red && (!bn_mask || !bn_x || !bn_ms || (bn_x2 && (!bn_ms2 || !bn_red2)))) return (int)hipErrorInvalidValue;
  if (bn_red && (variant == 0 || stride > 2)) return (int)hipErrorInvalidValue;  // fused only in the pipelined kernel
  ConvGeom g = dgrad_geom(N, H, W, C, K, R, S, stride, pad, dy, wt_packed, ds_dy);
  g.Y = (bf16_t*)dx;
  g.R_ = (const bf16_t*)residual; g.Rmask = (const bf16_t*)residual_mask;
  g.bnr_mask = (const bf16_t*)bn_mask; g.bnr_x = (const bf16_t*)bn_x; g.bnr_ms = bn_ms; g.bnr_red = bn_red;
  g.bnr_x2 = (const bf16_t*)bn_x2; g.bnr_ms2 = bn_ms2; g.bnr_red2 = bn_red2;
  g.Wt2 = (const bf16_t*)ds_wt_packed; g.K2 = ds_dy ? ds_K : 0;
  // dgrad_geom judged the 16-byte epilogue before dx and the epilogue operands were known (mer_conv_dgrad_rows has
  // none of them): judge it again with them, so a misaligned dx / residual / mask / BN operand / red buffer takes the
  // scalar epilogue, and the halo and split-K forms, which have the 16-byte one only, refuse it
  g.vec = conv_vec_ok(g);
  return launch_conv_plan<true>(g, conv_plan(g, true, variant), (hipStream_t)stream);
}
