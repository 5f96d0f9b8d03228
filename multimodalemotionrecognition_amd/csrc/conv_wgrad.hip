// Weight gradients of the ResNet18 trunk's convolutions (and of the Linear layers, as 1x1 convolutions); see conv.hip
// for the layouts.
#include "conv_common.h"
#include "mer.h"

// timing build (tools/pipe_phases.py wgrad): this unit's own stamp buffer, slots as in conv_pipe_kernel
MER_CT_BUFFER(mer_wct, 4096 * 8)
#define CTP(k) CTP_AT(mer_wct_buf, k)
// Diagnostic forms of the weight-gradient K loops (tools/pipe_phases.py wgrad --bound; results WRONG): 1 = no LDS-DMA
// issue after the prologue (what the loop costs without operand fill), 2 = the fragment reads of the first K-step
// only (what it costs without LDS reads).  The production library compiles CT_MODE() to the constant 0.
MER_CT_MODE_WORD(mer_wct_mode)
#ifdef MER_CONV_TIMING
#define CT_MODE() mer_wct_mode_v
#else
#define CT_MODE() 0
#endif

namespace {

// ---------------------------------------------------------------------------------------
// wgrad: dW[k][(r,s,c)] += sum_p dY[p][k] X(p; r,s,c).  Split-K over pixels (grid z): each split
// stores a coalesced fp32 slab, wgrad_reduce sums them into the PyTorch-layout gradient [Cout][Cin][R][S]
// (scattered fp32 atomics at stride R*S ran ~17x under the atomic peak: MI355X_MICROARCH 'Global float atomics').
// LDS images [pixel][channel] (+16 pad); MFMA fragments via ds_read_b64_tr_b16.
// ---------------------------------------------------------------------------------------
struct WgradGeom {
  int N, H, W, C;         // X (input activation, NHWC, C padded)
  int Ho, Wo, K;          // dY
  int R, S, st, pad;
  int Creal;              // real input channels (<= C) of the weight
  const bf16_t* X;
  const bf16_t* dY;
  float* ws;              // [splits][K][R*S*C] fp32 partial slabs
  int pix_per_split;
  long ldy;               // dY row stride (elements; K for a conv, a column slice of a wider matrix for a Linear)
  int flat;               // wgrad_pipe_kernel: 1-D grid of splits x tiles, a split's tiles on one XCD (see there)
};

template <int BM_, int BN_, int WM = 2, int WN = 2, int PF = 1>
__global__ __launch_bounds__(64 * WM * WN, 2) void wgrad_kernel(WgradGeom g) {
  constexpr int NT = 64 * WM * WN;
  constexpr int LDM = BM_ + 16, LDN = BN_ + 16;
  constexpr int IT = BM_ / WM / 16, JT = BN_ / WN / 16;
  constexpr int ACH = BM_ * 64 / 8 / NT, BCH = BN_ * 64 / 8 / NT;  // 16B chunks per thread
  static_assert(ACH * NT * 8 == BM_ * 64 && BCH * NT * 8 == BN_ * 64, "staging split");
  __shared__ __attribute__((aligned(16))) bf16_t lds[2][64 * LDM + 64 * LDN];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int Ntot = g.R * g.S * g.C;
  const int P = g.N * g.Ho * g.Wo;
  const int wnx = (Ntot + BN_ - 1) / BN_, wny = (g.K + BM_ - 1) / BM_;
  int wtx, wty;
  xcd_tile(blockIdx.x, wnx, wnx * wny, wtx, wty);
  const int m0 = wty * BM_, n0 = wtx * BN_;
  const int p_beg = blockIdx.z * g.pix_per_split, p_end = min(P, p_beg + g.pix_per_split);
  const int wm = (w / WN) * (BM_ / WM), wn = (w % WN) * (BN_ / WN);
  constexpr int ACPR = BM_ / 8, BCPR = BN_ / 8;  // chunks per LDS row

  // PF = 1: one register set, the next K-step's loads in flight during this one's MFMAs, __syncthreads per step.
  // PF = 2: two register sets, K-steps kt+1 and kt+2 in flight; the per-step barrier is a raw s_barrier after
  // lgkmcnt(0) (this wave's LDS traffic), so the younger register loads stay in flight across it (a
  // __syncthreads would drain vmcnt to 0 and leave one step of latency hiding).
  u32x4 ra[ACH], rb[BCH], ra2[ACH], rb2[BCH];
  // Per-thread constants: a thread always stages the same 16-byte column chunk, so its (tap, c) and the
  // row offsets of its chunks are fixed; only the pixel base moves (by 64) per K step.
  const int a_cc = t % ACPR, a_pr0 = t / ACPR;
  const int b_cc = t % BCPR, b_pr0 = t / BCPR;
  const int b_nn = n0 + b_cc * 8;
  const bool b_colok = b_nn < Ntot;
  const float inv_C = 1.f / g.C, inv_S = 1.f / g.S, inv_HoWo = 1.f / (g.Ho * g.Wo), inv_Wo = 1.f / g.Wo;
  const int b_tap = b_colok ? fdiv(b_nn, inv_C) : 0;
  const int b_c = b_colok ? b_nn - b_tap * g.C : 0;
  const int b_r = fdiv(b_tap, inv_S), b_s = b_tap - fdiv(b_tap, inv_S) * g.S;
  const int HoWo = g.Ho * g.Wo;
  // Branch-free staging: every load is unconditional from a clamped (valid) address, its validity kept in a
  // bit of `okm`; the zeroing select happens at the LDS store, after this K-step's MFMAs.  (A per-lane
  // condition around a load compiles to a branch and a wait for that load: the staging loads of a K-step
  // were serialised on the memory latency.)
  unsigned okm = 0u, okm2 = 0u;
  auto gload = [&](u32x4* ra, u32x4* rb, unsigned& okm, int p0) {
    okm = 0u;
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const int p = p0 + a_pr0 + i * (NT / ACPR), k = m0 + a_cc * 8;
      const bool ok = p < p_end && k < g.K;
      ra[i] = *reinterpret_cast<const u32x4*>(g.dY + (long)(p < p_end ? p : p_beg) * g.ldy + (k < g.K ? k : 0));
      okm |= (ok ? 1u : 0u) << i;
    }
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      const int p = p0 + b_pr0 + i * (NT / BCPR);
      const int pc = p < p_end ? p : p_beg;
      const int n = fdiv(pc, inv_HoWo);
      const int rem = pc - n * HoWo;
      const int oh = fdiv(rem, inv_Wo), ow = rem - oh * g.Wo;
      const int ih = oh * g.st - g.pad + b_r, iw = ow * g.st - g.pad + b_s;
      const bool ok = p < p_end && b_colok && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
      const int ihc = ih < 0 ? 0 : (ih >= g.H ? g.H - 1 : ih), iwc = iw < 0 ? 0 : (iw >= g.W ? g.W - 1 : iw);
      rb[i] = *reinterpret_cast<const u32x4*>(g.X + (((long)n * g.H + ihc) * g.W + iwc) * g.C + b_c);
      okm |= (ok ? 1u : 0u) << (ACH + i);
    }
  };
  auto lstore = [&](int buf, const u32x4* ra, const u32x4* rb, unsigned okm) {
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const int ch = t + NT * i;
      *reinterpret_cast<u32x4*>(&lds[buf][(ch / ACPR) * LDM + (ch % ACPR) * 8]) = ((okm >> i) & 1u) ? ra[i] : z;
    }
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      const int ch = t + NT * i;
      *reinterpret_cast<u32x4*>(&lds[buf][64 * LDM + (ch / BCPR) * LDN + (ch % BCPR) * 8]) =
          ((okm >> (ACH + i)) & 1u) ? rb[i] : z;
    }
  };
  // transposed fragment: elements j=0..7 = Img[k0 + 8*(lane>>4) + j][c0 + (lane&15)]
  auto tr_frag = [&](const bf16_t* img, int ld, int k0, int c0) -> bf16x8 {
    const int q = (lane & 15) >> 2, p4 = (lane & 3) * 4;
    const int kr = k0 + 8 * (lane >> 4);
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + (kr + q) * ld + c0 + p4));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + (kr + 4 + q) * ld + c0 + p4));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };

  f32x4 acc[IT][JT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (p_end - p_beg + 63) / 64;
  auto compute = [&](int cur) {
    const bf16_t* Aimg = &lds[cur][0];
    const bf16_t* Bimg = &lds[cur][64 * LDM];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 af[IT], bfr[JT];
#pragma unroll
      for (int i = 0; i < IT; ++i) af[i] = tr_frag(Aimg, LDM, s * 32, wm + i * 16);
#pragma unroll
      for (int j = 0; j < JT; ++j) bfr[j] = tr_frag(Bimg, LDN, s * 32, wn + j * 16);
#pragma unroll
      for (int i = 0; i < IT; ++i)
#pragma unroll
        for (int j = 0; j < JT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  };
  if (PF == 1) {
    if (nk > 0) {
      gload(ra, rb, okm, p_beg);
      lstore(0, ra, rb, okm);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      gload(ra, rb, okm, p_beg + (kt + 1 < nk ? kt + 1 : kt) * 64);  // unconditional (the last one re-reads, unused)
      compute(cur);
      if (kt + 1 < nk) lstore(cur ^ 1, ra, rb, okm);
      __syncthreads();
    }
  } else {
    // set 1 (ra, rb) carries the even K-steps, set 2 the odd ones; loads past the end re-read step nk-1, unused
    auto kstep = [&](int k) { return p_beg + (k < nk ? k : nk - 1) * 64; };
    if (nk > 0) {
      gload(ra, rb, okm, p_beg);
      gload(ra2, rb2, okm2, kstep(1));
      lstore(0, ra, rb, okm);
    }
    lds_barrier();
    for (int kt = 0; kt < nk; kt += 2) {
      gload(ra, rb, okm, kstep(kt + 2));  // set 1 was stored into LDS by the previous step
      compute(0);
      if (kt + 1 < nk) lstore(1, ra2, rb2, okm2);
      lds_barrier();
      if (kt + 1 >= nk) break;
      gload(ra2, rb2, okm2, kstep(kt + 3));
      compute(1);
      if (kt + 2 < nk) lstore(0, ra, rb, okm);
      lds_barrier();
    }
  }
  // partial tile -> this split's fp32 slab [K][R*S*C] (plain coalesced stores; summed by wgrad_reduce)
  float* slab = g.ws + (long)blockIdx.z * g.K * Ntot;
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      const int nn = n0 + wn + j * 16 + (lane & 15);
      if (nn >= Ntot) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int k = m0 + wm + i * 16 + (lane >> 4) * 4 + rr;
        if (k < g.K) slab[(long)k * Ntot + nn] = acc[i][j][rr];
      }
    }
}

// wgrad on a global_load_lds ring (the conv_pipe_kernel structure): no staging registers, STAGES-1 K-steps of
// 64 pixels in flight across each barrier (counted vmcnt + raw s_barrier).  LDS images [64 pixels][BM | BN]
// are dense rows of 16-byte chunks, chunk c of row r stored at c ^ wswz(r) (the DMA writes lane-linear, so the
// XOR is applied to each lane's SOURCE chunk and to the transposed fragment read): the 4 rows one
// ds_read_b64_tr_b16 lane group reads land on distinct bank groups.  Spatial padding, pixels past the split
// and channels past K / R*S*C read a 16-byte zero chunk in global memory.  Same partial slabs as wgrad_kernel.

__device__ __forceinline__ int wswz(int row, int nchunks) { return ((row & 7) << 1) & (nchunks - 1); }

// ds_read_b64_tr_b16 beside LDS-DMAs in flight.  Through the builtin, hipcc waits vmcnt(0) before the first transposed
// read after a global_load_lds (it cannot tell the ring slot being read from the one being filled): the K loops below
// issued the next K-step's DMAs and then drained them before reading the current one -- no K-step of fill ever
// overlapped compute (the .s of wgrad_pipe_kernel had `s_waitcnt vmcnt(0)` ahead of each K-step's reads; without the
// per-step DMA issue the layer1 K-step took 0.68 us instead of 1.11, profiles/r08/wgrad_bound.txt).  As inline asm the
// read carries no memory operand, so the counted vmcnt waits of the loop are the only ones; the compiler then does
// not count these reads on lgkmcnt either: lds_tr_wait<N>() + frag_ready() before the first use of a fragment.
__device__ __forceinline__ s16x4 lds_read_tr16(const void* p) {
  typedef __attribute__((address_space(3))) const char lds_cchar;
  const uint32_t a = (uint32_t)(uintptr_t)(lds_cchar*)p;
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(a) : "memory");
  return v;
}
// at most N LDS reads of this wave still in flight (they return in order)
template <int N>
__device__ __forceinline__ void lds_tr_wait() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}
// orders every use of f after the volatile asm statements before this one (the wait)
__device__ __forceinline__ void frag_ready(bf16x8& f) { asm volatile("" : "+v"(f)); }

// KG > 1: in-workgroup split-K over the pixels, as in conv_pipe_kernel: KG groups of WM x WN waves, each with its own
// ring and a contiguous 1/KG of the split's K-steps; the groups' tiles are summed in LDS in group order before the one
// slab store.  A KG = 2 launch covers the pixels of two one-group splits with the same waves per CU, so it writes (and
// the fold re-reads) half the fp32 slabs -- ~0.5 of the ~1 GB per step the trunk's weight gradients moved.
template <int BM_, int BN_, int WM, int WN, int STAGES, int KS = 64, int KG = 1>
__global__ __launch_bounds__(64 * WM * WN * KG, KG > 1 ? WM * WN * KG / 4 : 2) void wgrad_pipe_kernel(WgradGeom g) {
  constexpr int WAVES = WM * WN;  // per K-group
  constexpr int ACW = BM_ / 8, BCW = BN_ / 8;           // 16-byte chunks per LDS row
  constexpr int ARI = 64 / ACW, BRI = 64 / BCW;         // rows per glds instruction
  constexpr int IA = KS / ARI / WAVES, IB = KS / BRI / WAVES;  // glds per wave per K-step of KS pixels
  static_assert(IA * ARI * WAVES == KS && IB * BRI * WAVES == KS, "the K-step must split into whole glds rows");
  static_assert(KS % 32 == 0, "MFMA k = 32 pixels");
  constexpr int IT = BM_ / WM / 16, JT = BN_ / WN / 16;
  constexpr int BUF = KS * (BM_ + BN_);                 // bf16 elements per ring slot
  extern __shared__ __attribute__((aligned(16))) bf16_t smem_all[];
  const int t = threadIdx.x, lane = t & 63, kg = (t >> 6) / WAVES, w = (t >> 6) % WAVES;
  CTP(0);  // (timing build: tools/pipe_phases.py, slots as in conv_pipe_kernel)
  bf16_t* const smem = smem_all + kg * STAGES * BUF;  // this K-group's ring
  const int Ntot = g.R * g.S * g.C;
  const int P = g.N * g.Ho * g.Wo;
  const int wnx = (Ntot + BN_ - 1) / BN_, wny = (g.K + BM_ - 1) / BM_;
  int wtx, wty, zs;
  if (g.flat) {
    // Every tile of one split reads the same pixel range (dY rows and, for an R x S conv, R*S shifted windows of X
    // rows).  Split-major over the bijective XCD chunks (xcd_tile on the flattened (split, tile) index): an XCD runs
    // whole splits, so their tiles fetch the rows into ITS L2 once.  With the z grid the T tiles of a split went
    // to T different XCDs (linear dispatch order round-robins XCDs) and each re-fetched the rows from HBM:
    // layer1's 3x3 wgrad read 244 MB per launch for 51 MB of operands (gpurun_out/pmcstep).
    int tile;
    xcd_tile(blockIdx.x, wnx * wny, (int)gridDim.x, tile, zs);
    wty = tile / wnx;
    wtx = tile - wty * wnx;
  } else {
    xcd_tile(blockIdx.x, wnx, wnx * wny, wtx, wty);
    zs = blockIdx.z;
  }
  const int m0 = wty * BM_, n0 = wtx * BN_;
  const int p_beg = zs * g.pix_per_split, p_end = min(P, p_beg + g.pix_per_split);
  const int wm = (w / WN) * (BM_ / WM), wn = (w % WN) * (BN_ / WN);
  const bf16_t* zero = reinterpret_cast<const bf16_t*>(mer_conv_zero16);

  // this K-group's K-steps [kb, kb + nk) of the split's nk_all (every group runs the loop nkg times: workgroup-wide
  // barriers)
  const int nk_all = (p_end - p_beg + KS - 1) / KS;
  const int nkg = (nk_all + KG - 1) / KG, kb = __builtin_amdgcn_readfirstlane(kg * nkg);  // (kg is wave-uniform)
  const int nk = nk_all - kb < nkg ? (nk_all - kb > 0 ? nk_all - kb : 0) : nkg;
  const int pk0 = p_beg + kb * KS;

  // Staging walks the pixels incrementally: K-steps are staged strictly in order, pk0 first, and a lane's pixel moves
  // KS pixels per step.  Per DMA a lane keeps its source pointer (it may lie outside the tensor -- padding taps, pixels
  // past the split -- and is then only ever an operand of a select against the zero chunk) and, for the X operand, the
  // output pixel's (oh, ow): KS = (dn, dh, dw) in (image, row, column) steps is split once, so a step is two bounded
  // carries and one pointer add -- no division and no 64-bit multiply in the loop.
  const int HoWo = g.Ho * g.Wo;
  const bf16_t* ap[IA];  // dY: linear in the pixel
  int arow[IA];
  bool acok[IA];
#pragma unroll
  for (int j = 0; j < IA; ++j) {
    arow[j] = (w * IA + j) * ARI + lane / ACW;
    const int acol = m0 + ((lane % ACW) ^ wswz(arow[j], ACW)) * 8;
    acok[j] = acol < g.K;
    ap[j] = g.dY + ((long)(pk0 + arow[j]) * g.ldy + acol);
  }
  const long a_step = (long)KS * g.ldy;
  const bf16_t* bp[IB];  // X: the tap's pixel of output pixel (n, oh, ow), channel chunk included
  int brow[IB], boh[IB], bow[IB], bdr[IB], bds[IB];  // tap offset (dr, ds) = (r - pad, s - pad)
  bool bcok[IB];
#pragma unroll
  for (int j = 0; j < IB; ++j) {
    brow[j] = (w * IB + j) * BRI + lane / BCW;
    const int col = n0 + ((lane % BCW) ^ wswz(brow[j], BCW)) * 8;
    bcok[j] = col < Ntot;
    const int cc = bcok[j] ? col : 0;
    const int tap = cc / g.C, c = cc - tap * g.C;
    const int r = tap / g.S;
    bdr[j] = r - g.pad;
    bds[j] = tap - r * g.S - g.pad;
    const int p = pk0 + brow[j];
    const int n = p / HoWo, rem = p - n * HoWo;
    boh[j] = rem / g.Wo;
    bow[j] = rem - boh[j] * g.Wo;
    bp[j] = g.X + ((((long)n * g.H + boh[j] * g.st + bdr[j]) * g.W + bow[j] * g.st + bds[j]) * g.C + c);
  }
  const int s_dn = KS / HoWo, s_rem = KS - s_dn * HoWo, s_dh = s_rem / g.Wo, s_dw = s_rem - s_dh * g.Wo;
  const int d_step = ((s_dn * g.H + s_dh * g.st) * g.W + s_dw * g.st) * g.C;  // element deltas: the plain step,
  const int d_wrap_w = g.st * (g.W - g.Wo) * g.C;                            // ow -= Wo, oh += 1
  const int d_wrap_h = (g.H - g.Ho * g.st) * g.W * g.C;                      // oh -= Ho, n += 1
  int p_left = p_end - pk0;  // pixels of the split from the K-step being staged on
  auto stage = [&](int slot) {
    bf16_t* la = smem + slot * BUF;
    bf16_t* lb = la + KS * BM_;
#pragma unroll
    for (int j = 0; j < IA; ++j) {
      glds16(((int)(arow[j] < p_left) & (int)acok[j]) ? ap[j] : zero, la + (w * IA + j) * 512);
      ap[j] += a_step;
    }
#pragma unroll
    for (int j = 0; j < IB; ++j) {
      // (all four tests evaluated, one select: no per-lane branch)
      const int ok = (int)(brow[j] < p_left) & (int)bcok[j] &
                     (int)((unsigned)(__mul24(boh[j], g.st) + bdr[j]) < (unsigned)g.H) &
                     (int)((unsigned)(__mul24(bow[j], g.st) + bds[j]) < (unsigned)g.W);
      glds16(ok ? bp[j] : zero, lb + (w * IB + j) * 512);
      int d = d_step;
      bow[j] += s_dw;
      const bool cw = bow[j] >= g.Wo;
      bow[j] -= cw ? g.Wo : 0;
      d += cw ? d_wrap_w : 0;
      boh[j] += s_dh + (cw ? 1 : 0);
      const bool ch = boh[j] >= g.Ho;
      boh[j] -= ch ? g.Ho : 0;
      d += ch ? d_wrap_h : 0;
      bp[j] += d;
    }
    p_left -= KS;
  };
  // transposed fragment from a swizzled image with CW chunks per row: elements j = 0..7 =
  // Img[k0 + 8*(lane>>4) + j][c0 + (lane&15)]
  auto tr_frag = [&](const bf16_t* img, int CW, int k0, int c0) -> bf16x8 {
    const int q = (lane & 15) >> 2, p4 = (lane & 3) * 4;
    const int kr = k0 + 8 * (lane >> 4);
    const int lc = (c0 + p4) >> 3, sub = (c0 + p4) & 7;
    const int r0 = kr + q, r1 = kr + 4 + q;
    const s16x4 lo = lds_read_tr16(img + r0 * CW * 8 + ((lc ^ wswz(r0, CW)) << 3) + sub);
    const s16x4 hi = lds_read_tr16(img + r1 * CW * 8 + ((lc ^ wswz(r1, CW)) << 3) + sub);
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };

  f32x4 acc[IT][JT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int G = IA + IB;
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nk) stage(s);
  int wslot = STAGES - 1, rslot = 0;  // ring slots: wrapping counters
#ifdef MER_CONV_TIMING
  bf16x8 af_h[KS / 32][IT] = {}, bfr_h[KS / 32][JT] = {};  // CT_MODE() 2: the first K-step's fragments, reused
#endif
  CTP(1);
  for (int kt = 0; kt < nkg; ++kt) {
    const int left = nk - 1 - kt;
    const int ahead = left < (STAGES - 2) ? left : (STAGES - 2);
    wait_tiles_in_flight<G>(ahead);
    lds_barrier();
    if (kt + STAGES - 1 < nk && CT_MODE() != 1) stage(wslot);
    wslot = wslot == STAGES - 1 ? 0 : wslot + 1;
    const bf16_t* Aimg = smem + rslot * BUF;
    rslot = rslot == STAGES - 1 ? 0 : rslot + 1;
    if (KG > 1 && kt >= nk) continue;
    const bf16_t* Bimg = Aimg + KS * BM_;
#pragma unroll
    for (int s = 0; s < KS / 32; ++s) {
      bf16x8 af[IT], bfr[JT];
#ifdef MER_CONV_TIMING
      if (CT_MODE() == 2 && kt > 0) {
#pragma unroll
        for (int i = 0; i < IT; ++i) af[i] = af_h[s][i];
#pragma unroll
        for (int j = 0; j < JT; ++j) bfr[j] = bfr_h[s][j];
      } else
#endif
      {
#pragma unroll
        for (int i = 0; i < IT; ++i) af[i] = tr_frag(Aimg, ACW, s * 32, wm + i * 16);
#pragma unroll
        for (int j = 0; j < JT; ++j) bfr[j] = tr_frag(Bimg, BCW, s * 32, wn + j * 16);
        lds_tr_wait<0>();
#pragma unroll
        for (int i = 0; i < IT; ++i) frag_ready(af[i]);
#pragma unroll
        for (int j = 0; j < JT; ++j) frag_ready(bfr[j]);
      }
#ifdef MER_CONV_TIMING
      if (kt == 0) {
#pragma unroll
        for (int i = 0; i < IT; ++i) af_h[s][i] = af[i];
#pragma unroll
        for (int j = 0; j < JT; ++j) bfr_h[s][j] = bfr[j];
      }
#endif
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < IT; ++i)
#pragma unroll
        for (int j = 0; j < JT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  }
  CTP(2);
  if constexpr (KG > 1) {  // groups 1.. hand their tiles to group 0 through LDS; group 0 sums in group order
    constexpr int LDR = BN_ + 4;
    __syncthreads();  // every group's last fragment reads are done before the exchange reuses the rings
    float* const part = reinterpret_cast<float*>(smem_all);
    if (kg > 0) {
      float* mine = part + (kg - 1) * BM_ * LDR;
#pragma unroll
      for (int i = 0; i < IT; ++i)
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            mine[(wm + i * 16 + (lane >> 4) * 4 + rr) * LDR + wn + j * 16 + (lane & 15)] = acc[i][j][rr];
    }
    lds_barrier();
    if (kg > 0) return;
#pragma unroll
    for (int i = 0; i < IT; ++i)
#pragma unroll
      for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
          for (int q = 1; q < KG; ++q)
            acc[i][j][rr] += part[(q - 1) * BM_ * LDR + (wm + i * 16 + (lane >> 4) * 4 + rr) * LDR + wn + j * 16 +
                                  (lane & 15)];
  }
  CTP(3);
  float* slab = g.ws + (long)zs * g.K * Ntot;
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      const int nn = n0 + wn + j * 16 + (lane & 15);
      if (nn >= Ntot) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int k = m0 + wm + i * 16 + (lane >> 4) * 4 + rr;
        if (k < g.K) slab[(long)k * Ntot + nn] = acc[i][j][rr];
      }
    }
  CTP(4);
}

// ---------------------------------------------------------------------------------------
// Strip weight gradient of a 3x3 / stride-1 / pad-1 conv (variants 9 and 10): all nine taps from ONE LDS strip.
// wgrad_pipe_kernel tiles the (tap, c) axis over workgroups, so every 64x128 tile DMAs its own dY tile and its own
// shifted X window each K-step: layer1 filled LDS with ~376 MB per launch for 51 MB of operands, and the nine taps'
// windows are the same rows shifted by a pixel or an image row.  Here the reduction runs over a PADDED pixel index q:
// an image is H rows of W + 1 slots (slot W is the pad column -- one row's right pad and the next row's left pad)
// followed by one pad row, so in q space tap (r, s) is the constant shift (r - 1) * (W + 1) + (s - 1) and every
// border tap, the corners and the image seams included, lands on a pad slot:
//   dw[k][(r, s, c)] = sum_q dY[q][k] * X[q + (r - 1) * (W + 1) + (s - 1)][c],  dY = X = 0 at pad slots
// (pad slots DMA the 16-byte zero chunk: validity is evaluated unconditionally and feeds a select).  The cost is
// (H + 1)(W + 1) / (H W) more K: 7 % at 28x28, 15 % at 14x14.
// A workgroup owns a (KB output channels) x (9 taps x 64 input channels) tile of one split.  X rows stream through a
// ring of `xrows` LDS rows [q][64 channels] addressed by (stream row & (xrows - 1)); a K-step of 64 slots DMAs 64 new
// X rows and its 64 dY rows ([q][KB], a STAGES-deep ring) and reads rows [64 kt, 64 kt + 64 + 2 (W + 2)) of the X
// stream, which begins W + 2 rows before the split.  12 waves = (tap row r) x (16-channel quarter): a wave reads its dY
// fragments once per 32 slots and serves its three taps s = 0..2 from the strip at row base r (W + 1) + s with
// ds_read_b64_tr_b16 -- per K-step 2 x (KB/16 + 3) fragments for 2 x 3 KB/16 MFMAs.  Rows of 8 (4) 16-byte chunks
// are XOR-swizzled by row bits 1 and 3 (bit 3): the 8 rows {b..b+3, b+8..b+11} one 32-lane half of a transposed read
// touches then cover all 64 banks for any row base b.  Splits are ranges of image rows (pad rows included); the
// slabs are wgrad_pipe_kernel's [split][K][tap * C + c], the grid its split-major XCD order.
struct StripGeom {
  int N, H, W, C, K;
  const bf16_t* X;
  const bf16_t* dY;
  float* ws;
  int ldy;
  int rows_per_split;  // image rows (pad rows included) per split
  int xrows;           // rows of the X ring: a power of two >= 64 * (ceil(2 (W + 2) / 64) + STAGES)
};

__device__ __forceinline__ int sswz(int row, int nchunks) {
  return nchunks == 8 ? ((row & 2) | ((row >> 1) & 4)) : ((row >> 2) & 2);
}

// one DMA instruction's lane state: the source of this lane's 16 bytes (row `u` of the operand's stream, at padded
// slot (n, h, w)), walked 64 slots per issue with two bounded carries as in wgrad_pipe_kernel
struct StripUnit {
  const bf16_t* p;
  int n, h, w, u, lim, stride, wstride, dstep;
};

template <int KB, int STAGES>
__global__ __launch_bounds__(768, 3) void wgrad_strip_kernel(StripGeom g) {
  constexpr int KS = 64, NW = 12;
  constexpr int ACW = KB / 8;    // 16-byte chunks per dY row
  constexpr int ARI = 64 / ACW;  // dY rows per DMA instruction
  constexpr int NDU = KS / ARI;  // dY DMA instructions per K-step (the X chunk takes 8)
  constexpr int IT = KB / 16;
  constexpr int ABUF = KS * KB;  // bf16 elements per dY ring slot
  static_assert(NDU >= NW - 8 && 8 + NDU <= 2 * NW, "8 X + NDU dY instructions over 12 waves, one or two each");
  static_assert(STAGES >= 2 && STAGES <= 4, "vmcnt waits below cover (STAGES - 2) * 2 <= 4");
  extern __shared__ __attribute__((aligned(16))) bf16_t smem_all[];
  bf16_t* const xring = smem_all;
  bf16_t* const aring = smem_all + g.xrows * 64;
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  CTP(0);
  const int Wp = g.W + 1, Hp = g.H + 1, IQ = Hp * Wp, HL = Wp + 1;
  const int Ntot = 9 * g.C;
  const int nct = g.C / 64, ntile = nct * (g.K / KB);
  int tile, zs;
  xcd_tile(blockIdx.x, ntile, (int)gridDim.x, tile, zs);
  const int kti = tile / nct, cti = tile - kti * nct;
  const int k0 = kti * KB, c0 = cti * 64;
  const int TR = g.N * Hp;
  const int rb = zs * g.rows_per_split, re = min(TR, rb + g.rows_per_split);
  const int qb = rb * Wp, qlen = (re - rb) * Wp;
  const int nk = (qlen + KS - 1) / KS;
  const int NH = (2 * HL + KS - 1) / KS;  // X chunks a K-step reads beyond its own
  const int xmask = g.xrows - 1;
  const bf16_t* zero = reinterpret_cast<const bf16_t*>(mer_conv_zero16);

  const int s_dn = KS / IQ, s_rem = KS - s_dn * IQ, s_dh = s_rem / Wp, s_dw = s_rem - s_dh * Wp;
  auto unit_init = [&](bool isx, int ui) -> StripUnit {
    StripUnit a;
    int row, chunk;
    if (isx) {
      row = ui * 8 + (lane >> 3);
      chunk = (lane & 7) ^ sswz(row, 8);
      a.stride = g.C;
      a.lim = qlen + 2 * HL;
    } else {
      row = ui * ARI + lane / ACW;
      chunk = (lane % ACW) ^ sswz(row, ACW);
      a.stride = g.ldy;
      a.lim = qlen;
    }
    const int qq = qb + row - (isx ? HL : 0) + IQ;  // >= 0: the first image's halo lies in "image -1"
    const int n1 = qq / IQ, rem = qq - n1 * IQ;
    a.n = n1 - 1;
    a.h = rem / Wp;
    a.w = rem - a.h * Wp;
    a.u = row;
    a.wstride = g.W * a.stride;
    a.dstep = ((s_dn * g.H + s_dh) * g.W + s_dw) * a.stride;
    // (outside the tensor at pad slots: then only ever an operand of the select against the zero chunk)
    a.p = (isx ? g.X + c0 : g.dY + k0) + (((long)a.n * g.H + a.h) * g.W + a.w) * a.stride + chunk * 8;
    return a;
  };
  auto issue = [&](StripUnit& a, bf16_t* dst) {
    const int ok = (int)(a.u < a.lim) & (int)((unsigned)a.n < (unsigned)g.N) & (int)(a.h < g.H) & (int)(a.w < g.W);
    glds16(ok ? a.p : zero, dst);
    a.u += KS;
    int d = a.dstep;
    a.w += s_dw;
    const bool cw = a.w >= Wp;  // w -= W + 1, h += 1
    a.w -= cw ? Wp : 0;
    d -= cw ? a.stride : 0;
    a.h += s_dh + (cw ? 1 : 0);
    const bool ch = a.h >= Hp;  // h -= H + 1, n += 1
    a.h -= ch ? Hp : 0;
    d -= ch ? a.wstride : 0;
    a.n += s_dn + (ch ? 1 : 0);
    a.p += d;
  };
  // DMA instruction `unit` of a K-step: 0..7 the X chunk's 8-row groups, 8.. the dY rows.  Wave w issues unit w and,
  // where there is one, unit w + 12 (always dY).
  const bool s0x = w < 8;
  const bool has1 = NDU > NW - 8 && w + NW - 8 < NDU;
  StripUnit u0 = unit_init(s0x, s0x ? w : w - 8);
  StripUnit u1 = unit_init(false, has1 ? w + NW - 8 : 0);
  int xw = 0;  // ring row of the next X chunk
  auto stage_x = [&]() {
    if (s0x) issue(u0, xring + (xw + w * 8) * 64);
    xw = (xw + KS) & xmask;
  };
  auto stage = [&](int aslot) {  // K-step j: X chunk j + NH and dY chunk j
    bf16_t* la = aring + aslot * ABUF;
    stage_x();
    if (!s0x) issue(u0, la + (w - 8) * 512);
    if (has1) issue(u1, la + (w + NW - 8) * 512);
  };

  // fragment addresses (bytes from the ring bases): the dY ones are fixed per ring slot; an X row is
  // (64 kt + fixed) & xmask, and its swizzle reads row bits 1 and 3 only, so the column part is fixed too
  const int g4 = lane >> 4, fq = (lane & 15) >> 2, p4 = (lane & 3) * 4;
  const int tr = w >> 2, cq = w & 3;  // this wave's tap row and channel quarter
  int aoff[2][2][IT], xrow[3][2][2], xcol[3][2][2];
#pragma unroll
  for (int ss = 0; ss < 2; ++ss)
#pragma unroll
    for (int hi = 0; hi < 2; ++hi) {
      const int row = ss * 32 + 8 * g4 + 4 * hi + fq;
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int col = i * 16 + p4;
        aoff[ss][hi][i] = (row * KB + ((((col >> 3) ^ sswz(row, ACW))) << 3) + (col & 7)) * 2;
      }
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int xr = row + tr * Wp + s;
        const int col = cq * 16 + p4;
        xrow[s][ss][hi] = xr * 128;
        xcol[s][ss][hi] = (((((col >> 3) ^ sswz(xr, 8))) << 3) + (col & 7)) * 2;
      }
    }
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  auto frag = [&](const char* lo_p, const char* hi_p) -> bf16x8 {
    const s16x4 lo = lds_read_tr16(lo_p);
    const s16x4 hi = lds_read_tr16(hi_p);
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };

  f32x4 acc[3][IT];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int i = 0; i < IT; ++i) acc[s][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const char* const Xb = reinterpret_cast<const char*>(xring);
  auto read_frags = [&](int ss, const char* Ab, int xbB, bf16x8* af, bf16x8* bfr) {
#pragma unroll
    for (int i = 0; i < IT; ++i) af[i] = frag(Ab + aoff[ss][0][i], Ab + aoff[ss][1][i]);
#pragma unroll
    for (int s = 0; s < 3; ++s)
      bfr[s] = frag(Xb + (((xbB + xrow[s][ss][0]) & (g.xrows * 128 - 1)) + xcol[s][ss][0]),
                    Xb + (((xbB + xrow[s][ss][1]) & (g.xrows * 128 - 1)) + xcol[s][ss][1]));
    __builtin_amdgcn_sched_barrier(0);
  };
  constexpr int NFR = 2 * (IT + 3);  // LDS reads of one fragment set
  auto frags_ready = [&](bf16x8* af, bf16x8* bfr) {
#pragma unroll
    for (int i = 0; i < IT; ++i) frag_ready(af[i]);
#pragma unroll
    for (int s = 0; s < 3; ++s) frag_ready(bfr[s]);
  };
  auto mfma_all = [&](const bf16x8* af, const bf16x8* bfr) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int i = 0; i < IT; ++i) acc[s][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[s], acc[s][i], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  bf16x8 af0[IT], bf0[3], af1[IT] = {}, bf1[3] = {};

  for (int pc = 0; pc < NH; ++pc) stage_x();  // the X stream's first NH chunks: the halo before the split
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nk) stage(s);
  int wslot = STAGES - 1, rslot = 0;
  const int xmaskB = g.xrows * 128 - 1;
  int xbB = 0;  // byte offset of stream row 64 kt in the X ring
  const int gw = has1 ? 2 : 1;  // this wave's DMAs per stage
  CTP(1);
  for (int kt = 0; kt < nk; ++kt) {
    const int left = nk - 1 - kt;
    const int fly = (left < (STAGES - 2) ? left : (STAGES - 2)) * gw;  // own DMAs that may stay in flight
    if (fly <= 0) wait_vmcnt<0>();
    else if (fly == 1) wait_vmcnt<1>();
    else if (fly == 2) wait_vmcnt<2>();
    else wait_vmcnt<4>();
    lds_barrier();
    if (kt + STAGES - 1 < nk && CT_MODE() != 1) stage(wslot);
    wslot = wslot == STAGES - 1 ? 0 : wslot + 1;
    const char* Ab = reinterpret_cast<const char*>(aring + rslot * ABUF);
    rslot = rslot == STAGES - 1 ? 0 : rslot + 1;
    // two fragment sets, the reads one half-step ahead of the MFMAs: every wave reads right after the barrier, so
    // without MFMAs to issue meanwhile the LDS time of all 12 waves' reads was exposed in every half-step
    frags_ready(af1, bf1);  // set 1's reads of K-step kt - 1 retired at the barrier's lgkmcnt(0)
    if (CT_MODE() != 2 || kt == 0) read_frags(0, Ab, xbB, af0, bf0);
    mfma_all(af1, bf1);  // half-step 1 of K-step kt - 1 (zeros before the first)
    if (CT_MODE() != 2 || kt == 0) read_frags(1, Ab, xbB, af1, bf1);
    lds_tr_wait<NFR>();  // set 0 has landed, set 1 may still be in flight
    frags_ready(af0, bf0);
    mfma_all(af0, bf0);
    xbB = (xbB + KS * 128) & xmaskB;
  }
  lds_tr_wait<0>();
  frags_ready(af1, bf1);
  mfma_all(af1, bf1);
  CTP(2);
  CTP(3);
  float* slab = g.ws + (long)zs * g.K * Ntot;
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int nn = (tr * 3 + s) * g.C + c0 + cq * 16 + (lane & 15);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) slab[(long)(k0 + i * 16 + g4 * 4 + rr) * Ntot + nn] = acc[s][i][rr];
    }
  CTP(4);
}

// slab0[i] = sum_z ws[z][i] over the flat [K][R*S*C] index.  A block owns E = 256/SG consecutive elements
// and SG split-groups: thread (sg, e) sums splits sg, sg+SG, ... with 4 independent loads in flight (the
// split count reaches ~100 on the stem / layer1, where one serial chain per element was latency-bound),
// and the SG partials meet in LDS.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(int K, int C, int Creal, int RS, int splits, int SG,
                                                           float* __restrict__ ws) {
  __shared__ float part[256];
  const int E = 256 / SG, e = threadIdx.x % E, sg = threadIdx.x / E;
  const long total = (long)K * RS * C;
  const long idx = (long)blockIdx.x * E + e;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (idx < total) {
    int z = sg;
    for (; z + 3 * SG < splits; z += 4 * SG) {
      a0 += ws[(long)z * total + idx];
      a1 += ws[(long)(z + SG) * total + idx];
      a2 += ws[(long)(z + 2 * SG) * total + idx];
      a3 += ws[(long)(z + 3 * SG) * total + idx];
    }
    for (; z < splits; z += SG) a0 += ws[(long)z * total + idx];
  }
  part[threadIdx.x] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (sg != 0 || idx >= total) return;
  float s = 0.f;
  for (int q = 0; q < SG; ++q) s += part[q * E + e];
  ws[idx] = s;  // slab 0 (only this block ever reads element idx)
}

// dw[k][c][r][s] += sum_z ws[z][k][(r*S+s)*C + c] for c < Creal, in split order: one pass replacing the
// reduce + scatter pair.  Block (channel group of 32, k): each thread sums its (tap, channel) elements over
// the splits (8 loads in flight, clamped, branch-free) into an LDS [tap][32] tile, written back in the
// PyTorch order (c, r, s) -- a contiguous run of 32*R*S floats.
__global__ __launch_bounds__(256) void wgrad_fold_scatter_kernel(int K, int C, int Creal, int RS, int splits,
                                                                 const float* __restrict__ ws, float* __restrict__ dw) {
  __shared__ float tile[49 * 32];  // R*S <= 49 (7x7 stem)
  const int k = blockIdx.y, c0 = blockIdx.x * 32;
  const long slab = (long)K * RS * C;
  const float* src = ws + (long)k * RS * C;
  for (int i = threadIdx.x; i < RS * 32; i += 256) {
    const int tap = i >> 5, c = c0 + (i & 31);
    const float* e = src + tap * C + (c < Creal ? c : 0);
    float s = 0.f;
    for (int z0 = 0; z0 < splits; z0 += 8) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = e[(long)(z0 + q < splits ? z0 + q : splits - 1) * slab];
#pragma unroll
      for (int q = 0; q < 8; ++q) s += z0 + q < splits ? v[q] : 0.f;
    }
    tile[i] = c < Creal ? s : 0.f;
  }
  __syncthreads();
  const int ncl = min(32, Creal - c0);
  const float inv_RS = 1.f / RS;
  float* dst = dw + ((long)k * Creal + c0) * RS;
  for (int i = threadIdx.x; i < ncl * RS; i += 256) {  // i = cl*RS + tap
    const int cl = fdiv(i, inv_RS), tap = i - cl * RS;
    dst[i] += tile[tap * 32 + cl];
  }
}

// dw[k][c][r][s] += slab0[k][(r*S+s)*C + c] for c < Creal.  Block (channel group of 32, k): reads coalesced
// along c (one 128-byte segment per tap) into an LDS [tap][32] tile, written back in the PyTorch order
// (c, r, s) -- a contiguous run of 32*R*S floats.
__global__ __launch_bounds__(256) void wgrad_scatter_kernel(int C, int Creal, int RS, const float* __restrict__ ws,
                                                            float* __restrict__ dw) {
  __shared__ float tile[49 * 32];  // R*S <= 49 (7x7 stem)
  const int k = blockIdx.y, c0 = blockIdx.x * 32;
  const float* src = ws + (long)k * RS * C;
  for (int i = threadIdx.x; i < RS * 32; i += 256) {
    const int tap = i >> 5, c = c0 + (i & 31);
    tile[i] = c < Creal ? src[tap * C + c] : 0.f;
  }
  __syncthreads();
  const int ncl = min(32, Creal - c0);
  const float inv_RS = 1.f / RS;
  float* dst = dw + ((long)k * Creal + c0) * RS;
  for (int i = threadIdx.x; i < ncl * RS; i += 256) {  // i = cl*RS + tap
    const int cl = fdiv(i, inv_RS), tap = i - cl * RS;
    dst[i] += tile[tap * 32 + cl];
  }
}

// Batched fold of deferred split-K partial slabs: every weight gradient of one backward segment in ONE launch
// instead of one or two per convolution (the folds were ~30 launches of 5-12 us each on the critical stream).
// Record r: dw_r[k][c][tap] += sum_z ws_r[z][k][tap*C + c] (c < Creal), or with a scatter map
// dw_r[k][map[j]] for source column j = tap*C + c (-1: dropped) -- the stem's 4x4 space-to-depth form
// gathered back to 7x7x3.
//
// The per-element summation tree is a contract (a different fp32 order grows over the Adam
// steps into parameter differences far beyond rounding): SG = 8 / 4 / 1 split groups for > 48 / > 12 / fewer slabs;
// group sg takes slabs sg + SG*i in increasing i, slab i into chain a[i % 4] (each from +0), group partial
// (a0 + a1) + (a2 + a3); s = 0, s += partial[sg] in order; dw = dw_old + s.  Only additions: any thread mapping that
// follows the tree gives the same bits.
//
// Records without a map are tiled by DESTINATION (fold_tiled): a block owns output channel k and CC channels
// [c0, c0 + CC) over all RS taps.  Its slab reads are RS segments of CC consecutive floats (whole 128-byte lines),
// 16 bytes per thread, thread (sg, e) of E = 256/SG summing group sg of tile elements e, e + E, ...; the group
// partials go to an LDS tile [sg][tap][CC + 4] and the block read-modify-writes the CONTIGUOUS run
// dw[k][c0 .. c0 + CC)[0 .. RS) in 16-byte vectors (scalar where the run's ends are not 16-byte aligned).  The dw loads
// are issued first, ahead of the slab loads: one memory round trip per block.  (The source-order form this replaces
// touched dw in 4-byte pieces RS floats apart, after the sums and the barrier: 163 us per step in the trunk trace.)
// The stem's map record keeps the source order (fold_source: a thread owns 4 consecutive source elements, block of
// E threads x SG groups), its map and dw loads hoisted above the slab loop too.
struct FoldRec {
  const float* ws;
  float* dw;
  const int* map;
  int K, C, Creal, RS, splits, SG, blk0, nblk;
  int CC, chunks;  // tiled records: channels per block, blocks per output channel
};
constexpr int kFoldMaxRecs = 32;
struct FoldTable {
  int n;
  FoldRec r[kFoldMaxRecs];
};
constexpr int kFoldTile = 5120;   // LDS floats: SG * RS * (CC + 4) of a tiled record
constexpr int kFoldSlots = 5;     // 16-byte dw vectors per thread: RS * CC < kFoldTile
constexpr int kFoldRunSG = 1016;  // SG > 1: RS * CC at most this -- one dw vector per thread

// Group partials of thread (sg, e)'s tile elements base + x*E + e, x < NEB, all at once: NB slab loads per element
// issued before their adds (clamped addresses, selected adds: no serial tail, no branch between the loads).
// ONE: n <= NB, a single batch.
template <int NB, int NEB, bool ONE>
__device__ __forceinline__ void fold_tile_body(const float* __restrict__ src, long st, int C, int SG, int sg, int e,
                                               int E, int n, int T4, int cw4, int CCp, float* part, int base) {
  static_assert(NB % 4 == 0, "chain of slab i is i % 4");
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const float inv_cw4 = 1.f / cw4;
  int so[NEB], lo[NEB];  // element offsets in the slab row and in the LDS tile
#pragma unroll
  for (int x = 0; x < NEB; ++x) {
    const int q = base + x * E + e, qc = q < T4 ? q : 0;  // (past the tile: loaded, not written)
    const int tap = fdiv(qc, inv_cw4), c4 = qc - tap * cw4;
    so[x] = tap * C + c4 * 4;
    lo[x] = tap * CCp + c4 * 4;
  }
  f32x4 a[NEB][4];
#pragma unroll
  for (int x = 0; x < NEB; ++x)
#pragma unroll
    for (int c = 0; c < 4; ++c) a[x][c] = zero4;
  // Every load of a batch is issued, unconditionally, before the first add.  hipcc otherwise moves a load whose add
  // is conditional into the branch of that add (one load, one wait, ...): the slab count is kept in a vector
  // register it cannot see through, so the adds are selects, and each loaded value passes through an empty asm
  // statement in front of its add, which keeps the load out of any branch.
  int nv = n;
  asm volatile("" : "+v"(nv));
  auto batch = [&](int i0) {
    f32x4 w[NEB][NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int i = i0 + b < nv ? i0 + b : nv - 1;
      const float* slab = src + (long)(__mul24(SG, i) + sg) * st;  // slab sg + SG*i
#pragma unroll
      for (int x = 0; x < NEB; ++x) w[x][b] = *reinterpret_cast<const f32x4*>(slab + so[x]);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int x = 0; x < NEB; ++x) {
        asm volatile("" : "+v"(w[x][b]));
        if (i0 + b < nv) a[x][b & 3] += w[x][b];
      }
  };
  // the first batch outside the loop: straight-line code behind the dw loads (hipcc drains the loads in flight, the
  // dw loads too, in front of a loop that loads)
  if (n > 0) batch(0);
  if (!ONE)
    for (int i0 = NB; i0 < n; i0 += NB) batch(i0);
#pragma unroll
  for (int x = 0; x < NEB; ++x)
    if (base + x * E + e < T4) *reinterpret_cast<f32x4*>(part + lo[x]) = (a[x][0] + a[x][1]) + (a[x][2] + a[x][3]);
}

// The thread's ceil(T4 / E) <= kFoldSlots tile elements in groups of 4, 2 and 1 (at most 16 loads in flight per
// thread); no loop, see above
template <int NB, bool ONE>
__device__ __forceinline__ void fold_tile_sum(const float* __restrict__ src, long st, int C, int SG, int sg, int e,
                                              int E, int n, int T4, int cw4, int CCp, float* part) {
  constexpr int G = NB * 4 <= 16 ? 4 : (NB * 2 <= 16 ? 2 : 1);  // elements per group
  int base = 0, ne = (T4 + E - 1) / E;                            // block-uniform
#pragma unroll
  for (int g = 0; g < kFoldSlots / G; ++g)
    if (ne >= G) {
      fold_tile_body<NB, G, ONE>(src, st, C, SG, sg, e, E, n, T4, cw4, CCp, part, base);
      ne -= G, base += G * E;
    }
  if constexpr (G == 4)
    if (ne >= 2) {
      fold_tile_body<NB, 2, ONE>(src, st, C, SG, sg, e, E, n, T4, cw4, CCp, part, base);
      ne -= 2, base += 2 * E;
    }
  if constexpr (G >= 2)
    if (ne >= 1) fold_tile_body<NB, 1, ONE>(src, st, C, SG, sg, e, E, n, T4, cw4, CCp, part, base);
}

template <int NSLOT>
__device__ __forceinline__ void fold_tiled(const FoldRec& R, int lb, float* lds) {
  const int SG = R.SG, E = 256 / SG, tid = threadIdx.x, e = tid & (E - 1), sg = tid / E;
  const int RS = R.RS, k = lb / R.chunks, c0 = (lb - k * R.chunks) * R.CC;
  const int cw = min(R.CC, ((R.Creal + 3) & ~3) - c0), cw4 = cw >> 2, CCp = R.CC + 4;  // channels read
  const int L = min(cw, R.Creal - c0) * RS;  // floats of the dw run (channels c >= Creal are dropped)
  float* __restrict__ dst = R.dw + ((long)k * R.Creal + c0) * RS;
  // the run = `head` floats up to the first 16-byte boundary, nb whole 16-byte vectors (thread tid: vectors tid,
  // tid + 256, ...), `tail` floats; the head and tail floats go one each to threads 0-2 and 3-5
  const int head = min((4 - (int)(((uintptr_t)dst >> 2) & 3)) & 3, L), nb = (L - head) >> 2, tail0 = head + 4 * nb;
  const int ei = tid < 3 ? tid : tail0 + tid - 3;
  const bool edge = tid < 3 ? tid < head : (tid < 6 && ei < L);
  const long row = (long)RS * R.C, total = (long)R.K * row;
  const float* src = R.ws + (long)k * row + c0;
  // the dw loads first (their addresses need nothing but the block's place), branch-free: a thread without a j-th
  // vector re-reads the run's last one (a run shorter than a vector: 16 bytes of the slab, unused)
  const float* dwv = nb > 0 ? dst + head : src;
  f32x4 d[NSLOT];
#pragma unroll
  for (int j = 0; j < NSLOT; ++j) d[j] = *reinterpret_cast<const f32x4*>(dwv + 4 * min(tid + 256 * j, max(nb - 1, 0)));
  const float de = dst[edge ? ei : 0];
  const int splits = R.splits, n = splits > sg ? (splits - sg + SG - 1) / SG : 0, T4 = RS * cw4;
  float* part = lds + sg * RS * CCp;
  // few slabs (layer3 / layer4: SG = 1, at most 12): every slab of 4 / 2 / 1 elements in flight at once; else batches
  // of 8 slabs of 2 elements
  if (NSLOT == 1) fold_tile_sum<8, false>(src, total, R.C, SG, sg, e, E, n, T4, cw4, CCp, part);
  else if (splits <= 4) fold_tile_sum<4, true>(src, total, R.C, 1, 0, e, E, n, T4, cw4, CCp, part);
  else if (splits <= 8) fold_tile_sum<8, true>(src, total, R.C, 1, 0, e, E, n, T4, cw4, CCp, part);
  else fold_tile_sum<12, true>(src, total, R.C, 1, 0, e, E, n, T4, cw4, CCp, part);
  __syncthreads();
  const float inv_RS = 1.f / RS;
  auto sum_at = [&](int i) {  // s of run element i = cl*RS + tap: the group partials in order
    const int cl = fdiv(i, inv_RS), tap = i - cl * RS;
    float s = 0.f;
    for (int q = 0; q < SG; ++q) s += lds[(q * RS + tap) * CCp + cl];
    return s;
  };
#pragma unroll
  for (int j = 0; j < NSLOT; ++j)
    if (tid + 256 * j < nb) {
      const int i = head + 4 * (tid + 256 * j);
      f32x4 r;
#pragma unroll
      for (int x = 0; x < 4; ++x) r[x] = d[j][x] + sum_at(i + x);
      *reinterpret_cast<f32x4*>(dst + i) = r;
    }
  if (edge) dst[ei] = de + sum_at(ei);
}

__device__ __forceinline__ void fold_source(const FoldRec& R, int lb, f32x4* part) {
  const int SG = R.SG, E = 256 / SG, e = threadIdx.x & (E - 1), sg = threadIdx.x / E;
  const long row = (long)R.RS * R.C, total = (long)R.K * row;
  const long idx = ((long)lb * E + e) * 4;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 a0 = zero4, a1 = zero4, a2 = zero4, a3 = zero4;
  const int splits = R.splits;
  const bool writer = sg == 0 && idx < total;
  const int k = (int)(idx / row), j0 = (int)(idx - (long)k * row);
  float* __restrict__ dwk = R.dw + (long)k * R.Creal;
  int o[4] = {-1, -1, -1, -1};
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  if (writer) {  // map and dw loads ahead of the slab loads
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) o[c4] = R.map[j0 + c4];
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) d[c4] = dwk[o[c4] >= 0 ? o[c4] : 0];  // the 4 read-modify-writes' loads together
  }
  if (idx < total) {
    const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(R.ws + idx);
    const long st = total / 4;
    // this thread's splits z = sg + SG * i, i < n: batches of 8 loads issued before their adds (clamped
    // addresses, zero-selected), chains a0..a3 by i % 4 -- no serial tail
    const int n = splits > sg ? (splits - sg + SG - 1) / SG : 0;
    for (int i0 = 0; i0 < n; i0 += 8) {
      f32x4 w[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = i0 + q < n ? i0 + q : n - 1;
        w[q] = src[(long)(sg + SG * i) * st];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (i0 + q < n) {
          if ((q & 3) == 0) a0 += w[q];
          else if ((q & 3) == 1) a1 += w[q];
          else if ((q & 3) == 2) a2 += w[q];
          else a3 += w[q];
        }
    }
  }
  part[threadIdx.x] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (!writer) return;
  f32x4 s4 = zero4;
  for (int q = 0; q < SG; ++q) s4 += part[q * E + e];
#pragma unroll
  for (int c4 = 0; c4 < 4; ++c4)
    if (o[c4] >= 0) dwk[o[c4]] = d[c4] + s4[c4];
}

__global__ __launch_bounds__(256) void wgrad_fold_batch_kernel(FoldTable t) {
  __shared__ __attribute__((aligned(16))) float lds[kFoldTile];
  const int v = blockIdx.x;
  const int ri = table_find(t.n, v, [&](int i) { return t.r[i].blk0; });
  const FoldRec& R = t.r[ri];
  if (R.map) fold_source(R, v - R.blk0, reinterpret_cast<f32x4*>(lds));
  else if (R.SG > 1) fold_tiled<1>(R, v - R.blk0, lds);
  else fold_tiled<kFoldSlots>(R, v - R.blk0, lds);
}

// ---------------------------------------------------------------------------------------
// The weight-gradient plan.  Which kernel a weight gradient runs, how many splits it is asked for, how many slabs it
// then writes (every split non-empty, so fewer than asked where the rounding says so), the grid, the LDS bytes and the
// workspace are resolved ONCE, by wgrad_plan() below, from the geometry and the requested variant and splits.  The
// entry points launch from the plan and mer_conv_wgrad_plan reports from it: the caller sizes its workspace and tells
// the deferred fold (mer_wgrad_fold_batch) its slab count from the same record the launch runs by, so the fold cannot
// sum slabs nobody wrote or drop written ones.
// ---------------------------------------------------------------------------------------
enum WgradForm { kWgradReg, kWgradRing, kWgradStrip };  // wgrad_kernel / wgrad_pipe_kernel / wgrad_strip_kernel

// a variant's kernel as a type; the register-staged and ring tiles are BM x 128 (output channels x (tap, c) columns)
template <int BM_, int WM_, int WN_, int PF_>
struct RegTile {
  static constexpr WgradForm form = kWgradReg;
  static constexpr int BM = BM_, WM = WM_, WN = WN_, PF = PF_, STAGES = 0, KS = 64, KG = 1;
};
template <int BM_, int STAGES_, int KS_ = 64, int KG_ = 1>
struct RingTile {
  static constexpr WgradForm form = kWgradRing;
  static constexpr int BM = BM_, WM = 2, WN = 4, STAGES = STAGES_, KS = KS_, KG = KG_;
};
template <int KB>
struct StripTile {  // BM: the tile's output channels
  static constexpr WgradForm form = kWgradStrip;
  static constexpr int BM = KB, WM = 3, WN = 4, STAGES = 4, KS = 64, KG = 1;
};

struct WgradPlan {
  int err;        // what the launch returns instead of launching (hipSuccess: launch)
  int variant;    // the resolved variant (never -1)
  int splits;     // the splits the launch is asked for (resolved: never <= 0); the workspace holds this many slabs
  int slabs;      // the slabs the launch writes (<= splits): every split non-empty
  int per_split;  // output pixels (a multiple of 64) or, strip, image rows (each image's pad row counted) per slab
  WgradForm form;
  int BM, STAGES, KS, KG;  // tile height (64 / 128; strip: its output channels), ring depth, K-step, K-groups
  int xrows;               // strip: rows of the X ring
  unsigned grid_x, grid_z, threads;
  size_t lds;              // dynamic LDS bytes
  long long ws_floats;     // splits x K x R*S*C
};

// The kernel of a resolved variant: calls f(tile type{}) and returns what f returns.  The one copy of the ladder:
// wgrad_plan() records the tile through it, launch_wgrad_plan() instantiates the kernel through it.
template <int BM, class F>
int wgrad_tile_bm(int variant, F&& f) {
  switch (variant) {
    case 1: return f(RegTile<BM, 2, 2, 1>{});
    case 3: return f(RegTile<BM, 2, 4, 2>{});
    case 4: return f(RingTile<BM, 2>{});
    case 5: return f(RingTile<BM, 3>{});
    case 8: return f(RingTile<BM, 2, 64, 2>{});
    case 9: return f(StripTile<64>{});
    case 10: return f(StripTile<32>{});
  }
  if constexpr (BM == 128) {  // the 32-pixel K-steps are built for the 128-row tile only
    if (variant == 6) return f(RingTile<128, 4, 32>{});
    if (variant == 7) return f(RingTile<128, 3, 32>{});
  } else {
    if (variant == 6) return f(RingTile<64, 3>{});
  }
  return f(RegTile<BM, 2, 4, 1>{});
}
template <class F>
int wgrad_tile(const WgradGeom& g, int variant, F&& f) {
  return g.K <= 64 ? wgrad_tile_bm<64>(variant, f) : wgrad_tile_bm<128>(variant, f);
}

// `variant`, `splits`: as the entry points take them (-1 / <= 0: choose).
WgradPlan wgrad_plan(const WgradGeom& g, int variant, int splits) {
  WgradPlan p{};
  p.err = (int)hipErrorInvalidValue;
  if (g.N < 1 || g.H < 1 || g.W < 1 || g.C < 1 || g.K < 1 || g.R < 1 || g.S < 1 || g.st < 1 || g.pad < 0 ||
      g.H + 2 * g.pad < g.R || g.W + 2 * g.pad < g.S)
    return p;
  if (g.C % 8 || g.K % 8 || variant < -1 || variant > 10 || g.R * g.S > 49) return p;
  const long P = (long)g.N * g.Ho * g.Wo, Ntot = (long)g.R * g.S * g.C;
  if (P >= (1L << 31)) return p;  // the kernels count pixels in 32 bits
  // The default form for the stride-1 3x3 convs with K > 64 output channels (round 6): variant 8, two K-groups of 8
  // waves per workgroup (in-workgroup split-K over the pixels).  A launch of it covers the pixels of two one-group
  // splits: half the splits -- and half the fp32 slabs written and folded (~340 of the ~520 MB per step) -- for the
  // same waves per CU, so it targets half the workgroups.  The others keep the one-group ring (4): the 64-channel stem
  // / layer1 (its 48 KB blocks run three per CU, the 96 KB two-group block one: stem 78 -> 110 us standalone,
  // profiles/r06/bench_wgrad_kg.txt), and the stride-2 / 1x1 wgrads, whose slabs are small and whose kernels ran
  // 2-8 us slower each in the serialized trunk (profiles/r06/trunk_table_serial.txt).
  // Never the strip kernel: it sums in another fp32 order than the rings, and over the benchmark's 60 Adam steps that
  // rounding grows into parameter differences far beyond rounding (an element whose gradient is at rounding level
  // moves +lr or -lr), so the trunk keeps the rings' bits.
  if (variant == -1) variant = (g.K > 64 && g.st == 1 && g.R * g.S > 1) ? 8 : 4;
  p.variant = variant;
  wgrad_tile(g, variant, [&](auto t) {
    using T = decltype(t);
    p.form = T::form;
    p.BM = T::BM; p.STAGES = T::STAGES; p.KS = T::KS; p.KG = T::KG;
    p.threads = 64 * T::WM * T::WN * T::KG;
    return 0;
  });
  if (p.form == kWgradStrip) {
    // 3x3 / stride-1 / pad-1 convs on whole 64-channel chunks and whole tiles of output channels only; a dY row
    // stride, a padded pixel index and an X ring (a power of two of 64-row chunks >= 2 (W + 2) rows + the dY ring's
    // depth: W <= 126) the kernel's address arithmetic holds
    if (g.R != 3 || g.S != 3 || g.st != 1 || g.pad != 1 || g.C % 64 || g.K % p.BM || g.Creal != g.C) return p;
    const int Wp = g.W + 1, Hp = g.H + 1;
    const long TR = (long)g.N * Hp;  // image rows, each image's pad row counted
    if (g.ldy >= (1 << 24) || (TR + Hp) * Wp >= (1L << 30)) return p;
    int xc = 1;
    while (xc < (2 * (Wp + 1) + 63) / 64 + p.STAGES) xc *= 2;
    if (xc > 8) return p;
    p.xrows = xc * 64;
    // A tile spans every tap, so a split is (C / 64) * (K / tile) workgroups: one 12-wave workgroup per CU (256), and
    // at least 1024 padded pixels per split.
    const long stiles = (g.C / 64) * (g.K / p.BM);
    if (splits <= 0) splits = (int)std::max(1L, std::min(256 / stiles, TR * Wp / 1024));
    p.per_split = (int)((TR + splits - 1) / splits);
    p.slabs = (int)((TR + p.per_split - 1) / p.per_split);
    p.grid_x = (unsigned)(p.slabs * stiles);
    p.grid_z = 1;
    p.lds = ((size_t)p.xrows * 64 + (size_t)p.STAGES * 64 * p.BM) * sizeof(bf16_t);
  } else {
    const long tiles = ((g.K + p.BM - 1) / p.BM) * ((Ntot + 127) / 128);
    if (splits <= 0) {
      // Target workgroups per launch: 768, 8 waves each, 3 per CU (256 / 384 / 512 lose 3.1 / 1.3 / 0.3 % of the
      // step, 1024 loses 0.4 %).  Pixels per split, at least (tools/bench_conv.py on the ResNet18 layers, MI355X):
      // 1024 in general -- more, shorter splits lose to the fold of their partial slabs -- but 256 for the tiny 1x1
      // downsample outputs (a K loop of 16 64-pixel steps per split was the whole time: 26 -> 19 us) and 512 where the
      // output has so many tiles that 1024 leaves only 4 splits (layer4 3x3: 65 -> 58 us).  A two-K-group workgroup
      // counts as two.
      const long kg = variant == 8 ? 2 : 1;
      const long min_pix = Ntot * g.K <= 65536 ? 256 : (tiles >= 96 ? 512 : 1024);
      splits = (int)std::max(1L, std::min((768 + kg * tiles - 1) / (kg * tiles), P / (kg * min_pix)));
    }
    p.per_split = (int)(((P + splits - 1) / splits + 63) / 64 * 64);
    p.slabs = (int)((P + p.per_split - 1) / p.per_split);
    // the rings: a split-major 1-D grid over xcd_tile's XCD chunks -- the tiles of one split (same dY rows, same
    // shifted X windows) share an L2 (DESIGN.md section 4e'': layer1 / stem wgrad fetch 244 -> 67 MB per launch);
    // the register-staged kernels: splits on grid z
    p.grid_x = (unsigned)(p.form == kWgradRing ? tiles * p.slabs : tiles);
    p.grid_z = p.form == kWgradRing ? 1 : (unsigned)p.slabs;
    if (p.form == kWgradRing) {
      const size_t ring = (size_t)p.KG * p.STAGES * p.KS * (p.BM + 128) * sizeof(bf16_t);
      const size_t xchg = (size_t)(p.KG - 1) * p.BM * (128 + 4) * sizeof(float);  // the K-groups' tile exchange
      p.lds = ring > xchg ? ring : xchg;
    }
  }
  p.splits = splits;
  p.ws_floats = (long long)splits * g.K * Ntot;
  p.err = (int)hipSuccess;
  return p;
}

template <class T>
int launch_wgrad_tile(const WgradGeom& g0, const WgradPlan& p, hipStream_t st) {
  // the tile this walk of the ladder arrived at is the one the plan sized the grid and the LDS for
  if (T::form != p.form || T::BM != p.BM || T::STAGES != p.STAGES || T::KS != p.KS || T::KG != p.KG)
    return (int)hipErrorInvalidConfiguration;
  const dim3 grid(p.grid_x, 1, p.grid_z);
  if constexpr (T::form == kWgradStrip) {
    StripGeom g{};
    g.N = g0.N; g.H = g0.H; g.W = g0.W; g.C = g0.C; g.K = g0.K;
    g.X = g0.X; g.dY = g0.dY; g.ws = g0.ws; g.ldy = (int)g0.ldy;
    g.xrows = p.xrows;
    g.rows_per_split = p.per_split;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_strip_kernel<T::BM, T::STAGES>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds) != hipSuccess)
      return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((wgrad_strip_kernel<T::BM, T::STAGES>), grid, dim3(p.threads), p.lds, st, g);
  } else {
    WgradGeom g = g0;
    g.pix_per_split = p.per_split;
    if constexpr (T::form == kWgradRing) {
      g.flat = 1;
      if (hipFuncSetAttribute(
              reinterpret_cast<const void*>(&wgrad_pipe_kernel<T::BM, 128, T::WM, T::WN, T::STAGES, T::KS, T::KG>),
              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds) != hipSuccess)
        return (int)hipErrorInvalidConfiguration;
      hipLaunchKernelGGL((wgrad_pipe_kernel<T::BM, 128, T::WM, T::WN, T::STAGES, T::KS, T::KG>), grid,
                         dim3(p.threads), p.lds, st, g);
    } else {
      hipLaunchKernelGGL((wgrad_kernel<T::BM, 128, T::WM, T::WN, T::PF>), grid, dim3(p.threads), 0, st, g);
    }
  }
  return (int)hipSuccess;
}

// the only place that instantiates and launches the weight-gradient kernels
int launch_wgrad_plan(const WgradGeom& g, const WgradPlan& p, hipStream_t st) {
  if (p.err != (int)hipSuccess) return p.err;
  return wgrad_tile(g, p.variant, [&](auto t) { return launch_wgrad_tile<decltype(t)>(g, p, st); });
}

WgradGeom wgrad_geom(int N, int H, int W, int C, int Creal, int K, int R, int S, int stride, int pad, const void* x,
                     const void* dy, long ldy, float* workspace) {
  WgradGeom g{};
  g.N = N; g.H = H; g.W = W; g.C = C; g.Creal = Creal; g.K = K;
  g.R = R; g.S = S; g.st = stride; g.pad = pad;
  if (stride > 0) {
    g.Ho = (H + 2 * pad - R) / stride + 1;
    g.Wo = (W + 2 * pad - S) / stride + 1;
  }
  g.X = (const bf16_t*)x; g.dY = (const bf16_t*)dy; g.ws = workspace;
  g.ldy = ldy > 0 ? ldy : K;
  return g;
}

}  // namespace

MER_API int mer_conv_wgrad(int N, int H, int W, int C, int Creal, int K, int R, int S, int stride, int pad,
                           const void* x, const void* dy, float* dw, int splits, float* workspace, void* stream) {
  return mer_conv_wgrad_ex(N, H, W, C, Creal, K, R, S, stride, pad, x, dy, dw, splits, workspace, -1, stream);
}

static int conv_wgrad_impl(int N, int H, int W, int C, int Creal, int K, int R, int S, int stride, int pad,
                           const void* x, const void* dy, long ldy, float* dw, int splits, float* workspace,
                           int variant, void* stream, bool fold = true) {
  const WgradGeom g = wgrad_geom(N, H, W, C, Creal, K, R, S, stride, pad, x, dy, ldy, workspace);
  const WgradPlan p = wgrad_plan(g, variant, splits);
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_wgrad_plan(g, p, st);  // a refused plan or launch (LDS size): nothing is folded then
  if (rc != (int)hipSuccess) return rc;
  if (!fold) MER_LAUNCH_CHECK();  // partial slabs left for mer_wgrad_fold_batch
  constexpr int fold_max = 16;  // most slabs folded in the single fold+scatter pass
  if (p.slabs > fold_max) {  // many partial slabs: a wide reduce first (one serial chain per element was latency-bound)
    const int SG = p.slabs >= 64 ? 16 : 8;
    const long total = (long)K * R * S * C;
    const int E = 256 / SG;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + E - 1) / E)), dim3(256), 0, st, K, C, Creal, R * S,
                       p.slabs, SG, workspace);
    hipLaunchKernelGGL(wgrad_scatter_kernel, dim3((Creal + 31) / 32, K), dim3(256), 0, st, C, Creal, R * S, workspace,
                       dw);
  } else {  // few slabs: fold and scatter in one pass
    hipLaunchKernelGGL(wgrad_fold_scatter_kernel, dim3((Creal + 31) / 32, K), dim3(256), 0, st, K, C, Creal, R * S,
                       p.slabs, workspace, dw);
  }
  MER_LAUNCH_CHECK();
}

MER_API int mer_conv_wgrad_plan(int N, int H, int W, int C, int Creal, int K, int R, int S, int stride, int pad,
                                int variant, int splits, long long* out) {
  const WgradPlan p = wgrad_plan(wgrad_geom(N, H, W, C, Creal, K, R, S, stride, pad, nullptr, nullptr, K, nullptr),
                                 variant, splits);
  if (p.err != (int)hipSuccess) return p.err;
  out[0] = p.variant; out[1] = p.splits; out[2] = p.slabs; out[3] = p.ws_floats;
  return (int)hipSuccess;
}

MER_API int mer_conv_wgrad_ex(int N, int H, int W, int C, int Creal, int K, int R, int S, int stride, int pad,
                              const void* x, const void* dy, float* dw, int splits, float* workspace, int variant,
                              void* stream) {
  return conv_wgrad_impl(N, H, W, C, Creal, K, R, S, stride, pad, x, dy, K, dw, splits, workspace, variant, stream);
}

MER_API int mer_conv_wgrad_partials(int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                                    const void* x, const void* dy, int splits, float* workspace, int variant,
                                    void* stream) {
  return conv_wgrad_impl(N, H, W, C, C, K, R, S, stride, pad, x, dy, K, nullptr, splits, workspace, variant, stream,
                         false);
}

static int fold_sg_max() { return 8; }  // split groups per block for many-slab records

// rows: n x 8 int64 {ws, dw, map, K, C, Creal (map records: output floats per k), R*S, splits}
MER_API int mer_wgrad_fold_batch(int n, const long long* rows, void* stream) {
  if (n < 1 || n > kFoldMaxRecs) return (int)hipErrorInvalidValue;
  FoldTable t{};
  t.n = n;
  int blk = 0;
  for (int i = 0; i < n; ++i) {
    const long long* q = rows + 8 * i;
    FoldRec& r = t.r[i];
    r.ws = (const float*)q[0]; r.dw = (float*)q[1]; r.map = (const int*)q[2];
    r.K = (int)q[3]; r.C = (int)q[4]; r.Creal = (int)q[5]; r.RS = (int)q[6]; r.splits = (int)q[7];
    if (!r.ws || !r.dw || r.K < 1 || r.C < 1 || r.C % 4 || r.RS < 1 || r.splits < 1 || r.Creal < 1 ||
        (!r.map && r.Creal > r.C) || ((uintptr_t)r.ws & 15))
      return (int)hipErrorInvalidValue;
    // SG <= 8: E >= 32 consecutive floats per split group, i.e. whole 128-byte lines (SG 16 read half lines: the
    // slabs are cold by the time the segment folds, so half-used lines cost HBM bytes)
    r.SG = r.splits > 48 ? fold_sg_max() : (r.splits > 12 ? 4 : 1);
    const long total = (long)r.K * r.RS * r.C;
    r.blk0 = blk;
    if (r.map) {  // source order: E = 256/SG threads of 4 floats per block
      r.nblk = (int)((total + 4 * (256 / r.SG) - 1) / (4 * (256 / r.SG)));
    } else {
      // a 1x1 record's slab and dw are the same flat [K*C] order: fold it as rows of 1024 channels (a 64-channel row
      // alone would leave most of a block idle)
      if (r.RS == 1 && r.Creal == r.C && r.C < 1024 && total % 1024 == 0) {
        r.K = (int)(total / 1024);
        r.C = r.Creal = 1024;
      }
      // channels per block: the whole row for the few-slab records (SG = 1: several 16-byte elements and all their
      // slabs in flight per thread); for the many-slab ones the smallest multiple of 32 (whole 128-byte lines) that
      // gives each thread of a split group an element -- short rows cut into many blocks
      const int E = 256 / r.SG, cr4 = (r.Creal + 3) & ~3;
      int cap = (kFoldTile / (r.SG * r.RS) - 4) & ~3;
      if (r.SG > 1) cap = std::min(cap, (kFoldRunSG / r.RS) & ~3);
      if (cap < 4) return (int)hipErrorInvalidValue;
      int cc = cr4;
      if (r.SG > 1)
        for (cc = 32; r.RS * cc / 4 < E && cc < cr4;) cc *= 2;
      cc = std::min(std::min(cc, cr4), cap);
      if (cc > 32) cc &= ~31;
      r.CC = cc;
      r.chunks = (cr4 + cc - 1) / cc;
      r.nblk = r.K * r.chunks;
    }
    blk += r.nblk;
  }
  hipLaunchKernelGGL(wgrad_fold_batch_kernel, dim3(blk), dim3(256), 0, (hipStream_t)stream, t);
  MER_LAUNCH_CHECK();
}

// Linear weight gradient as a 1x1 convolution over M "pixels": dw[n][k] += sum_m dy[m][n] x[m][k].
MER_API int mer_linear_wgrad(int M, int N, int K, const void* x, const void* dy, long ldy, float* dw, int splits,
                             float* workspace, void* stream) {
  if (ldy < N || ldy % 8) return (int)hipErrorInvalidValue;
  return conv_wgrad_impl(1, 1, M, K, K, N, 1, 1, 1, 0, x, dy, ldy, dw, splits, workspace, -1, stream);
}
