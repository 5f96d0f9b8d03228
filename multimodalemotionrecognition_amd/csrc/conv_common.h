// Shared by the ResNet18 trunk's convolution units: conv.hip (forward / input gradient) and conv_wgrad.hip (weight
// gradient).
#pragma once
#include <type_traits>

#include "common.h"
#include "mer.h"

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;

// Phase timestamps (tools/halo_phases.py builds a separate library with -DMER_CONV_TIMING; the production library
// compiles every stamp to nothing).  A unit declares its stamp buffers with MER_CT_BUFFER(name, words), which also
// defines the name_reset() / name_read(host) accessors the tools call, and stamps them through CT_AT / CTP_AT.
#ifdef MER_CONV_TIMING
#define MER_CT_BUFFER(name, words) \
  static __device__ long long name##_buf[words]; \
  MER_API int name##_reset() { \
    static long long zeros[words]; \
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(name##_buf), zeros, sizeof(zeros), 0, hipMemcpyHostToDevice); \
  } \
  MER_API int name##_read(long long* host) { \
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(name##_buf), sizeof(long long) * (words), 0, \
                                    hipMemcpyDeviceToHost); \
  }
// a mode word the host sets through name(mode) and kernels read as name_v
#define MER_CT_MODE_WORD(name) \
  static __device__ int name##_v; \
  MER_API int name(int mode) { \
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(name##_v), &mode, sizeof(int), 0, hipMemcpyHostToDevice); \
  }
// buf[512 * 64]: wall_clock64() of workgroup blockIdx.x's thread 0 at slot k
#define CT_AT(buf, k) \
  do { \
    if (threadIdx.x == 0 && blockIdx.x < 512 && (k) < 64) buf[blockIdx.x * 64 + (k)] = wall_clock64(); \
  } while (0)
// buf[4096 * 8]: slot k of the linear block id (blockIdx.y * gridDim.x + blockIdx.x)
#define CTP_AT(buf, k) \
  do { \
    const unsigned b_ = blockIdx.y * gridDim.x + blockIdx.x; \
    if (threadIdx.x == 0 && b_ < 4096) buf[b_ * 8 + (k)] = wall_clock64(); \
  } while (0)
#else
#define MER_CT_BUFFER(name, words)
#define MER_CT_MODE_WORD(name)
#define CT_AT(buf, k) \
  do { \
  } while (0)
#define CTP_AT(buf, k) \
  do { \
  } while (0)
#endif

namespace {

constexpr int CBK = 64;  // K step

struct ConvGeom {
  int N, OH, OW;          // GEMM output spatial dims (fwd: Ho,Wo; dgrad: H,W)
  int IH, IW, IC;         // A-source spatial dims / channels (fwd: H,W,C; dgrad: Ho,Wo,K)
  int R, S, st, pad;
  int Ncols;              // GEMM N (fwd: Cout; dgrad: Cin)
  int Kred;               // R*S*IC
  const bf16_t* X;        // A source
  const bf16_t* Wt;       // [Ncols][Kred]
  bf16_t* Y;              // [M][ldy]
  long ldy;
  float* stats;           // fwd: per column (sum, sumsq), may be null
  const bf16_t* R_;       // residual added in the epilogue (dgrad), may be null
  const bf16_t* Rmask;    // residual is added only where Rmask > 0 (relu mask), may be null
  // dgrad only: the BatchNorm-backward reduction of the BN whose relu'd output this gradient flows
  // into, fused into the epilogue (bn_bwd_reduce semantics; NULL bnr_red = off).  g = (mask > 0) * y,
  // red[p][c] += (sum g, sum g * (x - mean) * rstd); red2 likewise for a second BN reading the same g
  // (the downsample branch).  One stored row per output row tile (MER_BN_RED_ROWS), like the forward statistics.
  const bf16_t* bnr_mask;
  const bf16_t* bnr_x;
  const float* bnr_ms;
  float* bnr_red;
  const bf16_t* bnr_x2;
  const float* bnr_ms2;
  float* bnr_red2;
  int vec;                // 16-byte epilogue (Ncols, ldy multiples of 8, every operand 16-byte aligned)
  // stride-2 dgrad only: a 1x1 / stride-2 / pad-0 downsample of the same input fused as an extra K segment of parity
  // class (0, 0) -- the only class its taps reach: dx[2i, 2j] += sum_k dY2[i, j, k] W2t[c][k] (NULL X2 = off)
  const bf16_t* X2;       // [N][IH][IW][K2], the downsample branch's output gradient
  const bf16_t* Wt2;      // [Ncols][K2]
  int K2;
};

__host__ __device__ inline bool conv_vec_ok(const ConvGeom& g) {
  const uintptr_t a = (uintptr_t)g.Y | (uintptr_t)g.R_ | (uintptr_t)g.Rmask | (uintptr_t)g.bnr_mask |
                      (uintptr_t)g.bnr_x | (uintptr_t)g.bnr_x2 | (uintptr_t)g.stats | (uintptr_t)g.bnr_red |
                      (uintptr_t)g.bnr_red2;
  return g.Ncols % 8 == 0 && g.ldy % 8 == 0 && (a & 15) == 0;
}

// the 16-byte zero chunk the LDS-DMA kernels point a lane at for padding (static: the library is built without
// relocatable device code, so each unit carries its own)
static __device__ __attribute__((aligned(16))) uint32_t mer_conv_zero16[4] = {0u, 0u, 0u, 0u};

int cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                hipSuccess || v <= 0)
      return 256;
    return v;
  }();
  return n;
}

}  // namespace
