// Log-mel front end of the mel audio path (ravdess.py:478-485): MelSpectrogram(sample_rate=16000, n_fft=400,
// win_length=400, hop_length=160, n_mels) + AmplitudeToDB(), fused in one kernel.
//
// A workgroup takes ML_TT = 32 time steps of one clip.  Its reflect-padded frames (raw samples; the periodic Hann
// window is folded into the DFT tables) are staged in LDS as a [32][400] matrix.  The DFT is two matrix products
// against the window-folded cos / sin tables ([400][208] fp32 each, built once on the host in fp64 and rounded; 665 KB,
// L2-resident) on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32): the four waves split the 13 column tiles of the 201
// (padded to 208) bins, and each table operand read feeds both 16-step row tiles.  The 400-term sums run as four
// chains of 100 terms added in order (a shorter fma chain, a smaller rounding error; the order is fixed).  The power
// re^2 + im^2 goes through LDS as [bin][t] into the mel product mel^T[m][t] = sum_f fb[f][m] P[f][t] of the same
// workgroup, so the accumulator's lane axis is t and the [n_mels][T] store is contiguous along T.  No atomics;
// every sum has a fixed order, results are bitwise repeatable.
// Partial tiles: time steps >= T are zero frames (not stored), table columns >= 201 and filterbank columns >= n_mels
// are zero padding (not stored).
#include "common.h"
#include "mer.h"

constexpr int ML_NFFT = 400, ML_HOP = 160, ML_PADL = 200, ML_BINS = 201;
constexpr int ML_FP = 208;                 // bins padded to 13 column tiles of 16
constexpr int ML_TT = 32;                  // time steps per workgroup
constexpr int ML_LDF = ML_NFFT + 1;        // frame row stride: 401 = 17 mod 32, the 16 rows of an operand read hit 16 banks
constexpr int ML_LDP = ML_TT + 4;          // power row stride (16-byte aligned rows)
constexpr int ML_KCH = 100;                // terms per fma chain
static_assert(ML_BINS == ML_NFFT / 2 + 1 && ML_BINS <= ML_FP && ML_FP % 16 == 0 && ML_NFFT % ML_KCH == 0, "tiling");

__global__ __launch_bounds__(256) void log_mel_kernel(int S, int T, int tiles_t, int n_mels, int nmp,
                                                      const float* __restrict__ wav, long wav_stride,
                                                      const float* __restrict__ ctab, const float* __restrict__ stab,
                                                      const float* __restrict__ fb, int to_db,
                                                      float* __restrict__ out) {
  // the frames, then (once every wave is through its DFT) the power image [208][ML_LDP] in the same LDS
  __shared__ __attribute__((aligned(16))) float Fs[ML_TT * ML_LDF];
  static_assert(ML_FP * ML_LDP <= ML_TT * ML_LDF, "the power image reuses the frame buffer");
  float* Ps = Fs;
  const int b = blockIdx.x / tiles_t, t0 = (blockIdx.x - b * tiles_t) * ML_TT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* x = wav + (long)b * wav_stride;

  // frames: Fs[t][n] = x[reflect(( t0 + t) * hop + n - 200)], zero rows past T
  for (int e = tid; e < ML_TT * ML_NFFT; e += 256) {
    const int t = e / ML_NFFT, n = e - t * ML_NFFT;
    float v = 0.f;
    if (t0 + t < T) {
      int s = (t0 + t) * ML_HOP + n - ML_PADL;
      if (s < 0) s = -s;
      if (s >= S) s = 2 * (S - 1) - s;  // S >= 201 (checked on the host): 0 <= s < S after one reflection
      v = x[s];
    }
    Fs[t * ML_LDF + n] = v;
  }
  __syncthreads();

  const int lr = lane & 15, lk = lane >> 4;
  f32x4 pw[4][2];  // this wave's column tiles w, w + 4, w + 8 (, 12): power, kept in registers until the frames are done
#pragma unroll
  for (int fi = 0; fi < 4; ++fi) {
    const int f0 = (w + 4 * fi) * 16;
    if (f0 >= ML_FP) break;  // wave-uniform
    f32x4 re[2], im[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) re[i] = im[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < ML_NFFT; kc += ML_KCH) {
      f32x4 cre[2], cim[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) cre[i] = cim[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
      for (int k0 = kc; k0 < kc + ML_KCH; k0 += 4) {
        const int k = k0 + lk;
        const float a0 = Fs[lr * ML_LDF + k], a1 = Fs[(16 + lr) * ML_LDF + k];
        const float bc = ctab[k * ML_FP + f0 + lr], bs = stab[k * ML_FP + f0 + lr];
        cre[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bc, cre[0], 0, 0, 0);
        cim[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bs, cim[0], 0, 0, 0);
        cre[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bc, cre[1], 0, 0, 0);
        cim[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bs, cim[1], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          re[i][r] += cre[i][r];
          im[i][r] += cim[i][r];
        }
    }
    // accumulator: row (t) = lk * 4 + r, column (bin) = lr  ->  Ps[bin][t], four consecutive t per lane
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f32x4 p;
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = re[i][r] * re[i][r] + im[i][r] * im[i][r];
      pw[fi][i] = p;
    }
  }
  __syncthreads();
#pragma unroll
  for (int fi = 0; fi < 4; ++fi) {
    const int f0 = (w + 4 * fi) * 16;
    if (f0 >= ML_FP) break;
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(&Ps[(f0 + lr) * ML_LDP + i * 16 + lk * 4]) = pw[fi][i];
  }
  __syncthreads();

  // mel^T[m][t] = sum_f fb[f][m] * P[f][t]: A = fb^T (lane: m = lr, f = k), B = P (lane: f = k, t = lr)
  const int tiles = (nmp / 16) * 2;
  for (int tile = w; tile < tiles; tile += 4) {
    const int m0 = (tile >> 1) * 16, tt = (tile & 1) * 16;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k0 = 0; k0 < ML_FP; k0 += 4) {
      const int k = k0 + lk;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[k * nmp + m0 + lr], Ps[k * ML_LDP + tt + lr], acc, 0, 0, 0);
    }
    const int t = t0 + tt + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + lk * 4 + r;
      if (m < n_mels && t < T) {
        float v = acc[r];
        if (to_db) v = 10.0f * log10f(fmaxf(v, 1e-10f));
        out[((long)b * n_mels + m) * T + t] = v;
      }
    }
  }
}

MER_API int mer_log_mel(int B, int S, int n_mels, const float* wav, long wav_stride, const float* ctab,
                        const float* stab, const float* fb, int to_db, float* out, void* stream) {
  if (B <= 0) return 0;
  if (S <= ML_PADL || n_mels < 1 || n_mels > 128 || wav_stride < S || !wav || !ctab || !stab || !fb || !out)
    return (int)hipErrorInvalidValue;
  const int T = 1 + S / ML_HOP, nmp = (n_mels + 15) / 16 * 16;
  const int tiles_t = (T + ML_TT - 1) / ML_TT;
  if ((long)tiles_t * B > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(log_mel_kernel, dim3(tiles_t * B), dim3(256), 0, (hipStream_t)stream, S, T, tiles_t, n_mels, nmp,
                     wav, wav_stride, ctab, stab, fb, to_db, out);
  MER_LAUNCH_CHECK();
}
