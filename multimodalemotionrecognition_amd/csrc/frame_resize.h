// One output pixel of the post-decode frame preprocessing (ravdess.py:352 cv2.resize INTER_LINEAR, :363 /255,
// :386-389 ImageNet normalisation + HWC->CHW), shared by csrc/clips.hip (frames in batch order) and
// csrc/timeline.hip (frames picked out of a recording by index): one definition, so both round alike.
//
// Resize follows OpenCV's scalar fixed-point INTER_LINEAR path: per output index the source index and two
// 11-bit weights (rounded to nearest even), an int horizontal pass, an int vertical pass rounded with
// (v + 2^21) >> 22 and saturated to uint8; an exact 2x downscale is OpenCV's INTER_AREA 2x2 average.
// Integer arithmetic end to end until the fp32 normalisation, so results are bit-exact against
// oracle/clips_ref.py.
#pragma once
#include "common.h"

struct LinTap {
  int s0, s1, a0, a1;
};

// OpenCV's coefficient table entry for destination index d (resize.cpp, INTER_LINEAR, ksize 2)
__device__ __forceinline__ LinTap lin_tap(int d, int src, double scale) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= src - 1) { f = 0.f; s = src - 1; }
  LinTap t;
  t.s0 = s;
  t.s1 = min(s + 1, src - 1);
  t.a0 = __float2int_rn((1.f - f) * 2048.f);
  t.a1 = __float2int_rn(f * 2048.f);
  return t;
}

// cv2.resize(frame, (S, S), INTER_LINEAR) of one output pixel's 3 channels (uint8 values)
__device__ __forceinline__ void resize_pixel(const uint8_t* f, int H0, int W0, int S, int x, int y, double scale_y,
                                             double scale_x, int v[3]) {
  if (H0 == 2 * S && W0 == 2 * S) {  // INTER_AREA fast path for an exact 2x downscale
    const uint8_t* p0 = f + ((long)(2 * y) * W0 + 2 * x) * 3;
    const uint8_t* p1 = p0 + (long)W0 * 3;
    for (int c = 0; c < 3; ++c) v[c] = (p0[c] + p0[3 + c] + p1[c] + p1[3 + c] + 2) >> 2;
  } else {
    const LinTap tx = lin_tap(x, W0, scale_x), ty = lin_tap(y, H0, scale_y);
    const uint8_t* r0 = f + (long)ty.s0 * W0 * 3;
    const uint8_t* r1 = f + (long)ty.s1 * W0 * 3;
    for (int c = 0; c < 3; ++c) {
      const int h0 = r0[tx.s0 * 3 + c] * tx.a0 + r0[tx.s1 * 3 + c] * tx.a1;
      const int h1 = r1[tx.s0 * 3 + c] * tx.a0 + r1[tx.s1 * 3 + c] * tx.a1;
      const int w = (h0 * ty.a0 + h1 * ty.a1 + (1 << 21)) >> 22;
      v[c] = w < 0 ? 0 : (w > 255 ? 255 : w);
    }
  }
}

struct FrameNorm {
  float m0, m1, m2, sd0, sd1, sd2;
};

// Pixel (x, y) of source frame f, resized and normalised, into output frame n of dst fp32 [N][3][S][S]:
// (x / 255 - mean) / std in fp32 with the reference's operation order (numpy float32, ravdess.py:363,388)
__device__ __forceinline__ void resize_normalize_pixel(const uint8_t* f, int H0, int W0, int S, int x, int y, int n,
                                                       double scale_y, double scale_x, FrameNorm nm,
                                                       float* __restrict__ dst) {
  int v[3];
  resize_pixel(f, H0, W0, S, x, y, scale_y, scale_x, v);
  const long plane = (long)S * S, o = (long)n * 3 * plane + (long)y * S + x;
  dst[o] = ((float)v[0] / 255.f - nm.m0) / nm.sd0;
  dst[o + plane] = ((float)v[1] / 255.f - nm.m1) / nm.sd1;
  dst[o + 2 * plane] = ((float)v[2] / 255.f - nm.m2) / nm.sd2;
}
