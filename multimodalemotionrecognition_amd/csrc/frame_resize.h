// One output pixel of the post-decode frame preprocessing (ravdess.py:352 cv2.resize INTER_LINEAR, :363 /255,
// :386-389 ImageNet normalisation + HWC->CHW), shared by csrc/clips.hip (frames in batch order) and
// csrc/timeline.hip (frames picked out of a recording by index) and csrc/frame_crop.hip (a rectangle of each of a
// ragged set of images): one definition, so all of them round alike.
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

// The rectangle a resize reads: H x W pixels whose row r starts at f + r * pitch bytes.  A stand-alone frame has
// pitch = W * 3; a crop of a larger frame keeps the frame's pitch and points f at the crop's first pixel
// (crop_origin), so a crop and its contiguous copy go through the same arithmetic.
__device__ __forceinline__ const uint8_t* crop_origin(const uint8_t* frame, long pitch, int ox, int oy) {
  return frame + (long)oy * pitch + (long)ox * 3;
}

// INTER_AREA fast path for an exact 2x downscale: the 2x2 average of output pixel (x, y)
__device__ __forceinline__ void area2x_pixel(const uint8_t* f, long pitch, int x, int y, int v[3]) {
  const uint8_t* p0 = f + (long)(2 * y) * pitch + (long)(2 * x) * 3;
  const uint8_t* p1 = p0 + pitch;
  for (int c = 0; c < 3; ++c) v[c] = (p0[c] + p0[3 + c] + p1[c] + p1[3 + c] + 2) >> 2;
}

// INTER_LINEAR output pixel from its two tap records (lin_tap of the rectangle's own width / height)
__device__ __forceinline__ void linear_pixel(const uint8_t* f, long pitch, LinTap tx, LinTap ty, int v[3]) {
  const uint8_t* r0 = f + (long)ty.s0 * pitch;
  const uint8_t* r1 = f + (long)ty.s1 * pitch;
  for (int c = 0; c < 3; ++c) {
    const int h0 = r0[tx.s0 * 3 + c] * tx.a0 + r0[tx.s1 * 3 + c] * tx.a1;
    const int h1 = r1[tx.s0 * 3 + c] * tx.a0 + r1[tx.s1 * 3 + c] * tx.a1;
    const int w = (h0 * ty.a0 + h1 * ty.a1 + (1 << 21)) >> 22;
    v[c] = w < 0 ? 0 : (w > 255 ? 255 : w);
  }
}

// cv2.resize(rect, (S, S), INTER_LINEAR) of one output pixel's 3 channels (uint8 values); rect = the H0 x W0 pixels
// at f with rows pitch bytes apart
__device__ __forceinline__ void resize_pixel(const uint8_t* f, long pitch, int H0, int W0, int S, int x, int y,
                                             double scale_y, double scale_x, int v[3]) {
  if (H0 == 2 * S && W0 == 2 * S)
    area2x_pixel(f, pitch, x, y, v);
  else
    linear_pixel(f, pitch, lin_tap(x, W0, scale_x), lin_tap(y, H0, scale_y), v);
}

struct FrameNorm {
  float m0, m1, m2, sd0, sd1, sd2;
};

// Three uint8 values of pixel (x, y) normalised into output frame n of dst fp32 [N][3][S][S]:
// (x / 255 - mean) / std in fp32 with the reference's operation order (numpy float32, ravdess.py:363,388)
__device__ __forceinline__ void store_normalized(const int v[3], int S, int x, int y, long n, FrameNorm nm,
                                                 float* __restrict__ dst) {
  const long plane = (long)S * S, o = n * 3 * plane + (long)y * S + x;
  dst[o] = ((float)v[0] / 255.f - nm.m0) / nm.sd0;
  dst[o + plane] = ((float)v[1] / 255.f - nm.m1) / nm.sd1;
  dst[o + 2 * plane] = ((float)v[2] / 255.f - nm.m2) / nm.sd2;
}

__device__ __forceinline__ void store_u8(const int v[3], int S, int x, int y, long n, uint8_t* __restrict__ dst) {
  uint8_t* o = dst + ((n * S + y) * S + x) * 3;
  o[0] = (uint8_t)v[0];
  o[1] = (uint8_t)v[1];
  o[2] = (uint8_t)v[2];
}

// Pixel (x, y) of the rectangle at f, resized and normalised, into output frame n
__device__ __forceinline__ void resize_normalize_pixel(const uint8_t* f, long pitch, int H0, int W0, int S, int x,
                                                       int y, int n, double scale_y, double scale_x, FrameNorm nm,
                                                       float* __restrict__ dst) {
  int v[3];
  resize_pixel(f, pitch, H0, W0, S, x, y, scale_y, scale_x, v);
  store_normalized(v, S, x, y, n, nm, dst);
}
