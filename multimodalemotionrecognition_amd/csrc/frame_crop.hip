// Ragged crop-and-resize (clips.crop_resize_frames): output frame n is the preprocessing of csrc/clips.hip applied to
// one rectangle of one image, both named by row n of a device descriptor table -- the face-box crop of
// face_crop.py:151-190 (crop_with_padding) followed by ravdess.py:352 cv2.resize, without the cropped copy.
//   frames: one byte buffer of tightly packed RGB uint8 images [H0][W0][3] of differing sizes
//   desc:   int64 [n_out][8] = {byte offset of the image, H0, W0, x1, y1, x2, y2, 0}; the rectangle is half-open,
//           frame[y1:y2, x1:x2], already padded and clipped on the host
// Output n has the bits the existing kernels give for the contiguous copy of that rectangle: the scales and the tap
// clamps come from the rectangle's width and height, the 2x INTER_AREA path is taken when the RECTANGLE is 2S x 2S,
// and rows are W0 * 3 bytes apart whatever the rectangle's width (frame_resize.h, one definition of the arithmetic).
//
// Work split: one workgroup makes a tile of up to 256 columns x 16 rows of one output frame.  The scales differ per
// frame, so the tile's tap records (two fp64 multiplies, a floor and two roundings each) are computed once per
// workgroup into LDS -- one column tap per thread, 16 row taps -- instead of twice per output pixel; the pixels then
// cost integer arithmetic and four byte-triple loads.  Threads run along x first, so the fp32 planes and the uint8
// rows are stored coalesced.  HBM- and latency-bound.
// The Python wrapper validates every row on the host; the kernel clamps image and rectangle into the buffer as well, so
// no launch reads outside frames whatever the table holds.
#include "common.h"
#include "frame_resize.h"
#include "mer.h"

namespace {

constexpr int TILE_W = 256, TILE_H = 16;
constexpr long MAX_SIDE = 1L << 24;  // keeps W0 * 3 and every tap offset inside an int

struct CropRect {
  const uint8_t* f;  // the rectangle's first pixel
  long pitch;        // bytes between rows: the image's W0 * 3
  int h, w;
};

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Row n of the table, forced into the buffer: an image that does not fit becomes the buffer's first pixel, an offset
// is moved so that the image ends inside, a rectangle is cut to the image and keeps at least one pixel.
__device__ __forceinline__ CropRect load_rect(const uint8_t* __restrict__ frames, long nbytes,
                                              const long* __restrict__ desc, long n) {
  const long* d = desc + n * 8;
  long H0 = clampl(d[1], 1, MAX_SIDE), W0 = clampl(d[2], 1, MAX_SIDE);
  if (H0 * W0 * 3 > nbytes) H0 = W0 = 1;  // (nbytes >= 3: checked by the entry point)
  const long off = clampl(d[0], 0, nbytes - H0 * W0 * 3);
  const long x1 = clampl(d[3], 0, W0 - 1), y1 = clampl(d[4], 0, H0 - 1);
  const long x2 = clampl(d[5], x1 + 1, W0), y2 = clampl(d[6], y1 + 1, H0);
  CropRect r;
  r.pitch = W0 * 3;
  r.f = crop_origin(frames + off, r.pitch, (int)x1, (int)y1);
  r.h = (int)(y2 - y1);
  r.w = (int)(x2 - x1);
  return r;
}

template <bool U8>
__global__ __launch_bounds__(256) void frames_crop_resize_kernel(const uint8_t* __restrict__ frames, long nbytes,
                                                                 const long* __restrict__ desc, long n0, int S,
                                                                 FrameNorm nm, void* __restrict__ dst) {
  __shared__ LinTap tap_x[TILE_W];
  __shared__ LinTap tap_y[TILE_H];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
  const long n = n0 + blockIdx.z;
  const int tw = min(TILE_W, S - x0), th = min(TILE_H, S - y0);
  const CropRect r = load_rect(frames, nbytes, desc, n);
  const bool area = r.h == 2 * S && r.w == 2 * S;
  if (!area) {  // (uniform over the workgroup: every thread read the same row)
    if (tid < tw) tap_x[tid] = lin_tap(x0 + tid, r.w, 1.0 / ((double)S / r.w));  // cv::resize: 1 / inv_scale
    if (tid >= TILE_W - th) {  // the last th threads: with tw < 256 they are otherwise idle here
      const int j = tid - (TILE_W - th);
      tap_y[j] = lin_tap(y0 + j, r.h, 1.0 / ((double)S / r.h));
    }
    __syncthreads();
  }
  // pixel p = tid, tid + 256, ... of the tile in row-major order, walked without a division per step
  const int dy = TILE_W / tw, dx = TILE_W - dy * tw;
  int yl = tid / tw, xl = tid - yl * tw;
  for (; yl < th; yl += dy) {
    int v[3];
    if (area)
      area2x_pixel(r.f, r.pitch, x0 + xl, y0 + yl, v);
    else
      linear_pixel(r.f, r.pitch, tap_x[xl], tap_y[yl], v);
    if (U8)
      store_u8(v, S, x0 + xl, y0 + yl, n, (uint8_t*)dst);
    else
      store_normalized(v, S, x0 + xl, y0 + yl, n, nm, (float*)dst);
    xl += dx;
    if (xl >= tw) {
      xl -= tw;
      ++yl;
    }
  }
}

}  // namespace

MER_API int mer_frames_crop_resize(const void* frames, long frames_bytes, int n_out, const long* desc, int S, int mode,
                                   float mean0, float mean1, float mean2, float std0, float std1, float std2, void* out,
                                   void* stream) {
  if (!frames || !desc || !out || S < 1 || n_out < 0 || frames_bytes < 3 || (mode != 0 && mode != 1))
    return (int)hipErrorInvalidValue;
  const long bands = ((long)S + TILE_H - 1) / TILE_H;
  if (bands > 65535) return (int)hipErrorInvalidValue;  // grid y
  if (n_out == 0) return 0;
  const FrameNorm nm{mean0, mean1, mean2, std0, std1, std2};
  const dim3 block(256);
  for (int n0 = 0; n0 < n_out; n0 += 65535) {  // grid z holds at most 65535 frames: one launch up to there
    const int nz = n_out - n0 < 65535 ? n_out - n0 : 65535;
    const dim3 grid((S + TILE_W - 1) / TILE_W, (unsigned)bands, nz);
    if (mode == 1)
      hipLaunchKernelGGL(frames_crop_resize_kernel<true>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)frames,
                         frames_bytes, desc, (long)n0, S, nm, out);
    else
      hipLaunchKernelGGL(frames_crop_resize_kernel<false>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)frames,
                         frames_bytes, desc, (long)n0, S, nm, out);
  }
  MER_LAUNCH_CHECK();
}
