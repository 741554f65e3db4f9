// GridMask of a training batch on the device (efficientdet/aug/gridmask.py:22-136): uint8 NHWC images [B, H, W, 3] ->
// uint8 [B, H, W, 3], never in place.  The reference builds an S x S int32 mask of stripes (:66-104), rotates it with TFA's
// bilinear projective transform (:50-55), crops its centre (:58-63) and multiplies (:117).  Nothing of that is materialised
// here: every output pixel evaluates the four taps of its own source position from the stripe formula.
//
//   mask[r][c] = stripe(r; s1) | stripe(c; s2),  stripe(t; s) = 1 iff 0 <= t < S, q = t - s >= 0, q / d < S / d, q % d < l
//
// 1 means KEPT, as the reference is written (fill = 1): the image survives on the cross-hatch and is zeroed in the holes.
// The draws and the six coefficients are the caller's, in device memory (edet_gridmask_image_t), so the launch never
// depends on them and a replayed graph sees new ones.
//
// Every result is compared bit for bit with a numpy restatement that does materialise (tests/gridmask_ref.py), so the
// arithmetic is part of the interface: this file is compiled with -ffp-contract=off (automl_amd/build.py), every product
// and sum below is a single rounded fp32 operation in the order written, and the blend is truncated to int32.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_SIDE = 1 << 30;      // S is clamped to it: S - H cannot overflow

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct Mask {
  int apply, S, d, l, s1, s2, lim, oy, ox;      // lim = d (S / d): the stripes start below it; (oy, ox): the crop's corner
  float c0, c1, c2, c3, c4, c5;
};

__device__ __forceinline__ int stripe(const Mask& m, int t, int s) {
  const int q = t - s;
  if (t < 0 || t >= m.S || q < 0 || q >= m.lim) return 0;
  return (int)((unsigned)q % (unsigned)m.d) < m.l;
}

// mask value at output pixel (x, y) of the image: ImageProjectiveTransformV2, BILINEAR, constant fill 0, on int32
__device__ __forceinline__ int mask_at(const Mask& m, int x, int y) {
  const float X = (float)(x + m.ox), Y = (float)(y + m.oy);
  const float sx = (m.c0 * X + m.c1 * Y) + m.c2;
  const float sy = (m.c3 * X + m.c4 * Y) + m.c5;
  // NaN, infinities and everything whose four taps all lie outside the mask: 0 (tested before any conversion)
  const float side = (float)m.S;
  if (!(sx > -1.f && sx < side && sy > -1.f && sy < side)) return 0;
  const float xf = floorf(sx), yf = floorf(sy);
  const float xc = xf + 1.f, yc = yf + 1.f;
  const int x0 = (int)xf, y0 = (int)yf;
  const int r0 = stripe(m, y0, m.s1), r1 = stripe(m, y0 + 1, m.s1);
  const int q0 = stripe(m, x0, m.s2), q1 = stripe(m, x0 + 1, m.s2);
  const bool in_x0 = x0 >= 0 && x0 < m.S, in_x1 = x0 + 1 >= 0 && x0 + 1 < m.S;
  const bool in_y0 = y0 >= 0 && y0 < m.S, in_y1 = y0 + 1 >= 0 && y0 + 1 < m.S;
  const float v00 = (float)((in_y0 && in_x0) ? (r0 | q0) : 0), v01 = (float)((in_y0 && in_x1) ? (r0 | q1) : 0);
  const float v10 = (float)((in_y1 && in_x0) ? (r1 | q0) : 0), v11 = (float)((in_y1 && in_x1) ? (r1 | q1) : 0);
  const float top = (xc - sx) * v00 + (sx - xf) * v01;
  const float bot = (xc - sx) * v10 + (sx - xf) * v11;
  return (int)((yc - sy) * top + (sy - yf) * bot);
}

// blockIdx.y = the image (the apply bit is uniform over a workgroup).  Dense batch (CANVAS = false): the image is h x w and its
// pixels are consecutive.  Canvas batch: h x w is the canvas, the image is the top-left sizes[img] of its slot -- clamped into
// the slot, so that no row of device memory can send an access outside it -- and only that rectangle is read and written.
// P pixels per thread and step: 4 (12 bytes in as dwords, three dword stores out) or 1 (byte by byte).
template <int P, bool CANVAS>
__device__ __forceinline__ void mask_images(const uint8_t* src, uint8_t* dst, int h, int w, const int32_t* sizes,
                                            const edet_gridmask_image_t* per_image) {
  const int img = blockIdx.y;
  const int slot_h = h, pitch = w;      // pitch: pixels from one row of the image to the next
  if constexpr (CANVAS) {
    h = clampi(sizes[2 * img], 1, slot_h);
    w = clampi(sizes[2 * img + 1], 1, pitch);
  }
  const int npix = h * w;
  const int slot = CANVAS ? slot_h * pitch : npix;      // pixels from one image to the next
  const edet_gridmask_image_t a = per_image[img];
  Mask m;
  // nothing in device memory may send a division by zero or an overflow into the stripe arithmetic
  m.apply = a.apply != 0;
  m.S = clampi(a.size, 0, MAX_SIDE);
  m.d = max(a.d, 1);
  m.l = clampi(a.l, 0, m.d);
  m.s1 = clampi(a.s1, 0, m.d);
  m.s2 = clampi(a.s2, 0, m.d);
  m.lim = m.d * (m.S / m.d);
  m.oy = (m.S - h) >> 1;      // floor division, as Python's //
  m.ox = (m.S - w) >> 1;
  m.c0 = a.coef[0]; m.c1 = a.coef[1]; m.c2 = a.coef[2]; m.c3 = a.coef[3]; m.c4 = a.coef[4]; m.c5 = a.coef[5];
  const uint8_t* in = src + (size_t)img * slot * 3;
  uint8_t* out = dst + (size_t)img * slot * 3;
  const int step = gridDim.x * THREADS;
  for (int q = blockIdx.x * THREADS + threadIdx.x; q * P < npix; q += step) {
    const int p0 = q * P;
    int y = p0 / w, x = p0 - y * w;
    if constexpr (P == 4) {
      // the group's first dword: a canvas group never leaves its row (w and the pitch are multiples of 4)
      const int q3 = CANVAS ? ((y * pitch + x) >> 2) * 3 : q * 3;
      uint32_t v[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = reinterpret_cast<const uint32_t*>(in)[q3 + k];
      if (m.apply) {
        uint32_t keep[3] = {0u, 0u, 0u};      // byte masks: 0xff over the three bytes of a kept pixel
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t on = mask_at(m, x, y) ? 0xffu : 0u;      // (the mask is 0 or 1: v * mask = v or 0)
#pragma unroll
          for (int c = 0; c < 3; ++c) keep[(3 * e + c) >> 2] |= on << (8 * ((3 * e + c) & 3));
          if (++x == w) { x = 0; ++y; }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] &= keep[k];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) reinterpret_cast<uint32_t*>(out)[q3 + k] = v[k];
    } else {
      const int on = m.apply ? mask_at(m, x, y) : 1;
      const size_t o = CANVAS ? (size_t)(y * pitch + x) * 3 : (size_t)p0 * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) out[o + c] = on ? in[o + c] : (uint8_t)0;
    }
  }
}

// P = 4 where H W is a multiple of 4 and both batches are 16-byte aligned, else 1
template <int P>
__global__ __launch_bounds__(THREADS) void k_gridmask(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w,
                                                     const edet_gridmask_image_t* __restrict__ per_image) {
  mask_images<P, false>(src, dst, h, w, nullptr, per_image);
}

// The grid is sized from the canvas; the threads a smaller image does not need leave the loop at once.  vec_ok: cw is a
// multiple of 4 and both batches are 16-byte aligned -- then the images whose own width is a multiple of 4 take the dword
// path (a choice per image, uniform over the workgroup).
__global__ __launch_bounds__(THREADS) void k_gridmask_canvas(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int ch,
                                                            int cw, const int32_t* __restrict__ sizes, int vec_ok,
                                                            const edet_gridmask_image_t* __restrict__ per_image) {
  if (vec_ok && clampi(sizes[2 * blockIdx.y + 1], 1, cw) % 4 == 0) mask_images<4, true>(src, dst, ch, cw, sizes, per_image);
  else mask_images<1, true>(src, dst, ch, cw, sizes, per_image);
}

}  // namespace

extern "C" int edet_gridmask(const uint8_t* src, uint8_t* dst, int batch, int height, int width,
                             const edet_gridmask_image_t* per_image_dev, void* stream) {
  EDET_CHECK(src && dst && per_image_dev, "edet_gridmask: null pointer");
  EDET_CHECK(src != dst, "edet_gridmask: in place");
  EDET_CHECK(batch > 0 && batch <= 65535 && height > 0 && width > 0, "edet_gridmask: batch %d, image %d x %d", batch, height,
             width);
  EDET_CHECK((int64_t)height * width * 3 < (int64_t)1 << 31, "edet_gridmask: image %d x %d too large", height, width);
  const int npix = height * width;
  const bool vec = npix % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  const int units = vec ? npix / 4 : npix;
  int gx = (units + THREADS * 4 - 1) / (THREADS * 4);      // about four steps per thread
  if (gx > 256) gx = 256;
  const dim3 grid((unsigned)gx, (unsigned)batch);
  hipStream_t st = to_stream(stream);
  if (vec) edet_launch(k_gridmask<4>, grid, dim3(THREADS), 0, st, src, dst, height, width, per_image_dev);
  else edet_launch(k_gridmask<1>, grid, dim3(THREADS), 0, st, src, dst, height, width, per_image_dev);
  EDET_LAUNCH_CHECK("edet_gridmask");
  return 0;
}

extern "C" int edet_gridmask_canvas(const uint8_t* src, uint8_t* dst, int batch, int canvas_h, int canvas_w,
                                    const int32_t* sizes_dev, const edet_gridmask_image_t* per_image_dev, void* stream) {
  EDET_CHECK(src && dst && sizes_dev && per_image_dev, "edet_gridmask_canvas: null pointer");
  EDET_CHECK(src != dst, "edet_gridmask_canvas: in place");
  EDET_CHECK(batch > 0 && batch <= 65535 && canvas_h > 0 && canvas_w > 0, "edet_gridmask_canvas: batch %d, canvas %d x %d", batch,
             canvas_h, canvas_w);
  EDET_CHECK((int64_t)canvas_h * canvas_w * 3 < (int64_t)1 << 31, "edet_gridmask_canvas: canvas %d x %d too large", canvas_h,
             canvas_w);
  const int npix = canvas_h * canvas_w;
  const bool vec = canvas_w % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  const int units = vec ? npix / 4 : npix;      // (an image on the byte path of a vec_ok batch takes four times the steps)
  int gx = (units + THREADS * 4 - 1) / (THREADS * 4);
  if (gx > 256) gx = 256;
  edet_launch(k_gridmask_canvas, dim3((unsigned)gx, (unsigned)batch), dim3(THREADS), 0, to_stream(stream), src, dst, canvas_h,
              canvas_w, sizes_dev, (int)vec, per_image_dev);
  EDET_LAUNCH_CHECK("edet_gridmask_canvas");
  return 0;
}
