// The bilinear tap rule that edet_crop_resize (crop_resize.hip) and edet_mosaic (mosaic.hip) share: tf.image.resize of a
// rectangle of a decoded uint8 image -- half-pixel centres, no antialiasing, taps clamped at the rectangle's edges -- as
// single rounded fp32 operations in the order of k_preprocess_infer (csrc/preprocess.hip).  Both files are compared bit for bit
// with numpy restatements on oracle/preprocess_oracle.resize_bilinear, so the order below is part of their interface, and
// every file that includes this header is compiled with -ffp-contract=off (automl_amd/build.py).
#pragma once
#include "common.h"

namespace resize_tap {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the three channel bytes of the pixel at byte offset `at` of the batch, in bits 0..23
__device__ __forceinline__ uint32_t load_px(const uint8_t* __restrict__ raw, size_t at, size_t total) {
  if (at + 4 <= total) {
    uint32_t v;
    __builtin_memcpy(&v, raw + at, 4);      // (no alignment promised: pixels are 3 bytes apart)
    return v;
  }
  return (uint32_t)raw[at] | ((uint32_t)raw[at + 1] << 8) | ((uint32_t)raw[at + 2] << 16);
}

// One axis of one output position: src = (o + 0.5) * scale - 0.5 with scale = in_n / out_n already rounded,
// lo = max(floor(src), 0), hi = min(ceil(src), in_n - 1), t = src - floor(src).
struct Axis {
  int lo, hi;
  float t;
};
__device__ __forceinline__ Axis axis_of(int o, float scale, int in_n) {
  const float s = ((float)o + 0.5f) * scale - 0.5f;
  const float f = floorf(s);
  Axis a;
  a.lo = max((int)f, 0);
  a.hi = min((int)ceilf(s), in_n - 1);
  a.t = s - f;
  return a;
}

// v[0..2] = the three channels of one output pixel: row_lo / row_hi are the byte offsets of the rectangle's first pixel in
// the two tap rows; top row, bottom row, then vertical, each as a + (b - a) * t.
__device__ __forceinline__ void pixel(const uint8_t* __restrict__ raw, size_t row_lo, size_t row_hi, size_t total, Axis x,
                                      float ly, float* v) {
  const uint32_t tl = load_px(raw, row_lo + (size_t)x.lo * 3, total), tr = load_px(raw, row_lo + (size_t)x.hi * 3, total);
  const uint32_t bl = load_px(raw, row_hi + (size_t)x.lo * 3, total), br = load_px(raw, row_hi + (size_t)x.hi * 3, total);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float ftl = (float)((tl >> (8 * c)) & 255), ftr = (float)((tr >> (8 * c)) & 255);
    const float fbl = (float)((bl >> (8 * c)) & 255), fbr = (float)((br >> (8 * c)) & 255);
    const float top = ftl + (ftr - ftl) * x.t;
    const float bot = fbl + (fbr - fbl) * x.t;
    v[c] = top + (bot - top) * ly;
  }
}

template <typename T> struct alignas(sizeof(T) * 4) Quad { T v[4]; };

// stores a thread's run of four pixels (12 converted values) at `o`: three 4-element vectors with VEC, else one store per
// value of the `pixels` (1..4) that lie inside the row
template <bool VEC, typename T, typename F>
__device__ __forceinline__ void store_run(T* __restrict__ o, const float* v, int pixels, F convert) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Quad<T> q;
#pragma unroll
      for (int e = 0; e < 4; ++e) q.v[e] = convert(v[4 * k + e]);
      reinterpret_cast<Quad<T>*>(o)[k] = q;
    }
  } else {
    const int n = pixels * 3;
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < n) o[k] = convert(v[k]);
  }
}

}  // namespace resize_tap
