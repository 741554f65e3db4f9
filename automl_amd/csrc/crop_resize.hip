// The front of the EfficientNetV2 input pipeline on the device (efficientnetv2/preprocessing.py:22-70): for every image of a
// batch of decoded uint8 images, tf.image.resize(tf.slice(image, crop), [out_h, out_w]) -- bilinear, half-pixel centres, no
// antialiasing -- then tf.image.random_flip_left_right with the decision taken, then either the clip / cast to uint8 of
// :49-50 (the input of edet_randaug_*) or the normalisation (v - 128) / 128 of :153 (the network input).
//
//   edet_crop_resize   raw uint8 [B][canvas_h][canvas_w][3], image b in the top-left height x width of its canvas; the crop,
//                      the valid extent and the flip bit per image come from device memory (edet_crop_image_t), so the
//                      launch never depends on the draws and a replayed graph sees new ones
//
// The taps clamp at the CROP edges (the reference slices before it resizes) and the mirror is on the OUTPUT: output column x
// is column out_w - 1 - x of the resized crop.  Every result is compared bit for bit with a numpy restatement
// (tests/crop_ref.py on oracle/preprocess_oracle.resize_bilinear), so the arithmetic is part of the interface: this file is
// compiled with -ffp-contract=off (automl_amd/build.py), and every product, sum and difference of the tap body (resize_tap.h,
// shared with csrc/mosaic.hip) is one rounded fp32 operation in the order of k_preprocess_infer (csrc/preprocess.hip):
// src = (o + 0.5) * (crop_n / out_n) - 0.5,
// lo = max(floor(src), 0), hi = min(ceil(src), crop_n - 1), t = src - floor(src); top row, bottom row, then vertical, each as
// a + (b - a) * t.
//
// A gather pass with little arithmetic: it reads about the crop area once and writes the output once.  A thread owns four
// consecutive pixels of one output row -- 12 bytes of uint8, 24 of bf16, 48 of fp32, stored as three 4-element vectors where
// out_w is a multiple of 4 (every run then starts on a vector boundary) -- and computes its row's y-taps once; the 64 lanes
// of a wave cover 256 consecutive pixels of that row, so a wave's stores are one contiguous stretch and its tap reads walk
// two source rows in order.  A tap pixel is read as one 4-byte load (three bytes used) where the four bytes lie inside the
// batch, which is everywhere but the batch's very last pixel.  No LDS, no atomics.
#include "resize_tap.h"

namespace {

using resize_tap::clampi;

constexpr int THREADS = 256;      // 4 waves = 4 output rows of 256 pixels
constexpr int RUN = 4;            // output pixels per thread
constexpr int OUT_U8 = 2;         // EDET_U8

template <typename T> __device__ __forceinline__ T out_of(float v);
// preprocessing.py:49-50: clip to [0, 255], then a truncating cast
template <> __device__ __forceinline__ uint8_t out_of<uint8_t>(float v) { return (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f); }
// preprocessing.py:153: (v - 128) / 128 (the division by a power of two is exact); bf16 rounds to nearest even
template <> __device__ __forceinline__ float out_of<float>(float v) { return (v - 128.0f) / 128.0f; }
template <> __device__ __forceinline__ bf16_t out_of<bf16_t>(float v) { return f2bf((v - 128.0f) / 128.0f); }

// grid: x = stretches of 256 pixels of a row, y = groups of 4 rows, z = the image.  VEC: out_w % 4 == 0 and `out` 16-byte
// aligned -> three vector stores per thread; else one store per value.
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void k_crop_resize(const uint8_t* __restrict__ raw, int canvas_h, int canvas_w, size_t total,
                                                        const edet_crop_image_t* __restrict__ per, T* __restrict__ out, int out_h,
                                                        int out_w) {
  const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * RUN;
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.z;
  if (x0 >= out_w || y >= out_h) return;
  // nothing in device memory may send an access outside the batch (automl_amd/v2_preprocessing.clamp_rows states the same)
  const edet_crop_image_t p = per[b];
  const int height = clampi(p.height, 1, canvas_h), width = clampi(p.width, 1, canvas_w);
  const int cy = clampi(p.crop_y, 0, height - 1), cx = clampi(p.crop_x, 0, width - 1);
  const int ch = clampi(p.crop_h, 1, height - cy), cw = clampi(p.crop_w, 1, width - cx);
  const bool flip = p.flip != 0;

  const resize_tap::Axis ty = resize_tap::axis_of(y, (float)ch / (float)out_h, ch);
  const size_t image = (size_t)b * canvas_h * canvas_w;
  const size_t row_lo = (image + (size_t)(cy + ty.lo) * canvas_w + cx) * 3;
  const size_t row_hi = (image + (size_t)(cy + ty.hi) * canvas_w + cx) * 3;
  const float xscale = (float)cw / (float)out_w;

  float v[RUN * 3];
#pragma unroll
  for (int e = 0; e < RUN; ++e) {
    const int x = min(x0 + e, out_w - 1);      // (a run that ends past the row repeats its last pixel and never stores it)
    const int xr = flip ? out_w - 1 - x : x;
    resize_tap::pixel(raw, row_lo, row_hi, total, resize_tap::axis_of(xr, xscale, cw), ty.t, v + e * 3);
  }
  T* o = out + (((size_t)b * out_h + y) * out_w + x0) * 3;
  resize_tap::store_run<VEC>(o, v, min(RUN, out_w - x0), [](float f) { return out_of<T>(f); });
}

template <typename T>
void launch(const uint8_t* raw, int batch, int canvas_h, int canvas_w, const edet_crop_image_t* per, void* out, int out_h,
            int out_w, hipStream_t st) {
  const dim3 grid(cdiv(out_w, 64 * RUN), cdiv(out_h, 4), batch);
  const size_t total = (size_t)batch * canvas_h * canvas_w * 3;
  const bool vec = out_w % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  if (vec) edet_launch(k_crop_resize<T, true>, grid, dim3(THREADS), 0, st, raw, canvas_h, canvas_w, total, per, (T*)out, out_h, out_w);
  else edet_launch(k_crop_resize<T, false>, grid, dim3(THREADS), 0, st, raw, canvas_h, canvas_w, total, per, (T*)out, out_h, out_w);
}

}  // namespace

extern "C" int edet_crop_resize(const uint8_t* raw, int batch, int canvas_h, int canvas_w,
                                const edet_crop_image_t* per_image_dev, void* out, int out_h, int out_w, int out_dtype,
                                void* stream) {
  EDET_CHECK(raw && per_image_dev && out, "edet_crop_resize: null pointer");
  EDET_CHECK(batch >= 1 && batch <= 65535 && canvas_h >= 1 && canvas_w >= 1 && out_h >= 1 && out_w >= 1,
             "edet_crop_resize: batch %d, canvas %d x %d, output %d x %d", batch, canvas_h, canvas_w, out_h, out_w);
  EDET_CHECK((int64_t)canvas_h * canvas_w * 3 < (int64_t)1 << 31, "edet_crop_resize: canvas %d x %d too large", canvas_h, canvas_w);
  EDET_CHECK(cdiv(out_h, 4) <= 65535, "edet_crop_resize: output %d x %d too tall", out_h, out_w);
  hipStream_t st = to_stream(stream);
  if (out_dtype == OUT_U8) launch<uint8_t>(raw, batch, canvas_h, canvas_w, per_image_dev, out, out_h, out_w, st);
  else if (out_dtype == EDET_F32) launch<float>(raw, batch, canvas_h, canvas_w, per_image_dev, out, out_h, out_w, st);
  else if (out_dtype == EDET_BF16) launch<bf16_t>(raw, batch, canvas_h, canvas_w, per_image_dev, out, out_h, out_w, st);
  else EDET_CHECK(false, "edet_crop_resize: bad out_dtype %d", out_dtype);
  EDET_LAUNCH_CHECK("edet_crop_resize");
  return 0;
}
