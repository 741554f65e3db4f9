// The front of the legacy EfficientNet input pipeline on the device (efficientnetv2/preprocess_legacy.py:80-127): for every
// image of a batch of decoded uint8 images, tf.image.resize_bicubic([crop], [out_h, out_w]) -- TensorFlow's LEGACY bicubic:
// align_corners=False, half_pixel_centers=False, a 1024-entry coefficient table with a = -0.75 -- then the left-right flip
// with the decision taken, then either the clip / cast to uint8 of :168-169 (the input of edet_randaug_*), or the resized
// values as they are, or the normalisation (v - mean[c]) / std[c] of :239-243 (the network input).
//
//   edet_crop_resize_bicubic   edet_crop_resize's contract (crop_resize.hip): raw uint8 [B][canvas_h][canvas_w][3], one
//                              edet_crop_image_t per image from device memory, clamped here, the flip on the output column,
//                              one launch per batch that never depends on the draws; plus the six floats of the
//                              normalisation, read on the host and passed by value
//
// NOT PINNED AGAINST TENSORFLOW: the definition below is written from TensorFlow's published resize_bicubic_op; TensorFlow is
// not installed where this project is tested and torch's bicubic is another filter (a = -0.75 as well, but half-pixel centres
// and no table).  What the kernel is compared with, bit for bit, is the numpy restatement tests/bicubic_ref.py: that
// restatement is the definition.
//
// The arithmetic is the interface (compiled with -ffp-contract=off, automl_amd/build.py).  Per axis, scale = float(crop_n) /
// float(out_n): in_f = float(o) * scale, in = floor(in_f), delta = in_f - float(in), off = lrintf(delta * 1024) (halves to
// even); weights (T[2 off + 1], T[2 off], T[2 (1024 - off)], T[2 (1024 - off) + 1]) on the taps in - 1, in, in + 1, in + 2,
// each clamped into [0, crop_n - 1] -- the CROP's edges: the reference crops before it resizes.  T[2i] = float(((a + 2) x -
// (a + 3)) x x + 1), T[2i + 1] = float(((a x' - 5a) x' + 8a) x' - 4a) for x = float(i / 1024), x' = float(x + 1), the
// polynomials in double: the table below is evaluated by the HOST compiler, once, and lies in the code object.  A value is
// formed vertically first: for each of the four tap columns c_k = p0 wy0 + p1 wy1 + p2 wy2 + p3 wy3, left to right, every
// product and sum one rounded fp32 operation; then v = c0 wx0 + c1 wx1 + c2 wx2 + c3 wx3 the same way.
//
// A gather pass shaped like k_crop_resize: a thread owns four consecutive pixels of one output row and computes the row's y
// taps once; the 64 lanes of a wave cover 256 consecutive pixels of that row, so a wave's stores are one contiguous stretch
// (three 4-element vectors per thread where out_w % 4 == 0) and its reads walk four source rows in order.  16 tap pixels per
// output pixel, each one 4-byte load (resize_tap::load_px: three bytes used; byte loads at the batch's very last pixel).  No
// LDS, no atomics.
#include "resize_tap.h"

namespace {

using resize_tap::clampi;

constexpr int THREADS = 256;      // 4 waves = 4 output rows of 256 pixels
constexpr int RUN = 4;            // output pixels per thread
constexpr int OUT_U8 = 2;         // EDET_U8
constexpr int TABLE = 1024;

struct Table { float v[2 * (TABLE + 1)]; };
constexpr Table make_table() {
  Table t{};
  const double a = -0.75;
  for (int i = 0; i <= TABLE; ++i) {
    const double x = (double)(float)(i / 1024.0);
    t.v[2 * i] = (float)(((a + 2) * x - (a + 3)) * x * x + 1);
    const double x1 = (double)((float)x + 1.0f);
    t.v[2 * i + 1] = (float)(((a * x1 - 5 * a) * x1 + 8 * a) * x1 - 4 * a);
  }
  return t;
}
__device__ const Table g_table = make_table();

struct Norm { float mean[3], std[3]; };      // by value in the kernel arguments

// one axis of one output position: the four clamped taps and their weights
struct Taps {
  int i[4];
  float w[4];
};
__device__ __forceinline__ Taps taps_of(int o, float scale, int in_n) {
  const float in_f = (float)o * scale;
  const float fl = floorf(in_f);
  const int in = (int)fl;
  const float delta = in_f - fl;
  const int off = clampi((int)lrintf(delta * 1024.0f), 0, TABLE);      // (delta is in [0, 1): the clamp only states it)
  Taps t;
#pragma unroll
  for (int k = 0; k < 4; ++k) t.i[k] = clampi(in - 1 + k, 0, in_n - 1);
  t.w[0] = g_table.v[2 * off + 1];
  t.w[1] = g_table.v[2 * off];
  t.w[2] = g_table.v[2 * (TABLE - off)];
  t.w[3] = g_table.v[2 * (TABLE - off) + 1];
  return t;
}

template <typename T> __device__ __forceinline__ T out_of(float v);
// preprocess_legacy.py:168-169: clip to [0, 255], then a truncating cast
template <> __device__ __forceinline__ uint8_t out_of<uint8_t>(float v) { return (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f); }
template <> __device__ __forceinline__ float out_of<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t out_of<bf16_t>(float v) { return f2bf(v); }

// grid: x = stretches of 256 pixels of a row, y = groups of 4 rows, z = the image.  VEC: out_w % 4 == 0 and `out` 16-byte
// aligned.  NORM: (v - mean[c]) / std[c] in front of the conversion (never for uint8).
template <typename T, bool VEC, bool NORM>
__global__ __launch_bounds__(THREADS) void k_crop_bicubic(const uint8_t* __restrict__ raw, int canvas_h, int canvas_w, size_t total,
                                                         const edet_crop_image_t* __restrict__ per, T* __restrict__ out, int out_h,
                                                         int out_w, Norm norm) {
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

  const Taps ty = taps_of(y, (float)ch / (float)out_h, ch);
  const size_t image = (size_t)b * canvas_h * canvas_w;
  size_t row[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) row[j] = (image + (size_t)(cy + ty.i[j]) * canvas_w + cx) * 3;
  const float xscale = (float)cw / (float)out_w;

  float v[RUN * 3];
#pragma unroll
  for (int e = 0; e < RUN; ++e) {
    const int x = min(x0 + e, out_w - 1);      // (a run that ends past the row repeats its last pixel and never stores it)
    const Taps tx = taps_of(flip ? out_w - 1 - x : x, xscale, cw);
    float col[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const size_t at = (size_t)tx.i[k] * 3;
      uint32_t px[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) px[j] = resize_tap::load_px(raw, row[j] + at, total);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float s = (float)((px[0] >> (8 * c)) & 255) * ty.w[0];
        s = s + (float)((px[1] >> (8 * c)) & 255) * ty.w[1];
        s = s + (float)((px[2] >> (8 * c)) & 255) * ty.w[2];
        col[k][c] = s + (float)((px[3] >> (8 * c)) & 255) * ty.w[3];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float s = col[0][c] * tx.w[0];
      s = s + col[1][c] * tx.w[1];
      s = s + col[2][c] * tx.w[2];
      s = s + col[3][c] * tx.w[3];
      if constexpr (NORM) s = (s - norm.mean[c]) / norm.std[c];      // two rounded operations, an IEEE division
      v[e * 3 + c] = s;
    }
  }
  T* o = out + (((size_t)b * out_h + y) * out_w + x0) * 3;
  resize_tap::store_run<VEC>(o, v, min(RUN, out_w - x0), [](float f) { return out_of<T>(f); });
}

template <typename T, bool NORM>
void launch(const uint8_t* raw, int batch, int canvas_h, int canvas_w, const edet_crop_image_t* per, void* out, int out_h,
            int out_w, const Norm& norm, hipStream_t st) {
  const dim3 grid(cdiv(out_w, 64 * RUN), cdiv(out_h, 4), batch);
  const size_t total = (size_t)batch * canvas_h * canvas_w * 3;
  const bool vec = out_w % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  if (vec) edet_launch(k_crop_bicubic<T, true, NORM>, grid, dim3(THREADS), 0, st, raw, canvas_h, canvas_w, total, per, (T*)out, out_h, out_w, norm);
  else edet_launch(k_crop_bicubic<T, false, NORM>, grid, dim3(THREADS), 0, st, raw, canvas_h, canvas_w, total, per, (T*)out, out_h, out_w, norm);
}

}  // namespace

extern "C" int edet_crop_resize_bicubic(const uint8_t* raw, int batch, int canvas_h, int canvas_w,
                                        const edet_crop_image_t* per_image_dev, void* out, int out_h, int out_w, int out_dtype,
                                        const float* mean_std, void* stream) {
  EDET_CHECK(raw && per_image_dev && out, "edet_crop_resize_bicubic: null pointer");
  EDET_CHECK(batch >= 1 && batch <= 65535 && canvas_h >= 1 && canvas_w >= 1 && out_h >= 1 && out_w >= 1,
             "edet_crop_resize_bicubic: batch %d, canvas %d x %d, output %d x %d", batch, canvas_h, canvas_w, out_h, out_w);
  EDET_CHECK((int64_t)canvas_h * canvas_w * 3 < (int64_t)1 << 31, "edet_crop_resize_bicubic: canvas %d x %d too large", canvas_h,
             canvas_w);
  EDET_CHECK(cdiv(out_h, 4) <= 65535, "edet_crop_resize_bicubic: output %d x %d too tall", out_h, out_w);
  Norm norm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
  if (mean_std) {
    for (int c = 0; c < 3; ++c) {
      norm.mean[c] = mean_std[c];
      norm.std[c] = mean_std[3 + c];
      EDET_CHECK(norm.std[c] != 0.f && norm.std[c] == norm.std[c] && norm.mean[c] == norm.mean[c],
                 "edet_crop_resize_bicubic: mean %g, std %g of channel %d", norm.mean[c], norm.std[c], c);
    }
  }
  hipStream_t st = to_stream(stream);
  const bool on = mean_std != nullptr;
  if (out_dtype == OUT_U8) launch<uint8_t, false>(raw, batch, canvas_h, canvas_w, per_image_dev, out, out_h, out_w, norm, st);
  else if (out_dtype == EDET_F32 && on) launch<float, true>(raw, batch, canvas_h, canvas_w, per_image_dev, out, out_h, out_w, norm, st);
  else if (out_dtype == EDET_F32) launch<float, false>(raw, batch, canvas_h, canvas_w, per_image_dev, out, out_h, out_w, norm, st);
  else if (out_dtype == EDET_BF16 && on) launch<bf16_t, true>(raw, batch, canvas_h, canvas_w, per_image_dev, out, out_h, out_w, norm, st);
  else if (out_dtype == EDET_BF16) launch<bf16_t, false>(raw, batch, canvas_h, canvas_w, per_image_dev, out, out_h, out_w, norm, st);
  else EDET_CHECK(false, "edet_crop_resize_bicubic: bad out_dtype %d", out_dtype);
  EDET_LAUNCH_CHECK("edet_crop_resize_bicubic");
  return 0;
}
