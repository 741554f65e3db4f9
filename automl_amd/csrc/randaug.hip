// RandAugment of a training batch on the device (efficientnetv2/autoaugment.py:79-441, :663-702): uint8 NHWC images
// [B, H, W, 3], one of 16 operations per image and layer.  The choice and its arguments are the caller's, in device memory,
// so the launch sequence never depends on the draws and a replayed graph sees new ones.
//
//   edet_randaug_stats   per-channel 256-bin histograms of the images whose operation is AutoContrast or Equalize (integer
//                        LDS atomics: exact in any order) -> a 3 x 256 uint8 look-up table per image
//   edet_randaug_apply   one layer, src -> dst (never in place: the geometric operations and Sharpness read neighbours);
//                        dst is uint8 or, for the last layer, the normalised network input (x - 128) / 128 in fp32 / bf16
//
// Every uint8 result is compared bit for bit with a numpy restatement (tests/randaug_ref.py), so the arithmetic is part of
// the interface: this file is compiled with -ffp-contract=off (automl_amd/build.py), every product and sum below is a single
// rounded fp32 operation in the order written, and every float -> uint8 conversion is a truncation after the stated clip.
//
// Contrast reproduces the reference as it is written (autoaugment.py:196-210): its "mean" is reduce_sum(histogram) / 256 =
// H W / 256, not the mean grey level, so the degenerate image is the constant uint8(min(H W / 256, 255)) and the operation
// needs no statistics pass.  Solarize compares in int32: a threshold >= 256 leaves every pixel as it is (what TensorFlow's
// conversion of an out-of-range Python integer to uint8 would do is pinned by nothing here).
#include "common.h"
#include "randaug_impl.h"

namespace {

constexpr int THREADS = 256;
constexpr int OP_AUTOCONTRAST = 0, OP_EQUALIZE = 1, OP_INVERT = 2, OP_ROTATE = 3, OP_POSTERIZE = 4, OP_SOLARIZE = 5,
              OP_COLOR = 6, OP_CONTRAST = 7, OP_BRIGHTNESS = 8, OP_SHARPNESS = 9, OP_SHEAR_X = 10, OP_TRANSLATE_Y = 13,
              OP_CUTOUT = 14, OP_SOLARIZE_ADD = 15, OP_IDENTITY = 16;
constexpr int OUT_U8 = 2;      // EDET_U8

using raug::blend;
using raug::clampi;
using raug::clip_u8;
using raug::gray_of;

// ---- statistics: one workgroup per image --------------------------------------------------------------------------------
// the bytes [p, p + n) into the three histograms: bytes in front of the first 4-byte boundary, whole words, bytes behind the
// last one; channel of byte k = k % 3 (p is the first byte of a pixel)
__device__ __forceinline__ void hist_span(const uint8_t* __restrict__ p, int n, int* hist) {
  const int head = min((int)((4 - (reinterpret_cast<uintptr_t>(p) & 3)) & 3), n);
  const int words = (n - head) / 4;
  if ((int)threadIdx.x < head) atomicAdd(&hist[(threadIdx.x % 3) * 256 + p[threadIdx.x]], 1);
  const uint32_t* pw = reinterpret_cast<const uint32_t*>(p + head);
  for (int i = threadIdx.x; i < words; i += THREADS) {
    const uint32_t v = pw[i];
    int c = (head + 4 * i) % 3;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      atomicAdd(&hist[c * 256 + ((v >> (8 * e)) & 255)], 1);
      c = c == 2 ? 0 : c + 1;
    }
  }
  const int tail = head + 4 * words;
  if ((int)threadIdx.x < n - tail) atomicAdd(&hist[((tail + threadIdx.x) % 3) * 256 + p[tail + threadIdx.x]], 1);
}

// One image of `rows` spans of n bytes each, pitch bytes apart (dense: one span, the whole image) -> its table.
__device__ __forceinline__ void stats_image(const uint8_t* __restrict__ p, int rows, int n, size_t pitch, int op,
                                            uint8_t* __restrict__ out) {
  __shared__ int hist[3 * 256];
  __shared__ int lo_s[3], hi_s[3], step_s[3];
  for (int i = threadIdx.x; i < 3 * 256; i += THREADS) hist[i] = 0;
  __syncthreads();
  for (int y = 0; y < rows; ++y) hist_span(p + (size_t)y * pitch, n, hist);
  __syncthreads();
  if (threadIdx.x < 3) {      // one thread per channel: lowest / highest occupied bin, Equalize's step, the running sum
    int* h = hist + threadIdx.x * 256;
    int lo = 255, hi = 0;
    for (int i = 0; i < 256; ++i) {
      if (h[i]) {
        lo = min(lo, i);
        hi = i;
      }
    }
    lo_s[threadIdx.x] = lo;
    hi_s[threadIdx.x] = hi;
    step_s[threadIdx.x] = (rows * (n / 3) - h[hi]) / 255;      // (sum of the non-zero bins - the last of them) // 255
    int run = 0;
    for (int i = 0; i < 256; ++i) {
      run += h[i];
      h[i] = run;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 768; i += THREADS) {
    const int c = i >> 8, v = i & 255;
    int r = v;
    if (op == OP_AUTOCONTRAST) {      // autoaugment.py:295-312
      const float lo = (float)lo_s[c], hi = (float)hi_s[c];
      if (hi > lo) {
        const float scale = 255.0f / (hi - lo);
        const float offset = -lo * scale;
        r = clip_u8((float)v * scale + offset);
      }
    } else {      // autoaugment.py:354-381
      const int step = step_s[c];
      if (step != 0) r = v == 0 ? 0 : clampi((hist[c * 256 + v - 1] + step / 2) / step, 0, 255);
    }
    out[i] = (uint8_t)r;
  }
}

__global__ __launch_bounds__(THREADS) void k_randaug_stats(const uint8_t* __restrict__ src, int n, const int32_t* __restrict__ ops,
                                                          uint8_t* __restrict__ luts) {
  const int img = blockIdx.x;
  const int op = ops[img];
  if (op != OP_AUTOCONTRAST && op != OP_EQUALIZE) return;      // (uniform over the workgroup)
  stats_image(src + (size_t)img * n, 1, n, 0, op, luts + (size_t)img * 768);
}

// The canvas batch: the histograms count the h x w rectangle of the image's slot only, (h, w) = sizes[img] clamped into the
// slot.  An image as wide as the canvas is one span, as in the dense batch; a narrower one is a span per row.
__global__ __launch_bounds__(THREADS) void k_randaug_stats_canvas(const uint8_t* __restrict__ src, int ch, int cw,
                                                                 const int32_t* __restrict__ sizes, const int32_t* __restrict__ ops,
                                                                 uint8_t* __restrict__ luts) {
  const int img = blockIdx.x;
  const int op = ops[img];
  if (op != OP_AUTOCONTRAST && op != OP_EQUALIZE) return;      // (uniform over the workgroup)
  const int h = clampi(sizes[2 * img], 1, ch), w = clampi(sizes[2 * img + 1], 1, cw);
  const uint8_t* p = src + (size_t)img * ch * cw * 3;
  if (w == cw) stats_image(p, 1, h * w * 3, 0, op, luts + (size_t)img * 768);
  else stats_image(p, h, w * 3, (size_t)cw * 3, op, luts + (size_t)img * 768);
}

// ---- one layer ----------------------------------------------------------------------------------------------------------
struct Args {
  int op, h, w, pitch, i0, i1, i2, i3;      // pitch: pixels from one row of the image to the next (dense: w)
  float a0, a1, a2, b0, b1, b2, f;
  const uint8_t* img;      // this image of src
  const uint8_t* lut;      // its 3 x 256 table
};

struct Px { int r, g, b; };
__device__ __forceinline__ Px load_px(const uint8_t* p) { return Px{p[0], p[1], p[2]}; }

// output pixel (x, y) of a geometric operation: the source pixel nearest to the transformed point (halves away from zero),
// 128 outside the image -- wrap / unwrap with replace = [128] * 3 (autoaugment.py:398-441)
__device__ __forceinline__ Px geometric(const Args& a, int x, int y) {
  const float fx = (float)x, fy = (float)y;
  const float sx = roundf((a.a0 * fx + a.a1 * fy) + a.a2);
  const float sy = roundf((a.b0 * fx + a.b1 * fy) + a.b2);
  if (!(sx >= 0.f && sx <= (float)(a.w - 1) && sy >= 0.f && sy <= (float)(a.h - 1))) return Px{128, 128, 128};
  return load_px(a.img + ((size_t)(int)sy * a.pitch + (int)sx) * 3);
}

// PIL's SMOOTH kernel on the interior, the original on the one-pixel border (autoaugment.py:323-349), then the blend
__device__ __forceinline__ Px sharpness(const Args& a, int x, int y, Px o) {
  if (x == 0 || y == 0 || x >= a.w - 1 || y >= a.h - 1) return o;      // blend(o, o, f) = o
  const float w1 = 1.0f / 13.0f, w5 = 5.0f / 13.0f;
  float sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const Px q = load_px(a.img + ((size_t)(y + dy) * a.pitch + (x + dx)) * 3);
      const float k = (dy == 0 && dx == 0) ? w5 : w1;
      sr = sr + k * (float)q.r;
      sg = sg + k * (float)q.g;
      sb = sb + k * (float)q.b;
    }
  }
  return Px{blend(clip_u8(sr), o.r, a.f), blend(clip_u8(sg), o.g, a.f), blend(clip_u8(sb), o.b, a.f)};
}

// one channel value of the operations that look at nothing else
__device__ __forceinline__ int pointwise(const Args& a, int v, int c) {
  switch (a.op) {
    case OP_AUTOCONTRAST:
    case OP_EQUALIZE: return a.lut[c * 256 + v];
    case OP_INVERT: return 255 - v;
    case OP_POSTERIZE: return ((v >> a.i0) << a.i0) & 255;
    case OP_SOLARIZE: return v < a.i0 ? v : 255 - v;
    case OP_SOLARIZE_ADD: return v < a.i1 ? clampi(v + a.i0, 0, 255) : v;
    case OP_CONTRAST: return blend(a.i0, v, a.f);
    case OP_BRIGHTNESS: return blend(0, v, a.f);
    default: return v;
  }
}

__device__ __forceinline__ Px apply_px(const Args& a, int x, int y, Px o) {
  if (a.op == OP_COLOR) {
    const int g = gray_of(o.r, o.g, o.b);
    return Px{blend(g, o.r, a.f), blend(g, o.g, a.f), blend(g, o.b, a.f)};
  }
  if (a.op == OP_SHARPNESS) return sharpness(a, x, y, o);
  if (a.op == OP_ROTATE || (a.op >= OP_SHEAR_X && a.op <= OP_TRANSLATE_Y)) return geometric(a, x, y);
  if (a.op == OP_CUTOUT) return (y >= a.i0 && y < a.i2 && x >= a.i1 && x < a.i3) ? Px{128, 128, 128} : o;
  return Px{pointwise(a, o.r, 0), pointwise(a, o.g, 1), pointwise(a, o.b, 2)};
}

template <typename T> __device__ __forceinline__ T out_of(int v);
template <> __device__ __forceinline__ uint8_t out_of<uint8_t>(int v) { return (uint8_t)v; }
// (x - 128) / 128 (efficientnetv2/preprocessing.py:153): at most 8 significant bits, exact in fp32 and in bf16
template <> __device__ __forceinline__ float out_of<float>(int v) { return (float)(v - 128) * (1.0f / 128.0f); }
template <> __device__ __forceinline__ bf16_t out_of<bf16_t>(int v) { return f2bf((float)(v - 128) * (1.0f / 128.0f)); }

// the conversion of one channel value into the destination's element: the fixed one above, or the legacy pipeline's
// (v - mean[c]) / std[c] (preprocess_legacy.py:239-243) -- two rounded fp32 operations with an IEEE division, bf16 the one
// final rounding of that value; uint8 is the value itself either way
template <typename T> struct FixedOut {
  __device__ __forceinline__ T operator()(int v, int) const { return out_of<T>(v); }
};
template <typename T> struct NormOut {
  float mean[3], std[3];
  __device__ __forceinline__ T operator()(int v, int c) const {
    if constexpr (sizeof(T) == 1) return (T)v;
    else return from_f<T>(((float)v - mean[c]) / std[c]);
  }
};

template <typename T> struct alignas(sizeof(T) * 4) Quad { T v[4]; };

// One image: `in` / `out` are its first pixel, `pitch` its row pitch in pixels (dense: w, the pixels are consecutive; canvas:
// the canvas width, and only the h x w rectangle is read and written).  P pixels per thread and step: 4 (12 bytes in, three
// 4-element stores out) or 1 (byte by byte); with CANVAS, P = 4 needs w and pitch to be multiples of 4.
template <typename T, int P, bool CANVAS, typename O = FixedOut<T>>
__device__ __forceinline__ void apply_image(const uint8_t* __restrict__ in, T* __restrict__ out, int h, int w, int pitch, int img,
                                            const int32_t* __restrict__ ops, const int32_t* __restrict__ iargs,
                                            const float* __restrict__ fargs, const uint8_t* __restrict__ luts, const O conv = O()) {
  const int npix = h * w;
  Args a;
  a.op = ops ? ops[img] : OP_IDENTITY;
  if (a.op < 0 || a.op > OP_IDENTITY) a.op = OP_IDENTITY;
  a.h = h;
  a.w = w;
  a.pitch = pitch;
  a.i0 = a.i1 = a.i2 = a.i3 = 0;
  a.a0 = a.a1 = a.a2 = a.b0 = a.b1 = a.b2 = 0.f;
  a.f = 1.f;
  if (a.op != OP_IDENTITY) {
    const int32_t* ia = iargs + (size_t)img * 4;
    const float* fa = fargs + (size_t)img * 8;
    a.i0 = ia[0]; a.i1 = ia[1]; a.i2 = ia[2]; a.i3 = ia[3];
    a.a0 = fa[0]; a.a1 = fa[1]; a.a2 = fa[2]; a.b0 = fa[3]; a.b1 = fa[4]; a.b2 = fa[5];
    a.f = fa[6];
  }
  // nothing in device memory may send an access outside the batch or a shift outside the value
  if (a.op == OP_POSTERIZE) a.i0 = clampi(a.i0, 0, 8);
  if (a.op == OP_SOLARIZE_ADD) a.i0 = clampi(a.i0, -255, 255);
  if (a.op == OP_CUTOUT) {
    a.i0 = clampi(a.i0, 0, h); a.i2 = clampi(a.i2, 0, h);
    a.i1 = clampi(a.i1, 0, w); a.i3 = clampi(a.i3, 0, w);
  }
  if (a.op == OP_CONTRAST) a.i0 = (int)fminf((float)npix / 256.0f, 255.f);
  a.img = in;
  a.lut = luts + (size_t)img * 768;
  const int step = gridDim.x * THREADS;
  for (int q = blockIdx.x * THREADS + threadIdx.x; q * P < npix; q += step) {
    const int p0 = q * P;
    int y = p0 / w, x = p0 - y * w;
    if constexpr (P == 4) {
      const int q3 = CANVAS ? ((y * pitch + x) >> 2) * 3 : q * 3;      // the group's first dword
      uint32_t in4[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) in4[k] = reinterpret_cast<const uint32_t*>(a.img)[q3 + k];
      int res[12];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        Px o;
        o.r = (in4[(3 * e) >> 2] >> (8 * ((3 * e) & 3))) & 255;
        o.g = (in4[(3 * e + 1) >> 2] >> (8 * ((3 * e + 1) & 3))) & 255;
        o.b = (in4[(3 * e + 2) >> 2] >> (8 * ((3 * e + 2) & 3))) & 255;
        const Px r = apply_px(a, x, y, o);
        res[3 * e] = r.r; res[3 * e + 1] = r.g; res[3 * e + 2] = r.b;
        if (++x == w) { x = 0; ++y; }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        Quad<T> o4;
#pragma unroll
        for (int e = 0; e < 4; ++e) o4.v[e] = conv(res[4 * k + e], (4 * k + e) % 3);
        reinterpret_cast<Quad<T>*>(out)[q3 + k] = o4;
      }
    } else {
      const size_t o = CANVAS ? (size_t)(y * pitch + x) * 3 : (size_t)p0 * 3;
      const Px r = apply_px(a, x, y, load_px(a.img + o));
      out[o] = conv(r.r, 0);
      out[o + 1] = conv(r.g, 1);
      out[o + 2] = conv(r.b, 2);
    }
  }
}

// blockIdx.y = the image (the operation is uniform over a workgroup).  P pixels per thread and step: 4 where H W is a
// multiple of 4 and both batches are 16-byte aligned, else 1.
template <typename T, int P>
__global__ __launch_bounds__(THREADS) void k_randaug_apply(const uint8_t* __restrict__ src, T* __restrict__ dst, int h, int w,
                                                          const int32_t* __restrict__ ops, const int32_t* __restrict__ iargs,
                                                          const float* __restrict__ fargs, const uint8_t* __restrict__ luts) {
  const int img = blockIdx.y;
  const int npix = h * w;
  apply_image<T, P, false>(src + (size_t)img * npix * 3, dst + (size_t)img * npix * 3, h, w, w, img, ops, iargs, fargs, luts);
}

// the same layer with the legacy normalisation in the last conversion (edet_randaug_apply_norm)
template <typename T, int P>
__global__ __launch_bounds__(THREADS) void k_randaug_apply_norm(const uint8_t* __restrict__ src, T* __restrict__ dst, int h, int w,
                                                               const int32_t* __restrict__ ops, const int32_t* __restrict__ iargs,
                                                               const float* __restrict__ fargs, const uint8_t* __restrict__ luts,
                                                               NormOut<T> conv) {
  const int img = blockIdx.y;
  const int npix = h * w;
  apply_image<T, P, false>(src + (size_t)img * npix * 3, dst + (size_t)img * npix * 3, h, w, w, img, ops, iargs, fargs, luts, conv);
}

// The canvas batch: image blockIdx.y is the top-left h x w of its ch x cw slot in src and in dst, (h, w) = sizes[img]
// clamped into the slot; the rest of the dst slot is not written.  The grid is sized from the canvas.  vec_ok: cw is a
// multiple of 4 and both batches are 16-byte aligned -- then the images whose own width is a multiple of 4 take the
// four-pixel path (a choice per image, uniform over the workgroup).
template <typename T>
__global__ __launch_bounds__(THREADS) void k_randaug_apply_canvas(const uint8_t* __restrict__ src, T* __restrict__ dst, int ch,
                                                                 int cw, const int32_t* __restrict__ sizes, int vec_ok,
                                                                 const int32_t* __restrict__ ops, const int32_t* __restrict__ iargs,
                                                                 const float* __restrict__ fargs, const uint8_t* __restrict__ luts) {
  const int img = blockIdx.y;
  const int h = clampi(sizes[2 * img], 1, ch), w = clampi(sizes[2 * img + 1], 1, cw);
  const size_t slot = (size_t)img * ch * cw * 3;
  if (vec_ok && w % 4 == 0) apply_image<T, 4, true>(src + slot, dst + slot, h, w, cw, img, ops, iargs, fargs, luts);
  else apply_image<T, 1, true>(src + slot, dst + slot, h, w, cw, img, ops, iargs, fargs, luts);
}

template <typename T>
void launch_apply(const uint8_t* src, void* dst, int batch, int h, int w, const int32_t* ops, const int32_t* iargs,
                  const float* fargs, const uint8_t* luts, hipStream_t st) {
  const int npix = h * w;
  const bool vec = npix % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  const int units = vec ? npix / 4 : npix;
  int gx = (units + THREADS * 4 - 1) / (THREADS * 4);      // about four steps per thread
  if (gx > 256) gx = 256;
  const dim3 grid((unsigned)gx, (unsigned)batch);
  if (vec) edet_launch(k_randaug_apply<T, 4>, grid, dim3(THREADS), 0, st, src, (T*)dst, h, w, ops, iargs, fargs, luts);
  else edet_launch(k_randaug_apply<T, 1>, grid, dim3(THREADS), 0, st, src, (T*)dst, h, w, ops, iargs, fargs, luts);
}

template <typename T>
void launch_apply_norm(const uint8_t* src, void* dst, int batch, int h, int w, const int32_t* ops, const int32_t* iargs,
                       const float* fargs, const uint8_t* luts, const float* mean_std, hipStream_t st) {
  NormOut<T> conv;
  for (int c = 0; c < 3; ++c) {
    conv.mean[c] = mean_std[c];
    conv.std[c] = mean_std[3 + c];
  }
  const int npix = h * w;
  const bool vec = npix % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  const int units = vec ? npix / 4 : npix;
  int gx = (units + THREADS * 4 - 1) / (THREADS * 4);      // launch_apply's grid
  if (gx > 256) gx = 256;
  const dim3 grid((unsigned)gx, (unsigned)batch);
  if (vec) edet_launch(k_randaug_apply_norm<T, 4>, grid, dim3(THREADS), 0, st, src, (T*)dst, h, w, ops, iargs, fargs, luts, conv);
  else edet_launch(k_randaug_apply_norm<T, 1>, grid, dim3(THREADS), 0, st, src, (T*)dst, h, w, ops, iargs, fargs, luts, conv);
}

template <typename T>
void launch_apply_canvas(const uint8_t* src, void* dst, int batch, int ch, int cw, const int32_t* sizes, const int32_t* ops,
                         const int32_t* iargs, const float* fargs, const uint8_t* luts, hipStream_t st) {
  const int npix = ch * cw;
  const bool vec = cw % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  const int units = vec ? npix / 4 : npix;
  int gx = (units + THREADS * 4 - 1) / (THREADS * 4);
  if (gx > 256) gx = 256;
  edet_launch(k_randaug_apply_canvas<T>, dim3((unsigned)gx, (unsigned)batch), dim3(THREADS), 0, st, src, (T*)dst, ch, cw, sizes,
              (int)vec, ops, iargs, fargs, luts);
}

}  // namespace

extern "C" int edet_randaug_stats(const uint8_t* src, int batch, int height, int width, const int32_t* ops, uint8_t* luts,
                                  void* stream) {
  EDET_CHECK(src && ops && luts, "edet_randaug_stats: null pointer");
  EDET_CHECK(batch > 0 && height > 0 && width > 0, "edet_randaug_stats: batch %d, image %d x %d", batch, height, width);
  EDET_CHECK((int64_t)height * width * 3 < (int64_t)1 << 31, "edet_randaug_stats: image %d x %d too large", height, width);
  edet_launch(k_randaug_stats, dim3(batch), dim3(THREADS), 0, to_stream(stream), src, height * width * 3, ops, luts);
  EDET_LAUNCH_CHECK("edet_randaug_stats");
  return 0;
}

extern "C" int edet_randaug_apply(const uint8_t* src, void* dst, int batch, int height, int width, const int32_t* ops,
                                  const int32_t* iargs, const float* fargs, const uint8_t* luts, int out_dtype, void* stream) {
  EDET_CHECK(src && dst, "edet_randaug_apply: null pointer");
  EDET_CHECK(!ops || (iargs && fargs && luts), "edet_randaug_apply: ops without iargs / fargs / luts");
  EDET_CHECK((const void*)src != dst, "edet_randaug_apply: in place (the geometric operations and Sharpness read neighbours)");
  EDET_CHECK(batch > 0 && batch <= 65535 && height > 0 && width > 0, "edet_randaug_apply: batch %d, image %d x %d", batch, height,
             width);
  EDET_CHECK((int64_t)height * width * 3 < (int64_t)1 << 31, "edet_randaug_apply: image %d x %d too large", height, width);
  hipStream_t st = to_stream(stream);
  if (out_dtype == OUT_U8) launch_apply<uint8_t>(src, dst, batch, height, width, ops, iargs, fargs, luts, st);
  else if (out_dtype == EDET_F32) launch_apply<float>(src, dst, batch, height, width, ops, iargs, fargs, luts, st);
  else if (out_dtype == EDET_BF16) launch_apply<bf16_t>(src, dst, batch, height, width, ops, iargs, fargs, luts, st);
  else EDET_CHECK(false, "edet_randaug_apply: bad out_dtype %d", out_dtype);
  EDET_LAUNCH_CHECK("edet_randaug_apply");
  return 0;
}

extern "C" int edet_randaug_apply_norm(const uint8_t* src, void* dst, int batch, int height, int width, const int32_t* ops,
                                       const int32_t* iargs, const float* fargs, const uint8_t* luts, int out_dtype,
                                       const float* mean_std, void* stream) {
  EDET_CHECK(src && dst && mean_std, "edet_randaug_apply_norm: null pointer");
  EDET_CHECK(!ops || (iargs && fargs && luts), "edet_randaug_apply_norm: ops without iargs / fargs / luts");
  EDET_CHECK((const void*)src != dst, "edet_randaug_apply_norm: in place (the geometric operations and Sharpness read neighbours)");
  EDET_CHECK(batch > 0 && batch <= 65535 && height > 0 && width > 0, "edet_randaug_apply_norm: batch %d, image %d x %d", batch,
             height, width);
  EDET_CHECK((int64_t)height * width * 3 < (int64_t)1 << 31, "edet_randaug_apply_norm: image %d x %d too large", height, width);
  for (int c = 0; c < 3; ++c)
    EDET_CHECK(mean_std[3 + c] != 0.f && mean_std[3 + c] == mean_std[3 + c] && mean_std[c] == mean_std[c],
               "edet_randaug_apply_norm: mean %g, std %g of channel %d", mean_std[c], mean_std[3 + c], c);
  hipStream_t st = to_stream(stream);
  if (out_dtype == OUT_U8) launch_apply_norm<uint8_t>(src, dst, batch, height, width, ops, iargs, fargs, luts, mean_std, st);
  else if (out_dtype == EDET_F32) launch_apply_norm<float>(src, dst, batch, height, width, ops, iargs, fargs, luts, mean_std, st);
  else if (out_dtype == EDET_BF16) launch_apply_norm<bf16_t>(src, dst, batch, height, width, ops, iargs, fargs, luts, mean_std, st);
  else EDET_CHECK(false, "edet_randaug_apply_norm: bad out_dtype %d", out_dtype);
  EDET_LAUNCH_CHECK("edet_randaug_apply_norm");
  return 0;
}

extern "C" int edet_randaug_stats_canvas(const uint8_t* src, int batch, int canvas_h, int canvas_w, const int32_t* sizes_dev,
                                         const int32_t* ops, uint8_t* luts, void* stream) {
  EDET_CHECK(src && sizes_dev && ops && luts, "edet_randaug_stats_canvas: null pointer");
  EDET_CHECK(batch > 0 && canvas_h > 0 && canvas_w > 0, "edet_randaug_stats_canvas: batch %d, canvas %d x %d", batch, canvas_h,
             canvas_w);
  EDET_CHECK((int64_t)canvas_h * canvas_w * 3 < (int64_t)1 << 31, "edet_randaug_stats_canvas: canvas %d x %d too large", canvas_h,
             canvas_w);
  edet_launch(k_randaug_stats_canvas, dim3(batch), dim3(THREADS), 0, to_stream(stream), src, canvas_h, canvas_w, sizes_dev, ops,
              luts);
  EDET_LAUNCH_CHECK("edet_randaug_stats_canvas");
  return 0;
}

extern "C" int edet_randaug_apply_canvas(const uint8_t* src, void* dst, int batch, int canvas_h, int canvas_w,
                                         const int32_t* sizes_dev, const int32_t* ops, const int32_t* iargs, const float* fargs,
                                         const uint8_t* luts, int out_dtype, void* stream) {
  EDET_CHECK(src && dst && sizes_dev, "edet_randaug_apply_canvas: null pointer");
  EDET_CHECK(!ops || (iargs && fargs && luts), "edet_randaug_apply_canvas: ops without iargs / fargs / luts");
  EDET_CHECK((const void*)src != dst, "edet_randaug_apply_canvas: in place (the geometric operations and Sharpness read neighbours)");
  EDET_CHECK(batch > 0 && batch <= 65535 && canvas_h > 0 && canvas_w > 0, "edet_randaug_apply_canvas: batch %d, canvas %d x %d",
             batch, canvas_h, canvas_w);
  EDET_CHECK((int64_t)canvas_h * canvas_w * 3 < (int64_t)1 << 31, "edet_randaug_apply_canvas: canvas %d x %d too large", canvas_h,
             canvas_w);
  hipStream_t st = to_stream(stream);
  if (out_dtype == OUT_U8) launch_apply_canvas<uint8_t>(src, dst, batch, canvas_h, canvas_w, sizes_dev, ops, iargs, fargs, luts, st);
  else if (out_dtype == EDET_F32) launch_apply_canvas<float>(src, dst, batch, canvas_h, canvas_w, sizes_dev, ops, iargs, fargs, luts, st);
  else if (out_dtype == EDET_BF16) launch_apply_canvas<bf16_t>(src, dst, batch, canvas_h, canvas_w, sizes_dev, ops, iargs, fargs, luts, st);
  else EDET_CHECK(false, "edet_randaug_apply_canvas: bad out_dtype %d", out_dtype);
  EDET_LAUNCH_CHECK("edet_randaug_apply_canvas");
  return 0;
}
