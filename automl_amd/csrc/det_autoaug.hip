// What makes the detector's AutoAugment / RandAugment box-aware (efficientdet/aug/autoaugment.py): the boxes follow the
// geometric operations, BBox_Cutout places its rectangle from a box in device memory, and Contrast blends with the true mean
// grey level.  The image operations themselves are edet_randaug_stats / edet_randaug_apply (randaug.hip), unchanged: the
// two kernels here write what those read.
//
//   edet_autoaug_boxes          one layer, one thread per box row: _rotate_bbox (:785-835), _shift_bbox (:881-919),
//                               _shear_bbox (:978-1025) with _clip_bbox / _check_bbox_area (:435-483); for BBox_Cutout the
//                               rectangle of _cutout_inside_bbox (:1245-1281) -> that image's iargs row, Cutout's layout
//   edet_autoaug_contrast_lut   contrast (:267-280): exact integer sum of the grey levels -> mean -> a 3 x 256 table of
//                               blend(mean, v, factor), and the image's apply id becomes the table look-up (Equalize's)
//
// The policy operation per image and layer and every argument are the caller's, in device memory, so the launch sequence never
// depends on the draws.  Every box is compared bit for bit with a numpy restatement (tests/det_autoaug_ref.py): this file is
// compiled with -ffp-contract=off (automl_amd/build.py), every product, sum and quotient below is a single rounded fp32
// operation in the order written, to_int32 truncates.  No trigonometry here: Rotate's cosine and sine are the image
// coefficients fargs[0] and fargs[3], made on the host.
#include "common.h"
#include "randaug_impl.h"

namespace {

using raug::blend;
using raug::clampi;
using raug::clip_u8;
using raug::gray_of;

constexpr int THREADS = 256;
// policy operation ids: NAME_TO_FUNC (:1350-1372) without the *_Only_BBoxes family, in its order
constexpr int AA_CONTRAST = 6, AA_BBOX_CUTOUT = 10, AA_ROTATE = 11, AA_TRANSLATE_X = 12, AA_TRANSLATE_Y = 13, AA_SHEAR_X = 14,
              AA_SHEAR_Y = 15;
constexpr int APPLY_LUT = 1;      // OP_EQUALIZE of randaug.hip: out = lut[c][v]

// tf.to_int32: truncation.  (The clamp keeps a box that is not finite or absurdly large away from an undefined conversion;
// it changes no value below 2^30.)
__device__ __forceinline__ int to_i32(float t) { return (int)fminf(fmaxf(t, -1073741824.f), 1073741824.f); }
// clip_by_value as min(max(t, 0), 1) with each of them a compare and select: -0.0 (Rotate makes it: -(0.5 - 0.5)) stays -0.0
__device__ __forceinline__ float clip01(float t) {
  t = t < 0.f ? 0.f : t;
  return t > 1.f ? 1.f : t;
}

struct Box { float y0, x0, y1, x1; };

// _clip_bbox then _check_bbox_area with delta = 0.05 (:435-483)
__device__ __forceinline__ Box clip_and_check(Box b) {
  b.y0 = clip01(b.y0); b.x0 = clip01(b.x0); b.y1 = clip01(b.y1); b.x1 = clip01(b.x1);
  if (b.y1 - b.y0 == 0.f) {
    b.y1 = fmaxf(b.y1, 0.05f);
    b.y0 = fminf(b.y0, 0.95f);
  }
  if (b.x1 - b.x0 == 0.f) {
    b.x1 = fmaxf(b.x1, 0.05f);
    b.x0 = fminf(b.x0, 0.95f);
  }
  return b;
}

// one entry of the 2 x 4 matrix product: two rounded products, one rounded add
__device__ __forceinline__ int dot_i32(float a, float y, float b, float x) { return to_i32(__fadd_rn(__fmul_rn(a, y), __fmul_rn(b, x))); }

struct MinMax { int lo, hi; };
__device__ __forceinline__ MinMax minmax4(int a, int b, int c, int d) {
  return MinMax{min(min(a, b), min(c, d)), max(max(a, b), max(c, d))};
}

// the four corners (y, x) = (min_y, min_x), (min_y, max_x), (max_y, min_x), (max_y, max_x) through [[m00, m01], [m10, m11]]
__device__ __forceinline__ void corners(float m00, float m01, float m10, float m11, int iy0, int ix0, int iy1, int ix1,
                                        MinMax& r0, MinMax& r1) {
  const float y0 = (float)iy0, x0 = (float)ix0, y1 = (float)iy1, x1 = (float)ix1;
  r0 = minmax4(dot_i32(m00, y0, m01, x0), dot_i32(m00, y0, m01, x1), dot_i32(m00, y1, m01, x0), dot_i32(m00, y1, m01, x1));
  r1 = minmax4(dot_i32(m10, y0, m11, x0), dot_i32(m10, y0, m11, x1), dot_i32(m10, y1, m11, x0), dot_i32(m10, y1, m11, x1));
}

__device__ __forceinline__ Box rotate_box(Box b, float H, float W, float c, float s) {      // :785-835
  const int iy0 = -to_i32(H * (b.y0 - 0.5f)), ix0 = to_i32(W * (b.x0 - 0.5f));
  const int iy1 = -to_i32(H * (b.y1 - 0.5f)), ix1 = to_i32(W * (b.x1 - 0.5f));
  MinMax r0, r1;
  corners(c, s, -s, c, iy0, ix0, iy1, ix1, r0, r1);
  Box o;
  o.y0 = -((float)r0.hi / H - 0.5f);
  o.x0 = (float)r1.lo / W + 0.5f;
  o.y1 = -((float)r0.lo / H - 0.5f);
  o.x1 = (float)r1.hi / W + 0.5f;
  return clip_and_check(o);
}

__device__ __forceinline__ Box shift_box(Box b, int h, int w, float H, float W, float pixels_f, bool horizontal) {      // :881-919
  const int pixels = to_i32(pixels_f);
  int iy0 = to_i32(H * b.y0), ix0 = to_i32(W * b.x0), iy1 = to_i32(H * b.y1), ix1 = to_i32(W * b.x1);
  if (horizontal) {
    ix0 = max(0, ix0 - pixels);
    ix1 = min(w, ix1 - pixels);
  } else {
    iy0 = max(0, iy0 - pixels);
    iy1 = min(h, iy1 - pixels);
  }
  return clip_and_check(Box{(float)iy0 / H, (float)ix0 / W, (float)iy1 / H, (float)ix1 / W});
}

__device__ __forceinline__ Box shear_box(Box b, float H, float W, float level, bool horizontal) {      // :978-1025
  const int iy0 = to_i32(H * b.y0), ix0 = to_i32(W * b.x0), iy1 = to_i32(H * b.y1), ix1 = to_i32(W * b.x1);
  MinMax r0, r1;
  if (horizontal) corners(1.f, 0.f, -level, 1.f, iy0, ix0, iy1, ix1, r0, r1);
  else corners(1.f, -level, 0.f, 1.f, iy0, ix0, iy1, ix1, r0, r1);
  return clip_and_check(Box{(float)r0.lo / H, (float)r1.lo / W, (float)r0.hi / H, (float)r1.hi / W});
}

// tf.random_uniform(minval = lo, maxval = hi, dtype = int32) from a draw u in [0, 1): lo + floor(u (hi - lo)), below hi.
// (hi <= lo, which the reference would refuse, gives lo.)
__device__ __forceinline__ int draw_int(double u, int lo, int hi) {
  const int n = max(hi - lo, 1);
  return lo + clampi((int)floor(u * (double)n), 0, n - 1);
}

// Image `img` of height h and width w.  boxes / out: [batch][m][4], the same buffer or two.
__device__ __forceinline__ void boxes_image(const float* boxes, float* out, const int32_t* __restrict__ counts, int m, int h, int w,
                                            int img, const int32_t* __restrict__ policy, int32_t* __restrict__ iargs,
                                            const float* __restrict__ fargs, const double* __restrict__ dargs) {
  const int op = policy[img];
  const int count = clampi(counts[img], 0, m);
  const float H = (float)h, W = (float)w;
  const float* fa = fargs + (size_t)img * 8;
  const float* in = boxes + (size_t)img * m * 4;
  float* o = out + (size_t)img * m * 4;
  if (op == AA_BBOX_CUTOUT && threadIdx.x == 0) {      // :1245-1281, :1321-1345; the boxes stay as they are
    int rect[4] = {0, 0, 0, 0};      // no box: nothing is cut out (:1344)
    if (count > 0) {
      const double* da = dargs + (size_t)img * 4;      // {pad_fraction, box draw, centre draw y, centre draw x}
      const float* bx = in + (size_t)draw_int(da[1], 0, count) * 4;
      const int iy0 = to_i32(H * bx[0]), ix0 = to_i32(W * bx[1]), iy1 = to_i32(H * bx[2]), ix1 = to_i32(W * bx[3]);
      const int pad_h = (int)(da[0] * ((double)(iy1 - iy0 + 1) / 2.0));
      const int pad_w = (int)(da[0] * ((double)(ix1 - ix0 + 1) / 2.0));
      const int cy = draw_int(da[2], iy0, iy1 + 1), cx = draw_int(da[3], ix0, ix1 + 1);
      const int lower = max(0, cy - pad_h), upper = max(0, h - cy - pad_h);
      const int left = max(0, cx - pad_w), right = max(0, w - cx - pad_w);
      rect[0] = lower; rect[1] = left; rect[2] = h - upper; rect[3] = w - right;
    }
    for (int k = 0; k < 4; ++k) iargs[(size_t)img * 4 + k] = rect[k];
  }
  const bool moves = op >= AA_ROTATE && op <= AA_SHEAR_Y;
  if (!moves && in == o) return;      // (uniform over the workgroup)
  for (int r = threadIdx.x; r < m; r += THREADS) {
    const float4 v = reinterpret_cast<const float4*>(in)[r];
    Box b{v.x, v.y, v.z, v.w};
    if (moves && r < count) {      // rows at or past the count pass through
      if (op == AA_ROTATE) b = rotate_box(b, H, W, fa[0], fa[3]);
      else if (op == AA_TRANSLATE_X) b = shift_box(b, h, w, H, W, fa[2], true);
      else if (op == AA_TRANSLATE_Y) b = shift_box(b, h, w, H, W, fa[5], false);
      else if (op == AA_SHEAR_X) b = shear_box(b, H, W, fa[1], true);
      else b = shear_box(b, H, W, fa[3], false);
    }
    reinterpret_cast<float4*>(o)[r] = make_float4(b.y0, b.x0, b.y1, b.x1);
  }
}

__global__ __launch_bounds__(THREADS) void k_autoaug_boxes(const float* boxes, float* out,
                                                          const int32_t* __restrict__ counts, int m, int h, int w,
                                                          const int32_t* __restrict__ policy, int32_t* __restrict__ iargs,
                                                          const float* __restrict__ fargs, const double* __restrict__ dargs) {
  boxes_image(boxes, out, counts, m, h, w, blockIdx.x, policy, iargs, fargs, dargs);
}

constexpr int MAX_EXTENT = (1 << 24) - 1;      // what the dense entry point accepts: every pixel coordinate is exact in fp32
// The canvas batch: (h, w) = sizes[img], clamped (the boxes are normalised: no slot is indexed here, and a size is only a
// factor)
__global__ __launch_bounds__(THREADS) void k_autoaug_boxes_canvas(const float* boxes, float* out,
                                                                 const int32_t* __restrict__ counts, int m,
                                                                 const int32_t* __restrict__ sizes,
                                                                 const int32_t* __restrict__ policy, int32_t* __restrict__ iargs,
                                                                 const float* __restrict__ fargs, const double* __restrict__ dargs) {
  const int img = blockIdx.x;
  boxes_image(boxes, out, counts, m, clampi(sizes[2 * img], 1, MAX_EXTENT), clampi(sizes[2 * img + 1], 1, MAX_EXTENT), img, policy,
              iargs, fargs, dargs);
}

// The image at p of n = h w pixels, `pitch` pixels from row to row (dense: its pixels are consecutive and w is not used)
// -> its table.  vec: four pixels (three words) per thread and step; p starts on a word and, with CANVAS, w and pitch are
// multiples of 4.
constexpr int LUT_THREADS = 1024;
template <bool CANVAS>
__device__ __forceinline__ void contrast_image(const uint8_t* __restrict__ p, int n, int w, int pitch, bool vec, int img,
                                               int32_t* __restrict__ ops, const float* __restrict__ fargs,
                                               uint8_t* __restrict__ luts) {
  __shared__ unsigned long long part[LUT_THREADS];
  unsigned long long sum = 0;
  if (vec) {
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(p);
    for (int q = threadIdx.x; q < n / 4; q += LUT_THREADS) {
      int q3 = q * 3;
      if (CANVAS) {
        const int y = (q * 4) / w;
        q3 = ((y * pitch + (q * 4 - y * w)) >> 2) * 3;
      }
      const uint32_t a = pw[q3], b = pw[q3 + 1], c = pw[q3 + 2];
      sum += (unsigned)(gray_of(a & 255, (a >> 8) & 255, (a >> 16) & 255) + gray_of(a >> 24, b & 255, (b >> 8) & 255) +
                        gray_of((b >> 16) & 255, b >> 24, c & 255) + gray_of((c >> 8) & 255, (c >> 16) & 255, c >> 24));
    }
  } else {
    for (int i = threadIdx.x; i < n; i += LUT_THREADS) {
      size_t o = (size_t)i * 3;
      if (CANVAS) {
        const int y = i / w;
        o = (size_t)(y * pitch + (i - y * w)) * 3;
      }
      sum += (unsigned)gray_of(p[o], p[o + 1], p[o + 2]);
    }
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int s = LUT_THREADS / 2; s > 0; s >>= 1) {      // integers: exact in any order
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  const int mean = clip_u8((float)part[0] / (float)n);
  const float f = fargs[(size_t)img * 8 + 6];
  uint8_t* out = luts + (size_t)img * 768;
  if (threadIdx.x < 768) out[threadIdx.x] = (uint8_t)blend(mean, threadIdx.x & 255, f);
  if (threadIdx.x == 0) ops[img] = APPLY_LUT;
}

// blockIdx.x = the image; n = H W pixels.  The word path where every image starts on a word.
__global__ __launch_bounds__(LUT_THREADS) void k_autoaug_contrast_lut(const uint8_t* __restrict__ src, int n,
                                                                     const int32_t* __restrict__ policy, int32_t* __restrict__ ops,
                                                                     const float* __restrict__ fargs, uint8_t* __restrict__ luts) {
  const int img = blockIdx.x;
  if (policy[img] != AA_CONTRAST) return;      // (uniform over the workgroup)
  contrast_image<false>(src + (size_t)img * n * 3, n, 0, 0, n % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0, img, ops, fargs,
                        luts);
}

// The canvas batch: the grey levels of the h x w rectangle of the image's slot only, (h, w) = sizes[img] clamped into the
// slot.  An image as wide as the canvas has consecutive pixels, as in the dense batch.
__global__ __launch_bounds__(LUT_THREADS) void k_autoaug_contrast_lut_canvas(const uint8_t* __restrict__ src, int ch, int cw,
                                                                            const int32_t* __restrict__ sizes,
                                                                            const int32_t* __restrict__ policy,
                                                                            int32_t* __restrict__ ops, const float* __restrict__ fargs,
                                                                            uint8_t* __restrict__ luts) {
  const int img = blockIdx.x;
  if (policy[img] != AA_CONTRAST) return;      // (uniform over the workgroup)
  const int h = clampi(sizes[2 * img], 1, ch), w = clampi(sizes[2 * img + 1], 1, cw);
  const uint8_t* p = src + (size_t)img * ch * cw * 3;
  const bool word = reinterpret_cast<uintptr_t>(p) % 4 == 0;
  if (w == cw) contrast_image<false>(p, h * w, 0, 0, word && (h * w) % 4 == 0, img, ops, fargs, luts);
  else contrast_image<true>(p, h * w, w, cw, word && w % 4 == 0 && cw % 4 == 0, img, ops, fargs, luts);
}

}  // namespace

extern "C" int edet_autoaug_boxes(const float* boxes, float* boxes_out, const int32_t* counts, int batch, int max_boxes,
                                  int height, int width, const int32_t* policy, int32_t* iargs, const float* fargs,
                                  const double* dargs, void* stream) {
  EDET_CHECK(boxes && boxes_out && counts && policy && iargs && fargs && dargs, "edet_autoaug_boxes: null pointer");
  EDET_CHECK(batch > 0 && max_boxes > 0 && height > 0 && width > 0, "edet_autoaug_boxes: batch %d, %d box rows, image %d x %d",
             batch, max_boxes, height, width);
  EDET_CHECK(height < (1 << 24) && width < (1 << 24), "edet_autoaug_boxes: image %d x %d too large", height, width);
  EDET_CHECK(reinterpret_cast<uintptr_t>(boxes) % 16 == 0 && reinterpret_cast<uintptr_t>(boxes_out) % 16 == 0 &&
                 reinterpret_cast<uintptr_t>(dargs) % 8 == 0,
             "edet_autoaug_boxes: boxes need 16-byte, dargs 8-byte alignment");
  edet_launch(k_autoaug_boxes, dim3(batch), dim3(THREADS), 0, to_stream(stream), boxes, boxes_out, counts, max_boxes, height,
              width, policy, iargs, fargs, dargs);
  EDET_LAUNCH_CHECK("edet_autoaug_boxes");
  return 0;
}

extern "C" int edet_autoaug_contrast_lut(const uint8_t* src, int batch, int height, int width, const int32_t* policy,
                                         int32_t* ops, const float* fargs, uint8_t* luts, void* stream) {
  EDET_CHECK(src && policy && ops && fargs && luts, "edet_autoaug_contrast_lut: null pointer");
  EDET_CHECK(batch > 0 && height > 0 && width > 0, "edet_autoaug_contrast_lut: batch %d, image %d x %d", batch, height, width);
  EDET_CHECK((int64_t)height * width * 3 < (int64_t)1 << 31, "edet_autoaug_contrast_lut: image %d x %d too large", height, width);
  edet_launch(k_autoaug_contrast_lut, dim3(batch), dim3(LUT_THREADS), 0, to_stream(stream), src, height * width, policy, ops, fargs,
              luts);
  EDET_LAUNCH_CHECK("edet_autoaug_contrast_lut");
  return 0;
}

extern "C" int edet_autoaug_boxes_canvas(const float* boxes, float* boxes_out, const int32_t* counts, int batch, int max_boxes,
                                         const int32_t* sizes_dev, const int32_t* policy, int32_t* iargs, const float* fargs,
                                         const double* dargs, void* stream) {
  EDET_CHECK(boxes && boxes_out && counts && sizes_dev && policy && iargs && fargs && dargs,
             "edet_autoaug_boxes_canvas: null pointer");
  EDET_CHECK(batch > 0 && max_boxes > 0, "edet_autoaug_boxes_canvas: batch %d, %d box rows", batch, max_boxes);
  EDET_CHECK(reinterpret_cast<uintptr_t>(boxes) % 16 == 0 && reinterpret_cast<uintptr_t>(boxes_out) % 16 == 0 &&
                 reinterpret_cast<uintptr_t>(dargs) % 8 == 0,
             "edet_autoaug_boxes_canvas: boxes need 16-byte, dargs 8-byte alignment");
  edet_launch(k_autoaug_boxes_canvas, dim3(batch), dim3(THREADS), 0, to_stream(stream), boxes, boxes_out, counts, max_boxes,
              sizes_dev, policy, iargs, fargs, dargs);
  EDET_LAUNCH_CHECK("edet_autoaug_boxes_canvas");
  return 0;
}

extern "C" int edet_autoaug_contrast_lut_canvas(const uint8_t* src, int batch, int canvas_h, int canvas_w,
                                                const int32_t* sizes_dev, const int32_t* policy, int32_t* ops, const float* fargs,
                                                uint8_t* luts, void* stream) {
  EDET_CHECK(src && sizes_dev && policy && ops && fargs && luts, "edet_autoaug_contrast_lut_canvas: null pointer");
  EDET_CHECK(batch > 0 && canvas_h > 0 && canvas_w > 0, "edet_autoaug_contrast_lut_canvas: batch %d, canvas %d x %d", batch,
             canvas_h, canvas_w);
  EDET_CHECK((int64_t)canvas_h * canvas_w * 3 < (int64_t)1 << 31, "edet_autoaug_contrast_lut_canvas: canvas %d x %d too large",
             canvas_h, canvas_w);
  edet_launch(k_autoaug_contrast_lut_canvas, dim3(batch), dim3(LUT_THREADS), 0, to_stream(stream), src, canvas_h, canvas_w,
              sizes_dev, policy, ops, fargs, luts);
  EDET_LAUNCH_CHECK("edet_autoaug_contrast_lut_canvas");
  return 0;
}
