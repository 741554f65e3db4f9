// Mosaic augmentation on the device (efficientdet/aug/mosaic.py): four decoded uint8 images, each resized WHOLE to one
// quadrant of the output around the divide points (x, y) -- x splits the rows, y the columns, the reference's names --
//
//        columns [0, y)          columns [y, out_w)
//   rows [0, x)       image 0 -> x by y          image 2 -> x by (out_w - y)
//   rows [x, out_h)   image 1 -> (out_h - x) by y   image 3 -> the rest
//
// (mosaic.py:115-128 and the concatenations of :246-250: image 1 lies BELOW image 0, whatever its variable is called).
//
//   edet_mosaic        `groups` mosaics in one launch from a canvas batch; the four source indices, the divide points and the
//                      sources' sizes come from device memory (edet_mosaic_t), so the launch depends on (groups, out_h,
//                      out_w, dtype) alone and a replayed graph sees new draws
//   edet_mosaic_boxes  the batch form's boxes: the valid rows of the four sources in order, moved into their quadrants
//
// Every pixel is edet_crop_resize's arithmetic for "resize the whole source to the quadrant's size" at the quadrant-local
// coordinate (resize_tap.h), compared bit for bit with tests/mosaic_ref.py: this file is compiled with -ffp-contract=off.
//
// The store pattern is k_crop_resize's: a thread owns four consecutive pixels of one output row, stored as three 4-element
// vectors where out_w % 4 == 0 and `out` is 16-byte aligned.  A row lies in two quadrants, so a thread prepares the y-taps of
// BOTH sources of its row (they are the same for the whole wave: one wave = one row) and every pixel of its run picks its
// side by column < y: the run that straddles the seam takes its left pixels from one source and its right pixels from the
// other.  No LDS, no atomics.
#include "resize_tap.h"

namespace {

using resize_tap::clampi;

constexpr int THREADS = 256;      // 4 waves = 4 output rows of 256 pixels
constexpr int RUN = 4;            // output pixels per thread
constexpr int OUT_U8 = 2;         // EDET_U8

template <typename T> __device__ __forceinline__ T out_of(float v);
// clip to [0, 255], then a truncating cast (the rule of edet_crop_resize's EDET_U8)
template <> __device__ __forceinline__ uint8_t out_of<uint8_t>(float v) { return (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f); }
// the reference returns tf.image.resize's float32 values as they are
template <> __device__ __forceinline__ float out_of<float>(float v) { return v; }

// what a row's pixels on one side of the column seam need: the source's two tap rows, its width and the column scale
struct Side {
  size_t row_lo, row_hi;
  float ly, xscale;
  int width;
};

// the source image `index` of `height` x `width` resized to qh x qw: the taps of quadrant-local row `r`
__device__ __forceinline__ Side side_of(int index, int height, int width, int batch, int canvas_h, int canvas_w, int r, int qh,
                                        int qw) {
  // nothing in device memory may send an access outside the batch or the image (automl_amd/mosaic.clamp_rows states the same)
  index = clampi(index, 0, batch - 1);
  height = clampi(height, 1, canvas_h);
  width = clampi(width, 1, canvas_w);
  const resize_tap::Axis ty = resize_tap::axis_of(r, (float)height / (float)qh, height);
  const size_t image = (size_t)index * canvas_h * canvas_w;
  Side s;
  s.row_lo = (image + (size_t)ty.lo * canvas_w) * 3;
  s.row_hi = (image + (size_t)ty.hi * canvas_w) * 3;
  s.ly = ty.t;
  s.xscale = (float)width / (float)qw;
  s.width = width;
  return s;
}

// grid: x = stretches of 256 pixels of a row, y = groups of 4 rows, z = the mosaic.  VEC as in k_crop_resize.
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void k_mosaic(const uint8_t* __restrict__ raw, int batch, int canvas_h, int canvas_w,
                                                   size_t total, const edet_mosaic_t* __restrict__ per, T* __restrict__ out,
                                                   int out_h, int out_w) {
  const int c0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * RUN;
  const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int g = blockIdx.z;
  if (c0 >= out_w || r >= out_h) return;
  const edet_mosaic_t p = per[g];
  const int x = clampi(p.x, 1, out_h - 1), y = clampi(p.y, 1, out_w - 1);
  const bool upper = r < x;
  const int qh = upper ? x : out_h - x, lr = upper ? r : r - x;
  const Side left = side_of(upper ? p.index[0] : p.index[1], upper ? p.height[0] : p.height[1],
                            upper ? p.width[0] : p.width[1], batch, canvas_h, canvas_w, lr, qh, y);
  const Side right = side_of(upper ? p.index[2] : p.index[3], upper ? p.height[2] : p.height[3],
                             upper ? p.width[2] : p.width[3], batch, canvas_h, canvas_w, lr, qh, out_w - y);

  float v[RUN * 3];
#pragma unroll
  for (int e = 0; e < RUN; ++e) {
    const int c = min(c0 + e, out_w - 1);      // (a run that ends past the row repeats its last pixel and never stores it)
    const bool l = c < y;
    const int lc = l ? c : c - y;
    const size_t row_lo = l ? left.row_lo : right.row_lo, row_hi = l ? left.row_hi : right.row_hi;
    const resize_tap::Axis tx = resize_tap::axis_of(lc, l ? left.xscale : right.xscale, l ? left.width : right.width);
    resize_tap::pixel(raw, row_lo, row_hi, total, tx, l ? left.ly : right.ly, v + e * 3);
  }
  T* o = out + (((size_t)g * out_h + r) * out_w + c0) * 3;
  resize_tap::store_run<VEC>(o, v, min(RUN, out_w - c0), [](float f) { return out_of<T>(f); });
}

template <typename T>
void launch(const uint8_t* raw, int batch, int canvas_h, int canvas_w, const edet_mosaic_t* per, int groups, void* out,
            int out_h, int out_w, hipStream_t st) {
  const dim3 grid(cdiv(out_w, 64 * RUN), cdiv(out_h, 4), groups);
  const size_t total = (size_t)batch * canvas_h * canvas_w * 3;
  const bool vec = out_w % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  if (vec) edet_launch(k_mosaic<T, true>, grid, dim3(THREADS), 0, st, raw, batch, canvas_h, canvas_w, total, per, (T*)out, out_h, out_w);
  else edet_launch(k_mosaic<T, false>, grid, dim3(THREADS), 0, st, raw, batch, canvas_h, canvas_w, total, per, (T*)out, out_h, out_w);
}

// one thread per output row j of mosaic g: rows [0, n0) are source 0's, [n0, n0 + n1) source 1's, ...; the rest is -1
__global__ __launch_bounds__(THREADS) void k_mosaic_boxes(const float* __restrict__ boxes, const float* __restrict__ classes,
                                                         const int32_t* __restrict__ counts, int batch, int max_boxes,
                                                         const edet_mosaic_t* __restrict__ per, int groups, int out_h,
                                                         int out_w, float* __restrict__ boxes_out,
                                                         float* __restrict__ classes_out, int32_t* __restrict__ counts_out) {
  const int rows = 4 * max_boxes;
  const int t = blockIdx.x * THREADS + threadIdx.x;
  if (t >= groups * rows) return;
  const int g = t / rows, j = t - g * rows;
  const edet_mosaic_t p = per[g];
  const int x = clampi(p.x, 1, out_h - 1), y = clampi(p.y, 1, out_w - 1);
  int first = 0, src = -1, at = 0, quadrant = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int b = clampi(p.index[q], 0, batch - 1);
    const int n = clampi(counts[b], 0, max_boxes);
    if (src < 0 && j < first + n) {
      src = b;
      at = j - first;
      quadrant = q;
    }
    first += n;
  }
  if (j == 0) counts_out[g] = first;
  float4 box = make_float4(-1.f, -1.f, -1.f, -1.f);
  float cls = -1.f;
  if (src >= 0) {
    const bool below = quadrant & 1, rightward = quadrant >= 2;
    const float oy = below ? (float)x : 0.f, ox = rightward ? (float)y : 0.f;
    const float qh = (float)(below ? out_h - x : x), qw = (float)(rightward ? out_w - y : y);
    const float4 in = reinterpret_cast<const float4*>(boxes)[(size_t)src * max_boxes + at];
    box.x = (oy + in.x * qh) / (float)out_h;
    box.y = (ox + in.y * qw) / (float)out_w;
    box.z = (oy + in.z * qh) / (float)out_h;
    box.w = (ox + in.w * qw) / (float)out_w;
    cls = classes[(size_t)src * max_boxes + at];
  }
  reinterpret_cast<float4*>(boxes_out)[t] = box;
  classes_out[t] = cls;
}

}  // namespace

extern "C" int edet_mosaic(const uint8_t* raw, int batch, int canvas_h, int canvas_w, const edet_mosaic_t* per_mosaic_dev,
                           int groups, void* out, int out_h, int out_w, int out_dtype, void* stream) {
  EDET_CHECK(raw && per_mosaic_dev && out, "edet_mosaic: null pointer");
  EDET_CHECK(batch >= 1 && canvas_h >= 1 && canvas_w >= 1 && groups >= 1 && groups <= 65535,
             "edet_mosaic: batch %d, canvas %d x %d, groups %d", batch, canvas_h, canvas_w, groups);
  EDET_CHECK(out_h >= 2 && out_w >= 2, "edet_mosaic: output %d x %d, want both >= 2", out_h, out_w);
  EDET_CHECK((int64_t)canvas_h * canvas_w * 3 < (int64_t)1 << 31, "edet_mosaic: canvas %d x %d too large", canvas_h, canvas_w);
  EDET_CHECK(cdiv(out_h, 4) <= 65535, "edet_mosaic: output %d x %d too tall", out_h, out_w);
  hipStream_t st = to_stream(stream);
  if (out_dtype == OUT_U8) launch<uint8_t>(raw, batch, canvas_h, canvas_w, per_mosaic_dev, groups, out, out_h, out_w, st);
  else if (out_dtype == EDET_F32) launch<float>(raw, batch, canvas_h, canvas_w, per_mosaic_dev, groups, out, out_h, out_w, st);
  else EDET_CHECK(false, "edet_mosaic: bad out_dtype %d", out_dtype);
  EDET_LAUNCH_CHECK("edet_mosaic");
  return 0;
}

extern "C" int edet_mosaic_boxes(const float* boxes, const float* classes, const int32_t* counts, int batch, int max_boxes,
                                 const edet_mosaic_t* per_mosaic_dev, int groups, int out_h, int out_w, float* boxes_out,
                                 float* classes_out, int32_t* counts_out, void* stream) {
  EDET_CHECK(boxes && classes && counts && per_mosaic_dev && boxes_out && classes_out && counts_out,
             "edet_mosaic_boxes: null pointer");
  EDET_CHECK(batch >= 1 && max_boxes >= 1 && groups >= 1, "edet_mosaic_boxes: batch %d, max_boxes %d, groups %d", batch,
             max_boxes, groups);
  EDET_CHECK(out_h >= 2 && out_w >= 2, "edet_mosaic_boxes: output %d x %d, want both >= 2", out_h, out_w);
  EDET_CHECK((int64_t)groups * 4 * max_boxes < (int64_t)1 << 31, "edet_mosaic_boxes: groups %d x 4 x max_boxes %d too large",
             groups, max_boxes);
  EDET_CHECK(reinterpret_cast<uintptr_t>(boxes) % 16 == 0 && reinterpret_cast<uintptr_t>(boxes_out) % 16 == 0,
             "edet_mosaic_boxes: boxes and boxes_out must be 16-byte aligned");
  edet_launch(k_mosaic_boxes, dim3(cdiv((int64_t)groups * 4 * max_boxes, THREADS)), dim3(THREADS), 0, to_stream(stream), boxes,
              classes, counts, batch, max_boxes, per_mosaic_dev, groups, out_h, out_w, boxes_out, classes_out, counts_out);
  EDET_LAUNCH_CHECK("edet_mosaic_boxes");
  return 0;
}
