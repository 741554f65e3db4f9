// The colour stage of the JPEG decoder for a crop window (include/edet_hip.h, "JPEG decode of a crop window";
// tf.image.decode_and_crop_jpeg).  The host stage stores only the blocks a window needs -- the kept grid, a rectangle of whole
// MCUs -- and describes it as an image of its own, so the inverse DCT of a windowed batch is edet_jpeg_idct_scaled
// (jpeg_scaled.hip) as it is.  k_jpeg_color_window is k_jpeg_color_scaled's contract with an origin: canvas pixel (r, q) of a
// slot is image pixel (y + r, x + q), the samples are read from the kept planes at their place minus the kept grid's first
// sample, and every edge rule of the up-sampling is the WHOLE image's.  Integer arithmetic only, restated in
// tests/jpeg_window_ref.py and compared byte for byte.  One launch per batch whatever mix of samplings, ratios and windows it
// holds: everything per image is read from its two descriptors in device memory.
#include "common.h"
#include "jpeg_impl.h"

namespace {

using namespace jpeg_impl;

constexpr int COLOR_THREADS = 256;

// The samples [from, to] of a component that output pixels first .. last need along one axis (the header's kept grid): u the
// up-sampling left along it, real the component's real samples.
__device__ __forceinline__ void needed(int first, int last, int u, int real, int& from, int& to) {
  from = first;
  to = last;
  if (u == 2) {
    from = max((first >> 1) - 1, 0);
    to = min((last >> 1) + 1, real - 1);
  }
}

// The up-sampling that is left for the chroma, h_max s_0 / s_1 and v_max s_0 / s_1 without the divisions: (1, 1), (2, 1) or
// (2, 2) -- the chroma of a 4:2:0 file below full size lies at the output's resolution.
__device__ __forceinline__ void chroma_factors(const edet_jpeg_image_t& d, int m, int& fh, int& fv) {
  const bool doubled = d.h_max == 2 && d.v_max == 2 && m < 8;
  fh = doubled ? 1 : d.h_max;
  fv = doubled ? 1 : d.v_max;
}

// Could the host stage have written this pair of descriptors, and does everything the kernel reads with them lie inside the
// kept planes?  d passes scaled_ok, so its planes lie inside the arena; the window lies inside the image and the canvas; the
// block grids are those of mcus_w x mcus_h MCUs; and per component and axis the needed samples minus the kept grid's first
// sample fall inside the plane.  The same in every lane of an image.
__device__ __forceinline__ bool window_ok(const edet_jpeg_image_t& d, const edet_jpeg_window_t& w, int64_t cap_blocks,
                                          int canvas_h, int canvas_w) {
  if (!scaled_ok(d, cap_blocks)) return false;
  if (w.image_h < 1 || w.image_h > 65535 || w.image_w < 1 || w.image_w > 65535) return false;
  if (w.y < 0 || w.x < 0 || w.h < 1 || w.w < 1 || w.h > w.image_h - w.y || w.w > w.image_w - w.x) return false;
  if (w.h > canvas_h || w.w > canvas_w) return false;
  if (w.mcu_x0 < 0 || w.mcu_x0 > 8192 || w.mcu_y0 < 0 || w.mcu_y0 > 8192 || w.mcus_w < 1 || w.mcus_w > 8192 ||
      w.mcus_h < 1 || w.mcus_h > 8192)
    return false;
  const int m = scaled_m(d), s0 = sample_size(d, m, 0);
  // luma: h_max x v_max blocks of s0 samples in an MCU, never up-sampled
  if (d.blocks_w[0] != w.mcus_w * d.h_max || d.blocks_h[0] != w.mcus_h * d.v_max) return false;      // (factors <= 8192)
  const int lx = w.x - w.mcu_x0 * d.h_max * s0, ly = w.y - w.mcu_y0 * d.v_max * s0;
  if (lx < 0 || lx + w.w > d.blocks_w[0] * s0 || ly < 0 || ly + w.h > d.blocks_h[0] * s0) return false;
  if (d.components == 1) return true;
  // chroma: one block of s1 samples in an MCU
  if (d.blocks_w[1] != w.mcus_w || d.blocks_w[2] != w.mcus_w || d.blocks_h[1] != w.mcus_h || d.blocks_h[2] != w.mcus_h)
    return false;
  const int s1 = sample_size(d, m, 1);
  int fh, fv, from, to;
  chroma_factors(d, m, fh, fv);
  needed(w.x, w.x + w.w - 1, fh, fh == 2 ? (w.image_w + 1) >> 1 : w.image_w, from, to);
  if (from - w.mcu_x0 * s1 < 0 || to - w.mcu_x0 * s1 >= w.mcus_w * s1) return false;
  needed(w.y, w.y + w.h - 1, fv, fv == 2 ? (w.image_h + 1) >> 1 : w.image_h, from, to);
  return from - w.mcu_y0 * s1 >= 0 && to - w.mcu_y0 * s1 < w.mcus_h * s1;
}

// `count` (1 .. 4) samples of a plane row from byte `at` of the planes: one word where that is aligned and the row holds all
// four (its stride a multiple of four, the first column too), else byte by byte
__device__ __forceinline__ void load4(const uint8_t* __restrict__ planes, size_t at, bool word, int count, int out[4]) {
  if (word) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(planes + at);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = (int)((v >> (8 * j)) & 0xFF);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = j < count ? (int)planes[at + j] : 0;
  }
}

template <bool VEC>
__global__ __launch_bounds__(COLOR_THREADS) void k_jpeg_color_window(const uint8_t* __restrict__ planes,
                                                                    const edet_jpeg_image_t* __restrict__ images,
                                                                    const edet_jpeg_window_t* __restrict__ windows,
                                                                    int canvas_h, int canvas_w, int64_t cap_blocks,
                                                                    uint8_t* __restrict__ raw) {
  const int img = blockIdx.y;
  const int groups = (canvas_w + 3) >> 2;
  const int64_t idx = (int64_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
  if (idx >= (int64_t)groups * canvas_h) return;
  const int r = (int)(idx / groups), q0 = (int)(idx - (int64_t)r * groups) * 4;
  const edet_jpeg_image_t d = images[img];
  const edet_jpeg_window_t w = windows[img];
  uint32_t rgb[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j) rgb[j][0] = rgb[j][1] = rgb[j][2] = 0;
  if (r < w.h && q0 < w.w && window_ok(d, w, cap_blocks, canvas_h, canvas_w)) {      // (outside the window: zeros, unchecked)
    const int m = scaled_m(d), s0 = sample_size(d, m, 0);
    const int y = w.y + r, x0 = w.x + q0;      // the thread's pixels in the image
    const int count = min(w.w - q0, 4);
    const int pw0 = d.blocks_w[0] * s0;
    const int lx = x0 - w.mcu_x0 * d.h_max * s0, ly = y - w.mcu_y0 * d.v_max * s0;      // in the kept luma plane
    int yy[4], cb[4], cr[4];
    // every plane starts on a 64-byte boundary, so a word is aligned where its row stride and its column are multiples of 4
    load4(planes, (size_t)d.first_block[0] * 64 + (size_t)ly * pw0 + lx, ((pw0 | lx) & 3) == 0, count, yy);
    if (d.components == 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) cb[j] = cr[j] = 128;
    } else {
      const int s1 = sample_size(d, m, 1);
      const int pw = d.blocks_w[1] * s1;
      int fh, fv;
      chroma_factors(d, m, fh, fv);
      const int ox = w.mcu_x0 * s1, oy = w.mcu_y0 * s1;      // the first kept chroma sample (one block per MCU)
      const size_t pb = (size_t)d.first_block[1] * 64, pr = (size_t)d.first_block[2] * 64;
      if (fh == 1) {
        const size_t at = (size_t)(y - oy) * pw + (x0 - ox);
        const bool word = ((pw | (x0 - ox)) & 3) == 0;
        load4(planes, pb + at, word, count, cb);
        load4(planes, pr + at, word, count, cr);
      } else {
        const int n = (w.image_w + 1) >> 1, rows = fv == 2 ? (w.image_h + 1) >> 1 : w.image_h;      // the component's real samples
        if (m > 1 && n > 2) {      // jdsample.c: fancy upsampling only above 1/8 and for more than two columns
          chroma4_window(planes + pb, pw, ox, oy, n, rows, fv == 2, y, x0, cb);
          chroma4_window(planes + pr, pw, ox, oy, n, rows, fv == 2, y, x0, cr);
        } else {
          const size_t at = (size_t)((fv == 2 ? y >> 1 : y) - oy) * pw;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int i = min(min((x0 + j) >> 1, n - 1) - ox, pw - 1);      // (>= 0: x0 is inside the window)
            cb[j] = planes[pb + at + i];
            cr[j] = planes[pr + at + i];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < count) {
        const int b = cb[j] - 128, c = cr[j] - 128;
        rgb[j][0] = (uint32_t)clamp255(yy[j] + ((91881 * c + 32768) >> 16));
        rgb[j][1] = (uint32_t)clamp255(yy[j] + ((-22554 * b - 46802 * c + 32768) >> 16));
        rgb[j][2] = (uint32_t)clamp255(yy[j] + ((116130 * b + 32768) >> 16));
      }
    }
  }
  uint8_t* dst = raw + (((size_t)img * canvas_h + r) * canvas_w + q0) * 3;
  if (VEC) {      // canvas_w % 4 == 0 and raw 4-byte aligned: twelve bytes as three words
    uint32_t* o = reinterpret_cast<uint32_t*>(dst);
    o[0] = rgb[0][0] | (rgb[0][1] << 8) | (rgb[0][2] << 16) | (rgb[1][0] << 24);
    o[1] = rgb[1][1] | (rgb[1][2] << 8) | (rgb[2][0] << 16) | (rgb[2][1] << 24);
    o[2] = rgb[2][2] | (rgb[3][0] << 8) | (rgb[3][1] << 16) | (rgb[3][2] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (q0 + j < canvas_w) {
        dst[3 * j] = (uint8_t)rgb[j][0];
        dst[3 * j + 1] = (uint8_t)rgb[j][1];
        dst[3 * j + 2] = (uint8_t)rgb[j][2];
      }
    }
  }
}

}  // namespace

extern "C" int edet_jpeg_color_window(const uint8_t* planes, const edet_jpeg_image_t* images_dev,
                                      const edet_jpeg_window_t* windows_dev, int batch, int canvas_h, int canvas_w,
                                      size_t plane_capacity, uint8_t* raw, void* stream) {
  EDET_CHECK(planes && images_dev && windows_dev && raw, "edet_jpeg_color_window: null pointer");
  EDET_CHECK(batch >= 1 && batch <= 65535 && canvas_h >= 1 && canvas_w >= 1 &&
                 (int64_t)canvas_h * canvas_w * 3 < ((int64_t)1 << 31),
             "edet_jpeg_color_window: batch %d (1..65535), canvas %d x %d", batch, canvas_h, canvas_w);
  EDET_CHECK(((uintptr_t)planes & 7) == 0 && ((uintptr_t)windows_dev & 3) == 0,
             "edet_jpeg_color_window: planes must be 8-byte aligned, windows_dev 4-byte aligned");
  const int64_t work = (int64_t)((canvas_w + 3) / 4) * canvas_h;
  const dim3 grid((unsigned)cdiv(work, COLOR_THREADS), (unsigned)batch);
  const int64_t cap = (int64_t)(plane_capacity / 64);
  if (canvas_w % 4 == 0 && ((uintptr_t)raw & 3) == 0)
    edet_launch(k_jpeg_color_window<true>, grid, dim3(COLOR_THREADS), 0, to_stream(stream), planes, images_dev, windows_dev,
                canvas_h, canvas_w, cap, raw);
  else
    edet_launch(k_jpeg_color_window<false>, grid, dim3(COLOR_THREADS), 0, to_stream(stream), planes, images_dev, windows_dev,
                canvas_h, canvas_w, cap, raw);
  EDET_LAUNCH_CHECK("edet_jpeg_color_window");
  return 0;
}
