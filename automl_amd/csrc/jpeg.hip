// The device stage of the JPEG decoder (include/edet_hip.h, "baseline JPEG decode"): what libjpeg does behind its Huffman
// decoder, on the coefficients csrc/jpeg_host.cpp leaves.  Integer arithmetic only (no floating point anywhere in this file),
// restated in tests/jpeg_ref.py and compared byte for byte.  Two kernels, one launch each per batch whatever the images' sizes
// and samplings are: the per-image descriptors and quantisation tables are read from device memory.
//
// k_jpeg_idct: eight lanes per 8x8 block, eight blocks per wave, 32 per workgroup; blockIdx.y is the image.  Lane r of a block
// loads coefficient row r (one 16-byte load) and its table row, multiplies, and hands the row to LDS; it takes column r back,
// runs jidctint.c's column pass on it, returns the column to the same LDS cells and takes row r of the result, runs the row
// pass and stores its eight samples with one 8-byte store.  The LDS tile of a block is 8 rows of 9 words, so that both the
// row and the column accesses of the eight lanes fall in different banks.  Sums, products and left shifts are unsigned and
// wrap; the right shifts are arithmetic.
//
// k_jpeg_color: one thread per four pixels of a canvas row; blockIdx.y is the image.  It writes the whole canvas: zero outside
// the image, zero everywhere for an image that was refused or whose descriptor does not fit the arenas.
#include "common.h"
#include "jpeg_impl.h"

namespace {

using namespace jpeg_impl;

constexpr int IDCT_THREADS = 256;
constexpr int IDCT_BLOCKS = IDCT_THREADS / 8;
constexpr int COLOR_THREADS = 256;

__global__ __launch_bounds__(IDCT_THREADS) void k_jpeg_idct(const int16_t* __restrict__ coef,
                                                            const edet_jpeg_image_t* __restrict__ images,
                                                            const uint16_t* __restrict__ qtables, int64_t cap_blocks,
                                                            uint8_t* __restrict__ planes) {
  __shared__ uint32_t tile[IDCT_BLOCKS][8][9];
  const int img = blockIdx.y;
  const edet_jpeg_image_t d = images[img];
  const int slot = threadIdx.x >> 3, r = threadIdx.x & 7;
  const int64_t g = (int64_t)blockIdx.x * IDCT_BLOCKS + slot;      // the block within the image
  const bool live = image_ok(d, cap_blocks) && g < d.total_blocks;      // (image_ok is the same in every lane)
  int c = 0, local = 0;
  if (live) {
    local = (int)g;
    while (c + 1 < d.components && local >= d.blocks_w[c] * d.blocks_h[c]) {
      local -= d.blocks_w[c] * d.blocks_h[c];
      ++c;
    }
  }
  uint32_t x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = 0;
  if (live) {
    const size_t at = ((size_t)d.first_block[0] + (size_t)g) * 64 + (size_t)r * 8;      // < 64 cap_blocks
    const uint4 cw = *reinterpret_cast<const uint4*>(coef + at);
    const uint4 qw = *reinterpret_cast<const uint4*>(qtables + ((size_t)img * 4 + d.quant_id[c]) * 64 + (size_t)r * 8);
    const uint32_t cv[4] = {cw.x, cw.y, cw.z, cw.w}, qv[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[2 * e] = (uint32_t)(int32_t)(int16_t)(cv[e] & 0xFFFFu) * (qv[e] & 0xFFFFu);
      x[2 * e + 1] = (uint32_t)((int32_t)cv[e] >> 16) * (qv[e] >> 16);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) tile[slot][r][e] = x[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = tile[slot][e][r];      // column r, top to bottom
  idct_1d(x, 11);
#pragma unroll
  for (int e = 0; e < 8; ++e) tile[slot][e][r] = x[e];      // the cells this lane alone read
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = tile[slot][r][e];
  idct_1d(x, 18);
  if (live) {
    uint32_t px[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) px[e] = (uint32_t)min(max((int32_t)x[e] + 128, 0), 255);
    uint2 o;
    o.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    o.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    const int bw = d.blocks_w[c], by = local / bw, bx = local - by * bw;
    const size_t to = (size_t)d.first_block[c] * 64 + ((size_t)by * 8 + r) * ((size_t)bw * 8) + (size_t)bx * 8;
    *reinterpret_cast<uint2*>(planes + to) = o;      // < 64 (first_block[c] + blocks of c) <= 64 cap_blocks
  }
}

template <bool VEC>
__global__ __launch_bounds__(COLOR_THREADS) void k_jpeg_color(const uint8_t* __restrict__ planes,
                                                             const edet_jpeg_image_t* __restrict__ images, int canvas_h,
                                                             int canvas_w, int64_t cap_blocks, uint8_t* __restrict__ raw) {
  const int img = blockIdx.y;
  const int groups = (canvas_w + 3) >> 2;
  const int64_t idx = (int64_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
  if (idx >= (int64_t)groups * canvas_h) return;
  const int y = (int)(idx / groups), x0 = (int)(idx - (int64_t)y * groups) * 4;
  const edet_jpeg_image_t d = images[img];
  uint32_t rgb[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j) rgb[j][0] = rgb[j][1] = rgb[j][2] = 0;
  if (image_ok(d, cap_blocks) && y < d.height && x0 < d.width) {
    // x0 + 3 < the plane's width: a multiple of 8 that is >= width > x0, and x0 is a multiple of 4
    const int pw0 = d.blocks_w[0] * 8;
    const uint8_t* py = planes + (size_t)d.first_block[0] * 64 + (size_t)y * pw0 + x0;
    const uint32_t yw = *reinterpret_cast<const uint32_t*>(py);      // 4-byte aligned: 64 first_block + y pw0 + x0
    int cb[4], cr[4];
    if (d.components == 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) cb[j] = cr[j] = 128;
    } else {
      const int pw = d.blocks_w[1] * 8;
      const uint8_t* pb = planes + (size_t)d.first_block[1] * 64;
      const uint8_t* pr = planes + (size_t)d.first_block[2] * 64;
      if (d.h_max == 1) {
        const uint32_t bw = *reinterpret_cast<const uint32_t*>(pb + (size_t)y * pw + x0);
        const uint32_t rw = *reinterpret_cast<const uint32_t*>(pr + (size_t)y * pw + x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          cb[j] = (int)((bw >> (8 * j)) & 0xFF);
          cr[j] = (int)((rw >> (8 * j)) & 0xFF);
        }
      } else {
        const int n = (d.width + 1) >> 1, rows = (d.height + d.v_max - 1) / d.v_max;
        chroma4(pb, pw, n, rows, d.v_max == 2, y, x0, cb);
        chroma4(pr, pw, n, rows, d.v_max == 2, y, x0, cr);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (x0 + j < d.width) {
        const int yy = (int)((yw >> (8 * j)) & 0xFF), b = cb[j] - 128, r = cr[j] - 128;
        rgb[j][0] = (uint32_t)clamp255(yy + ((91881 * r + 32768) >> 16));
        rgb[j][1] = (uint32_t)clamp255(yy + ((-22554 * b - 46802 * r + 32768) >> 16));
        rgb[j][2] = (uint32_t)clamp255(yy + ((116130 * b + 32768) >> 16));
      }
    }
  }
  uint8_t* dst = raw + (((size_t)img * canvas_h + y) * canvas_w + x0) * 3;
  if (VEC) {      // canvas_w % 4 == 0 and raw 4-byte aligned: twelve bytes as three words
    uint32_t* w = reinterpret_cast<uint32_t*>(dst);
    w[0] = rgb[0][0] | (rgb[0][1] << 8) | (rgb[0][2] << 16) | (rgb[1][0] << 24);
    w[1] = rgb[1][1] | (rgb[1][2] << 8) | (rgb[2][0] << 16) | (rgb[2][1] << 24);
    w[2] = rgb[2][2] | (rgb[3][0] << 8) | (rgb[3][1] << 16) | (rgb[3][2] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (x0 + j < canvas_w) {
        dst[3 * j] = (uint8_t)rgb[j][0];
        dst[3 * j + 1] = (uint8_t)rgb[j][1];
        dst[3 * j + 2] = (uint8_t)rgb[j][2];
      }
    }
  }
}

}  // namespace

extern "C" int edet_jpeg_idct(const int16_t* coef, const edet_jpeg_image_t* images_dev, const uint16_t* qtables_dev,
                              int batch, int max_blocks, uint8_t* planes, size_t plane_capacity, void* stream) {
  EDET_CHECK(coef && images_dev && qtables_dev && planes, "edet_jpeg_idct: null pointer");
  EDET_CHECK(batch >= 1 && batch <= 65535 && max_blocks >= 0, "edet_jpeg_idct: batch %d (1..65535), max_blocks %d", batch,
             max_blocks);
  EDET_CHECK(((uintptr_t)coef & 15) == 0 && ((uintptr_t)qtables_dev & 15) == 0 && ((uintptr_t)planes & 7) == 0,
             "edet_jpeg_idct: coef and qtables must be 16-byte aligned, planes 8-byte aligned");
  if (max_blocks == 0) return 0;
  edet_launch(k_jpeg_idct, dim3((unsigned)cdiv(max_blocks, IDCT_BLOCKS), (unsigned)batch), dim3(IDCT_THREADS), 0,
              to_stream(stream), coef, images_dev, qtables_dev, (int64_t)(plane_capacity / 64), planes);
  EDET_LAUNCH_CHECK("edet_jpeg_idct");
  return 0;
}

extern "C" int edet_jpeg_color(const uint8_t* planes, const edet_jpeg_image_t* images_dev, int batch, int canvas_h,
                               int canvas_w, size_t plane_capacity, uint8_t* raw, void* stream) {
  EDET_CHECK(planes && images_dev && raw, "edet_jpeg_color: null pointer");
  EDET_CHECK(batch >= 1 && batch <= 65535 && canvas_h >= 1 && canvas_w >= 1 && (int64_t)canvas_h * canvas_w * 3 < ((int64_t)1 << 31),
             "edet_jpeg_color: batch %d (1..65535), canvas %d x %d", batch, canvas_h, canvas_w);
  EDET_CHECK(((uintptr_t)planes & 7) == 0, "edet_jpeg_color: planes must be 8-byte aligned");
  const int64_t work = (int64_t)((canvas_w + 3) / 4) * canvas_h;
  const dim3 grid((unsigned)cdiv(work, COLOR_THREADS), (unsigned)batch);
  const int64_t cap = (int64_t)(plane_capacity / 64);
  if (canvas_w % 4 == 0 && ((uintptr_t)raw & 3) == 0)
    edet_launch(k_jpeg_color<true>, grid, dim3(COLOR_THREADS), 0, to_stream(stream), planes, images_dev, canvas_h, canvas_w,
                cap, raw);
  else
    edet_launch(k_jpeg_color<false>, grid, dim3(COLOR_THREADS), 0, to_stream(stream), planes, images_dev, canvas_h, canvas_w,
                cap, raw);
  EDET_LAUNCH_CHECK("edet_jpeg_color");
  return 0;
}
