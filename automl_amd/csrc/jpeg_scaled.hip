// The device stage of the JPEG decoder at libjpeg's reduced sizes (include/edet_hip.h, "JPEG decode at reduced size"):
// scale_denom 2, 4 and 8, which tf.io.decode_jpeg calls `ratio`.  The coefficients are the full-size ones
// (csrc/jpeg_host.cpp); a block is inverse-transformed straight to s x s samples, s = 8, 4, 2 or 1.  Integer arithmetic only,
// restated in tests/jpeg_scaled_ref.py and compared byte for byte.  Two kernels, one launch each per batch whatever mix of
// ratios, samplings and refusals it holds: everything per image is read from its descriptor in device memory, whose
// `reserved` field carries the denominator (0, which the full-size host entry point writes, reads as 1).
//
// k_jpeg_idct_scaled keeps k_jpeg_idct's shape (jpeg.hip): eight lanes per block, lane r loads coefficient row r with one
// 16-byte load, the transposes go through the same 8 x 9-word LDS tile.  s is the same in a block's eight lanes.  Lane r then
// takes column r; a column the reduced transform never reads (4 for s = 4; 2, 4 and 6 for s = 2) leaves its lane idle, as does
// a workspace row at or beyond s in the row pass.  s = 1 needs neither pass: lane 0 has the DC term in its own registers.  A
// block's row of s samples is stored with ONE store of s bytes -- the plane's row stride blocks_w s and the block's column bx s
// are multiples of s, and the plane starts on a 64-byte boundary, so that store is naturally aligned and never wider than the
// alignment allows.
//
// k_jpeg_color_scaled: k_jpeg_color's contract on planes of stride blocks_w s.  Four samples of a row are loaded as one word
// only where the stride is a multiple of four, else byte by byte (and only the bytes inside the image).
// scaled_m, sample_size and scaled_ok -- the denominator, the sample sizes and the descriptor check -- are jpeg_impl.h's,
// shared with jpeg_window.hip.
#include "common.h"
#include "jpeg_impl.h"

namespace {

using namespace jpeg_impl;

constexpr int IDCT_THREADS = 256;
constexpr int IDCT_BLOCKS = IDCT_THREADS / 8;
constexpr int COLOR_THREADS = 256;

// jidctred.c jpeg_idct_4x4, one pass: x[0 .. 3] and x[5 .. 7] in, x[0 .. 3] out; descale by n (12, then 19)
__device__ __forceinline__ void idct4_1d(uint32_t x[8], int n) {
  const uint32_t t0 = x[0] << 14;
  const uint32_t t2 = x[2] * 15137u + x[6] * (uint32_t)-6270;
  const uint32_t t10 = t0 + t2, t12 = t0 - t2;
  const uint32_t a = x[7] * (uint32_t)-1730 + x[5] * 11893u + x[3] * (uint32_t)-17799 + x[1] * 8697u;
  const uint32_t b = x[7] * (uint32_t)-4176 + x[5] * (uint32_t)-4926 + x[3] * 7373u + x[1] * 20995u;
  const uint32_t half = 1u << (n - 1);
  x[0] = sar(t10 + b + half, n);
  x[1] = sar(t12 + a + half, n);
  x[2] = sar(t12 - a + half, n);
  x[3] = sar(t10 - b + half, n);
}

// jidctred.c jpeg_idct_2x2, one pass: x[0], x[1], x[3], x[5], x[7] in, x[0 .. 1] out; descale by n (13, then 20)
__device__ __forceinline__ void idct2_1d(uint32_t x[8], int n) {
  const uint32_t t10 = x[0] << 15;
  const uint32_t t0 = x[7] * (uint32_t)-5906 + x[5] * 6967u + x[3] * (uint32_t)-10426 + x[1] * 29692u;
  const uint32_t half = 1u << (n - 1);
  x[0] = sar(t10 + t0 + half, n);
  x[1] = sar(t10 - t0 + half, n);
}

__device__ __forceinline__ uint32_t sample(uint32_t v) { return (uint32_t)min(max((int32_t)v + 128, 0), 255); }

__global__ __launch_bounds__(IDCT_THREADS) void k_jpeg_idct_scaled(const int16_t* __restrict__ coef,
                                                                   const edet_jpeg_image_t* __restrict__ images,
                                                                   const uint16_t* __restrict__ qtables, int64_t cap_blocks,
                                                                   uint8_t* __restrict__ planes) {
  __shared__ uint32_t tile[IDCT_BLOCKS][8][9];
  const int img = blockIdx.y;
  const edet_jpeg_image_t d = images[img];
  const int slot = threadIdx.x >> 3, r = threadIdx.x & 7;
  const int64_t g = (int64_t)blockIdx.x * IDCT_BLOCKS + slot;      // the block within the image
  const bool live = scaled_ok(d, cap_blocks) && g < d.total_blocks;      // (scaled_ok is the same in every lane)
  int c = 0, local = 0, s = 8;
  if (live) {
    local = (int)g;
    while (c + 1 < d.components && local >= d.blocks_w[c] * d.blocks_h[c]) {
      local -= d.blocks_w[c] * d.blocks_h[c];
      ++c;
    }
    s = sample_size(d, scaled_m(d), c);
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
  const uint32_t dc = x[0];      // lane 0: coefficient 0 times its table entry
#pragma unroll
  for (int e = 0; e < 8; ++e) tile[slot][r][e] = x[e];
  __syncthreads();
  // the column pass: lane r has column r, top to bottom, and returns it to the cells it alone read
  if (s == 8) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = tile[slot][e][r];
    idct_1d(x, 11);
#pragma unroll
    for (int e = 0; e < 8; ++e) tile[slot][e][r] = x[e];
  } else if (s == 4) {
    if (r != 4) {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = tile[slot][e][r];
      idct4_1d(x, 12);
#pragma unroll
      for (int e = 0; e < 4; ++e) tile[slot][e][r] = x[e];
    }
  } else if (s == 2) {
    if (r < 2 || (r & 1)) {      // columns 0, 1, 3, 5, 7
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = tile[slot][e][r];
      idct2_1d(x, 13);
      tile[slot][0][r] = x[0];
      tile[slot][1][r] = x[1];
    }
  }
  __syncthreads();
  if (!live || r >= s) return;      // (no barrier follows)
  const int bw = d.blocks_w[c], by = local / bw, bx = local - by * bw;
  // < 64 first_block[c] + s s (blocks of c) <= 64 cap_blocks
  uint8_t* to = planes + (size_t)d.first_block[c] * 64 + ((size_t)by * s + r) * ((size_t)bw * s) + (size_t)bx * s;
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = tile[slot][r][e];      // row r of the workspace
  if (s == 8) {
    idct_1d(x, 18);
    uint2 o;
    o.x = sample(x[0]) | (sample(x[1]) << 8) | (sample(x[2]) << 16) | (sample(x[3]) << 24);
    o.y = sample(x[4]) | (sample(x[5]) << 8) | (sample(x[6]) << 16) | (sample(x[7]) << 24);
    *reinterpret_cast<uint2*>(to) = o;
  } else if (s == 4) {
    idct4_1d(x, 19);
    *reinterpret_cast<uint32_t*>(to) = sample(x[0]) | (sample(x[1]) << 8) | (sample(x[2]) << 16) | (sample(x[3]) << 24);
  } else if (s == 2) {
    idct2_1d(x, 20);
    *reinterpret_cast<uint16_t*>(to) = (uint16_t)(sample(x[0]) | (sample(x[1]) << 8));
  } else {
    *to = (uint8_t)sample(sar(dc + 4u, 3));
  }
}

// four samples x0 .. x0 + 3 of a plane row (stride pw) whose first `width` samples are real: one word where the row stride
// keeps it aligned (64 first_block + y pw + x0, x0 a multiple of 4 below pw), else the bytes inside the image, 0 beyond
__device__ __forceinline__ void load4(const uint8_t* __restrict__ row, int pw, int x0, int width, int out[4]) {
  if ((pw & 3) == 0) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(row + x0);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = (int)((w >> (8 * j)) & 0xFF);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = x0 + j < width ? (int)row[x0 + j] : 0;
  }
}

template <bool VEC>
__global__ __launch_bounds__(COLOR_THREADS) void k_jpeg_color_scaled(const uint8_t* __restrict__ planes,
                                                                    const edet_jpeg_image_t* __restrict__ images,
                                                                    int canvas_h, int canvas_w, int64_t cap_blocks,
                                                                    uint8_t* __restrict__ raw) {
  const int img = blockIdx.y;
  const int groups = (canvas_w + 3) >> 2;
  const int64_t idx = (int64_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
  if (idx >= (int64_t)groups * canvas_h) return;
  const int y = (int)(idx / groups), x0 = (int)(idx - (int64_t)y * groups) * 4;
  const edet_jpeg_image_t d = images[img];
  uint32_t rgb[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j) rgb[j][0] = rgb[j][1] = rgb[j][2] = 0;
  if (scaled_ok(d, cap_blocks) && y < d.height && x0 < d.width) {
    const int m = scaled_m(d), s0 = sample_size(d, m, 0);
    const int pw0 = d.blocks_w[0] * s0;
    int yy[4], cb[4], cr[4];
    load4(planes + (size_t)d.first_block[0] * 64 + (size_t)y * pw0, pw0, x0, d.width, yy);
    if (d.components == 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) cb[j] = cr[j] = 128;
    } else {
      const int s1 = sample_size(d, m, 1);
      const int pw = d.blocks_w[1] * s1;
      const int fh = d.h_max * s0 / s1, fv = d.v_max * s0 / s1;      // (1, 1), (2, 1) or (2, 2)
      const uint8_t* pb = planes + (size_t)d.first_block[1] * 64;
      const uint8_t* pr = planes + (size_t)d.first_block[2] * 64;
      if (fh == 1) {
        load4(pb + (size_t)y * pw, pw, x0, d.width, cb);
        load4(pr + (size_t)y * pw, pw, x0, d.width, cr);
      } else {
        const int n = (d.width + 1) >> 1, rows = (d.height + fv - 1) / fv;      // the component's real samples
        if (m > 1 && n > 2) {      // jdsample.c: fancy upsampling only above 1/8 and for more than two columns
          chroma4(pb, pw, n, rows, fv == 2, y, x0, cb);
          chroma4(pr, pw, n, rows, fv == 2, y, x0, cr);
        } else {
          const size_t at = (size_t)(fv == 2 ? y >> 1 : y) * pw;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int i = min((x0 + j) >> 1, n - 1);
            cb[j] = pb[at + i];
            cr[j] = pr[at + i];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (x0 + j < d.width) {
        const int b = cb[j] - 128, r = cr[j] - 128;
        rgb[j][0] = (uint32_t)clamp255(yy[j] + ((91881 * r + 32768) >> 16));
        rgb[j][1] = (uint32_t)clamp255(yy[j] + ((-22554 * b - 46802 * r + 32768) >> 16));
        rgb[j][2] = (uint32_t)clamp255(yy[j] + ((116130 * b + 32768) >> 16));
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

extern "C" int edet_jpeg_idct_scaled(const int16_t* coef, const edet_jpeg_image_t* images_dev, const uint16_t* qtables_dev,
                                     int batch, int max_blocks, uint8_t* planes, size_t plane_capacity, void* stream) {
  EDET_CHECK(coef && images_dev && qtables_dev && planes, "edet_jpeg_idct_scaled: null pointer");
  EDET_CHECK(batch >= 1 && batch <= 65535 && max_blocks >= 0, "edet_jpeg_idct_scaled: batch %d (1..65535), max_blocks %d",
             batch, max_blocks);
  EDET_CHECK(((uintptr_t)coef & 15) == 0 && ((uintptr_t)qtables_dev & 15) == 0 && ((uintptr_t)planes & 7) == 0,
             "edet_jpeg_idct_scaled: coef and qtables must be 16-byte aligned, planes 8-byte aligned");
  if (max_blocks == 0) return 0;
  edet_launch(k_jpeg_idct_scaled, dim3((unsigned)cdiv(max_blocks, IDCT_BLOCKS), (unsigned)batch), dim3(IDCT_THREADS), 0,
              to_stream(stream), coef, images_dev, qtables_dev, (int64_t)(plane_capacity / 64), planes);
  EDET_LAUNCH_CHECK("edet_jpeg_idct_scaled");
  return 0;
}

extern "C" int edet_jpeg_color_scaled(const uint8_t* planes, const edet_jpeg_image_t* images_dev, int batch, int canvas_h,
                                      int canvas_w, size_t plane_capacity, uint8_t* raw, void* stream) {
  EDET_CHECK(planes && images_dev && raw, "edet_jpeg_color_scaled: null pointer");
  EDET_CHECK(batch >= 1 && batch <= 65535 && canvas_h >= 1 && canvas_w >= 1 &&
                 (int64_t)canvas_h * canvas_w * 3 < ((int64_t)1 << 31),
             "edet_jpeg_color_scaled: batch %d (1..65535), canvas %d x %d", batch, canvas_h, canvas_w);
  EDET_CHECK(((uintptr_t)planes & 7) == 0, "edet_jpeg_color_scaled: planes must be 8-byte aligned");
  const int64_t work = (int64_t)((canvas_w + 3) / 4) * canvas_h;
  const dim3 grid((unsigned)cdiv(work, COLOR_THREADS), (unsigned)batch);
  const int64_t cap = (int64_t)(plane_capacity / 64);
  if (canvas_w % 4 == 0 && ((uintptr_t)raw & 3) == 0)
    edet_launch(k_jpeg_color_scaled<true>, grid, dim3(COLOR_THREADS), 0, to_stream(stream), planes, images_dev, canvas_h,
                canvas_w, cap, raw);
  else
    edet_launch(k_jpeg_color_scaled<false>, grid, dim3(COLOR_THREADS), 0, to_stream(stream), planes, images_dev, canvas_h,
                canvas_w, cap, raw);
  EDET_LAUNCH_CHECK("edet_jpeg_color_scaled");
  return 0;
}
