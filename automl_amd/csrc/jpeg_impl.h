// What the two device stages of the JPEG decoder share (jpeg.hip: full size; jpeg_scaled.hip: libjpeg's reduced sizes): the
// descriptor check, jidctint.c's one-dimensional pass, jdsample.c's fancy upsampling and the small integer helpers.
#pragma once
#include "common.h"

namespace jpeg_impl {

__device__ __forceinline__ uint32_t sar(uint32_t v, int s) { return (uint32_t)((int32_t)v >> s); }

// jidctint.c's one-dimensional pass, in place; descale by s (11 behind the columns, 18 behind the rows)
__device__ __forceinline__ void idct_1d(uint32_t x[8], int s) {
  uint32_t z2 = x[2], z3 = x[6];
  uint32_t z1 = (z2 + z3) * 4433u;
  uint32_t tmp2 = z1 + z3 * (uint32_t)-15137;
  uint32_t tmp3 = z1 + z2 * 6270u;
  uint32_t tmp0 = (x[0] + x[4]) << 13;
  uint32_t tmp1 = (x[0] - x[4]) << 13;
  const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3;
  const uint32_t tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  uint32_t z4 = tmp1 + tmp3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
  z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995; z3 *= (uint32_t)-16069; z4 *= (uint32_t)-3196;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  const uint32_t half = 1u << (s - 1);
  x[0] = sar(tmp10 + tmp3 + half, s); x[7] = sar(tmp10 - tmp3 + half, s);
  x[1] = sar(tmp11 + tmp2 + half, s); x[6] = sar(tmp11 - tmp2 + half, s);
  x[2] = sar(tmp12 + tmp1 + half, s); x[5] = sar(tmp12 - tmp1 + half, s);
  x[3] = sar(tmp13 + tmp0 + half, s); x[4] = sar(tmp13 - tmp0 + half, s);
}

// Is the descriptor one the host stage writes, and does it stay inside arenas of cap_blocks blocks?  The kernels index
// with its fields, so nothing is read or written for an image that fails this: its canvas comes out zero.
__device__ __forceinline__ bool image_ok(const edet_jpeg_image_t& d, int64_t cap_blocks) {
  if (d.status != 0 || (d.components != 1 && d.components != 3)) return false;
  if (d.h_max < 1 || d.h_max > 2 || d.v_max < 1 || d.v_max > d.h_max || d.height < 1 || d.width < 1) return false;
  if (d.components == 1 && d.h_max != 1) return false;      // (1, 1), (2, 1) or (2, 2); one component: (1, 1)
  int64_t total = 0;
  for (int c = 0; c < d.components; ++c) {
    const int bw = d.blocks_w[c], bh = d.blocks_h[c];
    if (bw < 1 || bw > 8192 || bh < 1 || bh > 8192 || d.quant_id[c] < 0 || d.quant_id[c] > 3) return false;
    const int64_t n = (int64_t)bw * bh;
    if (d.first_block[c] < 0 || (int64_t)d.first_block[c] + n > cap_blocks) return false;
    if (c > 0 && (int64_t)d.first_block[c] != (int64_t)d.first_block[c - 1] + (int64_t)d.blocks_w[c - 1] * d.blocks_h[c - 1])
      return false;
    // the real samples of the component lie inside its plane
    const int hs = c == 0 ? 1 : d.h_max, vs = c == 0 ? 1 : d.v_max;
    if ((d.width + hs - 1) / hs > bw * 8 || (d.height + vs - 1) / vs > bh * 8) return false;
    total += n;
  }
  return total == (int64_t)d.total_blocks;
}

// jdsample.c's fancy upsampling for the four pixels x0 .. x0 + 3 of output row y from chroma plane p (row stride pw):
// n real columns, rows real rows; v2: h2v2 (two rows, weights 3:1), else h2v1
__device__ __forceinline__ void chroma4(const uint8_t* __restrict__ p, int pw, int n, int rows, bool v2, int y, int x0,
                                        int out[4]) {
  const int i0 = x0 >> 1;
  int col[4];
  int near = y, far = y;
  if (v2) {
    near = y >> 1;
    far = (y & 1) ? near + 1 : near - 1;
    far = min(max(far, 0), rows - 1);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = min(max(i0 - 1 + k, 0), n - 1);
    const int a = p[(size_t)near * pw + i];
    col[k] = v2 ? 3 * a + (int)p[(size_t)far * pw + i] : a;
  }
  // col[1] is column i0, col[2] column i0 + 1
  if (v2) {
    out[0] = i0 == 0 ? (4 * col[1] + 8) >> 4 : (3 * col[1] + col[0] + 8) >> 4;
    out[1] = i0 == n - 1 ? (4 * col[1] + 7) >> 4 : (3 * col[1] + col[2] + 7) >> 4;
    out[2] = (3 * col[2] + col[1] + 8) >> 4;
    out[3] = i0 + 1 == n - 1 ? (4 * col[2] + 7) >> 4 : (3 * col[2] + col[3] + 7) >> 4;
  } else {
    out[0] = i0 == 0 ? col[1] : (3 * col[1] + col[0] + 1) >> 2;
    out[1] = i0 == n - 1 ? col[1] : (3 * col[1] + col[2] + 2) >> 2;
    out[2] = (3 * col[2] + col[1] + 1) >> 2;
    out[3] = i0 + 1 == n - 1 ? col[2] : (3 * col[2] + col[3] + 2) >> 2;
  }
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

}  // namespace jpeg_impl
