// What the two device stages of the JPEG decoder share (jpeg.hip: full size; jpeg_scaled.hip: libjpeg's reduced sizes): the
// descriptor check, jidctint.c's one-dimensional pass, jdsample.c's fancy upsampling and the small integer helpers; and what
// the reduced sizes share with the window decode (jpeg_window.hip): the denominator, the sample sizes and their check.
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

// 8 / denominator, or 0 for a descriptor whose `reserved` is none of 0, 1, 2, 4, 8
__device__ __forceinline__ int scaled_m(const edet_jpeg_image_t& d) {
  const int r = d.reserved;
  return (r == 0 || r == 1) ? 8 : r == 2 ? 4 : r == 4 ? 2 : r == 8 ? 1 : 0;
}

// The side of component c's blocks after the inverse transform (jdmaster.c): m, and 2 m for the chroma of a 4:2:0 file below
// full size, which then lies at the output's resolution.
__device__ __forceinline__ int sample_size(const edet_jpeg_image_t& d, int m, int c) {
  return (c > 0 && d.h_max == 2 && d.v_max == 2 && m < 8) ? 2 * m : m;
}

// image_ok, the denominator, and the real samples of every component inside its REDUCED plane: d.height x d.width is the
// output size, the chroma's real samples are half of it (rounded up) in each direction that is still subsampled.
__device__ __forceinline__ bool scaled_ok(const edet_jpeg_image_t& d, int64_t cap_blocks) {
  const int m = scaled_m(d);
  if (m == 0 || !image_ok(d, cap_blocks)) return false;
  const int s0 = sample_size(d, m, 0);
  for (int c = 0; c < d.components; ++c) {
    const int s = sample_size(d, m, c);
    const int fh = c == 0 ? 1 : d.h_max * s0 / s, fv = c == 0 ? 1 : d.v_max * s0 / s;
    if ((d.width + fh - 1) / fh > d.blocks_w[c] * s || (d.height + fv - 1) / fv > d.blocks_h[c] * s) return false;
  }
  return true;
}

// chroma4 for a thread whose four pixels x0 .. x0 + 3 start at ANY column of the image, read from the kept planes of a window
// decode (jpeg_window.hip): sample (row, column) of the component lies at (row - oy, column - ox) of plane p, whose rows hold
// pw samples.  n, rows, y and x0 are the IMAGE's, so the edge rules are those of the whole image.  A column that only a
// pixel outside the window would read is clamped into the plane's row; its result is not used.
template <int T>
__device__ __forceinline__ int fancy1(const int col[4], int i0, int n, bool v2) {
  constexpr int e = T >> 1;      // pixel x0 + j, T = j + (x0 & 1): chroma column i0 + e is col[1 + e]
  const int i = i0 + e, cur = col[1 + e];
  if (T & 1) {
    const int next = col[e < 2 ? 2 + e : 3];
    return v2 ? (i == n - 1 ? (4 * cur + 7) >> 4 : (3 * cur + next + 7) >> 4) : (i == n - 1 ? cur : (3 * cur + next + 2) >> 2);
  }
  const int prev = col[e];
  return v2 ? (i == 0 ? (4 * cur + 8) >> 4 : (3 * cur + prev + 8) >> 4) : (i == 0 ? cur : (3 * cur + prev + 1) >> 2);
}

__device__ __forceinline__ void chroma4_window(const uint8_t* __restrict__ p, int pw, int ox, int oy, int n, int rows, bool v2,
                                               int y, int x0, int out[4]) {
  const int i0 = x0 >> 1;
  int col[4];
  int near = y, far = y;
  if (v2) {
    near = y >> 1;
    far = (y & 1) ? near + 1 : near - 1;
    far = min(max(far, 0), rows - 1);
  }
  near -= oy;
  far -= oy;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = min(max(min(max(i0 - 1 + k, 0), n - 1) - ox, 0), pw - 1);
    const int a = p[(size_t)near * pw + i];
    col[k] = v2 ? 3 * a + (int)p[(size_t)far * pw + i] : a;
  }
  if (x0 & 1) {
    out[0] = fancy1<1>(col, i0, n, v2);
    out[1] = fancy1<2>(col, i0, n, v2);
    out[2] = fancy1<3>(col, i0, n, v2);
    out[3] = fancy1<4>(col, i0, n, v2);
  } else {
    out[0] = fancy1<0>(col, i0, n, v2);
    out[1] = fancy1<1>(col, i0, n, v2);
    out[2] = fancy1<2>(col, i0, n, v2);
    out[3] = fancy1<3>(col, i0, n, v2);
  }
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

}  // namespace jpeg_impl
