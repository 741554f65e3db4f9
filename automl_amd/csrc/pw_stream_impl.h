// Streaming pointwise (1x1) convolution kernels for the bf16 path on gfx950 (wave64, MFMA 32x32x16): what the four
// kernel families share.  One family per source: pw_stream_fwd.hip (k_pw_fwd), pw_stream_dgrad.hip (k_pw_dgrad),
// pw_stream_wgrad.hip (k_pw_wgrad), pw_stream_fused.hip (k_pw_bwd_fused, k_noy_apply).
//
// The pointwise convolutions of EfficientDet are tall-skinny GEMMs (M = N*H*W rows up to 13.1 M,
// K, N <= a few hundred channels): 25-100 FLOP/B, i.e. HBM-bound on MI355X.  The structure below is
// therefore built around the memory stream, not around the matrix cores:
//
//   * one wave owns a CONTIGUOUS range of 32-row tiles and never synchronises with the other waves of
//     its workgroup inside the main loop (no __syncthreads between loads and MFMAs): 16 waves per CU
//     with independent load -> transform -> MFMA -> store chains hide HBM latency by themselves;
//   * the big operand is read once, in whole rows, 16 bytes per lane ("fixed-column" mapping: lane ->
//     (row r0 + lane / chunks_per_row, channel chunk lane % chunks_per_row), so the per-channel
//     BatchNorm / swish coefficients of the producing layer live in registers), transformed to the
//     activated bf16 value and staged in a wave-private LDS tile; the MFMA B' fragments (8 consecutive
//     k of one row) are ds_read_b128 from there;
//   * the small operand (weights, <= ~100 KB) sits in workgroup-shared LDS for the whole kernel;
//   * the product is computed transposed, D'[out channel][row], so that after the accumulator ->
//     LDS round trip every lane stores 16 contiguous bytes of one row (fully coalesced writes);
//   * BatchNorm statistic partials (sum, sum of squares) are taken from the ROUNDED values that were
//     stored, column-wise from the LDS tile, one partial row per workgroup.
//
// Reference call sites replaced: tf.keras.layers.Conv2D 1x1 in efficientdet/backbone/efficientnet_model.py
// :304-312 (expand), :345-353 (project); efficientdet/tf2/efficientdet_keras.py:286-290 (resample 1x1)
// and the pointwise half of SeparableConv2D (:195-207, :459-464, :546-556).
#pragma once
#include <stdlib.h>

#include "pw_impl.h"

namespace pws {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int THREADS = 256;
constexpr int WAVES = 4;
constexpr int TR = 32;        // rows per wave tile
constexpr int ECC = 64;       // epilogue chunk of the gradient kernels: channels per C tile

// Fixed-column mapping of a [32 rows][nvec 16-byte chunks] tile onto the 64 lanes of a wave.
struct ColMap {
  int nvec;   // chunks per row
  int rp;     // rows per pass = 64 / nvec   (nvec <= 64)
  int npass;  // ceil(32 / rp)
};

inline ColMap make_colmap(int channels) {
  ColMap m;
  m.nvec = (channels + 7) / 8;
  m.rp = 64 / m.nvec;
  m.npass = (TR + m.rp - 1) / m.rp;
  return m;
}

// LDS row stride (bytes) of a bf16 tile whose rows are read as MFMA fragments (lane = row, 16 B per lane):
// a multiple of 16 B with an ODD number of 16-B slots, so that the 16 rows one ds_read_b128 lane group
// touches fall on 16 different slots of the 64-bank row (a dense 128-B stride is 8-way conflicted:
// SQ_LDS_BANK_CONFLICT was 2x the useful LDS cycles of the 64-channel BiFPN / head layers).
// `need_zero_tail` reserves 16 zero bytes after the row for the k-step that overhangs K (K % 16 == 8).
inline int frag_stride(int cols, bool need_zero_tail) {
  int b = (cols * 2 + 15) / 16 * 16;
  if (need_zero_tail) b += 16;
  if ((b / 16) % 2 == 0) b += 16;
  return b;
}

// `n` units of work (super-tiles, steps) in contiguous ranges over the waves of about `grid` workgroups: the units
// per wave, and (returned) the workgroups that this many per wave leaves with work
inline int spread_over_waves(int n, int grid, int* per_wave) {
  *per_wave = (n + grid * WAVES - 1) / (grid * WAVES);
  return (n + *per_wave * WAVES - 1) / (*per_wave * WAVES);
}

// D'[out channel][row] for one 32-row tile and one 32-channel slice: A' = weight rows (LDS), B' = staged rows (LDS)
__device__ __forceinline__ f32x16 mma_tile(const unsigned char* wrow, const unsigned char* arow, int ksteps) {
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int ks = 0; ks < ksteps; ++ks) {
    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wrow + ks * 32);
    const bf16x8 bf = *reinterpret_cast<const bf16x8*>(arow + ks * 32);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, bf, acc, 0, 0, 0);
  }
  return acc;
}

// the same, continuing an accumulator (a second operand pair contracted into the same D' tile)
__device__ __forceinline__ f32x16 mma_tile_more(const unsigned char* wrow, const unsigned char* arow, int ksteps,
                                                f32x16 acc) {
  for (int ks = 0; ks < ksteps; ++ks) {
    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wrow + ks * 32);
    const bf16x8 bf = *reinterpret_cast<const bf16x8*>(arow + ks * 32);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, bf, acc, 0, 0, 0);
  }
  return acc;
}

// MFMA fragment "8 consecutive rows (row0 ...) of one column" of a [32][stride] bf16 tile through the gfx950 transpose
// read (ds_read_b64_tr_b16): within a 16-lane group lane i supplies the address of 4 consecutive channels (8 bytes) of
// row row0 + i / 4 -- together a [4 rows][16 channels] block starting at channel col0 -- and receives the 4 rows of
// channel col0 + i.  Two reads (rows +0..3, +4..7) replace the eight 2-byte reads and the packing of column_frag
// (pw_stream_wgrad.hip).  Addresses are 8-byte aligned: 16-byte row strides, col0 % 16 == 0.
typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 bf16x4v_t;
__device__ __forceinline__ bf16x8 column_frag_tr(const unsigned char* tile, int stride, int row0, int col0, int fi) {
  const unsigned char* p = tile + (size_t)(row0 + (fi >> 2)) * stride + (col0 + (fi & 3) * 4) * 2;
  typedef __attribute__((address_space(3))) bf16x4v_t* lds_ptr_t;
  const bf16x4v_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr_t)(p));
  const bf16x4v_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr_t)(p + 4 * stride));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

}  // namespace pws
