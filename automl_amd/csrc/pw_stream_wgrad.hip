// Streaming pointwise convolution, weight gradient: k_pw_wgrad and its host routine (design: pw_stream_impl.h).
#include "pw_stream_impl.h"

namespace pws {

// ---------------------------------------------------------------------------- weight gradient
// dW[k][n] = sum_m view(in)[m][k] * dy[m][n]: the contraction runs over the rows, so both operands are
// needed "transposed" (8 consecutive rows of one channel per lane).  Each wave owns a 64 x CV block of dW
// (U = the operand with more channels, sliced 64 wide; V = the other one, CV <= 64) over a contiguous row
// range: per 32-row step it loads its U slice and V in whole 16-byte chunks (fixed column per lane, so the
// BatchNorm / swish / BatchNorm-backward coefficients stay in registers), stages the transformed bf16 rows in
// wave-private LDS and gathers the MFMA fragments column-wise with ds_read_u16 (64 B/clk/CU, six times the
// HBM feed rate).  Partial blocks go to a workspace [split][K][N] that a second kernel sums into dW:
// deterministic, no atomics.
struct WgArgs {
  edet_tview_t tv;    // conv input view, K = tv.c
  edet_gview_t gv;    // dy, N = gv.c
  float* ws;          // [S][K][N]
  int M, K, N, hw;
  int CU, CV;         // channels of U and V
  int nus;            // 64-wide slices of U
  int S;              // row splits
  int rows_per_split; // multiple of 32
  int cpwV;           // V-side lanes per row (power of two >= CV/8, <= 8)
};

template <bool IS_G, bool GBN>
struct OperandRegs {
  uint4 r[4];
  uint4 y[(IS_G && GBN) ? 4 : 1];
};

// loads pass p (rows rbase + p*rpp + rowl) of one operand
template <bool IS_G, bool GBN>
__device__ __forceinline__ void wg_issue(const WgArgs& a, OperandRegs<IS_G, GBN>& o, int npass, int rpp, int rowl,
                                         int ch, bool col_ok, int m0, int m_end) {
  const bf16_t* P = reinterpret_cast<const bf16_t*>(IS_G ? a.gv.dz : a.tv.data);
  const bf16_t* Y = reinterpret_cast<const bf16_t*>(a.gv.y);
  const int ld = IS_G ? a.gv.ld : a.tv.ld;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (p < npass) {
      const int m = m0 + p * rpp + rowl;
      o.r[p] = make_uint4(0, 0, 0, 0);
      if (IS_G && GBN) o.y[p] = make_uint4(0, 0, 0, 0);
      if (col_ok && m < m_end) {
        o.r[p] = *reinterpret_cast<const uint4*>(P + (size_t)m * ld + ch);
        if (IS_G && GBN) o.y[p] = *reinterpret_cast<const uint4*>(Y + (size_t)m * ld + ch);
      }
    }
  }
}

// transforms the loaded passes and writes them (bf16) into the operand's LDS tile [32][stride]
template <bool IS_G, bool GBN, bool OACT>
__device__ __forceinline__ void wg_stage(const WgArgs& a, const OperandRegs<IS_G, GBN>& o, int npass, int rpp,
                                         int rowl, int coll, int ch, int cmax, bool col_ok, int m0, int m_end,
                                         unsigned char* tile, int stride) {
  if (!col_ok) return;
  float c0[8], c1[8], c2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { c0[e] = 1.f; c1[e] = 0.f; c2[e] = 0.f; }
  if (IS_G) {
    if (GBN) { loadf8(a.gv.a + ch, c0); loadf8(a.gv.b + ch, c1); loadf8(a.gv.cc + ch, c2); }
  } else if (a.tv.scale) {
    loadf8(a.tv.scale + ch, c0);
    loadf8(a.tv.shift + ch, c1);
  }
  const int valid = min(8, cmax - ch);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (p < npass) {
      const int r = p * rpp + rowl;
      const int m = m0 + r;
      float x[8];
      unpack8(o.r[p], x);
      if (m < m_end) {
        if (IS_G) {
          if (GBN) {
            float y[8];
            unpack8(o.y[p], y);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = fmaf(c0[e], x[e], fmaf(c1[e], y[e], c2[e]));
          }
        } else {
          if (a.tv.scale) {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = fmaf(x[e], c0[e], c1[e]);
          }
          if (OACT) {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = act_other_(a.tv.act, x[e]);
          } else if (a.tv.act == EDET_ACT_SWISH) {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = swishf_(x[e]);
          }
          if (a.tv.gate) {
            float gt[8];
            loadf8(a.tv.gate + (size_t)(m / a.hw) * a.K + ch, gt);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] *= gt[e];
          }
        }
        if (valid < 8) {
#pragma unroll
          for (int e = 0; e < 8; ++e) if (e >= valid) x[e] = 0.f;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.f;
      }
      if (r < TR) *reinterpret_cast<uint4*>(tile + r * stride + coll * 16) = pack8(x);
    }
  }
}

// 8 consecutive rows (8*h + 16*ks ...) of column `col` of a [32][stride] bf16 tile
__device__ __forceinline__ bf16x8 column_frag(const unsigned char* tile, int stride, int row0, int col) {
  const bf16_t* p = reinterpret_cast<const bf16_t*>(tile + row0 * stride) + col;
  const int ld = stride / 2;
  s16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (short)p[e * ld];
  return __builtin_bit_cast(bf16x8, v);
}

constexpr int WG_SU = 64 * 2 + 16;   // U tile stride (64 channels)
constexpr int WG_SV = 64 * 2 + 16;   // V tile stride (up to 64 channels)

template <bool UG, bool GBN, bool OACT>   // UG: U is the gradient operand (N >= K)
__global__ __launch_bounds__(THREADS, 2) void k_pw_wgrad(const WgArgs a) {
  __shared__ __align__(16) unsigned char smem[WAVES * TR * (WG_SU + WG_SV)];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  unsigned char* Ut = smem + wave * TR * (WG_SU + WG_SV);
  unsigned char* Vt = Ut + TR * WG_SU;
  // wave -> (U slice, row split)
  int us, rs;
  if (a.nus >= 3) {
    const int nus4 = (a.nus + 3) / 4;
    us = (blockIdx.x % nus4) * 4 + wave;
    rs = blockIdx.x / nus4;
  } else {
    us = wave % a.nus;
    rs = blockIdx.x * (WAVES / a.nus) + wave / a.nus;
  }
  if (us >= a.nus || rs >= a.S) return;
  const int m_begin = rs * a.rows_per_split;
  const int m_end = min(a.M, m_begin + a.rows_per_split);

  // U side: 8 chunks per row, 8 rows per pass, 4 passes; V side: cpwV chunks per row
  const int ucol = lane & 7, urow = lane >> 3;
  const int uch = us * 64 + ucol * 8;
  const bool u_ok = uch < a.CU;
  const int vcol = lane & (a.cpwV - 1), vrow = lane / a.cpwV;
  const int rppV = 64 / a.cpwV;
  const int npassV = rppV >= TR ? 1 : TR / rppV;
  const int vch = vcol * 8;
  const bool v_ok = vch < a.CV && vrow < TR;
  const int nvt = (a.CV + 31) / 32;                 // 1 or 2 V tiles

  // zero both tiles once (columns never written stay zero)
  for (int i = lane; i < TR * (WG_SU + WG_SV) / 16; i += 64) reinterpret_cast<uint4*>(Ut)[i] = make_uint4(0, 0, 0, 0);

  f32x16 acc[2][2];
#pragma unroll
  for (int ut = 0; ut < 2; ++ut)
#pragma unroll
    for (int vt = 0; vt < 2; ++vt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[ut][vt][e] = 0.f;

  OperandRegs<UG, GBN> ou;
  OperandRegs<!UG, GBN> ov;
  if (m_begin < m_end) {
    wg_issue<UG, GBN>(a, ou, 4, 8, urow, uch, u_ok, m_begin, m_end);
    wg_issue<!UG, GBN>(a, ov, npassV, rppV, vrow, vch, v_ok, m_begin, m_end);
  }
  const int j = lane & 31, h = lane >> 5;
  for (int m0 = m_begin; m0 < m_end; m0 += TR) {
    wg_stage<UG, GBN, OACT>(a, ou, 4, 8, urow, ucol, uch, a.CU, u_ok, m0, m_end, Ut, WG_SU);
    wg_stage<!UG, GBN, OACT>(a, ov, npassV, rppV, vrow, vcol, vch, a.CV, v_ok, m0, m_end, Vt, WG_SV);
    if (m0 + TR < m_end) {
      wg_issue<UG, GBN>(a, ou, 4, 8, urow, uch, u_ok, m0 + TR, m_end);
      wg_issue<!UG, GBN>(a, ov, npassV, rppV, vrow, vch, v_ok, m0 + TR, m_end);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int r0 = ks * 16 + h * 8;
      const bf16x8 u0 = column_frag(Ut, WG_SU, r0, j);
      const bf16x8 u1 = column_frag(Ut, WG_SU, r0, 32 + j);
      const bf16x8 v0 = column_frag(Vt, WG_SV, r0, j);
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u0, v0, acc[0][0], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u1, v0, acc[1][0], 0, 0, 0);
      if (nvt > 1) {
        const bf16x8 v1 = column_frag(Vt, WG_SV, r0, 32 + j);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u0, v1, acc[0][1], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u1, v1, acc[1][1], 0, 0, 0);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  // D[i = U channel][j = V channel]: lane holds V channel j (+32*vt), U channels (e&3)+8*(e>>2)+4*h (+32*ut)
  float* dst = a.ws + (size_t)rs * a.K * a.N;
#pragma unroll
  for (int ut = 0; ut < 2; ++ut)
#pragma unroll
    for (int vt = 0; vt < 2; ++vt) {
      if (vt < nvt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int iu = us * 64 + ut * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
          const int jv = vt * 32 + j;
          if (iu < a.CU && jv < a.CV) {
            const int k = UG ? jv : iu, n = UG ? iu : jv;
            dst[(size_t)k * a.N + n] = acc[ut][vt][e];
          }
        }
      }
    }
}

}  // namespace pws

int pws_try_wgrad(const edet_tview_t* in, const edet_gview_t* dy, float* dweight, void* workspace,
                  size_t workspace_bytes, hipStream_t st) {
  using namespace pws;
  const int K = in->c, N = dy->c;
  if (!workspace || K % 8 != 0 || dy->ld % 8 != 0 || in->ld % 8 != 0) return 0;
  const bool ug = N >= K;
  WgArgs a;
  memset(&a, 0, sizeof(a));
  a.tv = *in; a.gv = *dy; a.ws = reinterpret_cast<float*>(workspace);
  a.M = in->n * in->h * in->w; a.K = K; a.N = N; a.hw = in->h * in->w;
  a.CU = ug ? N : K; a.CV = ug ? K : N;
  if (a.CV > 64) return 0;
  const bool gbn = dy->a != nullptr;
  if (gbn && N % 8 != 0) return 0;
  a.nus = (a.CU + 63) / 64;
  const int nvecV = (a.CV + 7) / 8;
  a.cpwV = 1;
  while (a.cpwV < nvecV) a.cpwV <<= 1;
  // row splits: ~2048 waves in total, at least 8 steps of 32 rows each, bounded by the workspace
  const int64_t kn = (int64_t)K * N;
  int S = 2048 / a.nus;
  const int max_by_rows = (a.M + 8 * TR - 1) / (8 * TR);
  if (S > max_by_rows) S = max_by_rows;
  const int64_t max_by_ws = (int64_t)(workspace_bytes / sizeof(float)) / kn;
  if (S > max_by_ws) S = (int)max_by_ws;
  if (S < 1) return 0;
  a.rows_per_split = ((a.M + S - 1) / S + TR - 1) / TR * TR;
  a.S = (a.M + a.rows_per_split - 1) / a.rows_per_split;
  int grid;
  if (a.nus >= 3) grid = ((a.nus + 3) / 4) * a.S;
  else grid = (a.S + WAVES / a.nus - 1) / (WAVES / a.nus);
  static void (*const kern[2][2][2])(const WgArgs) = {      // [UG][GBN][OACT]
      {{k_pw_wgrad<false, false, false>, k_pw_wgrad<false, false, true>},
       {k_pw_wgrad<false, true, false>, k_pw_wgrad<false, true, true>}},
      {{k_pw_wgrad<true, false, false>, k_pw_wgrad<true, false, true>},
       {k_pw_wgrad<true, true, false>, k_pw_wgrad<true, true, true>}}};
  edet_launch(kern[ug][gbn][in->act > EDET_ACT_SWISH], dim3(grid), dim3(THREADS), 0, st, a);
  EDET_LAUNCH_CHECK("edet_pw_bwd_weight(stream)");
  if (edet_reduce_partials(a.ws, a.S, kn, dweight, st) != 0) return -2;
  return 1;
}
