// Streaming pointwise convolution, data gradient: k_pw_dgrad and its host routine (design: pw_stream_impl.h).
#include "pw_stream_impl.h"

namespace pws {

// ------------------------------------------------------------------------------ data gradient
// d(in)[m][k] = sum_n dy[m][n] * W[k][n], chained through the input view's activation in the epilogue.
// Same skeleton as the forward kernel with dy as the streamed operand (BatchNorm backward applied on load:
// dy = a*dz + b*y + c, two tensors per row) and an fp32 C tile; the epilogue works on 64-channel chunks with
// a fixed 8-channel column per lane (col = lane & 7, 8 rows per pass), reads the saved conv input x, applies
// act'(z), optionally accumulates into the existing gradient, stores 16 B per lane and keeps the BatchNorm
// backward sums (sum g, sum g*xhat) in registers across the sub-tiles.  With epi.dgate != NULL the gradient of the gated
// value is stored as it is; the SE gate-gradient sums belong to the dispatch (k_gate_sums, pw_gemm.hip).
struct BwdArgs {
  edet_gview_t gv;    // dy (contraction length R = gv.c)
  edet_tview_t tv;    // conv input view: raw x, scale, shift, gate, act; KO = tv.c output columns
  const bf16_t* W;    // [KO][ldw], n contiguous
  int ldw;
  edet_bwd_epi_t epi;
  int M, R, KO, hw;
  ColMap cr;
  int G, pst;
  int SA, SC, SW;     // SC: fp32 C tile stride in bytes
  int KOpad;          // KO rounded up to 32
  int spw, ksteps;
  int nvec_out;       // ceil(KO / 8)
};

template <int NS, bool GBN, bool OACT>
__global__ __launch_bounds__(THREADS, 2) void k_pw_dgrad(const BwdArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31, h = lane >> 5;
  unsigned char* Wl = smem;                                             // [KOpad][SW]
  float* red = reinterpret_cast<float*>(Wl + (size_t)a.KOpad * a.SW);   // [2][KOpad] stats
  const int a_rows = TR * a.G;
  const int a_alloc = a.pst * a.cr.rp;
  const size_t wave_bytes = (size_t)a_alloc * a.SA + (size_t)TR * a.SC + (size_t)3 * a.KOpad * 4;
  unsigned char* wbase = reinterpret_cast<unsigned char*>(red + 2 * a.KOpad) + (size_t)wave * wave_bytes;
  unsigned char* At = wbase;                                            // [a_alloc][SA] bf16 dy
  unsigned char* Ct = wbase + (size_t)a_alloc * a.SA;                   // [32][SC] fp32
  float* wst = reinterpret_cast<float*>(Ct + TR * a.SC);                // [2][KOpad] stat sums of this wave
  // (a third [KOpad] row per wave follows wst: reserved by the host's LDS formula, unused)
  const bool want_stats = a.epi.stat_partials != nullptr;
  const bool want_gate = a.epi.dgate != nullptr;      // SE-gated input: the gradient of the gated value is stored as it is
  const bool swish = !OACT && a.tv.act == EDET_ACT_SWISH, affine = a.tv.scale != nullptr;
  constexpr bool other = OACT;

  for (int i = tid; i < 2 * a.KOpad; i += THREADS) red[i] = 0.f;
  for (int i = lane; i < 2 * a.KOpad; i += 64) wst[i] = 0.f;
  for (int i = lane; i < a_alloc * a.SA / 16; i += 64) reinterpret_cast<uint4*>(At)[i] = make_uint4(0, 0, 0, 0);
  {  // weights -> LDS (zero-filled beyond KO and beyond R)
    const int slots = a.SW / 16;
    for (int q = tid; q < a.KOpad * slots; q += THREADS) {
      const int r = q / slots, sl = q - r * slots;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (r < a.KO && sl * 8 < a.R) v = *reinterpret_cast<const uint4*>(a.W + (size_t)r * a.ldw + sl * 8);
      *reinterpret_cast<uint4*>(Wl + (size_t)r * a.SW + sl * 16) = v;
    }
  }
  __syncthreads();

  // dy-side mapping
  const int lane_k = lane % (a.cr.nvec * a.cr.rp);
  const int colR = lane_k % a.cr.nvec, rsub = lane_k / a.cr.nvec;
  const int kvalid = min(8, a.R - colR * 8);                           // elements of this chunk inside R
  const bf16_t* DZ = reinterpret_cast<const bf16_t*>(a.gv.dz);
  const bf16_t* Y = reinterpret_cast<const bf16_t*>(a.gv.y);
  const bf16_t* X = reinterpret_cast<const bf16_t*>(a.tv.data);
  bf16_t* GO = reinterpret_cast<bf16_t*>(a.epi.gout);
  const uint32_t lane_off = (uint32_t)(rsub * a.gv.ld + colR * 8) * 2u;
  const size_t pass_bytes = (size_t)a.cr.rp * a.gv.ld * 2;

  const int nst = (a.M + a_rows - 1) / a_rows;
  const int gw = blockIdx.x * WAVES + wave;
  const int st0 = min(nst, gw * a.spw), st1 = min(nst, st0 + a.spw);

  uint4 rz[NS], ry[GBN ? NS : 1];
  auto issue = [&](int st) {
    const int row0 = st * a_rows;
    const bool full = row0 + a_alloc <= a.M;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      if (i < a.pst) {
        size_t off;
        if (full) off = (size_t)row0 * a.gv.ld * 2 + (size_t)i * pass_bytes + lane_off;
        else off = ((size_t)min(row0 + i * a.cr.rp + rsub, a.M - 1) * a.gv.ld + colR * 8) * 2;
        rz[i] = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(DZ) + off);
        if (GBN) ry[i] = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(Y) + off);
      }
    }
  };

  // epilogue mapping: 64-channel chunk, 8 lanes per row
  const int ecol = lane & 7, erow = lane >> 3;
  if (st0 < st1) issue(st0);
  for (int st = st0; st < st1; ++st) {
    const int row0 = st * a_rows;
    const int rows_in_st = min(a_rows, a.M - row0);
    {  // dy = a*dz + b*y + c, masked to the R valid columns, as bf16 into the A super-tile
      float ga[8], gb[8], gc[8];
      if (GBN) {
        loadf8(a.gv.a + colR * 8, ga); loadf8(a.gv.b + colR * 8, gb); loadf8(a.gv.cc + colR * 8, gc);
      }
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        if (i < a.pst) {
          float x[8];
          unpack8(rz[i], x);
          if (GBN) {
            float y[8];
            unpack8(ry[i], y);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = fmaf(ga[e], x[e], fmaf(gb[e], y[e], gc[e]));
          }
          if (kvalid < 8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) if (e >= kvalid) x[e] = 0.f;
          }
          *reinterpret_cast<uint4*>(At + (i * a.cr.rp + rsub) * a.SA + colR * 16) = pack8(x);
        }
      }
    }
    if (st + 1 < st1) issue(st + 1);
    __builtin_amdgcn_wave_barrier();

    for (int c0 = 0; c0 < a.KOpad; c0 += ECC) {
      const int ccols = min(ECC, a.KOpad - c0);                // 32 or 64
      const int ch0 = c0 + ecol * 8;                           // this lane's 8 output channels
      const bool col_ok = ch0 < a.KO && ecol * 8 < ccols;
      // s1: sum g; s2: sum g*x, turned into sum g*xhat when it is flushed
      float sc[8], sh[8], s1[8], s2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { sc[e] = 1.f; sh[e] = 0.f; s1[e] = s2[e] = 0.f; }
      if (col_ok && affine) { loadf8(a.tv.scale + ch0, sc); loadf8(a.tv.shift + ch0, sh); }
      const bool need_x = want_stats || (!want_gate && (swish || other));
      for (int sub = 0; sub * TR < rows_in_st; ++sub) {
        const int trow0 = row0 + sub * TR;
        const int rows_valid = min(TR, rows_in_st - sub * TR);
        // saved conv input for this (sub-tile, chunk): 4 passes of 8 rows, in flight during the MFMAs
        uint4 xr[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          xr[p] = make_uint4(0, 0, 0, 0);
          const int r = p * 8 + erow;
          if (need_x && col_ok && r < rows_valid)
            xr[p] = *reinterpret_cast<const uint4*>(X + (size_t)(trow0 + r) * a.tv.ld + ch0);
        }
        const unsigned char* arow = At + (size_t)(sub * TR + j) * a.SA + h * 16;
        for (int nt = 0; nt < ccols / 32; ++nt) {
          const f32x16 acc = mma_tile(Wl + (size_t)(c0 + nt * 32 + j) * a.SW + h * 16, arow, a.ksteps);
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(Ct + j * a.SC + (nt * 32 + 8 * g + 4 * h) * 4) =
                make_float4(acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int r = p * 8 + erow;
          if (col_ok && r < rows_valid) {
            const float4 d0 = *reinterpret_cast<const float4*>(Ct + r * a.SC + ecol * 32);
            const float4 d1 = *reinterpret_cast<const float4*>(Ct + r * a.SC + ecol * 32 + 16);
            float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
            float x[8], g[8];
            unpack8(xr[p], x);
            const size_t off = (size_t)(trow0 + r) * a.tv.ld + ch0;
            if (want_gate) {
#pragma unroll
              for (int e = 0; e < 8; ++e) g[e] = d[e];
            } else if (swish) {
#pragma unroll
              for (int e = 0; e < 8; ++e) g[e] = d[e] * swish_gradf_(fmaf(x[e], sc[e], sh[e]));
            } else if (other) {
#pragma unroll
              for (int e = 0; e < 8; ++e) g[e] = d[e] * act_other_grad_(a.tv.act, fmaf(x[e], sc[e], sh[e]));
            } else {
#pragma unroll
              for (int e = 0; e < 8; ++e) g[e] = d[e];
            }
            if (a.epi.beta) {
              float old[8];
              unpack8(*reinterpret_cast<const uint4*>(GO + off), old);
#pragma unroll
              for (int e = 0; e < 8; ++e) g[e] += old[e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) if (ch0 + e >= a.KO) g[e] = 0.f;
            *reinterpret_cast<uint4*>(GO + off) = pack8(g);
            if (want_stats) {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                s1[e] += g[e];
                s2[e] = fmaf(g[e], x[e], s2[e]);
              }
            }
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
      // chunk sums -> wave LDS accumulators (8 lanes share a column: LDS atomics)
      if (col_ok && want_stats) {
        float mu[8], rs[8];
        loadf8(a.epi.mean + ch0, mu);
        loadf8(a.epi.rstd + ch0, rs);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (ch0 + e < a.KO) {
            atomicAdd(&wst[ch0 + e], s1[e]);
            atomicAdd(&wst[a.KOpad + ch0 + e], rs[e] * (s2[e] - mu[e] * s1[e]));   // sum g*(x-mean)*rstd
          }
        }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (want_stats) {
    for (int c = lane; c < a.KO; c += 64) {
      atomicAdd(&red[c], wst[c]);
      atomicAdd(&red[a.KOpad + c], wst[a.KOpad + c]);
    }
    __syncthreads();
    float* dst = a.epi.stat_partials + (size_t)blockIdx.x * 2 * a.KO;
    for (int i = tid; i < 2 * a.KO; i += THREADS) {
      const int which = i / a.KO, col = i - which * a.KO;
      dst[i] = red[which * a.KOpad + col];
    }
  }
}

}  // namespace pws

int pws_try_dgrad(const edet_gview_t* dy, const void* w, int ldw, const edet_tview_t* in,
                  const edet_bwd_epi_t* epi, int* nparts_out, hipStream_t st) {
  using namespace pws;
  const int R = dy->c, KO = in->c;
  if (R > 128 || KO > 512 || KO % 8 != 0 || dy->ld % 8 != 0) return 0;
  BwdArgs a;
  memset(&a, 0, sizeof(a));
  a.gv = *dy; a.tv = *in; a.W = reinterpret_cast<const bf16_t*>(w); a.ldw = ldw; a.epi = *epi;
  a.M = in->n * in->h * in->w; a.R = R; a.KO = KO; a.hw = in->h * in->w;
  a.cr = make_colmap(R);
  const bool gbn = dy->a != nullptr;
  constexpr int NS = 8;                // load passes of the instantiations
  a.ksteps = (R + 15) / 16;
  a.SA = frag_stride((R + 7) / 8 * 8, ((R + 7) / 8 * 8) % 16 != 0);
  a.SW = a.SA;
  a.KOpad = (KO + 31) / 32 * 32;
  a.SC = ECC * 4 + 16;
  a.nvec_out = KO / 8;
  size_t lds = 0;
  int g0 = NS * a.cr.rp / TR;
  if (gbn) g0 /= 2;                    // two tensors per row: half the rows for the same bytes in flight
  if (g0 > 4) g0 = 4;
  for (a.G = g0;; --a.G) {
    if (a.G < 1) a.G = 1;
    a.pst = (TR * a.G + a.cr.rp - 1) / a.cr.rp;
    if (a.pst > NS) return 0;
    lds = (size_t)a.KOpad * a.SW + (size_t)2 * a.KOpad * 4 +
          (size_t)WAVES * ((size_t)a.pst * a.cr.rp * a.SA + (size_t)TR * a.SC + (size_t)3 * a.KOpad * 4);
    if (lds <= 53 * 1024 || a.G == 1) break;
  }
  if (lds > 150 * 1024) return 0;
  const int nst = (a.M + TR * a.G - 1) / (TR * a.G);
  // >= 4 super-tiles per wave (r03d lab: 2 / 4 / 8 -> backward 16.62 / 16.49 / 16.45 ms over 24 shapes)
  int grid = (nst + WAVES * 4 - 1) / (WAVES * 4);
  if (grid > EDET_MAX_PARTS) grid = EDET_MAX_PARTS;
  if (grid < 1) grid = 1;
  grid = spread_over_waves(nst, grid, &a.spw);
  if (nparts_out) *nparts_out = grid;
  static void (*const kern[2][2])(const BwdArgs) = {      // [GBN][OACT]
      {k_pw_dgrad<NS, false, false>, k_pw_dgrad<NS, false, true>},
      {k_pw_dgrad<NS, true, false>, k_pw_dgrad<NS, true, true>}};
  void (*const k)(const BwdArgs) = kern[gbn][in->act > EDET_ACT_SWISH];
  if (!edet_lds_optin(k, lds)) return 0;
  edet_launch(k, dim3(grid), dim3(THREADS), lds, st, a);
  EDET_LAUNCH_CHECK("edet_pw_bwd_data(stream)");
  return 1;
}
