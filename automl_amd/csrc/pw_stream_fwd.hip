// Streaming pointwise convolution, forward: k_pw_fwd and its host routine (design: pw_stream_impl.h).
#include "pw_stream_impl.h"

namespace pws {

constexpr int NCC = 64;       // output channels per LDS C tile (2 MFMA tiles)

// stride of the C tile (written 8 B per lane by rows, read 16 B per lane): one 16-B slot of padding
inline int ctile_stride(int cols) { return cols * 2 + 16; }

struct FwdArgs {
  edet_tview_t tv;
  const bf16_t* Wt;   // [N][ldw], k contiguous
  int ldw;
  const float* bias;  // [N] or null
  bf16_t* out;
  int ldo;
  int M, K, N, hw;
  float* stat_partials;
  ColMap ck;
  int G;              // 32-row tiles per super-tile (one super-tile = the loads kept in flight per wave)
  int pst;            // load passes per super-tile (<= NS)
  int SA, SC, SW;     // LDS row strides in bytes
  int Npad;           // N rounded up to 32
  int NWC, nwc;       // weight chunk rows (multiple of 32), number of chunks
  int spw;            // super-tiles per wave (contiguous range)
  int ksteps;         // ceil(K / 16)
  int nvec_out;       // valid 16-byte chunks per output row = ceil(N / 8)
};

// activated value of 8 raw bf16 elements -> 8 bf16 packed
// OACT: the view's activation is relu / relu6 / hswish (utils.activation_fn, utils.py:36-53; `act` carries the code) --
// a template parameter of the kernels, so that the swish / linear instantiations keep their code and registers
template <bool OACT>
__device__ __forceinline__ uint4 transform8(const uint4 raw, const float sc[8], const float sh[8],
                                            const float gt[8], bool affine, bool swish, bool gate, int act) {
  float x[8];
  unpack8(raw, x);
  if (affine) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = fmaf(x[e], sc[e], sh[e]);
  }
  if (OACT) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = act_other_(act, x[e]);
  } else if (swish) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = swishf_(x[e]);
  }
  if (gate) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] *= gt[e];
  }
  return pack8(x);
}

// column sums of a [rows][.] bf16 LDS tile: lane = column `c`
__device__ __forceinline__ void column_stats(const unsigned char* Ct, int SC, int c, int rows_valid, float& s,
                                             float& s2) {
  const bf16_t* colp = reinterpret_cast<const bf16_t*>(Ct) + c;
  const int ld = SC / 2;
  float u0 = 0.f, u1 = 0.f, v0 = 0.f, v1 = 0.f;
  if (rows_valid == TR) {
#pragma unroll 4
    for (int r = 0; r < TR; r += 2) {
      const float x0 = bf2f(colp[r * ld]), x1 = bf2f(colp[(r + 1) * ld]);
      u0 += x0; u1 += x1;
      v0 = fmaf(x0, x0, v0); v1 = fmaf(x1, x1, v1);
    }
  } else {
    for (int r = 0; r < rows_valid; ++r) {
      const float x0 = bf2f(colp[r * ld]);
      u0 += x0;
      v0 = fmaf(x0, x0, v0);
    }
  }
  s = u0 + u1;
  s2 = v0 + v1;
}

// ------------------------------------------------------------------------------------ forward
// EXACT: every one of the NS load passes is issued and staged unconditionally (a.pst == NS).  A load under a run-time
// guard makes every wait on the prefetched registers a wait for ALL outstanding loads and stores (r03j, the one-pass
// backward: 30 %); the guarded form remains for the relu / relu6 / hswish instantiations.
// (OACT stays the last template argument: tests/test_gpu_kernels.py reads it off the kernel symbol)
template <int NS, bool EXACT, bool OACT>
__global__ __launch_bounds__(THREADS, NS <= 8 ? 3 : 2) void k_pw_fwd(const FwdArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31, h = lane >> 5;
  // LDS carve-up
  unsigned char* Wl = smem;                                        // [NWC][SW]
  float* biasL = reinterpret_cast<float*>(Wl + (size_t)a.NWC * a.SW);   // [Npad]
  float* red = biasL + a.Npad;                                     // [WAVES][2][Npad]: one set of column sums per wave
  const int a_rows = TR * a.G;                                     // rows per super-tile
  const int a_alloc = a.pst * a.ck.rp;                             // >= a_rows: every load pass lands in-bounds
  const size_t wave_bytes = (size_t)a_alloc * a.SA + (size_t)TR * a.SC + (size_t)2 * a.NWC * 4;
  unsigned char* wbase = reinterpret_cast<unsigned char*>(red + 2 * WAVES * a.Npad) + (size_t)wave * wave_bytes;
  unsigned char* At = wbase;                                       // [32*G][SA]
  unsigned char* Ct = wbase + (size_t)a_alloc * a.SA;              // [32][SC]
  float* wst = reinterpret_cast<float*>(Ct + TR * a.SC);           // [2][NWC] this wave's column sums
  const bool want_stats = a.stat_partials != nullptr;

  for (int i = tid; i < a.Npad; i += THREADS) biasL[i] = (a.bias && i < a.N) ? a.bias[i] : 0.f;
  for (int i = tid; i < 2 * WAVES * a.Npad; i += THREADS) red[i] = 0.f;
  // zero this wave's A buffer once: the bytes after column K stay zero (k-step overhang)
  for (int i = lane; i < a_alloc * a.SA / 16; i += 64) reinterpret_cast<uint4*>(At)[i] = make_uint4(0, 0, 0, 0);

  // K-side mapping and coefficients
  // lanes beyond nvec*rp duplicate the work of lane % (nvec*rp): no divergence, no extra traffic
  const int lane_k = lane % (a.ck.nvec * a.ck.rp);
  const int colK = lane_k % a.ck.nvec, rsub = lane_k / a.ck.nvec;
  const bool activeK = true;
  const bool affine = a.tv.scale != nullptr, swish = a.tv.act == EDET_ACT_SWISH, gated = a.tv.gate != nullptr;
  float sc[8], sh[8], gt[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sc[e] = 1.f; sh[e] = 0.f; gt[e] = 1.f; }
  if (affine && activeK) { loadf8(a.tv.scale + colK * 8, sc); loadf8(a.tv.shift + colK * 8, sh); }
  const bf16_t* A = reinterpret_cast<const bf16_t*>(a.tv.data);

  const int nst = (a.M + a_rows - 1) / a_rows;                     // super-tiles
  const int gw = blockIdx.x * WAVES + wave;
  const int st0 = min(nst, gw * a.spw), st1 = min(nst, st0 + a.spw);

  uint4 raw[NS];
  // address = (uniform 64-bit base of the pass) + (32-bit lane offset): one VGPR of addressing for all passes
  const uint32_t lane_off = (uint32_t)(rsub * a.tv.ld + colK * 8) * 2u;
  const size_t pass_bytes = (size_t)a.ck.rp * a.tv.ld * 2;
  auto issue = [&](int st) {
    const int row0 = st * a_rows;
    const unsigned char* base = reinterpret_cast<const unsigned char*>(A) + (size_t)row0 * a.tv.ld * 2;
    const bool full = row0 + a_alloc <= a.M;
    if (EXACT) {
      if (full) {
#pragma unroll
        for (int i = 0; i < NS; ++i) raw[i] = *reinterpret_cast<const uint4*>(base + (size_t)i * pass_bytes + lane_off);
      } else {  // tail: rows past M re-read row M-1 (finite values, never stored)
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const int r = min(row0 + i * a.ck.rp + rsub, a.M - 1);
          raw[i] = *reinterpret_cast<const uint4*>(A + (size_t)r * a.tv.ld + colK * 8);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        if (i < a.pst) {
          if (full) {
            raw[i] = *reinterpret_cast<const uint4*>(base + (size_t)i * pass_bytes + lane_off);
          } else {
            const int r = min(row0 + i * a.ck.rp + rsub, a.M - 1);
            raw[i] = *reinterpret_cast<const uint4*>(A + (size_t)r * a.tv.ld + colK * 8);
          }
        }
      }
    }
  };

  for (int wc = 0; wc < a.nwc; ++wc) {
    const int n0 = wc * a.NWC;                       // first output channel of this weight chunk
    const int nrows = min(a.NWC, a.Npad - n0);       // multiple of 32
    __syncthreads();
    {  // weight chunk -> LDS (zero-filled beyond N and beyond K)
      const int slots = a.SW / 16;
      for (int q = tid; q < nrows * slots; q += THREADS) {
        const int r = q / slots, s = q - r * slots;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (n0 + r < a.N && s * 8 < a.K) v = *reinterpret_cast<const uint4*>(a.Wt + (size_t)(n0 + r) * a.ldw + s * 8);
        *reinterpret_cast<uint4*>(Wl + (size_t)r * a.SW + s * 16) = v;
      }
    }
    __syncthreads();
    for (int i = lane; i < 2 * a.NWC; i += 64) wst[i] = 0.f;

    int gate_img = -1;
    if (st0 < st1) issue(st0);
    for (int st = st0; st < st1; ++st) {
      const int row0 = st * a_rows;
      const int rows_in_st = min(a_rows, a.M - row0);
      // ---- transform the loaded rows into the activated A super-tile
      bool per_row_gate = false;
      if (gated) {
        const int img0 = row0 / a.hw, img1 = (row0 + rows_in_st - 1) / a.hw;
        per_row_gate = img0 != img1;
        if (!per_row_gate && img0 != gate_img && activeK) {
          loadf8(a.tv.gate + (size_t)img0 * a.K + colK * 8, gt);
          gate_img = img0;
        }
        if (per_row_gate) gate_img = -1;
      }
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        if (EXACT || i < a.pst) {
          const int r = i * a.ck.rp + rsub;
          if (per_row_gate) {
            const uint32_t rr = (uint32_t)min(row0 + r, a.M - 1);
            loadf8(a.tv.gate + (size_t)(rr / (uint32_t)a.hw) * a.K + colK * 8, gt);
          }
          *reinterpret_cast<uint4*>(At + r * a.SA + colK * 16) = transform8<OACT>(raw[i], sc, sh, gt, affine, swish, gated, a.tv.act);
        }
      }
      if (st + 1 < st1) issue(st + 1);               // next super-tile's loads fly during the MFMA phase
      __builtin_amdgcn_wave_barrier();

      for (int sub = 0; sub * TR < rows_in_st; ++sub) {
        const int trow0 = row0 + sub * TR;
        const int rows_valid = min(TR, rows_in_st - sub * TR);
        const unsigned char* arow = At + (size_t)(sub * TR + j) * a.SA + h * 16;
        // ---- MFMA over the output channels of this weight chunk, one C sub-tile (<= 128 channels) at a time
        for (int c0 = 0; c0 < nrows; c0 += NCC) {
          const int ccols = min(NCC, nrows - c0);    // multiple of 32
          for (int nt = 0; nt < ccols / 32; ++nt) {
            const f32x16 acc = mma_tile(Wl + (size_t)(c0 + nt * 32 + j) * a.SW + h * 16, arow, a.ksteps);
            // lane (row j, half h) holds channels nt*32 + (e&3) + 8*(e>>2) + 4*h
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int ch = c0 + nt * 32 + 8 * g + 4 * h;
              const float4 b4 = *reinterpret_cast<const float4*>(biasL + n0 + ch);
              uint2 pk;
              pk.x = pack2bf(acc[4 * g + 0] + b4.x, acc[4 * g + 1] + b4.y);
              pk.y = pack2bf(acc[4 * g + 2] + b4.z, acc[4 * g + 3] + b4.w);
              *reinterpret_cast<uint2*>(Ct + j * a.SC + (nt * 32 + 8 * g + 4 * h) * 2) = pk;
            }
          }
          __builtin_amdgcn_wave_barrier();
          // ---- C sub-tile -> global, 16 bytes per lane in row-major order
          {
            const int nvc_tile = ccols / 8;                                  // chunks per LDS row
            const int nvc = min(nvc_tile, a.nvec_out - (n0 + c0) / 8);       // valid chunks per row
            const int total = rows_valid * nvc;
            int row = lane / nvc, col = lane - row * nvc;
            const int drow = 64 / nvc, dcol = 64 - drow * nvc;
            bf16_t* obase = a.out + (size_t)trow0 * a.ldo + n0 + c0;
#pragma unroll 2
            for (int q = lane; q < total; q += 64) {
              const uint4 v = *reinterpret_cast<const uint4*>(Ct + row * a.SC + col * 16);
              *reinterpret_cast<uint4*>(obase + (size_t)row * a.ldo + col * 8) = v;
              row += drow; col += dcol;
              if (col >= nvc) { col -= nvc; ++row; }
            }
          }
          // ---- statistics of the stored values: lane = column
          if (want_stats) {
            if (lane < ccols) {
              float s, s2;
              column_stats(Ct, a.SC, lane, rows_valid, s, s2);
              wst[c0 + lane] += s;                 // wave-private LDS accumulators
              wst[a.NWC + c0 + lane] += s2;
            }
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
    if (want_stats) {
      __builtin_amdgcn_wave_barrier();
      // into this wave's own set (r04: no LDS atomics; the four sets are added in wave order at the end, so the
      // statistics are the same on every run)
      float* redw = red + (size_t)wave * 2 * a.Npad;
      for (int c = lane; c < nrows; c += 64) {
        if (n0 + c < a.N) {
          redw[n0 + c] += wst[c];
          redw[a.Npad + n0 + c] += wst[a.NWC + c];
        }
      }
    }
  }
  if (want_stats) {
    __syncthreads();
    float* dst = a.stat_partials + (size_t)blockIdx.x * 2 * a.N;
    for (int i = tid; i < 2 * a.N; i += THREADS) {
      const int which = i / a.N, col = i - which * a.N;
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) t += red[(size_t)w * 2 * a.Npad + which * a.Npad + col];
      dst[i] = t;
    }
  }
}

// Chooses the weight chunking so that the workgroup's LDS stays under `cap` bytes; returns total bytes
// or 0 when even one 32-row chunk does not fit.
inline size_t plan_lds(int Npad, int a_rows, int SA, int SW, size_t cap, int* NWC_out, int* SC_out) {
  for (int nwcr = Npad; nwcr >= 32; nwcr -= 32) {
    const int ccols = nwcr < NCC ? nwcr : NCC;
    const int SC = ctile_stride(ccols);
    const size_t total = (size_t)nwcr * SW + (size_t)(1 + 2 * WAVES) * Npad * 4 +
                         (size_t)WAVES * ((size_t)a_rows * SA + (size_t)TR * SC + (size_t)2 * nwcr * 4);
    if (total <= cap) {
      *NWC_out = nwcr;
      *SC_out = SC;
      return total;
    }
  }
  return 0;
}

// The instantiations, keyed by what the host decides: load passes, EXACT, OACT.  The EXACT rows stand in ascending order of
// their passes: pws_try_fwd takes the first one that covers the super-tile.
struct FwdVariant {
  int ns;
  bool exact, oact;
  void (*kern)(const FwdArgs);
};
template <int NS, bool EXACT, bool OACT>
constexpr FwdVariant fwd_variant() { return {NS, EXACT, OACT, k_pw_fwd<NS, EXACT, OACT>}; }
static const FwdVariant fwd_variants[] = {
    fwd_variant<4, true, false>(),  fwd_variant<6, true, false>(),  fwd_variant<7, true, false>(),
    fwd_variant<8, true, false>(),  fwd_variant<11, true, false>(), fwd_variant<16, true, false>(),
    fwd_variant<8, false, false>(), fwd_variant<8, false, true>(),  fwd_variant<16, false, false>(),
    fwd_variant<16, false, true>()};

inline const FwdVariant* find_fwd_variant(int ns, bool exact, bool oact) {
  for (const FwdVariant& v : fwd_variants)
    if (v.ns == ns && v.exact == exact && v.oact == oact) return &v;
  return nullptr;
}

}  // namespace pws

int pws_try_fwd(const edet_tview_t* in, const void* wt, int ldw, const float* bias, void* out, int cout,
                int ldo, float* stat_partials, int* nparts_out, hipStream_t st) {
  using namespace pws;
  const int K = in->c, N = cout;
  if (K > 256 || K % 8 != 0) return 0;
  FwdArgs a;
  memset(&a, 0, sizeof(a));
  a.tv = *in;
  a.Wt = reinterpret_cast<const bf16_t*>(wt); a.ldw = ldw; a.bias = bias;
  a.out = reinterpret_cast<bf16_t*>(out); a.ldo = ldo;
  a.M = in->n * in->h * in->w; a.K = K; a.N = N; a.hw = in->h * in->w;
  a.stat_partials = stat_partials;
  a.ck = make_colmap(K);
  const bool oact = in->act > EDET_ACT_SWISH;
  int NS = K > 128 ? 16 : 8;
  bool exact = false;
  a.ksteps = (K + 15) / 16;
  a.SA = frag_stride(K, K % 16 != 0);
  a.SW = a.SA;
  a.Npad = (N + 31) / 32 * 32;
  a.nvec_out = (N + 7) / 8;
  if (ldo < a.nvec_out * 8) return 0;
  // rows kept in flight per wave: as many 32-row tiles as NS load passes cover, shrunk until three
  // workgroups fit in a CU's LDS (53 KB each); the weight chunk may take it to one workgroup per CU
  size_t lds = 0;
  for (a.G = NS * a.ck.rp / TR > 4 ? 4 : NS * a.ck.rp / TR; ; --a.G) {
    if (a.G < 1) a.G = 1;
    a.pst = (TR * a.G + a.ck.rp - 1) / a.ck.rp;
    if (a.pst > NS) return 0;
    lds = plan_lds(a.Npad, a.pst * a.ck.rp, a.SA, a.SW, 53 * 1024, &a.NWC, &a.SC);
    if ((lds != 0 && a.NWC == a.Npad) || a.G == 1) break;
  }
  if (lds == 0 || a.NWC != a.Npad) {
    lds = plan_lds(a.Npad, a.pst * a.ck.rp, a.SA, a.SW, 80 * 1024, &a.NWC, &a.SC);
    if (lds == 0 || a.NWC != a.Npad) lds = plan_lds(a.Npad, a.pst * a.ck.rp, a.SA, a.SW, 150 * 1024, &a.NWC, &a.SC);
    if (lds == 0) return 0;
  }
  if (!oact) {
    // the EXACT instantiation with the fewest passes that covers the super-tile (the table lists them in ascending
    // order); its passes are all issued (rows beyond the super-tile are the wave's next rows) and staged, so the LDS
    // tile holds NS * rp rows
    int pick = 0;
    for (const FwdVariant& v : fwd_variants)
      if (v.exact && v.ns >= a.pst) { pick = v.ns; break; }
    if (pick > 0) {
      int nwc2 = 0, sc2 = 0;
      const size_t cap = lds <= 53 * 1024 ? 53 * 1024 : (lds <= 80 * 1024 ? 80 * 1024 : 150 * 1024);
      const size_t l2 = plan_lds(a.Npad, pick * a.ck.rp, a.SA, a.SW, cap, &nwc2, &sc2);
      if (l2 != 0 && nwc2 == a.NWC) { exact = true; NS = pick; a.pst = pick; lds = l2; a.SC = sc2; }
    }
  }
  a.nwc = (a.Npad + a.NWC - 1) / a.NWC;
  if (a.nwc > 2) return 0;   // the big operand would be re-read too often: leave it to the tiled kernel
  const int nst = (a.M + TR * a.G - 1) / (TR * a.G);
  // >= 4 super-tiles per wave (r03d lab, 24 pointwise layer shapes: 2 / 4 / 8 / 16 -> forward 4.85 / 4.79 / 4.82 / 4.87 ms)
  int grid = (nst + WAVES * 4 - 1) / (WAVES * 4);
  // One round: at most as many workgroups as the chip holds at once (3 per compute unit for the 8-pass kernel, 2 for the
  // 16-pass one).  r03h lab, caps of 1024 (the partial-row limit, round 2) / 768 / 512: 320x320x16->96 0.92 / 0.81 / 0.83
  // ms, 160x160x24->144 0.39 / 0.33 / 0.36, 320x320x32->16 0.46 / 0.40 / 0.48, 80x80x64->64 62 / 55 / 60 us; the
  // 144-channel inputs (2 per CU) 0.36 / 0.38 / 0.36: with 1024 workgroups on 768 slots the second round runs a third full.
  const FwdVariant* v = find_fwd_variant(NS, exact, oact);
  if (!v) return 0;
  const int slots_fwd = edet_resident_wgs(reinterpret_cast<const void*>(v->kern), THREADS, lds);
  if (slots_fwd > 0 && grid > slots_fwd) grid = slots_fwd;
  if (grid > EDET_MAX_PARTS) grid = EDET_MAX_PARTS;
  if (grid < 1) grid = 1;
  grid = spread_over_waves(nst, grid, &a.spw);
  if (nparts_out) *nparts_out = grid;
  if (!edet_lds_optin(v->kern, lds)) return 0;
  edet_launch(v->kern, dim3(grid), dim3(THREADS), lds, st, a);
  EDET_LAUNCH_CHECK("edet_pw_fwd(stream)");
  return 1;
}
