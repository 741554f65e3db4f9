// Streaming pointwise convolution, one-pass backward: k_pw_bwd_fused, its finisher k_noy_apply and their host routine
// (design: pw_stream_impl.h).
#include "pw_stream_impl.h"

namespace pws {

// ------------------------------------------------------------------ fused data + weight gradient
// Both gradients of a pointwise convolution in ONE pass over (dz, y, x): the data-gradient kernel (pw_stream_dgrad.hip)
// and the weight-gradient kernel (pw_stream_wgrad.hip) each stream the gradient pair (2 N channels per row) and the saved input (K channels),
// i.e. 7 tensor streams where one pass needs 4 (r01h PMC: 329 + 363 MB per launch pair against 194 MB
// algorithmic each).  Here a wave owns a contiguous range of 32-row tiles; per tile
//   * dz, y AND x are prefetched one tile ahead in whole 16-byte chunks (fixed column per lane: the BatchNorm
//     backward coefficients stay in registers), dy = a*dz + b*y + c goes to the LDS tile Dt as bf16, x is parked raw
//     in the LDS tile Xt;
//   * D'[k][row] = W[k][:] . dy[row][:] on 32x32x16 MFMAs, through the fp32 C tile into the 8-channel-per-lane
//     epilogue of k_pw_dgrad (act'(z), accumulate, BatchNorm-backward sums), which takes x from Xt
//     and leaves the ACTIVATED operand act(bn(x)) * gate there as bf16;
//   * dW[k][n] += sum_rows xa[row][k] * dy[row][n] on 16x16x32 MFMAs whose contraction runs over the tile's 32
//     rows: fragments are gathered column-wise (8 consecutive rows of one channel per lane) from Xt and Dt; the dW
//     block (<= 4 x 9 tiles of 16 x 16) stays in registers for the whole kernel.
// One wave per SIMD (the accumulators and a whole tile of loads in flight take ~400 registers): latency is hidden
// by the 14-21 KB every wave keeps in flight, not by occupancy.  At the end the four waves of a workgroup add their
// dW blocks in LDS (fixed order) and write one partial per workgroup; edet_reduce_partials sums them.
//
// NOY (r03): the BatchNorm backward WITHOUT the saved convolution output.  dy = a*dz + b*y + c and y = x~ W (x~ the
// operand the forward fed the matrix cores), so
//     dx~ = dy W^T   = dz (W diag(a))^T + x~ (W diag(b) W^T) + c W^T          = dz Wa^T + x~ G + v
//     dW  = x~^T dy  = (x~^T dz) diag(a) + (x~^T x~) W diag(b) + (sum_p x~) c^T = P diag(a) + S W diag(b) + s c^T
// with G = W diag(b) W^T a KO x KO matrix and S = x~^T x~ the Gram matrix of the input (KO <= 32 here): the 6x wider
// y is never read (the kernel's traffic drops from 2N + 2K to N + 2K channels per row: -43 % for 16 -> 96), dz goes
// from HBM to the LDS operand tile without being unpacked, and the only extra matrix work is one k-step against G
// and one or four 16 x 16 tiles of S.  Wa, G and v are made in the prologue from the weights already in LDS; the
// partial written per workgroup is [P | S | s] and k_noy_apply finishes dW.  Used when the convolution input is a
// plain stored tensor (every MBConv expansion reads a block output), so x~ = x and there is no chain epilogue work.
struct FusedArgs {
  edet_gview_t gv;    // dy: R = gv.c channels (the convolution's output channels)
  edet_tview_t tv;    // conv input view: raw x, scale, shift, gate, act; KO = tv.c channels
  const bf16_t* W;    // [KO][ldw], n contiguous (compute copy of the kernel)
  int ldw;
  edet_bwd_epi_t epi;
  float* ws;          // [grid][KO][R] fp32 partial weight gradients
  int M, R, KO, hw;
  ColMap cr, cx;      // load mappings of dy and of x
  int SA, SX, SC, SW; // LDS row strides in bytes: Dt, Xt, C tile, weights
  int KOpad;          // KO rounded up to 32
  int TK, TN;         // 16-wide tiles of dW along k and n
  int tpw, ksteps;    // steps per wave; ceil(R / 16)
  int SG, kxsteps;    // NOY: LDS row stride of G in bytes, ceil(KOpad / 16)
  int G;              // 32-row tiles per step: the loads of a whole step (32 G rows of dz, y, x) are in flight at once
};

// FT_S x FT_L = 16 x 16 tiles of dW kept per wave (min(TK, TN) <= FT_S, max(TK, TN) <= FT_L): 2 x 9 covers the expand
// layers (16..32 input channels, up to 144 output channels), 3 x 9 the project layers (up to 144 -> 48), 4 x 4 the
// 64 -> 64 layers of the BiFPN and the heads.
// NSR / NSX: load passes per step of dy / x, all issued unconditionally (r03j: run-time guards around the loads cost
// 30 % -- the waits degrade to vmcnt(0)); the host picks the instantiation that fits the step with the fewest rows
// to spare.  The round-2 kernel had two pairs, (8, 1) and (12, 2): 8 passes of 32 rows each for a 16-channel gradient
// whose 32-row tile needs one -- the reason the project layers measured slower in it.
// NCH: 64-channel epilogue chunks (KOpad <= 64 NCH); the per-channel sums of the BatchNorm backward are carried in
// registers across all tiles of the wave and reach LDS once per kernel.
// BETA: the instantiation can accumulate into gout (epi.beta; the old gradient rides along with x)
// STRADDLE: a 32-row tile may lie in two images (hw % 32 != 0) while an SE gate is involved
template <int NSR, int NSX, bool GBN, int FT_S, int FT_L, bool NOY = false, int NCH = 1, bool BETA = true, bool STRADDLE = true>
__global__ __launch_bounds__(THREADS, 1) void k_pw_bwd_fused(const FusedArgs a) {
  static_assert(!NOY || GBN, "NOY is a form of the BatchNorm backward on load");
  static_assert(!NOY || NCH == 1, "NOY: at most 32 input channels");
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31, h = lane >> 5;
  const bool has_beta = BETA && a.epi.beta != 0;
  const int srows = TR * a.G;                                           // rows per step
  unsigned char* Wl = smem;                                             // [KOpad][SW]
  float* red = reinterpret_cast<float*>(Wl + (size_t)a.KOpad * a.SW);   // [2][KOpad] stats
  float* coefS = red + 2 * a.KOpad;                                     // [KOpad] scale, [KOpad] shift of the view
  float* coefH = coefS + a.KOpad;
  const size_t wave_bytes = (size_t)srows * a.SA + (size_t)(has_beta ? 2 : 1) * srows * a.SX +
                            (size_t)TR * a.SC + (size_t)4 * a.KOpad * 4;
  float* vL = coefH + a.KOpad;                                          // NOY: [KOpad] v = c W^T
  unsigned char* Gl = reinterpret_cast<unsigned char*>(vL + (NOY ? a.KOpad : 0));      // NOY: [KOpad][SG] bf16 G
  unsigned char* wbase = Gl + (NOY ? (size_t)a.KOpad * a.SG : 0) + (size_t)wave * wave_bytes;
  unsigned char* Dt = wbase;                                            // [srows][SA] bf16 dy
  unsigned char* Xt = Dt + (size_t)srows * a.SA;                        // [srows][SX] bf16 x, then act(x)
  unsigned char* Ot = Xt + (size_t)srows * a.SX;                        // [srows][SX] bf16 old gout (beta only)
  unsigned char* Ct = Ot + (has_beta ? (size_t)srows * a.SX : 0);       // [32][SC] fp32
  float* wst = reinterpret_cast<float*>(Ct + TR * a.SC);                // [2][KOpad] sums (g, g*x) of this wave
  float* gateL = wst + 3 * a.KOpad;                                     // [KOpad] SE gate of the current image (the row before it: reserved, unused)
  // NOY: the host guarantees a plain input view and no sums (compile-time false: the code is not generated)
  const bool want_stats = !NOY && a.epi.stat_partials != nullptr;
  const bool swish = !NOY && a.tv.act == EDET_ACT_SWISH, affine = !NOY && a.tv.scale != nullptr;
  const bool gated = !NOY && a.tv.gate != nullptr;

  // Nothing inside the tile loop may wait on a global load other than the prefetched step (vmcnt is in order: a
  // wait for a later small load would drain the whole prefetch): per-channel vectors live in LDS.
  for (int i = tid; i < 2 * a.KOpad; i += THREADS) red[i] = 0.f;
  for (int i = tid; i < a.KOpad; i += THREADS) {
    coefS[i] = (affine && i < a.KO) ? a.tv.scale[i] : 1.f;
    coefH[i] = (affine && i < a.KO) ? a.tv.shift[i] : 0.f;
  }
  for (int i = lane; i < 2 * a.KOpad; i += 64) wst[i] = 0.f;
  for (int i = lane; i < a.KOpad; i += 64) gateL[i] = 1.f;
  for (int i = lane; i < (int)(((size_t)srows * a.SA + (size_t)srows * a.SX) / 16); i += 64)
    reinterpret_cast<uint4*>(Dt)[i] = make_uint4(0, 0, 0, 0);
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
  if (NOY) {
    // G[k][k'] = sum_n W[k][n] b[n] W[k'][n] (bf16 MFMA operand, zero beyond KO), v[k] = sum_n c[n] W[k][n] -- from the
    // bf16 weights the forward used; then the LDS weights become Wa[k][n] = a[n] W[k][n]
    for (int q = tid; q < a.KOpad * a.KOpad; q += THREADS) {
      const int k = q / a.KOpad, k2 = q - k * a.KOpad;
      float g = 0.f;
      if (k < a.KO && k2 < a.KO) {
        const bf16_t* w1 = reinterpret_cast<const bf16_t*>(Wl + (size_t)k * a.SW);
        const bf16_t* w2 = reinterpret_cast<const bf16_t*>(Wl + (size_t)k2 * a.SW);
        for (int n = 0; n < a.R; ++n) g = fmaf(bf2f(w1[n]) * a.gv.b[n], bf2f(w2[n]), g);
      }
      reinterpret_cast<bf16_t*>(Gl + (size_t)k * a.SG)[k2] = f2bf(g);
    }
    for (int q = tid; q < a.KOpad * (a.SG / 2 - a.KOpad); q += THREADS) {      // zero tail of every G row
      const int k = q / (a.SG / 2 - a.KOpad), t = q - k * (a.SG / 2 - a.KOpad);
      reinterpret_cast<bf16_t*>(Gl + (size_t)k * a.SG)[a.KOpad + t] = 0;
    }
    for (int k = tid; k < a.KOpad; k += THREADS) {
      float t = 0.f;
      if (k < a.KO) {
        const bf16_t* w1 = reinterpret_cast<const bf16_t*>(Wl + (size_t)k * a.SW);
        for (int n = 0; n < a.R; ++n) t = fmaf(a.gv.cc[n], bf2f(w1[n]), t);
      }
      vL[k] = t;
    }
    __syncthreads();
    for (int q = tid; q < a.KO * a.R; q += THREADS) {
      const int k = q / a.R, n = q - k * a.R;
      bf16_t* wp = reinterpret_cast<bf16_t*>(Wl + (size_t)k * a.SW) + n;
      *wp = f2bf(bf2f(*wp) * a.gv.a[n]);
    }
    __syncthreads();
  }

  // load mappings (lanes beyond nvec*rp duplicate the work of lane % (nvec*rp): no divergence)
  const int lane_r = lane % (a.cr.nvec * a.cr.rp);
  const int colR = lane_r % a.cr.nvec, rsubR = lane_r / a.cr.nvec;
  const int kvalid = min(8, a.R - colR * 8);
  const int lane_x = lane % (a.cx.nvec * a.cx.rp);
  const int colX = lane_x % a.cx.nvec, rsubX = lane_x / a.cx.nvec;
  const unsigned char* DZ = reinterpret_cast<const unsigned char*>(a.gv.dz);
  const unsigned char* Y = reinterpret_cast<const unsigned char*>(a.gv.y);
  const unsigned char* X = reinterpret_cast<const unsigned char*>(a.tv.data);
  bf16_t* GO = reinterpret_cast<bf16_t*>(a.epi.gout);

  const int nstep = (a.M + srows - 1) / srows;
  const int gw = blockIdx.x * WAVES + wave;
  const int t0 = min(nstep, gw * a.tpw), t1 = min(nstep, t0 + a.tpw);

  // native vector types: a HIP uint4 struct copied whole from a register array to LDS is not promoted to registers
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 rz[NSR], ry[(GBN && !NOY) ? NSR : 1];
  u32x4 rx[NSX], ro[BETA ? NSX : 1];
  // per-lane byte offsets inside a step (loop invariant) and the uniform byte strides between load passes: a step's
  // addresses are one scalar base + these (r03l: the 64-bit multiply-add per load and lane was ~15 % of the VALU work
  // of the expand layers)
  const uint32_t voffR = (uint32_t)(rsubR * a.gv.ld + colR * 8) * 2, voffX = (uint32_t)(rsubX * a.tv.ld + colX * 8) * 2;
  const uint32_t passR = (uint32_t)a.cr.rp * a.gv.ld * 2, passX = (uint32_t)a.cx.rp * a.tv.ld * 2;
  const int rows_touched = max(NSR * a.cr.rp, NSX * a.cx.rp);
  auto issue = [&](int t) {
    // every instantiated pass is issued, unconditionally and back to back (a load under a branch makes the compiler
    // wait for ALL outstanding loads and stores wherever one of them is consumed); a pass that reaches beyond the step
    // reads rows of the wave's NEXT step (they are in L2 when that step asks for them), rows past M re-read row M-1
    const int row0 = t * srows;
    if (row0 + rows_touched <= a.M) {
      const unsigned char* bz = DZ + (size_t)row0 * a.gv.ld * 2;
      const unsigned char* by = Y + (size_t)row0 * a.gv.ld * 2;
      const unsigned char* bx = X + (size_t)row0 * a.tv.ld * 2;
      const unsigned char* bo = reinterpret_cast<const unsigned char*>(GO) + (size_t)row0 * a.tv.ld * 2;
#pragma unroll
      for (int i = 0; i < NSR; ++i) {
        rz[i] = *reinterpret_cast<const u32x4*>(bz + (size_t)i * passR + voffR);
        if (GBN && !NOY) ry[i] = *reinterpret_cast<const u32x4*>(by + (size_t)i * passR + voffR);
      }
#pragma unroll
      for (int i = 0; i < NSX; ++i) rx[i] = *reinterpret_cast<const u32x4*>(bx + (size_t)i * passX + voffX);
      if (has_beta) {       // the gradient already in gout (residual / second consumer) rides along with x
#pragma unroll
        for (int i = 0; i < NSX; ++i) ro[BETA ? i : 0] = *reinterpret_cast<const u32x4*>(bo + (size_t)i * passX + voffX);
      }
    } else {                // the last steps of the tensor: clamp every row
#pragma unroll
      for (int i = 0; i < NSR; ++i) {
        const size_t off = ((size_t)min(row0 + i * a.cr.rp + rsubR, a.M - 1) * a.gv.ld + colR * 8) * 2;
        rz[i] = *reinterpret_cast<const u32x4*>(DZ + off);
        if (GBN && !NOY) ry[i] = *reinterpret_cast<const u32x4*>(Y + off);
      }
#pragma unroll
      for (int i = 0; i < NSX; ++i) {
        const size_t off = ((size_t)min(row0 + i * a.cx.rp + rsubX, a.M - 1) * a.tv.ld + colX * 8) * 2;
        rx[i] = *reinterpret_cast<const u32x4*>(X + off);
      }
      if (has_beta) {
#pragma unroll
        for (int i = 0; i < NSX; ++i) {
          const size_t off = ((size_t)min(row0 + i * a.cx.rp + rsubX, a.M - 1) * a.tv.ld + colX * 8) * 2;
          ro[BETA ? i : 0] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(GO) + off);
        }
      }
    }
  };

  // dW block of this wave: acc[s][l] is the 16 x 16 tile (s, l) of the (small side, large side) tile grid
  const bool ksmall = a.TK <= a.TN;
  const int TS = ksmall ? a.TK : a.TN, TL = ksmall ? a.TN : a.TK;
  f32x4 acc[FT_S][FT_L];
#pragma unroll
  for (int s = 0; s < FT_S; ++s)
#pragma unroll
    for (int l = 0; l < FT_L; ++l)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[s][l][e] = 0.f;

  float ga[8], gb[8], gc[8];
  if (GBN && !NOY) {
    loadf8(a.gv.a + colR * 8, ga); loadf8(a.gv.b + colR * 8, gb); loadf8(a.gv.cc + colR * 8, gc);
  }
  // this lane's running column sums over all its tiles (its 8 channels of every epilogue chunk never change):
  // ra = sum g, rb = sum g*x (BatchNorm backward); NOY: xacc = sum x
  float ra[NCH][8], rb[NCH][8];
#pragma unroll
  for (int ci = 0; ci < NCH; ++ci)
#pragma unroll
    for (int e = 0; e < 8; ++e) ra[ci][e] = rb[ci][e] = 0.f;
  float xacc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) xacc[e] = 0.f;
  // NOY: the Gram matrix S = x^T x of this wave's rows, 16 x 16 tiles (s, s2) of the k side
  f32x4 accS[NOY ? FT_S : 1][NOY ? FT_S : 1];
#pragma unroll
  for (int s = 0; s < (NOY ? FT_S : 1); ++s)
#pragma unroll
    for (int s2 = 0; s2 < (NOY ? FT_S : 1); ++s2)
#pragma unroll
      for (int e = 0; e < 4; ++e) accS[s][s2][e] = 0.f;
  // epilogue mapping of the 64-channel chunk ci: lanes per row = the chunk's 16-byte column groups rounded up to a
  // power of two (a 16-channel input: 2 lanes per row, all 32 rows of the tile in ONE pass instead of four passes with
  // 6 of 8 lanes idle -- the wave issues every instruction of a pass whatever the number of live lanes)
  auto chunk_lsh = [&](int ci) {
    const int nv = min(8, (a.KO - ci * ECC + 7) / 8);
    return nv <= 1 ? 0 : (nv <= 2 ? 1 : (nv <= 4 ? 2 : 3));
  };
  const int fi = lane & 15, fq = lane >> 4;        // 16x16x32 fragment coordinates
  int gateL_img = -1;                              // image whose SE gate is in gateL
  if (t0 < t1) issue(t0);
  for (int t = t0; t < t1; ++t) {
    const int rowS = t * srows;
    const int rows_step = min(srows, a.M - rowS);
    // ---- stage dy = a*dz + b*y + c (bf16, zero beyond R and beyond M), raw x and the old gradient
#pragma unroll
    for (int i = 0; i < NSR; ++i) {
      {
        const int r = i * a.cr.rp + rsubR;
        if (r < srows) {
          if (NOY) {         // dz is the matrix-core operand as it is (R % 8 == 0 on this path: whole chunks)
            u32x4 v = rz[i];
            if (r >= rows_step) v = u32x4{0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(Dt + r * a.SA + colR * 16) = v;
          } else {
            float x[8];
            unpack8(make_uint4(rz[i][0], rz[i][1], rz[i][2], rz[i][3]), x);
            if (GBN) {
              float y[8];
              const u32x4 yv = ry[(GBN && !NOY) ? i : 0];
              unpack8(make_uint4(yv[0], yv[1], yv[2], yv[3]), y);
#pragma unroll
              for (int e = 0; e < 8; ++e) x[e] = fmaf(ga[e], x[e], fmaf(gb[e], y[e], gc[e]));
            }
            if (kvalid < 8 || r >= rows_step) {
#pragma unroll
              for (int e = 0; e < 8; ++e) if (e >= kvalid || r >= rows_step) x[e] = 0.f;
            }
            *reinterpret_cast<uint4*>(Dt + r * a.SA + colR * 16) = pack8(x);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NSX; ++i) {
      {
        const int r = i * a.cx.rp + rsubX;
        if (r < srows) {
          *reinterpret_cast<u32x4*>(Xt + r * a.SX + colX * 16) = rx[i];
          if (has_beta) *reinterpret_cast<u32x4*>(Ot + r * a.SX + colX * 16) = ro[BETA ? i : 0];
        }
      }
    }
    if (t + 1 < t1) issue(t + 1);
    __builtin_amdgcn_wave_barrier();
    if (rows_step < srows) {
      // last, partial step: the rows past M hold copies of row M-1.  Their dy rows are zero, so they add nothing to dW,
      // to the sums or (the store is guarded) to gout -- except through NOY's Gram matrix and column sums of x: zero them
      const int slots = a.SX / 16;
      for (int q = lane; q < (srows - rows_step) * slots; q += 64)
        *reinterpret_cast<uint4*>(Xt + (size_t)(rows_step + q / slots) * a.SX + (q % slots) * 16) = make_uint4(0, 0, 0, 0);
      __builtin_amdgcn_wave_barrier();
    }

    for (int g = 0; g < a.G; ++g) {
      const int row0 = rowS + g * TR;
      if (row0 >= a.M) break;
      const int rows_valid = min(TR, a.M - row0);
      unsigned char* Dg = Dt + (size_t)g * TR * a.SA;
      unsigned char* Xg = Xt + (size_t)g * TR * a.SX;
      const unsigned char* Og = Ot + (size_t)g * TR * a.SX;
      const int img0 = row0 / a.hw;
      // STRADDLE = false: the host guarantees hw % 32 == 0 wherever a gate is involved -- a tile lies in one image
      const bool one_img = !STRADDLE || img0 == (row0 + rows_valid - 1) / a.hw;
      // SE gate of the tile's image -> LDS (once per image and wave: this load does wait behind the prefetch)
      if (gated && one_img && img0 != gateL_img) {
        for (int c = lane; c < a.KO; c += 64) gateL[c] = a.tv.gate[(size_t)img0 * a.KO + c];
        gateL_img = img0;
        __builtin_amdgcn_wave_barrier();
      }

      // ---- data gradient, 64 input channels at a time, and the activated operand for the weight gradient
      const unsigned char* arow = Dg + (size_t)j * a.SA + h * 16;
#pragma unroll
      for (int ci = 0; ci < NCH; ++ci) {
        const int c0 = ci * ECC;
        if (c0 < a.KOpad) {
          const int ccols = min(ECC, a.KOpad - c0);                // 32 or 64
          const int lsh = chunk_lsh(ci);
          const int ecol = lane & ((1 << lsh) - 1), erow = lane >> lsh, rpp = 64 >> lsh;
          const int ch0 = c0 + ecol * 8;                           // this lane's 8 channels (KO % 8 == 0: all or none)
          const bool col_ok = ch0 < a.KO;
          float sc[8], sh[8], gt[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) { sc[e] = 1.f; sh[e] = 0.f; gt[e] = 1.f; }
          if (col_ok) {
            loadf8(coefS + ch0, sc);
            loadf8(coefH + ch0, sh);
            if (gated && one_img) loadf8(gateL + ch0, gt);
          }
          for (int nt = 0; nt < ccols / 32; ++nt) {
            f32x16 d = mma_tile(Wl + (size_t)(c0 + nt * 32 + j) * a.SW + h * 16, arow, a.ksteps);
            if (NOY)         // + x G: the rows of Xt (raw x = the forward's operand on this path) against G
              d = mma_tile_more(Gl + (size_t)(c0 + nt * 32 + j) * a.SG + h * 16, Xg + (size_t)j * a.SX + h * 16, a.kxsteps, d);
#pragma unroll
            for (int q = 0; q < 4; ++q)
              *reinterpret_cast<float4*>(Ct + j * a.SC + (nt * 32 + 8 * q + 4 * h) * 4) =
                  make_float4(d[4 * q + 0], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
          }
          __builtin_amdgcn_wave_barrier();
          float vv[8];
          if (NOY) {
#pragma unroll
            for (int e = 0; e < 8; ++e) vv[e] = 0.f;
            if (col_ok) loadf8(vL + ch0, vv);
          }
          // one row of the lane's 8 channels
          auto pass = [&](int r) {
            uint4* xslot = reinterpret_cast<uint4*>(Xg + r * a.SX + (c0 / 8 + ecol) * 16);
            const float4 d0 = *reinterpret_cast<const float4*>(Ct + r * a.SC + ecol * 32);
            const float4 d1 = *reinterpret_cast<const float4*>(Ct + r * a.SC + ecol * 32 + 16);
            float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
            float x[8], gg[8], av[8];
            unpack8(*xslot, x);
            if (NOY) {
#pragma unroll
              for (int e = 0; e < 8; ++e) { d[e] += vv[e]; xacc[e] += x[e]; }     // xacc: sum_p x (the s of dW)
            }
            // z (pre-activation), its activation av and the chained gradient gg
            if (swish) {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float z = fmaf(x[e], sc[e], sh[e]);
                const float sg = sigmoidf_(z);
                av[e] = z * sg;
                gg[e] = d[e] * (sg * (1.0f + z * (1.0f - sg)));
              }
            } else {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                av[e] = fmaf(x[e], sc[e], sh[e]);
                gg[e] = d[e];
              }
            }
            if (gated) {
              if (STRADDLE && !one_img) loadf8(a.tv.gate + (size_t)(min(row0 + r, a.M - 1) / a.hw) * a.KO + ch0, gt);
#pragma unroll
              for (int e = 0; e < 8; ++e) av[e] *= gt[e];
            }
            if (has_beta) {
              float old[8];
              unpack8(*reinterpret_cast<const uint4*>(Og + r * a.SX + (c0 / 8 + ecol) * 16), old);
#pragma unroll
              for (int e = 0; e < 8; ++e) gg[e] += old[e];
            }
            if (r < rows_valid) *reinterpret_cast<uint4*>(GO + (size_t)(row0 + r) * a.tv.ld + ch0) = pack8(gg);
            *xslot = pack8(av);
            if (want_stats) {      // raw sums (g, g*x): sum g*(x-mean)*rstd is taken from the totals at the end
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                ra[ci][e] += gg[e];
                rb[ci][e] = fmaf(gg[e], x[e], rb[ci][e]);
              }
            }
          };
          if (col_ok) {
            if (lsh == 3) {
#pragma unroll
              for (int p = 0; p < 4; ++p) pass(p * 8 + erow);
            } else {
              for (int r = erow; r < TR; r += rpp) pass(r);
            }
          }
          __builtin_amdgcn_wave_barrier();
        }
      }

      // ---- weight gradient: dW[k][n] += sum over the tile's 32 rows of xa[row][k] * dy[row][n]
      {
        const unsigned char* St = ksmall ? Xg : Dg;      // small side: fragments kept in registers
        const unsigned char* Lt = ksmall ? Dg : Xg;
        const int sS = ksmall ? a.SX : a.SA, sL = ksmall ? a.SA : a.SX;
        bf16x8 sf[FT_S];
#pragma unroll
        for (int s = 0; s < FT_S; ++s)
          if (s < TS) sf[s] = column_frag_tr(St, sS, fq * 8, s * 16, fi);
        if (NOY) {           // S = x^T x (ksmall on this path: sf are the fragments of x)
#pragma unroll
          for (int s = 0; s < FT_S; ++s)
#pragma unroll
            for (int s2 = 0; s2 < FT_S; ++s2)
              if (s < TS && s2 < TS)
                accS[NOY ? s : 0][NOY ? s2 : 0] =
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(sf[s], sf[s2], accS[NOY ? s : 0][NOY ? s2 : 0], 0, 0, 0);
        }
#pragma unroll
        for (int l = 0; l < FT_L; ++l) {
          if (l < TL) {
            const bf16x8 lf = column_frag_tr(Lt, sL, fq * 8, l * 16, fi);
#pragma unroll
            for (int s = 0; s < FT_S; ++s) {
              if (s < TS) {
                // A = the k side (rows of dW), B = the n side (columns of dW)
                if (ksmall) acc[s][l] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sf[s], lf, acc[s][l], 0, 0, 0);
                else acc[s][l] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lf, sf[s], acc[s][l], 0, 0, 0);
              }
            }
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (NOY) {     // the lanes' column sums -> wst[0 .. KO) (the row-lanes of a column: LDS atomics, once per kernel)
    const int ch0 = (lane & ((1 << chunk_lsh(0)) - 1)) * 8;
    if (ch0 < a.KO) {
#pragma unroll
      for (int e = 0; e < 8; ++e) atomicAdd(&wst[ch0 + e], xacc[e]);
    }
    __builtin_amdgcn_wave_barrier();
  }
  const float xsum = (NOY && lane < a.KO) ? wst[lane] : 0.f;      // NOY: this wave's sum_p x[p][lane] (KO <= 32)
  if (want_stats) {
#pragma unroll
    for (int ci = 0; ci < NCH; ++ci) {
      const int ch0 = ci * ECC + (lane & ((1 << chunk_lsh(ci)) - 1)) * 8;
      if (ch0 < a.KO) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          atomicAdd(&wst[ch0 + e], ra[ci][e]);
          atomicAdd(&wst[a.KOpad + ch0 + e], rb[ci][e]);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    // the four waves in wave order (r04: no cross-wave LDS atomics -- the same sums on every run)
    for (int w = 0; w < WAVES; ++w) {
      if (wave == w) {
        for (int c = lane; c < a.KO; c += 64) {
          red[c] += wst[c];
          red[a.KOpad + c] += wst[a.KOpad + c];
        }
      }
      __syncthreads();
    }
    float* dst = a.epi.stat_partials + (size_t)blockIdx.x * 2 * a.KO;
    for (int c = tid; c < a.KO; c += THREADS) {
      const float sg = red[c], sgx = red[a.KOpad + c];
      dst[c] = sg;
      dst[a.KO + c] = a.epi.rstd[c] * (sgx - a.epi.mean[c] * sg);      // sum g*(x-mean)*rstd
    }
  }
  // ---- dW blocks of the four waves -> one partial per workgroup (fixed order: deterministic)
  __syncthreads();
  float* scratch = reinterpret_cast<float*>(smem);      // [KO][R] fp32; every LDS tile is dead by now
  for (int w = 0; w < WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int s = 0; s < FT_S; ++s)
#pragma unroll
        for (int l = 0; l < FT_L; ++l) {
          if (s < TS && l < TL) {
            const int tk = ksmall ? s : l, tn = ksmall ? l : s;
            const int n = tn * 16 + fi;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int k = tk * 16 + fq * 4 + e;
              if (k < a.KO && n < a.R) {
                float* p = scratch + (size_t)k * a.R + n;
                *p = (w == 0 ? 0.f : *p) + acc[s][l][e];
              }
            }
          }
        }
    }
    __syncthreads();
  }
  const size_t part = (size_t)a.KO * a.R + (NOY ? (size_t)a.KO * a.KO + a.KO : 0);
  float* dstw = a.ws + (size_t)blockIdx.x * part;
  for (int i = tid; i < a.KO * a.R; i += THREADS) dstw[i] = scratch[i];
  if (NOY) {
    // [S | s] behind P: the waves' Gram tiles and column sums in wave order (deterministic)
    __syncthreads();
    float* sS = scratch;                                  // [KO][KO]
    float* ss = scratch + (size_t)a.KO * a.KO;            // [KO]
    for (int w = 0; w < WAVES; ++w) {
      if (wave == w) {
#pragma unroll
        for (int s = 0; s < FT_S; ++s)
#pragma unroll
          for (int s2 = 0; s2 < FT_S; ++s2) {
            if (s < TS && s2 < TS) {
              const int k2 = s2 * 16 + fi;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int k = s * 16 + fq * 4 + e;
                if (k < a.KO && k2 < a.KO) {
                  float* p = sS + (size_t)k * a.KO + k2;
                  *p = (w == 0 ? 0.f : *p) + accS[NOY ? s : 0][NOY ? s2 : 0][e];
                }
              }
            }
          }
        if (lane < a.KO) ss[lane] = (w == 0 ? 0.f : ss[lane]) + xsum;
      }
      __syncthreads();
    }
    for (int i = tid; i < a.KO * a.KO + a.KO; i += THREADS) dstw[(size_t)a.KO * a.R + i] = scratch[i];
  }
}

// NOY: dW[k][n] += a[n] P[k][n] + b[n] sum_k' S[k][k'] W[k'][n] + c[n] s[k] from the summed partial [P | S | s]
__global__ __launch_bounds__(256) void k_noy_apply(const float* __restrict__ psum, const bf16_t* __restrict__ W, int ldw,
                                                  int KO, int R, const float* __restrict__ ga,
                                                  const float* __restrict__ gb, const float* __restrict__ gc,
                                                  float* __restrict__ dweight) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= KO * R) return;
  const int k = i / R, n = i - k * R;
  const float* S = psum + (size_t)KO * R + (size_t)k * KO;
  float t = 0.f;
  for (int k2 = 0; k2 < KO; ++k2) t = fmaf(S[k2], bf2f(W[(size_t)k2 * ldw + n]), t);
  dweight[i] += ga[n] * psum[i] + gb[n] * t + gc[n] * psum[(size_t)KO * R + (size_t)KO * KO + k];
}

// The instantiations, each with what the host compares to choose it: the form (class A through y or NOY, class B with a
// 4 x 4 or a 3 x 9 tile grid), the load passes (NSR, NSX) and GBN.  Among the rows of one form and GBN the host takes the
// pair that wastes the fewest loads, the earlier row on a tie.
enum { FUSED_A = 0, FUSED_NOY, FUSED_44, FUSED_39 };
struct FusedVariant {
  int form, nsr, nsx;
  bool gbn;
  void (*kern)(const FusedArgs);
};
template <int NSR, int NSX, bool GBN, int FT_S, int FT_L, bool NOY, int NCH, bool BETA>
constexpr FusedVariant fused_variant() {
  return {NOY ? FUSED_NOY : FT_S == 2 ? FUSED_A : FT_S == 4 ? FUSED_44 : FUSED_39, NSR, NSX, GBN,
          k_pw_bwd_fused<NSR, NSX, GBN, FT_S, FT_L, NOY, NCH, BETA, BETA>};
}
static const FusedVariant fused_variants[] = {
    fused_variant<13, 2, true, 2, 9, true, 1, true>(),    fused_variant<22, 4, true, 2, 9, true, 1, true>(),
    fused_variant<12, 4, true, 2, 9, false, 1, true>(),   fused_variant<12, 4, false, 2, 9, false, 1, true>(),
    fused_variant<4, 8, true, 4, 4, false, 1, false>(),   fused_variant<4, 8, false, 4, 4, false, 1, false>(),
    fused_variant<2, 11, true, 3, 9, false, 3, false>(),  fused_variant<2, 11, false, 3, 9, false, 3, false>(),
    fused_variant<3, 11, true, 3, 9, false, 3, false>(),  fused_variant<3, 11, false, 3, 9, false, 3, false>(),
    fused_variant<2, 7, true, 3, 9, false, 3, false>(),   fused_variant<2, 7, false, 3, 9, false, 3, false>()};

}  // namespace pws

// Both gradients of one pointwise layer in one pass (outside the envelope the caller runs the two separate kernels).
// dweight [KO][R] fp32 is accumulated into (edet_reduce_partials).
int pws_try_bwd_fused(const edet_gview_t* dy, const void* w, int ldw, const edet_tview_t* in,
                      const edet_bwd_epi_t* epi, int* nparts_out, float* dweight, void* workspace,
                      size_t workspace_bytes, hipStream_t st) {
  if (in->act > EDET_ACT_SWISH) return 0;     // relu / relu6 / hswish: the two streaming kernels (OACT instantiations)
  using namespace pws;
  const int R = dy->c, KO = in->c;
  if (!workspace || KO % 8 != 0 || dy->ld % 8 != 0 || in->ld % 8 != 0 || R > 160 || KO > 160) return 0;
  if (epi->stat_partials && epi->dgate) return 0;
  if (in->gate && epi->dgate) return 0;               // this kernel forms no SE gate-gradient sums (r06: its own were global atomics): the
                                                      // tiled one-pass kernel (ordered slots) or the two-kernel path + k_gate_sums do
  FusedArgs a;
  memset(&a, 0, sizeof(a));
  a.gv = *dy; a.tv = *in; a.W = reinterpret_cast<const bf16_t*>(w); a.ldw = ldw; a.epi = *epi;
  a.ws = reinterpret_cast<float*>(workspace);
  a.M = in->n * in->h * in->w; a.R = R; a.KO = KO; a.hw = in->h * in->w;
  a.TK = (KO + 15) / 16; a.TN = (R + 15) / 16;
  // Envelope = the instantiations below.  Class A, the "expand" shape (few input channels, many output channels:
  // R >= 2 KO, dW <= 2 x 9 tiles of 16 x 16).  r02d, D0 640x640 batch 128, both gradients: 320x320x16->96 2.44 -> 1.95
  // ms, 160x160x24->144 1.45 -> 0.73 ms.  Class B (r03): at most 64 output channels -- the project layers (dW <= 3 x 9
  // tiles) and the 64 -> 64 layers (4 x 4) -- which the round-2 kernel ran slower than the two-kernel path because it
  // issued 5-8x the gradient loads a tile needs (every instantiated pass) and paid 16-48 LDS atomics per tile for the
  // per-channel sums; EDET_PWS_FUSED_WIDE=0 keeps class A only (test selector, read per call).
  const int tmin = a.TK < a.TN ? a.TK : a.TN, tmax = a.TK < a.TN ? a.TN : a.TK;
  const bool class_a = R >= 2 * KO && a.TK <= 2 && a.TN <= 9;
  int form = FUSED_A;                                   // class B: the tile grid, 4 x 4 or 3 x 9; class A: NOY, below
  if (!class_a) {
    if (edet_env_int("EDET_PWS_FUSED_WIDE", 1) == 0) return 0;
    // project shape only.  r03m: the 64 -> 64 layers of the BiFPN / heads (plain input view, no chain epilogue) take
    // 0.181 ms one-pass against 0.169 ms for the two tiled kernels at 80x80, and a kernel that owns every register of
    // a CU shuts out the small pyramid levels' chain on the second stream (the step did not move: 64.6 ms)
    if (KO < 2 * R) return 0;
    if (R > 64 || epi->beta) return 0;       // class B instantiations do not accumulate into gout
    // r04: the one-pass TILED kernel (pw_tile_bwd.hip) takes the project layers from 96 input channels up -- lab, D0
    // 640x640 batch 128: 160x160x96->24 0.436 against 0.582 ms here, 80x80x144->40 0.226 / 0.274, 160x160x144->24 0.803 /
    // 0.796 (a tie, and the tiled kernel has no atomics); 320x320x32->16 stays here (0.787 against 0.841 ms).
    // EDET_PWT=0 (the tiled kernel off) restores the round-3 envelope.
    // ... and every SE-gated projection: the tiled kernel forms the gate-gradient sums in a fixed order, this one could only
    // with global atomics (r06, since removed; 320x320x32->16: 0.84 against 0.79 ms here -- the price of a reproducible step)
    if ((KO > 32 || in->gate) && edet_env_int("EDET_PWT", 1) != 0) return 0;
    if (in->gate && a.hw % TR != 0) return 0;   // ... and take every 32-row tile to lie in one image where a gate is involved
    if (tmax <= 4 && KO <= 64) form = FUSED_44;
    else if (tmin <= 3 && tmax <= 9) form = FUSED_39;
    else return 0;
    // r03k lab, 64 -> 64: 80x80 (819 K rows) 0.219 -> 0.165 ms, 40x40 (205 K rows) 0.071 -> 0.070, 20x20 0.030 -> 0.054:
    // the prologue, the LDS reduction of dW and one wave per SIMD need ~250 K rows to pay off
    if (a.M < edet_env_int("EDET_PWS_FUSED_MINROWS", 262144)) return 0;
  }
  a.cr = make_colmap(R);
  a.cx = make_colmap(KO);
  const int Rp = (R + 7) / 8 * 8;
  a.ksteps = (R + 15) / 16;
  a.SA = frag_stride(Rp, Rp % 16 != 0);
  a.SW = a.SA;
  a.SX = frag_stride(KO, false);
  a.KOpad = (KO + 31) / 32 * 32;
  if (a.SX < a.KOpad * 2) a.SX = frag_stride(a.KOpad, false);     // the epilogue addresses whole 32-channel tiles
  a.SC = ECC * 4 + 16;
  const bool gbn = dy->a != nullptr;
  // NOY: BatchNorm backward without the saved convolution output (see the kernel's header): dy carries a BatchNorm
  // backward, the input is a plain stored tensor (x~ = x; no chain epilogue), whole 16-byte chunks of dz.
  // EDET_PW_NOY=0 keeps the form that reads y (test selector, read per call).  r03c, first version (column sums of x through
  // 16 LDS atomics per tile): SLOWER than reading y, 320x320x16->96 1.86 -> 2.31 ms -- the kernel runs one wave per SIMD
  // with one tile of loads in flight and is bound by that latency, not by bytes.  r03d, sums kept in registers across the
  // tiles: 1.90 -> 1.75 ms, 160x160x24->144 0.76 -> 0.68 ms (-8 / -10 %), with 43 % less traffic.
  const bool noy = class_a && gbn && (epi->flags & EDET_EPI_Y_IS_CONV_OF_INPUT) && dy->b && dy->cc && !in->scale && !in->gate &&
                   in->act == EDET_ACT_NONE &&
                   !epi->stat_partials && !epi->dgate && R % 8 == 0 && KO <= 32 && edet_env_int("EDET_PW_NOY", 1) != 0;
  if (noy) form = FUSED_NOY;
  a.SG = frag_stride(a.KOpad, false);
  a.kxsteps = (KO + 15) / 16;
  const size_t part = (size_t)KO * R + (noy ? (size_t)KO * KO + KO : 0);      // floats per workgroup partial
  // Rows in flight: G tiles of 32 rows per step, as many as an instantiated (NSR, NSX) pair of load passes covers
  // without loading more than ~30 % past the step, the LDS (150 KB) and a budget of ~24 KB of loads per wave allow (the
  // kernel runs one wave per SIMD: the bytes in flight per wave ARE the latency hiding).  r03j, D0 640x640 batch 128:
  // 320x320x32->16 1.87 / 1.57 / 1.43 ms at G = 1 / 2 / 4.  The pairs are the rows of fused_variants with this call's form
  // and GBN, in table order.
  const int rbytes = ((gbn && !noy) ? 2 : 1) * Rp * 2, xbytes = (epi->beta ? 2 : 1) * KO * 2;
  size_t lds = 0;
  const FusedVariant* pick = nullptr;
  double pick_waste = 1e30;
  a.G = 0;
  for (int g = 4; g >= 1; --g) {
    const int nsr = (TR * g + a.cr.rp - 1) / a.cr.rp, nsx = (TR * g + a.cx.rp - 1) / a.cx.rp;
    if (g > 1 && TR * g * (rbytes + xbytes) > 24 * 1024) continue;
    const size_t l = (size_t)a.KOpad * a.SW + (size_t)4 * a.KOpad * 4 +
                     (noy ? (size_t)a.KOpad * 4 + (size_t)a.KOpad * a.SG : 0) +
                     (size_t)WAVES * ((size_t)TR * g * a.SA + (size_t)(epi->beta ? 2 : 1) * TR * g * a.SX +
                                      (size_t)TR * a.SC + (size_t)4 * a.KOpad * 4);
    if (l > 150 * 1024) continue;
    for (const FusedVariant& v : fused_variants) {
      if (v.form != form || v.gbn != gbn || v.nsr < nsr || v.nsx < nsx) continue;
      const double waste = ((double)(v.nsr * a.cr.rp - TR * g) * rbytes + (double)(v.nsx * a.cx.rp - TR * g) * xbytes) /
                           ((double)TR * g * (rbytes + xbytes));
      if (waste < pick_waste - 1e-9 && (!pick || pick_waste > 0.3)) {
        pick = &v; pick_waste = waste; a.G = g; lds = l;
      }
    }
    if (pick && pick_waste <= 0.3) break;
  }
  if (!pick || lds < (size_t)KO * R * 4 + (noy ? (size_t)(KO * KO + KO) * 4 : 0)) return 0;
  const int nstep = (a.M + TR * a.G - 1) / (TR * a.G);
  // one workgroup per compute unit, a single round (r03d lab: grids of 1024 / 512 / 256 -> 320x320x16->96 1.90 / 1.83 /
  // 1.81 ms, 160x160x24->144 0.69 / 0.64 / 0.61 ms: every workgroup pays the prologue and the dW partial once); at
  // least 2 steps per wave, partials bounded by the workspace
  int grid = 256;
  const int64_t max_by_ws = (int64_t)(workspace_bytes / sizeof(float)) / (int64_t)part - (noy ? 1 : 0);
  if (grid > max_by_ws) grid = (int)max_by_ws;
  if (grid > EDET_MAX_PARTS) grid = EDET_MAX_PARTS;
  const int max_by_steps = (nstep + WAVES * 2 - 1) / (WAVES * 2);
  if (grid > max_by_steps) grid = max_by_steps;
  if (grid < 1) return 0;
  grid = spread_over_waves(nstep, grid, &a.tpw);
  if (nparts_out) *nparts_out = grid;
  if (!edet_lds_optin(pick->kern, lds)) return 0;
  edet_launch(pick->kern, dim3(grid), dim3(THREADS), lds, st, a);
  EDET_LAUNCH_CHECK("edet_pw_bwd(fused)");
  if (noy) {
    // partials [grid][P | S | s] -> their sum behind them in the workspace -> dW
    float* psum = a.ws + (size_t)grid * part;
    if (edet_reduce_partials_set(a.ws, grid, (int64_t)part, psum, st) != 0) return -2;
    edet_launch(k_noy_apply, dim3((KO * R + 255) / 256), dim3(256), 0, st, psum, a.W, ldw, KO, R, dy->a, dy->b, dy->cc, dweight);
    EDET_LAUNCH_CHECK("edet_pw_bwd(noy apply)");
    return 1;
  }
  if (edet_reduce_partials(a.ws, grid, (int64_t)KO * R, dweight, st) != 0) return -2;
  return 1;
}
