// BatchNorm statistics (forward finalize / backward reduce + finalize), block-output materialisation, elementwise add.
//
// Reference: efficientdet/utils.py:166-266 (BatchNorm classes, eps 1e-3, momentum 0.99),
// efficientdet/tf2/util_keras.py:29-66, efficientdet/backbone/efficientnet_model.py:393-410 (project BN + identity skip).
#include "rowmap_impl.h"

namespace {

constexpr int THREADS = 256;
static_assert(THREADS == ROW_THREADS, "the row map is laid out for this workgroup size");

// ------------------------------------------------------------------ forward statistics finalize
// Column sums of the [nparts][2][c] partial rows: one 1024-lane workgroup per FIN_CH channels, FIN_SL row slices per
// channel (8 rows = 16 independent loads in flight per thread), fp64 accumulation, the slices added in order at the end.
constexpr int FIN_SL = 64;      // r05d, same box, 30 steps: 32 -> 50.99 / 50.87 ms, 64 -> 50.71 ms, 64 + DEEP 50.97, 32 + DEEP 51.81
constexpr int FIN_CH = 1024 / FIN_SL;   // 1024-lane workgroups: FIN_SL rows of partials per step

__device__ __forceinline__ void partial_colsum(const float* __restrict__ partials, int nparts, int c, int ch,
                                               int slice, double& s, double& s2) {
  double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
  if (ch < c) {
    int p = slice;
    // eight rows (16 loads) in flight per thread first -- the kernel is a chain of L2 latencies, ~10 us of step time per
    // launch and 216 launches per EfficientDet-D0 step -- added in exactly the order of the two-row loop below (same bits)
    for (; p + 7 * FIN_SL < nparts; p += 8 * FIN_SL) {
      float u[8], v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        u[i] = partials[((size_t)(p + i * FIN_SL) * 2) * c + ch];
        v[i] = partials[((size_t)(p + i * FIN_SL) * 2 + 1) * c + ch];
      }
#pragma unroll
      for (int i = 0; i < 8; i += 2) { a0 += (double)u[i]; b0 += (double)v[i]; a1 += (double)u[i + 1]; b1 += (double)v[i + 1]; }
    }
    for (; p + FIN_SL < nparts; p += 2 * FIN_SL) {
      const float u0 = partials[((size_t)p * 2) * c + ch], v0 = partials[((size_t)p * 2 + 1) * c + ch];
      const float u1 = partials[((size_t)(p + FIN_SL) * 2) * c + ch];
      const float v1 = partials[((size_t)(p + FIN_SL) * 2 + 1) * c + ch];
      a0 += (double)u0; b0 += (double)v0; a1 += (double)u1; b1 += (double)v1;
    }
    if (p < nparts) {
      a0 += (double)partials[((size_t)p * 2) * c + ch];
      b0 += (double)partials[((size_t)p * 2 + 1) * c + ch];
    }
  }
  __shared__ double red[2][FIN_SL][FIN_CH];
  const int cl = threadIdx.x & (FIN_CH - 1);
  red[0][slice][cl] = a0 + a1;
  red[1][slice][cl] = b0 + b1;
  __syncthreads();
  // the slices in two fixed levels (r06: one thread adding all FIN_SL slices was a chain of FIN_SL dependent LDS reads,
  // ~1 us of a ~6 us kernel that runs 216 times per step): FIN_G leaders add FIN_SL / FIN_G consecutive slices each,
  // slice 0 adds the leaders in order -- the same tree on every run
  constexpr int FIN_G = 8, PER = FIN_SL / FIN_G;
  static_assert(FIN_SL % FIN_G == 0, "slice groups");
  double u = 0.0, v = 0.0;
  if (slice < FIN_G) {
#pragma unroll
    for (int i = 0; i < PER; ++i) { u += red[0][slice * PER + i][cl]; v += red[1][slice * PER + i][cl]; }
  }
  __syncthreads();                   // every leader has read its slices before any of them overwrites rows 0 .. FIN_G - 1
  if (slice < FIN_G) {
    red[0][slice][cl] = u;
    red[1][slice][cl] = v;
  }
  __syncthreads();
  s = 0.0; s2 = 0.0;
  if (slice == 0) {
#pragma unroll
    for (int i = 0; i < FIN_G; ++i) { s += red[0][i][cl]; s2 += red[1][i][cl]; }
  }
}

__global__ __launch_bounds__(FIN_CH * FIN_SL) void k_bn_finalize(
    const float* __restrict__ partials, int nparts, int c, double count, const float* gamma, const float* beta,
    float eps, float momentum, int bessel, float* moving_mean, float* moving_var, float* scale, float* shift,
    float* mean_out, float* rstd_out) {
  const int ch = blockIdx.x * FIN_CH + (threadIdx.x & (FIN_CH - 1));
  const int slice = threadIdx.x / FIN_CH;
  double s, s2;
  partial_colsum(partials, nparts, c, ch, slice, s, s2);
  if (slice != 0 || ch >= c) return;
  const double mean = s / count;
  double var = s2 / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = gamma[ch] * rstd;
  scale[ch] = sc;
  shift[ch] = beta[ch] - (float)mean * sc;
  mean_out[ch] = (float)mean;
  rstd_out[ch] = rstd;
  if (momentum >= 0.f && moving_mean) {
    // Keras fused BatchNorm (the single-replica classes): moving variance is updated with the Bessel-corrected batch
    // variance; SyncBatchNormalization / TpuBatchNormalization run un-fused (utils.py:172,211): biased variance
    const double unbiased = (bessel && count > 1.0) ? var * count / (count - 1.0) : var;
    moving_mean[ch] = moving_mean[ch] * momentum + (float)mean * (1.f - momentum);
    moving_var[ch] = moving_var[ch] * momentum + (float)unbiased * (1.f - momentum);
  }
}

__global__ void k_bn_eval(int c, const float* gamma, const float* beta, float eps,
                          const float* moving_mean, const float* moving_var, float* scale, float* shift) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  const float sc = gamma[ch] * rsqrtf(moving_var[ch] + eps);
  scale[ch] = sc;
  shift[ch] = beta[ch] - moving_mean[ch] * sc;
}

// ------------------------------------------------------------------ backward reduce / finalize
template <typename T>
__global__ __launch_bounds__(THREADS) void k_bn_bwd_reduce(const T* __restrict__ dz, const T* __restrict__ y,
                                                          int64_t rows, int c, int ld, const float* mean,
                                                          const float* rstd, float* partials, RowMap m) {
  const int tid = threadIdx.x;
  const int cv = tid % m.tpr, rr = tid / m.tpr;
  extern __shared__ float red[];  // [2][c] + scratch [2][THREADS * 8]
  float* scr = red + 2 * c;
  // channel blocks of tpr*8 (<= 2048) channels: one iteration for every layer up to 2048 channels, two for the
  // widest EfficientNet-B3..B7 stages
  for (int cb = 0; cb < c; cb += m.tpr * 8) {
    const int c0 = cb + cv * 8;
    const bool ok = c0 < c;
    float mu[8], rs[8], s1[8], s2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { mu[e] = 0.f; rs[e] = 0.f; s1[e] = s2[e] = 0.f; }
    if (ok) {
      loadf8(mean + c0, mu);
      loadf8(rstd + c0, rs);
      // three rows (six 16-byte loads) in flight per thread, see k_se_pool (se.hip); sums in row order
      const int64_t st = (int64_t)gridDim.x * m.rpp;
      int64_t r = (int64_t)blockIdx.x * m.rpp + rr;
      for (; r + 2 * st < rows; r += 3 * st) {
        float g[3][8], x[3][8];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          load8<T>(dz + (r + u * st) * ld + c0, g[u]);
          load8<T>(y + (r + u * st) * ld + c0, x[u]);
        }
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
          for (int e = 0; e < 8; ++e) { s1[e] += g[u][e]; s2[e] += g[u][e] * (x[u][e] - mu[e]) * rs[e]; }
      }
      for (; r < rows; r += st) {
        float g[8], x[8];
        load8<T>(dz + r * ld + c0, g);
        load8<T>(y + r * ld + c0, x);
#pragma unroll
        for (int e = 0; e < 8; ++e) { s1[e] += g[e]; s2[e] += g[e] * (x[e] - mu[e]) * rs[e]; }
      }
    }
    rowlane_sums(scr, m, cv, rr, ok, s1, s2, red, cb, c);
  }
  __syncthreads();
  for (int i = tid; i < 2 * c; i += THREADS) partials[(size_t)blockIdx.x * 2 * c + i] = red[i];
}

__global__ __launch_bounds__(FIN_CH * FIN_SL) void k_bn_bwd_finalize(
    const float* __restrict__ partials, int nparts, int c, double count, const float* gamma, const float* mean,
    const float* rstd, float* dgamma, float* dbeta, float* a, float* b, float* cc) {
  const int ch = blockIdx.x * FIN_CH + (threadIdx.x & (FIN_CH - 1));
  const int slice = threadIdx.x / FIN_CH;
  double s1, s2;
  partial_colsum(partials, nparts, c, ch, slice, s1, s2);
  if (slice != 0 || ch >= c) return;
  if (dbeta) dbeta[ch] += (float)s1;
  if (dgamma) dgamma[ch] += (float)s2;
  const double m1 = s1 / count, m2 = s2 / count;
  const double g = gamma[ch], r = rstd[ch], mu = mean[ch];
  // dy = g*r*(dz - m1 - xhat*m2), xhat = (y - mu)*r
  a[ch] = (float)(g * r);
  b[ch] = (float)(-g * r * r * m2);
  cc[ch] = (float)(-g * r * m1 + g * r * r * m2 * mu);
}

// ------------------------------------------------------------------ out = y*scale+shift (+res)
template <typename T>
__global__ void k_bn_res(const edet_tview_t y, const T* __restrict__ res, T* __restrict__ out, int ldo,
                         int64_t rows) {
  const int nvec = y.c / 8;
  const int64_t total = rows * nvec;
  const int hw = y.h * y.w;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = q / nvec;
    const int c0 = (int)(q - r * nvec) * 8;
    float x[8];
    load8<T>(reinterpret_cast<const T*>(y.data) + r * y.ld + c0, x);
    ViewCoef vc;
    view_load_coef(y, c0, vc);
    view_apply(y, vc, c0, y.gate ? (int)(r / hw) : 0, x);   // gate [n][c]: stochastic-depth scale per image
    if (res) {
      float rr[8];
      load8<T>(res + r * ldo + c0, rr);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] += rr[e];
    }
    store8<T>(out + r * ldo + c0, x);
  }
}

template <typename T>
__global__ void k_add(T* __restrict__ dst, const T* __restrict__ src, int64_t rows, int c, int ld, int beta) {
  const int nvec = c / 8;
  const int64_t total = rows * nvec;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = q / nvec;
    const int c0 = (int)(q - r * nvec) * 8;
    float x[8];
    load8<T>(src + r * ld + c0, x);
    if (beta) {
      float d[8];
      load8<T>(dst + r * ld + c0, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] += d[e];
    }
    store8<T>(dst + r * ld + c0, x);
  }
}

}  // namespace

extern "C" int edet_bn_finalize(const float* partials, int nparts, int c, double count, const float* gamma,
                                const float* beta, float eps, float momentum, int bessel, float* moving_mean,
                                float* moving_var, float* scale, float* shift, float* mean, float* rstd, void* stream) {
  EDET_CHECK(partials && gamma && beta && scale && shift && mean && rstd, "edet_bn_finalize: null pointer");
  edet_launch(k_bn_finalize, dim3(cdiv(c, FIN_CH)), dim3(FIN_CH * FIN_SL), 0, to_stream(stream), partials, nparts, c, count,
              gamma, beta, eps, momentum, bessel, moving_mean, moving_var, scale, shift, mean, rstd);
  EDET_LAUNCH_CHECK("edet_bn_finalize");
  return 0;
}

extern "C" int edet_bn_eval(int c, const float* gamma, const float* beta, float eps, const float* moving_mean,
                            const float* moving_var, float* scale, float* shift, void* stream) {
  EDET_CHECK(gamma && beta && moving_mean && moving_var && scale && shift, "edet_bn_eval: null pointer");
  edet_launch(k_bn_eval, dim3(cdiv(c, 128)), dim3(128), 0, to_stream(stream), c, gamma, beta, eps, moving_mean, moving_var, scale, shift);
  EDET_LAUNCH_CHECK("edet_bn_eval");
  return 0;
}

extern "C" int edet_bn_bwd_reduce(const void* dz, const void* y, int64_t rows, int c, int ld,
                                  const float* mean, const float* rstd, float* stat_partials,
                                  int* nparts_out, int dtype, void* stream) {
  EDET_CHECK(dz && y && mean && rstd && stat_partials, "edet_bn_bwd_reduce: null pointer");
  EDET_CHECK(c % 8 == 0 && ld % 8 == 0 && c <= 6144, "edet_bn_bwd_reduce: c/ld must be multiples of 8, c <= 6144");
  const RowMap m = row_map(c);
  const int grid = persistent_grid(rows, m.rpp, 512);
  if (nparts_out) *nparts_out = grid;
  const size_t lds = (size_t)(2 * c + 2 * THREADS * 8) * sizeof(float);
  const bool known = dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    edet_launch(k_bn_bwd_reduce<T>, grid, dim3(THREADS), lds, to_stream(stream), (const T*)dz, (const T*)y, rows, c, ld, mean, rstd, stat_partials, m);
  });
  EDET_CHECK(known, "edet_bn_bwd_reduce: bad dtype %d", dtype);
  EDET_LAUNCH_CHECK("edet_bn_bwd_reduce");
  return 0;
}

extern "C" int edet_bn_bwd_finalize(const float* partials, int nparts, int c, double count, const float* gamma,
                                    const float* mean, const float* rstd, float* dgamma, float* dbeta, float* dbias,
                                    float* a, float* b, float* cc, void* stream) {
  EDET_CHECK(partials && gamma && mean && rstd && a && b && cc, "edet_bn_bwd_finalize: null pointer");
  (void)dbias;  // d(bias before BatchNorm) is analytically zero: BN removes the mean
  edet_launch(k_bn_bwd_finalize, dim3(cdiv(c, FIN_CH)), dim3(FIN_CH * FIN_SL), 0, to_stream(stream), partials, nparts, c, count,
              gamma, mean, rstd, dgamma, dbeta, a, b, cc);
  EDET_LAUNCH_CHECK("edet_bn_bwd_finalize");
  return 0;
}

extern "C" int edet_bn_res(const edet_tview_t* y, const void* residual, void* out, int ldo, int dtype, void* stream) {
  EDET_CHECK(y && y->data && out, "edet_bn_res: null pointer");
  EDET_CHECK(y->c % 8 == 0 && y->ld % 8 == 0 && ldo % 8 == 0, "edet_bn_res: c/ld % 8");
  const int64_t rows = (int64_t)y->n * y->h * y->w;
  const int grid = ew_grid(rows * (y->c / 8), dtype == EDET_BF16 ? reinterpret_cast<const void*>(&k_bn_res<bf16_t>) : nullptr);
  const bool known = dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    edet_launch(k_bn_res<T>, grid, dim3(THREADS), 0, to_stream(stream), *y, (const T*)residual, (T*)out, ldo, rows);
  });
  EDET_CHECK(known, "edet_bn_res: bad dtype %d", dtype);
  EDET_LAUNCH_CHECK("edet_bn_res");
  return 0;
}

extern "C" int edet_add(void* dst, const void* src, int64_t rows, int c, int ld, int beta, int dtype, void* stream) {
  EDET_CHECK(dst && src, "edet_add: null pointer");
  EDET_CHECK(c % 8 == 0 && ld % 8 == 0, "edet_add: c/ld % 8");
  const int grid = ew_grid(rows * (c / 8), dtype == EDET_BF16 ? reinterpret_cast<const void*>(&k_add<bf16_t>) : nullptr);
  const bool known = dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    edet_launch(k_add<T>, grid, dim3(THREADS), 0, to_stream(stream), (T*)dst, (const T*)src, rows, c, ld, beta);
  });
  EDET_CHECK(known, "edet_add: bad dtype %d", dtype);
  EDET_LAUNCH_CHECK("edet_add");
  return 0;
}
