// Squeeze-and-excitation: pooling, the two 1x1 layers (one workgroup per image, or sliced over the channel axis for wide
// blocks), their backward stages and the gate backward fused with the BatchNorm-backward sums.
//
// Reference: efficientdet/backbone/efficientnet_model.py:153-195 (SE).
#include "rowmap_impl.h"

namespace {

constexpr int THREADS = 256;
static_assert(THREADS == ROW_THREADS, "the row map is laid out for this workgroup size");

// ------------------------------------------------------------------ pooling
// Global average pooling WITHOUT atomics and with a summation order that does not depend on the batch: an image's
// rows are cut into chunks of `cr` rows (a function of the map and channel count only, se_chunk_rows), one workgroup
// per (image, chunk); thread (rr, cv) adds the rows rr, rr + rpp, ... of its chunk in row order, the rpp row-slices of
// a workgroup are added in slice order through LDS, and the chunk sums of an image are added in chunk order by the
// consumer (k_se_pool_finish or k_se_fc).  The same image therefore gives bit-identical pooled sums whatever batch it
// sits in and from run to run (the first version used fp32 atomics on both levels).
// parts[(n * nchunks + chunk) * c + i] = sum over the chunk's pixels of view(in)
template <typename T>
__global__ __launch_bounds__(THREADS) void k_se_pool(const edet_tview_t in, float* __restrict__ parts, int nchunks,
                                                    int cr, RowMap m) {
  const int tid = threadIdx.x;
  const int n = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
  const int cv = tid % m.tpr, rr = tid / m.tpr;
  const int hw = in.h * in.w;
  const int r0 = chunk * cr, r1 = min(hw, r0 + cr);
  extern __shared__ float red[];  // [rpp][cblk], cblk = min(c, tpr * 8)
  const int cblk = min(in.c, m.tpr * 8);
  edet_tview_t v = in;
  v.gate = nullptr;
  const T* base = reinterpret_cast<const T*>(in.data) + (size_t)n * hw * in.ld;
  float* out = parts + ((size_t)n * nchunks + chunk) * in.c;
  for (int cb = 0; cb < in.c; cb += m.tpr * 8) {     // channel blocks of <= 2048 channels
    const int c0 = cb + cv * 8;
    if (c0 < in.c) {
      float s[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = 0.f;
      ViewCoef vc;
      view_load_coef(in, c0, vc);
      // four rows of loads in flight per thread (16 waves/CU x 16 B per lane is ~4 MB in flight over the chip, a
      // third of what 2 us of HBM latency at 5 TB/s needs); the sums keep their row order
      const int st = m.rpp;
      int r = r0 + rr;
      for (; r + 3 * st < r1; r += 4 * st) {
        float x[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) load8<T>(base + (size_t)(r + u * st) * in.ld + c0, x[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          view_apply(v, vc, c0, n, x[u]);
#pragma unroll
          for (int e = 0; e < 8; ++e) s[e] += x[u][e];
        }
      }
      for (; r < r1; r += st) {
        float x[8];
        load8<T>(base + (size_t)r * in.ld + c0, x);
        view_apply(v, vc, c0, n, x);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += x[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) red[rr * cblk + cv * 8 + e] = s[e];
    }
    __syncthreads();
    for (int i = tid; i < cblk && cb + i < in.c; i += THREADS) {
      float t = red[i];
      for (int q = 1; q < m.rpp; ++q) t += red[q * cblk + i];      // row slices in slice order
      out[cb + i] = t;
    }
    __syncthreads();
  }
}

// An image's chunk sums p[0], p[stride], ..., p[(nchunks - 1) * stride] added in chunk order: the first, then k = 1 ..
__device__ __forceinline__ float chunk_sum(const float* p, int nchunks, int stride) {
  float t = p[0];
  for (int k = 1; k < nchunks; ++k) t += p[(size_t)k * stride];
  return t;
}
// The same walk over the channel slices' shares of a hidden unit (hpart [n][nslice][se]), in slice order
__device__ __forceinline__ float slice_sum(const float* p, int nslice, int se) { return chunk_sum(p, nslice, se); }

// pooled[n][i] = chunk sums of image n added in chunk order
__global__ __launch_bounds__(THREADS) void k_se_pool_finish(const float* __restrict__ parts, int nchunks, int c,
                                                           float* __restrict__ pooled, int total) {
  const int idx = blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  const int n = idx / c, i = idx - n * c;
  pooled[idx] = chunk_sum(parts + (size_t)n * nchunks * c + i, nchunks, c);
}

// one workgroup (SE_FC_THREADS lanes) per image.  pooled_parts != nullptr: the pooled sums are still k_se_pool's chunk
// rows [n][nchunks][c]; they are added here in chunk order and written to pooled (the backward pass reads them).
constexpr int SE_FC_THREADS = 1024;
__global__ __launch_bounds__(SE_FC_THREADS) void k_se_fc(float* __restrict__ pooled,
                                                        const float* __restrict__ pooled_parts, int nchunks, int c,
                                                        int se, float inv_hw, const float* w1, const float* b1,
                                                        const float* w2, const float* b2, float* hidden_pre,
                                                        float* gate, int act) {
  extern __shared__ float sm[];  // p[c], h[se], hp[nthr]
  float* p = sm;
  float* h = sm + c;
  float* hp = sm + c + se;
  const int n = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  for (int i = tid; i < c; i += nthr) {
    float t;
    if (pooled_parts) {
      t = chunk_sum(pooled_parts + (size_t)n * nchunks * c + i, nchunks, c);
      pooled[(size_t)n * c + i] = t;
    } else {
      t = pooled[(size_t)n * c + i];
    }
    p[i] = t * inv_hw;
  }
  __syncthreads();
  // thread (j, part): hidden unit j over the channels i = part, part + nparts, ... (w1 loads coalesced along
  // j; four independent partial sums keep four loads in flight); the parts of a unit are added in part order
  if (se <= nthr) {
    const int nparts = nthr / se, j = tid % se, part = tid / se;
    if (part < nparts) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int i = part;
      for (; i + 3 * nparts < c; i += 4 * nparts) {
        a0 = fmaf(p[i], w1[(size_t)i * se + j], a0);
        a1 = fmaf(p[i + nparts], w1[(size_t)(i + nparts) * se + j], a1);
        a2 = fmaf(p[i + 2 * nparts], w1[(size_t)(i + 2 * nparts) * se + j], a2);
        a3 = fmaf(p[i + 3 * nparts], w1[(size_t)(i + 3 * nparts) * se + j], a3);
      }
      for (; i < c; i += nparts) a0 = fmaf(p[i], w1[(size_t)i * se + j], a0);
      hp[part * se + j] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
    if (tid < se) {
      float t = hp[tid];
      for (int q = 1; q < nparts; ++q) t += hp[q * se + tid];
      h[tid] = t;
    }
  } else {
    for (int j = tid; j < se; j += nthr) {
      float acc = 0.f;
      for (int i = 0; i < c; ++i) acc = fmaf(p[i], w1[(size_t)i * se + j], acc);
      h[j] = acc;
    }
  }
  __syncthreads();
  for (int j = tid; j < se; j += nthr) {
    const float acc = h[j] + b1[j];
    hidden_pre[(size_t)n * se + j] = acc;
    h[j] = act_apply_(act, acc);
  }
  __syncthreads();
  for (int i = tid; i < c; i += nthr) {
    float a0 = b2[i], a1 = 0.f;
    int j = 0;
    for (; j + 1 < se; j += 2) {
      a0 = fmaf(h[j], w2[(size_t)j * c + i], a0);
      a1 = fmaf(h[j + 1], w2[(size_t)(j + 1) * c + i], a1);
    }
    if (j < se) a0 = fmaf(h[j], w2[(size_t)j * c + i], a0);
    gate[(size_t)n * c + i] = sigmoidf_(a0 + a1);
  }
}

// ---- the two 1x1 layers for WIDE squeeze-and-excitation blocks (c * se >= SE_SPLIT_MIN) ------------------------------
// k_se_fc streams both weight matrices through ONE compute unit per image: 3840 x 160 is 4.9 MB (144 us per call at
// efficientdet-d7x batch 8, 7.5 ms per step), and at batch 256 (efficientnetv2-s, 1536 x 64) every image's workgroup
// re-reads the same 0.8 MB from L2 (17 us per call, L2-bound).  Here the channel axis is cut into slices of SE_SLICE
// channels -- a function of c only, so the summation order of an image does not depend on the batch -- and a workgroup
// handles SE_IB images at once, so a weight element is loaded once per SE_IB images: (slice, image block) workgroups
// produce partial hidden sums (k_se_fc1_split), (slice, image block) workgroups add them in slice order, apply bias +
// activation and compute the gates of their slice (k_se_fc2_split).  Each image's sums are formed exactly as with
// SE_IB = 1 (its own accumulators, same order).
constexpr int SE_SLICE = 128;
constexpr int SE_IB = 4;
constexpr int SE_SPLIT_MIN = 1 << 15;       // forward (image-blocked: also pays at large batch)
constexpr int SE_SPLIT_MIN_BWD = 1 << 17;   // backward (per image: pays where one CU per image is the bottleneck)
__global__ __launch_bounds__(THREADS) void k_se_fc1_split(float* __restrict__ pooled,
                                                         const float* __restrict__ pooled_parts, int nchunks, int c,
                                                         int se, float inv_hw, const float* __restrict__ w1,
                                                         float* __restrict__ hpart, int nslice, int nimg) {
  __shared__ float p[SE_IB][SE_SLICE];
  __shared__ float hp[SE_IB][THREADS];
  const int sl = blockIdx.x, n0 = blockIdx.y * SE_IB, tid = threadIdx.x;
  const int c0 = sl * SE_SLICE, cn = min(SE_SLICE, c - c0);
  for (int q = tid; q < SE_IB * SE_SLICE; q += THREADS) {
    const int b = q / SE_SLICE, i = q - b * SE_SLICE, n = n0 + b;
    float t = 0.f;
    if (i < cn && n < nimg) {
      if (pooled_parts) {
        t = chunk_sum(pooled_parts + (size_t)n * nchunks * c + c0 + i, nchunks, c);
        pooled[(size_t)n * c + c0 + i] = t;
      } else {
        t = pooled[(size_t)n * c + c0 + i];
      }
    }
    p[b][i] = t * inv_hw;
  }
  __syncthreads();
  // thread (j, part): hidden unit j over the slice's channels part, part + nparts, ...; parts added in part order
  for (int j0 = 0; j0 < se; j0 += THREADS) {           // se <= THREADS in practice: one round
    const int seb = min(THREADS, se - j0);
    const int nparts = THREADS / seb, j = tid % seb, part = tid / seb;
    if (part < nparts) {
      float a0[SE_IB], a1[SE_IB];
#pragma unroll
      for (int b = 0; b < SE_IB; ++b) a0[b] = a1[b] = 0.f;
      int i = part;
      for (; i + nparts < cn; i += 2 * nparts) {
        const float u = w1[(size_t)(c0 + i) * se + j0 + j], v = w1[(size_t)(c0 + i + nparts) * se + j0 + j];
#pragma unroll
        for (int b = 0; b < SE_IB; ++b) { a0[b] = fmaf(p[b][i], u, a0[b]); a1[b] = fmaf(p[b][i + nparts], v, a1[b]); }
      }
      if (i < cn) {
        const float u = w1[(size_t)(c0 + i) * se + j0 + j];
#pragma unroll
        for (int b = 0; b < SE_IB; ++b) a0[b] = fmaf(p[b][i], u, a0[b]);
      }
#pragma unroll
      for (int b = 0; b < SE_IB; ++b) hp[b][part * seb + j] = a0[b] + a1[b];
    }
    __syncthreads();
    for (int q = tid; q < SE_IB * seb; q += THREADS) {
      const int b = q / seb, jj = q - b * seb;
      if (n0 + b < nimg) {
        float t = hp[b][jj];
        for (int r = 1; r < nparts; ++r) t += hp[b][r * seb + jj];
        hpart[((size_t)(n0 + b) * nslice + sl) * se + j0 + jj] = t;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(THREADS) void k_se_fc2_split(const float* __restrict__ hpart, int nslice, int c, int se,
                                                         const float* __restrict__ b1, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, float* __restrict__ hidden_pre,
                                                         float* __restrict__ gate, int act, int nimg) {
  extern __shared__ float h[];       // [SE_IB][se]
  const int sl = blockIdx.x, n0 = blockIdx.y * SE_IB, tid = threadIdx.x;
  for (int q = tid; q < SE_IB * se; q += THREADS) {
    const int b = q / se, j = q - b * se, n = n0 + b;
    float v = 0.f;
    if (n < nimg) {
      const float acc = slice_sum(hpart + (size_t)n * nslice * se + j, nslice, se) + b1[j];
      if (sl == 0) hidden_pre[(size_t)n * se + j] = acc;
      v = act_apply_(act, acc);
    }
    h[q] = v;
  }
  __syncthreads();
  const int c0 = sl * SE_SLICE;
  for (int i = c0 + tid; i < min(c, c0 + SE_SLICE); i += THREADS) {
    float a0[SE_IB], a1[SE_IB];
#pragma unroll
    for (int b = 0; b < SE_IB; ++b) { a0[b] = b2[i]; a1[b] = 0.f; }
    int j = 0;
    for (; j + 1 < se; j += 2) {
      const float u = w2[(size_t)j * c + i], v = w2[(size_t)(j + 1) * c + i];
#pragma unroll
      for (int b = 0; b < SE_IB; ++b) { a0[b] = fmaf(h[b * se + j], u, a0[b]); a1[b] = fmaf(h[b * se + j + 1], v, a1[b]); }
    }
    if (j < se) {
      const float u = w2[(size_t)j * c + i];
#pragma unroll
      for (int b = 0; b < SE_IB; ++b) a0[b] = fmaf(h[b * se + j], u, a0[b]);
    }
#pragma unroll
    for (int b = 0; b < SE_IB; ++b)
      if (n0 + b < nimg) gate[(size_t)(n0 + b) * c + i] = sigmoidf_(a0[b] + a1[b]);
  }
}

// ---- backward of the two 1x1 layers ------------------------------------------------------------------------------------
// The caller's scratch of edet_se_fc_bwd for n images, c channels and se hidden units, in floats:
//   [dpre2 n*c | dpre1 n*se | hact = act(hidden_pre) n*se | hpart n*ceil(c/SE_SLICE)*se | SE_SPLIT partials [dw1 | dw2 | db1 | db2]]
// The offsets are stated here only; total() is the size include/edet_hip.h documents (se_bwd_scratch_floats in automl_amd/_lib.py).
constexpr int SE_SPLIT = 8;              // image slices of the parameter gradients
struct SeBwdScratch {
  size_t n; int c, se;
  __host__ __device__ size_t dpre2() const { return 0; }
  __host__ __device__ size_t dpre1() const { return n * c; }
  __host__ __device__ size_t hact() const { return n * (c + se); }
  __host__ __device__ size_t hpart() const { return n * (c + 2 * se); }
  __host__ __device__ size_t parts() const { return n * (c + (2 + (c + SE_SLICE - 1) / SE_SLICE) * se); }
  __host__ __device__ size_t part_floats() const { return (size_t)2 * c * se + se + c; }      // one image slice's partial
  __host__ __device__ size_t total() const { return parts() + SE_SPLIT * part_floats(); }
};

// per image: dgate -> dpre2, dh, dpre1, dpool; dpre2, dpre1 and hact go to the scratch (SeBwdScratch)
__global__ __launch_bounds__(SE_FC_THREADS) void k_se_fc_bwd_img(const float* __restrict__ hidden_pre,
                                                          const float* __restrict__ gate,
                                                          const float* __restrict__ dgate, int nimg, int c,
                                                          int se, float inv_hw, const float* w1,
                                                          const float* w2, float* dpool, float* scratch, int act) {
  extern __shared__ float sm[];  // dpre2[c], dpre1[se]
  float* d2 = sm;
  float* d1 = sm + c;
  const int n = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const SeBwdScratch L{(size_t)nimg, c, se};
  float* dpre2_g = scratch + L.dpre2() + (size_t)n * c;
  float* dpre1_g = scratch + L.dpre1() + (size_t)n * se;
  float* hact_g = scratch + L.hact() + (size_t)n * se;
  for (int i = tid; i < c; i += nthr) {
    const float g = gate[(size_t)n * c + i];
    const float v = dgate[(size_t)n * c + i] * g * (1.f - g);
    d2[i] = v;
    dpre2_g[i] = v;
  }
  __syncthreads();
  // dh[j] = sum_i dpre2[i] * w2[j][i]: one wave per j (coalesced along i), shuffle reduction
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = wave; j < se; j += nthr / 64) {
    float acc = 0.f;
    for (int i = lane; i < c; i += 64) acc = fmaf(d2[i], w2[(size_t)j * c + i], acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) {
      const float hp = hidden_pre[(size_t)n * se + j];
      const float v = acc * act_grad_(act, hp);
      d1[j] = v;
      dpre1_g[j] = v;
      hact_g[j] = act_apply_(act, hp);
    }
  }
  __syncthreads();
  for (int i = tid; i < c; i += nthr) {
    float acc = 0.f;
    for (int j = 0; j < se; ++j) acc = fmaf(d1[j], w1[(size_t)i * se + j], acc);
    dpool[(size_t)n * c + i] = acc * inv_hw;
  }
}

// the same per-image work for WIDE blocks (c * se >= SE_SPLIT_MIN_BWD), sliced over the channel axis like k_se_fc1_split /
// k_se_fc2_split: (slice, image) workgroups make dpre2 and the slice's share of dh, then add the shares in slice order,
// finish dpre1 / the activated hidden units and compute dpool of their slice.  hpart: [n][nslice][se], SeBwdScratch's
// fourth region.
__global__ __launch_bounds__(THREADS) void k_se_fc_bwd_img1(const float* __restrict__ gate,
                                                           const float* __restrict__ dgate, int nimg, int c, int se,
                                                           const float* __restrict__ w2, float* __restrict__ scratch,
                                                           float* __restrict__ hpart, int nslice) {
  __shared__ float d2[SE_SLICE];
  const int sl = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int c0 = sl * SE_SLICE, cn = min(SE_SLICE, c - c0);
  float* dpre2_g = scratch + SeBwdScratch{(size_t)nimg, c, se}.dpre2() + (size_t)n * c;
  for (int i = tid; i < SE_SLICE; i += THREADS) {
    float v = 0.f;
    if (i < cn) {
      const float g = gate[(size_t)n * c + c0 + i];
      v = dgate[(size_t)n * c + c0 + i] * g * (1.f - g);
      dpre2_g[c0 + i] = v;
    }
    d2[i] = v;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  float* dst = hpart + ((size_t)n * nslice + sl) * se;
  for (int j = wave; j < se; j += THREADS / 64) {
    float acc = 0.f;
    for (int i = lane; i < cn; i += 64) acc = fmaf(d2[i], w2[(size_t)j * c + c0 + i], acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) dst[j] = acc;
  }
}

__global__ __launch_bounds__(THREADS) void k_se_fc_bwd_img2(const float* __restrict__ hidden_pre,
                                                           const float* __restrict__ hpart, int nslice, int nimg,
                                                           int c, int se, float inv_hw, const float* __restrict__ w1,
                                                           float* __restrict__ dpool, float* __restrict__ scratch,
                                                           int act) {
  extern __shared__ float d1[];      // [se]
  const int sl = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const SeBwdScratch L{(size_t)nimg, c, se};
  float* dpre1_g = scratch + L.dpre1() + (size_t)n * se;
  float* hact_g = scratch + L.hact() + (size_t)n * se;
  for (int j = tid; j < se; j += THREADS) {
    const float t = slice_sum(hpart + (size_t)n * nslice * se + j, nslice, se);
    const float hp = hidden_pre[(size_t)n * se + j];
    const float v = t * act_grad_(act, hp);
    d1[j] = v;
    if (sl == 0) {
      dpre1_g[j] = v;
      hact_g[j] = act_apply_(act, hp);
    }
  }
  __syncthreads();
  const int c0 = sl * SE_SLICE;
  for (int i = c0 + tid; i < min(c, c0 + SE_SLICE); i += THREADS) {
    float acc = 0.f;
    for (int j = 0; j < se; ++j) acc = fmaf(d1[j], w1[(size_t)i * se + j], acc);
    dpool[(size_t)n * c + i] = acc * inv_hw;
  }
}

// parameter gradients.  Workgroup = 64 channels i x 4 hidden-unit groups, for one slice of the images
// (blockIdx.y) and one block of SE_JB hidden units (blockIdx.z); thread (i, jg) owns the (i, j) pairs with
// j % 4 == jg and sums over its images (loads coalesced along i).  r04: every image slice writes its sums to its own
// partial [dw1 | dw2 | db1 | db2] in the scratch and k_se_fc_bwd_sum adds the SE_SPLIT partials in slice order -- the
// same gradients on every run (rounds 2-3 combined the slices with fp32 atomics; summing all images in one workgroup
// instead was measured at twice the time: 45 -> 89 us per call over the 16 blocks of D0).
//   dw1[i][j] += sum_n pooled[n][i]*inv_hw * dpre1[n][j];  dw2[j][i] += sum_n hact[n][j] * dpre2[n][i]
constexpr int SE_MAX_JPT = 12;           // hidden units per thread
constexpr int SE_JB = 4 * SE_MAX_JPT;    // hidden units per workgroup (48)
constexpr int SE_NB = 64;                // images per LDS chunk
__global__ __launch_bounds__(THREADS) void k_se_fc_bwd_par(const float* __restrict__ pooled,
                                                          const float* __restrict__ scratch, int nimg, int c,
                                                          int se, float inv_hw, float* __restrict__ parts,
                                                          int per_split) {
  extern __shared__ float sm[];  // dpre1 [NB][jb], hact [NB][jb] for the current chunk of images
  const SeBwdScratch L{(size_t)nimg, c, se};
  const float* dpre2 = scratch + L.dpre2();
  const float* dpre1_g = scratch + L.dpre1();
  const float* hact_g = scratch + L.hact();
  const int j0 = blockIdx.z * SE_JB, jb = min(SE_JB, se - j0);
  float* d1 = sm;
  float* ha = sm + (size_t)SE_NB * SE_JB;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 64 + (tid & 63), jg = tid >> 6;
  const int nbeg = blockIdx.y * per_split, nend = min(nimg, nbeg + per_split);
  const size_t cs = (size_t)c * se;
  float* pw1 = parts + (size_t)blockIdx.y * (2 * cs + se + c);      // this slice's partial: dw1 [c][se]
  float* pw2 = pw1 + cs;                                             // dw2 [se][c]
  float* pb1 = pw2 + cs;                                             // db1 [se]
  float* pb2 = pb1 + se;                                             // db2 [c]
  float a1[SE_MAX_JPT], a2[SE_MAX_JPT];
#pragma unroll
  for (int t = 0; t < SE_MAX_JPT; ++t) a1[t] = a2[t] = 0.f;
  float sb2 = 0.f, sb1 = 0.f;
  for (int n0 = nbeg; n0 < nend; n0 += SE_NB) {
    const int nb = min(SE_NB, nend - n0);
    __syncthreads();
    for (int q = tid; q < nb * jb; q += THREADS) {
      const int n = q / jb, j = q - n * jb;
      d1[q] = dpre1_g[(size_t)(n0 + n) * se + j0 + j];
      ha[q] = hact_g[(size_t)(n0 + n) * se + j0 + j];
    }
    __syncthreads();
    if (i < c) {
      for (int n = 0; n < nb; ++n) {
        const float pl = pooled[(size_t)(n0 + n) * c + i] * inv_hw;
        const float d2 = dpre2[(size_t)(n0 + n) * c + i];
        sb2 += d2;
#pragma unroll
        for (int t = 0; t < SE_MAX_JPT; ++t) {
          const int j = jg + 4 * t;
          if (j < jb) {
            a1[t] = fmaf(pl, d1[n * jb + j], a1[t]);
            a2[t] = fmaf(ha[n * jb + j], d2, a2[t]);
          }
        }
      }
    }
    if (blockIdx.x == 0 && tid < jb)
      for (int n = 0; n < nb; ++n) sb1 += d1[n * jb + tid];
  }
  if (blockIdx.x == 0 && tid < jb) pb1[j0 + tid] = sb1;
  if (i < c) {
    if (jg == 0 && blockIdx.z == 0) pb2[i] = sb2;
#pragma unroll
    for (int t = 0; t < SE_MAX_JPT; ++t) {
      const int j = jg + 4 * t;
      if (j < jb) {
        pw1[(size_t)i * se + j0 + j] = a1[t];
        pw2[(size_t)(j0 + j) * c + i] = a2[t];
      }
    }
  }
}

// (dw1, dw2, db1, db2) += the nsplit partials, in slice order
__global__ __launch_bounds__(THREADS) void k_se_fc_bwd_sum(const float* __restrict__ parts, int nsplit, int c, int se,
                                                          float* dw1, float* db1, float* dw2, float* db2) {
  const size_t cs = (size_t)c * se, total = 2 * cs + se + c;
  const size_t q = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (q >= total) return;
  float t = 0.f;
  for (int p = 0; p < nsplit; ++p) t += parts[(size_t)p * total + q];
  if (q < cs) dw1[q] += t;
  else if (q < 2 * cs) dw2[q - cs] += t;
  else if (q < 2 * cs + se) db1[q - 2 * cs] += t;
  else db2[q - 2 * cs - se] += t;
}

// g (in place, holds D) -> dz = (D*gate + dpool)*act'(z); BN backward stat partials.  OTHER: an activation beyond
// swish (its own instantiation: the extra selects cost the swish kernel three VGPRs and one occupancy step)
template <typename T, bool OTHER>
__global__ __launch_bounds__(THREADS) void k_se_gate_bwd(const edet_tview_t in, T* g, const float* dpool,
                                                        const float* mean, const float* rstd,
                                                        float* partials, int wg_per_img, RowMap m) {
  const int tid = threadIdx.x;
  const int n = blockIdx.x / wg_per_img, part = blockIdx.x % wg_per_img;
  const int cv = tid % m.tpr, rr = tid / m.tpr;
  const int hw = in.h * in.w;
  extern __shared__ float red[];  // [2][c] + scratch [2][THREADS * 8]
  float* scr = red + 2 * in.c;
  for (int cb = 0; cb < in.c; cb += m.tpr * 8) {     // channel blocks of <= 2048 channels
    const int c0 = cb + cv * 8;
    const bool ok = c0 < in.c;
    float s1[8], s2[8], sc[8], sh[8], mu[8], rs[8], gt[8], dp[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] = s2[e] = 0.f; sc[e] = 1.f; sh[e] = 0.f; mu[e] = 0.f; rs[e] = 1.f; gt[e] = 1.f; dp[e] = 0.f; }
    if (ok) {
      if (in.scale) { loadf8(in.scale + c0, sc); loadf8(in.shift + c0, sh); }
      loadf8(mean + c0, mu);
      loadf8(rstd + c0, rs);
      loadf8(in.gate + (size_t)n * in.c + c0, gt);
      loadf8(dpool + (size_t)n * in.c + c0, dp);
      const size_t base = (size_t)n * hw * in.ld;
      auto chain = [&](float (&d)[8], const float (&x)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float z = fmaf(x[e], sc[e], sh[e]);
          const float da = fmaf(d[e], gt[e], dp[e]);
          if (OTHER) d[e] = da * act_other_grad_(in.act, z);
          else d[e] = in.act == EDET_ACT_SWISH ? da * swish_gradf_(z) : da;
          s1[e] += d[e];
          s2[e] += d[e] * (x[e] - mu[e]) * rs[e];
        }
      };
      // two rows (four 16-byte loads) in flight per thread, see k_se_pool (three rows would cost the fourth wave per
      // SIMD that the 1024-workgroup grid needs to be resident at once); sums in row order
      const int st = wg_per_img * m.rpp;
      int r = part * m.rpp + rr;
      for (; r + st < hw; r += 2 * st) {
        float d[2][8], x[2][8];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const size_t off = base + (size_t)(r + u * st) * in.ld + c0;
          load8<T>(g + off, d[u]);
          load8<T>(reinterpret_cast<const T*>(in.data) + off, x[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          chain(d[u], x[u]);
          store8<T>(g + base + (size_t)(r + u * st) * in.ld + c0, d[u]);
        }
      }
      for (; r < hw; r += st) {
        const size_t off = base + (size_t)r * in.ld + c0;
        float d[8], x[8];
        load8<T>(g + off, d);
        load8<T>(reinterpret_cast<const T*>(in.data) + off, x);
        chain(d, x);
        store8<T>(g + off, d);
      }
    }
    rowlane_sums(scr, m, cv, rr, ok, s1, s2, red, cb, in.c);
  }
  __syncthreads();
  for (int i = tid; i < 2 * in.c; i += THREADS) partials[(size_t)blockIdx.x * 2 * in.c + i] = red[i];
}

}  // namespace

static int se_wg_per_img(int n, int hw, int rpp) {
  int passes = cdiv(hw, rpp);
  int w = 1024 / (n > 0 ? n : 1);
  if (w < 1) w = 1;
  if (w > passes) w = passes;
  if (w > 64) w = 64;
  return w;
}

// Rows of one image per k_se_pool workgroup: ~64 K elements (128 KB of bf16), at least four passes of the row map; a
// function of the map size and channel count ONLY, so an image is summed the same way in every batch.  If the chunk rows
// of the whole batch do not fit the caller's scratch the chunks grow (then the order depends on the scratch size; the
// engine's scratch -- EDET_MAX_PARTS * 2 * widest layer floats -- holds every EfficientDet / EfficientNetV2 layer up to
// batch x chunks = 2048 at the widest layer).
static int se_chunk_rows(int hw, int c, int rpp, int n, size_t scratch_floats, int* nchunks_out) {
  int cr = cdiv(cdiv(65536, c), rpp) * rpp;
  if (cr < 4 * rpp) cr = 4 * rpp;
  // at most 64 chunks per image: the consumer adds an image's chunk sums one after the other (r03c: the 768x768 and
  // 384x384 maps of efficientdet-d7x had 400-650 chunks and the FC kernel spent 100 us adding them)
  const int cap = cdiv(cdiv(hw, 64), rpp) * rpp;
  if (cr < cap) cr = cap;
  while ((size_t)n * cdiv(hw, cr) * c > scratch_floats && cr < hw) cr *= 2;
  *nchunks_out = cdiv(hw, cr);
  return cr;
}

static int se_pool_launch(const edet_tview_t* in, float* parts, size_t scratch_floats, int dtype, void* stream,
                          int* nchunks_out) {
  EDET_CHECK(in->c % 8 == 0 && in->ld % 8 == 0 && in->c <= 8192, "edet_se_pool: c/ld");
  const RowMap m = row_map(in->c);
  const int cr = se_chunk_rows(in->h * in->w, in->c, m.rpp, in->n, scratch_floats, nchunks_out);
  const int nchunks = *nchunks_out;
  EDET_CHECK((size_t)in->n * nchunks * in->c <= scratch_floats, "edet_se_pool: scratch of %zu floats < %d x %d", scratch_floats,
             in->n, in->c);
  const int cblk = in->c < m.tpr * 8 ? in->c : m.tpr * 8;
  const size_t lds = (size_t)m.rpp * cblk * sizeof(float);
  const bool known = dtype_dispatch(dtype, [&](auto t) {
    edet_launch(k_se_pool<typename decltype(t)::type>, dim3(in->n * nchunks), dim3(THREADS), lds, to_stream(stream), *in, parts, nchunks, cr, m);
  });
  EDET_CHECK(known, "edet_se_pool: bad dtype %d", dtype);
  return 0;
}

extern "C" int edet_se_pool(const edet_tview_t* in, float* pooled_sum, void* scratch, size_t scratch_bytes,
                            int dtype, void* stream) {
  EDET_CHECK(in && in->data && pooled_sum && scratch, "edet_se_pool: null pointer");
  int nchunks = 1;
  if (se_pool_launch(in, (float*)scratch, scratch_bytes / sizeof(float), dtype, stream, &nchunks)) return -1;
  const int total = in->n * in->c;
  edet_launch(k_se_pool_finish, dim3(cdiv(total, THREADS)), dim3(THREADS), 0, to_stream(stream), (const float*)scratch, nchunks, in->c, pooled_sum, total);
  EDET_LAUNCH_CHECK("edet_se_pool");
  return 0;
}

// k_se_fc for n images; pooled_parts: the chunk rows still to be added (with their count), or NULL: pooled holds the sums
static void launch_se_fc(float* pooled, const float* pooled_parts, int nchunks, int n, int c, int se, float inv_hw,
                         const float* w1, const float* b1, const float* w2, const float* b2, float* hidden_pre, float* gate,
                         int act, void* stream) {
  const int threads = c >= 512 ? SE_FC_THREADS : THREADS;
  edet_launch(k_se_fc, dim3(n), dim3(threads), (size_t)(c + se + threads) * sizeof(float), to_stream(stream), pooled, pooled_parts,
              nchunks, c, se, inv_hw, w1, b1, w2, b2, hidden_pre, gate, act);
}

extern "C" int edet_se_fc(const float* pooled_sum, int n, int c, int se, float inv_hw,
                          const float* w1, const float* b1, const float* w2, const float* b2,
                          float* hidden_pre, float* gate, int act, void* stream) {
  EDET_CHECK(pooled_sum && w1 && b1 && w2 && b2 && hidden_pre && gate, "edet_se_fc: null pointer");
  EDET_CHECK(act >= EDET_ACT_NONE && act <= EDET_ACT_LAST, "edet_se_fc: activation %d", act);
  launch_se_fc(const_cast<float*>(pooled_sum), nullptr, 0, n, c, se, inv_hw, w1, b1, w2, b2, hidden_pre, gate, act, stream);
  EDET_LAUNCH_CHECK("edet_se_fc");
  return 0;
}

extern "C" int edet_se_squeeze_excite(const edet_tview_t* in, void* scratch, size_t scratch_bytes, int se,
                                      float inv_hw, const float* w1, const float* b1, const float* w2, const float* b2,
                                      float* pooled_sum, float* hidden_pre, float* gate, int act, int dtype,
                                      void* stream) {
  EDET_CHECK(in && in->data && scratch && pooled_sum && w1 && b1 && w2 && b2 && hidden_pre && gate,
             "edet_se_squeeze_excite: null pointer");
  EDET_CHECK(act >= EDET_ACT_NONE && act <= EDET_ACT_LAST, "edet_se_squeeze_excite: activation %d", act);
  int nchunks = 1;
  if (se_pool_launch(in, (float*)scratch, scratch_bytes / sizeof(float), dtype, stream, &nchunks)) return -1;
  const int c = in->c;
  // wide blocks: the sliced pair of kernels, if the partial hidden sums fit behind the pooling's chunk sums
  const int nslice = cdiv(c, SE_SLICE);
  const size_t used = ((size_t)in->n * nchunks * c + 63) / 64 * 64;
  if ((int64_t)c * se >= SE_SPLIT_MIN && used + (size_t)in->n * nslice * se <= scratch_bytes / sizeof(float)) {
    float* hpart = (float*)scratch + used;
    const int nblk = cdiv(in->n, SE_IB);
    edet_launch(k_se_fc1_split, dim3(nslice, nblk), dim3(THREADS), 0, to_stream(stream), pooled_sum, (const float*)scratch, nchunks, c, se, inv_hw, w1, hpart, nslice, in->n);
    edet_launch(k_se_fc2_split, dim3(nslice, nblk), dim3(THREADS), (size_t)SE_IB * se * sizeof(float), to_stream(stream), (const float*)hpart, nslice, c, se, b1, w2, b2, hidden_pre, gate, act, in->n);
  } else launch_se_fc(pooled_sum, (const float*)scratch, nchunks, in->n, c, se, inv_hw, w1, b1, w2, b2, hidden_pre, gate, act, stream);
  EDET_LAUNCH_CHECK("edet_se_squeeze_excite");
  return 0;
}

extern "C" int edet_se_fc_bwd(const float* pooled_sum, const float* hidden_pre, const float* gate, const float* dgate,
                              int n, int c, int se, float inv_hw, const float* w1, const float* w2,
                              float* dw1, float* db1, float* dw2, float* db2,
                              float* dpool, float* scratch, int act, void* stream) {
  EDET_CHECK(act >= EDET_ACT_NONE && act <= EDET_ACT_LAST, "edet_se_fc_bwd: activation %d", act);
  EDET_CHECK(pooled_sum && hidden_pre && gate && dgate && w1 && w2 && dw1 && db1 && dw2 && db2 && dpool && scratch,
             "edet_se_fc_bwd: null pointer");
  const SeBwdScratch L{(size_t)n, c, se};
  if ((int64_t)c * se >= SE_SPLIT_MIN_BWD) {      // wide blocks: sliced over the channel axis
    const int nslice = cdiv(c, SE_SLICE);
    float* hpart = scratch + L.hpart();
    edet_launch(k_se_fc_bwd_img1, dim3(nslice, n), dim3(THREADS), 0, to_stream(stream), gate, dgate, n, c, se, w2, scratch, hpart, nslice);
    edet_launch(k_se_fc_bwd_img2, dim3(nslice, n), dim3(THREADS), (size_t)se * sizeof(float), to_stream(stream), hidden_pre, (const float*)hpart, nslice, n, c, se, inv_hw, w1, dpool, scratch, act);
  } else {
    edet_launch(k_se_fc_bwd_img, dim3(n), dim3(c >= 512 ? SE_FC_THREADS : THREADS), (size_t)(c + se) * sizeof(float), to_stream(stream), hidden_pre, gate, dgate, n, c, se, inv_hw, w1, w2, dpool, scratch, act);
  }
  const int nsplit = n >= 2 * SE_SPLIT ? SE_SPLIT : 1;
  const int per_split = cdiv(n, nsplit);
  const int nsl = cdiv(n, per_split);
  float* parts = scratch + L.parts();
  edet_launch(k_se_fc_bwd_par, dim3(cdiv(c, 64), nsl, cdiv(se, SE_JB)), dim3(THREADS), (size_t)2 * SE_NB * SE_JB * sizeof(float),
              to_stream(stream), pooled_sum, (const float*)scratch, n, c, se, inv_hw, parts, per_split);
  edet_launch(k_se_fc_bwd_sum, dim3(cdiv(L.part_floats(), THREADS)), dim3(THREADS), 0, to_stream(stream), (const float*)parts, nsl, c, se,
              dw1, db1, dw2, db2);
  EDET_LAUNCH_CHECK("edet_se_fc_bwd");
  return 0;
}

extern "C" int edet_se_gate_bwd(const edet_tview_t* in, void* g, const float* dpool, const float* mean, const float* rstd,
                                float* stat_partials, int* nparts_out, int dtype, void* stream) {
  EDET_CHECK(in && in->data && in->gate && g && dpool && mean && rstd && stat_partials, "edet_se_gate_bwd: null pointer");
  EDET_CHECK(in->c % 8 == 0 && in->ld % 8 == 0 && in->c <= 6144, "edet_se_gate_bwd: c/ld (c <= 6144)");
  const RowMap m = row_map(in->c);
  int wpi = se_wg_per_img(in->n, in->h * in->w, m.rpp);
  while (in->n * wpi > EDET_MAX_PARTS && wpi > 1) --wpi;
  EDET_CHECK(in->n * wpi <= EDET_MAX_PARTS, "edet_se_gate_bwd: batch %d exceeds %d partial rows", in->n, EDET_MAX_PARTS);
  if (nparts_out) *nparts_out = in->n * wpi;
  const size_t lds = (size_t)(2 * in->c + 2 * THREADS * 8) * sizeof(float);
  const bool known = dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    auto launch = [&](auto kern) { edet_launch(kern, dim3(in->n * wpi), dim3(THREADS), lds, to_stream(stream), *in, (T*)g, dpool, mean, rstd, stat_partials, wpi, m); };
    if (in->act > EDET_ACT_SWISH) launch(k_se_gate_bwd<T, true>);      // OTHER
    else launch(k_se_gate_bwd<T, false>);
  });
  EDET_CHECK(known, "edet_se_gate_bwd: bad dtype %d", dtype);
  EDET_LAUNCH_CHECK("edet_se_gate_bwd");
  return 0;
}
