// Detection loss (focal + Huber) forward and backward in one pass, and the fused optimizer
// (L2 regularisation, per-tensor + global gradient clipping, SGD momentum, EMA) over a flat
// fp32 parameter arena.
//
// Reference: efficientdet/tf2/train_lib.py:357-406 (FocalLoss), :409-437 (BoxLoss / Keras Huber),
// :493-604 (_detection_loss), :486-491 (_reg_l2_loss), :675-683 (clip + apply), :176-199 (optimizer).
#include "rowmap_impl.h"

#include <cfloat>
#include <type_traits>

namespace {

constexpr int THREADS = 256;
static_assert(THREADS == ROW_THREADS, "the row map is laid out for this workgroup size");

// logits [positions][ld], channel j = anchor * num_classes + class.
// Per element (train_lib.py:357-406 with label_smoothing 0): u = +-x, 1 - p_t = sigmoid(u),
// ce = softplus(u); loss = alpha_t * sigmoid(u)^gamma * softplus(u) / normalizer.  One exp, one rcp,
// one log and one sqrt (gamma = 1.5) or one pow (general gamma; pow(0, 0) = 1) per logit; the anchor index is
// advanced incrementally along the 8-wide chunk, so there is one integer division per 16 bytes.
// LS: label smoothing (tf2/train_lib.py:400-402): the cross entropy is taken against y*(1-ls) + ls/2 while alpha and the
// modulating factor keep the hard label.  With u = -x for the positive class and x otherwise, ce_smoothed = softplus(u) -
// (ls/2) u in both cases, so d/du [sg^gamma (sp - h u)] = sg^gamma (gamma (1-sg) (sp - h u) + sg - h), h = ls/2.  A
// template parameter of the shared body: k_focal (ls = 0) keeps its instruction count (the kernel is VALU-bound) and
// its symbol; k_focal_ls is the smoothed one.
// Tail of the two loss kernels: the workgroup's loss sum and its per-channel bias-gradient sums.  r04: combined in a fixed
// order (wave shuffles, waves in order, row-lanes in order through LDS -- no LDS atomics); with a partial buffer the
// workgroup writes its row [nch | 1] there and edet_reduce_partials2 adds the rows in order (the same loss and bias gradient on
// every run); without one the kernel is launched as ONE workgroup, which adds into the destinations itself -- no atomics.
// LDS: scr[THREADS * 8] floats (dynamic).
// GRAD = false (the loss-only kernels of the evaluation step, edet_focal_loss_eval / edet_box_loss_eval): the same loss sum in
// the same order, no bias-gradient rows -- a partial row is the workgroup's loss alone.
template <bool GRAD = true>
__device__ __forceinline__ void loss_tail(float loss_acc, const float (&db)[8], bool ok, int nch, const RowMap& m, float* scr,
                                          float* part, float* sum_dst, float* dbias) {
  __shared__ float wsum[THREADS / 64];
  const int tid = threadIdx.x;
  const int cv = tid % m.tpr, rr = tid / m.tpr;
  const int width = m.tpr * 8;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) loss_acc += __shfl_down(loss_acc, off, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = loss_acc;
  if (GRAD) {
#pragma unroll
    for (int e = 0; e < 8; ++e) scr[rr * width + cv * 8 + e] = ok ? db[e] : 0.f;
  }
  __syncthreads();
  float* row = part ? part + (size_t)blockIdx.x * (GRAD ? 1 + nch : 1) : nullptr;      // [bias gradient (nch) | loss]
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < THREADS / 64; ++w) t += wsum[w];
    if (row) row[GRAD ? nch : 0] = t; else *sum_dst += t;          // (no partial buffer: the kernel runs as ONE workgroup)
  }
  if (GRAD && (dbias || row)) {
    for (int i = tid; i < nch; i += THREADS) {
      float t = 0.f;
      for (int r = 0; r < m.rpp; ++r) t += scr[r * width + i];
      if (row) row[i] = t; else dbias[i] += t;
    }
  }
}

template <typename T, bool G15, bool LS, bool GRAD = true>
__device__ __forceinline__ void focal_body(const T* __restrict__ logits, int ld,
                                                  const int32_t* __restrict__ tgt, int64_t positions,
                                                  int na, int nc, float alpha, float gamma, float inv_norm_h,
                                                  const float* __restrict__ norm_scale,
                                                  T* __restrict__ dlogits, float* dbias, float* sums, float* part, RowMap m,
                                                  float half_ls) {
  const float inv_norm = norm_scale ? inv_norm_h * norm_scale[0] : inv_norm_h;
  const int tid = threadIdx.x;
  const int cv = tid % m.tpr, rr = tid / m.tpr;
  const int j0 = cv * 8;
  const int nch = na * nc;
  const bool ok = j0 < ld;
  const int a0 = j0 / nc, k0 = j0 - a0 * nc;
  float loss_acc = 0.f, db[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) db[e] = 0.f;
  if (ok && nc < 8) {
    // fewer than 8 classes: an 8-element chunk can span more than two anchors -- the simple form, one row at a time,
    // the anchor's target fetched when the class index wraps
    for (int64_t p = (int64_t)blockIdx.x * m.rpp + rr; p < positions; p += (int64_t)gridDim.x * m.rpp) {
      float x[8], g[8];
      load8<T>(logits + p * ld + j0, x);
      int a = a0, k = k0;
      int t = a < na ? tgt[p * na + a] : -2;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        g[e] = 0.f;
        if (j0 + e < nch && t != -2) {
          const bool pos = (t == k);
          const float u = pos ? -x[e] : x[e];
          const float ex = __builtin_amdgcn_exp2f(-1.44269504f * fabsf(u));
          const float inv = __builtin_amdgcn_rcpf(1.f + ex);
          const float sg = u >= 0.f ? inv : ex * inv;
          float sp = fmaxf(u, 0.f) + 0.69314718f * __builtin_amdgcn_logf(1.f + ex);
          if (LS) sp = fmaf(-half_ls, u, sp);
          const float af = pos ? alpha : 1.f - alpha;
          const float mod = G15 ? sg * __builtin_amdgcn_sqrtf(sg) : __powf(sg, gamma);
          loss_acc = fmaf(af * mod, sp * inv_norm, loss_acc);
          if (GRAD) {
            const float dldu = af * mod * fmaf(gamma * (1.f - sg), sp, LS ? sg - half_ls : sg) * inv_norm;
            g[e] = pos ? -dldu : dldu;
          }
        }
        if (GRAD) db[e] += g[e];
        if (++k == nc) {
          k = 0;
          ++a;
          t = a < na ? tgt[p * na + a] : -2;
        }
      }
      if (GRAD) store8<T>(dlogits + p * ld + j0, g);
    }
  } else if (ok) {
    // One row per step, the next row's logits and targets requested before this row is worked on (r03: the first
    // version loaded, computed and stored one row at a time and fetched the second anchor's target in the middle of the
    // element loop -- a dependent global load under a branch; 85 % "VALU busy" was mostly that wait).  An 8-element
    // chunk spans at most two anchors (num_classes >= 8): both targets are loaded up front, the element loop is
    // branch-free.
    const int64_t step = (int64_t)gridDim.x * m.rpp;
    int64_t p = (int64_t)blockIdx.x * m.rpp + rr;
    const bool has_a1 = a0 + 1 < na;
    float x[8], xn[8];
    int t0 = -2, t1 = -2, t0n = -2, t1n = -2;
    if (p < positions) {
      load8<T>(logits + p * ld + j0, x);
      t0 = a0 < na ? tgt[p * na + a0] : -2;
      t1 = has_a1 ? tgt[p * na + a0 + 1] : -2;
    }
    while (p < positions) {
      const int64_t pn = p + step;
      if (pn < positions) {
        load8<T>(logits + pn * ld + j0, xn);
        t0n = a0 < na ? tgt[pn * na + a0] : -2;
        t1n = has_a1 ? tgt[pn * na + a0 + 1] : -2;
      }
      float g[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int idx = k0 + e;
        const bool cross = idx >= nc;
        const int k = cross ? idx - nc : idx;
        const int t = cross ? t1 : t0;
        const bool pos = (t == k);
        const bool valid = (j0 + e < nch) && t != -2;
        const float xe = valid ? x[e] : 0.f;                 // padding columns / ignored anchors may hold anything
        const float u = pos ? -xe : xe;
        // hardware transcendentals (1 ulp: v_exp_f32, v_rcp_f32, v_log_f32, v_sqrt_f32); the IEEE-rounded
        // library forms (__frcp_rn, __fsqrt_rn, __logf) expanded to ~35 extra VALU instructions per logit and
        // made this kernel 100 % VALU-bound.  1 + ex is in [1, 2]: no denormal handling is needed.
        const float ex = __builtin_amdgcn_exp2f(-1.44269504f * fabsf(u));
        const float inv = __builtin_amdgcn_rcpf(1.f + ex);
        const float sg = u >= 0.f ? inv : ex * inv;          // sigmoid(u) = 1 - p_t
        float sp = fmaxf(u, 0.f) + 0.69314718f * __builtin_amdgcn_logf(1.f + ex);   // softplus(u) = cross entropy
        if (LS) sp = fmaf(-half_ls, u, sp);                    // ... against the smoothed label
        const float af = pos ? alpha : 1.f - alpha;
        const float mod = G15 ? sg * __builtin_amdgcn_sqrtf(sg) : __powf(sg, gamma);
        const float wgt = valid ? af * mod * inv_norm : 0.f;
        loss_acc = fmaf(wgt, sp, loss_acc);
        if (GRAD) {
          // d/du [sg^gamma * softplus(u)] = sg^gamma * (gamma*(1-sg)*sp + sg)
          const float dldu = wgt * fmaf(gamma * (1.f - sg), sp, LS ? sg - half_ls : sg);
          g[e] = pos ? -dldu : dldu;
          db[e] += g[e];
        }
      }
      if (GRAD) store8<T>(dlogits + p * ld + j0, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = xn[e];
      t0 = t0n; t1 = t1n;
      p = pn;
    }
  }
  extern __shared__ float red[];  // [THREADS * 8]
  loss_tail<GRAD>(loss_acc, db, ok, nch, m, red, part, &sums[0], dbias);
}

template <typename T, bool G15>
__global__ __launch_bounds__(THREADS) void k_focal(const T* __restrict__ logits, int ld,
                                                  const int32_t* __restrict__ tgt, int64_t positions,
                                                  int na, int nc, float alpha, float gamma, float inv_norm_h,
                                                  const float* __restrict__ norm_scale,
                                                  T* __restrict__ dlogits, float* dbias, float* sums, float* part, RowMap m) {
  focal_body<T, G15, false>(logits, ld, tgt, positions, na, nc, alpha, gamma, inv_norm_h, norm_scale, dlogits, dbias, sums, part, m, 0.f);
}
template <typename T, bool G15>
__global__ __launch_bounds__(THREADS) void k_focal_ls(const T* __restrict__ logits, int ld,
                                                     const int32_t* __restrict__ tgt, int64_t positions,
                                                     int na, int nc, float alpha, float gamma, float inv_norm_h,
                                                     const float* __restrict__ norm_scale,
                                                     T* __restrict__ dlogits, float* dbias, float* sums, float* part, RowMap m,
                                                     float half_ls) {
  focal_body<T, G15, true>(logits, ld, tgt, positions, na, nc, alpha, gamma, inv_norm_h, norm_scale, dlogits, dbias, sums, part, m, half_ls);
}

// the loss alone (GRAD = false): the arithmetic and the summation order of k_focal / k_focal_ls, no gradient stores
template <typename T, bool G15, bool LS>
__global__ __launch_bounds__(THREADS) void k_focal_eval(const T* __restrict__ logits, int ld,
                                                       const int32_t* __restrict__ tgt, int64_t positions,
                                                       int na, int nc, float alpha, float gamma, float inv_norm_h,
                                                       const float* __restrict__ norm_scale, float* sums, float* part, RowMap m,
                                                       float half_ls) {
  focal_body<T, G15, LS, false>(logits, ld, tgt, positions, na, nc, alpha, gamma, inv_norm_h, norm_scale, nullptr, nullptr, sums, part, m, half_ls);
}

template <typename T, bool GRAD>
__device__ __forceinline__ void box_body(const T* out, int ld, const float* tgt, int64_t positions, int nch,
                                         float delta, float inv_norm_h, float grad_scale, const float* norm_scale,
                                         T* dbox, float* dbias, float* sums, float* part, RowMap m) {
  const float inv_norm = norm_scale ? inv_norm_h * norm_scale[0] : inv_norm_h;
  const int tid = threadIdx.x;
  const int cv = tid % m.tpr, rr = tid / m.tpr;
  const int j0 = cv * 8;
  const bool ok = j0 < ld;
  float loss_acc = 0.f, db[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) db[e] = 0.f;
  if (ok) {
    for (int64_t p = (int64_t)blockIdx.x * m.rpp + rr; p < positions; p += (int64_t)gridDim.x * m.rpp) {
      float x[8], g[8];
      load8<T>(out + p * ld + j0, x);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = j0 + e;
        g[e] = 0.f;
        if (j < nch) {
          const float t = tgt[p * nch + j];
          if (t != 0.f) {
            const float err = x[e] - t;
            const float ae = fabsf(err);
            const bool quad = ae <= delta;
            loss_acc += (quad ? 0.5f * err * err : delta * ae - 0.5f * delta * delta) * inv_norm;
            if (GRAD) g[e] = (quad ? err : (err > 0.f ? delta : -delta)) * inv_norm * grad_scale;
          }
        }
        if (GRAD) db[e] += g[e];
      }
      if (GRAD) store8<T>(dbox + p * ld + j0, g);
    }
  }
  extern __shared__ float red[];  // [THREADS * 8]
  loss_tail<GRAD>(loss_acc, db, ok, nch, m, red, part, &sums[1], dbias);
}

template <typename T>
__global__ __launch_bounds__(THREADS) void k_box(const T* __restrict__ out, int ld,
                                                const float* __restrict__ tgt, int64_t positions, int nch,
                                                float delta, float inv_norm_h, float grad_scale,
                                                const float* __restrict__ norm_scale,
                                                T* __restrict__ dbox, float* dbias, float* sums, float* part, RowMap m) {
  box_body<T, true>(out, ld, tgt, positions, nch, delta, inv_norm_h, grad_scale, norm_scale, dbox, dbias, sums, part, m);
}
template <typename T>
__global__ __launch_bounds__(THREADS) void k_box_eval(const T* __restrict__ out, int ld,
                                                     const float* __restrict__ tgt, int64_t positions, int nch,
                                                     float delta, float inv_norm_h,
                                                     const float* __restrict__ norm_scale, float* sums, float* part, RowMap m) {
  box_body<T, false>(out, ld, tgt, positions, nch, delta, inv_norm_h, 0.f, norm_scale, nullptr, nullptr, sums, part, m);
}

// ----------------------------------------------------------------------------------- optimizer
__device__ __forceinline__ float block_sum(float v, float* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < THREADS / 64; ++i) t += sh[i];
  return t;
}

// Every tensor segment is cut into up to OPT_SPLIT slices of >= 1024 elements, one workgroup per
// (segment, slice): the few large kernels (>100 k elements) no longer serialise on one workgroup, the
// many small tensors still cost one workgroup each, and every reduction keeps a fixed order.
constexpr int OPT_SPLIT = EDET_OPT_SPLIT;

__device__ __forceinline__ bool slice_range(const int64_t* seg_off, int s, int j, int64_t& b, int64_t& e) {
  const int64_t sb = seg_off[s], se = seg_off[s + 1];
  int64_t chunk = ((se - sb + OPT_SPLIT - 1) / OPT_SPLIT + 3) / 4 * 4;
  if (chunk < 1024) chunk = 1024;
  b = sb + (int64_t)j * chunk;
  e = b + chunk < se ? b + chunk : se;
  return b < e;
}

// GRAD = false (k_l2_loss_slices, the evaluation step): the wsq sums alone, in the same order -- the gradient arena is neither
// read nor written, seg_sqnorm is [nseg][OPT_SPLIT] L2 shares
template <bool GRAD>
__device__ __forceinline__ void l2_norms_body(float* grads, const float* params,
                                                     const int64_t* seg_off, const int32_t* seg_flags,
                                                     float wd, float* seg_sqnorm, int nseg) {
  __shared__ float sh[THREADS / 64];
  const int s = blockIdx.x, j = blockIdx.y;
  int64_t b, e;
  const bool any = slice_range(seg_off, s, j, b, e);
  const bool frozen = (seg_flags[s] & EDET_SEG_FROZEN) != 0;
  const bool reg = (seg_flags[s] & EDET_SEG_L2) != 0 && !frozen;
  float gsq = 0.f, wsq = 0.f;
  if (any && frozen) {
    // a frozen variable (config.var_freeze_expr) has no gradient: zeroed here, no share in the norms, skipped by the update
    if (GRAD) {
      for (int64_t i = b + threadIdx.x; i < e; i += THREADS) grads[i] = 0.f;
    }
  } else if (any) {
    if ((b & 3) == 0) {
      const int64_t nv = (e - b) >> 2;
      float4* g4 = GRAD ? reinterpret_cast<float4*>(grads + b) : nullptr;
      const float4* w4 = reinterpret_cast<const float4*>(params + b);
      for (int64_t i = threadIdx.x; i < nv; i += THREADS) {
        float4 g = GRAD ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (reg) {
          const float4 w = w4[i];
          if (GRAD) {
            g.x = fmaf(wd, w.x, g.x); g.y = fmaf(wd, w.y, g.y); g.z = fmaf(wd, w.z, g.z); g.w = fmaf(wd, w.w, g.w);
            g4[i] = g;
          }
          wsq += w.x * w.x + w.y * w.y + w.z * w.z + w.w * w.w;
        }
        if (GRAD) gsq += g.x * g.x + g.y * g.y + g.z * g.z + g.w * g.w;
      }
      b += nv << 2;
    }
    for (int64_t i = b + threadIdx.x; i < e; i += THREADS) {
      float g = GRAD ? grads[i] : 0.f;
      if (reg) {
        const float w = params[i];
        if (GRAD) {
          g = fmaf(wd, w, g);
          grads[i] = g;
        }
        wsq = fmaf(w, w, wsq);
      }
      if (GRAD) gsq = fmaf(g, g, gsq);
    }
  }
  const float tg = GRAD ? block_sum(gsq, sh) : 0.f;
  const float tw = block_sum(wsq, sh);
  if (threadIdx.x == 0) {
    if (GRAD) seg_sqnorm[(size_t)s * OPT_SPLIT + j] = tg;
    // this slice's share of the L2 loss, summed in a fixed order by k_clip_factors (r04: no atomics)
    seg_sqnorm[((size_t)(GRAD ? nseg : 0) + s) * OPT_SPLIT + j] = (any && reg) ? 0.5f * wd * tw : 0.f;
  }
}

__global__ __launch_bounds__(THREADS) void k_l2_norms(float* grads, const float* params,
                                                     const int64_t* seg_off, const int32_t* seg_flags,
                                                     float wd, float* seg_sqnorm, int nseg) {
  l2_norms_body<true>(grads, params, seg_off, seg_flags, wd, seg_sqnorm, nseg);
}
__global__ __launch_bounds__(THREADS) void k_l2_loss_slices(const float* params, const int64_t* seg_off,
                                                           const int32_t* seg_flags, float wd, float* seg_l2, int nseg) {
  l2_norms_body<false>(nullptr, params, seg_off, seg_flags, wd, seg_l2, nseg);
}
// the L2 half of k_clip_factors: the slices' shares added in its order (segments strided over the lanes, a segment's slices
// in order, block_sum), WRITTEN to l2_out[0]
__global__ __launch_bounds__(THREADS) void k_l2_loss_sum(const float* seg_l2, int nseg, float* l2_out) {
  __shared__ float sh[THREADS / 64];
  float l2 = 0.f;
  for (int s = threadIdx.x; s < nseg; s += THREADS) {
#pragma unroll
    for (int j = 0; j < OPT_SPLIT; ++j) l2 += seg_l2[(size_t)s * OPT_SPLIT + j];
  }
  const float l2tot = block_sum(l2, sh);
  if (threadIdx.x == 0) l2_out[0] = l2tot;
}

// tf.clip_by_norm per tensor, then tf.clip_by_global_norm over the clipped tensors
__global__ __launch_bounds__(THREADS) void k_clip_factors(const float* seg_sqnorm, int nseg, float clip,
                                                         float* seg_factor, float* gnorm_out, float* l2_sum) {
  __shared__ float sh[THREADS / 64];
  float acc = 0.f, l2 = 0.f;
  for (int s = threadIdx.x; s < nseg; s += THREADS) {
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < OPT_SPLIT; ++j) {
      sq += seg_sqnorm[(size_t)s * OPT_SPLIT + j];
      l2 += seg_sqnorm[((size_t)nseg + s) * OPT_SPLIT + j];
    }
    const float nrm = sqrtf(sq);
    float f = 1.f;
    if (clip > 0.f) f = clip / fmaxf(nrm, clip);
    seg_factor[s] = f;
    const float cn = nrm * f;
    acc = fmaf(cn, cn, acc);
  }
  const float tot = block_sum(acc, sh);
  const float l2tot = block_sum(l2, sh);
  if (threadIdx.x == 0 && l2_sum) l2_sum[0] += l2tot;
  const float gn = sqrtf(tot);
  float f2 = 1.f;
  if (clip > 0.f) f2 = clip / fmaxf(gn, clip);
  __syncthreads();
  for (int s = threadIdx.x; s < nseg; s += THREADS) seg_factor[s] *= f2;
  if (threadIdx.x == 0 && gnorm_out) gnorm_out[0] = gn * f2;
}

__global__ __launch_bounds__(THREADS) void k_scale(float* grads, const int64_t* seg_off,
                                                  const float* seg_factor) {
  const int s = blockIdx.x;
  int64_t b, e;
  if (!slice_range(seg_off, s, blockIdx.y, b, e)) return;
  const float f = seg_factor[s];
  if ((b & 3) == 0) {
    const int64_t nv = (e - b) >> 2;
    float4* g4 = reinterpret_cast<float4*>(grads + b);
    for (int64_t i = threadIdx.x; i < nv; i += THREADS) {
      float4 g = g4[i];
      g.x *= f; g.y *= f; g.z *= f; g.w *= f;
      g4[i] = g;
    }
    b += nv << 2;
  }
  for (int64_t i = b + threadIdx.x; i < e; i += THREADS) grads[i] *= f;
}

// ---- the parameter update: one walk over a segment's slice (update_walk), whatever the optimizer.  A rule holds its scalars, says how
// many slot arrays it keeps (SLOTS) and updates one element; the TFA MovingAverage shadow (ema -= (1-decay)*(ema - w)) rides
// on every rule.  hyper[0] = the step's learning rate (Adam: bias-corrected by the host), hyper[1] = the EMA decay.
// Keras SGD: v = m*v - lr*g ; w += v
struct SgdRule {
  static constexpr int SLOTS = 1;
  float momentum;
  __device__ __forceinline__ void operator()(float g, float& v, float&, float& w, float& em, float lr, float decay,
                                             bool has_ema) const {
    v = momentum * v - lr * g;
    w += v;
    if (has_ema) em -= (1.f - decay) * (em - w);
  }
};

// tf.keras.optimizers.Adam (ResourceApplyAdam): m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); w -= alpha m / (sqrt(v) + eps)
// with alpha = lr sqrt(1 - b2^t) / (1 - b1^t) formed by the host for this step (hyper[0])
struct AdamRule {
  static constexpr int SLOTS = 2;
  float b1, b2, eps;
  __device__ __forceinline__ void operator()(float g, float& m, float& u, float& w, float& em, float alpha, float decay,
                                             bool has_ema) const {
    m += (g - m) * (1.f - b1);
    u += (g * g - u) * (1.f - b2);
    w -= (m * alpha) / (sqrtf(u) + eps);
    if (has_ema) em -= (1.f - decay) * (em - w);
  }
};

// TensorFlow's ApplyRMSProp with momentum (what tf.keras.optimizers.RMSprop runs): ms += (1 - rho)(g^2 - ms);
// mom = momentum mom + lr g / sqrt(ms + eps); w -= mom
struct RmspropRule {
  static constexpr int SLOTS = 2;
  float rho, momentum, eps;
  __device__ __forceinline__ void operator()(float g, float& ms, float& mom, float& w, float& em, float lr, float decay,
                                             bool has_ema) const {
    ms += (g * g - ms) * (1.f - rho);
    mom = momentum * mom + (lr * g) / sqrtf(ms + eps);
    w -= mom;
    if (has_ema) em -= (1.f - decay) * (em - w);
  }
};

template <typename Rule>
__device__ __forceinline__ void update_walk(Rule rule, float* params, const float* grads, float* slot_a, float* slot_b,
                                            float* ema, const int64_t* seg_off, const float* seg_factor,
                                            const int32_t* seg_flags, const float* hyper) {
  constexpr bool two = Rule::SLOTS == 2;      // slot_b is read and written by the two-slot rules only
  const int s = blockIdx.x;
  int64_t b, e;
  if (!slice_range(seg_off, s, blockIdx.y, b, e)) return;
  // frozen variables are not in the optimizer's variable list (tf2/train_lib.py:478-491,683): value, slots and EMA shadow
  // stay exactly as they are
  if (seg_flags && (seg_flags[s] & EDET_SEG_FROZEN)) return;
  const float f = seg_factor ? seg_factor[s] : 1.f;
  const float lr = hyper[0], decay = hyper[1];
  const bool has_ema = ema != nullptr;
  if ((b & 3) == 0) {
    const int64_t nv = (e - b) >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(grads + b);
    float4* p4 = reinterpret_cast<float4*>(slot_a + b);
    float4* q4 = reinterpret_cast<float4*>(two ? slot_b + b : nullptr);
    float4* w4 = reinterpret_cast<float4*>(params + b);
    float4* e4 = has_ema ? reinterpret_cast<float4*>(ema + b) : nullptr;
    for (int64_t i = threadIdx.x; i < nv; i += THREADS) {
      const float4 g = g4[i];
      float4 p = p4[i], q = make_float4(0.f, 0.f, 0.f, 0.f), w = w4[i], em = has_ema ? e4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (two) q = q4[i];
      rule(g.x * f, p.x, q.x, w.x, em.x, lr, decay, has_ema);
      rule(g.y * f, p.y, q.y, w.y, em.y, lr, decay, has_ema);
      rule(g.z * f, p.z, q.z, w.z, em.z, lr, decay, has_ema);
      rule(g.w * f, p.w, q.w, w.w, em.w, lr, decay, has_ema);
      p4[i] = p;
      if constexpr (two) q4[i] = q;
      w4[i] = w;
      if (has_ema) e4[i] = em;
    }
    b += nv << 2;
  }
  for (int64_t i = b + threadIdx.x; i < e; i += THREADS) {
    float p = slot_a[i], q = 0.f, w = params[i], em = has_ema ? ema[i] : 0.f;
    if constexpr (two) q = slot_b[i];
    rule(grads[i] * f, p, q, w, em, lr, decay, has_ema);
    slot_a[i] = p;
    if constexpr (two) slot_b[i] = q;
    params[i] = w;
    if (has_ema) ema[i] = em;
  }
}

// The kernels keep their names and parameter lists: the committed rocprofv3 statistics (profiles/) and the coverage test
// that reads them know the update by kernel symbol.  The second launch bound (8 waves per SIMD, so at most 64 VGPRs) is
// for the two-slot rules: without it the 4-wide Adam body takes 73 VGPRs and drops to 6 waves.
__global__ __launch_bounds__(THREADS, 8) void k_sgd_ema(float* params, float* grads, float* vel, float* ema,
                                                    const int64_t* seg_off, const float* seg_factor,
                                                    const int32_t* seg_flags, const float* hyper, float momentum) {
  update_walk(SgdRule{momentum}, params, grads, vel, nullptr, ema, seg_off, seg_factor, seg_flags, hyper);
}

__global__ __launch_bounds__(THREADS, 8) void k_adam_ema(float* params, const float* grads, float* m1, float* m2, float* ema,
                                                     const int64_t* seg_off, const float* seg_factor,
                                                     const int32_t* seg_flags, const float* hyper, float b1, float b2, float eps) {
  update_walk(AdamRule{b1, b2, eps}, params, grads, m1, m2, ema, seg_off, seg_factor, seg_flags, hyper);
}

__global__ __launch_bounds__(THREADS, 8) void k_rmsprop_ema(float* params, const float* grads, float* ms, float* mom, float* ema,
                                                        const int64_t* seg_off, const float* seg_factor,
                                                        const int32_t* seg_flags, const float* hyper, float rho, float momentum,
                                                        float eps) {
  update_walk(RmspropRule{rho, momentum, eps}, params, grads, ms, mom, ema, seg_off, seg_factor, seg_flags, hyper);
}

// ---- the launch rule of the loss kernels: ONE place, so that the evaluation entry points run the grid of the training ones
// (their sums are promised bit for bit: the partial rows must line up).  Rows are strided over the grid: a quarter of the
// passes, at most `cap` workgroups; ordered partial rows [g][1 + nch] -- the TRAINING row width, whoever asks -- when the
// workspace holds them, else ONE workgroup that adds into the destinations itself.
struct LossGrid { RowMap m; int g; float* part; size_t lds; };
inline LossGrid loss_grid(int ld, int64_t positions, int nch, int64_t cap, void* workspace, size_t workspace_bytes) {
  LossGrid L;
  L.m = row_map(ld);
  L.lds = (size_t)THREADS * 8 * sizeof(float);
  int64_t g = (positions + L.m.rpp - 1) / L.m.rpp;
  g = (g + 3) / 4;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  L.part = (workspace && workspace_bytes >= (size_t)g * (1 + nch) * sizeof(float)) ? reinterpret_cast<float*>(workspace) : nullptr;
  L.g = L.part ? (int)g : 1;
  return L;
}
constexpr int64_t BOX_GRID_CAP = 2048;

// focal cap: one round of the workgroups the chip holds at once, asked of the training kernel k_focal<T, G15> (also with
// label smoothing, and for the evaluation kernels)
inline int64_t focal_grid_cap(int dtype, bool g15) {
  const void* fn = dtype == EDET_BF16 ? (g15 ? reinterpret_cast<const void*>(&k_focal<bf16_t, true>) : reinterpret_cast<const void*>(&k_focal<bf16_t, false>))
                                      : (g15 ? reinterpret_cast<const void*>(&k_focal<float, true>) : reinterpret_cast<const void*>(&k_focal<float, false>));
  const int slots = edet_resident_wgs(fn, THREADS, (size_t)THREADS * 8 * sizeof(float));
  return slots > 0 ? slots : 4096;
}

// f(T{}, bool_constant<G15>, bool_constant<LS>) for the runtime (dtype, gamma == 1.5, label smoothing on); dtype is checked
template <typename F>
inline void focal_dispatch(int dtype, bool g15, bool ls, F&& f) {
  auto by_flags = [&](auto t) {
    if (g15) { if (ls) f(t, std::true_type{}, std::true_type{}); else f(t, std::true_type{}, std::false_type{}); }
    else { if (ls) f(t, std::false_type{}, std::true_type{}); else f(t, std::false_type{}, std::false_type{}); }
  };
  (void)dtype_dispatch(dtype, by_flags);
}

// the hyper-parameters every focal entry point accepts: alpha in [0, 1], gamma finite and >= 0 (a NaN fails both)
inline bool focal_args_ok(float alpha, float gamma) { return alpha >= 0.f && alpha <= 1.f && gamma >= 0.f && gamma <= FLT_MAX; }

}  // namespace

extern "C" int edet_focal_loss_smooth(const void* logits, int ld, const int32_t* cls_targets,
                                      int64_t positions, int num_anchors, int num_classes,
                                      float alpha, float gamma, float label_smoothing, float inv_normalizer,
                                      const float* norm_scale_dev,
                                      void* dlogits, float* dbias, float* sums, void* workspace, size_t workspace_bytes,
                                      int dtype, void* stream) {
  EDET_CHECK(logits && cls_targets && dlogits && sums, "edet_focal_loss: null pointer");
  EDET_CHECK(ld % 8 == 0 && ld >= num_anchors * num_classes && ld <= 2048, "edet_focal_loss: bad ld %d", ld);
  EDET_CHECK(num_classes >= 1, "edet_focal_loss: num_classes must be positive");
  EDET_CHECK(num_anchors >= 1 && positions >= 0, "edet_focal_loss: bad shape");
  EDET_CHECK(label_smoothing >= 0.f && label_smoothing <= 1.f, "edet_focal_loss: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  EDET_CHECK(dtype == EDET_BF16 || dtype == EDET_F32, "edet_focal_loss: bad dtype %d", dtype);
  EDET_CHECK(focal_args_ok(alpha, gamma), "edet_focal_loss: alpha %g outside [0, 1] or gamma %g negative or not finite", (double)alpha, (double)gamma);
  if (positions == 0) return 0;      // nothing to add: sums, dbias and dlogits stay as they are
  const bool g15 = gamma == 1.5f;
  const float half_ls = 0.5f * label_smoothing;
  const int nch = num_anchors * num_classes;
  const LossGrid L = loss_grid(ld, positions, nch, focal_grid_cap(dtype, g15), workspace, workspace_bytes);
  focal_dispatch(dtype, g15, label_smoothing != 0.f, [&](auto t, auto G, auto LS) {
    using T = typename decltype(t)::type;
    if constexpr (decltype(LS)::value)
      edet_launch(k_focal_ls<T, decltype(G)::value>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const T*)logits, ld, cls_targets, positions,
                  num_anchors, num_classes, alpha, gamma, inv_normalizer, norm_scale_dev, (T*)dlogits, dbias, sums, L.part, L.m, half_ls);
    else
      edet_launch(k_focal<T, decltype(G)::value>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const T*)logits, ld, cls_targets, positions,
                  num_anchors, num_classes, alpha, gamma, inv_normalizer, norm_scale_dev, (T*)dlogits, dbias, sums, L.part, L.m);
  });
  if (L.part && edet_reduce_partials2(L.part, L.g, 1 + nch, dbias, nch, &sums[0], to_stream(stream)) != 0) return -2;
  EDET_LAUNCH_CHECK("edet_focal_loss");
  return 0;
}

extern "C" int edet_focal_loss(const void* logits, int ld, const int32_t* cls_targets,
                               int64_t positions, int num_anchors, int num_classes,
                               float alpha, float gamma, float inv_normalizer,
                               const float* norm_scale_dev,
                               void* dlogits, float* dbias, float* sums, void* workspace, size_t workspace_bytes,
                               int dtype, void* stream) {
  return edet_focal_loss_smooth(logits, ld, cls_targets, positions, num_anchors, num_classes, alpha, gamma, 0.f,
                                inv_normalizer, norm_scale_dev, dlogits, dbias, sums, workspace, workspace_bytes, dtype,
                                stream);
}

extern "C" int edet_box_loss(const void* box_out, int ld, const float* box_targets,
                             int64_t positions, int nch, float delta, float inv_normalizer,
                             float grad_scale, const float* norm_scale_dev, void* dbox, float* dbias,
                             float* sums, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  EDET_CHECK(box_out && box_targets && dbox && sums, "edet_box_loss: null pointer");
  EDET_CHECK(ld % 8 == 0 && nch >= 1 && ld >= nch && ld <= 2048 && positions >= 0, "edet_box_loss: bad ld %d", ld);
  EDET_CHECK(dtype == EDET_BF16 || dtype == EDET_F32, "edet_box_loss: bad dtype %d", dtype);
  EDET_CHECK(delta > 0.f && delta <= FLT_MAX, "edet_box_loss: delta %g must be positive and finite", (double)delta);
  if (positions == 0) return 0;      // nothing to add: sums, dbias and dbox stay as they are
  const LossGrid L = loss_grid(ld, positions, nch, BOX_GRID_CAP, workspace, workspace_bytes);
  if (dtype == EDET_BF16)
    edet_launch(k_box<bf16_t>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const bf16_t*)box_out, ld, box_targets, positions, nch, delta, inv_normalizer, grad_scale, norm_scale_dev, (bf16_t*)dbox, dbias, sums, L.part, L.m);
  else
    edet_launch(k_box<float>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const float*)box_out, ld, box_targets, positions, nch, delta, inv_normalizer, grad_scale, norm_scale_dev, (float*)dbox, dbias, sums, L.part, L.m);
  if (L.part && edet_reduce_partials2(L.part, L.g, 1 + nch, dbias, nch, &sums[1], to_stream(stream)) != 0) return -2;
  EDET_LAUNCH_CHECK("edet_box_loss");
  return 0;
}

// ---- the evaluation step's losses (tf2/train_lib.py:686-732, test_step): the sums of the entry points above, bit for bit, with
// no gradient written anywhere.  The grids of loss_grid (a partial row is the workgroup's loss alone), GRAD = false
// instantiations of the same bodies.
extern "C" int edet_focal_loss_eval(const void* logits, int ld, const int32_t* cls_targets,
                                    int64_t positions, int num_anchors, int num_classes,
                                    float alpha, float gamma, float label_smoothing, float inv_normalizer,
                                    const float* norm_scale_dev, float* sums, void* workspace, size_t workspace_bytes,
                                    int dtype, void* stream) {
  EDET_CHECK(logits && cls_targets && sums, "edet_focal_loss_eval: null pointer");
  EDET_CHECK(ld % 8 == 0 && ld >= num_anchors * num_classes && ld <= 2048, "edet_focal_loss_eval: bad ld %d", ld);
  EDET_CHECK(num_classes >= 1 && num_anchors >= 1 && positions >= 0, "edet_focal_loss_eval: bad shape");
  EDET_CHECK(label_smoothing >= 0.f && label_smoothing <= 1.f, "edet_focal_loss_eval: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  EDET_CHECK(dtype == EDET_BF16 || dtype == EDET_F32, "edet_focal_loss_eval: bad dtype %d", dtype);
  EDET_CHECK(focal_args_ok(alpha, gamma), "edet_focal_loss_eval: alpha %g outside [0, 1] or gamma %g negative or not finite", (double)alpha, (double)gamma);
  if (positions == 0) return 0;
  const bool g15 = gamma == 1.5f;
  const float half_ls = 0.5f * label_smoothing;
  const LossGrid L = loss_grid(ld, positions, num_anchors * num_classes, focal_grid_cap(dtype, g15), workspace, workspace_bytes);
  focal_dispatch(dtype, g15, label_smoothing != 0.f, [&](auto t, auto G, auto LS) {
    using T = typename decltype(t)::type;
    edet_launch(k_focal_eval<T, decltype(G)::value, decltype(LS)::value>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const T*)logits, ld, cls_targets,
                positions, num_anchors, num_classes, alpha, gamma, inv_normalizer, norm_scale_dev, sums, L.part, L.m, half_ls);
  });
  if (L.part && edet_reduce_partials2(L.part, L.g, 1, nullptr, 0, &sums[0], to_stream(stream)) != 0) return -2;
  EDET_LAUNCH_CHECK("edet_focal_loss_eval");
  return 0;
}

extern "C" int edet_box_loss_eval(const void* box_out, int ld, const float* box_targets,
                                  int64_t positions, int nch, float delta, float inv_normalizer,
                                  const float* norm_scale_dev, float* sums, void* workspace, size_t workspace_bytes,
                                  int dtype, void* stream) {
  EDET_CHECK(box_out && box_targets && sums, "edet_box_loss_eval: null pointer");
  EDET_CHECK(ld % 8 == 0 && nch >= 1 && ld >= nch && ld <= 2048 && positions >= 0, "edet_box_loss_eval: bad ld %d", ld);
  EDET_CHECK(dtype == EDET_BF16 || dtype == EDET_F32, "edet_box_loss_eval: bad dtype %d", dtype);
  EDET_CHECK(delta > 0.f && delta <= FLT_MAX, "edet_box_loss_eval: delta %g must be positive and finite", (double)delta);
  if (positions == 0) return 0;
  const LossGrid L = loss_grid(ld, positions, nch, BOX_GRID_CAP, workspace, workspace_bytes);
  if (dtype == EDET_BF16)
    edet_launch(k_box_eval<bf16_t>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const bf16_t*)box_out, ld, box_targets, positions, nch, delta, inv_normalizer, norm_scale_dev, sums, L.part, L.m);
  else
    edet_launch(k_box_eval<float>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const float*)box_out, ld, box_targets, positions, nch, delta, inv_normalizer, norm_scale_dev, sums, L.part, L.m);
  if (L.part && edet_reduce_partials2(L.part, L.g, 1, nullptr, 0, &sums[1], to_stream(stream)) != 0) return -2;
  EDET_LAUNCH_CHECK("edet_box_loss_eval");
  return 0;
}

extern "C" int edet_l2_loss(const float* params, const int64_t* seg_offsets, const int32_t* seg_flags, int nseg,
                            float weight_decay, float* seg_l2, float* l2_out, void* stream) {
  EDET_CHECK(params && seg_offsets && seg_flags && seg_l2 && l2_out && nseg > 0, "edet_l2_loss: bad arguments");
  edet_launch(k_l2_loss_slices, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), params, seg_offsets, seg_flags, weight_decay, seg_l2, nseg);
  edet_launch(k_l2_loss_sum, dim3(1), dim3(THREADS), 0, to_stream(stream), (const float*)seg_l2, nseg, l2_out);
  EDET_LAUNCH_CHECK("edet_l2_loss");
  return 0;
}

extern "C" int edet_opt_l2_norms(float* grads, const float* params, const int64_t* seg_offsets,
                                 const int32_t* seg_flags, int nseg, float weight_decay,
                                 float* seg_sqnorm, void* stream) {
  EDET_CHECK(grads && params && seg_offsets && seg_flags && seg_sqnorm && nseg > 0, "edet_opt_l2_norms: bad arguments");
  edet_launch(k_l2_norms, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), grads, params, seg_offsets, seg_flags, weight_decay, seg_sqnorm, nseg);
  EDET_LAUNCH_CHECK("edet_opt_l2_norms");
  return 0;
}

extern "C" int edet_opt_clip_factors(const float* seg_sqnorm, int nseg, float clip_norm,
                                     float* seg_factor, float* global_norm_out, float* l2_sum, void* stream) {
  EDET_CHECK(seg_sqnorm && seg_factor && nseg > 0, "edet_opt_clip_factors: bad arguments");
  edet_launch(k_clip_factors, dim3(1), dim3(THREADS), 0, to_stream(stream), seg_sqnorm, nseg, clip_norm, seg_factor, global_norm_out, l2_sum);
  EDET_LAUNCH_CHECK("edet_opt_clip_factors");
  return 0;
}

extern "C" int edet_opt_scale(float* grads, const int64_t* seg_offsets, const float* seg_factor,
                              int nseg, void* stream) {
  EDET_CHECK(grads && seg_offsets && seg_factor && nseg > 0, "edet_opt_scale: bad arguments");
  edet_launch(k_scale, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), grads, seg_offsets, seg_factor);
  EDET_LAUNCH_CHECK("edet_opt_scale");
  return 0;
}

extern "C" int edet_opt_sgd_ema(float* params, float* grads, float* velocity, float* ema,
                                const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                                const float* hyper_dev, float momentum, void* stream) {
  EDET_CHECK(params && grads && velocity && seg_offsets && hyper_dev && nseg > 0, "edet_opt_sgd_ema: bad arguments");
  edet_launch(k_sgd_ema, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), params, grads, velocity, ema, seg_offsets,
              seg_factor, seg_flags, hyper_dev, momentum);
  EDET_LAUNCH_CHECK("edet_opt_sgd_ema");
  return 0;
}

extern "C" int edet_opt_adam_ema(float* params, const float* grads, float* m, float* v, float* ema,
                                 const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                                 const float* hyper_dev, float beta1, float beta2, float epsilon, void* stream) {
  EDET_CHECK(params && grads && m && v && seg_offsets && hyper_dev && nseg > 0, "edet_opt_adam_ema: bad arguments");
  edet_launch(k_adam_ema, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), params, grads, m, v, ema, seg_offsets,
              seg_factor, seg_flags, hyper_dev, beta1, beta2, epsilon);
  EDET_LAUNCH_CHECK("edet_opt_adam_ema");
  return 0;
}

extern "C" int edet_opt_rmsprop_ema(float* params, const float* grads, float* ms, float* mom, float* ema,
                                    const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                                    const float* hyper_dev, float rho, float momentum, float epsilon, void* stream) {
  EDET_CHECK(params && grads && ms && mom && seg_offsets && hyper_dev && nseg > 0, "edet_opt_rmsprop_ema: bad arguments");
  edet_launch(k_rmsprop_ema, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), params, grads, ms, mom, ema, seg_offsets,
              seg_factor, seg_flags, hyper_dev, rho, momentum, epsilon);
  EDET_LAUNCH_CHECK("edet_opt_rmsprop_ema");
  return 0;
}

// ---- step plumbing that used to be torch calls (round 6: every launch of a step goes through this ABI, so that a step
// can be recorded and replayed by a host without a Python interpreter: net_runtime.cpp) ---------------------------------
namespace {
__global__ __launch_bounds__(THREADS) void k_axpy_clear(float* __restrict__ dst, float* __restrict__ src, int64_t n, int clear) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) {
    dst[i] += src[i];
    if (clear) src[i] = 0.f;
  }
}
// inv_out[0] = 1 / (sum_i mean_num_positives[i] + 1): one wave, lanes in a fixed order (the counts are integers: exact)
__global__ __launch_bounds__(64) void k_loss_normalizer(const float* __restrict__ mnp, int n, float* __restrict__ inv_out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) s += mnp[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) inv_out[0] = 1.0f / (s + 1.0f);
}
}  // namespace

namespace {
__global__ __launch_bounds__(THREADS) void k_widen_bf16(const bf16_t* __restrict__ src, float* __restrict__ dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride)
    dst[i] = __uint_as_float((uint32_t)src[i] << 16);
}
}  // namespace

extern "C" int edet_cast_to_f32(const void* src, float* dst, int64_t count, int src_dtype, void* stream) {
  EDET_CHECK(src && dst, "edet_cast_to_f32: null pointer");
  if (count <= 0) return 0;
  if (src_dtype == EDET_F32) {
    const hipError_t e = hipMemcpyAsync(dst, src, (size_t)count * 4, hipMemcpyDeviceToDevice, to_stream(stream));
    EDET_CHECK(e == hipSuccess, "edet_cast_to_f32: hipMemcpyAsync: %s", hipGetErrorString(e));
    return 0;
  }
  EDET_CHECK(src_dtype == EDET_BF16, "edet_cast_to_f32: bad dtype %d", src_dtype);
  int64_t grid = (count + THREADS - 1) / THREADS;
  if (grid > 4096) grid = 4096;
  edet_launch(k_widen_bf16, dim3((unsigned)grid), dim3(THREADS), 0, to_stream(stream), (const bf16_t*)src, dst, count);
  EDET_LAUNCH_CHECK("edet_cast_to_f32");
  return 0;
}

namespace {
// dst[r][0 .. cw) = src[r][0 .. cw) in 4-byte words: a [rows][ld] tensor without its padding columns
__global__ __launch_bounds__(THREADS) void k_compact_rows(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                         int64_t rows, int cw, int ldw) {
  const int64_t total = rows * cw, stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / cw;
    dst[i] = src[r * ldw + (i - r * cw)];
  }
}
}  // namespace

extern "C" int edet_compact_rows(const void* src, int64_t rows, int c, int ld, void* dst, int elem_bytes, void* stream) {
  EDET_CHECK(src && dst && rows >= 0 && c > 0 && ld >= c, "edet_compact_rows: bad arguments");
  EDET_CHECK((elem_bytes == 2 || elem_bytes == 4) && (c * elem_bytes) % 4 == 0 && (ld * elem_bytes) % 4 == 0,
             "edet_compact_rows: rows must be whole 4-byte words (elem_bytes %d, c %d, ld %d)", elem_bytes, c, ld);
  if (rows == 0) return 0;
  const int cw = c * elem_bytes / 4, ldw = ld * elem_bytes / 4;
  int64_t grid = (rows * cw + THREADS - 1) / THREADS;
  if (grid > 4096) grid = 4096;
  edet_launch(k_compact_rows, dim3((unsigned)grid), dim3(THREADS), 0, to_stream(stream), (const uint32_t*)src, (uint32_t*)dst,
              rows, cw, ldw);
  EDET_LAUNCH_CHECK("edet_compact_rows");
  return 0;
}

namespace {
// A kernel, not hipMemsetAsync: a memset NODE of a captured graph costs a ~50 us bubble in front of it on this runtime
// (r06zz timeline: two fillBufferAligned nodes and the kernel behind them, 0.2 ms of idle queue per step)
__global__ __launch_bounds__(THREADS) void k_zero(uint4* __restrict__ dst16, size_t n16, unsigned char* __restrict__ tail, int ntail) {
  const size_t stride = (size_t)gridDim.x * THREADS;
  for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < n16; i += stride) dst16[i] = make_uint4(0, 0, 0, 0);
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0;
}
}  // namespace

extern "C" int edet_zero(void* dst, size_t bytes, void* stream) {
  EDET_CHECK(dst || bytes == 0, "edet_zero: null pointer");
  if (bytes == 0) return 0;
  // head up to the first 16-byte boundary and tail behind the last one: byte stores of block 0 (at most 15 + 15)
  unsigned char* p = reinterpret_cast<unsigned char*>(dst);
  const size_t mis = (16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15;
  if (mis >= bytes || mis != 0) {
    // unaligned start (not what the engine passes: its buffers are 256-byte aligned): the memset path
    const hipError_t e = hipMemsetAsync(dst, 0, bytes, to_stream(stream));
    EDET_CHECK(e == hipSuccess, "edet_zero: hipMemsetAsync: %s", hipGetErrorString(e));
    return 0;
  }
  const size_t n16 = bytes / 16;
  const int ntail = (int)(bytes - n16 * 16);
  size_t grid = (n16 + THREADS - 1) / THREADS;
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  edet_launch(k_zero, dim3((unsigned)grid), dim3(THREADS), 0, to_stream(stream), reinterpret_cast<uint4*>(p), n16, p + n16 * 16, ntail);
  EDET_LAUNCH_CHECK("edet_zero");
  return 0;
}

extern "C" int edet_axpy_clear(float* dst, float* src, int64_t n, int clear_src, void* stream) {
  EDET_CHECK(dst && src && n >= 0, "edet_axpy_clear: bad arguments");
  if (n == 0) return 0;
  int64_t grid = (n + THREADS - 1) / THREADS;
  if (grid > 2048) grid = 2048;
  edet_launch(k_axpy_clear, dim3((unsigned)grid), dim3(THREADS), 0, to_stream(stream), dst, src, n, clear_src);
  EDET_LAUNCH_CHECK("edet_axpy_clear");
  return 0;
}

extern "C" int edet_loss_normalizer(const float* mean_num_positives, int n, float* inv_out, void* stream) {
  EDET_CHECK(mean_num_positives && inv_out && n > 0, "edet_loss_normalizer: bad arguments");
  edet_launch(k_loss_normalizer, dim3(1), dim3(64), 0, to_stream(stream), mean_num_positives, n, inv_out);
  EDET_LAUNCH_CHECK("edet_loss_normalizer");
  return 0;
}

// ---- EfficientNetV2 classifier training (efficientnetv2/main_tf2.py:36-117,199-207) ------------------------------------
namespace {
constexpr int XENT_ROWS = THREADS / 64;       // one wave per row

// tf.keras.losses.CategoricalCrossentropy(label_smoothing, from_logits=True), mean over the batch, with its gradient and the
// TopKCategoricalAccuracy(1 / 5) counts in one pass over the logits.  Per row: m = max x, lse = m + log sum exp(x - m),
// y_c = (1 - s) [c == label] + s / nc, loss = lse - sum_c y_c x_c, d x_c = (softmax_c - y_c) * grad_scale / B.  A wave owns a
// row (8-element chunks strided over the lanes, xor butterflies: a fixed tree); the waves of a workgroup add their rows in
// wave order, workgroups write [loss / B | top1 | top5] rows that edet_reduce_partials2 adds in order -- no atomics.
// A label outside [0, nc) is refused by the host wrapper's callers (it cannot be seen here without a synchronisation); the
// kernel reads nothing out of bounds for one: such a row has no hot class and counts for neither metric.
template <typename T>
__global__ __launch_bounds__(THREADS) void k_softmax_xent(const T* __restrict__ logits, int ld, const int32_t* __restrict__ labels,
                                                         int batch, int nc, float ls, float gscale, float inv_b,
                                                         T* __restrict__ dlogits, float* sums, float* part) {
  __shared__ float sh[XENT_ROWS][3];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float uni = ls / (float)nc, hot = 1.f - ls;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int row = blockIdx.x * XENT_ROWS + wv; row < batch; row += gridDim.x * XENT_ROWS) {
    const T* x = logits + (size_t)row * ld;
    const int lab = labels[row];
    const bool lab_ok = lab >= 0 && lab < nc;
    const float xl = lab_ok ? to_f<T>(x[lab]) : 0.f;
    float m = -INFINITY;
    for (int c0 = lane * 8; c0 < nc; c0 += 64 * 8) {
      float v[8];
      load8<T>(x + c0, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) if (c0 + e < nc) m = fmaxf(m, v[e]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float r[3] = {0.f, 0.f, 0.f};      // sum exp(x - m), sum x, logits strictly greater than the label's
    for (int c0 = lane * 8; c0 < nc; c0 += 64 * 8) {
      float v[8];
      load8<T>(x + c0, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (c0 + e < nc) {
          r[0] += __expf(v[e] - m);
          r[1] += v[e];
          r[2] += v[e] > xl ? 1.f : 0.f;
        }
      }
    }
    wave_group_sum(r, 1);
    const float inv_se = 1.f / r[0];
    const float lse = m + __logf(r[0]);
    acc[0] += (lse - hot * xl - uni * r[1]) * inv_b;
    acc[1] += (lab_ok && r[2] < 1.f) ? 1.f : 0.f;
    acc[2] += (lab_ok && r[2] < 5.f) ? 1.f : 0.f;
    T* dx = dlogits + (size_t)row * ld;
    for (int c0 = lane * 8; c0 < ld; c0 += 64 * 8) {
      float v[8], g[8];
      load8<T>(x + c0, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = c0 + e;
        const float y = uni + ((lab_ok && c == lab) ? hot : 0.f);
        g[e] = c < nc ? (__expf(v[e] - m) * inv_se - y) * gscale : 0.f;      // padding columns: zeros
      }
      store8<T>(dx + c0, g);
    }
  }
  if (lane == 0) {
    sh[wv][0] = acc[0]; sh[wv][1] = acc[1]; sh[wv][2] = acc[2];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float t = 0.f;
    for (int w = 0; w < XENT_ROWS; ++w) t += sh[w][threadIdx.x];
    if (part) part[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
    else sums[threadIdx.x] += t;          // (no partial buffer: the kernel runs as ONE workgroup)
  }
}

// 8 fp32 soft labels of columns [c0, c0 + 8) of a row, columns >= nc as zeros.  vec: the rows are 16-byte aligned and
// padded to a multiple of 8 columns (two 16-byte loads); otherwise column by column, reading nothing behind column nc.
__device__ __forceinline__ void load8_soft(const float* __restrict__ y, int c0, int nc, bool vec, float v[8]) {
  if (vec && c0 < nc) {
    loadf8(y + c0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = c0 + e < nc ? v[e] : 0.f;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = c0 + e < nc ? y[c0 + e] : 0.f;
  }
}

// The same loss against dense fp32 labels y [batch][label_ld] (one-hot, mixup / cutmix mixtures, anything a caller made):
// Keras smooths whatever it is given, y'_c = (1 - s) y_c + s / nc, and nothing here assumes that a row sums to 1:
// loss = lse * sum y' - sum y'_c x_c, d x_c = (softmax_c * sum y' - y'_c) * grad_scale / B.  The sums are taken of x - m, so
// that the loss is sum y' * log(sum exp(x - m)) - sum y'_c (x_c - m) without the cancellation of two numbers of the size of
// the logits.  TopKCategoricalAccuracy takes the row's class as argmax_c y_c (the first index on ties, found in the pass
// that finds m) and then counts as the sparse kernel does.  Same structure, same ordered sums.
template <typename T>
__global__ __launch_bounds__(THREADS) void k_softmax_xent_soft(const T* __restrict__ logits, int ld, const float* __restrict__ soft,
                                                              int label_ld, int vec, int batch, int nc, float ls, float gscale,
                                                              float inv_b, T* __restrict__ dlogits, float* sums, float* part) {
  __shared__ float sh[XENT_ROWS][3];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float uni = ls / (float)nc, hot = 1.f - ls;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int row = blockIdx.x * XENT_ROWS + wv; row < batch; row += gridDim.x * XENT_ROWS) {
    const T* x = logits + (size_t)row * ld;
    const float* y = soft + (size_t)row * label_ld;
    float m = -INFINITY, ybest = -INFINITY;
    int cls = nc;
    for (int c0 = lane * 8; c0 < nc; c0 += 64 * 8) {
      float v[8], yv[8];
      load8<T>(x + c0, v);
      load8_soft(y, c0, nc, vec, yv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (c0 + e < nc) {
          m = fmaxf(m, v[e]);
          if (yv[e] > ybest) { ybest = yv[e]; cls = c0 + e; }      // (a lane walks its columns in rising order)
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      m = fmaxf(m, __shfl_xor(m, off, 64));
      const float oy = __shfl_xor(ybest, off, 64);
      const int oc = __shfl_xor(cls, off, 64);
      if (oy > ybest || (oy == ybest && oc < cls)) { ybest = oy; cls = oc; }
    }
    const bool cls_ok = cls < nc;
    const float xl = cls_ok ? to_f<T>(x[cls]) : 0.f;
    float r[5] = {0.f, 0.f, 0.f, 0.f, 0.f};      // sum exp(x - m), sum (x - m), logits > the class's, sum y, sum y (x - m)
    for (int c0 = lane * 8; c0 < nc; c0 += 64 * 8) {
      float v[8], yv[8];
      load8<T>(x + c0, v);
      load8_soft(y, c0, nc, vec, yv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (c0 + e < nc) {
          const float d = v[e] - m;
          r[0] += __expf(d);
          r[1] += d;
          r[2] += v[e] > xl ? 1.f : 0.f;
          r[3] += yv[e];
          r[4] += yv[e] * d;
        }
      }
    }
    wave_group_sum(r, 1);
    const float inv_se = 1.f / r[0];
    const float ysum = hot * r[3] + ls;          // sum_c y'_c
    acc[0] += (ysum * __logf(r[0]) - hot * r[4] - uni * r[1]) * inv_b;
    acc[1] += (cls_ok && r[2] < 1.f) ? 1.f : 0.f;
    acc[2] += (cls_ok && r[2] < 5.f) ? 1.f : 0.f;
    T* dx = dlogits + (size_t)row * ld;
    const float pscale = inv_se * ysum;
    for (int c0 = lane * 8; c0 < ld; c0 += 64 * 8) {
      float v[8], yv[8], g[8];
      load8<T>(x + c0, v);
      load8_soft(y, c0, nc, vec, yv);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        g[e] = c0 + e < nc ? (__expf(v[e] - m) * pscale - (hot * yv[e] + uni)) * gscale : 0.f;      // padding columns: zeros
      store8<T>(dx + c0, g);
    }
  }
  if (lane == 0) {
    sh[wv][0] = acc[0]; sh[wv][1] = acc[1]; sh[wv][2] = acc[2];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float t = 0.f;
    for (int w = 0; w < XENT_ROWS; ++w) t += sh[w][threadIdx.x];
    if (part) part[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
    else sums[threadIdx.x] += t;          // (no partial buffer: the kernel runs as ONE workgroup)
  }
}

// out = cast(src * mask): the head dropout (effnetv2_model.py:464-467,483-484) folded into the cast of the pooled sums;
// mask == NULL is edet_cast.  In place (dst == src, fp32) for the backward pass.
template <typename T>
__global__ __launch_bounds__(THREADS) void k_dropout_cast(const float* src, const float* __restrict__ mask, T* dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride)
    dst[i] = from_f<T>(mask ? src[i] * mask[i] : src[i]);
}
}  // namespace

extern "C" int edet_softmax_xent(const void* logits, int ld, const int32_t* labels, int batch, int num_classes,
                                 float label_smoothing, float grad_scale, void* dlogits, float* sums, void* workspace,
                                 size_t workspace_bytes, int dtype, void* stream) {
  EDET_CHECK(logits && labels && dlogits && sums, "edet_softmax_xent: null pointer");
  EDET_CHECK(batch > 0 && num_classes >= 1, "edet_softmax_xent: batch %d, num_classes %d", batch, num_classes);
  EDET_CHECK(ld % 8 == 0 && ld >= num_classes, "edet_softmax_xent: bad ld %d (num_classes %d)", ld, num_classes);
  EDET_CHECK(label_smoothing >= 0.f && label_smoothing <= 1.f, "edet_softmax_xent: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  int g = (batch + XENT_ROWS - 1) / XENT_ROWS;
  if (g > 1024) g = 1024;
  // ordered partial rows [g][3] when the workspace holds them (else: one workgroup walks every row)
  float* part = (g > 1 && workspace && workspace_bytes >= (size_t)g * 3 * sizeof(float)) ? reinterpret_cast<float*>(workspace) : nullptr;
  if (!part) g = 1;
  const float inv_b = 1.f / (float)batch;
  if (dtype == EDET_BF16)
    edet_launch(k_softmax_xent<bf16_t>, dim3(g), dim3(THREADS), 0, to_stream(stream), (const bf16_t*)logits, ld, labels, batch, num_classes, label_smoothing, grad_scale * inv_b, inv_b, (bf16_t*)dlogits, sums, part);
  else if (dtype == EDET_F32)
    edet_launch(k_softmax_xent<float>, dim3(g), dim3(THREADS), 0, to_stream(stream), (const float*)logits, ld, labels, batch, num_classes, label_smoothing, grad_scale * inv_b, inv_b, (float*)dlogits, sums, part);
  else EDET_CHECK(false, "edet_softmax_xent: bad dtype %d", dtype);
  if (part && edet_reduce_partials2(part, g, 3, nullptr, 0, sums, to_stream(stream)) != 0) return -2;
  EDET_LAUNCH_CHECK("edet_softmax_xent");
  return 0;
}

extern "C" int edet_softmax_xent_soft(const void* logits, int ld, const float* soft_labels, int label_ld, int batch, int num_classes,
                                      float label_smoothing, float grad_scale, void* dlogits, float* sums, void* workspace,
                                      size_t workspace_bytes, int dtype, void* stream) {
  EDET_CHECK(logits && soft_labels && dlogits && sums, "edet_softmax_xent_soft: null pointer");
  EDET_CHECK(batch > 0 && num_classes >= 1, "edet_softmax_xent_soft: batch %d, num_classes %d", batch, num_classes);
  EDET_CHECK(ld % 8 == 0 && ld >= num_classes, "edet_softmax_xent_soft: bad ld %d (num_classes %d)", ld, num_classes);
  EDET_CHECK(label_ld >= num_classes, "edet_softmax_xent_soft: bad label_ld %d (num_classes %d)", label_ld, num_classes);
  EDET_CHECK(label_smoothing >= 0.f && label_smoothing <= 1.f, "edet_softmax_xent_soft: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  int g = (batch + XENT_ROWS - 1) / XENT_ROWS;
  if (g > 1024) g = 1024;
  float* part = (g > 1 && workspace && workspace_bytes >= (size_t)g * 3 * sizeof(float)) ? reinterpret_cast<float*>(workspace) : nullptr;
  if (!part) g = 1;
  const float inv_b = 1.f / (float)batch;
  const int vec = label_ld % 8 == 0 && reinterpret_cast<uintptr_t>(soft_labels) % 16 == 0;
  if (dtype == EDET_BF16)
    edet_launch(k_softmax_xent_soft<bf16_t>, dim3(g), dim3(THREADS), 0, to_stream(stream), (const bf16_t*)logits, ld, soft_labels, label_ld, vec, batch, num_classes, label_smoothing, grad_scale * inv_b, inv_b, (bf16_t*)dlogits, sums, part);
  else if (dtype == EDET_F32)
    edet_launch(k_softmax_xent_soft<float>, dim3(g), dim3(THREADS), 0, to_stream(stream), (const float*)logits, ld, soft_labels, label_ld, vec, batch, num_classes, label_smoothing, grad_scale * inv_b, inv_b, (float*)dlogits, sums, part);
  else EDET_CHECK(false, "edet_softmax_xent_soft: bad dtype %d", dtype);
  if (part && edet_reduce_partials2(part, g, 3, nullptr, 0, sums, to_stream(stream)) != 0) return -2;
  EDET_LAUNCH_CHECK("edet_softmax_xent_soft");
  return 0;
}

extern "C" int edet_dropout_cast(const float* src, const float* mask, void* dst, int64_t count, int dtype, void* stream) {
  EDET_CHECK(src && dst, "edet_dropout_cast: null pointer");
  if (count <= 0) return 0;
  int64_t grid = (count + THREADS - 1) / THREADS;
  if (grid > 2048) grid = 2048;
  if (dtype == EDET_BF16) edet_launch(k_dropout_cast<bf16_t>, dim3((unsigned)grid), dim3(THREADS), 0, to_stream(stream), src, mask, (bf16_t*)dst, count);
  else if (dtype == EDET_F32) edet_launch(k_dropout_cast<float>, dim3((unsigned)grid), dim3(THREADS), 0, to_stream(stream), src, mask, (float*)dst, count);
  else EDET_CHECK(false, "edet_dropout_cast: bad dtype %d", dtype);
  EDET_LAUNCH_CHECK("edet_dropout_cast");
  return 0;
}
