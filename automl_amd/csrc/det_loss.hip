// Detection loss (focal + Huber) forward and backward in one pass, the loss-only twins of the evaluation step, the one grid
// rule they share and the loss normalizer.
//
// Reference: efficientdet/tf2/train_lib.py:357-406 (FocalLoss), :409-437 (BoxLoss / Keras Huber),
// :493-604 (_detection_loss), :686-732 (test_step).
#include "iou_impl.h"
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

// acc + v * s and acc + v * s1 * s2 with every product rounded (no contraction: the evaluation kernel's sum is the training
// kernel's bit for bit, whatever else each instantiation computes)
__device__ __forceinline__ float iou_add_scaled(float acc, float v, float s) {
#pragma clang fp contract(off)
  const float t = v * s;
  return acc + t;
}
__device__ __forceinline__ float iou_add_scaled2(float acc, float v, float s1, float s2) {
#pragma clang fp contract(off)
  const float t = v * s1 * s2;
  return acc + t;
}

// The IoU loss of a workgroup (box_body<.., IOU = true>): the loss_tail of a second sum, with an LDS array of its own so that
// it may follow loss_tail without a barrier in between.  part: the workgroup's slot of the ordered partial column, else the
// kernel runs as ONE workgroup and adds into the destination itself.
__device__ __forceinline__ void iou_tail(float acc, float* part, float* sum_dst) {
  __shared__ float wsum_iou[THREADS / 64];
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & 63) == 0) wsum_iou[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < THREADS / 64; ++w) t += wsum_iou[w];
    if (part) part[blockIdx.x] = t; else *sum_dst += t;
  }
}

// What the IoU loss adds to the arguments of the box kernels (train_lib.py:440-464, :580-600): the level's first anchor row
// [ymin, xmin, ymax, xmax] (row (p mod hw) * A + a belongs to position p, anchor a), the type (iou_impl.h), the weight of its
// gradient and the partial column of its sum.
struct IouArgs { const float* anchors; int64_t hw; int type; float grad_scale; float* part; };

// IOU: the thread's 8-channel chunk is two whole anchors (j0 % 8 == 0, four channels each; j < nch cuts the last chunk to one
// for an odd number of anchors).  Where some target component of an anchor is non-zero, iou_decoded adds its loss to a second
// sum (sums[3]) and its gradient, times inv_norm * grad_scale, to the Huber gradient in fp32: dbox is rounded and written
// once, dbias sums what was written.  IOU = false is the kernel as it was, instruction for instruction.
template <typename T, bool GRAD, bool IOU = false>
__device__ __forceinline__ void box_body(const T* out, int ld, const float* tgt, int64_t positions, int nch,
                                         float delta, float inv_norm_h, float grad_scale, const float* norm_scale,
                                         T* dbox, float* dbias, float* sums, float* part, RowMap m, IouArgs iou = IouArgs{}) {
  const float inv_norm = norm_scale ? inv_norm_h * norm_scale[0] : inv_norm_h;
  const int tid = threadIdx.x;
  const int cv = tid % m.tpr, rr = tid / m.tpr;
  const int j0 = cv * 8;
  const bool ok = j0 < ld;
  float loss_acc = 0.f, iou_acc = 0.f, db[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) db[e] = 0.f;
  if (ok) {
    for (int64_t p = (int64_t)blockIdx.x * m.rpp + rr; p < positions; p += (int64_t)gridDim.x * m.rpp) {
      float x[8], g[8], tg[8];
      load8<T>(out + p * ld + j0, x);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = j0 + e;
        g[e] = 0.f;
        if (IOU) tg[e] = 0.f;
        if (j < nch) {
          const float t = tgt[p * nch + j];
          if (IOU) tg[e] = t;
          if (t != 0.f) {
            const float err = x[e] - t;
            const float ae = fabsf(err);
            const bool quad = ae <= delta;
            loss_acc += (quad ? 0.5f * err * err : delta * ae - 0.5f * delta * delta) * inv_norm;
            if (GRAD) g[e] = (quad ? err : (err > 0.f ? delta : -delta)) * inv_norm * grad_scale;
          }
        }
        if (GRAD && !IOU) db[e] += g[e];
      }
      if (IOU) {
        const int64_t arow = (p % iou.hw) * (nch >> 2) + (j0 >> 2);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const float tq[4] = {tg[4 * q], tg[4 * q + 1], tg[4 * q + 2], tg[4 * q + 3]};
          if (tq[0] != 0.f || tq[1] != 0.f || tq[2] != 0.f || tq[3] != 0.f) {      // (never true past nch: tg is 0 there)
            const float4 av = *reinterpret_cast<const float4*>(iou.anchors + (arow + q) * 4);
            const float a[4] = {av.x, av.y, av.z, av.w};
            const float xq[4] = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
            float dx[4];
            const float l = iou_decoded<GRAD>(a, xq, tq, iou.type, dx);
            iou_acc = iou_add_scaled(iou_acc, l, inv_norm);
            if (GRAD) {
#pragma unroll
              for (int k = 0; k < 4; ++k) g[4 * q + k] = iou_add_scaled2(g[4 * q + k], dx[k], inv_norm, iou.grad_scale);
            }
          }
        }
        if (GRAD) {
#pragma unroll
          for (int e = 0; e < 8; ++e) db[e] += g[e];
        }
      }
      if (GRAD) store8<T>(dbox + p * ld + j0, g);
    }
  }
  extern __shared__ float red[];  // [THREADS * 8]
  loss_tail<GRAD>(loss_acc, db, ok, nch, m, red, part, &sums[1], dbias);
  if (IOU) iou_tail(iou_acc, iou.part, &sums[3]);
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

// the box kernels with the IoU loss fused in: one pass over the outputs and the targets, the Huber sum to sums[1] as k_box /
// k_box_eval form it, the IoU sum to sums[3]
template <typename T>
__global__ __launch_bounds__(THREADS) void k_box_iou(const T* __restrict__ out, int ld,
                                                    const float* __restrict__ tgt, int64_t positions, int nch,
                                                    float delta, float inv_norm_h, float grad_scale,
                                                    const float* __restrict__ norm_scale,
                                                    T* __restrict__ dbox, float* dbias, float* sums, float* part, RowMap m,
                                                    IouArgs iou) {
  box_body<T, true, true>(out, ld, tgt, positions, nch, delta, inv_norm_h, grad_scale, norm_scale, dbox, dbias, sums, part, m, iou);
}
template <typename T>
__global__ __launch_bounds__(THREADS) void k_box_iou_eval(const T* __restrict__ out, int ld,
                                                         const float* __restrict__ tgt, int64_t positions, int nch,
                                                         float delta, float inv_norm_h,
                                                         const float* __restrict__ norm_scale, float* sums, float* part, RowMap m,
                                                         IouArgs iou) {
  box_body<T, false, true>(out, ld, tgt, positions, nch, delta, inv_norm_h, 0.f, norm_scale, nullptr, nullptr, sums, part, m, iou);
}

// inv_out[0] = 1 / (sum_i mean_num_positives[i] + 1): one wave, lanes in a fixed order (the counts are integers: exact)
__global__ __launch_bounds__(64) void k_loss_normalizer(const float* __restrict__ mnp, int n, float* __restrict__ inv_out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) s += mnp[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) inv_out[0] = 1.0f / (s + 1.0f);
}

// ---- the launch rule of the loss kernels: ONE place, so that the evaluation entry points run the grid of the training ones
// (their sums are promised bit for bit: the partial rows must line up).  Rows are strided over the grid: a quarter of the
// passes, at most `cap` workgroups; ordered partial rows [g][1 + nch] -- the TRAINING row width, whoever asks -- when the
// workspace holds them, else ONE workgroup that adds into the destinations itself.
struct LossGrid { RowMap m; int g; float* part; size_t lds; };
// extra: further one-float columns behind the g rows (the IoU sum of edet_box_iou_loss: g more floats).
inline LossGrid loss_grid(int ld, int64_t positions, int nch, int64_t cap, void* workspace, size_t workspace_bytes, int extra = 0) {
  LossGrid L;
  L.m = row_map(ld);
  L.lds = (size_t)THREADS * 8 * sizeof(float);
  int64_t g = (positions + L.m.rpp - 1) / L.m.rpp;
  g = (g + 3) / 4;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  L.part = (workspace && workspace_bytes >= (size_t)g * (1 + nch + extra) * sizeof(float)) ? reinterpret_cast<float*>(workspace) : nullptr;
  L.g = L.part ? (int)g : 1;
  return L;
}
constexpr int64_t BOX_GRID_CAP = 2048;

// f(T{}, bool_constant<G15>, bool_constant<LS>) for the runtime (dtype, gamma == 1.5, label smoothing on); dtype is checked
template <typename F>
inline void focal_dispatch(int dtype, bool g15, bool ls, F&& f) {
  auto by_flags = [&](auto t) {
    if (g15) { if (ls) f(t, std::true_type{}, std::true_type{}); else f(t, std::true_type{}, std::false_type{}); }
    else { if (ls) f(t, std::false_type{}, std::true_type{}); else f(t, std::false_type{}, std::false_type{}); }
  };
  (void)dtype_dispatch(dtype, by_flags);
}

// focal cap: one round of the workgroups the chip holds at once, asked of the training kernel k_focal<T, G15> (also with
// label smoothing, and for the evaluation kernels)
inline int64_t focal_grid_cap(int dtype, bool g15) {
  const void* fn = nullptr;
  focal_dispatch(dtype, g15, false, [&](auto t, auto G, auto) {
    fn = reinterpret_cast<const void*>(&k_focal<typename decltype(t)::type, decltype(G)::value>);
  });
  const int slots = edet_resident_wgs(fn, THREADS, (size_t)THREADS * 8 * sizeof(float));
  return slots > 0 ? slots : 4096;
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
  (void)dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    edet_launch(k_box<T>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const T*)box_out, ld, box_targets, positions, nch, delta,
                inv_normalizer, grad_scale, norm_scale_dev, (T*)dbox, dbias, sums, L.part, L.m);
  });
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
  (void)dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    edet_launch(k_box_eval<T>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const T*)box_out, ld, box_targets, positions, nch, delta,
                inv_normalizer, norm_scale_dev, sums, L.part, L.m);
  });
  if (L.part && edet_reduce_partials2(L.part, L.g, 1, nullptr, 0, &sums[1], to_stream(stream)) != 0) return -2;
  EDET_LAUNCH_CHECK("edet_box_loss_eval");
  return 0;
}

// ---- the box loss with the IoU loss fused in (tf2/train_lib.py:440-464, :580-600).  The grid of edet_box_loss for the same
// shape; the partial rows [nch | 1] of edet_box_loss followed by a column of g IoU sums, each added in row order by
// edet_reduce_partials2: sums[1] and, with iou_grad_scale = 0, dbox and dbias are edet_box_loss's bit for bit.  A workspace too
// small for rows and column: ONE workgroup.  No atomics anywhere.
namespace {
inline int iou_args_check(const char* who, const float* anchors, int64_t positions, int nch, int64_t hw, int iou_type) {
  EDET_CHECK(anchors && ((uintptr_t)anchors & 15) == 0, "%s: anchors must be a 16-byte aligned device pointer", who);
  EDET_CHECK(nch % 4 == 0, "%s: nch %d is no multiple of 4", who, nch);
  EDET_CHECK(hw >= 1 && positions % hw == 0, "%s: positions %lld are no multiple of hw %lld", who, (long long)positions, (long long)hw);
  EDET_CHECK(iou_type >= 0 && iou_type < IOU_TYPES, "%s: bad iou_type %d", who, iou_type);
  return 0;
}
}  // namespace

extern "C" int edet_box_iou_loss(const void* box_out, int ld, const float* box_targets,
                                 int64_t positions, int nch, float delta, float inv_normalizer,
                                 float grad_scale, const float* norm_scale_dev, void* dbox, float* dbias,
                                 float* sums, void* workspace, size_t workspace_bytes, int dtype, void* stream,
                                 const float* anchors, int64_t hw, int iou_type, float iou_grad_scale) {
  EDET_CHECK(box_out && box_targets && dbox && sums, "edet_box_iou_loss: null pointer");
  EDET_CHECK(ld % 8 == 0 && nch >= 1 && ld >= nch && ld <= 2048 && positions >= 0, "edet_box_iou_loss: bad ld %d", ld);
  EDET_CHECK(dtype == EDET_BF16 || dtype == EDET_F32, "edet_box_iou_loss: bad dtype %d", dtype);
  EDET_CHECK(delta > 0.f && delta <= FLT_MAX, "edet_box_iou_loss: delta %g must be positive and finite", (double)delta);
  if (iou_args_check("edet_box_iou_loss", anchors, positions, nch, hw, iou_type) != 0) return -1;
  if (positions == 0) return 0;
  const LossGrid L = loss_grid(ld, positions, nch, BOX_GRID_CAP, workspace, workspace_bytes, 1);
  float* part_iou = L.part ? L.part + (size_t)L.g * (1 + nch) : nullptr;
  const IouArgs iou{anchors, hw, iou_type, iou_grad_scale, part_iou};
  (void)dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    edet_launch(k_box_iou<T>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const T*)box_out, ld, box_targets, positions, nch, delta,
                inv_normalizer, grad_scale, norm_scale_dev, (T*)dbox, dbias, sums, L.part, L.m, iou);
  });
  if (L.part && edet_reduce_partials2(L.part, L.g, 1 + nch, dbias, nch, &sums[1], to_stream(stream)) != 0) return -2;
  if (L.part && edet_reduce_partials2(part_iou, L.g, 1, nullptr, 0, &sums[3], to_stream(stream)) != 0) return -2;
  EDET_LAUNCH_CHECK("edet_box_iou_loss");
  return 0;
}

extern "C" int edet_box_iou_loss_eval(const void* box_out, int ld, const float* box_targets,
                                      int64_t positions, int nch, float delta, float inv_normalizer,
                                      const float* norm_scale_dev, float* sums, void* workspace, size_t workspace_bytes,
                                      int dtype, void* stream, const float* anchors, int64_t hw, int iou_type) {
  EDET_CHECK(box_out && box_targets && sums, "edet_box_iou_loss_eval: null pointer");
  EDET_CHECK(ld % 8 == 0 && nch >= 1 && ld >= nch && ld <= 2048 && positions >= 0, "edet_box_iou_loss_eval: bad ld %d", ld);
  EDET_CHECK(dtype == EDET_BF16 || dtype == EDET_F32, "edet_box_iou_loss_eval: bad dtype %d", dtype);
  EDET_CHECK(delta > 0.f && delta <= FLT_MAX, "edet_box_iou_loss_eval: delta %g must be positive and finite", (double)delta);
  if (iou_args_check("edet_box_iou_loss_eval", anchors, positions, nch, hw, iou_type) != 0) return -1;
  if (positions == 0) return 0;
  const LossGrid L = loss_grid(ld, positions, nch, BOX_GRID_CAP, workspace, workspace_bytes, 1);
  float* part_iou = L.part ? L.part + L.g : nullptr;
  const IouArgs iou{anchors, hw, iou_type, 0.f, part_iou};
  (void)dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    edet_launch(k_box_iou_eval<T>, dim3(L.g), dim3(THREADS), L.lds, to_stream(stream), (const T*)box_out, ld, box_targets, positions, nch,
                delta, inv_normalizer, norm_scale_dev, sums, L.part, L.m, iou);
  });
  if (L.part && edet_reduce_partials2(L.part, L.g, 1, nullptr, 0, &sums[1], to_stream(stream)) != 0) return -2;
  if (L.part && edet_reduce_partials2(part_iou, L.g, 1, nullptr, 0, &sums[3], to_stream(stream)) != 0) return -2;
  EDET_LAUNCH_CHECK("edet_box_iou_loss_eval");
  return 0;
}

extern "C" int edet_loss_normalizer(const float* mean_num_positives, int n, float* inv_out, void* stream) {
  EDET_CHECK(mean_num_positives && inv_out && n > 0, "edet_loss_normalizer: bad arguments");
  edet_launch(k_loss_normalizer, dim3(1), dim3(64), 0, to_stream(stream), mean_num_positives, n, inv_out);
  EDET_LAUNCH_CHECK("edet_loss_normalizer");
  return 0;
}
