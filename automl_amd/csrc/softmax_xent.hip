// EfficientNetV2 classifier training (efficientnetv2/main_tf2.py:36-117,199-207): softmax cross-entropy against sparse and
// against dense labels with its gradient and the top-1 / top-5 counts, and the head dropout folded into a cast.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int XENT_ROWS = THREADS / 64;       // one wave per row

// The tail the two cross-entropy kernels share: the waves of the workgroup add their [loss / B | top1 | top5] sums in wave
// order, and the workgroup writes its row of part, or adds into sums itself.
__device__ __forceinline__ void xent_tail(float loss, float top1, float top5, int lane, int wv, float* sums, float* part) {
  __shared__ float sh[XENT_ROWS][3];
  if (lane == 0) {
    sh[wv][0] = loss; sh[wv][1] = top1; sh[wv][2] = top5;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float t = 0.f;
    for (int w = 0; w < XENT_ROWS; ++w) t += sh[w][threadIdx.x];
    if (part) part[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
    else sums[threadIdx.x] += t;          // (no partial buffer: the kernel runs as ONE workgroup)
  }
}

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
  xent_tail(acc[0], acc[1], acc[2], lane, wv, sums, part);
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
  xent_tail(acc[0], acc[1], acc[2], lane, wv, sums, part);
}

// out = cast(src * mask): the head dropout (effnetv2_model.py:464-467,483-484) folded into the cast of the pooled sums;
// mask == NULL is edet_cast.  In place (dst == src, fp32) for the backward pass.
template <typename T>
__global__ __launch_bounds__(THREADS) void k_dropout_cast(const float* src, const float* __restrict__ mask, T* dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride)
    dst[i] = from_f<T>(mask ? src[i] * mask[i] : src[i]);
}

// The host side the two cross-entropy entry points share (`name`: the entry point, for its messages): the checks on the
// common arguments, one workgroup per XENT_ROWS rows up to 1024, ordered partial rows [g][3] when there is more than one
// workgroup and the workspace holds them (else: one workgroup walks every row and adds into sums itself), and their sum.
// launch(type_tag<T>, g, part, inv_b) launches the entry point's kernel.
template <typename Launch>
int softmax_xent_run(const char* name, int ld, int batch, int num_classes, float label_smoothing, float* sums, void* workspace,
                     size_t workspace_bytes, int dtype, hipStream_t st, Launch&& launch) {
  EDET_CHECK(batch > 0 && num_classes >= 1, "%s: batch %d, num_classes %d", name, batch, num_classes);
  EDET_CHECK(ld % 8 == 0 && ld >= num_classes, "%s: bad ld %d (num_classes %d)", name, ld, num_classes);
  EDET_CHECK(label_smoothing >= 0.f && label_smoothing <= 1.f, "%s: label_smoothing %g outside [0, 1]", name, (double)label_smoothing);
  int g = (batch + XENT_ROWS - 1) / XENT_ROWS;
  if (g > 1024) g = 1024;
  float* part = (g > 1 && workspace && workspace_bytes >= (size_t)g * 3 * sizeof(float)) ? reinterpret_cast<float*>(workspace) : nullptr;
  if (!part) g = 1;
  const float inv_b = 1.f / (float)batch;
  EDET_CHECK(dtype_dispatch(dtype, [&](auto t) { launch(t, g, part, inv_b); }), "%s: bad dtype %d", name, dtype);
  if (part && edet_reduce_partials2(part, g, 3, nullptr, 0, sums, st) != 0) return -2;
  EDET_LAUNCH_CHECK(name);
  return 0;
}

}  // namespace

extern "C" int edet_softmax_xent(const void* logits, int ld, const int32_t* labels, int batch, int num_classes,
                                 float label_smoothing, float grad_scale, void* dlogits, float* sums, void* workspace,
                                 size_t workspace_bytes, int dtype, void* stream) {
  EDET_CHECK(logits && labels && dlogits && sums, "edet_softmax_xent: null pointer");
  return softmax_xent_run("edet_softmax_xent", ld, batch, num_classes, label_smoothing, sums, workspace, workspace_bytes, dtype,
                          to_stream(stream), [&](auto t, int g, float* part, float inv_b) {
    using T = typename decltype(t)::type;
    edet_launch(k_softmax_xent<T>, dim3(g), dim3(THREADS), 0, to_stream(stream), (const T*)logits, ld, labels, batch, num_classes,
                label_smoothing, grad_scale * inv_b, inv_b, (T*)dlogits, sums, part);
  });
}

extern "C" int edet_softmax_xent_soft(const void* logits, int ld, const float* soft_labels, int label_ld, int batch, int num_classes,
                                      float label_smoothing, float grad_scale, void* dlogits, float* sums, void* workspace,
                                      size_t workspace_bytes, int dtype, void* stream) {
  EDET_CHECK(logits && soft_labels && dlogits && sums, "edet_softmax_xent_soft: null pointer");
  EDET_CHECK(label_ld >= num_classes, "edet_softmax_xent_soft: bad label_ld %d (num_classes %d)", label_ld, num_classes);
  const int vec = label_ld % 8 == 0 && reinterpret_cast<uintptr_t>(soft_labels) % 16 == 0;
  return softmax_xent_run("edet_softmax_xent_soft", ld, batch, num_classes, label_smoothing, sums, workspace, workspace_bytes, dtype,
                          to_stream(stream), [&](auto t, int g, float* part, float inv_b) {
    using T = typename decltype(t)::type;
    edet_launch(k_softmax_xent_soft<T>, dim3(g), dim3(THREADS), 0, to_stream(stream), (const T*)logits, ld, soft_labels, label_ld, vec,
                batch, num_classes, label_smoothing, grad_scale * inv_b, inv_b, (T*)dlogits, sums, part);
  });
}

extern "C" int edet_dropout_cast(const float* src, const float* mask, void* dst, int64_t count, int dtype, void* stream) {
  EDET_CHECK(src && dst, "edet_dropout_cast: null pointer");
  if (count <= 0) return 0;
  EDET_CHECK(dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    edet_launch(k_dropout_cast<T>, dim3(flat_grid(count, 2048)), dim3(THREADS), 0, to_stream(stream), src, mask, (T*)dst, count);
  }), "edet_dropout_cast: bad dtype %d", dtype);
  EDET_LAUNCH_CHECK("edet_dropout_cast");
  return 0;
}
