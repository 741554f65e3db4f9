// Weighted box fusion on the device (efficientdet/tf2/wbf.py:70-95): the sequential clustering of one image's detections per
// class and the final ordering by score.  The algorithm is stated in include/edet_hip.h and restated in numpy as
// tests/wbf_ref.py; the outputs are compared with that restatement bit for bit, so the arithmetic is part of the interface:
// this file is compiled with -ffp-contract=off (automl_amd/build.py) and every fp32 product, sum and quotient below is one
// rounded operation in the order written.
//
// k_wbf_cluster: one workgroup of ONE wave per (image, class).  The wave first lists the rows of its class in input order (a
// ballot and a prefix count per 64 rows) and leaves at once if there are none.  Cluster j lives in lane j % 64, slot j / 64:
// its running sums (the four coordinates times the score, the scores), its member count, its first member and its current
// average sit in LDS at index j, and only lane j % 64 ever reads or writes them, so the row loop needs no barrier.  Per row
// every lane computes the IoU of its clusters' averages with the row and keeps its best; a butterfly of shuffles under one
// total order (a NaN beats every number, then the larger value, then the lower index) leaves the same winner in every lane;
// the owning lane adds the row to that cluster or founds a new one.  A cluster's result goes to the row of its first member
// in `scratch`, which no other wave writes.
//
// k_wbf_order: one workgroup per image.  The rank of a flagged row is the number of flagged rows with a higher score, or an
// equal score and a smaller (class, row) key: the stable descending sort of the reference's list without a sort.
#include "common.h"

namespace {

constexpr int MAXN = EDET_WBF_MAX_ROWS;
constexpr int F = 7;      // floats per row: image id, x1, y1, x2, y2, score, class
constexpr int ORDER_THREADS = 256;

// wbf.py:21-34, operation by operation.  fmaxf / fminf are exact here: the coordinates are finite by contract, and the only
// NaN that can arise is the final quotient (0 / 0 between two boxes without area), which is never passed through them.
__device__ __forceinline__ float wbf_iou(float x11, float y11, float x12, float y12, float x21, float y21, float x22, float y22) {
  const float xa = fmaxf(x11, x21), ya = fmaxf(y11, y21);
  const float xb = fminf(x12, x22), yb = fminf(y12, y22);
  const float inter = fmaxf(xb - xa, 0.f) * fmaxf(yb - ya, 0.f);
  const float area_a = (x12 - x11) * (y12 - y11);
  const float area_b = (x22 - x21) * (y22 - y21);
  return inter / ((area_a + area_b) - inter);
}

// is candidate (av, ai) ahead of (bv, bi) as numpy's max / argmax see them?  An index < 0 is "no candidate".
__device__ __forceinline__ bool wbf_ahead(float av, int ai, float bv, int bi) {
  if (ai < 0) return false;
  if (bi < 0) return true;
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return (an && bn) ? ai < bi : an;
  if (av != bv) return av > bv;
  return ai < bi;
}

__global__ __launch_bounds__(64) void k_wbf_cluster(const float* __restrict__ dets, const int32_t* __restrict__ counts, int N,
                                                   int num_classes, int num_models, float* __restrict__ scratch,
                                                   int32_t* __restrict__ flags) {
  __shared__ int s_rows[MAXN];
  __shared__ float s_sum[5][MAXN];      // sum of x1 s, y1 s, x2 s, y2 s, s over the members, in member order
  __shared__ float s_avg[4][MAXN];      // the current weighted averages of the coordinates
  __shared__ int s_n[MAXN], s_first[MAXN];
  const int img = blockIdx.x / num_classes, cid = blockIdx.x - img * num_classes;
  const int lane = threadIdx.x;
  const float* rows = dets + (size_t)img * N * F;
  int count = counts ? counts[img] : N;
  count = min(max(count, 0), N);
  const float want = (float)cid;

  int total = 0;
  for (int base = 0; base < count; base += 64) {
    const int r = base + lane;
    const bool mine = r < count && rows[(size_t)r * F + 6] == want;
    const uint64_t ball = __ballot(mine);
    if (mine) s_rows[total + __popcll(ball & (((uint64_t)1 << lane) - 1))] = r;      // < count <= N <= MAXN
    total += __popcll(ball);
  }
  if (total == 0) return;      // the same in every lane
  __syncthreads();

  int ncl = 0;      // clusters so far, the same in every lane
  for (int m = 0; m < total; ++m) {
    const int r = s_rows[m];
    const float* d = rows + (size_t)r * F;
    const float x1 = d[1], y1 = d[2], x2 = d[3], y2 = d[4], sc = d[5];
    float bv = 0.f;
    int bi = -1;
    for (int j = lane; j < ncl; j += 64) {
      const float v = wbf_iou(s_avg[0][j], s_avg[1][j], s_avg[2][j], s_avg[3][j], x1, y1, x2, y2);
      if (wbf_ahead(v, j, bv, bi)) { bv = v; bi = j; }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (wbf_ahead(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    // wbf.py:41-48: no cluster yet, or max < 0.55 (a NaN is not below it)
    const bool found = ncl == 0 || bv < 0.55f;
    const int j = found ? ncl : bi;      // 0 <= j <= m < MAXN
    if ((j & 63) == lane) {
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
      int n = 0;
      if (found) {
        s_first[j] = r;
      } else {
        s0 = s_sum[0][j]; s1 = s_sum[1][j]; s2 = s_sum[2][j]; s3 = s_sum[3][j]; s4 = s_sum[4][j];
        n = s_n[j];
      }
      s0 = s0 + x1 * sc; s1 = s1 + y1 * sc; s2 = s2 + x2 * sc; s3 = s3 + y2 * sc; s4 = s4 + sc;
      s_sum[0][j] = s0; s_sum[1][j] = s1; s_sum[2][j] = s2; s_sum[3][j] = s3; s_sum[4][j] = s4;
      s_n[j] = n + 1;
      s_avg[0][j] = s0 / s4; s_avg[1][j] = s1 / s4; s_avg[2][j] = s2 / s4; s_avg[3][j] = s3 / s4;
    }
    ncl += found;
  }

  for (int j = lane; j < ncl; j += 64) {
    const int first = s_first[j], n = s_n[j];
    const float* d = rows + (size_t)first * F;
    float* o = scratch + ((size_t)img * N + first) * F;
    const double part = (double)n / (double)num_models;      // min(1, n / num_models), Python's double
    const float factor = (float)(part < 1.0 ? part : 1.0);
    o[0] = d[0];
    o[1] = s_avg[0][j]; o[2] = s_avg[1][j]; o[3] = s_avg[2][j]; o[4] = s_avg[3][j];
    o[5] = (s_sum[4][j] / (float)n) * factor;
    o[6] = d[6];
    flags[(size_t)img * N + first] = 1;
  }
}

__global__ __launch_bounds__(ORDER_THREADS) void k_wbf_order(const float* __restrict__ scratch, const int32_t* __restrict__ flags,
                                                            int N, float* __restrict__ fused, int32_t* __restrict__ fused_counts) {
  __shared__ float s_score[MAXN], s_cls[MAXN];
  __shared__ int s_flag[MAXN];
  const int img = blockIdx.x, tid = threadIdx.x;
  const float* in = scratch + (size_t)img * N * F;
  float* out = fused + (size_t)img * N * F;
  for (int r = tid; r < N; r += ORDER_THREADS) {
    const int f = flags[(size_t)img * N + r] != 0;
    s_flag[r] = f;
    s_score[r] = f ? in[(size_t)r * F + 5] : 0.f;
    s_cls[r] = f ? in[(size_t)r * F + 6] : 0.f;
  }
  __syncthreads();
  int total = 0;
  for (int e = 0; e < N; ++e) total += s_flag[e];
  for (int r = tid; r < N; r += ORDER_THREADS) {
    if (s_flag[r]) {
      const float sr = s_score[r], cr = s_cls[r];
      int rank = 0;
      for (int e = 0; e < N; ++e) {
        const float se = s_score[e], ce = s_cls[e];
        rank += s_flag[e] && (se > sr || (se == sr && (ce < cr || (ce == cr && e < r))));
      }
      for (int c = 0; c < F; ++c) out[(size_t)rank * F + c] = in[(size_t)r * F + c];      // rank < total <= N
    }
    if (r >= total) {
      for (int c = 0; c < F; ++c) out[(size_t)r * F + c] = 0.f;
    }
  }
  if (tid == 0) fused_counts[img] = total;
}

}  // namespace

extern "C" int edet_wbf_cluster(const float* dets, const int32_t* counts, int batch, int rows, int num_classes, int num_models,
                                float* scratch, int32_t* flags, void* stream) {
  EDET_CHECK(dets && scratch && flags, "edet_wbf_cluster: null pointer");
  EDET_CHECK(batch > 0 && rows >= 1 && rows <= MAXN && num_classes > 0 && num_models >= 1,
             "edet_wbf_cluster: %d images, %d rows (1..%d), %d classes, %d models", batch, rows, MAXN, num_classes, num_models);
  EDET_CHECK((int64_t)batch * num_classes < (int64_t)1 << 31, "edet_wbf_cluster: %d images x %d classes too large", batch,
             num_classes);
  edet_launch(k_wbf_cluster, dim3((unsigned)(batch * num_classes)), dim3(64), 0, to_stream(stream), dets, counts, rows,
              num_classes, num_models, scratch, flags);
  EDET_LAUNCH_CHECK("edet_wbf_cluster");
  return 0;
}

extern "C" int edet_wbf_order(const float* scratch, const int32_t* flags, int batch, int rows, float* fused,
                              int32_t* fused_counts, void* stream) {
  EDET_CHECK(scratch && flags && fused && fused_counts, "edet_wbf_order: null pointer");
  EDET_CHECK(batch > 0 && rows >= 1 && rows <= MAXN, "edet_wbf_order: %d images, %d rows (1..%d)", batch, rows, MAXN);
  edet_launch(k_wbf_order, dim3((unsigned)batch), dim3(ORDER_THREADS), 0, to_stream(stream), scratch, flags, rows, fused,
              fused_counts);
  EDET_LAUNCH_CHECK("edet_wbf_order");
  return 0;
}
