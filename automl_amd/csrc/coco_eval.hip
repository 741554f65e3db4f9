// COCO box AP / AR on the device (efficientdet/coco_metric.py, which wraps pycocotools' COCOeval for iouType 'bbox'): the
// per-image matching and the per-cell precision / recall curves.  The algorithm is stated in include/edet_hip.h and restated
// in numpy as tests/coco_ref.py; every output is compared with that restatement bit for bit, so the arithmetic is part of the
// interface: this file is compiled with -ffp-contract=off (automl_amd/build.py), every fp64 product, sum and quotient below is
// one rounded operation in the order written, and the thresholds are the caller's doubles, read from device memory.
//
// k_coco_match: one workgroup of ONE wave per image.  The image's rows sit in LDS; lane a * 10 + t holds area range a and IoU
// threshold t (40 of the 64 lanes) and carries its own "ground truth taken" set of 128 bits in two registers.  Rows are
// visited by descending score; for each, the 64 lanes first compute its IoU with every ground truth of its class (one row of
// doubles in LDS, never a matrix), then every (a, t) lane walks the ground truths twice -- the not ignored ones, then the
// ignored ones, which is COCOeval's stable sort by the ignore flag without a sort.  The ten threshold bits of an area range
// come together by one ballot per row.
//
// k_coco_accumulate: one workgroup per (category, area range, cap, threshold).  The category's segment of `perm` is cut into
// 256 consecutive runs, one per thread; the integer tp / fp prefix sums, the suffix maximum of the precision and the 101
// look-ups all work on those runs, so nothing is added in an order that could change.  Only a true-positive row can raise
// the suffix maximum or move the recall, so precision[r] = max of tp / ((fp + tp) + eps) over the true positives whose running
// count c satisfies c / npig >= rec_thrs[r] -- the same doubles COCOeval's searchsorted compares.
#include "common.h"

namespace {

constexpr int NT = EDET_COCO_THRS, NR = EDET_COCO_RECS, NA = EDET_COCO_AREAS, NM = EDET_COCO_CAPS;
constexpr int MAXD = EDET_COCO_MAX_DETS, MAXG = EDET_COCO_MAX_GTS;
constexpr int DF = 6, GF = 7;      // floats per detection / ground-truth row
constexpr int ACC_THREADS = 256;

__device__ __forceinline__ double box_iou(const float* d, const float* g, bool crowd) {
  const double dx = d[0], dy = d[1], dw = d[2], dh = d[3];
  const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
  const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
  if (w <= 0.0) return 0.0;
  const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
  if (h <= 0.0) return 0.0;
  const double i = w * h;
  const double da = dw * dh;
  const double u = crowd ? da : (da + gw * gh) - i;
  return i / u;
}

__global__ __launch_bounds__(64) void k_coco_match(const float* __restrict__ dets, const float* __restrict__ gts, int D, int M,
                                                  const double* __restrict__ iou_thrs, const double* __restrict__ area_rng,
                                                  int32_t* __restrict__ rank, uint16_t* __restrict__ matched,
                                                  uint16_t* __restrict__ ignored) {
  __shared__ float s_d[MAXD * DF];
  __shared__ float s_g[MAXG * GF];
  __shared__ double s_iou[MAXG];
  __shared__ int s_order[MAXD];
  __shared__ uint16_t s_m[NA * MAXD], s_i[NA * MAXD];
  const int img = blockIdx.x, lane = threadIdx.x;
  const float* din = dets + (size_t)img * D * DF;
  const float* gin = gts + (size_t)img * M * GF;
  for (int i = lane; i < D * DF; i += 64) s_d[i] = din[i];
  for (int i = lane; i < M * GF; i += 64) s_g[i] = gin[i];
  for (int i = lane; i < D; i += 64) s_order[i] = -1;
  for (int i = lane; i < NA * D; i += 64) { s_m[i] = 0; s_i[i] = 0; }
  __syncthreads();

  // the order of the visit and the rank among the rows of the same class: by counting, stable in row order
  for (int d = lane; d < D; d += 64) {
    const float cls = s_d[d * DF + 5], sc = s_d[d * DF + 4];
    int r = -1;
    if (cls > -1.f) {
      int p = 0;
      r = 0;
      for (int e = 0; e < D; ++e) {
        const float ce = s_d[e * DF + 5], se = s_d[e * DF + 4];
        const bool before = ce > -1.f && (se > sc || (se == sc && e < d));
        p += before;
        r += before && ce == cls;
      }
      s_order[p] = d;      // p <= D - 1: row d itself is never counted
    }
    rank[(size_t)img * D + d] = r;
  }
  __syncthreads();

  const bool active = lane < NA * NT;
  const int a = active ? lane / NT : 0, t = active ? lane % NT : 0;
  const double thr = iou_thrs[t], lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  uint64_t taken_lo = 0, taken_hi = 0;      // ground truths 0..63 and 64..127 matched at this (a, t)
  for (int p = 0; p < D; ++p) {
    const int d = s_order[p];      // the same in every lane
    if (d < 0) continue;
    const float* dr = s_d + d * DF;
    const float dcls = dr[5];
    for (int g = lane; g < M; g += 64) {
      const float* gr = s_g + g * GF;
      s_iou[g] = (gr[6] > -1.f && gr[6] == dcls) ? box_iou(dr, gr, gr[4] != 0.f) : 0.0;
    }
    __syncthreads();
    double best = fmin(thr, 1.0 - 1e-10);
    int m = -1;
    bool m_ig = false;
    if (active) {
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && m >= 0) break;      // a not ignored match is held: COCOeval stops at the first ignored one
        for (int g = 0; g < M; ++g) {
          const float* gr = s_g + g * GF;
          if (!(gr[6] > -1.f && gr[6] == dcls)) continue;
          const bool crowd = gr[4] != 0.f;
          const double area = gr[5];
          const bool g_ig = crowd || area < lo || area > hi;
          if (g_ig != (pass == 1)) continue;
          const bool was = ((g < 64 ? taken_lo >> g : taken_hi >> (g - 64)) & 1) != 0;
          if (was && !crowd) continue;
          const double v = s_iou[g];
          if (v < best) continue;
          best = v;
          m = g;
          m_ig = g_ig;
        }
      }
    }
    const bool mt = active && m >= 0;
    if (mt) {
      if (m < 64) taken_lo |= (uint64_t)1 << m;
      else taken_hi |= (uint64_t)1 << (m - 64);
    }
    const double darea = (double)(dr[2] * dr[3]);      // the fp32 product, as COCO.loadRes makes it
    const bool ig = active && (mt ? m_ig : (darea < lo || darea > hi));
    const uint64_t bm = __ballot(mt), bi = __ballot(ig);
    if (lane < NA) {
      s_m[lane * D + d] = (uint16_t)((bm >> (lane * NT)) & ((1u << NT) - 1));
      s_i[lane * D + d] = (uint16_t)((bi >> (lane * NT)) & ((1u << NT) - 1));
    }
    __syncthreads();      // s_iou is rewritten for the next row
  }
  __syncthreads();
  for (int i = lane; i < NA * D; i += 64) {
    matched[(size_t)img * NA * D + i] = s_m[i];
    ignored[(size_t)img * NA * D + i] = s_i[i];
  }
}

struct Cell {
  const int32_t* perm;
  const int32_t* rank;
  const uint16_t* matched;
  const uint16_t* ignored;
  int L, D, a, t, cap;
};

// rows [begin, end) of perm: f(tp, fp) after every true positive, with the running counts
template <typename F>
__device__ __forceinline__ void walk(const Cell& c, int begin, int end, int& tp, int& fp, F f) {
  for (int j = begin; j < end; ++j) {
    const int idx = c.perm[j];
    if ((unsigned)idx >= (unsigned)c.L) continue;
    const int rk = c.rank[idx];
    if (rk < 0 || rk >= c.cap) continue;
    const int n = idx / c.D, d = idx - n * c.D;
    const size_t off = ((size_t)n * NA + c.a) * c.D + d;
    if ((c.ignored[off] >> c.t) & 1) continue;
    if ((c.matched[off] >> c.t) & 1) {
      ++tp;
      f(tp, fp);
    } else {
      ++fp;
    }
  }
}

__device__ __forceinline__ double precision_at(int tp, int fp) {
  return (double)tp / (((double)fp + (double)tp) + 0x1p-52);      // np.spacing(1)
}

__global__ __launch_bounds__(ACC_THREADS) void k_coco_accumulate(const int32_t* __restrict__ perm, const int32_t* __restrict__ seg,
                                                                const int32_t* __restrict__ rank,
                                                                const uint16_t* __restrict__ matched,
                                                                const uint16_t* __restrict__ ignored,
                                                                const int32_t* __restrict__ npig, int L, int D, int K,
                                                                const double* __restrict__ rec_thrs, const int32_t* __restrict__ caps,
                                                                double* __restrict__ precision, double* __restrict__ recall) {
  __shared__ int s_tp[ACC_THREADS + 1], s_fp[ACC_THREADS + 1];      // counts in front of each run; [256]: the totals
  __shared__ double s_max[ACC_THREADS + 1];                         // the best precision from each run on to the end
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int t = b % NT; b /= NT;
  const int m = b % NM; b /= NM;
  const int a = b % NA;
  const int k = b / NA;
  const int np = npig[k * NA + a];
  if (np <= 0) return;      // the cell stays -1 (the same in every thread)
  const int s = min(max(seg[k], 0), L), e = min(max(seg[k + 1], s), L);
  const int per = (e - s + ACC_THREADS - 1) / ACC_THREADS;
  const int begin = min(s + tid * per, e), end = min(begin + per, e);
  Cell c;
  c.perm = perm; c.rank = rank; c.matched = matched; c.ignored = ignored;
  c.L = L; c.D = D; c.a = a; c.t = t; c.cap = caps[m];

  int tp = 0, fp = 0;
  walk(c, begin, end, tp, fp, [](int, int) {});
  s_tp[tid + 1] = tp;
  s_fp[tid + 1] = fp;
  __syncthreads();
  if (tid == 0) {      // 256 integer additions: not worth a parallel scan
    s_tp[0] = 0;
    s_fp[0] = 0;
    for (int i = 1; i <= ACC_THREADS; ++i) { s_tp[i] += s_tp[i - 1]; s_fp[i] += s_fp[i - 1]; }
  }
  __syncthreads();
  tp = s_tp[tid];
  fp = s_fp[tid];
  double best = 0.0;
  walk(c, begin, end, tp, fp, [&](int tp_, int fp_) { best = fmax(best, precision_at(tp_, fp_)); });
  s_max[tid] = best;
  __syncthreads();
  if (tid == 0) {
    s_max[ACC_THREADS] = 0.0;
    for (int i = ACC_THREADS - 1; i >= 0; --i) s_max[i] = fmax(s_max[i], s_max[i + 1]);
  }
  __syncthreads();
  const int total = s_tp[ACC_THREADS];
  const double npd = (double)np;
  if (tid == ACC_THREADS - 1) recall[((size_t)t * K + k) * NA * NM + a * NM + m] = (double)total / npd;
  if (tid < NR) {
    const double thr = rec_thrs[tid];
    // the smallest count c with c / npig >= thr, by the comparison searchsorted makes; the estimate is off by one at most
    int cnt = (int)fmin(fmax(ceil(thr * npd), 0.0), 2147483000.0);
    for (int it = 0; it < 4 && cnt > 0 && (double)(cnt - 1) / npd >= thr; ++it) --cnt;
    for (int it = 0; it < 4 && (double)cnt / npd < thr; ++it) ++cnt;
    if (cnt < 1) cnt = 1;      // rc >= 0 holds at the first row: every true positive counts
    double q = 0.0;
    if (cnt <= total) {
      int lo_ = 0, hi_ = ACC_THREADS - 1;      // the last run with fewer than cnt true positives in front of it
      while (lo_ < hi_) {
        const int mid = (lo_ + hi_ + 1) >> 1;
        if (s_tp[mid] < cnt) lo_ = mid; else hi_ = mid - 1;
      }
      q = s_max[lo_ + 1];
      const int rb = min(s + lo_ * per, e), re = min(rb + per, e);
      int tp2 = s_tp[lo_], fp2 = s_fp[lo_];
      walk(c, rb, re, tp2, fp2, [&](int tp_, int fp_) { if (tp_ >= cnt) q = fmax(q, precision_at(tp_, fp_)); });
    }
    precision[(((size_t)t * NR + tid) * K + k) * NA * NM + a * NM + m] = q;
  }
}

}  // namespace

extern "C" int edet_coco_match(const float* dets, const float* gts, int n_images, int max_dets, int max_gts,
                               const double* iou_thrs, const double* area_rng, int32_t* rank, uint16_t* matched,
                               uint16_t* ignored, void* stream) {
  EDET_CHECK(dets && gts && iou_thrs && area_rng && rank && matched && ignored, "edet_coco_match: null pointer");
  EDET_CHECK(n_images > 0 && max_dets >= 1 && max_dets <= MAXD && max_gts >= 1 && max_gts <= MAXG,
             "edet_coco_match: %d images, %d detection rows (1..%d), %d ground-truth rows (1..%d)", n_images, max_dets, MAXD,
             max_gts, MAXG);
  EDET_CHECK((int64_t)n_images * max_dets < (int64_t)1 << 29, "edet_coco_match: %d images x %d rows too large", n_images,
             max_dets);
  edet_launch(k_coco_match, dim3((unsigned)n_images), dim3(64), 0, to_stream(stream), dets, gts, max_dets, max_gts, iou_thrs,
              area_rng, rank, matched, ignored);
  EDET_LAUNCH_CHECK("edet_coco_match");
  return 0;
}

extern "C" int edet_coco_accumulate(const int32_t* perm, const int32_t* seg, const int32_t* rank, const uint16_t* matched,
                                    const uint16_t* ignored, const int32_t* npig, int n_images, int max_dets, int n_cats,
                                    const double* rec_thrs, const int32_t* caps, double* precision, double* recall,
                                    void* stream) {
  EDET_CHECK(perm && seg && rank && matched && ignored && npig && rec_thrs && caps && precision && recall,
             "edet_coco_accumulate: null pointer");
  EDET_CHECK(n_images > 0 && max_dets >= 1 && max_dets <= MAXD && n_cats > 0 && n_cats <= (1 << 20),
             "edet_coco_accumulate: %d images, %d detection rows (1..%d), %d categories", n_images, max_dets, MAXD, n_cats);
  EDET_CHECK((int64_t)n_images * max_dets < (int64_t)1 << 29, "edet_coco_accumulate: %d images x %d rows too large", n_images,
             max_dets);
  const unsigned grid = (unsigned)n_cats * NA * NM * NT;
  edet_launch(k_coco_accumulate, dim3(grid), dim3(ACC_THREADS), 0, to_stream(stream), perm, seg, rank, matched, ignored, npig,
              n_images * max_dets, max_dets, n_cats, rec_thrs, caps, precision, recall);
  EDET_LAUNCH_CHECK("edet_coco_accumulate");
  return 0;
}
