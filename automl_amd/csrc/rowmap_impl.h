// The row x channel-vector thread map of the 256-lane elementwise / reduction kernels (bn.hip, se.hip, det_loss.hip) and
// the grid rule of the grid-stride elementwise kernels (bn.hip, fuse.hip).  Everything sits in the unnamed namespace:
// RowMap is a kernel parameter, so its name is part of those kernels' symbols.
#pragma once
#include "common.h"

namespace {

constexpr int ROW_THREADS = 256;    // the workgroup size of every kernel that uses these helpers (asserted by the includers)

// Row x channel-vector mapping with a *fixed* channel vector per thread, so per-channel partial
// sums can live in registers: tpr = threads per row (power of two >= c/8, <= 256).
struct RowMap { int tpr, rpp; };  // threads per row, rows per pass
inline RowMap row_map(int c) {
  int nvec = c / 8, tpr = 1;
  while (tpr < nvec && tpr < ROW_THREADS) tpr <<= 1;
  return RowMap{tpr, ROW_THREADS / tpr};
}
inline int persistent_grid(int64_t rows, int rpp, int max_wg) {
  int64_t passes = (rows + rpp - 1) / rpp;
  int64_t g = (passes + 7) / 8;  // at least ~8 passes per workgroup
  if (g < 1) g = 1;
  if (g > max_wg) g = max_wg;
  return (int)g;
}

// The per-channel sums of a workgroup WITHOUT LDS atomics (r04: run-to-run identical results): the row-lanes (rr) of a
// channel chunk park their 8 + 8 sums in scr[2][ROW_THREADS * 8] and the first tpr * 8 threads add them in row-lane order
// into red[cb ..] / red[c + cb ..].  Called by every thread of the workgroup (two barriers).
__device__ __forceinline__ void rowlane_sums(float* scr, const RowMap& m, int cv, int rr, bool ok, const float (&s1)[8],
                                             const float (&s2)[8], float* red, int cb, int c) {
  const int width = m.tpr * 8;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    scr[rr * width + cv * 8 + e] = ok ? s1[e] : 0.f;
    scr[ROW_THREADS * 8 + rr * width + cv * 8 + e] = ok ? s2[e] : 0.f;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < width; t += ROW_THREADS) {
    float u = 0.f, v = 0.f;
    for (int r = 0; r < m.rpp; ++r) { u += scr[r * width + t]; v += scr[ROW_THREADS * 8 + r * width + t]; }
    if (cb + t < c) { red[cb + t] = u; red[c + cb + t] = v; }
  }
}

// grid of a grid-stride elementwise kernel: one thread per item up to ONE ROUND of what the chip holds of this kernel
// (occupancy query; 4096 when unknown) -- with more workgroups than resident slots the last round runs partly empty
inline int ew_grid(int64_t total, const void* fn = nullptr, size_t lds = 0) {
  int64_t g = (total + ROW_THREADS - 1) / ROW_THREADS;
  int cap = 4096;
  if (fn) {
    const int slots = edet_resident_wgs(fn, ROW_THREADS, lds);
    if (slots > 0) cap = slots;
  }
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace
