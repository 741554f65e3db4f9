// The partial-sum reduction service: "dst += the sum of my P partial rows", the last stage of every kernel that hands its
// workgroups' sums over through a workspace instead of atomics (pw_gemm, pw_big, pw_stream_*, pw_tile_bwd, dwconv, dw_march,
// stem, fuse, det_loss, softmax_xent): at once (k_reduce_partials) or recorded per stream and batched (k_reduce_batch, edet_reduce_defer).
#include <map>
#include <vector>

#include "common.h"

namespace {

// dst[i] += sum over the P partial rows: thread (element e = tid & 15, slice sl = tid >> 4) sums rows
// sl, sl+64, ... with two independent loads in flight, the 64 slices are combined through LDS.
constexpr int RED_SL = 64;      // row slices per element: 16 elements x 64 slices = 1024 lanes
__global__ __launch_bounds__(16 * RED_SL) void k_reduce_partials(const float* __restrict__ ws, int P, int64_t n,
                                                                float* __restrict__ dst, int accumulate,
                                                                int64_t n_a = -1, float* __restrict__ dst_b = nullptr) {
  __shared__ float red[RED_SL][17];
  const int e = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int64_t i = (int64_t)blockIdx.x * 16 + e;
  float s0 = 0.f, s1 = 0.f;
  if (i < n) {
    int p = sl;
    for (; p + RED_SL < P; p += 2 * RED_SL) {
      s0 += ws[(size_t)p * n + i];
      s1 += ws[(size_t)(p + RED_SL) * n + i];
    }
    if (p < P) s0 += ws[(size_t)p * n + i];
  }
  red[sl][e] = s0 + s1;
  __syncthreads();
  if (sl == 0 && i < n) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < RED_SL; ++k) t += red[k][e];
    // two destinations (edet_reduce_partials2): columns [0, n_a) -> dst (may be NULL: dropped), [n_a, n) -> dst_b
    float* d = (n_a < 0 || i < n_a) ? (dst ? dst + i : nullptr) : dst_b + (i - n_a);
    if (d) *d = accumulate ? *d + t : t;
  }
}

int launch_reduce(const char* who, const float* ws, int P, int64_t n, float* dst, int accumulate, int64_t n_a, float* dst_b,
                  hipStream_t st) {
  edet_launch(k_reduce_partials, dim3((unsigned)((n + 15) / 16)), dim3(16 * RED_SL), 0, st, ws, P, n, dst, accumulate, n_a, dst_b);
  EDET_LAUNCH_CHECK(who);
  return 0;
}

// ---- deferred, batched partial-sum reductions (r04) -----------------------------------------------------------------
// Every weight-gradient kernel of the backward pass ends in "dst += sum of my P partial rows": 192 launches of ~7 us per
// D0 step, each a kernel boundary on the critical chain.  With deferral on for a stream (edet_reduce_defer),
// edet_reduce_partials records (ws, P, n, dst) instead of launching; edet_reduce_flush launches ONE kernel over the
// recorded table (passed by value as kernel arguments, <= RED_BATCH entries per launch: nothing is copied to the device,
// so a flush is legal inside a hipGraph capture).  Entries with the same destination (the tower kernels shared by the
// pyramid levels) form a group that one set of workgroups adds in recording order: a fixed summation order (the same bits on
// every run), though not the immediate kernel's.  The caller keeps the partial regions intact until the flush (edet_reduce_deferred_end tells it how
// far they reach).
constexpr int RED_BATCH = 96;
struct RedItem { const float* ws; float* dst; int P; int n; };
struct RedBatch {
  RedItem it[RED_BATCH];
  unsigned short gfirst[RED_BATCH + 1];     // group g = items gfirst[g] .. gfirst[g+1]-1 (same dst, same n)
  int gblock[RED_BATCH + 1];                // prefix sum of the groups' 64-element blocks
  int ngroups;
};

// Workgroup = 64 consecutive elements x 4 row slices: every row is read in whole 256-byte segments (the immediate kernel
// reads 64-byte ones), thread (e, sl) adds the rows sl, sl + 4, ... with four independent running sums, the four slices
// are combined in slice order.  A fixed order -- the same bits on every run -- but not the immediate kernel's order.
constexpr int RB_E = 64, RB_S = 4;
__global__ __launch_bounds__(RB_E * RB_S) void k_reduce_batch(const RedBatch b) {
  __shared__ float red[RB_S][RB_E];
  int g = 0;
  while (g + 1 < b.ngroups && (int)blockIdx.x >= b.gblock[g + 1]) ++g;
  const int e = threadIdx.x & (RB_E - 1), sl = threadIdx.x / RB_E;
  const int64_t n = b.it[b.gfirst[g]].n;
  const int64_t i = (int64_t)(blockIdx.x - b.gblock[g]) * RB_E + e;
  const bool ok = i < n;
  float acc = 0.f;
  float* dst = b.it[b.gfirst[g]].dst;
  if (sl == 0 && ok) acc = dst[i];
  for (int m = b.gfirst[g]; m < b.gfirst[g + 1]; ++m) {
    const float* ws = b.it[m].ws + (ok ? i : 0);
    const int P = b.it[m].P;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int p = sl;
    for (; p + 3 * RB_S < P; p += 4 * RB_S) {
      s0 += ws[(size_t)p * n];
      s1 += ws[(size_t)(p + RB_S) * n];
      s2 += ws[(size_t)(p + 2 * RB_S) * n];
      s3 += ws[(size_t)(p + 3 * RB_S) * n];
    }
    for (; p < P; p += RB_S) s0 += ws[(size_t)p * n];
    __syncthreads();
    red[sl][e] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sl == 0) acc += (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  }
  if (sl == 0 && ok) dst[i] = acc;
}

struct DeferState {
  bool on = false;
  std::vector<RedItem> items;
  const unsigned char* hi = nullptr;
};
std::map<hipStream_t, DeferState>& defer_map() {
  static std::map<hipStream_t, DeferState> m;
  return m;
}

int flush_stream(hipStream_t st, DeferState& d) {
  std::vector<RedItem> items;
  items.swap(d.items);
  d.hi = nullptr;
  // groups: entries with the same destination, members in recording order, groups in order of first appearance
  std::vector<std::vector<RedItem>> groups;
  for (const RedItem& r : items) {
    size_t g = 0;
    while (g < groups.size() && groups[g][0].dst != r.dst) ++g;
    if (g == groups.size()) groups.emplace_back();
    groups[g].push_back(r);
  }
  RedBatch b;
  int ni = 0, ng = 0, nblocks = 0;
  auto launch = [&]() -> int {
    if (ni == 0) return 0;
    b.gfirst[ng] = (unsigned short)ni;
    b.gblock[ng] = nblocks;
    b.ngroups = ng;
    edet_launch(k_reduce_batch, dim3((unsigned)nblocks), dim3(RB_E * RB_S), 0, st, b);
    EDET_LAUNCH_CHECK("edet_reduce_flush");
    ni = ng = nblocks = 0;
    return 0;
  };
  memset(&b, 0, sizeof(b));
  for (const std::vector<RedItem>& grp : groups) {
    size_t pos = 0;
    while (pos < grp.size()) {
      const size_t left = grp.size() - pos;
      size_t take = left < (size_t)(RED_BATCH - ni) ? left : (size_t)(RED_BATCH - ni);
      // a group is split over two launches (stream order keeps the sum order) only when it alone exceeds a batch
      if (take == 0 || (take < left && ni > 0)) {
        if (int rc = launch()) return rc;
        continue;
      }
      b.gfirst[ng] = (unsigned short)ni;
      b.gblock[ng] = nblocks;
      for (size_t k = 0; k < take; ++k) b.it[ni++] = grp[pos + k];
      nblocks += (grp[0].n + RB_E - 1) / RB_E;
      ++ng;
      pos += take;
    }
  }
  return launch();
}

}  // namespace

extern "C" int edet_reduce_defer(void* stream, int enable) {
  DeferState& d = defer_map()[to_stream(stream)];
  if (!enable && d.on && !d.items.empty()) {
    if (int rc = flush_stream(to_stream(stream), d)) return rc;
  }
  d.on = enable != 0;
  return 0;
}
extern "C" int edet_reduce_flush(void* stream) {
  auto it = defer_map().find(to_stream(stream));
  if (it == defer_map().end() || it->second.items.empty()) return 0;
  return flush_stream(to_stream(stream), it->second);
}
extern "C" int edet_reduce_deferred_end(void* stream, const void** hi_out) {
  EDET_CHECK(hi_out, "edet_reduce_deferred_end: null pointer");
  auto it = defer_map().find(to_stream(stream));
  *hi_out = it == defer_map().end() ? nullptr : it->second.hi;
  return 0;
}

// dst_a[i] += column i (i < n_a; dst_a may be NULL), dst_b[i - n_a] += column i (n_a <= i < n)
int edet_reduce_partials2(const float* ws, int P, int64_t n, float* dst_a, int64_t n_a, float* dst_b, hipStream_t st) {
  return launch_reduce("edet_reduce_partials2", ws, P, n, dst_a, 1, n_a, dst_b, st);
}
// dst[i] += sum of the partial rows; with deferral on for the stream the sum is recorded for the next flush instead
int edet_reduce_partials(const float* ws, int P, int64_t n, float* dst, hipStream_t st) {
  auto it = defer_map().find(st);
  if (it != defer_map().end() && it->second.on && n < (int64_t)1 << 31) {
    DeferState& d = it->second;
    d.items.push_back(RedItem{ws, dst, P, (int)n});
    const unsigned char* end = reinterpret_cast<const unsigned char*>(ws) + (size_t)P * n * sizeof(float);
    if (!d.hi || end > d.hi) d.hi = end;
    return 0;
  }
  return launch_reduce("edet_reduce_partials", ws, P, n, dst, 1, -1, nullptr, st);
}
// dst[i] = sum of the partial rows (no accumulation)
int edet_reduce_partials_set(const float* ws, int P, int64_t n, float* dst, hipStream_t st) {
  return launch_reduce("edet_reduce_partials", ws, P, n, dst, 0, -1, nullptr, st);
}
