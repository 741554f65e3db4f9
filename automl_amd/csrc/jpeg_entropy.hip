// The Huffman stage of the JPEG decoder on the device (include/edet_hip.h, "JPEG Huffman decode on the device"): the scan
// arena edet_jpeg_scan_prepare leaves -> the int16 coefficient arena edet_jpeg_idct[_scaled] read, bit for bit what the host
// stage (csrc/jpeg_host.cpp, decode_scan) writes.  Integer arithmetic only.  Restated in tests/jpeg_entropy_ref.py; the
// per-unit code is csrc/jpeg_entropy_impl.h, the text the host checker runs too.
//
// k_jpeg_entropy: ONE workgroup per image, so every wait below is a workgroup barrier and no thread ever waits on memory
// another workgroup writes.  Threads walk the image's units with a stride of the workgroup.  The image's Huffman tables live
// in LDS, the unit states in the unit scratch (global memory that only this workgroup touches; the barriers order it).
//   1. check the descriptors, load the tables, zero the image's coefficients, check the segment rows;
//   2. round 0: every unit decodes from (unit start, 0, 0);
//   3. rounds: a unit whose predecessor's end state differs from the start it last used adopts it (all reads, then a vote
//      that is also the barrier) and decodes again (all writes, barrier) -- at most `units` rounds, since round r settles
//      unit r of every segment at the latest;
//   4. each thread sums the block counts of a contiguous run of units, thread 0 scans the 256 sums, each thread writes its
//      units' exclusive prefix; a segment that completed fewer blocks than its share refuses the image;
//   5. every unit decodes once more from its settled start and writes AC values and DC differences;
//   6. the DC predictors: each thread sums the differences of a contiguous run of MCUs per component (reset where a segment
//      starts), thread 0 chains the 256 sums, each thread walks its run again and stores the low 16 bits.
// Loop bounds: decode_unit consumes a bit per symbol (at most subseq_bits + 31 symbols); the segment search halves a range of
// at most 2^31; everything else counts units, segments, MCUs, blocks or table words of the image, all read once from the
// descriptors and checked against the capacities passed by value.
#include "common.h"
#include "jpeg_impl.h"
#include "jpeg_entropy_impl.h"

namespace {

using namespace jpeg_entropy;

constexpr int THREADS = 256;
constexpr int UW = EDET_JPEG_UNIT_WORDS;
constexpr int TABLE_VECS = EDET_JPEG_TABLES * EDET_JPEG_TABLE_BYTES / 16;
enum { U_START_P, U_START_BK, U_END_P, U_END_BK, U_COUNT, U_SEG, U_DIRTY, U_BASE };

// Is any thread's v set?  Also a workgroup barrier.  flags: three LDS words, zero at first; `turn` counts the calls (the
// same in every thread).  The word of call n + 1 is cleared in front of call n's barrier: its last readers passed the barrier
// of call n - 1, its next writers wait behind this one.
__device__ __forceinline__ bool workgroup_any(bool v, uint32_t* flags, int& turn) {
  const int cur = turn % 3;
  turn = turn == 2 ? 0 : turn + 1;
  if (threadIdx.x == 0) flags[turn] = 0;
  if (v) flags[cur] = 1;
  __syncthreads();
  return flags[cur] != 0;
}

// segment row `j` of the table as the decoder reads it; a row that does not lie inside the arena has no bits
__device__ __forceinline__ Segment load_segment(const uint8_t* __restrict__ scan, uint64_t scan_bytes,
                                                const edet_jpeg_segment_t* __restrict__ segs, int64_t j, uint32_t* first_unit) {
  const edet_jpeg_segment_t sg = segs[j];
  const uint64_t words = ((uint64_t)sg.length + 3) >> 2;
  const bool ok = (sg.offset & 3) == 0 && sg.length < (1u << 28) && (uint64_t)sg.offset + 4 * words <= scan_bytes;
  Segment s;
  s.data = reinterpret_cast<const uint32_t*>(scan + (ok ? sg.offset : 0));
  s.words = ok ? (uint32_t)words : 0;
  s.bits = ok ? 8 * sg.length : 0;
  *first_unit = sg.first_unit;
  return s;
}

struct WriteSink {
  int16_t* coef;
  uint16_t* dc_diff;      // at the image's first block, in scan order
  const edet_jpeg_image_t* d;
  const Mcu* m;
  int mcus_w;
  uint32_t first, share, base;      // the segment's first block in scan order, its share, its blocks completed before this unit
  __device__ __forceinline__ void dc(uint32_t n, int v) {
    const uint32_t i = base + n;
    if (i < share) dc_diff[first + i] = (uint16_t)v;
  }
  __device__ __forceinline__ void ac(uint32_t n, int k, int v) {
    const uint32_t i = base + n;
    if (i < share) coef[64 * block_slot(*d, mcus_w, *m, first + i) + natural(k)] = (int16_t)v;
  }
};

__global__ __launch_bounds__(THREADS) void k_jpeg_entropy(const uint8_t* __restrict__ scan, uint64_t scan_bytes,
                                                          const edet_jpeg_segment_t* __restrict__ segs, int64_t segment_count,
                                                          const uint8_t* __restrict__ tables, edet_jpeg_scan_t* scans,
                                                          edet_jpeg_image_t* images, uint32_t subseq, uint32_t* units,
                                                          int64_t unit_capacity, uint16_t* dc, int16_t* coef,
                                                          int64_t cap_blocks, int32_t* status) {
  __shared__ uint4 table_raw[TABLE_VECS];
  __shared__ uint32_t part[THREADS][4];
  __shared__ uint32_t carry[THREADS + 1][3];
  __shared__ uint32_t flags[3];
  const int img = blockIdx.x, tid = threadIdx.x;
  const edet_jpeg_image_t d = images[img];
  const edet_jpeg_scan_t s = scans[img];
  Mcu m;
  m.luma = d.h_max * d.v_max;
  m.blocks = s.blocks_per_mcu;
  bool ok = jpeg_impl::image_ok(d, cap_blocks);
  const int64_t mcus = (int64_t)s.mcus_w * s.mcus_h;
  const int ri = s.restart_interval;
  if (ok) {
    ok = m.blocks == m.luma + (d.components == 3 ? 2 : 0) && s.mcus_w >= 1 && s.mcus_h >= 1 &&
         d.blocks_w[0] == s.mcus_w * d.h_max && d.blocks_h[0] == s.mcus_h * d.v_max;
    for (int c = 0; c < 3; ++c) {
      const bool live = c < d.components;
      if (live && c > 0) ok = ok && d.blocks_w[c] == s.mcus_w && d.blocks_h[c] == s.mcus_h;
      if (live) ok = ok && s.dc_table[c] >= 0 && s.dc_table[c] < EDET_JPEG_TABLES && s.ac_table[c] >= 0 && s.ac_table[c] < EDET_JPEG_TABLES;
      m.dc[c] = live && ok ? s.dc_table[c] : 0;
      m.ac[c] = live && ok ? s.ac_table[c] : 0;
    }
    ok = ok && ri >= 0 && s.segments >= 1 && (int64_t)s.segments == (ri ? (mcus + ri - 1) / ri : 1) && s.first_segment >= 0 &&
         (int64_t)s.first_segment + s.segments <= segment_count && s.first_unit >= 0 && s.units >= 0 &&
         (int64_t)s.first_unit + s.units <= unit_capacity;
  }
  if (!ok) {      // (the same in every thread) refused by the host, or a descriptor the host could not have written
    if (tid == 0) {
      const int st = d.status ? d.status : EDET_JPEG_MALFORMED;
      status[img] = st;
      if (!d.status) images[img].status = st;
      if (!d.status) scans[img].status = st;
    }
    return;
  }
  if (tid < 3) flags[tid] = 0;
  int turn = 0;
  const uint32_t nunits = (uint32_t)s.units, nseg = (uint32_t)s.segments;
  const uint32_t total = (uint32_t)d.total_blocks;      // == mcus * m.blocks (image_ok and the grids above)
  const edet_jpeg_segment_t* my_segs = segs + s.first_segment;
  uint32_t* U = units + (size_t)s.first_unit * UW;
  uint16_t* my_dc = dc + d.first_block[0];

  // 1. tables, zeros, segment rows
  {
    const uint4* src = reinterpret_cast<const uint4*>(tables + (size_t)img * EDET_JPEG_TABLES * EDET_JPEG_TABLE_BYTES);
    for (int i = tid; i < TABLE_VECS; i += THREADS) table_raw[i] = src[i];
    uint4* z = reinterpret_cast<uint4*>(coef + (size_t)64 * d.first_block[0]);
    for (int64_t i = tid; i < (int64_t)total * 8; i += THREADS) z[i] = make_uint4(0, 0, 0, 0);
  }
  bool bad = false;
  for (uint32_t j = tid; j < nseg; j += THREADS) {      // the rows partition the image's units, in order
    uint32_t fu, next_fu = nunits;
    const Segment sg = load_segment(scan, scan_bytes, my_segs, j, &fu);
    if (j + 1 < nseg) next_fu = my_segs[j + 1].first_unit;
    bad = bad || (my_segs[j].length != 0 && sg.bits == 0) || (j == 0 && fu != 0) || fu > next_fu || next_fu > nunits ||
          units_of(sg.bits, subseq) != next_fu - fu;
  }
  __syncthreads();      // (flags are zero)
  if (workgroup_any(bad, flags, turn)) {
    if (tid == 0) {
      status[img] = EDET_JPEG_MALFORMED;
      images[img].status = EDET_JPEG_MALFORMED;
      scans[img].status = EDET_JPEG_MALFORMED;
    }
    return;
  }
  const HuffTable* tabs = reinterpret_cast<const HuffTable*>(table_raw);
  NoSink none;

  // 2. round 0
  for (uint32_t u = tid; u < nunits; u += THREADS) {
    uint32_t lo = 0, hi = nseg;      // the last row whose first unit is <= u (rows without units share the next row's)
    for (int step = 0; step < 32 && hi - lo > 1; ++step) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (my_segs[mid].first_unit <= u) lo = mid;
      else hi = mid;
    }
    uint32_t fu;
    const Segment sg = load_segment(scan, scan_bytes, my_segs, lo, &fu);
    State st;
    st.p = (u - fu) * subseq;
    st.bk = 0;
    uint32_t* W = U + (size_t)u * UW;
    W[U_START_P] = st.p;
    W[U_START_BK] = 0;
    bool err;
    const uint32_t end = st.p + subseq;
    W[U_COUNT] = decode_unit(sg, end, tabs, m, st, err, none);
    W[U_END_P] = st.p;
    W[U_END_BK] = st.bk;
    W[U_SEG] = lo;
    W[U_DIRTY] = 0;
  }
  __syncthreads();

  // 3. rounds
  uint32_t rounds = 1;
  for (uint32_t r = 1; r <= nunits; ++r) {
    bool any = false;
    for (uint32_t u = tid; u < nunits; u += THREADS) {
      uint32_t* W = U + (size_t)u * UW;
      if (u == 0 || my_segs[W[U_SEG]].first_unit == u) continue;      // a segment's first unit started from the truth
      const uint32_t* P = W - UW;
      if (P[U_END_P] != W[U_START_P] || P[U_END_BK] != W[U_START_BK]) {
        W[U_START_P] = P[U_END_P];
        W[U_START_BK] = P[U_END_BK];
        W[U_DIRTY] = 1;
        any = true;
      }
    }
    if (!workgroup_any(any, flags, turn)) break;
    rounds = r + 1;
    for (uint32_t u = tid; u < nunits; u += THREADS) {
      uint32_t* W = U + (size_t)u * UW;
      if (!W[U_DIRTY]) continue;
      uint32_t fu;
      const Segment sg = load_segment(scan, scan_bytes, my_segs, W[U_SEG], &fu);
      State st;
      st.p = W[U_START_P];
      st.bk = W[U_START_BK];
      bool err;
      W[U_COUNT] = decode_unit(sg, (u - fu) * subseq + subseq, tabs, m, st, err, none);
      W[U_END_P] = st.p;
      W[U_END_BK] = st.bk;
      W[U_DIRTY] = 0;
    }
    __syncthreads();
  }

  // 4. each unit's first block: an exclusive prefix sum of the counts over the image's units
  const uint32_t per = (nunits + THREADS - 1) / THREADS;
  const uint32_t u0 = min((uint32_t)tid * per, nunits), u1 = min(u0 + per, nunits);
  {
    uint32_t sum = 0;
    for (uint32_t u = u0; u < u1; ++u) sum += U[(size_t)u * UW + U_COUNT];
    part[tid][0] = sum;
    __syncthreads();
    if (tid == 0) {
      uint32_t run = 0;
      for (int t = 0; t < THREADS; ++t) {
        const uint32_t v = part[t][0];
        part[t][0] = run;
        run += v;
      }
    }
    __syncthreads();
    sum = part[tid][0];
    for (uint32_t u = u0; u < u1; ++u) {
      U[(size_t)u * UW + U_BASE] = sum;
      sum += U[(size_t)u * UW + U_COUNT];
    }
    __syncthreads();
  }
  const uint32_t seg_blocks = ri ? (uint32_t)min((int64_t)ri * m.blocks, (int64_t)total) : total;      // of all but the last
  bad = false;
  for (uint32_t j = tid; j < nseg; j += THREADS) {
    const uint32_t fu = my_segs[j].first_unit, next_fu = j + 1 < nseg ? my_segs[j + 1].first_unit : nunits;
    const uint32_t done = next_fu > fu ? U[(size_t)(next_fu - 1) * UW + U_BASE] + U[(size_t)(next_fu - 1) * UW + U_COUNT] -
                                             U[(size_t)fu * UW + U_BASE] : 0;
    const uint32_t share = min(seg_blocks, total - j * seg_blocks);      // (j seg_blocks < total: segments = ceil(mcus / ri))
    bad = bad || done < share;
  }
  if (workgroup_any(bad, flags, turn)) {
    if (tid == 0) {
      status[img] = EDET_JPEG_MALFORMED;
      images[img].status = EDET_JPEG_MALFORMED;
      scans[img].status = EDET_JPEG_MALFORMED;
      scans[img].rounds = (int32_t)rounds;
    }
    return;
  }

  // 5. the values
  for (uint32_t u = tid; u < nunits; u += THREADS) {
    const uint32_t* W = U + (size_t)u * UW;
    const uint32_t j = W[U_SEG];
    uint32_t fu;
    const Segment sg = load_segment(scan, scan_bytes, my_segs, j, &fu);
    WriteSink sink;
    sink.coef = coef;
    sink.dc_diff = my_dc;
    sink.d = &d;
    sink.m = &m;
    sink.mcus_w = s.mcus_w;
    sink.first = j * seg_blocks;
    sink.share = min(seg_blocks, total - j * seg_blocks);
    sink.base = W[U_BASE] - U[(size_t)fu * UW + U_BASE];
    State st;
    st.p = W[U_START_P];
    st.bk = W[U_START_BK];
    bool err;
    (void)decode_unit(sg, (u - fu) * subseq + subseq, tabs, m, st, err, sink);
  }
  __syncthreads();

  // 6. the DC predictors, per component in scan order, reset where a segment starts
  {
    const uint32_t nm = (uint32_t)mcus, mper = (nm + THREADS - 1) / THREADS;
    const uint32_t m0 = min((uint32_t)tid * mper, nm), m1 = min(m0 + mper, nm);
    uint32_t sum[3] = {0, 0, 0};
    bool reset = false;
    for (uint32_t mc = m0; mc < m1; ++mc) {
      if (ri && mc % (uint32_t)ri == 0) {
        sum[0] = sum[1] = sum[2] = 0;
        reset = true;
      }
      for (int bi = 0; bi < m.blocks; ++bi) {
        const uint32_t v = (uint32_t)(int32_t)(int16_t)my_dc[mc * (uint32_t)m.blocks + bi];
        if (bi < m.luma) sum[0] += v;
        else if (bi == m.luma) sum[1] += v;
        else sum[2] += v;
      }
    }
    part[tid][0] = sum[0];
    part[tid][1] = sum[1];
    part[tid][2] = sum[2];
    part[tid][3] = reset;
    __syncthreads();
    if (tid == 0) {
      carry[0][0] = carry[0][1] = carry[0][2] = 0;
      for (int t = 0; t < THREADS; ++t)
        for (int c = 0; c < 3; ++c) carry[t + 1][c] = (part[t][3] ? 0 : carry[t][c]) + part[t][c];
    }
    __syncthreads();
    uint32_t pred[3] = {carry[tid][0], carry[tid][1], carry[tid][2]};
    for (uint32_t mc = m0; mc < m1; ++mc) {
      if (ri && mc % (uint32_t)ri == 0) pred[0] = pred[1] = pred[2] = 0;
      for (int bi = 0; bi < m.blocks; ++bi) {
        const uint32_t at = mc * (uint32_t)m.blocks + bi;
        const uint32_t v = (uint32_t)(int32_t)(int16_t)my_dc[at];
        uint32_t& p = bi < m.luma ? pred[0] : bi == m.luma ? pred[1] : pred[2];
        p += v;
        coef[64 * block_slot(d, s.mcus_w, m, at)] = (int16_t)(uint16_t)(p & 0xFFFFu);
      }
    }
  }
  if (tid == 0) {
    status[img] = 0;
    scans[img].rounds = (int32_t)rounds;
  }
}

}  // namespace

extern "C" int edet_jpeg_entropy_device(const uint8_t* scan_dev, size_t scan_bytes, const edet_jpeg_segment_t* segments_dev,
                                        size_t segment_count, const uint8_t* tables_dev, edet_jpeg_scan_t* scans_dev,
                                        edet_jpeg_image_t* images_dev, int batch, int subseq_bits, uint32_t* units_dev,
                                        size_t unit_capacity, uint16_t* dc_dev, int16_t* coef, size_t coef_capacity,
                                        int32_t* status_dev, void* stream) {
  EDET_CHECK(scan_dev && segments_dev && tables_dev && scans_dev && images_dev && units_dev && dc_dev && coef && status_dev,
             "edet_jpeg_entropy_device: null pointer");
  EDET_CHECK(batch >= 1 && batch <= 65535, "edet_jpeg_entropy_device: batch %d (1..65535)", batch);
  EDET_CHECK(subseq_bits >= 64 && subseq_bits <= 8192 && subseq_bits % 32 == 0,
             "edet_jpeg_entropy_device: subseq_bits %d is not a multiple of 32 in 64 .. 8192", subseq_bits);
  EDET_CHECK(scan_bytes < ((size_t)1 << 31) && segment_count < ((size_t)1 << 31) && unit_capacity < ((size_t)1 << 31) &&
                 coef_capacity / 64 < ((size_t)1 << 31),
             "edet_jpeg_entropy_device: an arena of 2^31 or more bytes, segments, units or blocks");
  EDET_CHECK(((uintptr_t)coef & 15) == 0 && ((uintptr_t)tables_dev & 15) == 0 && ((uintptr_t)scan_dev & 3) == 0 &&
                 ((uintptr_t)units_dev & 3) == 0 && ((uintptr_t)dc_dev & 1) == 0,
             "edet_jpeg_entropy_device: coef and tables must be 16-byte aligned, scan and units 4-byte aligned");
  edet_launch(k_jpeg_entropy, dim3((unsigned)batch), dim3(THREADS), 0, to_stream(stream), scan_dev, (uint64_t)scan_bytes,
              segments_dev, (int64_t)segment_count, tables_dev, scans_dev, images_dev, (uint32_t)subseq_bits, units_dev,
              (int64_t)unit_capacity, dc_dev, coef, (int64_t)(coef_capacity / 64), status_dev);
  EDET_LAUNCH_CHECK("edet_jpeg_entropy_device");
  return 0;
}
