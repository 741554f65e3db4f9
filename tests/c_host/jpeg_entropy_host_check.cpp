// Stand-alone checker of the device entropy decoder's host half and of the code its kernel runs per unit
// (automl_amd/csrc/jpeg_host.cpp: edet_jpeg_scan_prepare; automl_amd/csrc/jpeg_entropy_impl.h), built by
// tests/test_jpeg_entropy.py with the host compiler under the address and undefined-behaviour sanitizers and run as a child
// process.  No device, nothing loaded into an interpreter.
//
//   jpeg_entropy_host_check DIR
//
// DIR/list.txt has one line per stream: "<file> <expected status, or -1 for any> <1 = also mutate it>".  Every stream goes
// through edet_jpeg_entropy_decode (the yardstick) and through edet_jpeg_scan_prepare plus a sequential emulation of the
// workgroup of csrc/jpeg_entropy.hip -- round 0, the rounds, the prefix sum, the write pass, the DC sums, in the kernel's order
// with its threads run one after the other -- at subseq_bits 64, 128 and 1024.  Where the host stage returns 0 the emulation
// must return 0, the same descriptor and tables and identical coefficients; where it returns a status the emulation must
// return a non-zero status.  Of a stream marked for mutation every prefix and 300 copies with one byte changed (fixed seed)
// go through the same comparison at 64 and 1024 bits.  Exit 0 = all of that held and no sanitizer report ended the run.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <vector>

#include "../../automl_amd/csrc/jpeg_entropy_impl.h"
#include "../../include/edet_hip.h"

void edet_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  va_end(ap);
}

namespace {

using namespace jpeg_entropy;

constexpr int CANVAS = 1024;
constexpr size_t CAPACITY = (size_t)64 * 12 * (CANVAS / 16) * (CANVAS / 16);      // one worst-case image
constexpr int THREADS = 7;      // of the emulated workgroup: few, so that every thread walks several units

struct Unit {
  State start, end;
  uint32_t count, seg, base;
  bool dirty;
};

struct Sink {
  int16_t* coef;
  uint16_t* dc_diff;
  const edet_jpeg_image_t* d;
  const Mcu* m;
  int mcus_w;
  uint32_t first, share, base;
  void dc(uint32_t n, int v) {
    const uint32_t i = base + n;
    if (i < share) dc_diff[first + i] = (uint16_t)v;
  }
  void ac(uint32_t n, int k, int v) {
    const uint32_t i = base + n;
    if (i < share) coef[64 * block_slot(*d, mcus_w, *m, first + i) + natural(k)] = (int16_t)v;
  }
};

// what edet_jpeg_scan_prepare wrote for ONE image, in exactly sized copies: a read outside them is a read outside an allocation
struct Prepared {
  std::vector<uint32_t> scan;      // (words: the decoder reads aligned words)
  std::vector<edet_jpeg_segment_t> segs;
  std::vector<HuffTable> tables;
  edet_jpeg_scan_t sc;
  edet_jpeg_image_t im;
  std::vector<uint16_t> qt;
  int status;
};

int prepare(const std::vector<uint8_t>& stream, int subseq, size_t coef_capacity, Prepared& P, size_t scan_capacity = SIZE_MAX,
            size_t segment_capacity = 4096, size_t unit_capacity = (size_t)1 << 24) {
  const uint8_t* ptr = stream.data();
  const size_t size = stream.size();
  if (scan_capacity == SIZE_MAX) scan_capacity = size + 4096 * 4 + 64;
  std::vector<uint32_t> arena(scan_capacity / 4 + 1);
  std::vector<edet_jpeg_segment_t> segs(segment_capacity + 1);      // (never a null pointer)
  P.tables.assign(EDET_JPEG_TABLES, HuffTable());
  P.qt.assign(256, 0);
  size_t used[3] = {0, 0, 0};
  int32_t status = -1;
  const int rc = edet_jpeg_scan_prepare(&ptr, &size, 1, CANVAS, CANVAS, 1, nullptr, coef_capacity, subseq,
                                        reinterpret_cast<uint8_t*>(arena.data()), scan_capacity, segs.data(), segment_capacity,
                                        unit_capacity, reinterpret_cast<uint8_t*>(P.tables.data()), &P.sc, &P.im, P.qt.data(),
                                        &status, used, 1);
  P.status = status;
  if (rc != 0) return rc;
  if (used[0] % 4 != 0 || used[0] > scan_capacity || used[1] > segment_capacity || used[2] > unit_capacity) return -3;
  P.scan.assign(arena.begin(), arena.begin() + used[0] / 4);
  P.segs.assign(segs.begin(), segs.begin() + used[1]);
  if (!status && ((size_t)P.sc.segments != used[1] || (size_t)P.sc.units != used[2] || P.sc.first_segment != 0 ||
                  P.sc.first_unit != 0))
    return -4;
  return 0;
}

Segment segment_of(const Prepared& P, uint32_t j) {
  const edet_jpeg_segment_t& sg = P.segs[j];
  Segment s;
  s.data = P.scan.data() + sg.offset / 4;
  s.words = (sg.length + 3) / 4;
  s.bits = 8 * sg.length;
  return s;
}

// the workgroup of k_jpeg_entropy on one image, its threads one after the other -> 0 or EDET_JPEG_MALFORMED; *rounds
int emulate(const Prepared& P, uint32_t subseq, std::vector<int16_t>& coef, int* rounds) {
  const edet_jpeg_image_t& d = P.im;
  const edet_jpeg_scan_t& s = P.sc;
  Mcu m;
  m.luma = d.h_max * d.v_max;
  m.blocks = s.blocks_per_mcu;
  for (int c = 0; c < 3; ++c) {
    m.dc[c] = c < d.components ? s.dc_table[c] : 0;
    m.ac[c] = c < d.components ? s.ac_table[c] : 0;
  }
  const uint32_t nunits = (uint32_t)s.units, nseg = (uint32_t)s.segments, total = (uint32_t)d.total_blocks;
  const int ri = s.restart_interval;
  const uint32_t mcus = (uint32_t)s.mcus_w * (uint32_t)s.mcus_h;
  if (total != mcus * (uint32_t)m.blocks || nseg != (ri ? (mcus + ri - 1) / ri : 1)) return -1;
  std::fill(coef.begin() + (size_t)64 * d.first_block[0], coef.begin() + (size_t)64 * (d.first_block[0] + total), (int16_t)0);
  for (uint32_t j = 0; j < nseg; ++j) {
    const uint32_t next_fu = j + 1 < nseg ? P.segs[j + 1].first_unit : nunits;
    if ((P.segs[j].offset & 3) || P.segs[j].first_unit > next_fu || units_of(8 * P.segs[j].length, subseq) != next_fu - P.segs[j].first_unit)
      return -1;
  }
  std::vector<Unit> U(nunits);
  std::vector<uint16_t> dc(total, 0xDCDC);
  const HuffTable* tabs = P.tables.data();
  NoSink none;
  bool err;
  for (int tid = 0; tid < THREADS; ++tid) {
    for (uint32_t u = tid; u < nunits; u += THREADS) {
      uint32_t lo = 0, hi = nseg;
      while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (P.segs[mid].first_unit <= u) lo = mid;
        else hi = mid;
      }
      const Segment sg = segment_of(P, lo);
      Unit& W = U[u];
      W.start.p = (u - P.segs[lo].first_unit) * subseq;
      W.start.bk = 0;
      W.end = W.start;
      W.count = decode_unit(sg, W.start.p + subseq, tabs, m, W.end, err, none);
      W.seg = lo;
      W.dirty = false;
    }
  }
  *rounds = 1;
  for (uint32_t r = 1; r <= nunits; ++r) {
    bool any = false;
    for (int tid = 0; tid < THREADS; ++tid) {
      for (uint32_t u = tid; u < nunits; u += THREADS) {
        Unit& W = U[u];
        if (u == 0 || P.segs[W.seg].first_unit == u) continue;
        if (!same(U[u - 1].end, W.start)) {
          W.start = U[u - 1].end;
          W.dirty = true;
          any = true;
        }
      }
    }
    if (!any) break;
    *rounds = (int)r + 1;
    for (int tid = 0; tid < THREADS; ++tid) {
      for (uint32_t u = tid; u < nunits; u += THREADS) {
        Unit& W = U[u];
        if (!W.dirty) continue;
        W.end = W.start;
        W.count = decode_unit(segment_of(P, W.seg), (u - P.segs[W.seg].first_unit) * subseq + subseq, tabs, m, W.end, err, none);
        W.dirty = false;
      }
    }
  }
  uint32_t run = 0;
  for (uint32_t u = 0; u < nunits; ++u) {
    U[u].base = run;
    run += U[u].count;
  }
  const uint32_t seg_blocks = ri ? (uint32_t)std::min<int64_t>((int64_t)ri * m.blocks, total) : total;
  for (uint32_t j = 0; j < nseg; ++j) {
    const uint32_t fu = P.segs[j].first_unit, next_fu = j + 1 < nseg ? P.segs[j + 1].first_unit : nunits;
    const uint32_t done = next_fu > fu ? U[next_fu - 1].base + U[next_fu - 1].count - U[fu].base : 0;
    if (done < std::min(seg_blocks, total - j * seg_blocks)) return EDET_JPEG_MALFORMED;
  }
  for (uint32_t u = 0; u < nunits; ++u) {
    const Unit& W = U[u];
    Sink sink;
    sink.coef = coef.data();
    sink.dc_diff = dc.data();
    sink.d = &d;
    sink.m = &m;
    sink.mcus_w = s.mcus_w;
    sink.first = W.seg * seg_blocks;
    sink.share = std::min(seg_blocks, total - W.seg * seg_blocks);
    sink.base = W.base - U[P.segs[W.seg].first_unit].base;
    State st = W.start;
    (void)decode_unit(segment_of(P, W.seg), (u - P.segs[W.seg].first_unit) * subseq + subseq, tabs, m, st, err, sink);
  }
  // the DC sums, in the kernel's three steps
  const uint32_t mper = (mcus + THREADS - 1) / THREADS;
  uint32_t part[THREADS][4], carry[THREADS + 1][3];
  for (int pass = 0; pass < 2; ++pass) {
    for (int tid = 0; tid < THREADS; ++tid) {
      const uint32_t m0 = std::min((uint32_t)tid * mper, mcus), m1 = std::min(m0 + mper, mcus);
      uint32_t sum[3] = {0, 0, 0};
      if (pass) memcpy(sum, carry[tid], sizeof(sum));
      bool reset = false;
      for (uint32_t mc = m0; mc < m1; ++mc) {
        if (ri && mc % (uint32_t)ri == 0) {
          sum[0] = sum[1] = sum[2] = 0;
          reset = true;
        }
        for (int bi = 0; bi < m.blocks; ++bi) {
          const uint32_t at = mc * (uint32_t)m.blocks + bi;
          uint32_t& p = sum[bi < m.luma ? 0 : bi == m.luma ? 1 : 2];
          p += (uint32_t)(int32_t)(int16_t)dc[at];
          if (pass) coef[64 * block_slot(d, s.mcus_w, m, at)] = (int16_t)(uint16_t)(p & 0xFFFFu);
        }
      }
      if (!pass) {
        memcpy(part[tid], sum, sizeof(sum));
        part[tid][3] = reset;
      }
    }
    if (!pass) {
      carry[0][0] = carry[0][1] = carry[0][2] = 0;
      for (int t = 0; t < THREADS; ++t)
        for (int c = 0; c < 3; ++c) carry[t + 1][c] = (part[t][3] ? 0 : carry[t][c]) + part[t][c];
    }
  }
  return 0;
}

struct Tally {
  int bad = 0;
  long runs = 0, accepted = 0, most_rounds = 0;
};

// one stream at one subsequence size against the host stage
void compare(const std::vector<uint8_t>& stream, int subseq, int expect, Tally& t, const char* what, size_t index) {
  const uint8_t* ptr = stream.data();
  const size_t size = stream.size();
  static std::vector<int16_t> want(CAPACITY, 0x5A5A), got(CAPACITY, 0x5A5A);      // (filled again below, where they were used)
  edet_jpeg_image_t im;
  std::vector<uint16_t> qt(256);
  int32_t st = -1;
  if (edet_jpeg_entropy_decode(&ptr, &size, 1, CANVAS, CANVAS, want.data(), want.size(), &im, qt.data(), &st, 1) != 0) ++t.bad;
  Prepared P;
  const int rc = prepare(stream, subseq, CAPACITY, P);
  int mine = P.status, rounds = 0;
  if (rc == 0 && mine == 0) mine = emulate(P, (uint32_t)subseq, got, &rounds);
  ++t.runs;
  t.accepted += st == 0;
  if (rounds > t.most_rounds) t.most_rounds = rounds;
  bool ok = rc == 0 && mine >= 0 && mine <= EDET_JPEG_UNSUPPORTED && (expect < 0 || st == expect);
  if (st == 0) {
    ok = ok && mine == 0 && memcmp(&im, &P.im, sizeof(im)) == 0 && memcmp(qt.data(), P.qt.data(), 512) == 0 && want == got;
  } else {
    ok = ok && mine != 0;
    if (mine == P.status && P.status != 0) ok = ok && memcmp(&im, &P.im, sizeof(im)) == 0;      // refused on the host: the same row
  }
  const size_t dirty = std::min(CAPACITY, (size_t)64 * (size_t)std::max(im.total_blocks, P.im.total_blocks));
  std::fill(want.begin(), want.begin() + dirty, (int16_t)0x5A5A);
  std::fill(got.begin(), got.begin() + dirty, (int16_t)0x5A5A);
  if (!ok) {
    fprintf(stderr, "%s %zu at %d bits: host stage %d, prepare rc %d status %d, emulation %d\n", what, index, subseq, (int)st, rc,
            P.status, mine);
    ++t.bad;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: jpeg_entropy_host_check DIR\n");
    return 2;
  }
  const std::string dir = argv[1];
  std::ifstream list(dir + "/list.txt");
  std::vector<std::vector<uint8_t>> streams;
  std::vector<int> expect, mutate;
  std::string name;
  int want, mut;
  while (list >> name >> want >> mut) {
    std::ifstream f(dir + "/" + name, std::ios::binary);
    if (!f) {
      fprintf(stderr, "cannot read %s\n", name.c_str());
      return 2;
    }
    streams.emplace_back((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    expect.push_back(want);
    mutate.push_back(mut);
  }
  if (streams.empty()) {
    fprintf(stderr, "no streams\n");
    return 2;
  }
  Tally t;
  for (size_t i = 0; i < streams.size(); ++i)
    for (int subseq : {64, 128, 1024}) compare(streams[i], subseq, expect[i], t, "stream", i);
  // an arena too small for the scan, the segments or the units is TOO_LARGE, decided on the host
  for (size_t i = 0; i < streams.size(); ++i) {
    Prepared P;
    if (prepare(streams[i], 64, CAPACITY, P) != 0 || P.status != 0) continue;
    const size_t bytes = P.scan.size() * 4;
    Prepared Q;
    bool ok = prepare(streams[i], 64, CAPACITY, Q, bytes - 16) == 0 && Q.status == EDET_JPEG_TOO_LARGE;
    ok = ok && prepare(streams[i], 64, CAPACITY, Q, SIZE_MAX, (size_t)P.sc.segments - 1) == 0 && Q.status == EDET_JPEG_TOO_LARGE;
    if (!ok) {
      fprintf(stderr, "stream %zu: an arena too small gives status %d\n", i, Q.status);
      ++t.bad;
    }
    if (P.sc.units > 0 && (prepare(streams[i], 64, CAPACITY, Q, SIZE_MAX, 4096, (size_t)P.sc.units - 1) != 0 || Q.status != EDET_JPEG_TOO_LARGE)) ++t.bad;
    if (prepare(streams[i], 64, CAPACITY, Q, SIZE_MAX, 4096, (size_t)P.sc.units) != 0 || Q.status != 0) ++t.bad;
  }
  // prefixes and single-byte changes
  uint32_t seed = 0x2545F491u;
  auto rnd = [&seed]() {
    seed ^= seed << 13;
    seed ^= seed >> 17;
    seed ^= seed << 5;
    return seed;
  };
  for (size_t i = 0; i < streams.size(); ++i) {
    if (!mutate[i]) continue;
    const std::vector<uint8_t>& s = streams[i];
    for (size_t n = 0; n < s.size(); ++n) {
      std::vector<uint8_t> cut(s.begin(), s.begin() + n);      // exactly sized: a read past the prefix is a read past an allocation
      for (int subseq : {64, 1024}) compare(cut, subseq, -1, t, "prefix", n);
    }
    for (int k = 0; k < 300; ++k) {
      std::vector<uint8_t> mutated(s);
      mutated[rnd() % mutated.size()] = (uint8_t)rnd();
      for (int subseq : {64, 1024}) compare(mutated, subseq, -1, t, "change", (size_t)k);
    }
  }
  printf("%zu streams, %ld runs (%ld decoded by the host stage), at most %ld rounds, %d failures\n", streams.size(), t.runs,
         t.accepted, t.most_rounds, t.bad);
  return t.bad ? 1 : 0;
}
