// What the host and the device share of the parallel Huffman decoder (include/edet_hip.h, "JPEG Huffman decode on the
// device"): the derived table, the bit reader over an unstuffed segment, decode_unit and the scan-order -> arena-slot mapping.
// One text for both: csrc/jpeg_host.cpp builds the tables with it, csrc/jpeg_entropy.hip runs it per thread, and
// tests/c_host/jpeg_entropy_host_check.cpp compiles it with a host compiler alone and emulates a workgroup with it under the
// sanitizers.  No device header, no allocation, no global state.
//
// A segment is the entropy-coded data of one restart interval with the FF 00 stuffing removed, stored at a 4-byte aligned
// offset of the scan arena; bit position p counts from its first bit, most significant bit of a byte first.  Reading past its
// last bit gives zeros, as Bits::peek16 of the host stage does, and a symbol that needs such bits is an error, as there.
#pragma once
#include <stdint.h>

#include "../../include/edet_hip.h"

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define JPEG_HD inline
#endif

namespace jpeg_entropy {

constexpr int LOOK_BITS = 10;

// jdhuff.c's derived table: a look-up for codes of up to LOOK_BITS bits, the canonical ranges for longer ones.  EDET_JPEG_TABLE_BYTES
// each; an image has EDET_JPEG_TABLES of them, and its components name theirs by slot.
struct HuffTable {
  uint16_t look[1 << LOOK_BITS];      // (length << 8) | symbol, 0 = no code of <= LOOK_BITS bits starts like this
  int32_t mincode[17], count[17], valptr[17];
  uint8_t vals[256];
  int32_t pad;
};
static_assert(sizeof(HuffTable) == EDET_JPEG_TABLE_BYTES, "edet_hip.h: EDET_JPEG_TABLE_BYTES");

// zigzag position -> natural (row-major) position
JPEG_HD int natural(int k) {
  static constexpr uint8_t N[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return N[k & 63];
}

// the decoder's state at a bit position: bk = (block inside the MCU << 8) | zigzag position, 0 = a DC symbol is next
struct State {
  uint32_t p, bk;
};
JPEG_HD bool same(const State& a, const State& b) { return a.p == b.p && a.bk == b.bk; }

// one segment: `words` 32-bit words hold its `bits` bits (bits <= 32 words), big-endian within a word
struct Segment {
  const uint32_t* data;
  uint32_t words, bits;
};

// what decode_unit needs of the image: blocks per MCU, how many of them are luma, the table slots per component
struct Mcu {
  int blocks, luma;
  int dc[3], ac[3];      // 0 .. EDET_JPEG_TABLES - 1
};

// bits p .. p + 31 of the segment, zeros behind its last bit
JPEG_HD uint32_t window32(const Segment& s, uint32_t p) {
  if (p >= s.bits) return 0;
  const uint32_t w = p >> 5, sh = p & 31;
  const uint32_t hi = w < s.words ? __builtin_bswap32(s.data[w]) : 0;
  const uint32_t lo = w + 1 < s.words ? __builtin_bswap32(s.data[w + 1]) : 0;
  uint32_t v = sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
  const uint32_t left = s.bits - p;
  if (left < 32) v &= ~(uint32_t)0 << (32 - left);
  return v;
}

// Bits::symbol of the host stage on the 16 bits `peek`: -> (length << 8) | symbol, or 0: no such code.  Every index is
// checked, so a table nobody validated gives "no such code", never a read outside it.
JPEG_HD uint32_t lookup(const HuffTable& H, uint32_t peek) {
  const uint32_t e = H.look[(peek >> (16 - LOOK_BITS)) & ((1u << LOOK_BITS) - 1)];
  if (e >> 8) return (e >> 8) <= (uint32_t)LOOK_BITS ? e : 0;
  for (int l = LOOK_BITS + 1; l <= 16; ++l) {
    const int32_t code = (int32_t)(peek >> (16 - l));
    if (H.count[l] > 0 && code >= H.mincode[l] && code - H.mincode[l] < H.count[l]) {
      const int64_t at = (int64_t)H.valptr[l] + (code - H.mincode[l]);
      if (at < 0 || at > 255) return 0;
      return ((uint32_t)l << 8) | H.vals[at];
    }
  }
  return 0;
}

// jdhuff.c's HUFF_EXTEND of the s bits (1 .. 15) v
JPEG_HD int extend(uint32_t v, int s) { return v >= (1u << (s - 1)) ? (int)v : (int)v - (1 << s) + 1; }

struct NoSink {
  JPEG_HD void dc(uint32_t, int) {}
  JPEG_HD void ac(uint32_t, int, int) {}
};

// Decodes whole symbols (a code and its extra bits) from state `st` until p >= end (end <= seg.bits); -> the blocks completed,
// `st` the end state.  sink.dc(n, difference) and sink.ac(n, zigzag position, value) receive what is decoded, n counting the
// blocks this call completed before.  An absent code, a code or extra bits that run past the segment, a DC symbol above 15 or
// a run that lands behind position 63 with a value stops the unit: st = (seg.bits, 0, 0), error = true.  Every symbol consumes
// at least one bit, so the loop runs at most end - st.p times.
template <class Sink>
JPEG_HD uint32_t decode_unit(const Segment& seg, uint32_t end, const HuffTable* tables, const Mcu& m, State& st, bool& error,
                             Sink& sink) {
  uint32_t p = st.p, n = 0;
  int b = (int)(st.bk >> 8), k = (int)(st.bk & 0xFF);
  error = false;
  if (end > seg.bits) end = seg.bits;
  if (b >= m.blocks || k > 63) {      // (not a state this function leaves)
    b = 0;
    k = 0;
  }
  while (p < end) {
    const int c = b < m.luma ? 0 : b - m.luma + 1;
    const uint32_t w = window32(seg, p), left = seg.bits - p;
    // (selects, not m.dc[c]: an index the compiler cannot resolve would put the struct into scratch memory on the device)
    const int slot = k == 0 ? (c == 0 ? m.dc[0] : c == 1 ? m.dc[1] : m.dc[2]) : (c == 0 ? m.ac[0] : c == 1 ? m.ac[1] : m.ac[2]);
    const uint32_t e = lookup(tables[slot], w >> 16);
    const uint32_t len = e >> 8;
    const int sym = (int)(e & 0xFF), s = sym & 15;
    bool bad = len == 0 || len + (uint32_t)s > left, done = false;
    if (!bad) {
      const int v = s ? extend((w << len) >> (32 - s), s) : 0;
      if (k == 0) {
        bad = sym > 15;
        if (!bad) sink.dc(n, v);
        k = 1;
      } else if (s == 0) {
        if ((sym >> 4) != 15) done = true;
        else k += 16;
      } else {
        k += sym >> 4;
        bad = k > 63;
        if (!bad) sink.ac(n, k, v);
        ++k;
      }
    }
    if (bad) {
      st.p = seg.bits;
      st.bk = 0;
      error = true;
      return n;
    }
    p += len + (uint32_t)s;
    if (done || k > 63) {
      ++n;
      k = 0;
      b = b + 1 == m.blocks ? 0 : b + 1;
    }
  }
  st.p = p;
  st.bk = ((uint32_t)b << 8) | (uint32_t)k;
  return n;
}

// Block `scan_block` of the image in scan order -> its block in the arenas: MCU by MCU, per MCU the components in order, per
// component its blocks row by row (decode_scan's expression).  mcus_w > 0; the caller keeps scan_block below total_blocks.
JPEG_HD int64_t block_slot(const edet_jpeg_image_t& d, int mcus_w, const Mcu& m, uint32_t scan_block) {
  const uint32_t mcu = scan_block / (uint32_t)m.blocks, bi = scan_block - mcu * (uint32_t)m.blocks;
  const uint32_t my = mcu / (uint32_t)mcus_w, mx = mcu - my * (uint32_t)mcus_w;
  if ((int)bi < m.luma) {
    const uint32_t yy = bi / (uint32_t)d.h_max, xx = bi - yy * (uint32_t)d.h_max;
    return (int64_t)d.first_block[0] + (int64_t)(my * (uint32_t)d.v_max + yy) * d.blocks_w[0] + (mx * (uint32_t)d.h_max + xx);
  }
  const bool cb = (int)bi == m.luma;
  return (int64_t)(cb ? d.first_block[1] : d.first_block[2]) + (int64_t)my * (cb ? d.blocks_w[1] : d.blocks_w[2]) + mx;
}

// the units of a segment of `bits` bits
JPEG_HD uint32_t units_of(uint32_t bits, uint32_t subseq_bits) { return bits / subseq_bits + (bits % subseq_bits ? 1 : 0); }

}  // namespace jpeg_entropy
