// The host stage of the JPEG decoder (include/edet_hip.h, "baseline JPEG decode"): the marker walk and the Huffman decode of
// SOF0 / SOF1 streams into int16 coefficients.  Plain C++17 -- no device call and no device header, so the same file builds
// with a host compiler alone (tests/c_host/jpeg_host_check.cpp runs it under the address and undefined-behaviour sanitizers).
// Everything behind it -- dequantisation, inverse DCT, upsampling, colour -- is csrc/jpeg.hip, and csrc/jpeg_scaled.hip for the
// reduced sizes: edet_jpeg_entropy_decode_scaled differs from edet_jpeg_entropy_decode only in the headers -- a denominator per
// image, the output size in the descriptor -- and shares everything else with it (entropy_decode below).
//
// The statuses, the order in which a file is refused and every stored coefficient are those of tests/jpeg_ref.py (walk,
// check_frame, parse), statement for statement.  Every read of the input goes through a length check, every table index is
// validated before use: a hostile file gives a status.  Arithmetic that a corrupt stream can drive out of range (the DC
// predictor) is unsigned and wraps.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../include/edet_hip.h"
#include "jpeg_entropy_impl.h"

void edet_set_error(const char* fmt, ...);      // error.cpp (the stand-alone checker brings its own)

namespace {

constexpr int MAX_THREADS = 16;
using jpeg_entropy::LOOK_BITS;

const uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct RawHuff {
  bool present = false;
  uint8_t counts[16];
  uint8_t vals[256];
  int total = 0;
};

// what the walk up to SOS leaves: the frame, the tables and where the scan starts
struct Parsed {
  edet_jpeg_info_t info;
  bool have_frame = false;
  bool have_qt[4] = {false, false, false, false};
  uint16_t qt[4][64];
  RawHuff huff[2][4];
  const uint8_t* sos = nullptr;      // the SOS segment behind its length
  size_t sos_len = 0;
  size_t scan = 0;                   // position of the entropy-coded data
};

// jpeg_ref.walk: the markers up to the first SOS -> 0, or EDET_JPEG_MALFORMED
int walk(const uint8_t* d, size_t n, Parsed& P) {
  memset(&P.info, 0, sizeof(P.info));
  memset(P.qt, 0, sizeof(P.qt));
  P.info.adobe_transform = -1;
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return EDET_JPEG_MALFORMED;
  size_t p = 2;
  for (;;) {
    if (p >= n || d[p] != 0xFF) return EDET_JPEG_MALFORMED;
    while (p < n && d[p] == 0xFF) ++p;
    if (p >= n) return EDET_JPEG_MALFORMED;
    const int m = d[p++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9) return EDET_JPEG_MALFORMED;
    if (n - p < 2) return EDET_JPEG_MALFORMED;
    const size_t len = ((size_t)d[p] << 8) | d[p + 1];
    if (len < 2 || len > n - p) return EDET_JPEG_MALFORMED;
    const uint8_t* seg = d + p + 2;
    const size_t sl = len - 2;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      if (P.have_frame || sl < 6) return EDET_JPEG_MALFORMED;
      const int nc = seg[5];
      if (sl != (size_t)6 + 3 * (size_t)nc) return EDET_JPEG_MALFORMED;
      P.have_frame = true;
      P.info.precision = seg[0];
      P.info.height = (seg[1] << 8) | seg[2];
      P.info.width = (seg[3] << 8) | seg[4];
      P.info.components = nc;
      P.info.sof = m;
      P.info.kind = m == 0xC0 ? EDET_JPEG_KIND_BASELINE : m == 0xC1 ? EDET_JPEG_KIND_EXTENDED
                    : m == 0xC2 ? EDET_JPEG_KIND_PROGRESSIVE : EDET_JPEG_KIND_OTHER;
      for (int i = 0; i < nc && i < 4; ++i) {
        P.info.comp_id[i] = seg[6 + 3 * i];
        P.info.h_samp[i] = seg[7 + 3 * i] >> 4;
        P.info.v_samp[i] = seg[7 + 3 * i] & 15;
        P.info.quant_id[i] = seg[8 + 3 * i];
      }
    } else if (m == 0xDB) {
      size_t q = 0;
      while (q < sl) {
        const int pq = seg[q] >> 4, tq = seg[q] & 15;
        const size_t size = pq ? 128 : 64;
        if (pq > 1 || tq > 3 || q + 1 + size > sl) return EDET_JPEG_MALFORMED;
        const uint8_t* v = seg + q + 1;
        for (int i = 0; i < 64; ++i) P.qt[tq][NATURAL[i]] = pq ? (uint16_t)((v[2 * i] << 8) | v[2 * i + 1]) : v[i];
        P.have_qt[tq] = true;
        q += 1 + size;
      }
    } else if (m == 0xC4) {
      size_t q = 0;
      while (q < sl) {
        if (q + 17 > sl) return EDET_JPEG_MALFORMED;
        const int tc = seg[q] >> 4, th = seg[q] & 15;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += seg[q + 1 + i];
        if (tc > 1 || th > 3 || total > 256 || q + 17 + (size_t)total > sl) return EDET_JPEG_MALFORMED;
        RawHuff& H = P.huff[tc][th];
        H.present = true;
        H.total = total;
        memcpy(H.counts, seg + q + 1, 16);
        memcpy(H.vals, seg + q + 17, (size_t)total);
        q += 17 + (size_t)total;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return EDET_JPEG_MALFORMED;
      P.info.restart_interval = (seg[0] << 8) | seg[1];
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(seg, "JFIF\0", 5) == 0) P.info.jfif = 1;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) P.info.adobe_transform = seg[11];
    } else if (m == 0xDA) {
      if (!P.have_frame) return EDET_JPEG_MALFORMED;
      P.sos = seg;
      P.sos_len = sl;
      P.scan = p + len;
      return 0;
    }
    p += len;
  }
}

// the smallest denominator in {1, 2, 4, 8} not above max_denom whose output ceil(height / d) x ceil(width / d) fits the
// canvas, or `forced` if that is not 0; 0: nothing fits
int choose_denom(int height, int width, int canvas_h, int canvas_w, int max_denom, int forced) {
  for (int d = forced ? forced : 1; d <= (forced ? forced : max_denom); d *= 2)
    if ((height + d - 1) / d <= canvas_h && (width + d - 1) / d <= canvas_w) return d;
  return 0;
}

// jpeg_ref.check_frame; *denom: the denominator the image is decoded at (choose_denom)
int check_frame(const edet_jpeg_info_t& f, int canvas_h, int canvas_w, int max_denom, int forced, int* denom) {
  if (f.kind == EDET_JPEG_KIND_PROGRESSIVE) return EDET_JPEG_PROGRESSIVE;
  if (f.kind == EDET_JPEG_KIND_OTHER)
    return (f.sof == 0xC9 || f.sof == 0xCA || f.sof == 0xCB || f.sof == 0xCD || f.sof == 0xCE || f.sof == 0xCF)
               ? EDET_JPEG_ARITHMETIC : EDET_JPEG_UNSUPPORTED;
  if (f.precision != 8) return EDET_JPEG_PRECISION;
  if (f.components != 1 && f.components != 3) return EDET_JPEG_COMPONENTS;
  if (f.components == 3) {
    const bool chroma = f.h_samp[1] == 1 && f.v_samp[1] == 1 && f.h_samp[2] == 1 && f.v_samp[2] == 1;
    const bool luma = (f.h_samp[0] == 1 && f.v_samp[0] == 1) || (f.h_samp[0] == 2 && f.v_samp[0] == 1) ||
                      (f.h_samp[0] == 2 && f.v_samp[0] == 2);
    if (!chroma || !luma) return EDET_JPEG_SAMPLING;
    const bool rgb_ids = f.comp_id[0] == 'R' && f.comp_id[1] == 'G' && f.comp_id[2] == 'B';
    if (f.adobe_transform == 0 || (f.adobe_transform < 0 && !f.jfif && rgb_ids)) return EDET_JPEG_UNSUPPORTED;
  } else if (f.h_samp[0] < 1 || f.h_samp[0] > 4 || f.v_samp[0] < 1 || f.v_samp[0] > 4) {
    return EDET_JPEG_MALFORMED;
  }
  if (f.height < 1 || f.width < 1) return EDET_JPEG_MALFORMED;
  *denom = choose_denom(f.height, f.width, canvas_h, canvas_w, max_denom, forced);
  return *denom ? 0 : EDET_JPEG_TOO_LARGE;
}

// the scan header against the frame (jpeg_ref.parse up to the tables): the Huffman table ids per component
int check_scan(const Parsed& P, int td[3], int ta[3]) {
  const edet_jpeg_info_t& f = P.info;
  const int nc = f.components;
  const uint8_t* s = P.sos;
  if (P.sos_len < 1 || P.sos_len != (size_t)4 + 2 * (size_t)s[0]) return EDET_JPEG_MALFORMED;
  const int ns = s[0];
  for (int i = 0; i < ns; ++i) {
    bool known = false;
    for (int c = 0; c < nc; ++c) known |= s[1 + 2 * i] == f.comp_id[c];
    if (!known) return EDET_JPEG_MALFORMED;
  }
  if (ns != nc) return EDET_JPEG_UNSUPPORTED;
  for (int i = 0; i < nc; ++i)
    if (s[1 + 2 * i] != f.comp_id[i]) return EDET_JPEG_UNSUPPORTED;
  if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return EDET_JPEG_MALFORMED;
  for (int i = 0; i < nc; ++i) {
    td[i] = s[2 + 2 * i] >> 4;
    ta[i] = s[2 + 2 * i] & 15;
    if (td[i] > 3 || ta[i] > 3 || !P.huff[0][td[i]].present || !P.huff[1][ta[i]].present) return EDET_JPEG_MALFORMED;
    if (f.quant_id[i] > 3 || !P.have_qt[f.quant_id[i]]) return EDET_JPEG_MALFORMED;
  }
  return 0;
}

// jdhuff.c's derived table (jpeg_entropy_impl.h has the layout: the device decoder reads the same bytes)
struct Huff : jpeg_entropy::HuffTable {
  bool build(const RawHuff& R, bool is_dc) {
    memset(look, 0, sizeof(look));
    mincode[0] = count[0] = valptr[0] = pad = 0;
    memcpy(vals, R.vals, sizeof(vals));
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      count[len] = R.counts[len - 1];
      mincode[len] = (int32_t)code;
      valptr[len] = k;
      for (int i = 0; i < count[len]; ++i) {
        if (code >= ((uint32_t)1 << len)) return false;      // more codes than the length has
        if (k >= R.total) return false;
        const int sym = R.vals[k];
        if (is_dc && sym > 15) return false;
        if (len <= LOOK_BITS) {
          const uint32_t lo = code << (LOOK_BITS - len);
          for (uint32_t j = 0; j < ((uint32_t)1 << (LOOK_BITS - len)); ++j) look[lo + j] = (uint16_t)((len << 8) | sym);
        }
        ++code;
        ++k;
      }
      code <<= 1;
    }
    return true;
  }
};

// the entropy-coded bytes from `p` up to the next marker, unstuffed on the fly; bits come from the top of `acc`
struct Bits {
  const uint8_t* d;
  size_t n, p;
  uint64_t acc = 0;
  int have = 0;
  bool stopped = false;

  Bits(const uint8_t* data, size_t size, size_t pos) : d(data), n(size), p(pos) {}

  void fill() {
    while (have <= 56 && !stopped) {
      if (p >= n) { stopped = true; break; }
      const uint8_t b = d[p];
      if (b == 0xFF) {
        if (p + 1 < n && d[p + 1] == 0) { p += 2; }
        else { stopped = true; break; }      // a marker or the end: p stays on the 0xFF
      } else {
        ++p;
      }
      acc = (acc << 8) | b;
      have += 8;
    }
  }

  // the next 16 bits, zero-filled past the end
  uint32_t peek16() {
    if (have < 16) fill();
    return have >= 16 ? (uint32_t)(acc >> (have - 16)) & 0xFFFFu : (uint32_t)(acc << (16 - have)) & 0xFFFFu;
  }

  // -> symbol, or -1: no such code, or the code runs past the data
  int symbol(const Huff& H) {
    const uint32_t peek = peek16();
    const uint16_t e = H.look[peek >> (16 - LOOK_BITS)];
    int len = e >> 8, sym = e & 0xFF;
    if (!len) {
      for (int l = LOOK_BITS + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(peek >> (16 - l));
        if (H.count[l] && code >= H.mincode[l] && code - H.mincode[l] < H.count[l]) {
          const int at = H.valptr[l] + (code - H.mincode[l]);
          if (at > 255) return -1;
          len = l;
          sym = H.vals[at];
          break;
        }
      }
      if (!len) return -1;
    }
    if (len > have) return -1;
    have -= len;
    return sym;
  }

  // `s` bits (1 .. 15) as jdhuff.c's HUFF_EXTEND -> value; ok = false when the data ends first
  int receive_extend(int s, bool& ok) {
    if (have < s) fill();
    if (have < s) { ok = false; return 0; }
    const int v = (int)((acc >> (have - s)) & (((uint64_t)1 << s) - 1));
    have -= s;
    return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
  }
};

// the kept MCUs of an image, in MCUs of its full grid: all of them, or what a window needs (kept_grid)
struct Kept {
  int x0, y0, w, h;      // first column and row, columns and rows kept
  int full_w, full_h;    // the file's MCU grid
};

// The scan of one image -> coefficients; 0 or EDET_JPEG_MALFORMED.  im's block grids are those of the KEPT MCUs (the whole
// grid for the full-size and scaled entry points): a block outside them is parsed, since the DC predictors must advance, and
// not stored, and the scan is read no further than the last kept MCU row.
int decode_scan(const uint8_t* d, size_t n, const Parsed& P, const int td[3], const int ta[3], const edet_jpeg_image_t& im,
                const Kept& K, int16_t* coef) {
  const int nc = im.components;
  std::vector<Huff> tables(2 * (size_t)nc);
  for (int c = 0; c < nc; ++c) {
    if (!tables[2 * c].build(P.huff[0][td[c]], true)) return EDET_JPEG_MALFORMED;
    if (!tables[2 * c + 1].build(P.huff[1][ta[c]], false)) return EDET_JPEG_MALFORMED;
  }
  memset(coef + (size_t)64 * im.first_block[0], 0, sizeof(int16_t) * 64 * (size_t)im.total_blocks);
  const int hs[3] = {im.h_max, 1, 1}, vs[3] = {im.v_max, 1, 1};
  const int mcus_w = K.full_w, mcus_h = K.y0 + K.h;      // (<= K.full_h: nothing behind the last kept row is read)
  int16_t skipped[64];      // where a block outside the kept grid goes
  uint32_t pred[3] = {0, 0, 0};
  Bits bits(d, n, P.scan);
  const int ri = P.info.restart_interval;
  int todo = ri, next_rst = 0;
  for (int my = 0; my < mcus_h; ++my) {
    for (int mx = 0; mx < mcus_w; ++mx) {
      if (ri && todo == 0) {
        // the bits left in this interval are padding; the reader stopped on (or in front of) the marker's 0xFF
        bits.fill();
        size_t q = bits.p;
        if (!bits.stopped) {      // a full accumulator: the interval has bytes it never needed; go to the next marker
          while (q < n && !(d[q] == 0xFF && !(q + 1 < n && d[q + 1] == 0))) q += (d[q] == 0xFF) ? 2 : 1;
        }
        if (q >= n || d[q] != 0xFF) return EDET_JPEG_MALFORMED;
        while (q < n && d[q] == 0xFF) ++q;
        if (q >= n || d[q] != 0xD0 + next_rst) return EDET_JPEG_MALFORMED;
        next_rst = (next_rst + 1) & 7;
        bits = Bits(d, n, q + 1);
        pred[0] = pred[1] = pred[2] = 0;
        todo = ri;
      }
      --todo;
      const bool kept = my >= K.y0 && mx >= K.x0 && mx < K.x0 + K.w;
      for (int c = 0; c < nc; ++c) {
        const Huff& dc = tables[2 * c];
        const Huff& ac = tables[2 * c + 1];
        for (int yy = 0; yy < vs[c]; ++yy) {
          for (int xx = 0; xx < hs[c]; ++xx) {
            const size_t at = (size_t)im.first_block[c] + (size_t)((my - K.y0) * vs[c] + yy) * im.blocks_w[c] +
                              ((mx - K.x0) * hs[c] + xx);
            int16_t* blk = kept ? coef + 64 * at : skipped;
            bool ok = true;
            int s = bits.symbol(dc);
            if (s < 0) return EDET_JPEG_MALFORMED;
            if (s) pred[c] += (uint32_t)bits.receive_extend(s, ok);
            if (!ok) return EDET_JPEG_MALFORMED;
            blk[0] = (int16_t)(uint16_t)(pred[c] & 0xFFFFu);
            int k = 1;
            while (k < 64) {
              const int rs = bits.symbol(ac);
              if (rs < 0) return EDET_JPEG_MALFORMED;
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;
                k += 16;
                continue;
              }
              k += r;
              if (k > 63) return EDET_JPEG_MALFORMED;
              blk[NATURAL[k]] = (int16_t)bits.receive_extend(s, ok);
              if (!ok) return EDET_JPEG_MALFORMED;
              ++k;
            }
          }
        }
      }
    }
  }
  return 0;
}

}  // namespace

extern "C" int edet_jpeg_info(const uint8_t* data, size_t n, edet_jpeg_info_t* out) {
  if (!data || !out) {
    edet_set_error("edet_jpeg_info: null pointer");
    return -1;
  }
  Parsed P;
  if (walk(data, n, P) != 0) {
    memset(out, 0, sizeof(*out));
    edet_set_error("edet_jpeg_info: not a JPEG stream with a frame and a scan (%zu bytes)", n);
    return -1;
  }
  *out = P.info;
  return 0;
}

namespace {

// The side of component c's blocks after the inverse transform at 8 / denom = m (jpeg_scaled.hip, sample_size)
int sample_size(int h_max, int v_max, int m, int c) { return (c > 0 && h_max == 2 && v_max == 2 && m < 8) ? 2 * m : m; }

// The kept grid of a window (include/edet_hip.h, "JPEG decode of a crop window"): the smallest rectangle of whole MCUs that
// holds the samples every component needs for output pixels [y, y + h) x [x, x + w) of an out_h x out_w output.
void kept_grid(int components, int h_max, int v_max, int denom, int out_h, int out_w, const int32_t win[4], Kept& K) {
  const int m = 8 / denom, s0 = sample_size(h_max, v_max, m, 0);
  int lo[2] = {INT32_MAX, INT32_MAX}, hi[2] = {-1, -1};      // MCU columns, MCU rows
  for (int c = 0; c < components; ++c) {
    const int s = sample_size(h_max, v_max, m, c);
    for (int a = 0; a < 2; ++a) {      // 0: along x, 1: along y
      const int samp = a == 0 ? h_max : v_max;
      const int u = c == 0 ? 1 : samp * s0 / s;      // the up-sampling that is left, 1 or 2
      const int per_mcu = c == 0 ? samp : 1;         // blocks of the component in an MCU
      const int first = a == 0 ? win[1] : win[0], last = first + (a == 0 ? win[3] : win[2]) - 1;
      const int real = ((a == 0 ? out_w : out_h) + u - 1) / u;
      int from = first, to = last;
      if (u == 2) {
        from = (first >> 1) - 1 > 0 ? (first >> 1) - 1 : 0;
        to = (last >> 1) + 1 < real - 1 ? (last >> 1) + 1 : real - 1;
      }
      from = from / s / per_mcu;
      to = to / s / per_mcu;
      if (from < lo[a]) lo[a] = from;
      if (to > hi[a]) hi[a] = to;
    }
  }
  K.x0 = lo[0];
  K.w = hi[0] - lo[0] + 1;
  K.y0 = lo[1];
  K.h = hi[1] - lo[1] + 1;
}

struct Job {
  Parsed P;
  int td[3], ta[3];
  Kept K;
};

// the arguments every entry point checks; -> the worker threads to use, or -1 (the error is set)
int check_args(const char* who, bool pointers, int batch, int max_denom, const int32_t* denoms, int threads) {
  if (!pointers || batch < 1) {
    edet_set_error("%s: null pointer or batch %d < 1", who, batch);
    return -1;
  }
  if (max_denom != 1 && max_denom != 2 && max_denom != 4 && max_denom != 8) {
    edet_set_error("%s: max_denom %d is not 1, 2, 4 or 8", who, max_denom);
    return -1;
  }
  for (int b = 0; denoms && b < batch; ++b) {
    if (denoms[b] != 1 && denoms[b] != 2 && denoms[b] != 4 && denoms[b] != 8) {
      edet_set_error("%s: denoms[%d] = %d is not 1, 2, 4 or 8", who, b, (int)denoms[b]);
      return -1;
    }
  }
  if (threads <= 0) threads = batch < MAX_THREADS ? batch : MAX_THREADS;
  if (threads > MAX_THREADS) threads = MAX_THREADS;
  if (threads > batch) threads = batch;
  return threads;
}

// The headers of a batch, one image after the other: the place of an image in the arena depends on the images in front of
// it.  Writes every descriptor, table and status; jobs[b] is what the scan of image b needs.
void headers(const uint8_t* const* datas, const size_t* sizes, int batch, int canvas_h, int canvas_w, int max_denom,
             const int32_t* denoms, bool scaled, const int32_t* windows, edet_jpeg_window_t* wins, size_t coef_capacity,
             edet_jpeg_image_t* images_host, uint16_t* qtables_host, int32_t* status, std::vector<Job>& jobs) {
  size_t next_block = 0;
  const size_t cap_blocks = coef_capacity / 64;
  for (int b = 0; b < batch; ++b) {
    Job& J = jobs[(size_t)b];
    edet_jpeg_image_t& im = images_host[b];
    memset(&im, 0, sizeof(im));
    memset(qtables_host + (size_t)b * 256, 0, 256 * sizeof(uint16_t));
    int st = walk(datas[b], sizes[b], J.P);
    int denom = 1;
    if (windows) {      // the window has to fit the canvas, not the image; its coordinates are those of ONE denominator
      memset(&wins[b], 0, sizeof(wins[b]));
      if (!st) st = check_frame(J.P.info, INT32_MAX, INT32_MAX, max_denom, denoms ? (int)denoms[b] : 1, &denom);
    } else if (!st) {
      st = check_frame(J.P.info, canvas_h, canvas_w, max_denom, denoms ? (int)denoms[b] : 0, &denom);
    }
    if (!st) st = check_scan(J.P, J.td, J.ta);
    if (!st && windows) {
      const edet_jpeg_info_t& f = J.P.info;
      const int32_t* w = windows + 4 * (size_t)b;
      const int out_h = (f.height + denom - 1) / denom, out_w = (f.width + denom - 1) / denom;
      if (w[0] < 0 || w[1] < 0 || w[2] < 1 || w[3] < 1 || w[2] > out_h - w[0] || w[3] > out_w - w[1]) st = EDET_JPEG_WINDOW;
      else if (w[2] > canvas_h || w[3] > canvas_w) st = EDET_JPEG_TOO_LARGE;
    }
    if (!st) {
      const edet_jpeg_info_t& f = J.P.info;
      im.height = (f.height + denom - 1) / denom;      // the output size; the block grids below are the file's
      im.width = (f.width + denom - 1) / denom;
      im.reserved = scaled ? denom : 0;
      im.components = f.components;
      im.h_max = f.components == 3 ? f.h_samp[0] : 1;
      im.v_max = f.components == 3 ? f.v_samp[0] : 1;
      const int mw = (f.width + 8 * im.h_max - 1) / (8 * im.h_max), mh = (f.height + 8 * im.v_max - 1) / (8 * im.v_max);
      Kept& K = J.K;
      K.x0 = K.y0 = 0;
      K.w = K.full_w = mw;
      K.h = K.full_h = mh;
      edet_jpeg_window_t win;
      memset(&win, 0, sizeof(win));
      if (windows) {
        // The image descriptor describes the kept MCUs as an image of their own -- their block grids, and for height and
        // width their output pixels inside the image -- so edet_jpeg_idct_scaled runs on it as it is.
        const int32_t* w = windows + 4 * (size_t)b;
        kept_grid(f.components, im.h_max, im.v_max, denom, im.height, im.width, w, K);
        const int m = 8 / denom;
        const int px = im.h_max * sample_size(im.h_max, im.v_max, m, 0), py = im.v_max * sample_size(im.h_max, im.v_max, m, 0);
        win.y = w[0]; win.x = w[1]; win.h = w[2]; win.w = w[3];
        win.image_h = im.height; win.image_w = im.width;
        win.mcu_x0 = K.x0; win.mcu_y0 = K.y0; win.mcus_w = K.w; win.mcus_h = K.h;
        const int right = (K.x0 + K.w) * px < im.width ? (K.x0 + K.w) * px : im.width;
        const int bottom = (K.y0 + K.h) * py < im.height ? (K.y0 + K.h) * py : im.height;
        im.width = right - K.x0 * px;
        im.height = bottom - K.y0 * py;
      }
      size_t total = 0;
      for (int c = 0; c < f.components; ++c) {
        im.blocks_w[c] = c == 0 ? K.w * im.h_max : K.w;
        im.blocks_h[c] = c == 0 ? K.h * im.v_max : K.h;
        im.quant_id[c] = f.quant_id[c];
        total += (size_t)im.blocks_w[c] * (size_t)im.blocks_h[c];      // <= 3 * 8192 * 8192
      }
      if (total > cap_blocks || next_block > cap_blocks - total || next_block + total > (size_t)INT32_MAX) {
        st = EDET_JPEG_TOO_LARGE;
      } else {
        size_t at = next_block;
        for (int c = 0; c < f.components; ++c) {
          im.first_block[c] = (int32_t)at;
          at += (size_t)im.blocks_w[c] * (size_t)im.blocks_h[c];
        }
        im.total_blocks = (int32_t)total;
        next_block += total;
        memcpy(qtables_host + (size_t)b * 256, J.P.qt, sizeof(J.P.qt));
        if (windows) wins[b] = win;
      }
    }
    if (st) {
      memset(&im, 0, sizeof(im));
    }
    im.status = st;
    status[b] = st;
  }
}

// `work` on `threads` threads, the caller's among them
template <class F>
void run_parallel(int threads, F& work) {
  if (threads == 1) {
    work();
    return;
  }
  std::vector<std::thread> pool;
  pool.reserve((size_t)threads - 1);
  for (int t = 1; t < threads; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
}

// The three host entry points: the headers, then the scans.  windows / wins NULL: the whole grid of every image is kept.
// max_denom 1 and denoms NULL is the full-size decode; `scaled` says whether the descriptor carries the denominator (the
// full-size entry point keeps writing 0 there).
int entropy_decode(const char* who, const uint8_t* const* datas, const size_t* sizes, int batch, int canvas_h, int canvas_w,
                   int max_denom, const int32_t* denoms, bool scaled, const int32_t* windows, edet_jpeg_window_t* wins,
                   int16_t* coef_host, size_t coef_capacity, edet_jpeg_image_t* images_host, uint16_t* qtables_host,
                   int32_t* status, int threads) {
  threads = check_args(who, datas && sizes && coef_host && images_host && qtables_host && status, batch, max_denom, denoms,
                       threads);
  if (threads < 0) return -1;
  std::vector<Job> jobs((size_t)batch);
  headers(datas, sizes, batch, canvas_h, canvas_w, max_denom, denoms, scaled, windows, wins, coef_capacity, images_host,
          qtables_host, status, jobs);

  // the scans, in parallel: an image refused here keeps its place in the arena, unused
  std::atomic<int> next(0);
  auto work = [&]() {
    for (;;) {
      const int b = next.fetch_add(1);
      if (b >= batch) return;
      edet_jpeg_image_t& im = images_host[b];
      if (im.status) continue;
      const Job& J = jobs[(size_t)b];
      const int st = decode_scan(datas[b], sizes[b], J.P, J.td, J.ta, im, J.K, coef_host);
      if (st) {
        memset(&im, 0, sizeof(im));
        if (windows) memset(&wins[b], 0, sizeof(wins[b]));
        memset(qtables_host + (size_t)b * 256, 0, 256 * sizeof(uint16_t));
        im.status = st;
        status[b] = st;
      }
    }
  };
  run_parallel(threads, work);
  return 0;
}

// The scan of one image for the device decoder: its entropy-coded bytes, FF 00 stuffing removed, into arena[at, at + room),
// one segment per restart interval, each at a 4-byte aligned offset and zero-padded to a whole word.  Segments end where
// Bits::fill stops and the markers between them are checked as decode_scan checks them; nothing behind the last segment is
// looked at.  -> 0, EDET_JPEG_MALFORMED (a restart marker missing or out of sequence) or EDET_JPEG_TOO_LARGE (no room).
int copy_scan(const uint8_t* d, size_t n, size_t q, int nseg, uint8_t* arena, size_t at, size_t room,
              edet_jpeg_segment_t* segs) {
  const size_t end = at + room;
  for (int j = 0; j < nseg; ++j) {
    const size_t first = at;
    for (;;) {
      const uint8_t* ff = q < n ? (const uint8_t*)memchr(d + q, 0xFF, n - q) : nullptr;
      const size_t run = (ff ? (size_t)(ff - d) : n) - q;
      if (run > end - at) return EDET_JPEG_TOO_LARGE;
      memcpy(arena + at, d + q, run);
      at += run;
      q += run;
      if (!ff || !(q + 1 < n && d[q + 1] == 0)) break;      // the end of the data, or a marker: q stays on its 0xFF
      if (at >= end) return EDET_JPEG_TOO_LARGE;
      arena[at++] = 0xFF;
      q += 2;
    }
    const size_t length = at - first;
    if (length >= ((size_t)1 << 28) || first > (size_t)UINT32_MAX) return EDET_JPEG_TOO_LARGE;      // (bit positions are 32-bit)
    while (at & 3) {
      if (at >= end) return EDET_JPEG_TOO_LARGE;
      arena[at++] = 0;
    }
    segs[j].offset = (uint32_t)first;
    segs[j].length = (uint32_t)length;
    segs[j].first_unit = 0;      // (the caller's, once every length is known)
    segs[j].reserved = 0;
    if (j + 1 < nseg) {
      if (q >= n || d[q] != 0xFF) return EDET_JPEG_MALFORMED;
      while (q < n && d[q] == 0xFF) ++q;
      if (q >= n || d[q] != 0xD0 + (j & 7)) return EDET_JPEG_MALFORMED;
      ++q;
    }
  }
  return 0;
}

}  // namespace

extern "C" int edet_jpeg_scan_prepare(const uint8_t* const* datas, const size_t* sizes, int batch, int canvas_h, int canvas_w,
                                      int max_denom, const int32_t* denoms, size_t coef_capacity, int subseq_bits,
                                      uint8_t* scan_host, size_t scan_capacity, edet_jpeg_segment_t* segments_host,
                                      size_t segment_capacity, size_t unit_capacity, uint8_t* tables_host,
                                      edet_jpeg_scan_t* scans_host, edet_jpeg_image_t* images_host, uint16_t* qtables_host,
                                      int32_t* status, size_t* used, int threads) {
  const char* who = "edet_jpeg_scan_prepare";
  threads = check_args(who, datas && sizes && scan_host && segments_host && tables_host && scans_host && images_host &&
                                qtables_host && status && used, batch, max_denom, denoms, threads);
  if (threads < 0) return -1;
  if (subseq_bits < 64 || subseq_bits > 8192 || subseq_bits % 32 != 0 || ((uintptr_t)scan_host & 3) != 0) {
    edet_set_error("%s: subseq_bits %d is not a multiple of 32 in 64 .. 8192, or scan_host is not 4-byte aligned", who, subseq_bits);
    return -1;
  }
  std::vector<Job> jobs((size_t)batch);
  // (max_denom 1 without denoms: edet_jpeg_entropy_decode's descriptors; otherwise edet_jpeg_entropy_decode_scaled's)
  headers(datas, sizes, batch, canvas_h, canvas_w, max_denom, denoms, max_denom != 1 || denoms, nullptr, nullptr, coef_capacity,
          images_host, qtables_host, status, jobs);
  auto refuse = [&](int b, int st) {
    memset(&images_host[b], 0, sizeof(images_host[b]));
    memset(&scans_host[b], 0, sizeof(scans_host[b]));
    memset(qtables_host + (size_t)b * 256, 0, 256 * sizeof(uint16_t));
    images_host[b].status = st;
    status[b] = st;
  };
  // the tables, and each image's room in the arenas: what is left of the file behind SOS bounds its scan, so the place of an
  // image does not wait for the walk over the image in front of it
  memset(tables_host, 0, (size_t)batch * EDET_JPEG_TABLES * EDET_JPEG_TABLE_BYTES);
  std::vector<size_t> scan_at((size_t)batch), scan_room((size_t)batch);
  size_t next_byte = 0, next_seg = 0;
  for (int b = 0; b < batch; ++b) {
    edet_jpeg_image_t& im = images_host[b];
    edet_jpeg_scan_t& sc = scans_host[b];
    memset(&sc, 0, sizeof(sc));
    if (im.status) continue;
    const Job& J = jobs[(size_t)b];
    const int nc = im.components;
    Huff* tables = reinterpret_cast<Huff*>(tables_host + (size_t)b * EDET_JPEG_TABLES * EDET_JPEG_TABLE_BYTES);
    int slots = 0, cls_of[EDET_JPEG_TABLES], id_of[EDET_JPEG_TABLES];
    bool built = true;
    for (int c = 0; c < nc && built; ++c) {
      for (int cls = 0; cls < 2 && built; ++cls) {      // 0: DC, 1: AC; components that name one table share its slot
        const int id = cls ? J.ta[c] : J.td[c];
        int s = 0;
        while (s < slots && !(cls_of[s] == cls && id_of[s] == id)) ++s;
        if (s == slots) {
          built = tables[s].build(J.P.huff[cls][id], cls == 0);
          cls_of[s] = cls;
          id_of[s] = id;
          ++slots;
        }
        (cls ? sc.ac_table : sc.dc_table)[c] = s;
      }
    }
    if (!built) {
      memset(tables, 0, (size_t)EDET_JPEG_TABLES * EDET_JPEG_TABLE_BYTES);
      refuse(b, EDET_JPEG_MALFORMED);
      continue;
    }
    const int64_t mcus = (int64_t)J.K.full_w * J.K.full_h;
    const int ri = J.P.info.restart_interval;
    const int64_t nseg = ri ? (mcus + ri - 1) / ri : 1;
    const size_t room = ((sizes[b] - J.P.scan) + 4 * (size_t)nseg + 15) & ~(size_t)15;
    if ((size_t)nseg > segment_capacity - next_seg || next_seg > segment_capacity || room > scan_capacity - next_byte ||
        next_byte > scan_capacity || next_byte + room > (size_t)INT32_MAX) {
      memset(tables, 0, (size_t)EDET_JPEG_TABLES * EDET_JPEG_TABLE_BYTES);
      refuse(b, EDET_JPEG_TOO_LARGE);
      continue;
    }
    sc.first_segment = (int32_t)next_seg;
    sc.segments = (int32_t)nseg;
    sc.restart_interval = ri;
    sc.mcus_w = J.K.full_w;
    sc.mcus_h = J.K.full_h;
    sc.blocks_per_mcu = im.h_max * im.v_max + (nc == 3 ? 2 : 0);
    scan_at[(size_t)b] = next_byte;
    scan_room[(size_t)b] = room;
    next_byte += room;
    next_seg += (size_t)nseg;
  }
  // the scans, in parallel
  std::atomic<int> next(0);
  std::vector<int> scan_status((size_t)batch, 0);
  auto work = [&]() {
    for (;;) {
      const int b = next.fetch_add(1);
      if (b >= batch) return;
      if (images_host[b].status) continue;
      const edet_jpeg_scan_t& sc = scans_host[b];
      scan_status[(size_t)b] = copy_scan(datas[b], sizes[b], jobs[(size_t)b].P.scan, sc.segments, scan_host, scan_at[(size_t)b],
                                         scan_room[(size_t)b], segments_host + sc.first_segment);
    }
  };
  run_parallel(threads, work);
  // the units, which need every length
  size_t next_unit = 0;
  for (int b = 0; b < batch; ++b) {
    edet_jpeg_scan_t& sc = scans_host[b];
    if (images_host[b].status) continue;
    int st = scan_status[(size_t)b];
    size_t units = 0;
    for (int j = 0; !st && j < sc.segments; ++j) {
      edet_jpeg_segment_t& sg = segments_host[sc.first_segment + j];
      sg.first_unit = (uint32_t)units;
      units += jpeg_entropy::units_of(8 * sg.length, (uint32_t)subseq_bits);
    }
    if (!st && (units > unit_capacity - next_unit || next_unit + units > (size_t)INT32_MAX)) st = EDET_JPEG_TOO_LARGE;
    if (st) {
      memset(tables_host + (size_t)b * EDET_JPEG_TABLES * EDET_JPEG_TABLE_BYTES, 0, (size_t)EDET_JPEG_TABLES * EDET_JPEG_TABLE_BYTES);
      refuse(b, st);
      continue;
    }
    sc.first_unit = (int32_t)next_unit;
    sc.units = (int32_t)units;
    next_unit += units;
  }
  used[0] = next_byte;
  used[1] = next_seg;
  used[2] = next_unit;
  return 0;
}

extern "C" int edet_jpeg_entropy_decode(const uint8_t* const* datas, const size_t* sizes, int batch, int canvas_h,
                                        int canvas_w, int16_t* coef_host, size_t coef_capacity,
                                        edet_jpeg_image_t* images_host, uint16_t* qtables_host, int32_t* status,
                                        int threads) {
  return entropy_decode("edet_jpeg_entropy_decode", datas, sizes, batch, canvas_h, canvas_w, 1, nullptr, false, nullptr,
                        nullptr, coef_host, coef_capacity, images_host, qtables_host, status, threads);
}

extern "C" int edet_jpeg_entropy_decode_scaled(const uint8_t* const* datas, const size_t* sizes, int batch, int canvas_h,
                                               int canvas_w, int max_denom, const int32_t* denoms, int16_t* coef_host,
                                               size_t coef_capacity, edet_jpeg_image_t* images_host,
                                               uint16_t* qtables_host, int32_t* status, int threads) {
  return entropy_decode("edet_jpeg_entropy_decode_scaled", datas, sizes, batch, canvas_h, canvas_w, max_denom, denoms, true,
                        nullptr, nullptr, coef_host, coef_capacity, images_host, qtables_host, status, threads);
}

extern "C" int edet_jpeg_entropy_decode_window(const uint8_t* const* datas, const size_t* sizes, int batch, int canvas_h,
                                               int canvas_w, int max_denom, const int32_t* denoms, const int32_t* windows,
                                               int16_t* coef_host, size_t coef_capacity, edet_jpeg_image_t* images_host,
                                               edet_jpeg_window_t* windows_host, uint16_t* qtables_host, int32_t* status,
                                               int threads) {
  if (!windows || !windows_host) {
    edet_set_error("edet_jpeg_entropy_decode_window: null windows");
    return -1;
  }
  return entropy_decode("edet_jpeg_entropy_decode_window", datas, sizes, batch, canvas_h, canvas_w, max_denom, denoms, true,
                        windows, windows_host, coef_host, coef_capacity, images_host, qtables_host, status, threads);
}
