// Stand-alone checker of the window entry point of the JPEG host stage (automl_amd/csrc/jpeg_host.cpp and nothing else),
// built by tests/test_jpeg_window.py with the host compiler under the address and undefined-behaviour sanitizers and run as a
// child process.
//
//   jpeg_window_host_check FILE [FILE ...]
//
// Each FILE is one small decodable stream.  Through edet_jpeg_entropy_decode_window it is decoded with a sweep of windows at
// every denominator -- valid ones, whose whole-image case must give the coefficients of edet_jpeg_entropy_decode, and invalid
// ones (negative, empty, past the image, larger than the canvas), which must give EDET_JPEG_WINDOW or EDET_JPEG_TOO_LARGE --
// into an arena sized exactly for the kept blocks, so a block stored outside the kept grid is a write past an allocation;
// then every prefix of the stream and 300 copies with one byte changed (fixed seed) are decoded with a window.  Every answer
// must be a status and a pair of descriptors that fit the arena and the canvas.  The arguments the call refuses must fail it.
// Exit 0 = all of that held and no sanitizer report ended the run.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/edet_hip.h"

void edet_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  va_end(ap);
}

namespace {

struct Answer {
  edet_jpeg_image_t image;
  edet_jpeg_window_t window;
  std::vector<uint16_t> qt;
  int32_t status = -1;
  Answer() : qt(256) {}
};

int decode(const std::vector<uint8_t>& s, int canvas_h, int canvas_w, int max_denom, const int32_t* denoms,
           const int32_t* window, std::vector<int16_t>& coef, Answer& a) {
  const uint8_t* p = s.data();
  const size_t n = s.size();
  return edet_jpeg_entropy_decode_window(&p, &n, 1, canvas_h, canvas_w, max_denom, denoms, window, coef.data(), coef.size(),
                                         &a.image, &a.window, a.qt.data(), &a.status, 1);
}

// what every answer of the stage has to satisfy
bool sound(const Answer& a, const int32_t* w, int canvas_h, int canvas_w, size_t capacity) {
  if (a.status < EDET_JPEG_OK || a.status > EDET_JPEG_WINDOW || a.status != a.image.status) return false;
  if (a.status)
    return a.image.height == 0 && a.image.total_blocks == 0 && a.image.reserved == 0 && a.window.h == 0 && a.window.w == 0 &&
           a.window.mcus_w == 0 && a.window.image_h == 0;
  const int d = a.image.reserved;
  if (!(d == 1 || d == 2 || d == 4 || d == 8)) return false;
  if (a.window.y != w[0] || a.window.x != w[1] || a.window.h != w[2] || a.window.w != w[3]) return false;
  if (w[0] < 0 || w[1] < 0 || w[2] < 1 || w[3] < 1 || w[0] + w[2] > a.window.image_h || w[1] + w[3] > a.window.image_w) return false;
  if (w[2] > canvas_h || w[3] > canvas_w) return false;
  if (a.window.mcus_w < 1 || a.window.mcus_h < 1 || a.window.mcu_x0 < 0 || a.window.mcu_y0 < 0) return false;
  if (a.image.blocks_w[0] != a.window.mcus_w * a.image.h_max || a.image.blocks_h[0] != a.window.mcus_h * a.image.v_max) return false;
  return a.image.height >= 1 && a.image.width >= 1 && a.image.total_blocks >= 1 &&
         (size_t)(a.image.first_block[0] + a.image.total_blocks) * 64 <= capacity;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: jpeg_window_host_check FILE [FILE ...]\n");
    return 2;
  }
  int bad = 0;
  long runs = 0, accepted = 0, windows = 0, refused = 0;
  for (int arg = 1; arg < argc; ++arg) {
    std::ifstream f(argv[arg], std::ios::binary);
    if (!f) {
      fprintf(stderr, "cannot read %s\n", argv[arg]);
      return 2;
    }
    const std::vector<uint8_t> s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    // the full-size stage: the size and the coefficients to compare with
    std::vector<int16_t> full((size_t)64 * 4096);
    Answer fa;
    {
      const uint8_t* p = s.data();
      const size_t n = s.size();
      if (edet_jpeg_entropy_decode(&p, &n, 1, 4096, 4096, full.data(), full.size(), &fa.image, fa.qt.data(), &fa.status, 1) != 0 ||
          fa.status != 0) {
        fprintf(stderr, "%s is not decoded at full size: status %d\n", argv[arg], fa.status);
        return 2;
      }
    }
    const int h = fa.image.height, w = fa.image.width;
    const size_t used = (size_t)64 * fa.image.total_blocks;
    std::vector<int16_t> roomy(used);
    Answer a;
    for (int d = 1; d <= 8; d *= 2) {
      const int oh = (h + d - 1) / d, ow = (w + d - 1) / d;
      const int32_t forced = d;
      // the whole image: the full-size stage's coefficients
      const int32_t whole[4] = {0, 0, oh, ow};
      if (decode(s, oh, ow, 8, &forced, whole, roomy, a) != 0 || a.status != 0 || !sound(a, whole, oh, ow, used) ||
          (size_t)64 * a.image.total_blocks != used || memcmp(roomy.data(), full.data(), used * sizeof(int16_t)) != 0 ||
          memcmp(a.qt.data(), fa.qt.data(), 256 * sizeof(uint16_t)) != 0 || a.image.height != oh || a.image.width != ow) {
        fprintf(stderr, "denominator %d: the whole-image window differs from the full-size stage\n", d);
        ++bad;
      }
      // a sweep of windows, invalid ones among them; each valid one a second time into an arena of exactly its kept blocks
      const int ys[] = {-1, 0, 1, oh / 2, oh - 1, oh}, hs[] = {0, 1, 2, oh / 2 + 1, oh, oh + 1};
      const int xs[] = {-1, 0, 1, 7, ow / 2, ow - 1, ow}, ws[] = {-3, 1, 2, 9, ow, ow + 1};
      for (int y : ys) for (int wh : hs) for (int x : xs) for (int ww : ws) {
        const int32_t win[4] = {y, x, wh, ww};
        const int ch = oh > 2 ? oh - 1 : oh, cw = ow;      // a canvas one row short of the image where that is possible
        const bool inside = y >= 0 && x >= 0 && wh >= 1 && ww >= 1 && y + wh <= oh && x + ww <= ow;
        if (decode(s, ch, cw, 8, &forced, win, roomy, a) != 0 || !sound(a, win, ch, cw, used)) ++bad;
        ++windows;
        const int want = !inside ? EDET_JPEG_WINDOW : (wh > ch || ww > cw) ? EDET_JPEG_TOO_LARGE : EDET_JPEG_OK;
        if (a.status != want) {
          fprintf(stderr, "denominator %d window (%d, %d, %d, %d): status %d, not %d\n", d, y, x, wh, ww, a.status, want);
          ++bad;
        }
        refused += a.status != 0;
        if (a.status == 0) {
          std::vector<int16_t> exact((size_t)64 * a.image.total_blocks);
          Answer b;
          if (decode(s, ch, cw, 8, &forced, win, exact, b) != 0 || b.status != 0 ||
              memcmp(exact.data(), roomy.data(), exact.size() * sizeof(int16_t)) != 0 ||
              memcmp(&b.image, &a.image, sizeof(a.image)) != 0 || memcmp(&b.window, &a.window, sizeof(a.window)) != 0)
            ++bad;
          if (exact.size() > 64) {      // one block short: the arena runs out
            exact.resize(exact.size() - 64);
            if (decode(s, ch, cw, 8, &forced, win, exact, b) != 0 || b.status != EDET_JPEG_TOO_LARGE) ++bad;
          }
        }
      }
    }
    // arguments the call refuses
    const int32_t whole[4] = {0, 0, h, w};
    const int32_t three = 3, one = 1;
    {
      const uint8_t* p = s.data();
      const size_t n = s.size();
      if (decode(s, h, w, 3, nullptr, whole, roomy, a) != -1 || decode(s, h, w, 8, &three, whole, roomy, a) != -1) ++bad;
      if (decode(s, h, w, 8, nullptr, nullptr, roomy, a) != -1) ++bad;
      if (edet_jpeg_entropy_decode_window(&p, &n, 1, h, w, 8, nullptr, whole, roomy.data(), roomy.size(), &a.image, nullptr,
                                          a.qt.data(), &a.status, 1) != -1)
        ++bad;
      if (decode(s, h, w, 8, nullptr, whole, roomy, a) != 0 || a.status != 0 || a.image.reserved != 1) ++bad;      // NULL: 1
      if (decode(s, h, w, 1, &one, whole, roomy, a) != 0 || a.status != 0) ++bad;
    }
    // prefixes and single-byte changes, with a window in the lower right quarter at 1/2
    const int32_t two = 2;
    const int oh = (h + 1) / 2, ow = (w + 1) / 2;
    const int32_t win[4] = {oh / 2, ow / 2, oh - oh / 2, ow - ow / 2};
    uint32_t seed = 0x2545F491u;
    auto rnd = [&seed]() {
      seed ^= seed << 13;
      seed ^= seed >> 17;
      seed ^= seed << 5;
      return seed;
    };
    for (size_t n = 0; n < s.size(); ++n) {
      std::vector<uint8_t> cut(s.begin(), s.begin() + n);      // exactly sized: a read past the prefix is past an allocation
      if (decode(cut, oh, ow, 8, &two, win, roomy, a) != 0 || !sound(a, win, oh, ow, used)) ++bad;
      ++runs;
      accepted += a.status == 0;
    }
    for (int k = 0; k < 300; ++k) {
      std::vector<uint8_t> m(s);
      m[rnd() % m.size()] = (uint8_t)rnd();
      const int32_t first[4] = {0, 0, 1, 1};
      if (decode(m, oh, ow, 8, &two, k & 1 ? win : first, roomy, a) != 0 || !sound(a, k & 1 ? win : first, oh, ow, used)) ++bad;
      ++runs;
      accepted += a.status == 0;
    }
    printf("%d x %d: ", h, w);
  }
  printf("%ld windows (%ld refused), %ld mutated runs (%ld still decoded), %d failures\n", windows, refused, runs, accepted, bad);
  return bad ? 1 : 0;
}
