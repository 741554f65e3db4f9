// Stand-alone checker of the JPEG host stage (automl_amd/csrc/jpeg_host.cpp and nothing else), built by tests/test_jpeg.py
// with the host compiler under the address and undefined-behaviour sanitizers and run as a child process.
//
//   jpeg_host_check DIR
//
// DIR/list.txt has one line per stream: "<file> <expected status, or -1 for any> <1 = also mutate it>".  Every stream is
// decoded alone and must give the expected status; all of them are decoded as one batch on 4 threads and must give the same
// statuses and coefficients.  Of a stream marked for mutation every prefix is decoded, and 300 copies with one byte changed
// (fixed seed); each must give status 0 or a refusal code.  Exit 0 = all of that held and no sanitizer report ended the run.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "../../include/edet_hip.h"

void edet_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  va_end(ap);
}

namespace {

constexpr int CANVAS = 1024;
constexpr size_t CAPACITY = (size_t)64 * 12 * (CANVAS / 16) * (CANVAS / 16);      // one worst-case image

struct Arena {
  std::vector<int16_t> coef;
  std::vector<edet_jpeg_image_t> images;
  std::vector<uint16_t> qt;
  std::vector<int32_t> status;
  explicit Arena(size_t batch, size_t elements = CAPACITY) : coef(elements), images(batch), qt(256 * batch), status(batch) {}
};

int decode(const std::vector<std::vector<uint8_t>>& streams, Arena& a, int threads) {
  std::vector<const uint8_t*> ptrs;
  std::vector<size_t> sizes;
  for (const auto& s : streams) {
    ptrs.push_back(s.data());
    sizes.push_back(s.size());
  }
  return edet_jpeg_entropy_decode(ptrs.data(), sizes.data(), (int)streams.size(), CANVAS, CANVAS, a.coef.data(),
                                  a.coef.size(), a.images.data(), a.qt.data(), a.status.data(), threads);
}

bool status_ok(int s) { return s >= EDET_JPEG_OK && s <= EDET_JPEG_UNSUPPORTED; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: jpeg_host_check DIR\n");
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
  int bad = 0;
  Arena one(1);
  std::vector<std::vector<int16_t>> alone;
  for (size_t i = 0; i < streams.size(); ++i) {
    edet_jpeg_info_t info;
    const int irc = edet_jpeg_info(streams[i].data(), streams[i].size(), &info);
    if (irc != 0 && irc != -1) ++bad;
    if (decode({streams[i]}, one, 1) != 0 || !status_ok(one.status[0]) || (expect[i] >= 0 && one.status[0] != expect[i])) {
      fprintf(stderr, "stream %zu: status %d, expected %d\n", i, one.status[0], expect[i]);
      ++bad;
    }
    const size_t n = one.status[0] ? 0 : (size_t)64 * one.images[0].total_blocks;
    alone.emplace_back(one.coef.begin(), one.coef.begin() + n);
  }
  // the same streams as one batch on several threads
  Arena all(streams.size(), 2 * CAPACITY);      // (the streams of the fixture are small: a sixth of it is used)
  if (decode(streams, all, 4) != 0) ++bad;
  for (size_t i = 0; i < streams.size(); ++i) {
    const edet_jpeg_image_t& im = all.images[i];
    if (expect[i] >= 0 && all.status[i] != expect[i]) ++bad;
    if (all.status[i] == 0) {
      const size_t n = (size_t)64 * im.total_blocks;
      if (n != alone[i].size() || memcmp(all.coef.data() + (size_t)64 * im.first_block[0], alone[i].data(), n * 2) != 0) {
        fprintf(stderr, "stream %zu: the batch differs from the single decode\n", i);
        ++bad;
      }
    }
  }
  // prefixes and single-byte changes
  uint32_t seed = 0x2545F491u;
  auto rnd = [&seed]() {
    seed ^= seed << 13;
    seed ^= seed >> 17;
    seed ^= seed << 5;
    return seed;
  };
  long runs = 0, accepted = 0;
  for (size_t i = 0; i < streams.size(); ++i) {
    if (!mutate[i]) continue;
    const std::vector<uint8_t>& s = streams[i];
    for (size_t n = 0; n < s.size(); ++n) {
      // an exactly sized copy, so that a read past the prefix is a read past an allocation
      std::vector<uint8_t> cut(s.begin(), s.begin() + n);
      edet_jpeg_info_t info;
      (void)edet_jpeg_info(cut.data(), cut.size(), &info);
      if (decode({cut}, one, 1) != 0 || !status_ok(one.status[0])) ++bad;
      ++runs;
      accepted += one.status[0] == 0;
    }
    for (int k = 0; k < 300; ++k) {
      std::vector<uint8_t> m(s);
      m[rnd() % m.size()] = (uint8_t)rnd();
      edet_jpeg_info_t info;
      (void)edet_jpeg_info(m.data(), m.size(), &info);
      if (decode({m}, one, 1) != 0 || !status_ok(one.status[0])) ++bad;
      ++runs;
      accepted += one.status[0] == 0;
    }
  }
  printf("%zu streams, %ld mutated runs (%ld still decoded), %d failures\n", streams.size(), runs, accepted, bad);
  return bad ? 1 : 0;
}
