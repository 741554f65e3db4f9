// Stand-alone checker of the TFRecord host stage (automl_amd/csrc/tfrecord_host.cpp and nothing else), built by
// tests/test_tfrecord.py with the host compiler under the address and undefined-behaviour sanitizers and run as a child
// process.  It makes its own inputs: a three-record file of small tf.train.Example messages, then
//   - the CRC-32C known answers, and a split-and-continue call at every cut of a 70-byte buffer
//   - every prefix of the file, in an exactly sized allocation: a status, never more than three records
//   - every single-byte change of the second record's framing (12 + 4 bytes, all 255 other values): refused with the CRCs
//     verified, a status without
//   - the walk continued record by record after "capacity reached"
//   - a length field of 2^63 and of 2^64 - 1, with a correct length CRC (the file "ends inside the record") and without
//   - every prefix and 400 single-byte changes (fixed seed) of one Example: a status, whatever it is; the batch on 1 and on 4
//     threads gives the same bytes
// Exit 0 = all of that held and no sanitizer report ended the run.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/edet_hip.h"

void edet_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  va_end(ap);
}

namespace {

typedef std::vector<uint8_t> Bytes;

void varint(Bytes& out, uint64_t v) {
  while (v >= 0x80) {
    out.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  out.push_back((uint8_t)v);
}

void field(Bytes& out, int number, const Bytes& payload) {
  varint(out, (uint64_t)number << 3 | 2);
  varint(out, payload.size());
  out.insert(out.end(), payload.begin(), payload.end());
}

Bytes entry(const std::string& key, int member, const Bytes& list) {
  Bytes feature, e;
  field(feature, member, list);
  field(e, 1, Bytes(key.begin(), key.end()));
  field(e, 2, feature);
  return e;
}

// An Example with a bytes, a float (packed and unpacked values) and an int64 feature, and unknown fields in between.
Bytes example(int boxes) {
  Bytes feats;
  Bytes blist;
  field(blist, 1, Bytes(37, 0xD8));
  field(feats, 1, entry("image/encoded", 1, blist));
  Bytes packed, flist;
  for (int i = 0; i < boxes; ++i)
    for (int k = 0; k < 4; ++k) packed.push_back((uint8_t)(17 * i + k));
  field(flist, 1, packed);
  flist.push_back(1 << 3 | 5);      // one unpacked value behind the packed ones
  for (int k = 0; k < 4; ++k) flist.push_back((uint8_t)(0x3f - k));
  field(feats, 1, entry("image/object/bbox/xmin", 2, flist));
  Bytes ints, ilist;
  for (int i = 0; i < boxes; ++i) varint(ints, i % 2 ? (uint64_t)-1 : (uint64_t)i * 300);
  field(ilist, 1, ints);
  ilist.push_back(1 << 3 | 0);
  varint(ilist, 1ull << 63);
  field(feats, 1, entry("image/object/class/label", 3, ilist));
  feats.push_back(7 << 3 | 0);      // an unknown varint field
  varint(feats, 123456789);
  for (uint8_t b : {8 << 3 | 3, 2 << 3 | 0, 5, 9 << 3 | 3, 9 << 3 | 4, 8 << 3 | 4}) feats.push_back(b);      // an unknown group, one nested
  Bytes ex;
  ex.push_back(9 << 3 | 1);         // an unknown fixed64 field
  for (int k = 0; k < 8; ++k) ex.push_back((uint8_t)k);
  field(ex, 1, feats);
  return ex;
}

uint32_t crc_of(const uint8_t* p, size_t n) {
  uint32_t c = 0;
  edet_crc32c(p, n, &c);
  return c;
}

uint32_t masked(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

void put32(Bytes& out, uint32_t v) {
  for (int k = 0; k < 4; ++k) out.push_back((uint8_t)(v >> (8 * k)));
}

void frame(Bytes& out, const Bytes& record, uint64_t stated) {
  Bytes head;
  for (int k = 0; k < 8; ++k) head.push_back((uint8_t)(stated >> (8 * k)));
  out.insert(out.end(), head.begin(), head.end());
  put32(out, masked(crc_of(head.data(), 8)));
  out.insert(out.end(), record.begin(), record.end());
  put32(out, masked(crc_of(record.data(), record.size())));
}

struct Index {
  uint64_t offsets[8], lengths[8];
  size_t count, consumed;
  int status;
};

Index index_of(const Bytes& file, int verify, size_t capacity = 8) {
  Index ix;
  Bytes exact(file);      // an exactly sized copy: a read past the end is a read past an allocation
  ix.status = edet_tfrecord_index(exact.data(), exact.size(), verify, ix.offsets, ix.lengths, capacity, &ix.count, &ix.consumed);
  return ix;
}

constexpr int CAP = 6;
struct Parsed {
  std::vector<int64_t> spans, ints;
  std::vector<float> floats;
  std::vector<int32_t> counts, status;
  explicit Parsed(size_t n) : spans(n * 2, -7), ints(n * CAP, -7), floats(n * CAP, -7.0f), counts(n * 3, -7), status(n, -7) {}
};

int parse(const std::vector<Bytes>& records, Parsed& p, int threads) {
  std::vector<Bytes> exact(records);
  std::vector<const uint8_t*> ptrs;
  std::vector<size_t> sizes;
  for (const auto& r : exact) {
    ptrs.push_back(r.data());
    sizes.push_back(r.size());
  }
  const edet_example_spec_t spec[3] = {{"image/encoded", 13, EDET_EXAMPLE_BYTES, 1, 0},
                                       {"image/object/bbox/xmin", 22, EDET_EXAMPLE_FLOAT, CAP, 0},
                                       {"image/object/class/label", 24, EDET_EXAMPLE_INT64, CAP, 0}};
  void* values[3] = {p.spans.data(), p.floats.data(), p.ints.data()};
  return edet_example_parse(ptrs.data(), sizes.data(), (int)records.size(), spec, 3, threads, values, p.counts.data(),
                            p.status.data());
}

bool example_status_ok(int s) { return s >= EDET_EXAMPLE_OK && s <= EDET_EXAMPLE_KIND; }

}  // namespace

int main() {
  int bad = 0;
  long runs = 0;
  auto expect = [&bad](bool ok, const char* what, long a = 0, long b = 0) {
    if (!ok) {
      fprintf(stderr, "failed: %s (%ld, %ld)\n", what, a, b);
      ++bad;
    }
  };
  // CRC-32C
  expect(crc_of((const uint8_t*)"123456789", 9) == 0xE3069283u, "crc of 123456789");
  expect(crc_of(Bytes(32, 0).data(), 32) == 0x8A9136AAu, "crc of 32 zero bytes");
  expect(crc_of(Bytes(32, 0xFF).data(), 32) == 0x62A8AB43u, "crc of 32 0xFF bytes");
  Bytes ramp(70);
  for (size_t i = 0; i < ramp.size(); ++i) ramp[i] = (uint8_t)(i * 37 + 5);
  for (size_t cut = 0; cut <= ramp.size(); ++cut) {
    Bytes a(ramp.begin(), ramp.begin() + cut), b(ramp.begin() + cut, ramp.end());
    uint32_t c = 0;
    edet_crc32c(a.data(), a.size(), &c);
    edet_crc32c(b.data(), b.size(), &c);
    expect(c == crc_of(ramp.data(), ramp.size()), "crc continued at a cut", (long)cut);
  }
  // the file
  const std::vector<Bytes> records = {example(2), example(0), example(5)};
  Bytes file;
  std::vector<size_t> starts;
  for (const auto& r : records) {
    starts.push_back(file.size());
    frame(file, r, r.size());
  }
  for (int verify = 0; verify < 2; ++verify) {
    const Index ix = index_of(file, verify);
    expect(ix.status == EDET_TFRECORD_OK && ix.count == 3 && ix.consumed == file.size(), "the whole file", ix.status, (long)ix.count);
    for (size_t i = 0; i < 3 && i < ix.count; ++i)
      expect(ix.offsets[i] == starts[i] + 12 && ix.lengths[i] == records[i].size(), "offset and length", (long)i);
  }
  // every prefix
  for (size_t n = 0; n < file.size(); ++n) {
    const Index ix = index_of(Bytes(file.begin(), file.begin() + n), 1), un = index_of(Bytes(file.begin(), file.begin() + n), 0);
    size_t whole = 0;
    while (whole < 3 && starts[whole] + 12 + records[whole].size() + 4 <= n) ++whole;
    const bool boundary = n == 0 || (whole > 0 && starts[whole - 1] + 12 + records[whole - 1].size() + 4 == n);
    const size_t left = n - (whole ? starts[whole - 1] + 12 + records[whole - 1].size() + 4 : 0);
    const int want = boundary ? EDET_TFRECORD_OK : left < 12 ? EDET_TFRECORD_TRUNCATED_HEADER : EDET_TFRECORD_TRUNCATED_PAYLOAD;
    expect(ix.status == want && ix.count == whole, "a prefix", (long)n, ix.status);
    expect(un.status == (want == EDET_TFRECORD_TRUNCATED_PAYLOAD ? EDET_TFRECORD_LENGTH_RANGE : want) && un.count == whole,
           "a prefix, not verified", (long)n, un.status);
    ++runs;
  }
  // the second record's framing, byte by byte
  const size_t at[2] = {starts[1], starts[1] + 12 + records[1].size()};
  for (int part = 0; part < 2; ++part) {
    for (size_t k = 0; k < (part ? 4u : 12u); ++k) {
      for (int delta = 1; delta < 256; ++delta) {
        Bytes m(file);
        m[at[part] + k] = (uint8_t)(m[at[part] + k] + delta);
        const Index v = index_of(m, 1), u = index_of(m, 0);
        expect(v.status == (part ? EDET_TFRECORD_DATA_CRC : EDET_TFRECORD_LENGTH_CRC) && v.count == 1 && v.consumed == starts[1],
               "a changed framing byte, verified", (long)k, v.status);
        expect(u.status >= EDET_TFRECORD_OK && u.status <= EDET_TFRECORD_CAPACITY && u.count <= 8, "a changed framing byte, not verified",
               (long)k, u.status);
        runs += 2;
      }
    }
  }
  // a changed payload byte is the data CRC's
  {
    Bytes m(file);
    m[starts[2] + 12 + 3] ^= 0x10;
    const Index v = index_of(m, 1);
    expect(v.status == EDET_TFRECORD_DATA_CRC && v.count == 2 && v.consumed == starts[2], "a changed payload byte", v.status);
  }
  // record by record after "capacity reached"
  {
    size_t pos = 0, seen = 0;
    for (;;) {
      Bytes rest(file.begin() + pos, file.end());
      const Index ix = index_of(rest, 1, 1);
      if (ix.count == 1) {
        expect(seen < 3 && pos + ix.offsets[0] == starts[seen] + 12 && ix.lengths[0] == records[seen].size(), "a continued walk", (long)seen);
        ++seen;
      }
      pos += ix.consumed;
      if (ix.status != EDET_TFRECORD_CAPACITY) {
        expect(ix.status == EDET_TFRECORD_OK && pos == file.size() && seen == 3, "the end of a continued walk", ix.status, (long)seen);
        break;
      }
    }
  }
  // a length of 2^63
  {
    Bytes huge;
    frame(huge, records[0], 1ull << 63);
    for (uint64_t stated : {(uint64_t)1 << 63, ~(uint64_t)0, ~(uint64_t)0 - 11, (uint64_t)huge.size() + 1}) {
      Bytes h;
      frame(h, records[0], stated);
      expect(index_of(h, 1).status == EDET_TFRECORD_TRUNCATED_PAYLOAD && index_of(h, 0).status == EDET_TFRECORD_LENGTH_RANGE, "a huge length");
    }
    Bytes h;
    frame(h, records[0], records[0].size() + 1);      // one byte more than there is
    expect(index_of(h, 1).status == EDET_TFRECORD_TRUNCATED_PAYLOAD && index_of(h, 0).status == EDET_TFRECORD_LENGTH_RANGE,
           "a length one too large");
    huge[8] ^= 1;
    expect(index_of(huge, 1).status == EDET_TFRECORD_LENGTH_CRC && index_of(huge, 0).status == EDET_TFRECORD_LENGTH_RANGE,
           "a huge length with a wrong CRC");
  }
  // Examples
  Parsed one(3), four(3);
  expect(parse(records, one, 1) == 0 && parse(records, four, 4) == 0, "parse");
  expect(one.status == four.status && one.counts == four.counts && one.spans == four.spans && one.ints == four.ints &&
             memcmp(one.floats.data(), four.floats.data(), one.floats.size() * 4) == 0, "1 and 4 threads");
  const int want_counts[3][3] = {{1, 3, 3}, {1, 1, 1}, {1, 6, 6}};
  for (int i = 0; i < 3; ++i) {
    expect(one.status[i] == EDET_EXAMPLE_OK, "an Example's status", i, one.status[i]);
    for (int k = 0; k < 3; ++k) expect(one.counts[3 * i + k] == want_counts[i][k], "an Example's counts", i, k);
    expect(one.spans[2 * i + 1] == 37, "the image span", i);
  }
  expect(one.ints[2] == INT64_MIN && one.ints[1] == -1, "int64 values");
  {
    std::vector<Bytes> seven = {example(6)};      // seven values for a capacity of six
    Parsed p(1);
    expect(parse(seven, p, 1) == 0 && p.status[0] == EDET_EXAMPLE_CAPACITY, "a list longer than its capacity", p.status[0]);
  }
  const Bytes& ex = records[2];
  Parsed p(1);
  for (size_t n = 0; n < ex.size(); ++n) {
    expect(parse({Bytes(ex.begin(), ex.begin() + n)}, p, 1) == 0 && example_status_ok(p.status[0]), "a prefix of an Example", (long)n);
    ++runs;
  }
  uint32_t seed = 0x2545F491u;
  auto rnd = [&seed]() {
    seed ^= seed << 13;
    seed ^= seed >> 17;
    seed ^= seed << 5;
    return seed;
  };
  long accepted = 0;
  for (int k = 0; k < 400; ++k) {
    Bytes m(ex);
    m[rnd() % m.size()] = (uint8_t)rnd();
    expect(parse({m}, p, 1) == 0 && example_status_ok(p.status[0]), "a changed byte of an Example", k);
    accepted += p.status[0] == 0;
    ++runs;
  }
  printf("%ld runs (%ld changed Examples still parsed), %d failures\n", runs, accepted, bad);
  return bad ? 1 : 0;
}
