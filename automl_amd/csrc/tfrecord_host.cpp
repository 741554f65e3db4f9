// TFRecord framing, CRC-32C and tf.train.Example wire parsing on the host (include/edet_hip.h, "TFRecord input").  Plain C++,
// no device call: serial byte work in front of the JPEG host stage (jpeg_host.cpp), on at most 16 worker threads.  Every
// input is a (pointer, length) pair into the caller's memory, every output a caller-allocated array with a stated capacity;
// nothing is allocated here, and every read is checked against the end of the message it belongs to before it is made.
// Restated in tests/tfrecord_ref.py; tests/c_host/tfrecord_host_check.cpp runs this file alone under the sanitizers.
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../include/edet_hip.h"

void edet_set_error(const char* fmt, ...);      // error.cpp (the stand-alone checker brings its own)

namespace {

constexpr int MAX_THREADS = 16;

// ---- CRC-32C, slicing by eight: table k maps a byte that has k more bytes behind it in the same 8-byte step ------------
struct CrcTables {
  uint32_t t[8][256];
  CrcTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82f63b78u : c >> 1;
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int k = 1; k < 8; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xff];
  }
};

const CrcTables& crc_tables() {
  static const CrcTables tables;      // built once, by whichever thread comes first
  return tables;
}

uint32_t crc_extend(uint32_t crc, const uint8_t* p, size_t n) {
  const CrcTables& T = crc_tables();
  uint32_t c = ~crc;
  while (n >= 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4);
    memcpy(&hi, p + 4, 4);
    lo ^= c;
    c = T.t[7][lo & 0xff] ^ T.t[6][(lo >> 8) & 0xff] ^ T.t[5][(lo >> 16) & 0xff] ^ T.t[4][lo >> 24] ^
        T.t[3][hi & 0xff] ^ T.t[2][(hi >> 8) & 0xff] ^ T.t[1][(hi >> 16) & 0xff] ^ T.t[0][hi >> 24];
    p += 8;
    n -= 8;
  }
  while (n--) c = T.t[0][(c ^ *p++) & 0xff] ^ (c >> 8);
  return ~c;
}

uint32_t crc_mask(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

uint32_t load32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

uint64_t load64(const uint8_t* p) { return (uint64_t)load32(p) | (uint64_t)load32(p + 4) << 32; }

// ---- protobuf wire format ---------------------------------------------------------------------------------------------
// A cursor over one message: [p, end).  Every helper returns an EDET_EXAMPLE_* status and moves p only on success.
struct Cursor {
  const uint8_t* p;
  const uint8_t* end;
};

int get_varint(Cursor& c, uint64_t* out) {
  uint64_t v = 0;
  for (int k = 0; k < 10; ++k) {
    if (c.p == c.end) return EDET_EXAMPLE_VARINT;      // cut off by the end of its message
    const uint8_t b = *c.p++;
    if (k < 9) v |= (uint64_t)(b & 0x7f) << (7 * k);
    else v |= (uint64_t)(b & 0x01) << 63;              // the tenth byte: one bit is left of the 64
    if (!(b & 0x80)) {
      *out = v;
      return EDET_EXAMPLE_OK;
    }
  }
  return EDET_EXAMPLE_VARINT;      // an eleventh byte
}

// A length-delimited field's payload as a cursor of its own; the length is checked in subtraction form.
int get_span(Cursor& c, Cursor* out) {
  uint64_t n;
  const int rc = get_varint(c, &n);
  if (rc) return rc;
  if (n > (uint64_t)(c.end - c.p)) return EDET_EXAMPLE_LENGTH;
  out->p = c.p;
  out->end = c.p + n;
  c.p += n;
  return EDET_EXAMPLE_OK;
}

int get_tag(Cursor& c, uint32_t* field, uint32_t* wire) {
  uint64_t tag;
  const int rc = get_varint(c, &tag);
  if (rc) return rc;
  *wire = (uint32_t)(tag & 7);
  *field = (uint32_t)((tag >> 3) & 0xffffffffu);
  if (tag >> 35) *field = 0xffffffffu;      // a field number protobuf does not allow: unknown, skipped by its wire type
  return EDET_EXAMPLE_OK;
}

constexpr int MAX_GROUP_DEPTH = 32;

// Skips one unknown field whose tag has been read.  A group (wire type 3) is skipped field by field up to the end-group tag
// (wire type 4) of the same number, as protobuf skips it; an end-group tag that closes nothing, groups nested deeper than
// MAX_GROUP_DEPTH and the undefined wire types 6 and 7 are a status; a group that its message ends inside is a length error.
int skip_field(Cursor& c, uint32_t field, uint32_t wire, int depth = 0) {
  uint64_t v;
  Cursor s;
  switch (wire) {
    case 0: return get_varint(c, &v);
    case 1:
      if (c.end - c.p < 8) return EDET_EXAMPLE_LENGTH;
      c.p += 8;
      return EDET_EXAMPLE_OK;
    case 2: return get_span(c, &s);
    case 3:
      if (depth >= MAX_GROUP_DEPTH) return EDET_EXAMPLE_WIRE_TYPE;
      for (;;) {
        if (c.p == c.end) return EDET_EXAMPLE_LENGTH;
        uint32_t f, w;
        int rc = get_tag(c, &f, &w);
        if (rc) return rc;
        if (w == 4) return f == field ? EDET_EXAMPLE_OK : EDET_EXAMPLE_WIRE_TYPE;
        if ((rc = skip_field(c, f, w, depth + 1))) return rc;
      }
    case 5:
      if (c.end - c.p < 4) return EDET_EXAMPLE_LENGTH;
      c.p += 4;
      return EDET_EXAMPLE_OK;
    default: return EDET_EXAMPLE_WIRE_TYPE;      // an end-group tag outside a group, and the two undefined wire types
  }
}

// Where one wanted key's values of one record go.
struct Slot {
  int kind, capacity;
  int64_t* spans;      // bytes: [capacity][2]
  float* floats;
  int64_t* ints;
  int32_t* count;
};

// BytesList / FloatList / Int64List: `value = 1`, repeated; appended behind what the slot holds.
int parse_list(Cursor list, const uint8_t* record, const Slot& s) {
  while (list.p < list.end) {
    uint32_t field, wire;
    int rc = get_tag(list, &field, &wire);
    if (rc) return rc;
    if (field != 1) {
      if ((rc = skip_field(list, field, wire))) return rc;
      continue;
    }
    if (s.kind == EDET_EXAMPLE_BYTES) {
      if (wire != 2) return EDET_EXAMPLE_WIRE_TYPE;
      Cursor v;
      if ((rc = get_span(list, &v))) return rc;
      if (*s.count >= s.capacity) return EDET_EXAMPLE_CAPACITY;
      s.spans[2 * *s.count] = (int64_t)(v.p - record);
      s.spans[2 * *s.count + 1] = (int64_t)(v.end - v.p);
      ++*s.count;
    } else if (s.kind == EDET_EXAMPLE_FLOAT) {
      if (wire == 5) {
        if (list.end - list.p < 4) return EDET_EXAMPLE_LENGTH;
        if (*s.count >= s.capacity) return EDET_EXAMPLE_CAPACITY;
        const uint32_t bits = load32(list.p);
        memcpy(&s.floats[*s.count], &bits, 4);
        ++*s.count;
        list.p += 4;
      } else if (wire == 2) {
        Cursor v;
        if ((rc = get_span(list, &v))) return rc;
        const size_t n = (size_t)(v.end - v.p);
        if (n % 4) return EDET_EXAMPLE_LENGTH;
        if (n / 4 > (size_t)(s.capacity - *s.count)) return EDET_EXAMPLE_CAPACITY;
        for (size_t i = 0; i < n / 4; ++i) {
          const uint32_t bits = load32(v.p + 4 * i);
          memcpy(&s.floats[*s.count + (int)i], &bits, 4);
        }
        *s.count += (int)(n / 4);
      } else {
        return EDET_EXAMPLE_WIRE_TYPE;
      }
    } else {
      uint64_t x;
      if (wire == 0) {
        if ((rc = get_varint(list, &x))) return rc;
        if (*s.count >= s.capacity) return EDET_EXAMPLE_CAPACITY;
        memcpy(&s.ints[*s.count], &x, 8);
        ++*s.count;
      } else if (wire == 2) {
        Cursor v;
        if ((rc = get_span(list, &v))) return rc;
        while (v.p < v.end) {
          if ((rc = get_varint(v, &x))) return rc;
          if (*s.count >= s.capacity) return EDET_EXAMPLE_CAPACITY;
          memcpy(&s.ints[*s.count], &x, 8);
          ++*s.count;
        }
      } else {
        return EDET_EXAMPLE_WIRE_TYPE;
      }
    }
  }
  return EDET_EXAMPLE_OK;
}

// Feature: oneof kind { bytes_list = 1, float_list = 2, int64_list = 3 }.  The same member again is merged (appended), a
// different member resets the oneof, as protobuf reads it; a member other than the wanted one left standing is a status.
int parse_feature(Cursor f, const uint8_t* record, const Slot& s) {
  *s.count = 0;
  uint32_t set = 0;
  while (f.p < f.end) {
    uint32_t field, wire;
    int rc = get_tag(f, &field, &wire);
    if (rc) return rc;
    if (field < 1 || field > 3) {
      if ((rc = skip_field(f, field, wire))) return rc;
      continue;
    }
    if (wire != 2) return EDET_EXAMPLE_WIRE_TYPE;
    Cursor list;
    if ((rc = get_span(f, &list))) return rc;
    if (field != set) *s.count = 0;
    set = field;
    if ((int)field == s.kind) {
      if ((rc = parse_list(list, record, s))) return rc;
    }
  }
  return set && (int)set != s.kind ? EDET_EXAMPLE_KIND : EDET_EXAMPLE_OK;
}

struct Job {
  const uint8_t* const* records;
  const size_t* lengths;
  const edet_example_spec_t* spec;
  int nspec;
  void* const* values;
  int32_t* counts;
};

Slot slot_of(const Job& j, int i, int k) {
  Slot s;
  s.kind = j.spec[k].kind;
  s.capacity = j.spec[k].capacity;
  const size_t at = (size_t)i * (size_t)s.capacity;
  s.spans = s.kind == EDET_EXAMPLE_BYTES ? (int64_t*)j.values[k] + 2 * at : nullptr;
  s.floats = s.kind == EDET_EXAMPLE_FLOAT ? (float*)j.values[k] + at : nullptr;
  s.ints = s.kind == EDET_EXAMPLE_INT64 ? (int64_t*)j.values[k] + at : nullptr;
  s.count = j.counts + (size_t)i * (size_t)j.nspec + k;
  return s;
}

// Example.features = 1 -> Features.feature = 1 (map entries: key = 1, value = 2).
int parse_example(const Job& j, int i) {
  const uint8_t* record = j.records[i];
  for (int k = 0; k < j.nspec; ++k) j.counts[(size_t)i * (size_t)j.nspec + k] = -1;      // absent
  if (!record && j.lengths[i]) return EDET_EXAMPLE_LENGTH;
  Cursor ex = {record, record + j.lengths[i]};
  while (ex.p < ex.end) {
    uint32_t field, wire;
    int rc = get_tag(ex, &field, &wire);
    if (rc) return rc;
    if (field != 1) {
      if ((rc = skip_field(ex, field, wire))) return rc;
      continue;
    }
    if (wire != 2) return EDET_EXAMPLE_WIRE_TYPE;
    Cursor feats;
    if ((rc = get_span(ex, &feats))) return rc;
    while (feats.p < feats.end) {
      if ((rc = get_tag(feats, &field, &wire))) return rc;
      if (field != 1) {
        if ((rc = skip_field(feats, field, wire))) return rc;
        continue;
      }
      if (wire != 2) return EDET_EXAMPLE_WIRE_TYPE;
      Cursor entry;
      if ((rc = get_span(feats, &entry))) return rc;
      Cursor key = {entry.p, entry.p}, value = {entry.p, entry.p};      // absent: the empty string, the empty Feature
      while (entry.p < entry.end) {
        if ((rc = get_tag(entry, &field, &wire))) return rc;
        if (field != 1 && field != 2) {
          if ((rc = skip_field(entry, field, wire))) return rc;
          continue;
        }
        if (wire != 2) return EDET_EXAMPLE_WIRE_TYPE;
        if ((rc = get_span(entry, field == 1 ? &key : &value))) return rc;      // the last of each wins
      }
      const size_t klen = (size_t)(key.end - key.p);
      for (int k = 0; k < j.nspec; ++k) {
        if ((size_t)j.spec[k].key_len == klen && (klen == 0 || memcmp(j.spec[k].key, key.p, klen) == 0)) {
          if ((rc = parse_feature(value, record, slot_of(j, i, k)))) return rc;      // a repeated key: the last entry wins
          break;
        }
      }
    }
  }
  return EDET_EXAMPLE_OK;
}

}  // namespace

extern "C" int edet_crc32c(const uint8_t* data, size_t n, uint32_t* crc) {
  if (!crc || (!data && n)) {
    edet_set_error("edet_crc32c: null pointer");
    return -1;
  }
  *crc = crc_extend(*crc, data, n);
  return 0;
}

extern "C" int edet_tfrecord_index(const uint8_t* buf, size_t nbytes, int verify, uint64_t* offsets, uint64_t* lengths,
                                   size_t capacity, size_t* count, size_t* consumed) {
  if (!count || !consumed || (!buf && nbytes) || ((!offsets || !lengths) && capacity)) {
    edet_set_error("edet_tfrecord_index: null pointer");
    return -1;
  }
  size_t pos = 0, n = 0;
  int status = EDET_TFRECORD_OK;
  while (pos < nbytes) {
    const size_t left = nbytes - pos;
    if (left < 12) {
      status = EDET_TFRECORD_TRUNCATED_HEADER;
      break;
    }
    const uint64_t len = load64(buf + pos);
    if (verify && crc_mask(crc_extend(0, buf + pos, 8)) != load32(buf + pos + 8)) {
      status = EDET_TFRECORD_LENGTH_CRC;
      break;
    }
    if (left - 12 < 4 || len > (uint64_t)(left - 12 - 4)) {      // subtraction form: a length of 2^63 cannot wrap
      // the payload or its CRC ends behind the buffer: a length whose CRC matched is the writer's, so the file was cut;
      // a length nobody checked is just a length out of range
      status = verify ? EDET_TFRECORD_TRUNCATED_PAYLOAD : EDET_TFRECORD_LENGTH_RANGE;
      break;
    }
    if (n == capacity) {      // in front of the payload's CRC: the call that goes on from here computes it
      status = EDET_TFRECORD_CAPACITY;
      break;
    }
    const uint8_t* payload = buf + pos + 12;
    if (verify && crc_mask(crc_extend(0, payload, (size_t)len)) != load32(payload + len)) {
      status = EDET_TFRECORD_DATA_CRC;
      break;
    }
    offsets[n] = (uint64_t)(pos + 12);
    lengths[n] = len;
    ++n;
    pos += 12 + (size_t)len + 4;
  }
  *count = n;
  *consumed = pos;      // the start of the record the status is about; of the next one to index after "capacity reached"
  return status;
}

extern "C" int edet_example_parse(const uint8_t* const* records, const size_t* lengths, int n,
                                  const edet_example_spec_t* spec, int nspec, int threads, void* const* values,
                                  int32_t* counts, int32_t* status) {
  if (n < 0 || nspec < 0 || (n && (!records || !lengths || !status)) || (nspec && (!spec || !values || (n && !counts)))) {
    edet_set_error("edet_example_parse: null pointer, n %d < 0 or nspec %d < 0", n, nspec);
    return -1;
  }
  for (int k = 0; k < nspec; ++k) {
    if (spec[k].kind < EDET_EXAMPLE_BYTES || spec[k].kind > EDET_EXAMPLE_INT64 || spec[k].capacity < 0 || spec[k].key_len < 0 ||
        (!spec[k].key && spec[k].key_len) || (!values[k] && spec[k].capacity && n)) {
      edet_set_error("edet_example_parse: spec %d: kind %d, capacity %d, key length %d or a null pointer", k, spec[k].kind,
                     spec[k].capacity, spec[k].key_len);
      return -1;
    }
  }
  if (n == 0) return 0;
  if (threads <= 0 || threads > MAX_THREADS) threads = MAX_THREADS;      // never the machine's core count
  if (threads > n) threads = n;
  const Job job = {records, lengths, spec, nspec, values, counts};
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) status[i] = parse_example(job, i);
  };
  if (threads == 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    pool.reserve((size_t)threads - 1);
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
  }
  return 0;
}
