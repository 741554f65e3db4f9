// Decoder of plan files and state files (plan_file.h).  Every byte read goes through Cursor, every range test through fits().
#include "plan_file.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <set>

namespace plan_file {
namespace {

#define PLAN_STUBS_TABLES_ONLY      // kPlanFnNames / kPlanFnArgs without the call stubs
#include "plan_stubs.inc"

// Reads forward through a byte span.  Sticky: after the first read past the end every read fails and yields zeros.
struct Cursor {
  const unsigned char* p;
  size_t left;
  bool ok = true;
  const unsigned char* bytes(size_t n) {
    if (!ok || n > left) {
      ok = false;
      return nullptr;
    }
    const unsigned char* at = p;
    p += n;
    left -= n;
    return at;
  }
  template <class T> T get() {
    T v{};
    if (const unsigned char* at = bytes(sizeof(T))) memcpy(&v, at, sizeof(T));
    return v;
  }
  std::string str() {
    const uint16_t n = get<uint16_t>();
    const unsigned char* at = bytes(n);
    return at ? std::string((const char*)at, n) : std::string();
  }
  // True when the bytes that remain can hold `count` records of at least min_record bytes each: asked of every count the
  // file gives before anything is sized by it.
  bool room(uint64_t count, size_t min_record) const { return ok && count <= left / min_record; }
};

bool fail(std::string* err, const char* fmt, ...) {
  char text[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(text, sizeof(text), fmt, ap);
  va_end(ap);
  *err = text;
  return false;
}
#define PLAN_CHECK(cond, ...) \
  do {                        \
    if (!(cond)) return fail(err, __VA_ARGS__); \
  } while (0)

int find_fn(const std::string& name) {
  const int n = (int)(sizeof(kPlanFnNames) / sizeof(kPlanFnNames[0]));
  for (int i = 0; i < n; ++i)
    if (name == kPlanFnNames[i]) return i;
  return -1;
}

// The last entry of that name, as a handle (property = false) or an integer property (true); nullptr if there is none.
const Name* find_name(const PlanFile& pf, const char* name, bool property) {
  for (size_t i = pf.names.size(); i-- > 0;)
    if ((pf.names[i].buf == NULL_BUF) == property && pf.names[i].name == name) return &pf.names[i];
  return nullptr;
}

// A pointer into a buffer: null where `nullable`, else at most one past the buffer's end.
bool good_ref(const PlanFile& pf, const DevRef& r, bool nullable) {
  if (r.buf == NULL_BUF) return nullable;
  return r.buf < pf.buffers.size() && fits(r.off, 0, pf.buffers[r.buf].bytes);
}

bool parse_call(Cursor& r, const PlanFile& pf, const std::vector<int>& fn_map, const std::string& prog, Op& op, std::string* err) {
  const uint16_t fid = r.get<uint16_t>();
  const uint8_t nargs = r.get<uint8_t>();
  PLAN_CHECK(r.ok && fid < fn_map.size(), "bad entry-point index in program '%s'", prog.c_str());
  op.fn = fn_map[fid];
  PLAN_CHECK(nargs == kPlanFnArgs[op.fn], "%s takes %d arguments, the plan passes %d (plan from another version of the library?)",
             kPlanFnNames[op.fn], kPlanFnArgs[op.fn], (int)nargs);
  op.args.resize(nargs);
  for (Arg& a : op.args) {
    a.type = r.get<uint8_t>();
    if (a.type == A_INT) {
      a.i = r.get<int64_t>();
    } else if (a.type == A_DOUBLE) {
      a.f = r.get<double>();
    } else if (a.type == A_DEVPTR) {
      a.ptr.buf = r.get<uint32_t>();
      a.ptr.off = r.get<uint64_t>();
      PLAN_CHECK(r.ok && good_ref(pf, a.ptr, true), "bad device pointer");
    } else if (a.type == A_STREAM) {
      a.stream = r.get<uint32_t>();
      PLAN_CHECK(r.ok && a.stream < pf.nstreams, "bad stream index");
    } else if (a.type == A_BLOB) {
      a.blob_bytes = r.get<uint32_t>();
      PLAN_CHECK(r.ok && fits(0, a.blob_bytes, 1u << 20), "bad argument blob");
      a.blob = r.bytes(a.blob_bytes);
      PLAN_CHECK(r.ok, "truncated plan (blob)");
      const uint16_t nreloc = r.get<uint16_t>();
      PLAN_CHECK(r.room(nreloc, 16), "truncated plan (blob relocations)");
      a.relocs.resize(nreloc);
      for (BlobReloc& q : a.relocs) {
        q.at = r.get<uint32_t>();
        q.to.buf = r.get<uint32_t>();
        q.to.off = r.get<uint64_t>();
        PLAN_CHECK(r.ok && fits(q.at, 8, a.blob_bytes) && good_ref(pf, q.to, false), "bad blob relocation");
      }
    } else {
      PLAN_CHECK(a.type == A_NULL, "unknown argument type %d", (int)a.type);
    }
  }
  return true;
}

bool parse_programs(Cursor& r, uint32_t nprog, const std::vector<int>& fn_map, PlanFile* pf, std::string* err) {
  pf->programs.resize(nprog);
  for (Program& prog : pf->programs) {
    prog.name = r.str();
    const uint32_t nops = r.get<uint32_t>();
    PLAN_CHECK(r.room(nops, 4), "truncated plan (program header)");
    prog.ops.resize(nops);
    for (Op& op : prog.ops) {
      op.kind = r.get<uint8_t>();
      if (op.kind == OP_CALL) {
        if (!parse_call(r, *pf, fn_map, prog.name, op, err)) return false;
      } else if (op.kind == OP_EVENT_RECORD || op.kind == OP_STREAM_WAIT) {
        const uint32_t a = r.get<uint32_t>(), b = r.get<uint32_t>();
        op.event = op.kind == OP_EVENT_RECORD ? a : b;
        op.stream = op.kind == OP_EVENT_RECORD ? b : a;
        PLAN_CHECK(r.ok && op.event < pf->nevents && op.stream < pf->nstreams, "bad event operation");
      } else if (op.kind == OP_ALLREDUCE) {
        op.ptr.buf = r.get<uint32_t>();
        op.ptr.off = r.get<uint64_t>();
        op.count = r.get<uint64_t>();
        op.stream = r.get<uint32_t>();
        // `count` floats at `off`: the count is bounded by division first, so that 4 * count cannot wrap
        PLAN_CHECK(r.ok && op.ptr.buf < pf->buffers.size() && fits(0, op.count, pf->buffers[op.ptr.buf].bytes / 4) &&
                   fits(op.ptr.off, 4 * op.count, pf->buffers[op.ptr.buf].bytes) && op.stream < pf->nstreams,
                   "bad all-reduce operation");
      } else {
        PLAN_CHECK(false, "unknown operation %d", (int)op.kind);
      }
      PLAN_CHECK(r.ok, "truncated plan (program '%s')", prog.name.c_str());
    }
  }
  return true;
}

// The variable table (optional section behind the last program).
bool parse_vars(Cursor& r, PlanFile* pf, std::string* err) {
  const Name* announced = find_name(*pf, "num_variables", true);
  if (!announced) return true;
  const unsigned char* magic = r.bytes(8);
  PLAN_CHECK(magic && memcmp(magic, "EDETVARS", 8) == 0, "the plan announces a variable table and holds none");
  const uint32_t nvars = r.get<uint32_t>();
  PLAN_CHECK(r.room(nvars, 20) && nvars == announced->off, "bad variable table (count)");
  auto arena_elems = [&](const char* arena) -> int64_t {
    const Name* n = find_name(*pf, arena, false);
    return n ? (int64_t)(n->bytes / 4) : -1;
  };
  const int64_t cap_train = arena_elems(kSlotArenas[0]), cap_state = arena_elems(kStateArena);
  for (int slot = 1; slot < NUM_SLOTS; ++slot) {
    const int64_t c = arena_elems(kSlotArenas[slot]);
    PLAN_CHECK(c < 0 || c == cap_train, "bad variable table (the '%s' arena is not of the size of 'params')", kSlotArenas[slot]);
  }
  std::set<std::string> seen;
  pf->vars.resize(nvars);
  for (uint32_t i = 0; i < nvars; ++i) {
    Var& v = pf->vars[i];
    v.name = r.str();
    v.trainable = r.get<uint8_t>() ? 1 : 0;
    v.rank = r.get<uint8_t>();
    PLAN_CHECK(r.ok && v.rank <= MAX_RANK, "bad variable table (entry %u)", i);
    uint64_t prod = 1;
    bool small = true;
    for (int d = 0; d < v.rank; ++d) {
      const uint64_t dim = r.get<uint64_t>();
      small = small && dim <= (1ull << 40) && (dim == 0 || prod <= (1ull << 40) / dim);
      if (small) prod *= dim;
      v.dims[d] = (int64_t)dim;
    }
    v.off = r.get<uint64_t>();
    v.count = r.get<uint64_t>();
    const int64_t cap = v.trainable ? cap_train : cap_state;
    PLAN_CHECK(r.ok && small && v.count == prod && cap >= 0 && fits(v.off, v.count, (uint64_t)cap),
               "bad variable table (variable '%s' does not fit its arena)", v.name.c_str());
    PLAN_CHECK(seen.insert(v.name).second, "bad variable table ('%s' twice)", v.name.c_str());
  }
  pf->has_vars = true;
  return true;
}

bool parse_optimizer(PlanFile* pf, std::string* err) {
  auto prop = [&](const char* name, int64_t fallback) {
    const Name* n = find_name(*pf, name, true);
    return n ? (int64_t)n->off : fallback;
  };
  const int64_t optimizer = prop("optimizer", -1);
  pf->iterations = prop("iterations", 0);
  PLAN_CHECK(optimizer >= -1 && optimizer <= 2 && pf->iterations >= 0, "bad optimizer properties");
  pf->optimizer = (int)optimizer;
  if (pf->optimizer == 1) {
    PLAN_CHECK(find_name(*pf, "adam_beta1_bits", true) && find_name(*pf, "adam_beta2_bits", true),
               "an Adam plan without its beta properties");
    const int64_t b1 = prop("adam_beta1_bits", 0), b2 = prop("adam_beta2_bits", 0);
    memcpy(&pf->beta1, &b1, 8);
    memcpy(&pf->beta2, &b2, 8);
    PLAN_CHECK(pf->beta1 >= 0.0 && pf->beta1 < 1.0 && pf->beta2 >= 0.0 && pf->beta2 < 1.0, "bad Adam betas");
  }
  if (pf->optimizer == 2) {
    // Lion: the constants are arguments of the recorded update launch; the properties say what the plan was recorded with
    PLAN_CHECK(find_name(*pf, "lion_beta1_bits", true) && find_name(*pf, "lion_beta2_bits", true) &&
                   find_name(*pf, "lion_wd_bits", true),
               "a Lion plan without its beta and wd properties");
    const int64_t b1 = prop("lion_beta1_bits", 0), b2 = prop("lion_beta2_bits", 0), wd = prop("lion_wd_bits", 0);
    memcpy(&pf->beta1, &b1, 8);
    memcpy(&pf->beta2, &b2, 8);
    memcpy(&pf->lion_wd, &wd, 8);
    PLAN_CHECK(pf->beta1 >= 0.0 && pf->beta1 < 1.0 && pf->beta2 >= 0.0 && pf->beta2 < 1.0 && pf->lion_wd >= 0.0,
               "bad Lion constants");
  }
  return true;
}

}  // namespace

bool parse_plan(const unsigned char* data, size_t n, PlanFile* pf, std::string* err) {
  *pf = PlanFile();
  Cursor r{data, n};
  const unsigned char* magic = r.bytes(8);
  PLAN_CHECK(magic && memcmp(magic, "EDETPLAN", 8) == 0, "not a plan file");
  pf->version = r.get<uint32_t>();
  const uint32_t nbuf = r.get<uint32_t>(), nnames = r.get<uint32_t>();
  pf->nstreams = r.get<uint32_t>();
  pf->nevents = r.get<uint32_t>();
  const uint32_t nprog = r.get<uint32_t>(), nfn = r.get<uint32_t>(), ndevreloc = r.get<uint32_t>();
  PLAN_CHECK(r.ok, "truncated plan (header)");
  PLAN_CHECK(pf->version == 1, "plan version %u (this library reads version 1)", pf->version);
  PLAN_CHECK(pf->nstreams >= 1 && pf->nstreams <= 255, "bad stream count %u", pf->nstreams);
  PLAN_CHECK(r.room(nfn, 2), "truncated plan (entry-point names)");
  std::vector<int> fn_map(nfn);
  for (uint32_t i = 0; i < nfn; ++i) {
    pf->entry_points.push_back(r.str());
    fn_map[i] = find_fn(pf->entry_points[i]);
    PLAN_CHECK(fn_map[i] >= 0, "the plan calls %s, which this library does not export", pf->entry_points[i].c_str());
  }
  PLAN_CHECK(r.room(nbuf, 16), "truncated plan (buffer table)");
  pf->buffers.resize(nbuf);
  for (Buffer& b : pf->buffers) {
    b.bytes = r.get<uint64_t>();
    b.init_offset = r.get<uint64_t>();
  }
  PLAN_CHECK(r.room(nnames, 22), "truncated plan (names)");
  pf->names.resize(nnames);
  for (Name& m : pf->names) {
    m.name = r.str();
    m.buf = r.get<uint32_t>();
    m.off = r.get<uint64_t>();
    m.bytes = r.get<uint64_t>();
    PLAN_CHECK(r.ok && (m.buf == NULL_BUF || (m.buf < nbuf && fits(m.off, m.bytes, pf->buffers[m.buf].bytes))),
               "bad named buffer '%s'", m.name.c_str());
  }
  PLAN_CHECK(r.room(ndevreloc, 24), "truncated plan (device relocations)");
  pf->dev_relocs.resize(ndevreloc);
  for (DevReloc& d : pf->dev_relocs) {
    d.buf = r.get<uint32_t>();
    d.at = r.get<uint64_t>();
    d.to.buf = r.get<uint32_t>();
    d.to.off = r.get<uint64_t>();
    PLAN_CHECK(r.ok && d.buf < nbuf && fits(d.at, 8, pf->buffers[d.buf].bytes) && good_ref(*pf, d.to, false),
               "bad device relocation");
  }
  PLAN_CHECK(r.room(nprog, 6), "truncated plan (programs)");
  if (!parse_programs(r, nprog, fn_map, pf, err) || !parse_vars(r, pf, err) || !parse_optimizer(pf, err)) return false;
  // last, so that a file cut anywhere in front of its initial contents is refused as truncated where it was cut
  for (uint32_t i = 0; i < nbuf; ++i)
    PLAN_CHECK(pf->buffers[i].init_offset == 0 || fits(pf->buffers[i].init_offset, pf->buffers[i].bytes, n),
               "truncated plan (the initial contents of buffer %u lie outside the file)", i);
  return true;
}

bool parse_state(const unsigned char* data, size_t n, StateFile* sf, std::string* err) {
  *sf = StateFile();
  Cursor r{data, n};
  const unsigned char* magic = r.bytes(8);
  PLAN_CHECK(magic && memcmp(magic, "EDETSTAT", 8) == 0, "not a state file");
  sf->version = r.get<uint32_t>();
  const uint32_t announced = r.get<uint32_t>();
  sf->iterations = r.get<int64_t>();
  PLAN_CHECK(r.ok, "truncated state file (header)");
  PLAN_CHECK(sf->version == 1, "state file version %u (this library reads version 1)", sf->version);
  PLAN_CHECK(sf->iterations >= 0, "bad iteration count %lld", (long long)sf->iterations);
  PLAN_CHECK(r.room(announced, 12), "truncated state file (%u records announced)", announced);
  sf->records.resize(announced);
  for (uint32_t i = 0; i < announced; ++i) {
    StateRecord& rec = sf->records[i];
    rec.name = r.str();
    rec.slot = r.get<uint8_t>();
    rec.rank = r.get<uint8_t>();
    PLAN_CHECK(r.ok && rec.rank <= MAX_RANK, "truncated or bad record %u", i);
    for (int d = 0; d < rec.rank; ++d) rec.dims[d] = r.get<uint64_t>();
    rec.count = r.get<uint64_t>();
    PLAN_CHECK(r.room(rec.count, 4), "truncated state file (variable '%s')", rec.name.c_str());
    rec.data = r.bytes((size_t)rec.count * 4);
  }
  PLAN_CHECK(r.left == 0, "the file carries bytes after its last record");
  return true;
}

}  // namespace plan_file
