// Stand-alone checker of the plan / state file parser (automl_amd/csrc/plan_file.cpp): no HIP, no library.
//   plan_check FILE             prints the parsed plan as text, exit 0; a file that is refused: "error: <text>", exit 1
//   plan_check --state FILE     the same for a state file
//   plan_check --prefixes FILE  parses every proper prefix of the plan's head (what lies in front of the first initial
//                               contents; the whole file if it has none); exit 0 iff each was refused with a message
// tests/test_plan_file.py formats automl_amd.plan's reading of the same file the same way and compares the texts.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../automl_amd/csrc/plan_file.h"
#define PLAN_STUBS_TABLES_ONLY      // kPlanFnNames, for the calls' names
#include "../../automl_amd/csrc/plan_stubs.inc"

using namespace plan_file;
typedef unsigned long long ull;

static ull fnv1a(const unsigned char* p, size_t n) {
  ull h = 14695981039346656037ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

static void print_plan(const PlanFile& pf) {
  printf("plan version %u buffers %zu names %zu streams %u events %u programs %zu entry_points %zu device_relocations %zu "
         "variables %zu\n", pf.version, pf.buffers.size(), pf.names.size(), pf.nstreams, pf.nevents, pf.programs.size(),
         pf.entry_points.size(), pf.dev_relocs.size(), pf.vars.size());
  for (size_t i = 0; i < pf.entry_points.size(); ++i) printf("fn %zu %s\n", i, pf.entry_points[i].c_str());
  for (size_t i = 0; i < pf.buffers.size(); ++i)
    printf("buffer %zu bytes %llu init %llu\n", i, (ull)pf.buffers[i].bytes, (ull)pf.buffers[i].init_offset);
  for (const Name& m : pf.names) printf("name %s buf %u off %llu bytes %llu\n", m.name.c_str(), m.buf, (ull)m.off, (ull)m.bytes);
  for (const DevReloc& d : pf.dev_relocs) printf("devreloc %u+%llu to %u+%llu\n", d.buf, (ull)d.at, d.to.buf, (ull)d.to.off);
  for (const Program& prog : pf.programs) {
    printf("program %s ops %zu\n", prog.name.c_str(), prog.ops.size());
    for (const Op& op : prog.ops) {
      if (op.kind == OP_EVENT_RECORD) printf("op evrec %u %u\n", op.event, op.stream);
      if (op.kind == OP_STREAM_WAIT) printf("op wait %u %u\n", op.stream, op.event);
      if (op.kind == OP_ALLREDUCE) printf("op allreduce %u+%llu %llu %u\n", op.ptr.buf, (ull)op.ptr.off, (ull)op.count, op.stream);
      if (op.kind != OP_CALL) continue;
      printf("op call %s", kPlanFnNames[op.fn]);
      for (const Arg& a : op.args) {
        ull bits;
        memcpy(&bits, &a.f, 8);
        if (a.type == A_INT) printf(" i:%lld", (long long)a.i);
        if (a.type == A_DOUBLE) printf(" f:%016llx", bits);
        if (a.type == A_DEVPTR) printf(" p:%u+%llu", a.ptr.buf, (ull)a.ptr.off);
        if (a.type == A_STREAM) printf(" s:%u", a.stream);
        if (a.type == A_NULL) printf(" n");
        if (a.type != A_BLOB) continue;
        printf(" b:%u:%016llx[", a.blob_bytes, fnv1a(a.blob, a.blob_bytes));
        for (const BlobReloc& q : a.relocs) printf("%u>%u+%llu,", q.at, q.to.buf, (ull)q.to.off);
        printf("]");
      }
      printf("\n");
    }
  }
  for (const Var& v : pf.vars) {
    printf("var %s trainable %d shape", v.name.c_str(), v.trainable);
    for (int d = 0; d < v.rank; ++d) printf(" %lld", (long long)v.dims[d]);
    printf(" off %llu count %llu\n", (ull)v.off, (ull)v.count);
  }
}

static void print_state(const StateFile& sf) {
  printf("state records %zu iterations %lld\n", sf.records.size(), (long long)sf.iterations);
  for (const StateRecord& rec : sf.records) {
    printf("rec %s slot %d shape", rec.name.c_str(), rec.slot);
    for (int d = 0; d < rec.rank; ++d) printf(" %llu", (ull)rec.dims[d]);
    printf(" count %llu fnv %016llx\n", (ull)rec.count, fnv1a(rec.data, (size_t)rec.count * 4));
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc == 3 ? argv[1] : "";
  if (argc != 2 && !(argc == 3 && (mode == "--state" || mode == "--prefixes"))) {
    fprintf(stderr, "usage: plan_check [--state | --prefixes] FILE\n");
    return 2;
  }
  FILE* f = fopen(argv[argc - 1], "rb");
  if (!f) {
    printf("error: cannot open %s\n", argv[argc - 1]);
    return 1;
  }
  std::vector<unsigned char> data;
  unsigned char chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) data.insert(data.end(), chunk, chunk + n);
  fclose(f);
  std::string err;
  if (mode == "--state") {
    StateFile sf;
    if (!parse_state(data.data(), data.size(), &sf, &err)) {
      printf("error: %s\n", err.c_str());
      return 1;
    }
    print_state(sf);
    return 0;
  }
  PlanFile pf;
  if (!parse_plan(data.data(), data.size(), &pf, &err)) {
    printf("error: %s\n", err.c_str());
    return 1;
  }
  if (mode.empty()) {
    print_plan(pf);
    return 0;
  }
  size_t head = data.size();
  for (const Buffer& b : pf.buffers)
    if (b.init_offset && b.init_offset < head) head = (size_t)b.init_offset;
  for (size_t cut = 0; cut < head; ++cut) {
    // a copy of exactly `cut` bytes, so that a read past the prefix is a read past an allocation
    const std::vector<unsigned char> prefix(data.begin(), data.begin() + cut);
    err.clear();
    if (parse_plan(prefix.data(), prefix.size(), &pf, &err) || err.empty()) {
      printf("a prefix of %zu bytes was not refused\n", cut);
      return 1;
    }
  }
  printf("%zu prefixes refused\n", head);
  return 0;
}
