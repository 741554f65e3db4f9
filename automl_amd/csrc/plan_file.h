// Plan files and state files decoded and validated on the host, before anything touches the device.  Standard headers
// only: no HIP, no library state.  File layouts: automl_amd/plan.py (docstring).
//
// A PlanFile / StateFile holds what the file says and nothing else -- every device pointer is still (buffer, offset).  Blob
// and payload bytes are NOT copied: they point into the span that was parsed, which must outlive the description.
#ifndef EDET_PLAN_FILE_H_
#define EDET_PLAN_FILE_H_
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace plan_file {

constexpr uint32_t NULL_BUF = 0xffffffffu;
constexpr int MAX_RANK = 4;
enum OpKind : uint8_t { OP_CALL = 0, OP_EVENT_RECORD = 1, OP_STREAM_WAIT = 2, OP_ALLREDUCE = 3 };
enum ArgType : uint8_t { A_INT = 0, A_DOUBLE = 1, A_DEVPTR = 2, A_STREAM = 3, A_BLOB = 4, A_NULL = 5 };

// The slots of a variable (EDET_SLOT_* of edet_net.h) and the named arena each lives in, at the variable's element offset.
// A moving statistic has the value slot only, in "bn_state".
constexpr int NUM_SLOTS = 4;
constexpr const char* kSlotNames[NUM_SLOTS] = {"value", "ema", "momentum", "adam_v"};
constexpr const char* kSlotArenas[NUM_SLOTS] = {"params", "ema", "velocity", "adam_v"};
constexpr const char* kStateArena = "bn_state";

// THE range test on file-derived values: [off, off + len) lies inside [0, cap), in a form that cannot wrap.
inline bool fits(uint64_t off, uint64_t len, uint64_t cap) { return len <= cap && off <= cap - len; }

struct DevRef {
  uint32_t buf = NULL_BUF;      // NULL_BUF: a null pointer
  uint64_t off = 0;
};

struct BlobReloc {
  uint32_t at;      // byte offset of the 8-byte pointer slot inside the blob
  DevRef to;
};

struct Arg {
  uint8_t type = A_NULL;
  int64_t i = 0;                       // A_INT
  double f = 0.0;                      // A_DOUBLE
  DevRef ptr;                          // A_DEVPTR
  uint32_t stream = 0;                 // A_STREAM
  const unsigned char* blob = nullptr; // A_BLOB: blob_bytes bytes inside the parsed span
  uint32_t blob_bytes = 0;
  std::vector<BlobReloc> relocs;       // A_BLOB
};

struct Op {
  uint8_t kind = OP_CALL;
  int fn = -1;                // OP_CALL: index into kPlanFnNames
  std::vector<Arg> args;      // OP_CALL
  uint32_t event = 0, stream = 0;      // OP_EVENT_RECORD / OP_STREAM_WAIT; OP_ALLREDUCE: stream
  DevRef ptr;                 // OP_ALLREDUCE: `count` floats
  uint64_t count = 0;
};

struct Program {
  std::string name;
  std::vector<Op> ops;
};

struct Buffer {
  uint64_t bytes, init_offset;      // init_offset 0: zero-filled
};

struct Name {
  std::string name;
  uint32_t buf;      // NULL_BUF: an integer property, its value in `off`
  uint64_t off, bytes;
};

struct DevReloc {
  uint32_t buf;
  uint64_t at;
  DevRef to;
};

// One entry of the variable table: `off` / `count` are ELEMENTS inside the variable's fp32 arena.
struct Var {
  std::string name;
  int trainable = 0;
  int rank = 0;
  int64_t dims[MAX_RANK] = {0, 0, 0, 0};
  uint64_t off = 0, count = 0;
};

struct PlanFile {
  uint32_t version = 0, nstreams = 0, nevents = 0;
  std::vector<std::string> entry_points;      // as the file lists them
  std::vector<Buffer> buffers;
  std::vector<Name> names;
  std::vector<DevReloc> dev_relocs;
  std::vector<Program> programs;
  bool has_vars = false;
  std::vector<Var> vars;
  int optimizer = -1;                         // property "optimizer": 0 sgd, 1 adam, 2 lion; -1 = a plan without it
  int64_t iterations = 0;
  double beta1 = 0.0, beta2 = 0.0;            // Adam and Lion plans
  double lion_wd = 0.0;                       // Lion plans
};

struct StateRecord {
  std::string name;
  int slot = 0, rank = 0;
  uint64_t dims[MAX_RANK] = {0, 0, 0, 0};
  uint64_t count = 0;
  const unsigned char* data = nullptr;      // count fp32 values inside the parsed span (unaligned)
};

struct StateFile {
  uint32_t version = 0;
  int64_t iterations = 0;
  std::vector<StateRecord> records;
};

// `data` .. `data + n` is the WHOLE file.  True: *out describes it.  False: *err says why not (no prefix, no path).
bool parse_plan(const unsigned char* data, size_t n, PlanFile* out, std::string* err);
bool parse_state(const unsigned char* data, size_t n, StateFile* out, std::string* err);

}  // namespace plan_file
#endif  // EDET_PLAN_FILE_H_
