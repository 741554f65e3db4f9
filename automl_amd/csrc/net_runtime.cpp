// Network-level C ABI (include/edet_net.h): loads a step plan written by automl_amd/plan.py and replays its programs --
// the launches of EfficientDetNet.call (efficientdet/tf2/efficientdet_keras.py:893-915) and of
// EfficientDetNetTrain.train_step (efficientdet/tf2/train_lib.py:606-684) -- through the operator-level ABI of this
// library, eagerly or as one captured hipGraph per program.  Host code only: no kernels in this file.
//
// A plan holds no code and no host pointers: every device pointer is (buffer, offset), every structure / array argument is
// a byte blob with relocation entries, every stream an index (0 = the caller's stream), every fork / join an event
// operation.  File layout: automl_amd/plan.py (docstring).  The files are decoded and checked in plan_file.cpp, which knows
// nothing of the device; nothing here reads a file's bytes except to copy checked ranges of them.
#include <fcntl.h>
#include <math.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <deque>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "plan_file.h"
#include "../../include/edet_net.h"

namespace {

union PlanSlot {
  int64_t i;
  double f;
  void* p;
};

#include "plan_stubs.inc"

using plan_file::kSlotArenas;
using plan_file::kSlotNames;
using plan_file::NUM_SLOTS;
using plan_file::OP_ALLREDUCE;
using plan_file::OP_CALL;
using plan_file::OP_EVENT_RECORD;
using plan_file::OP_STREAM_WAIT;
using plan_file::Var;

struct Op {
  uint8_t kind;
  int fn;                       // OP_CALL: index into kPlanFnNames
  std::vector<PlanSlot> args;   // OP_CALL: decoded slots (stream slots are patched per run)
  std::vector<int> stream_args; // OP_CALL: (slot index << 8) | stream index
  uint32_t a = 0, b = 0;        // event / stream indices
  void* ptr = nullptr;          // OP_ALLREDUCE
  uint64_t count = 0;
};

struct Program {
  std::string name;
  std::vector<Op> ops;
  int runs = 0;
  hipGraphExec_t exec = nullptr;
  hipGraph_t graph = nullptr;
  hipStream_t captured_on = nullptr;
};

struct Named {
  uint32_t buf;
  uint64_t off, bytes;
};

}  // namespace

struct edet_net {
  std::vector<void*> bufs;
  std::vector<std::string> name_list;
  std::map<std::string, Named> names;
  std::map<std::string, int64_t> props;
  std::vector<Program> programs;
  std::vector<hipStream_t> streams;      // [0] unused (the caller's stream)
  std::vector<hipEvent_t> events;
  std::deque<std::vector<unsigned char>> blobs;      // patched structure / array arguments; a deque: stable addresses
  bool use_graph = false;
  std::vector<Var> vars;                 // the variable table, in the Python arena's creation order
  std::map<std::string, int64_t> var_index;
  bool has_vars = false;
  int optimizer = -1;                    // property "optimizer": 0 sgd, 1 adam, 2 lion; -1 = a plan without it
  int64_t iterations = 0;
  double beta1 = 0.0, beta2 = 0.0;       // Adam plans (Lion's constants are arguments of the recorded update launch)
  edet_allreduce_fn allreduce = nullptr;
  void* allreduce_ctx = nullptr;
};

namespace {

// A whole file mapped read-only for the time of a load (an empty file: ok, no bytes).
struct MappedFile {
  const unsigned char* data = nullptr;
  size_t size = 0;
  bool ok = false;
  explicit MappedFile(const char* path) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return;
    struct stat st;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
      size = (size_t)st.st_size;
      void* p = size ? mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
      ok = p != MAP_FAILED;
      data = ok ? (const unsigned char*)p : nullptr;
    }
    close(fd);
  }
  ~MappedFile() {
    if (data) munmap((void*)data, size);
  }
  MappedFile(const MappedFile&) = delete;
  MappedFile& operator=(const MappedFile&) = delete;
};

void free_net(edet_net* net) {
  if (!net) return;
  for (auto& p : net->programs) {
    if (p.exec) (void)hipGraphExecDestroy(p.exec);
    if (p.graph) (void)hipGraphDestroy(p.graph);
  }
  for (size_t i = 1; i < net->streams.size(); ++i)
    if (net->streams[i]) (void)hipStreamDestroy(net->streams[i]);
  for (auto e : net->events)
    if (e) (void)hipEventDestroy(e);
  for (auto b : net->bufs)
    if (b) (void)hipFree(b);
  delete net;
}

Program* find_program(edet_net* net, const char* name) {
  for (auto& p : net->programs)
    if (p.name == name) return &p;
  return nullptr;
}

// Issues the operations of a program on `main` (stream index 0) and the network's own streams.
int issue(edet_net* net, Program& prog, hipStream_t main) {
  std::vector<PlanSlot> slots;
  for (Op& op : prog.ops) {
    switch (op.kind) {
      case OP_CALL: {
        slots = op.args;
        for (int sa : op.stream_args) {
          const int idx = sa & 0xff;
          slots[sa >> 8].p = idx == 0 ? (void*)main : (void*)net->streams[idx];
        }
        const int rc = plan_dispatch(op.fn, slots.data());
        if (rc != 0) return rc;      // the entry point has set the error text
        break;
      }
      case OP_EVENT_RECORD: {
        const hipError_t e = hipEventRecord(net->events[op.a], op.b == 0 ? main : net->streams[op.b]);
        EDET_CHECK(e == hipSuccess, "plan '%s': hipEventRecord: %s", prog.name.c_str(), hipGetErrorString(e));
        break;
      }
      case OP_STREAM_WAIT: {
        const hipError_t e = hipStreamWaitEvent(op.a == 0 ? main : net->streams[op.a], net->events[op.b], 0);
        EDET_CHECK(e == hipSuccess, "plan '%s': hipStreamWaitEvent: %s", prog.name.c_str(), hipGetErrorString(e));
        break;
      }
      case OP_ALLREDUCE: {
        if (net->allreduce) {
          const int rc = net->allreduce(net->allreduce_ctx, (float*)op.ptr, (size_t)op.count,
                                        op.a == 0 ? (void*)main : (void*)net->streams[op.a]);
          EDET_CHECK(rc == 0, "plan '%s': the gradient all-reduce callback returned %d", prog.name.c_str(), rc);
        }
        break;
      }
      default:
        EDET_CHECK(false, "plan '%s': unknown operation %d", prog.name.c_str(), (int)op.kind);
    }
  }
  return 0;
}

int run_program(edet_net* net, const char* name, void* stream) {
  EDET_CHECK(net, "edet_net: null network");
  Program* prog = find_program(net, name);
  EDET_CHECK(prog, "edet_net: the plan holds no program '%s'", name);
  hipStream_t main = reinterpret_cast<hipStream_t>(stream);
  // first run eager (one-time kernel attribute setup of the library is not capturable); with use_graph the second run is
  // captured -- the side streams join the capture through the recorded fork / join events -- and replayed from then on
  if (net->use_graph && prog->runs >= 1) {
    if (prog->exec && prog->captured_on != main) {      // a graph is tied to nothing, but keep one exec per stream simple
      (void)hipGraphExecDestroy(prog->exec);
      (void)hipGraphDestroy(prog->graph);
      prog->exec = nullptr;
      prog->graph = nullptr;
    }
    if (!prog->exec) {
      EDET_CHECK(main != nullptr, "edet_net: graph mode needs a non-default stream (stream capture)");
      hipError_t e = hipStreamBeginCapture(main, hipStreamCaptureModeThreadLocal);
      EDET_CHECK(e == hipSuccess, "edet_net: hipStreamBeginCapture: %s", hipGetErrorString(e));
      const int rc = issue(net, *prog, main);
      hipGraph_t g = nullptr;
      e = hipStreamEndCapture(main, &g);
      if (rc != 0) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
      }
      EDET_CHECK(e == hipSuccess && g, "edet_net: hipStreamEndCapture: %s", hipGetErrorString(e));
      hipGraphExec_t x = nullptr;
      e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
      if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        EDET_CHECK(false, "edet_net: hipGraphInstantiate: %s", hipGetErrorString(e));
      }
      prog->graph = g;
      prog->exec = x;
      prog->captured_on = main;
    }
    const hipError_t e = hipGraphLaunch(prog->exec, main);
    EDET_CHECK(e == hipSuccess, "edet_net: hipGraphLaunch: %s", hipGetErrorString(e));
    ++prog->runs;
    return 0;
  }
  const int rc = issue(net, *prog, main);
  if (rc == 0) ++prog->runs;
  return rc;
}

void* dev_ptr(const edet_net* net, const plan_file::DevRef& r) {      // bounds: checked by parse_plan
  return r.buf == plan_file::NULL_BUF ? nullptr : (void*)((char*)net->bufs[r.buf] + r.off);
}

// Buffers, streams and events of a parsed plan, and its programs with every (buffer, offset) turned into a pointer.
int instantiate(edet_net* net, const plan_file::PlanFile& pf) {
  net->bufs.assign(pf.buffers.size(), nullptr);
  for (size_t i = 0; i < pf.buffers.size(); ++i) {
    const uint64_t bytes = pf.buffers[i].bytes;
    const hipError_t e = hipMalloc(&net->bufs[i], bytes ? bytes : 1);
    EDET_CHECK(e == hipSuccess, "edet_create: hipMalloc(%llu bytes) for buffer %u: %s", (unsigned long long)bytes, (unsigned)i,
               hipGetErrorString(e));
    if (!pf.buffers[i].init_offset) {
      const hipError_t m = hipMemset(net->bufs[i], 0, bytes);
      EDET_CHECK(m == hipSuccess, "edet_create: hipMemset: %s", hipGetErrorString(m));
    }
  }
  net->streams.assign(pf.nstreams, nullptr);
  for (uint32_t i = 1; i < pf.nstreams; ++i) {
    const hipError_t e = hipStreamCreateWithFlags(&net->streams[i], hipStreamNonBlocking);
    EDET_CHECK(e == hipSuccess, "edet_create: hipStreamCreate: %s", hipGetErrorString(e));
  }
  net->events.assign(pf.nevents, nullptr);
  for (uint32_t i = 0; i < pf.nevents; ++i) {
    const hipError_t e = hipEventCreateWithFlags(&net->events[i], hipEventDisableTiming);
    EDET_CHECK(e == hipSuccess, "edet_create: hipEventCreate: %s", hipGetErrorString(e));
  }
  for (const plan_file::Name& n : pf.names) {
    if (n.buf == plan_file::NULL_BUF) {
      net->props[n.name] = (int64_t)n.off;
    } else {
      net->names[n.name] = Named{n.buf, n.off, n.bytes};
      net->name_list.push_back(n.name);
    }
  }
  net->vars = pf.vars;
  for (size_t i = 0; i < net->vars.size(); ++i) net->var_index[net->vars[i].name] = (int64_t)i;
  net->has_vars = pf.has_vars;
  net->optimizer = pf.optimizer;
  net->iterations = pf.iterations;
  net->beta1 = pf.beta1;
  net->beta2 = pf.beta2;
  net->programs.resize(pf.programs.size());
  for (size_t pi = 0; pi < pf.programs.size(); ++pi) {
    Program& prog = net->programs[pi];
    prog.name = pf.programs[pi].name;
    prog.ops.resize(pf.programs[pi].ops.size());
    for (size_t oi = 0; oi < prog.ops.size(); ++oi) {
      const plan_file::Op& src = pf.programs[pi].ops[oi];
      Op& op = prog.ops[oi];
      op.kind = src.kind;
      op.fn = src.fn;
      op.a = src.kind == OP_EVENT_RECORD ? src.event : src.stream;
      op.b = src.kind == OP_EVENT_RECORD ? src.stream : src.event;
      op.ptr = src.kind == OP_ALLREDUCE ? dev_ptr(net, src.ptr) : nullptr;
      op.count = src.count;
      op.args.resize(src.args.size());
      for (size_t k = 0; k < src.args.size(); ++k) {
        const plan_file::Arg& a = src.args[k];
        PlanSlot& s = op.args[k];
        s.i = 0;
        if (a.type == plan_file::A_INT) {
          s.i = a.i;
        } else if (a.type == plan_file::A_DOUBLE) {
          s.f = a.f;
        } else if (a.type == plan_file::A_DEVPTR) {
          s.p = dev_ptr(net, a.ptr);
        } else if (a.type == plan_file::A_STREAM) {
          op.stream_args.push_back(((int)k << 8) | (int)a.stream);
        } else if (a.type == plan_file::A_BLOB) {
          net->blobs.emplace_back((a.blob_bytes + 15) / 8 * 8);      // padded to 8 bytes, plus slack
          unsigned char* blob = net->blobs.back().data();
          if (a.blob_bytes) memcpy(blob, a.blob, a.blob_bytes);
          for (const plan_file::BlobReloc& q : a.relocs) {
            void* p = dev_ptr(net, q.to);
            memcpy(blob + q.at, &p, 8);
          }
          s.p = blob;
        }
      }
    }
  }
  return 0;
}

// Initial contents through one pinned staging buffer, then the device pointers stored inside them.
int upload(edet_net* net, const plan_file::PlanFile& pf, const unsigned char* file) {
  const size_t CH = 64u << 20;
  void* stage = nullptr;
  EDET_CHECK(hipHostMalloc(&stage, CH, hipHostMallocDefault) == hipSuccess, "edet_create: hipHostMalloc failed");
  bool good = true;
  for (size_t i = 0; i < pf.buffers.size() && good; ++i) {
    const plan_file::Buffer& b = pf.buffers[i];
    if (!b.init_offset) continue;
    for (uint64_t done = 0; good && done < b.bytes; done += CH) {
      const size_t n = (size_t)(b.bytes - done < CH ? b.bytes - done : CH);
      memcpy(stage, file + b.init_offset + done, n);      // inside the file: checked by parse_plan
      good = hipMemcpy((char*)net->bufs[i] + done, stage, n, hipMemcpyHostToDevice) == hipSuccess;
    }
  }
  (void)hipHostFree(stage);
  EDET_CHECK(good, "edet_create: could not read / upload the initial contents");
  for (const plan_file::DevReloc& d : pf.dev_relocs) {
    void* p = dev_ptr(net, d.to);
    EDET_CHECK(hipMemcpy((char*)net->bufs[d.buf] + d.at, &p, 8, hipMemcpyHostToDevice) == hipSuccess,
               "edet_create: device relocation upload failed");
  }
  EDET_CHECK(hipDeviceSynchronize() == hipSuccess, "edet_create: hipDeviceSynchronize failed");
  return 0;
}

}  // namespace

// The file is decoded and checked as a whole (plan_file.cpp) before anything is allocated on the device.
extern "C" int edet_create(const char* plan_path, edet_net_t** net_out) {
  EDET_CHECK(plan_path && net_out, "edet_create: null argument");
  *net_out = nullptr;
  const MappedFile file(plan_path);
  EDET_CHECK(file.ok, "edet_create: cannot open %s", plan_path);
  plan_file::PlanFile pf;
  std::string err;
  EDET_CHECK(plan_file::parse_plan(file.data, file.size, &pf, &err), "edet_create: %s: %s", plan_path, err.c_str());
  std::unique_ptr<edet_net, void (*)(edet_net*)> net(new edet_net(), free_net);      // released on every failure below
  if (instantiate(net.get(), pf) != 0 || upload(net.get(), pf, file.data) != 0) return -1;
  *net_out = net.release();
  return 0;
}

extern "C" int edet_destroy(edet_net_t* net) {
  if (net) (void)hipDeviceSynchronize();
  free_net(net);
  return 0;
}

extern "C" int edet_net_buffer(edet_net_t* net, const char* name, void** device_ptr, size_t* bytes) {
  EDET_CHECK(net && name, "edet_net_buffer: null argument");
  auto it = net->names.find(name);
  EDET_CHECK(it != net->names.end(), "edet_net_buffer: the plan names no buffer '%s'", name);
  if (device_ptr) *device_ptr = (char*)net->bufs[it->second.buf] + it->second.off;
  if (bytes) *bytes = (size_t)it->second.bytes;
  return 0;
}

extern "C" int edet_net_num_buffers(edet_net_t* net) { return net ? (int)net->name_list.size() : 0; }

extern "C" const char* edet_net_buffer_name(edet_net_t* net, int index) {
  if (!net || index < 0 || index >= (int)net->name_list.size()) return nullptr;
  return net->name_list[index].c_str();
}

extern "C" int edet_net_property(edet_net_t* net, const char* name, int64_t* value) {
  EDET_CHECK(net && name && value, "edet_net_property: null argument");
  auto it = net->props.find(name);
  EDET_CHECK(it != net->props.end(), "edet_net_property: the plan holds no property '%s'", name);
  *value = it->second;
  return 0;
}

extern "C" int edet_net_has_program(edet_net_t* net, const char* program) {
  return net && program && find_program(net, program) ? 1 : 0;
}

extern "C" int edet_copy_to_host(void* host, const void* device, size_t bytes) {
  EDET_CHECK((host && device) || bytes == 0, "edet_copy_to_host: null pointer");
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && bytes) e = hipMemcpy(host, device, bytes, hipMemcpyDeviceToHost);
  EDET_CHECK(e == hipSuccess, "edet_copy_to_host: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int edet_copy_to_device(void* device, const void* host, size_t bytes) {
  EDET_CHECK((host && device) || bytes == 0, "edet_copy_to_device: null pointer");
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && bytes) e = hipMemcpy(device, host, bytes, hipMemcpyHostToDevice);
  EDET_CHECK(e == hipSuccess, "edet_copy_to_device: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int edet_net_use_graph(edet_net_t* net, int on) {
  EDET_CHECK(net, "edet_net_use_graph: null network");
  net->use_graph = on != 0;
  return 0;
}

extern "C" int edet_forward(edet_net_t* net, void* stream) { return run_program(net, "forward", stream); }

extern "C" int edet_detect(edet_net_t* net, void* stream) { return run_program(net, "detect", stream); }

extern "C" int edet_train_step(edet_net_t* net, float learning_rate, float ema_decay, void* stream) {
  EDET_CHECK(net, "edet_train_step: null network");
  auto it = net->names.find("hyper");
  EDET_CHECK(it != net->names.end() && it->second.bytes >= 8, "edet_train_step: the plan names no 'hyper' buffer");
  // per-step scalars of the schedule: a stream-ordered copy from pageable memory (staged by the runtime before it
  // returns), in front of -- never inside -- the replayed graph, as Engine.set_hyper does
  float h[2] = {learning_rate, ema_decay};
  if (net->optimizer == 1) {
    // tf.keras Adam's bias-corrected rate of THIS step, in the operation order of Engine.set_hyper (engine.py):
    // lr * sqrt(1 - beta2 ** t) / (1 - beta1 ** t) in double, rounded to float once
#pragma clang fp contract(off)
    const double t = (double)(net->iterations + 1);
    const double alpha = (double)learning_rate * sqrt(1.0 - pow(net->beta2, t)) / (1.0 - pow(net->beta1, t));
    h[0] = (float)alpha;
  }
  // (SGD and Lion -- optimizer 0 and 2 -- take the schedule's rate as it is: Lion has no bias correction)
  const hipError_t e = hipMemcpyAsync((char*)net->bufs[it->second.buf] + it->second.off, h, sizeof(h), hipMemcpyHostToDevice,
                                      reinterpret_cast<hipStream_t>(stream));
  EDET_CHECK(e == hipSuccess, "edet_train_step: hipMemcpyAsync: %s", hipGetErrorString(e));
  const int rc = run_program(net, "train_step", stream);
  if (rc == 0) ++net->iterations;
  return rc;
}

// ---- variables by name ------------------------------------------------------------------------------------------------
namespace {

// The named arena that holds a slot of a variable, at the variable's element offset (the table: plan_file.h).
const char* slot_arena(const Var& v, int slot) {
  return slot == EDET_SLOT_VALUE && !v.trainable ? plan_file::kStateArena : kSlotArenas[slot];
}

// Device address of a variable's slot, or nullptr with the error text set (the message names the variable).
float* slot_ptr(edet_net* net, const Var& v, int slot, const char* who) {
  if (slot < 0 || slot >= NUM_SLOTS) {
    edet_set_error("%s: variable '%s': unknown slot %d", who, v.name.c_str(), slot);
    return nullptr;
  }
  if (slot != EDET_SLOT_VALUE && !v.trainable) {
    edet_set_error("%s: variable '%s' is not trainable: it has no %s slot", who, v.name.c_str(), kSlotNames[slot]);
    return nullptr;
  }
  auto it = net->names.find(slot_arena(v, slot));
  if (it == net->names.end() || (slot == EDET_SLOT_ADAM_V && net->optimizer != 1)) {
    edet_set_error("%s: variable '%s' has no %s slot in this plan%s", who, v.name.c_str(), kSlotNames[slot],
                   slot == EDET_SLOT_ADAM_V ? " (its optimizer is not Adam)" : "");
    return nullptr;
  }
  return (float*)((char*)net->bufs[it->second.buf] + it->second.off) + v.off;      // bounds: checked by parse_plan
}

bool has_slot(edet_net* net, const Var& v, int slot) {
  if (slot == EDET_SLOT_VALUE) return true;
  if (!v.trainable || (slot == EDET_SLOT_ADAM_V && net->optimizer != 1)) return false;
  return net->names.count(slot_arena(v, slot)) != 0;
}

const Var* find_var(edet_net* net, const char* name, const char* who) {
  if (!net || !name) {
    edet_set_error("%s: null argument", who);
    return nullptr;
  }
  if (!net->has_vars) {
    edet_set_error("%s: variable '%s': the plan was recorded without a variable table", who, name);
    return nullptr;
  }
  auto it = net->var_index.find(name);
  if (it == net->var_index.end()) {
    edet_set_error("%s: the plan has no variable '%s'", who, name);
    return nullptr;
  }
  return &net->vars[(size_t)it->second];
}

}  // namespace

extern "C" int edet_net_num_variables(edet_net_t* net, int64_t* count) {
  EDET_CHECK(net && count, "edet_net_num_variables: null argument");
  EDET_CHECK(net->has_vars, "edet_net_num_variables: the plan was recorded without a variable table");
  *count = (int64_t)net->vars.size();
  return 0;
}

extern "C" int edet_net_variable_info(edet_net_t* net, int64_t index, edet_var_info* out) {
  EDET_CHECK(net && out, "edet_net_variable_info: null argument");
  EDET_CHECK(net->has_vars, "edet_net_variable_info: the plan was recorded without a variable table");
  EDET_CHECK(index >= 0 && index < (int64_t)net->vars.size(), "edet_net_variable_info: index %lld of %lld variables",
             (long long)index, (long long)net->vars.size());
  const Var& v = net->vars[(size_t)index];
  out->name = v.name.c_str();
  out->rank = v.rank;
  out->trainable = v.trainable;
  for (int d = 0; d < 4; ++d) out->dims[d] = v.dims[d];
  out->count = (int64_t)v.count;
  return 0;
}

extern "C" int edet_net_find_variable(edet_net_t* net, const char* name, int64_t* index) {
  EDET_CHECK(index, "edet_net_find_variable: null argument");
  const Var* v = find_var(net, name, "edet_net_find_variable");
  if (!v) return -1;
  *index = (int64_t)(v - net->vars.data());
  return 0;
}

extern "C" int edet_get_variable(edet_net_t* net, const char* name, int slot, float* host, int64_t capacity) {
  const Var* v = find_var(net, name, "edet_get_variable");
  if (!v) return -1;
  EDET_CHECK(host && capacity >= (int64_t)v->count, "edet_get_variable: variable '%s' has %lld elements, the capacity is %lld",
             name, (long long)v->count, (long long)capacity);
  float* p = slot_ptr(net, *v, slot, "edet_get_variable");
  if (!p) return -1;
  return edet_copy_to_host(host, p, (size_t)v->count * 4);
}

extern "C" int edet_set_variable(edet_net_t* net, const char* name, int slot, const float* host, int64_t count) {
  const Var* v = find_var(net, name, "edet_set_variable");
  if (!v) return -1;
  EDET_CHECK(host && count == (int64_t)v->count, "edet_set_variable: variable '%s' has %lld elements, got %lld", name,
             (long long)v->count, (long long)count);
  float* p = slot_ptr(net, *v, slot, "edet_set_variable");
  if (!p) return -1;
  if (edet_copy_to_device(p, host, (size_t)v->count * 4) != 0) return -1;
  // until the first optimizer step the moving average follows the variable (ParamArena.set_params)
  if (slot == EDET_SLOT_VALUE && v->trainable && net->iterations == 0 && has_slot(net, *v, EDET_SLOT_EMA)) {
    float* e = slot_ptr(net, *v, EDET_SLOT_EMA, "edet_set_variable");
    if (!e || edet_copy_to_device(e, host, (size_t)v->count * 4) != 0) return -1;
  }
  return 0;
}

extern "C" int edet_net_get_iterations(edet_net_t* net, int64_t* iterations) {
  EDET_CHECK(net && iterations, "edet_net_get_iterations: null argument");
  *iterations = net->iterations;
  return 0;
}

extern "C" int edet_net_set_iterations(edet_net_t* net, int64_t iterations) {
  EDET_CHECK(net, "edet_net_set_iterations: null network");
  EDET_CHECK(iterations >= 0, "edet_net_set_iterations: negative iteration count %lld", (long long)iterations);
  net->iterations = iterations;
  return 0;
}

// State files (layout: include/edet_net.h).
extern "C" int edet_net_save_state(edet_net_t* net, const char* path) {
  EDET_CHECK(net && path, "edet_net_save_state: null argument");
  EDET_CHECK(net->has_vars, "edet_net_save_state: the plan was recorded without a variable table");
  uint32_t nrec = 0;
  for (const Var& v : net->vars)
    for (int slot = 0; slot < NUM_SLOTS; ++slot) nrec += has_slot(net, v, slot) ? 1 : 0;
  FILE* f = fopen(path, "wb");
  EDET_CHECK(f, "edet_net_save_state: cannot open %s", path);
  const uint32_t version = 1;
  bool good = fwrite("EDETSTAT", 1, 8, f) == 8 && fwrite(&version, 4, 1, f) == 1 && fwrite(&nrec, 4, 1, f) == 1 &&
              fwrite(&net->iterations, 8, 1, f) == 1;
  std::vector<float> host;
  int rc = 0;
  for (size_t i = 0; good && rc == 0 && i < net->vars.size(); ++i) {
    const Var& v = net->vars[i];
    for (int slot = 0; good && rc == 0 && slot < NUM_SLOTS; ++slot) {
      if (!has_slot(net, v, slot)) continue;
      float* p = slot_ptr(net, v, slot, "edet_net_save_state");
      host.resize((size_t)v.count + 1);
      rc = p ? edet_copy_to_host(host.data(), p, (size_t)v.count * 4) : -1;
      const uint16_t len = (uint16_t)v.name.size();
      const uint8_t s8 = (uint8_t)slot, r8 = (uint8_t)v.rank;
      good = fwrite(&len, 2, 1, f) == 1 && fwrite(v.name.data(), 1, len, f) == len && fwrite(&s8, 1, 1, f) == 1 &&
             fwrite(&r8, 1, 1, f) == 1;
      for (int d = 0; good && d < v.rank; ++d) {
        const uint64_t dim = (uint64_t)v.dims[d];
        good = fwrite(&dim, 8, 1, f) == 1;
      }
      good = good && fwrite(&v.count, 8, 1, f) == 1 && fwrite(host.data(), 4, (size_t)v.count, f) == (size_t)v.count;
    }
  }
  good = (fclose(f) == 0) && good;
  if (rc != 0) return rc;
  EDET_CHECK(good, "edet_net_save_state: could not write %s", path);
  return 0;
}

extern "C" int edet_net_load_state(edet_net_t* net, const char* path) {
  EDET_CHECK(net && path, "edet_net_load_state: null argument");
  EDET_CHECK(net->has_vars, "edet_net_load_state: the plan was recorded without a variable table");
  const MappedFile file(path);
  EDET_CHECK(file.ok, "edet_net_load_state: cannot open %s", path);
  plan_file::StateFile sf;
  std::string err;
  EDET_CHECK(plan_file::parse_state(file.data, file.size, &sf, &err), "edet_net_load_state: %s: %s", path, err.c_str());
  // pass 1: every record against the plan; nothing on the device changes unless the whole file is good
  std::vector<char> seen(net->vars.size() * NUM_SLOTS, 0);
  EDET_CHECK(sf.records.size() <= seen.size(), "edet_net_load_state: %s holds %u records, the plan has %llu variable slots", path,
             (unsigned)sf.records.size(), (unsigned long long)seen.size());
  std::vector<const Var*> var_of;
  for (const plan_file::StateRecord& rec : sf.records) {
    const char* name = rec.name.c_str();
    auto it = net->var_index.find(rec.name);
    EDET_CHECK(it != net->var_index.end(), "edet_net_load_state: the plan has no variable '%s'", name);
    const Var& v = net->vars[(size_t)it->second];
    EDET_CHECK(rec.slot < NUM_SLOTS && has_slot(net, v, rec.slot), "edet_net_load_state: variable '%s' has no slot %d in this plan",
               name, rec.slot);
    EDET_CHECK(rec.count == v.count, "edet_net_load_state: variable '%s' has %llu elements, the file holds %llu", name,
               (unsigned long long)v.count, (unsigned long long)rec.count);
    bool same = rec.rank == v.rank;
    for (int d = 0; same && d < rec.rank; ++d) same = rec.dims[d] == (uint64_t)v.dims[d];
    EDET_CHECK(same, "edet_net_load_state: variable '%s': the shape in the file differs from the plan's", name);
    char& mark = seen[(size_t)it->second * NUM_SLOTS + rec.slot];
    EDET_CHECK(!mark, "edet_net_load_state: variable '%s' comes twice in slot %s", name, kSlotNames[rec.slot]);
    mark = 1;
    var_of.push_back(&v);
  }
  for (size_t i = 0; i < net->vars.size(); ++i)
    for (int slot = 0; slot < NUM_SLOTS; ++slot)
      EDET_CHECK(seen[i * NUM_SLOTS + slot] || !has_slot(net, net->vars[i], slot),
                 "edet_net_load_state: %s does not hold the %s of variable '%s'", path, kSlotNames[slot], net->vars[i].name.c_str());
  // pass 2: the payloads, straight from the mapped file
  for (size_t i = 0; i < sf.records.size(); ++i) {
    float* p = slot_ptr(net, *var_of[i], sf.records[i].slot, "edet_net_load_state");
    if (!p || edet_copy_to_device(p, sf.records[i].data, (size_t)sf.records[i].count * 4) != 0) return -1;
  }
  net->iterations = sf.iterations;
  return 0;
}

extern "C" int edet_dp_init(edet_net_t* net, edet_allreduce_fn fn, void* ctx) {
  EDET_CHECK(net, "edet_dp_init: null network");
  Program* p = find_program(net, "train_step");
  EDET_CHECK(p, "edet_dp_init: the plan holds no training step");
  net->allreduce = fn;
  net->allreduce_ctx = ctx;
  if (p->exec) {      // the captured step was recorded without / with another exchange: capture again at the next run
    (void)hipGraphExecDestroy(p->exec);
    (void)hipGraphDestroy(p->graph);
    p->exec = nullptr;
    p->graph = nullptr;
  }
  return 0;
}

// tf2/anchors.py:117-165 (Anchors._generate_configs / _generate_boxes) with utils.get_feat_sizes (utils.py:497-526); float64
// arithmetic in the reference's order of operations, cast to float32 at the end.
extern "C" int edet_anchors(int min_level, int max_level, int num_scales, const double* aspect_ratios, int num_aspects,
                            double anchor_scale, int image_height, int image_width, float* boxes_out, int64_t capacity,
                            int64_t* count) {
  EDET_CHECK(min_level >= 0 && max_level >= min_level && max_level < 16 && num_scales > 0 && aspect_ratios && num_aspects > 0 &&
             image_height > 0 && image_width > 0 && count, "edet_anchors: bad arguments");
  int fh[17], fw[17];
  fh[0] = image_height;
  fw[0] = image_width;
  for (int l = 1; l <= max_level; ++l) {
    fh[l] = (fh[l - 1] - 1) / 2 + 1;
    fw[l] = (fw[l - 1] - 1) / 2 + 1;
  }
  int64_t n = 0;
  for (int level = min_level; level <= max_level; ++level) {
    const double sy = (double)fh[0] / (double)fh[level], sx = (double)fw[0] / (double)fw[level];
    // np.arange(stride / 2, image_size, stride): ceil((stop - start) / step) samples start + i * step
    const int64_t ny = (int64_t)ceil(((double)image_height - sy / 2) / sy), nx = (int64_t)ceil(((double)image_width - sx / 2) / sx);
    const int A = num_scales * num_aspects;
    if (boxes_out) {
      EDET_CHECK(n + ny * nx * A <= capacity, "edet_anchors: capacity %lld boxes is too small", (long long)capacity);
      for (int octave = 0; octave < num_scales; ++octave) {
        for (int ai = 0; ai < num_aspects; ++ai) {
          const double octave_scale = (double)octave / (double)num_scales;
          const double base_x = anchor_scale * sx * pow(2.0, octave_scale);
          const double base_y = anchor_scale * sy * pow(2.0, octave_scale);
          const double ax = sqrt(aspect_ratios[ai]), ay = 1.0 / ax;
          const double half_x = base_x * ax / 2.0, half_y = base_y * ay / 2.0;
          const int a = octave * num_aspects + ai;
          for (int64_t y = 0; y < ny; ++y) {
            const double yv = sy / 2 + (double)y * sy;
            for (int64_t x = 0; x < nx; ++x) {
              const double xv = sx / 2 + (double)x * sx;
              float* o = boxes_out + 4 * (n + (y * nx + x) * A + a);
              o[0] = (float)(yv - half_y);
              o[1] = (float)(xv - half_x);
              o[2] = (float)(yv + half_y);
              o[3] = (float)(xv + half_x);
            }
          }
        }
      }
    }
    n += ny * nx * A;
  }
  *count = n;
  return 0;
}
