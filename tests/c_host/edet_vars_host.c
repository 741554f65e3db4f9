/* A host WITHOUT an interpreter that works on a network's variables BY NAME: lists them, sets one and watches the logits
 * move, trains, saves the state it trained and resumes from it in another process (include/edet_net.h:
 * edet_net_variable_info / edet_set_variable / edet_net_save_state / edet_net_load_state).  C99, links libedet_hip.so and the
 * HIP runtime only; tests/test_plan_vars_gpu.py compares what it dumps.
 *   edet_vars_host list PLAN
 *   edet_vars_host setvar PLAN OUTDIR NAME VALUE       class logits before (".before") and after (".after") the write
 *   edet_vars_host train PLAN OUTDIR N [STATE_IN|-] [STATE_OUT|-]   N steps at a fixed rate and decay
 * Inputs: the plan's recorded ones, or -- a plan recorded with keep_inputs=False -- OUTDIR/<buffer>.in for every named
 * buffer that has such a file ("/" and ":" of the name written as "_").  */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../../include/edet_hip.h"
#include "../../include/edet_net.h"

#define LEARNING_RATE 0.015625f
#define EMA_DECAY 0.875f

#define CHECK(call)                                                              \
  do {                                                                           \
    if ((call) != 0) {                                                           \
      fprintf(stderr, "%s failed: %s\n", #call, edet_last_error());             \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

static void file_name(char* path, size_t cap, const char* dir, const char* name, const char* suffix) {
  snprintf(path, cap, "%s/%s%s", dir, name, suffix);
  for (char* c = path + strlen(dir) + 1; *c; ++c)
    if (*c == ':' || *c == '/') *c = '_';
}

static int dump(edet_net_t* net, const char* name, const char* dir, const char* suffix) {
  void* p = NULL;
  size_t n = 0;
  char path[1024];
  if (edet_net_buffer(net, name, &p, &n) != 0) return 1;
  void* host = malloc(n ? n : 1);
  if (!host || edet_copy_to_host(host, p, n) != 0) return 1;
  file_name(path, sizeof(path), dir, name, suffix);
  FILE* f = fopen(path, "wb");
  if (!f) return 1;
  const size_t done = fwrite(host, 1, n, f);
  fclose(f);
  free(host);
  return done == n ? 0 : 1;
}

/* fills every named buffer that has a file OUTDIR/<name>.in of exactly its size */
static int load_inputs(edet_net_t* net, const char* dir) {
  const int count = edet_net_num_buffers(net);
  for (int i = 0; i < count; ++i) {
    const char* name = edet_net_buffer_name(net, i);
    char path[1024];
    void* p = NULL;
    size_t n = 0;
    file_name(path, sizeof(path), dir, name, ".in");
    FILE* f = fopen(path, "rb");
    if (!f) continue;
    if (edet_net_buffer(net, name, &p, &n) != 0) return 1;
    void* host = malloc(n + 1);
    const size_t got = host ? fread(host, 1, n + 1, f) : 0;
    fclose(f);
    if (got != n) {
      fprintf(stderr, "%s: %lu bytes, the buffer holds %lu\n", path, (unsigned long)got, (unsigned long)n);
      return 1;
    }
    if (edet_copy_to_device(p, host, n) != 0) return 1;
    free(host);
  }
  return 0;
}

static int dump_class_logits(edet_net_t* net, const char* dir, const char* suffix) {
  int64_t min_level = 0, max_level = 0;
  char name[64];
  CHECK(edet_net_property(net, "min_level", &min_level));
  CHECK(edet_net_property(net, "max_level", &max_level));
  for (int64_t l = min_level; l <= max_level; ++l) {
    snprintf(name, sizeof(name), "cls_outputs_%d", (int)l);
    if (dump(net, name, dir, suffix)) return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s list PLAN | setvar PLAN OUTDIR NAME VALUE | train PLAN OUTDIR N [STATE_IN|-] [STATE_OUT|-]\n", argv[0]);
    return 2;
  }
  const char* mode = argv[1];
  edet_net_t* net = NULL;
  hipStream_t stream;
  if (hipStreamCreate(&stream) != hipSuccess) return 1;
  CHECK(edet_create(argv[2], &net));
  if (strcmp(mode, "list") == 0) {
    int64_t count = 0;
    CHECK(edet_net_num_variables(net, &count));
    for (int64_t i = 0; i < count; ++i) {
      edet_var_info v;
      CHECK(edet_net_variable_info(net, i, &v));
      printf("%s %d", v.name, (int)v.rank);
      for (int d = 0; d < v.rank; ++d) printf("%s%lld", d ? "x" : " ", (long long)v.dims[d]);
      if (v.rank == 0) printf(" -");
      printf(" %d\n", (int)v.trainable);
    }
  } else if (strcmp(mode, "setvar") == 0 && argc >= 6) {
    const char* dir = argv[3];
    int64_t index = 0;
    edet_var_info v;
    if (load_inputs(net, dir)) return 1;
    CHECK(edet_forward(net, stream));
    if (hipStreamSynchronize(stream) != hipSuccess) return 1;
    if (dump_class_logits(net, dir, ".before.bin")) return 1;
    CHECK(edet_net_find_variable(net, argv[4], &index));
    CHECK(edet_net_variable_info(net, index, &v));
    float* values = (float*)malloc((size_t)(v.count ? v.count : 1) * sizeof(float));
    if (!values) return 1;
    for (int64_t i = 0; i < v.count; ++i) values[i] = (float)atof(argv[5]);
    CHECK(edet_set_variable(net, argv[4], EDET_SLOT_VALUE, values, v.count));
    free(values);
    CHECK(edet_forward(net, stream));
    if (hipStreamSynchronize(stream) != hipSuccess) return 1;
    if (dump_class_logits(net, dir, ".after.bin")) return 1;
  } else if (strcmp(mode, "train") == 0 && argc >= 5) {
    const char* dir = argv[3];
    const int steps = atoi(argv[4]);
    const char* state_in = argc > 5 && strcmp(argv[5], "-") != 0 ? argv[5] : NULL;
    const char* state_out = argc > 6 && strcmp(argv[6], "-") != 0 ? argv[6] : NULL;
    void* p = NULL;
    size_t n = 0;
    int64_t iterations = 0;
    char path[1024];
    if (load_inputs(net, dir)) return 1;
    if (state_in) CHECK(edet_net_load_state(net, state_in));
    CHECK(edet_net_use_graph(net, 1));
    for (int s = 0; s < steps; ++s) CHECK(edet_train_step(net, LEARNING_RATE, EMA_DECAY, stream));
    if (hipStreamSynchronize(stream) != hipSuccess) return 1;
    if (state_out) CHECK(edet_net_save_state(net, state_out));
    const char* state[] = {"params", "ema", "velocity", "bn_state", "loss_sums"};
    for (int k = 0; k < 5; ++k)
      if (dump(net, state[k], dir, ".bin")) return 1;
    if (edet_net_buffer(net, "adam_v", &p, &n) == 0 && dump(net, "adam_v", dir, ".bin")) return 1;
    CHECK(edet_net_get_iterations(net, &iterations));
    snprintf(path, sizeof(path), "%s/iterations.txt", dir);
    FILE* f = fopen(path, "w");
    if (!f) return 1;
    fprintf(f, "%lld\n", (long long)iterations);
    fclose(f);
  } else {
    fprintf(stderr, "%s: unknown mode or too few arguments\n", mode);
    return 2;
  }
  CHECK(edet_destroy(net));
  printf("edet_vars_host: %s ok\n", mode);
  return 0;
}
