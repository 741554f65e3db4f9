// Shared device helpers for the gfx950 EfficientDet kernels (wave64, NHWC, fp32 math).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/edet_hip.h"

typedef uint16_t bf16_t;  // raw bfloat16 bits
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// ---------------------------------------------------------------- error handling
void edet_set_error(const char* fmt, ...);
#define EDET_CHECK(cond, ...)            \
  do {                                   \
    if (!(cond)) {                       \
      edet_set_error(__VA_ARGS__);       \
      return -1;                         \
    }                                    \
  } while (0)
#define EDET_LAUNCH_CHECK(name)                                          \
  do {                                                                   \
    hipError_t e_ = hipGetLastError();                                   \
    if (e_ != hipSuccess) {                                              \
      edet_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
      return -2;                                                         \
    }                                                                    \
  } while (0)

// ---------------------------------------------------------------- kernel launches
// Every kernel of the library is launched through edet_launch, so that the debug launch log
// (edet_debug_launch_log / edet_debug_launch_names in include/edet_hip.h) can name the kernel symbols a run
// used: the parity tests assert that every symbol of the full-size benchmark step is also launched by a
// test that checks results against the oracle.  With the log off the cost is one predictable branch.
#include <tuple>
#include <utility>
extern int g_edet_launch_log_on;
void edet_log_launch(const void* host_fn);
template <typename Tuple, size_t... I>
inline hipError_t edet_launch_impl(const void* fn, dim3 grid, dim3 block, size_t lds, hipStream_t st, Tuple& params,
                                   std::index_sequence<I...>) {
  void* ptrs[] = {static_cast<void*>(&std::get<I>(params))..., nullptr};
  return hipLaunchKernel(fn, grid, block, ptrs, lds, st);
}
// kern<<<grid, block, lds, st>>>(args...) with the arguments converted to the kernel's parameter types
template <typename... KArgs, typename... Args>
inline void edet_launch(void (*kern)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t st, Args&&... args) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "edet_launch: wrong number of kernel arguments");
  const void* fn = reinterpret_cast<const void*>(kern);
  if (g_edet_launch_log_on) edet_log_launch(fn);
  std::tuple<typename std::decay<KArgs>::type...> params(static_cast<KArgs>(args)...);
  (void)edet_launch_impl(fn, grid, block, lds, st, params, std::index_sequence_for<KArgs...>{});
}

// ---------------------------------------------------------------- scalar conversions
__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
// round-to-nearest-even fp32 -> bf16: gfx950 has v_cvt_pk_bf16_f32, which the compiler selects for a
// plain float -> __bf16 conversion (one instruction per two elements)
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
  bf16x2_t v;
  v[0] = (__bf16)lo;
  v[1] = (__bf16)hi;
  return __builtin_bit_cast(uint32_t, v);
}

template <typename T> __device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<bf16_t>(bf16_t v) { return bf2f(v); }
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f<bf16_t>(float v) { return f2bf(v); }

// ---------------------------------------------------------------- 8 bf16 in 16 bytes <-> 8 floats
__device__ __forceinline__ void unpack8(const uint4 raw, float x[8]) {
  x[0] = __uint_as_float(raw.x << 16); x[1] = __uint_as_float(raw.x & 0xffff0000u);
  x[2] = __uint_as_float(raw.y << 16); x[3] = __uint_as_float(raw.y & 0xffff0000u);
  x[4] = __uint_as_float(raw.z << 16); x[5] = __uint_as_float(raw.z & 0xffff0000u);
  x[6] = __uint_as_float(raw.w << 16); x[7] = __uint_as_float(raw.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 pack8(const float x[8]) {
  uint4 o;
  o.x = pack2bf(x[0], x[1]); o.y = pack2bf(x[2], x[3]);
  o.z = pack2bf(x[4], x[5]); o.w = pack2bf(x[6], x[7]);
  return o;
}

// ---------------------------------------------------------------- 8-element vector I/O
// p must be 16-byte aligned for bf16 (8 elems) and fp32 (2 x float4).
template <typename T> __device__ __forceinline__ void load8(const T* p, float v[8]);
template <> __device__ __forceinline__ void load8<float>(const float* p, float v[8]) {
  float4 a = *reinterpret_cast<const float4*>(p);
  float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float v[8]) {
  unpack8(*reinterpret_cast<const uint4*>(p), v);
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float v[8]);
template <> __device__ __forceinline__ void store8<float>(float* p, const float v[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float v[8]) {
  *reinterpret_cast<uint4*>(p) = pack8(v);
}
__device__ __forceinline__ void loadf8(const float* p, float v[8]) { load8<float>(p, v); }

// ---------------------------------------------------------------- 4-element vector I/O
// 8-byte aligned for bf16, 16-byte aligned for fp32.
template <typename T> __device__ __forceinline__ void load4(const T* p, float v[4]);
template <> __device__ __forceinline__ void load4<float>(const float* p, float v[4]) {
  float4 a = *reinterpret_cast<const float4*>(p);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
template <> __device__ __forceinline__ void load4<bf16_t>(const bf16_t* p, float v[4]) {
  uint2 a = *reinterpret_cast<const uint2*>(p);
  v[0] = __uint_as_float(a.x << 16); v[1] = __uint_as_float(a.x & 0xffff0000u);
  v[2] = __uint_as_float(a.y << 16); v[3] = __uint_as_float(a.y & 0xffff0000u);
}
template <typename T> __device__ __forceinline__ void store4(T* p, const float v[4]);
template <> __device__ __forceinline__ void store4<float>(float* p, const float v[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void store4<bf16_t>(bf16_t* p, const float v[4]) {
  uint2 a;
  a.x = pack2bf(v[0], v[1]); a.y = pack2bf(v[2], v[3]);
  *reinterpret_cast<uint2*>(p) = a;
}

// ---------------------------------------------------------------- activations
// v_exp_f32 + v_rcp_f32 (1 ulp each); a full-precision divide would cost ~10 more VALU instructions
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float swishf_(float x) { return x * sigmoidf_(x); }
// d/dx x*sigmoid(x) = s * (1 + x * (1 - s))
__device__ __forceinline__ float swish_gradf_(float x) {
  float s = sigmoidf_(x);
  return s * (1.0f + x * (1.0f - s));
}

// The other activation types of utils.activation_fn (act > EDET_ACT_SWISH): relu, relu6, hswish, mish, srelu.
// Derivatives as TensorFlow's gradient kernels define them at the kinks (ReluGrad: x > 0; Relu6Grad: 0 < x < 6).
// mish: tanh(softplus(z)) = w / (w + 2) with w = e^z (e^z + 2) (exact identity; z > 20: 1 to fp32 precision).
// srelu (utils.srelu_fn, utils.py:25-31): beta = (20^2)^2 -- the reference makes its `srelu_beta` variable afresh, at 20.0,
// in every call, so it is a constant of the graph, not a trained value.
constexpr float SRELU_BETA = 160000.f;
__device__ __forceinline__ float act_other_(int act, float z) {
  if (act == EDET_ACT_RELU) return fmaxf(z, 0.f);
  if (act == EDET_ACT_RELU6) return fminf(fmaxf(z, 0.f), 6.f);
  if (act == EDET_ACT_HSWISH) return z * fminf(fmaxf(z + 3.f, 0.f), 6.f) / 6.f;
  if (act == EDET_ACT_MISH) {
    if (z > 20.f) return z;
    const float n = __expf(z), w = n * (n + 2.f);
    return z * w / (w + 2.f);
  }
  if (!(z > 0.f)) return 0.f;
  // u = beta z below 1/16: z - log(1 + u) / beta cancels to u^2 / (2 beta) and 1 + u loses u altogether below 2^-24 --
  // the series of u - log(1 + u) instead (next term u^6 / 6: 2^-17 of the result)
  const float u = SRELU_BETA * z;
  if (u < 0.0625f) return z * u * (0.5f - u * ((1.f / 3.f) - u * (0.25f - u * 0.2f)));
  return z - __logf(fmaf(SRELU_BETA, z, 1.f)) * (1.f / SRELU_BETA);
}
__device__ __forceinline__ float act_other_grad_(int act, float z) {
  if (act == EDET_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  if (act == EDET_ACT_RELU6) return (z > 0.f && z < 6.f) ? 1.f : 0.f;
  if (act == EDET_ACT_HSWISH) return z <= -3.f ? 0.f : (z >= 3.f ? 1.f : (2.f * z + 3.f) / 6.f);
  if (act == EDET_ACT_MISH) {
    if (z > 20.f) return 1.f;
    // t + z (1 - t^2) sigmoid(z), with 1 - t^2 = 4 (w + 1) / (w + 2)^2: taken from a rounded t it is a difference of two
    // numbers next to 1 for z > 8, and z times the rounding of t reached 22 ulps of the result
    const float n = __expf(z), w = n * (n + 2.f), r = 1.f / (w + 2.f), t = w * r;
    return fmaf(z * (4.f * (w + 1.f) * r * r), n / (1.f + n), t);
  }
  // beta z / (1 + beta z): 1 - 1 / (1 + beta z) is 0 for every beta z below 2^-24
  if (!(z > 0.f)) return 0.f;
  const float u = SRELU_BETA * z;
  return u / (1.f + u);
}
// any activation code (kernel-uniform): value and derivative
__device__ __forceinline__ float act_apply_(int act, float z) {
  return act == EDET_ACT_SWISH ? swishf_(z) : (act == EDET_ACT_NONE ? z : act_other_(act, z));
}
__device__ __forceinline__ float act_grad_(int act, float z) {
  return act == EDET_ACT_SWISH ? swish_gradf_(z) : (act == EDET_ACT_NONE ? 1.f : act_other_grad_(act, z));
}

// Activated-view element transform for 8 consecutive channels starting at c0.
// img = image index of the row (only used when gate != NULL).
struct ViewCoef {
  float scale[8], shift[8];
};
__device__ __forceinline__ void view_load_coef(const edet_tview_t& v, int c0, ViewCoef& k) {
  if (v.scale) {
    loadf8(v.scale + c0, k.scale);
    loadf8(v.shift + c0, k.shift);
  }
}
// x (raw) -> z (pre-activation) -> value
__device__ __forceinline__ void view_apply(const edet_tview_t& v, const ViewCoef& k, int c0,
                                           int img, float x[8]) {
  if (v.scale) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = fmaf(x[e], k.scale[e], k.shift[e]);
  }
  if (v.act == EDET_ACT_SWISH) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = swishf_(x[e]);
  } else if (v.act > EDET_ACT_SWISH) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = act_other_(v.act, x[e]);
  }
  if (v.gate) {
    float g[8];
    loadf8(v.gate + (size_t)img * v.c + c0, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] *= g[e];
  }
}

struct GradCoef {
  float a[8], b[8], cc[8];
};
__device__ __forceinline__ void grad_load_coef(const edet_gview_t& g, int c0, GradCoef& k) {
  if (g.a) {
    loadf8(g.a + c0, k.a);
    loadf8(g.b + c0, k.b);
    loadf8(g.cc + c0, k.cc);
  }
}
// loads dy for 8 channels at element offset `off` (= row*ld + c0)
template <typename T>
__device__ __forceinline__ void grad_load(const edet_gview_t& g, const GradCoef& k, size_t off,
                                          float dy[8]) {
  load8<T>(reinterpret_cast<const T*>(g.dz) + off, dy);
  if (g.a) {
    float y[8];
    load8<T>(reinterpret_cast<const T*>(g.y) + off, y);
#pragma unroll
    for (int e = 0; e < 8; ++e) dy[e] = fmaf(k.a[e], dy[e], fmaf(k.b[e], y[e], k.cc[e]));
  }
}

// ---------------------------------------------------------------- ordered (run-to-run identical) sums
// Sum of v[] over the lanes of a wave that share lane % group (group: a power of two <= 64), by an xor butterfly:
// a fixed tree, so the same bits on every run; afterwards every lane of a class holds the class total.  All 64 lanes
// must be active at the call.  Used by the fp32 / generic kernels instead of LDS atomics; the waves of a workgroup then
// add their totals into LDS one wave after the other (wave order), and workgroups hand partial rows to
// edet_reduce_partials -- no floating-point atomics anywhere on the way.  The same holds for the SE gate gradient: a data-
// gradient kernel given epi.dgate stores the gradient of the gated value as it is, and its dispatch forms the sums afterwards
// from the stored gradient (k_gate_sums in pw_gemm.hip: one writer per element, a fixed order).  No kernel adds to dgate with
// a global atomic (tests/test_abi.py scans the sources for it).
template <int NV>
__device__ __forceinline__ void wave_group_sum(float (&v)[NV], int group) {
  for (int off = group; off < 64; off <<= 1) {
#pragma unroll
    for (int e = 0; e < NV; ++e) v[e] += __shfl_xor(v[e], off, 64);
  }
}

// TF 'SAME' geometry
__host__ __device__ inline int same_out(int in, int s) { return (in + s - 1) / s; }
__host__ __device__ inline int same_pad_before(int in, int k, int s) {
  int out = (in + s - 1) / s;
  int total = (out - 1) * s + k - in;
  if (total < 0) total = 0;
  return total / 2;
}

// dst[i] += sum_p ws[p*n + i]  (p < P): 16 elements x 64 partial-row slices per workgroup (reduce.hip); recorded for one
// batched launch instead while edet_reduce_defer is on for the stream
int edet_reduce_partials(const float* ws, int P, int64_t n, float* dst, hipStream_t st);
int edet_reduce_partials_set(const float* ws, int P, int64_t n, float* dst, hipStream_t st);
// two destinations: dst_a[i] += column i for i < n_a (dst_a may be NULL), dst_b[i - n_a] += column i for n_a <= i < n
int edet_reduce_partials2(const float* ws, int P, int64_t n, float* dst_a, int64_t n_a, float* dst_b, hipStream_t st);

// Lets kernel `kern` be launched with `bytes` of dynamic LDS: above 64 KiB a kernel has to opt in.  The runtime is asked once
// per kernel (again only if a later launch needs more); false = it refused.  (error.cpp)
bool edet_lds_optin(const void* kern, size_t bytes);
template <typename... KArgs> inline bool edet_lds_optin(void (*kern)(KArgs...), size_t bytes) {
  return edet_lds_optin(reinterpret_cast<const void*>(kern), bytes);
}

// workgroups of kernel `fn` (block size `threads`, `lds` bytes of dynamic LDS) the device holds at once; 0 = unknown
int edet_resident_wgs(const void* fn, int threads, size_t lds);

// The implementation selectors the parity tests set to reach a reference path, read per call:
// the integer value of environment variable `name`, or `dflt` when it is unset or empty
static inline int edet_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return (e && e[0]) ? atoi(e) : dflt;
}

// f(type_tag<T>{}) with T the storage type of the runtime `dtype`; false (nothing called) = not a dtype
template <typename T> struct type_tag { using type = T; };
template <typename F> inline bool dtype_dispatch(int dtype, F&& f) {
  if (dtype == EDET_BF16) return f(type_tag<bf16_t>{}), true;
  if (dtype == EDET_F32) return f(type_tag<float>{}), true;
  return false;
}

static inline hipStream_t to_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// grid of a one-dimensional grid-stride kernel with 256-lane workgroups: one thread per item, at most `cap` workgroups (the
// caps are the callers' own; rowmap_impl.h's ew_grid sizes by residency instead)
static inline unsigned flat_grid(int64_t count, int64_t cap) {
  const int64_t g = (count + 255) / 256;
  return (unsigned)(g < cap ? g : cap);
}
