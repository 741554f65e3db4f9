// The bf16 depthwise family: the host entry points of the row-marching kernels (dw_march.hip) that the dispatch in dwconv.hip
// tries first, and the helpers those kernels share with the fused MBConv head (mbconv_fused.hip), whose second half is the
// same march.
#pragma once
#include "common.h"

// ---- row-marching kernels (dw_march.hip).  Every function returns 1 = handled, 0 = the call lies outside its envelope
// (nothing was launched: the caller goes on to the generic kernels of dwconv.hip), < 0 = error (edet_set_error has the text).
// forward (k_fwd_v2); *nparts_out = rows written to stat_partials
int dwm_try_fwd(const edet_tview_t* in, const float* weight, int k, int s, void* out, int ldo,
                float* stat_partials, int* nparts_out, hipStream_t st);
// weight gradient (k_wgrad_lx): partial sums in the workspace, added into dweight [k][k][c] fp32 in a fixed order
int dwm_try_wgrad(const edet_tview_t* in, const edet_gview_t* dy, int k, int s, float* dweight, void* workspace,
                  size_t workspace_bytes, hipStream_t st);
// data gradient (k_dgrad_lx); *nparts_out = rows written to epi->stat_partials
int dwm_try_dgrad(const edet_gview_t* dy, const float* weight, int k, int s, const edet_tview_t* in,
                  const edet_bwd_epi_t* epi, int* nparts_out, hipStream_t st);
// both gradients from one read of (dz, y, x) (k_bwd_one, any stride); 0: the caller runs the two functions above
int dwm_try_bwd_fused(const edet_gview_t* dy, const float* weight, int k, int s, const edet_tview_t* in,
                      const edet_bwd_epi_t* epi, int* nparts_out, float* dweight, void* workspace,
                      size_t workspace_bytes, hipStream_t st);

// Rows per tile of a march over `space_h` rows: balanced tiles of at most 80 rows on the 160 / 320-row maps, 40 below (fixed
// 32-row tiles left a short last tile that still pays the K - 1 halo rows and the pipeline fill; taller tiles than this leave
// the 80-row maps with too few tiles to fill the chip).  r02i / r02j lab, 15 depthwise layer shapes of D0 640x640 batch 128:
// backward 12.08 -> 11.49 (40) -> 10.81 ms (80), forward 5.08 -> 4.71 -> 4.59 ms.
// slack_h: rows of the marched space beyond the map (the padding rows of k_bwd_one's shifted row space) that must not cost an
// extra tile
inline int dw_row_tile(int space_h, int slack_h = 0) {
  const int cap = space_h >= 160 ? 80 : 40;
  const int nt = max(1, (space_h - slack_h + cap - 1) / cap);
  return (space_h + nt - 1) / nt;
}

// ---- device helpers of the march
namespace dwi {

typedef float f2 __attribute__((ext_vector_type(2)));      // two adjacent channels: v_pk_fma_f32 on naturally paired registers

__host__ __device__ constexpr int gcd_(int x, int y) { return y == 0 ? x : gcd_(y, x % y); }
// floor(a / b), ceil(a / b), b > 0
__host__ __device__ constexpr int fdiv_(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
__host__ __device__ constexpr int cdiv_(int a, int b) { return -fdiv_(-a, b); }
// static slot of a (possibly negative) relative row among n rotating accumulators
__host__ __device__ constexpr int slot_of(int rel, int n) { return ((rel % n) + n) % n; }

// a uniform "lo <= v < lo + span" as one unsigned compare
struct URange {
  int lo; uint32_t span;
  __device__ __forceinline__ void set(int l, int h) { lo = l; span = h > l ? (uint32_t)(h - l) : 0u; }
  __device__ __forceinline__ bool has(int v) const { return (uint32_t)(v - lo) < span; }
};

// Raw buffer access: address = descriptor base (4 SGPRs, uniform: the image) + soff (SGPR, uniform: the row) + voff (one
// VGPR, the thread's column / channel offset, constant over a tile) -- no VALU address arithmetic per load.  (Plain
// pointers did not get there: the compiler widened the hoisted 32-bit offsets to 64-bit VGPR pairs and added the row
// pointer on the VALU, two to four instructions per load.)  num_records = 2^31 - 1: the range check is not used by the
// loads -- rows and columns are clamped by the caller -- and an offset of 2^31 and above is a store the hardware drops.
typedef __amdgpu_buffer_rsrc_t brsrc_t;
__device__ __forceinline__ brsrc_t make_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}

// NV 2-vectors of adjacent bf16 channels as they lie in memory, and their way through registers and LDS
template <int NV> struct RawV { uint32_t u[NV]; };
template <int NV> __device__ __forceinline__ RawV<NV> ldg(brsrc_t r, uint32_t voff, uint32_t soff);
template <> __device__ __forceinline__ RawV<1> ldg<1>(brsrc_t r, uint32_t voff, uint32_t soff) {
  RawV<1> v; v.u[0] = __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0); return v;
}
template <> __device__ __forceinline__ RawV<2> ldg<2>(brsrc_t r, uint32_t voff, uint32_t soff) {
  const auto t = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
  RawV<2> v; v.u[0] = t[0]; v.u[1] = t[1]; return v;
}
template <int NV> __device__ __forceinline__ void unpackv(const RawV<NV>& r, f2 (&x)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    x[i].x = __uint_as_float(r.u[i] << 16);
    x[i].y = __uint_as_float(r.u[i] & 0xffff0000u);
  }
}
template <int NV> __device__ __forceinline__ void stg(brsrc_t r, uint32_t voff, uint32_t soff, const f2 (&x)[NV]);
template <> __device__ __forceinline__ void stg<1>(brsrc_t r, uint32_t voff, uint32_t soff, const f2 (&x)[1]) {
  __builtin_amdgcn_raw_buffer_store_b32(pack2bf(x[0].x, x[0].y), r, voff, soff, 0);
}
template <> __device__ __forceinline__ void stg<2>(brsrc_t r, uint32_t voff, uint32_t soff, const f2 (&x)[2]) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  u2 o; o[0] = pack2bf(x[0].x, x[0].y); o[1] = pack2bf(x[1].x, x[1].y);
  __builtin_amdgcn_raw_buffer_store_b64(o, r, voff, soff, 0);
}
template <int NV> __device__ __forceinline__ void lds_putv(float* p, const f2 (&x)[NV]);
template <> __device__ __forceinline__ void lds_putv<1>(float* p, const f2 (&x)[1]) { *reinterpret_cast<f2*>(p) = x[0]; }
template <> __device__ __forceinline__ void lds_putv<2>(float* p, const f2 (&x)[2]) {
  *reinterpret_cast<float4*>(p) = make_float4(x[0].x, x[0].y, x[1].x, x[1].y);
}
template <int NV> __device__ __forceinline__ void lds_getv(const float* p, f2 (&x)[NV]);
template <> __device__ __forceinline__ void lds_getv<1>(const float* p, f2 (&x)[1]) { x[0] = *reinterpret_cast<const f2*>(p); }
template <> __device__ __forceinline__ void lds_getv<2>(const float* p, f2 (&x)[2]) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  x[0].x = v.x; x[0].y = v.y; x[1].x = v.z; x[1].y = v.w;
}
// fp32 per-channel coefficients
template <int NV> __device__ __forceinline__ void loadv(const float* p, f2 (&x)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) x[i] = *reinterpret_cast<const f2*>(p + 2 * i);
}

}  // namespace dwi
