// Plain data movement: casts (fp32 -> storage type, flat, as a padded / transposed matrix, a whole plan in one launch; bf16
// -> fp32), row compaction, zero fill and accumulate-and-clear.  Step plumbing that used to be torch calls (round 6: every
// launch of a step goes through this ABI, so that a step can be recorded and replayed by a host without a Python
// interpreter: net_runtime.cpp).
#include "common.h"

namespace {

constexpr int THREADS = 256;

template <typename T>
__global__ void k_cast(const float* __restrict__ src, T* __restrict__ dst, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = from_f<T>(src[i]);
}

// dst[r][c] (ld_out, zero padded) = src[r][c]            (transpose == 0, dst rows = rows)
// dst[c][r] (ld_out, zero padded) = src[r][c]            (transpose == 1, dst rows = cols)
template <typename T>
__global__ void k_cast_matrix(const float* __restrict__ src, T* __restrict__ dst, int rows, int cols,
                              int ld_out, int transpose) {
  const int drows = transpose ? cols : rows;
  const int dcols = transpose ? rows : cols;
  const int64_t total = (int64_t)drows * ld_out;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / ld_out), c = (int)(i - (int64_t)r * ld_out);
    float v = 0.f;
    if (c < dcols) v = transpose ? src[(size_t)c * cols + r] : src[(size_t)r * cols + c];
    dst[i] = from_f<T>(v);
  }
}

// every item of a cast plan in one launch: blockIdx.y = item, blockIdx.x strides over its elements
template <typename T>
__global__ void k_cast_batch(const edet_cast_item_t* __restrict__ items) {
  const edet_cast_item_t it = items[blockIdx.y];
  const float* src = it.src;
  T* dst = reinterpret_cast<T*>(it.dst);
  const int drows = it.transpose ? it.cols : it.rows;
  const int dcols = it.transpose ? it.rows : it.cols;
  const int64_t total = (int64_t)drows * it.ld_out;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / it.ld_out), c = (int)(i - (int64_t)r * it.ld_out);
    float v = 0.f;
    if (c < dcols) v = it.transpose ? src[(size_t)c * it.cols + r] : src[(size_t)r * it.cols + c];
    dst[i] = from_f<T>(v);
  }
}

__global__ __launch_bounds__(THREADS) void k_widen_bf16(const bf16_t* __restrict__ src, float* __restrict__ dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride)
    dst[i] = __uint_as_float((uint32_t)src[i] << 16);
}

// dst[r][0 .. cw) = src[r][0 .. cw) in 4-byte words: a [rows][ld] tensor without its padding columns
__global__ __launch_bounds__(THREADS) void k_compact_rows(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                         int64_t rows, int cw, int ldw) {
  const int64_t total = rows * cw, stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / cw;
    dst[i] = src[r * ldw + (i - r * cw)];
  }
}

// A kernel, not hipMemsetAsync: a memset NODE of a captured graph costs a ~50 us bubble in front of it on this runtime
// (r06zz timeline: two fillBufferAligned nodes and the kernel behind them, 0.2 ms of idle queue per step)
__global__ __launch_bounds__(THREADS) void k_zero(uint4* __restrict__ dst16, size_t n16, unsigned char* __restrict__ tail, int ntail) {
  const size_t stride = (size_t)gridDim.x * THREADS;
  for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < n16; i += stride) dst16[i] = make_uint4(0, 0, 0, 0);
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0;
}

__global__ __launch_bounds__(THREADS) void k_axpy_clear(float* __restrict__ dst, float* __restrict__ src, int64_t n, int clear) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) {
    dst[i] += src[i];
    if (clear) src[i] = 0.f;
  }
}

}  // namespace

extern "C" int edet_cast(const float* src, void* dst, int64_t count, int dtype, void* stream) {
  EDET_CHECK(src && dst, "edet_cast: null pointer");
  if (count <= 0) return 0;
  EDET_CHECK(dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    edet_launch(k_cast<T>, dim3(flat_grid(count, 2048)), dim3(THREADS), 0, to_stream(stream), src, (T*)dst, count);
  }), "edet_cast: bad dtype %d", dtype);
  EDET_LAUNCH_CHECK("edet_cast");
  return 0;
}

extern "C" int edet_cast_matrix(const float* src, void* dst, int rows, int cols, int ld_out,
                                int transpose, int dtype, void* stream) {
  EDET_CHECK(src && dst, "edet_cast_matrix: null pointer");
  EDET_CHECK(ld_out >= (transpose ? rows : cols), "edet_cast_matrix: ld_out too small");
  const int64_t total = (int64_t)(transpose ? cols : rows) * ld_out;
  EDET_CHECK(dtype_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    edet_launch(k_cast_matrix<T>, dim3(flat_grid(total, 2048)), dim3(THREADS), 0, to_stream(stream), src, (T*)dst, rows, cols, ld_out,
                transpose);
  }), "edet_cast_matrix: bad dtype %d", dtype);
  EDET_LAUNCH_CHECK("edet_cast_matrix");
  return 0;
}

extern "C" int edet_cast_batch(const edet_cast_item_t* items_dev, int count, int max_blocks_per_item, int dtype,
                               void* stream) {
  EDET_CHECK(items_dev && count > 0 && max_blocks_per_item > 0, "edet_cast_batch: bad arguments");
  EDET_CHECK(dtype_dispatch(dtype, [&](auto t) {
    edet_launch(k_cast_batch<typename decltype(t)::type>, dim3(max_blocks_per_item, count), dim3(THREADS), 0, to_stream(stream), items_dev);
  }), "edet_cast_batch: bad dtype %d", dtype);
  EDET_LAUNCH_CHECK("edet_cast_batch");
  return 0;
}

extern "C" int edet_cast_to_f32(const void* src, float* dst, int64_t count, int src_dtype, void* stream) {
  EDET_CHECK(src && dst, "edet_cast_to_f32: null pointer");
  if (count <= 0) return 0;
  if (src_dtype == EDET_F32) {
    const hipError_t e = hipMemcpyAsync(dst, src, (size_t)count * 4, hipMemcpyDeviceToDevice, to_stream(stream));
    EDET_CHECK(e == hipSuccess, "edet_cast_to_f32: hipMemcpyAsync: %s", hipGetErrorString(e));
    return 0;
  }
  EDET_CHECK(src_dtype == EDET_BF16, "edet_cast_to_f32: bad dtype %d", src_dtype);
  edet_launch(k_widen_bf16, dim3(flat_grid(count, 4096)), dim3(THREADS), 0, to_stream(stream), (const bf16_t*)src, dst, count);
  EDET_LAUNCH_CHECK("edet_cast_to_f32");
  return 0;
}

extern "C" int edet_compact_rows(const void* src, int64_t rows, int c, int ld, void* dst, int elem_bytes, void* stream) {
  EDET_CHECK(src && dst && rows >= 0 && c > 0 && ld >= c, "edet_compact_rows: bad arguments");
  EDET_CHECK((elem_bytes == 2 || elem_bytes == 4) && (c * elem_bytes) % 4 == 0 && (ld * elem_bytes) % 4 == 0,
             "edet_compact_rows: rows must be whole 4-byte words (elem_bytes %d, c %d, ld %d)", elem_bytes, c, ld);
  if (rows == 0) return 0;
  const int cw = c * elem_bytes / 4, ldw = ld * elem_bytes / 4;
  edet_launch(k_compact_rows, dim3(flat_grid(rows * cw, 4096)), dim3(THREADS), 0, to_stream(stream), (const uint32_t*)src, (uint32_t*)dst,
              rows, cw, ldw);
  EDET_LAUNCH_CHECK("edet_compact_rows");
  return 0;
}

extern "C" int edet_zero(void* dst, size_t bytes, void* stream) {
  EDET_CHECK(dst || bytes == 0, "edet_zero: null pointer");
  if (bytes == 0) return 0;
  // head up to the first 16-byte boundary and tail behind the last one: byte stores of block 0 (at most 15 + 15)
  unsigned char* p = reinterpret_cast<unsigned char*>(dst);
  const size_t mis = (16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15;
  if (mis >= bytes || mis != 0) {
    // unaligned start (not what the engine passes: its buffers are 256-byte aligned): the memset path
    const hipError_t e = hipMemsetAsync(dst, 0, bytes, to_stream(stream));
    EDET_CHECK(e == hipSuccess, "edet_zero: hipMemsetAsync: %s", hipGetErrorString(e));
    return 0;
  }
  const size_t n16 = bytes / 16;
  const int ntail = (int)(bytes - n16 * 16);
  unsigned grid = flat_grid((int64_t)n16, 2048);
  if (grid < 1) grid = 1;          // fewer than 16 bytes: block 0 still writes the tail
  edet_launch(k_zero, dim3(grid), dim3(THREADS), 0, to_stream(stream), reinterpret_cast<uint4*>(p), n16, p + n16 * 16, ntail);
  EDET_LAUNCH_CHECK("edet_zero");
  return 0;
}

extern "C" int edet_axpy_clear(float* dst, float* src, int64_t n, int clear_src, void* stream) {
  EDET_CHECK(dst && src && n >= 0, "edet_axpy_clear: bad arguments");
  if (n == 0) return 0;
  edet_launch(k_axpy_clear, dim3(flat_grid(n, 2048)), dim3(THREADS), 0, to_stream(stream), dst, src, n, clear_src);
  EDET_LAUNCH_CHECK("edet_axpy_clear");
  return 0;
}
