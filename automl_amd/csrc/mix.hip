// Mixup and CutMix of a training batch on the device (efficientnetv2/datasets.py:191-301): the images in place, the
// sparse labels into dense fp32 soft labels.  The draws (mixup weights, cutmix boxes) are the caller's, in device memory, so
// that a replayed graph sees new ones.
//
// The batch is split as the reference's `mixing` splits it: rows [0, n_mixup) are mixed by mixup, rows [n_mixup, batch) by
// cutmix, each part with itself in reverse order (partner of mixup row i: n_mixup - 1 - i; of cutmix row i:
// n_mixup + batch - 1 - i).  Partners come in pairs, so one thread owns the same chunk of a row and of its partner, reads
// both and then writes both: that is all the in-place pass needs.  No reduction over floating-point values, no atomics.
#include "common.h"

namespace {

constexpr int THREADS = 256;

struct Box { int y1, x1, y2, x2; };
// y1, x1, y2, x2 (half-open) clamped to the image: a box from device memory can make no access leave the row
__device__ __forceinline__ Box load_box(const int32_t* __restrict__ boxes, int row, int h, int w) {
  Box b;
  b.y1 = min(max(boxes[row * 4 + 0], 0), h);
  b.x1 = min(max(boxes[row * 4 + 1], 0), w);
  b.y2 = min(max(boxes[row * 4 + 2], 0), h);
  b.x2 = min(max(boxes[row * 4 + 3], 0), w);
  if (b.y2 <= b.y1 || b.x2 <= b.x1) b.y1 = b.y2 = b.x1 = b.x2 = 0;      // empty
  return b;
}

template <typename T, int V> struct alignas(sizeof(T) * V) Chunk { T v[V]; };
template <typename T, int V> __device__ __forceinline__ Chunk<T, V> load_chunk(const T* p) {
  Chunk<T, V> c;
  if constexpr (V == 1) c.v[0] = *p;
  else *reinterpret_cast<uint4*>(c.v) = *reinterpret_cast<const uint4*>(p);
  return c;
}
template <typename T, int V> __device__ __forceinline__ void store_chunk(T* p, const Chunk<T, V>& c) {
  if constexpr (V == 1) *p = c.v[0];
  else *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(c.v);
}

// blockIdx.y = the pair: first the ceil(n_mixup / 2) mixup pairs, then the ceil((batch - n_mixup) / 2) cutmix pairs.
// V elements (16 bytes, or 1 where a row is not a whole number of 16-byte chunks) per thread and step.
template <typename T, int V>
__global__ __launch_bounds__(THREADS) void k_mix_images(T* __restrict__ img, int batch, int h, int w, int ch, int n_mixup,
                                                       const float* __restrict__ weights, const int32_t* __restrict__ boxes) {
  const int64_t n = (int64_t)h * w * ch;      // elements of one image
  const int mix_pairs = (n_mixup + 1) / 2;
  const int pair = blockIdx.y;
  const int64_t step = (int64_t)gridDim.x * THREADS;
  if (pair < mix_pairs) {
    const int i = pair, p = n_mixup - 1 - pair;
    T* a = img + (size_t)i * n;
    T* b = img + (size_t)p * n;
    const float wi = weights[i], wp = weights[p];
    const float ui = 1.f - wi, up = 1.f - wp;
    for (int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x; c * V < n; c += step) {
      const Chunk<T, V> xa = load_chunk<T, V>(a + c * V), xb = load_chunk<T, V>(b + c * V);
      Chunk<T, V> oa, ob;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float fa = to_f<T>(xa.v[e]), fb = to_f<T>(xb.v[e]);
        oa.v[e] = from_f<T>(fa * wi + fb * ui);
        ob.v[e] = from_f<T>(fb * wp + fa * up);
      }
      store_chunk<T, V>(a + c * V, oa);
      if (p != i) store_chunk<T, V>(b + c * V, ob);      // (the middle row of an odd part is its own partner: once)
    }
    return;
  }
  const int k = pair - mix_pairs;
  const int i = n_mixup + k, p = batch - 1 - k;
  if (p == i) return;      // its own partner: the box is filled with what is there
  const Box bi = load_box(boxes, i, h, w), bp = load_box(boxes, p, h, w);
  const bool ei = bi.y2 == 0, ep = bp.y2 == 0;
  if (ei && ep) return;
  // image rows that one of the two boxes touches; nothing outside them is read or written
  const int y_lo = ei ? bp.y1 : ep ? bi.y1 : min(bi.y1, bp.y1);
  const int y_hi = max(bi.y2, bp.y2);
  const int wc = w * ch;
  const int ia = bi.x1 * ch, ib = bi.x2 * ch, pa = bp.x1 * ch, pb = bp.x2 * ch;      // the boxes' element columns
  T* a = img + (size_t)i * n;
  T* b = img + (size_t)p * n;
  const int64_t c_lo = (int64_t)y_lo * wc / V, c_hi = ((int64_t)y_hi * wc + V - 1) / V;
  for (int64_t c = c_lo + (int64_t)blockIdx.x * THREADS + threadIdx.x; c < c_hi; c += step) {
    int y = (int)(c * V / wc);
    int x = (int)(c * V - (int64_t)y * wc);
    bool in_i[V], in_p[V], any = false;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      in_i[e] = y >= bi.y1 && y < bi.y2 && x >= ia && x < ib;
      in_p[e] = y >= bp.y1 && y < bp.y2 && x >= pa && x < pb;
      any = any || in_i[e] || in_p[e];
      if (++x == wc) { x = 0; ++y; }
    }
    if (!any) continue;
    const Chunk<T, V> xa = load_chunk<T, V>(a + c * V), xb = load_chunk<T, V>(b + c * V);
    Chunk<T, V> oa, ob;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      oa.v[e] = in_i[e] ? xb.v[e] : xa.v[e];
      ob.v[e] = in_p[e] ? xa.v[e] : xb.v[e];
    }
    store_chunk<T, V>(a + c * V, oa);
    store_chunk<T, V>(b + c * V, ob);
  }
}

// One workgroup per row.  A = mean mask area of the cutmix part (datasets.py:236): box areas are integers, so their sum is
// exact in any order; every workgroup forms it for itself.
__global__ __launch_bounds__(THREADS) void k_mix_labels(const int32_t* __restrict__ labels, int batch, int nc, int h, int w,
                                                       int n_mixup, const float* __restrict__ weights,
                                                       const int32_t* __restrict__ boxes, float* __restrict__ soft, int label_ld) {
  __shared__ int wsum[THREADS / 64];
  const int row = blockIdx.x;
  int li, lp;
  float wa, wb;
  if (row < n_mixup) {      // (uniform over the workgroup)
    li = labels[row];
    lp = labels[n_mixup - 1 - row];
    wa = weights[row];
    wb = 1.f - wa;
  } else {
    int area = 0;
    for (int r = n_mixup + threadIdx.x; r < batch; r += THREADS) {
      const Box b = load_box(boxes, r, h, w);
      area += (b.y2 - b.y1) * (b.x2 - b.x1);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) area += __shfl_xor(area, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = area;
    __syncthreads();
    area = 0;
    for (int k = 0; k < THREADS / 64; ++k) area += wsum[k];
    li = labels[row];
    lp = labels[n_mixup + batch - 1 - row];
    wb = (float)area / (float)((batch - n_mixup) * h * w);
    wa = 1.f - wb;
  }
  float* out = soft + (size_t)row * label_ld;
  for (int c = threadIdx.x; c < label_ld; c += THREADS)
    out[c] = c < nc ? (c == li ? wa : 0.f) + (c == lp ? wb : 0.f) : 0.f;      // padding columns: zeros
}

template <typename T>
void launch_mix_images(void* images, int batch, int h, int w, int ch, int n_mixup, const float* weights, const int32_t* boxes,
                       int pairs, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  const int64_t n = (int64_t)h * w * ch;
  const bool vec = n % V == 0 && reinterpret_cast<uintptr_t>(images) % 16 == 0;
  const int64_t chunks = vec ? n / V : n;
  int64_t gx = (chunks + THREADS * 4 - 1) / (THREADS * 4);      // about four chunks per thread
  if (gx > 256) gx = 256;
  const dim3 grid((unsigned)gx, (unsigned)pairs);
  if (vec) edet_launch(k_mix_images<T, V>, grid, dim3(THREADS), 0, st, (T*)images, batch, h, w, ch, n_mixup, weights, boxes);
  else edet_launch(k_mix_images<T, 1>, grid, dim3(THREADS), 0, st, (T*)images, batch, h, w, ch, n_mixup, weights, boxes);
}

}  // namespace

extern "C" int edet_mix_images(void* images, int batch, int height, int width, int channels, int n_mixup, const float* weights,
                               const int32_t* boxes, int dtype, void* stream) {
  EDET_CHECK(images && weights && boxes, "edet_mix_images: null pointer");
  EDET_CHECK(batch > 0 && height > 0 && width > 0 && channels > 0, "edet_mix_images: batch %d, image %d x %d x %d", batch, height,
             width, channels);
  EDET_CHECK((int64_t)height * width * channels < (int64_t)1 << 31, "edet_mix_images: image %d x %d x %d too large", height, width, channels);
  EDET_CHECK(n_mixup >= 0 && n_mixup <= batch, "edet_mix_images: n_mixup %d outside [0, %d]", n_mixup, batch);
  const int pairs = (n_mixup + 1) / 2 + (batch - n_mixup + 1) / 2;
  EDET_CHECK(pairs <= 65535, "edet_mix_images: batch %d too large", batch);
  if (dtype == EDET_BF16) launch_mix_images<bf16_t>(images, batch, height, width, channels, n_mixup, weights, boxes, pairs, to_stream(stream));
  else if (dtype == EDET_F32) launch_mix_images<float>(images, batch, height, width, channels, n_mixup, weights, boxes, pairs, to_stream(stream));
  else EDET_CHECK(false, "edet_mix_images: bad dtype %d", dtype);
  EDET_LAUNCH_CHECK("edet_mix_images");
  return 0;
}

extern "C" int edet_mix_labels(const int32_t* labels, int batch, int num_classes, int height, int width, int n_mixup,
                               const float* weights, const int32_t* boxes, float* soft_labels, int label_ld, void* stream) {
  EDET_CHECK(labels && weights && boxes && soft_labels, "edet_mix_labels: null pointer");
  EDET_CHECK(batch > 0 && num_classes >= 1 && height > 0 && width > 0, "edet_mix_labels: batch %d, num_classes %d, image %d x %d",
             batch, num_classes, height, width);
  EDET_CHECK(label_ld >= num_classes, "edet_mix_labels: bad label_ld %d (num_classes %d)", label_ld, num_classes);
  EDET_CHECK(n_mixup >= 0 && n_mixup <= batch, "edet_mix_labels: n_mixup %d outside [0, %d]", n_mixup, batch);
  EDET_CHECK((int64_t)batch * height * width < (int64_t)1 << 31, "edet_mix_labels: %d images of %d x %d: the area sum leaves int32", batch,
             height, width);
  edet_launch(k_mix_labels, dim3(batch), dim3(THREADS), 0, to_stream(stream), labels, batch, num_classes, height, width, n_mixup,
              weights, boxes, soft_labels, label_ld);
  EDET_LAUNCH_CHECK("edet_mix_labels");
  return 0;
}
