// iou_utils.iou_loss on decoded boxes (efficientdet/iou_utils.py:127-191): rows of k anchors [ymin, xmin, ymax, xmax] each,
// the row's loss summed over its anchors in anchor order, and on request the derivative with respect to the prediction.
// The body is iou_impl.h's, the one the training kernels of det_loss.hip run after decoding.
#include "iou_impl.h"

namespace {

constexpr int THREADS = 256;

template <bool GRAD>
__global__ __launch_bounds__(THREADS) void k_iou_loss(const float* __restrict__ pred, const float* __restrict__ target,
                                                     int64_t rows, int k, int type, float* __restrict__ loss_out,
                                                     float* __restrict__ dpred) {
  for (int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x; r < rows; r += (int64_t)gridDim.x * THREADS) {
    float acc = 0.f;
    for (int i = 0; i < k; ++i) {
      const int64_t o = (r * k + i) * 4;
      const float4 pv = *reinterpret_cast<const float4*>(pred + o);
      const float4 tv = *reinterpret_cast<const float4*>(target + o);
      const float p[4] = {pv.x, pv.y, pv.z, pv.w}, t[4] = {tv.x, tv.y, tv.z, tv.w};
      float dp[4];
      acc += iou_boxes<GRAD>(p, t, type, dp);
      if (GRAD) *reinterpret_cast<float4*>(dpred + o) = make_float4(dp[0], dp[1], dp[2], dp[3]);
    }
    loss_out[r] = acc;
  }
}

}  // namespace

extern "C" int edet_iou_loss(const float* pred_boxes, const float* target_boxes, int64_t rows, int k, int iou_type,
                             float* loss_out, float* dpred_out, void* stream) {
  EDET_CHECK(pred_boxes && target_boxes && loss_out, "edet_iou_loss: null pointer");
  EDET_CHECK(rows >= 0 && k >= 1, "edet_iou_loss: bad shape");
  EDET_CHECK(iou_type >= 0 && iou_type < IOU_TYPES, "edet_iou_loss: bad iou_type %d", iou_type);
  EDET_CHECK(((uintptr_t)pred_boxes | (uintptr_t)target_boxes | (uintptr_t)dpred_out) % 16 == 0,
             "edet_iou_loss: boxes must be 16-byte aligned");
  if (rows == 0) return 0;
  int64_t g = (rows + THREADS - 1) / THREADS;
  if (g > 4096) g = 4096;
  if (dpred_out)
    edet_launch(k_iou_loss<true>, dim3((unsigned)g), dim3(THREADS), 0, to_stream(stream), pred_boxes, target_boxes, rows, k,
                iou_type, loss_out, dpred_out);
  else
    edet_launch(k_iou_loss<false>, dim3((unsigned)g), dim3(THREADS), 0, to_stream(stream), pred_boxes, target_boxes, rows, k,
                iou_type, loss_out, (float*)nullptr);
  EDET_LAUNCH_CHECK("edet_iou_loss");
  return 0;
}
