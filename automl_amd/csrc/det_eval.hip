// The evaluation branch of the detector's input: the ground-truth packing of InputReader.dataset_parser and process_example
// (efficientdet/dataloader.py:344-353, :389) for a batch.
//
//   boxes *= image_scale_to_original                                  :345-346   one rounded fp32 product per coordinate
//   boxes     = pad_to_fixed_size(boxes, -1, [max_instances, 4])      :348
//   is_crowds = pad_to_fixed_size(is_crowds, 0, [max_instances, 1])   :347, :349
//   areas     = pad_to_fixed_size(areas, -1, [max_instances, 1])      :351
//   classes   = pad_to_fixed_size(classes, -1, [max_instances, 1])    :352
//   groundtruth_data = concat([boxes, is_crowds, areas, classes], 2)  :389
//
// Kept as the reference is written: resize_and_crop_boxes drops the boxes without area WITH their classes (:186-190), but
// is_crowds and areas are the decoder's, unfiltered.  So columns 0-3 and 6 of a row hold the row-th KEPT box and columns 4
// and 5 the row-th ANNOTATION: behind a dropped box the two halves of a row belong to different annotations, and the last
// rows hold a crowd flag and an area next to a box of -1.
//
// The evaluation step's loss kernels (edet_focal_loss_eval, edet_box_loss_eval, edet_l2_loss) are instantiations of the
// training kernels' bodies and live with them in det_loss.hip: their sums have to come out of the same contracted arithmetic.
// This file is compiled with -ffp-contract=off (automl_amd/build.py), as the other restatements of the input pipeline are.
#include "common.h"

namespace {

constexpr int GT_THREADS = 256;

// one thread per output row [y1, x1, y2, x2, is_crowd, area, class]
__global__ __launch_bounds__(GT_THREADS) void k_pack_groundtruth(const float* __restrict__ boxes, const float* __restrict__ classes,
                                                                const int32_t* __restrict__ kept_counts,
                                                                const float* __restrict__ is_crowds, const float* __restrict__ areas,
                                                                const int32_t* __restrict__ counts, const float* __restrict__ scales,
                                                                int batch, int max_boxes, int max_instances, float* __restrict__ gt) {
  const int64_t total = (int64_t)batch * max_instances;
  const int64_t i = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x;
  if (i >= total) return;
  const int b = (int)(i / max_instances), r = (int)(i - (int64_t)b * max_instances);
  // counts come from device memory: clamped before they index anything
  const int kept = min(max(kept_counts[b], 0), max_boxes);
  const int given = min(max(counts[b], 0), max_boxes);
  float row[7] = {-1.f, -1.f, -1.f, -1.f, 0.f, -1.f, -1.f};
  if (r < kept) {
    const size_t src = (size_t)b * max_boxes + r;
    const float s = scales[b];
#pragma unroll
    for (int k = 0; k < 4; ++k) row[k] = __fmul_rn(boxes[src * 4 + k], s);
    row[6] = classes[src];
  }
  if (r < given) {
    const size_t src = (size_t)b * max_boxes + r;
    row[4] = is_crowds[src];
    row[5] = areas[src];
  }
  float* dst = gt + (size_t)i * 7;
#pragma unroll
  for (int k = 0; k < 7; ++k) dst[k] = row[k];
}

}  // namespace

extern "C" int edet_pack_groundtruth(const float* boxes, const float* classes, const int32_t* kept_counts,
                                     const float* is_crowds, const float* areas, const int32_t* counts,
                                     const float* image_scales, int batch, int max_boxes, int max_instances,
                                     float* groundtruth_data, void* stream) {
  EDET_CHECK(boxes && classes && kept_counts && is_crowds && areas && counts && image_scales && groundtruth_data,
             "edet_pack_groundtruth: null pointer");
  EDET_CHECK(batch >= 1 && max_boxes >= 1 && max_instances >= max_boxes,
             "edet_pack_groundtruth: batch %d, %d box rows, max_instances_per_image %d (pad_to_fixed_size needs rows <= it)",
             batch, max_boxes, max_instances);
  const int64_t total = (int64_t)batch * max_instances;
  EDET_CHECK(total * 7 < (int64_t)1 << 31, "edet_pack_groundtruth: output too large");
  edet_launch(k_pack_groundtruth, dim3((unsigned)((total + GT_THREADS - 1) / GT_THREADS)), dim3(GT_THREADS), 0, to_stream(stream),
              boxes, classes, kept_counts, is_crowds, areas, counts, image_scales, batch, max_boxes, max_instances,
              groundtruth_data);
  EDET_LAUNCH_CHECK("edet_pack_groundtruth");
  return 0;
}
