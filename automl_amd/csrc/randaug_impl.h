// Value helpers shared by the image-augmentation kernels (randaug.hip, det_autoaug.hip).  The two reference modules
// (efficientnetv2/autoaugment.py, efficientdet/aug/autoaugment.py) have the same blend and the same grey conversion; both
// files that include this are compiled with -ffp-contract=off (automl_amd/build.py): every product and sum is a single
// rounded fp32 operation in the order written.
#pragma once
#include "common.h"

namespace raug {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
// clip to [0, 255] then truncate (NaN -> 0)
__device__ __forceinline__ int clip_u8(float t) { return (int)fminf(fmaxf(t, 0.f), 255.f); }

// blend for one value: a + f (b - a) as a subtract, a multiply and an add
__device__ __forceinline__ int blend(int a, int b, float f) {
  if (f == 0.f) return a;
  if (f == 1.f) return b;
  const float fa = (float)a;
  const float t = fa + f * ((float)b - fa);
  return clip_u8(t);      // (0 < f < 1 stays inside [0, 255]: the clip changes nothing there)
}

// tf.image.rgb_to_grayscale on uint8: v / 255 as a product, the three weights left to right, * 255.5, saturate, truncate
__device__ __forceinline__ int gray_of(int r, int g, int b) {
  const float k = 1.0f / 255.0f;
  const float s = ((float)r * k) * 0.2989f + ((float)g * k) * 0.5870f + ((float)b * k) * 0.1140f;
  return clip_u8(s * 255.5f);
}

}  // namespace raug
