// The per-anchor body of the IoU / GIoU / DIoU / CIoU box loss: value and the derivative with respect to the prediction.
// One place for the arithmetic of edet_iou_loss (iou_loss.hip) and of edet_box_iou_loss / edet_box_iou_loss_eval (det_loss.hip).
//
// Reference: efficientdet/iou_utils.py:27-124 (_get_v, _iou_per_anchor), :174-191 (the validity mask),
// efficientdet/tf2/anchors.py:30-58 (decode_box_outputs), efficientdet/tf2/train_lib.py:456-463 (BoxIouLoss.call).
//
// The gradient is the reference's as TensorFlow executes it:
//   * maximum(x, y) hands its gradient to x where x >= y, minimum(x, y) to x where x <= y, x and y in the order the reference
//     writes them: maximum(zero, w) gives w nothing at w == 0, maximum(p, t) gives the prediction the tie;
//   * divide_no_nan is 0 with zero gradient where its denominator is 0;
//   * CIoU's v is a constant of the backward pass (tf.custom_gradient propagates to the function's arguments, which are the
//     TARGET's height and width); alpha = v / ((1 - iou) + v) is still differentiated through iou;
//   * the squared centre distance and the squared diagonal are sums of squares (the reference squares tf.linalg.norm): their
//     gradient at the zero vector is 0.
// No fused multiply-add contraction: every instantiation of the body rounds alike, and like the float32 numpy restatement.
#pragma once
#include "common.h"

namespace {

enum { IOU_IOU = 0, IOU_GIOU = 1, IOU_DIOU = 2, IOU_CIOU = 3, IOU_TYPES = 4 };

// Decoded boxes p, t = [ymin, xmin, ymax, xmax] -> loss = m * (1 - metric), m = the target has positive height and width.
// GRAD: dp[k] = d loss / d p[k].
template <bool GRAD>
__device__ __forceinline__ float iou_boxes(const float (&p)[4], const float (&t)[4], int type, float (&dp)[4]) {
#pragma clang fp contract(off)
  if (GRAD) dp[0] = dp[1] = dp[2] = dp[3] = 0.f;
  if (!(t[2] > t[0] && t[3] > t[1])) return 0.f;      // iou_utils.py:181-188: every coordinate and the result times 0
  const float pw_raw = p[3] - p[1], ph_raw = p[2] - p[0];
  const float pw = fmaxf(0.f, pw_raw), ph = fmaxf(0.f, ph_raw);
  const float tw = fmaxf(0.f, t[3] - t[1]), th = fmaxf(0.f, t[2] - t[0]);
  const float pa = pw * ph, ta = tw * th;
  const float iy0 = fmaxf(p[0], t[0]), ix0 = fmaxf(p[1], t[1]), iy1 = fminf(p[2], t[2]), ix1 = fminf(p[3], t[3]);
  const float iw_raw = ix1 - ix0, ih_raw = iy1 - iy0;
  const float iw = fmaxf(0.f, iw_raw), ih = fmaxf(0.f, ih_raw);
  const float ia = iw * ih;
  const float ua = pa + ta - ia;
  const float iou = ua != 0.f ? ia / ua : 0.f;
  float metric = iou;
  float g_iou = -1.f;                 // d loss / d iou
  float g_ua = 0.f;                   // d loss / d union, the part that does not go through iou
  float g_ey0 = 0.f, g_ex0 = 0.f, g_ey1 = 0.f, g_ex1 = 0.f;      // d loss / d enclosing box
  float g_dy = 0.f, g_dx = 0.f;       // d loss / d (t_center - p_center)
  float ey0 = 0.f, ex0 = 0.f, ey1 = 0.f, ex1 = 0.f;
  if (type != IOU_IOU) {
    ey0 = fminf(p[0], t[0]); ex0 = fminf(p[1], t[1]); ey1 = fmaxf(p[2], t[2]); ex1 = fmaxf(p[3], t[3]);
  }
  if (type == IOU_GIOU) {
    const float ew_raw = ex1 - ex0, eh_raw = ey1 - ey0;
    const float ew = fmaxf(0.f, ew_raw), eh = fmaxf(0.f, eh_raw);
    const float ea = ew * eh;
    const float num = ea - ua;
    if (ea != 0.f) {
      metric = iou - num / ea;
      if (GRAD) {
        const float g_ea = 1.f / ea - (num / ea) / ea;
        g_ua = -1.f / ea;
        if (ew_raw > 0.f) { g_ex1 = g_ea * eh; g_ex0 = -(g_ea * eh); }
        if (eh_raw > 0.f) { g_ey1 = g_ea * ew; g_ey0 = -(g_ea * ew); }
      }
    }
  } else if (type == IOU_DIOU || type == IOU_CIOU) {
    const float dy = (t[0] + t[2]) / 2.f - (p[0] + p[2]) / 2.f, dx = (t[1] + t[3]) / 2.f - (p[1] + p[3]) / 2.f;
    const float cy = ey1 - ey0, cx = ex1 - ex0;
    const float d2 = dy * dy + dx * dx, c2 = cy * cy + cx * cx;
    if (c2 != 0.f) {
      metric = iou - d2 / c2;
      if (GRAD) {
        const float g_d2 = 1.f / c2, g_c2 = -((d2 / c2) / c2);
        g_dy = g_d2 * (2.f * dy); g_dx = g_d2 * (2.f * dx);
        g_ey1 = g_c2 * (2.f * cy); g_ey0 = -g_ey1;
        g_ex1 = g_c2 * (2.f * cx); g_ex0 = -g_ex1;
      }
    }
    if (type == IOU_CIOU) {
      const float at = atanf(ph != 0.f ? pw / ph : 0.f) - atanf(th != 0.f ? tw / th : 0.f);
      const float q = at / 3.14159265358979323846f;
      const float v = 4.f * (q * q);
      const float den = (1.f - iou) + v;
      if (den != 0.f) {
        const float alpha = v / den;
        metric = metric - alpha * v;
        if (GRAD) g_iou = g_iou + v * ((v / den) / den);      // v is a constant here; alpha moves with iou
      }
    }
  }
  if (GRAD) {
    float g_ia = 0.f;
    if (ua != 0.f) {
      g_ia = g_iou / ua;
      g_ua = g_ua - g_iou * (iou / ua);
    }
    g_ia = g_ia - g_ua;                 // union = p_area + t_area - intersection
    const float g_pw = g_ua * ph, g_ph = g_ua * pw;
    const float g_iw = g_ia * ih, g_ih = g_ia * iw;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
    if (pw_raw > 0.f) { g3 += g_pw; g1 -= g_pw; }
    if (ph_raw > 0.f) { g2 += g_ph; g0 -= g_ph; }
    if (iw_raw > 0.f) {
      if (p[3] <= t[3]) g3 += g_iw;
      if (p[1] >= t[1]) g1 -= g_iw;
    }
    if (ih_raw > 0.f) {
      if (p[2] <= t[2]) g2 += g_ih;
      if (p[0] >= t[0]) g0 -= g_ih;
    }
    if (type != IOU_IOU) {
      if (p[0] <= t[0]) g0 += g_ey0;
      if (p[1] <= t[1]) g1 += g_ex0;
      if (p[2] >= t[2]) g2 += g_ey1;
      if (p[3] >= t[3]) g3 += g_ex1;
      g0 -= g_dy / 2.f; g2 -= g_dy / 2.f;
      g1 -= g_dx / 2.f; g3 -= g_dx / 2.f;
    }
    dp[0] = g0; dp[1] = g1; dp[2] = g2; dp[3] = g3;
  }
  return 1.f - metric;
}

// The raw outputs x = (ty, tx, th, tw) and raw targets tg of one anchor a = [ymin, xmin, ymax, xmax], both decoded with that
// anchor (anchors.py:30-58), each decoded coordinate of both boxes times (tg[k] != 0) (train_lib.py:458-460).
// GRAD: dx[k] = d loss / d x[k].  All four targets 0: no arithmetic at all, loss 0 and gradient 0.
template <bool GRAD>
__device__ __forceinline__ float iou_decoded(const float (&a)[4], const float (&x)[4], const float (&tg)[4], int type,
                                             float (&dx)[4]) {
#pragma clang fp contract(off)
  if (GRAD) dx[0] = dx[1] = dx[2] = dx[3] = 0.f;
  if (tg[0] == 0.f && tg[1] == 0.f && tg[2] == 0.f && tg[3] == 0.f) return 0.f;
  const float yca = (a[0] + a[2]) / 2.f, xca = (a[1] + a[3]) / 2.f;
  const float ha = a[2] - a[0], wa = a[3] - a[1];
  float p[4], t[4], dp[4];
  const float pw = expf(x[3]) * wa, ph = expf(x[2]) * ha;
  {
    const float yc = x[0] * ha + yca, xc = x[1] * wa + xca;
    p[0] = yc - ph / 2.f; p[1] = xc - pw / 2.f; p[2] = yc + ph / 2.f; p[3] = xc + pw / 2.f;
  }
  {
    const float w = expf(tg[3]) * wa, h = expf(tg[2]) * ha;
    const float yc = tg[0] * ha + yca, xc = tg[1] * wa + xca;
    t[0] = yc - h / 2.f; t[1] = xc - w / 2.f; t[2] = yc + h / 2.f; t[3] = xc + w / 2.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (tg[k] == 0.f) { p[k] = 0.f; t[k] = 0.f; }
  const float loss = iou_boxes<GRAD>(p, t, type, dp);
  if (GRAD) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (tg[k] == 0.f) dp[k] = 0.f;
    dx[0] = (dp[0] + dp[2]) * ha;
    dx[1] = (dp[1] + dp[3]) * wa;
    dx[2] = ((dp[2] - dp[0]) / 2.f) * ph;
    dx[3] = ((dp[3] - dp[1]) / 2.f) * pw;
  }
  return loss;
}

}  // namespace
