"""The IoU / GIoU / DIoU / CIoU box loss restated in numpy, for any float type: the definition the kernels are held to.

Forward: efficientdet/tf2/anchors.py:30-58 (decode), tf2/train_lib.py:456-463 (the componentwise target mask, the reduction),
efficientdet/iou_utils.py:70-124 (the metric), :179-188 (the validity mask).  The gradient is derived by hand under the rules
TensorFlow executes the reference by:
  * maximum(x, y) hands its gradient to x where x >= y, minimum(x, y) to x where x <= y, in the order the reference writes the
    arguments (maximum(zero, w) gives w nothing at w == 0; maximum(p, t) gives the prediction the tie);
  * divide_no_nan is 0, with zero gradient, where the denominator is 0;
  * CIoU's v is a constant of the backward pass (its custom gradient reaches the TARGET's height and width only), alpha is
    differentiated through iou;
  * squared lengths are sums of squares: zero gradient at the zero vector;
  * an anchor whose four raw targets are 0 does no arithmetic: loss 0, gradient 0.
"""
import numpy as np

IOU_TYPES = ('iou', 'giou', 'diou', 'ciou')


def _dnn(x, y):
  """divide_no_nan"""
  ok = y != 0
  return np.where(ok, x / np.where(ok, y, 1), 0).astype(x.dtype)


def iou_boxes(p, t, iou_type, v_const=None):
  """p, t: [..., 4] decoded boxes [ymin, xmin, ymax, xmax] -> (loss [...], dloss/dp [..., 4]) in p's dtype.
  v_const: CIoU's v held at this value (the finite-difference tests: the backward pass treats v as a constant)."""
  if iou_type not in IOU_TYPES:
    raise ValueError('Unknown loss_type {}, not iou/ciou/diou/giou'.format(iou_type))
  p = np.asarray(p)
  dt = p.dtype
  t = np.asarray(t, dt)
  zero, one, two = dt.type(0), dt.type(1), dt.type(2)
  m = (t[..., 2] > t[..., 0]) & (t[..., 3] > t[..., 1])
  mf = m.astype(dt)
  p = p * mf[..., None]
  t = t * mf[..., None]
  p0, p1, p2, p3 = (p[..., k] for k in range(4))
  t0, t1, t2, t3 = (t[..., k] for k in range(4))
  pw_raw, ph_raw = p3 - p1, p2 - p0
  pw, ph = np.maximum(zero, pw_raw), np.maximum(zero, ph_raw)
  tw, th = np.maximum(zero, t3 - t1), np.maximum(zero, t2 - t0)
  pa, ta = pw * ph, tw * th
  iy0, ix0, iy1, ix1 = np.maximum(p0, t0), np.maximum(p1, t1), np.minimum(p2, t2), np.minimum(p3, t3)
  iw_raw, ih_raw = ix1 - ix0, iy1 - iy0
  iw, ih = np.maximum(zero, iw_raw), np.maximum(zero, ih_raw)
  ia = iw * ih
  ua = pa + ta - ia
  iou = _dnn(ia, ua)
  metric = iou
  g_iou = np.full_like(iou, -1)
  g_ua = np.zeros_like(iou)
  g_ey0, g_ex0, g_ey1, g_ex1 = (np.zeros_like(iou) for _ in range(4))
  g_dy, g_dx = np.zeros_like(iou), np.zeros_like(iou)
  if iou_type != 'iou':
    ey0, ex0, ey1, ex1 = np.minimum(p0, t0), np.minimum(p1, t1), np.maximum(p2, t2), np.maximum(p3, t3)
  if iou_type == 'giou':
    ew_raw, eh_raw = ex1 - ex0, ey1 - ey0
    ew, eh = np.maximum(zero, ew_raw), np.maximum(zero, eh_raw)
    ea = ew * eh
    num = ea - ua
    metric = iou - _dnn(num, ea)
    g_ea = _dnn(np.ones_like(ea), ea) - _dnn(_dnn(num, ea), ea)
    g_ua = -_dnn(np.ones_like(ea), ea)
    g_ex1 = np.where(ew_raw > 0, g_ea * eh, zero)
    g_ex0 = -g_ex1
    g_ey1 = np.where(eh_raw > 0, g_ea * ew, zero)
    g_ey0 = -g_ey1
  elif iou_type in ('diou', 'ciou'):
    dy = (t0 + t2) / two - (p0 + p2) / two
    dx = (t1 + t3) / two - (p1 + p3) / two
    cy, cx = ey1 - ey0, ex1 - ex0
    d2, c2 = dy * dy + dx * dx, cy * cy + cx * cx
    metric = iou - _dnn(d2, c2)
    g_d2 = _dnn(np.ones_like(c2), c2)
    g_c2 = -_dnn(_dnn(d2, c2), c2)
    g_dy, g_dx = g_d2 * (two * dy), g_d2 * (two * dx)
    g_ey1 = g_c2 * (two * cy)
    g_ey0 = -g_ey1
    g_ex1 = g_c2 * (two * cx)
    g_ex0 = -g_ex1
    if iou_type == 'ciou':
      if v_const is None:
        at = np.arctan(_dnn(pw, ph)) - np.arctan(_dnn(tw, th))
        q = at / dt.type(np.pi)
        v = dt.type(4) * (q * q)
      else:
        v = np.asarray(v_const, dt)
      den = (one - iou) + v
      alpha = _dnn(v, den)
      metric = metric - alpha * v
      g_iou = g_iou + v * _dnn(_dnn(v, den), den)
  g_ia = _dnn(g_iou, ua)
  g_ua = g_ua - g_iou * _dnn(iou, ua)
  g_ia = g_ia - g_ua
  g_pw, g_ph = g_ua * ph, g_ua * pw
  g_iw, g_ih = g_ia * ih, g_ia * iw
  z = np.zeros_like(iou)
  g0, g1, g2, g3 = z.copy(), z.copy(), z.copy(), z.copy()
  g3 = g3 + np.where(pw_raw > 0, g_pw, zero)
  g1 = g1 - np.where(pw_raw > 0, g_pw, zero)
  g2 = g2 + np.where(ph_raw > 0, g_ph, zero)
  g0 = g0 - np.where(ph_raw > 0, g_ph, zero)
  g3 = g3 + np.where((iw_raw > 0) & (p3 <= t3), g_iw, zero)
  g1 = g1 - np.where((iw_raw > 0) & (p1 >= t1), g_iw, zero)
  g2 = g2 + np.where((ih_raw > 0) & (p2 <= t2), g_ih, zero)
  g0 = g0 - np.where((ih_raw > 0) & (p0 >= t0), g_ih, zero)
  if iou_type != 'iou':
    g0 = g0 + np.where(p0 <= t0, g_ey0, zero)
    g1 = g1 + np.where(p1 <= t1, g_ex0, zero)
    g2 = g2 + np.where(p2 >= t2, g_ey1, zero)
    g3 = g3 + np.where(p3 >= t3, g_ex1, zero)
    g0 = g0 - g_dy / two
    g2 = g2 - g_dy / two
    g1 = g1 - g_dx / two
    g3 = g3 - g_dx / two
  loss = (mf * (one - metric)).astype(dt)
  grad = (np.stack([g0, g1, g2, g3], -1) * mf[..., None]).astype(dt)
  return loss, grad


def ciou_v(p, t):
  """CIoU's v of decoded boxes (for the tests that hold it constant)."""
  p = np.asarray(p)
  dt = p.dtype
  t = np.asarray(t, dt)
  mf = ((t[..., 2] > t[..., 0]) & (t[..., 3] > t[..., 1])).astype(dt)[..., None]
  p, t = p * mf, t * mf
  zero = dt.type(0)
  pw, ph = np.maximum(zero, p[..., 3] - p[..., 1]), np.maximum(zero, p[..., 2] - p[..., 0])
  tw, th = np.maximum(zero, t[..., 3] - t[..., 1]), np.maximum(zero, t[..., 2] - t[..., 0])
  q = (np.arctan(_dnn(pw, ph)) - np.arctan(_dnn(tw, th))) / dt.type(np.pi)
  return dt.type(4) * (q * q)


def iou_loss(pred_boxes, target_boxes, iou_type='iou'):
  """iou_utils.iou_loss: [..., 4k] -> (loss [...] summed over the k anchors, gradient [..., 4k])."""
  pred_boxes = np.asarray(pred_boxes)
  if iou_type not in IOU_TYPES:
    raise ValueError('Unknown loss_type {}, not iou/ciou/diou/giou'.format(iou_type))
  assert pred_boxes.shape[-1] % 4 == 0
  shp = pred_boxes.shape
  p = pred_boxes.reshape(shp[:-1] + (shp[-1] // 4, 4))
  t = np.asarray(target_boxes, pred_boxes.dtype).reshape(p.shape)
  loss, grad = iou_boxes(p, t, iou_type)
  total = np.zeros(shp[:-1], pred_boxes.dtype)
  for i in range(p.shape[-2]):
    total = total + loss[..., i]
  return total, grad.reshape(shp)


def decode(x, anchors):
  """anchors.py:30-58 -> (boxes [..., 4], (ha, wa, h, w))"""
  dt = x.dtype
  a = np.asarray(anchors, dt)
  two = dt.type(2)
  yca, xca = (a[..., 0] + a[..., 2]) / two, (a[..., 1] + a[..., 3]) / two
  ha, wa = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
  w, h = np.exp(x[..., 3]) * wa, np.exp(x[..., 2]) * ha
  yc, xc = x[..., 0] * ha + yca, x[..., 1] * wa + xca
  return np.stack([yc - h / two, xc - w / two, yc + h / two, xc + w / two], -1), (ha, wa, h, w)


def box_iou_per_anchor(box_outputs, box_targets, anchors, iou_type, v_const=None):
  """Raw outputs and raw targets [N, 4] of N anchors [N, 4] -> (per-anchor loss [N], d loss / d box_outputs [N, 4]), in
  box_outputs' dtype.  Rows whose four targets are 0 are not computed: loss 0, gradient 0."""
  x = np.asarray(box_outputs)
  dt = x.dtype
  tg = np.asarray(box_targets, dt)
  a = np.asarray(anchors, dt)
  loss = np.zeros(x.shape[:-1], dt)
  grad = np.zeros(x.shape, dt)
  pos = (tg != 0).any(-1)
  if not pos.any():
    return loss, grad
  xs, ts, as_ = x[pos], tg[pos], a[pos]
  mask = (ts != 0).astype(dt)
  with np.errstate(over='ignore', invalid='ignore'):
    p, (ha, wa, h, w) = decode(xs, as_)
    t, _ = decode(ts, as_)
    p, t = np.where(mask != 0, p, dt.type(0)), np.where(mask != 0, t, dt.type(0))
    l, dp = iou_boxes(p, t, iou_type, None if v_const is None else np.asarray(v_const)[pos])
    dp = dp * mask
    two = dt.type(2)
    g = np.stack([(dp[..., 0] + dp[..., 2]) * ha, (dp[..., 1] + dp[..., 3]) * wa,
                  ((dp[..., 2] - dp[..., 0]) / two) * h, ((dp[..., 3] - dp[..., 1]) / two) * w], -1)
  loss[pos] = l
  grad[pos] = g
  return loss, grad


def decoded_pair(box_outputs, box_targets, anchors):
  """The masked decoded boxes (p, t) that box_iou_per_anchor hands to iou_boxes (all rows)."""
  x = np.asarray(box_outputs)
  dt = x.dtype
  tg = np.asarray(box_targets, dt)
  mask = tg != 0
  with np.errstate(over='ignore', invalid='ignore'):
    p, _ = decode(x, anchors)
    t, _ = decode(tg, anchors)
  return np.where(mask, p, dt.type(0)), np.where(mask, t, dt.type(0))


def box_iou_loss(box_outputs, box_targets, anchors, iou_type, normalizer):
  """BoxIouLoss.call (train_lib.py:452-464): sum over the anchors / (4 * normalizer), and its gradient."""
  loss, grad = box_iou_per_anchor(box_outputs, box_targets, anchors, iou_type)
  dt = loss.dtype
  inv = dt.type(1) / (dt.type(normalizer) * dt.type(4))
  return loss.sum(dtype=dt) * inv, grad * inv


# ---- the input recipe shared by tests/golden/make_golden_iou_loss.py and the device tests -------------------------------------
def make_anchors(h, w, num_anchors, stride=8.0):
  """[h * w * A, 4] float32 anchors [ymin, xmin, ymax, xmax] in the order (y, x, anchor): centres on the stride grid, sizes
  from three octave scales x three aspect ratios as anchors.Anchors forms them (the first A of the nine)."""
  cfgs = [(2.0 ** (o / 3.0), r) for o in range(3) for r in (1.0, 2.0, 0.5)][:num_anchors]
  out = np.zeros((h, w, num_anchors, 4), np.float64)
  for k, (scale, ratio) in enumerate(cfgs):
    base = 4.0 * stride * scale
    ah, aw = base / np.sqrt(ratio) / 2.0, base * np.sqrt(ratio) / 2.0
    yc, xc = np.meshgrid((np.arange(h) + 0.5) * stride, (np.arange(w) + 0.5) * stride, indexing='ij')
    out[:, :, k] = np.stack([yc - ah, xc - aw, yc + ah, xc + aw], -1)
  return out.reshape(-1, 4).astype(np.float32)


def kink_margin(box_outputs, box_targets, anchors):
  """The smallest distance (pixels, float64) of a positive anchor's masked decoded boxes to a kink of the metric: an equality
  in a max / min between the two boxes (on a coordinate that is not masked out), a zero width or height of the prediction, the
  target, the intersection or the enclosing box.  inf without positives."""
  x, tg, a = (np.asarray(v, np.float64) for v in (box_outputs, box_targets, anchors))
  pos = (tg != 0).any(-1)
  if not pos.any():
    return np.inf
  p, t = decoded_pair(x[pos], tg[pos], a[pos])
  live = tg[pos] != 0
  d = [np.where(live, np.abs(p - t), np.inf).min()]
  for b in (p, t):
    d += [np.abs(b[:, 2] - b[:, 0]).min(), np.abs(b[:, 3] - b[:, 1]).min()]
  iw = np.minimum(p[:, 3], t[:, 3]) - np.maximum(p[:, 1], t[:, 1])
  ih = np.minimum(p[:, 2], t[:, 2]) - np.maximum(p[:, 0], t[:, 0])
  ew = np.maximum(p[:, 3], t[:, 3]) - np.minimum(p[:, 1], t[:, 1])
  eh = np.maximum(p[:, 2], t[:, 2]) - np.minimum(p[:, 0], t[:, 0])
  d += [np.abs(v).min() for v in (iw, ih, ew, eh)]
  return float(min(d))


def draw_inputs(rng, anchors, zero_component_row=True, dtype=np.float32):
  """One draw of raw box outputs and raw targets [N, 4] (|value| <= 2) for N anchors: about a quarter of the rows positive,
  in turn overlapping (the prediction is the target plus noise), disjoint (centres 1.7 anchor heights or widths apart, sizes
  within exp(+-0.3)) and nested (one centre, sizes exp(+-0.7) apart); every other row has all four targets 0 and arbitrary
  outputs.  zero_component_row: the first overlapping row gets ONE target component that is exactly 0 (its ty)."""
  n = anchors.shape[0]
  x = rng.uniform(-2.0, 2.0, (n, 4))
  tg = np.zeros((n, 4))
  rows = np.flatnonzero(rng.random(n) < 0.25)
  if len(rows) < 3:
    rows = np.arange(min(n, 3))
  for i, r in enumerate(rows):
    kind = i % 3
    t = rng.uniform(0.05, 1.0, 4) * rng.choice([-1.0, 1.0], 4)
    if kind == 0:
      p = t + rng.normal(0.0, 0.3, 4)
    elif kind == 1:
      t[2:] = rng.uniform(0.05, 0.3, 2) * rng.choice([-1.0, 1.0], 2)
      p = t.copy()
      p[2:] = rng.uniform(-0.3, 0.3, 2)
      axis = int(rng.integers(0, 2))
      side = rng.choice([-1.0, 1.0])
      t[axis], p[axis] = -0.85 * side, 0.85 * side
      p[1 - axis] = t[1 - axis] + rng.normal(0.0, 0.2)
    else:
      p = t.copy()
      p[:2] += rng.normal(0.0, 0.02, 2)
      p[2:] = t[2:] + 0.7 * rng.choice([-1.0, 1.0]) + rng.normal(0.0, 0.05, 2)
    x[r], tg[r] = np.clip(p, -2.0, 2.0), t
  if zero_component_row:
    tg[rows[0], 0] = 0.0
  return x.astype(dtype), tg.astype(dtype)


def draw_case(seed, anchors, margin=1e-3, max_draws=64, **kwargs):
  """draw_inputs until no positive anchor lies within `margin` of a kink -> (box_outputs, box_targets, draws rejected)."""
  rng = np.random.default_rng(seed)
  for rejected in range(max_draws):
    x, tg = draw_inputs(rng, anchors, **kwargs)
    if kink_margin(x, tg, anchors) >= margin and np.abs(x).max() <= 2.0 and np.abs(tg).max() <= 2.0:
      return x, tg, rejected
  raise AssertionError('no draw with a kink margin of %g in %d' % (margin, max_draws))
