"""numpy restatement of the detector's box-aware AutoAugment / RandAugment (efficientdet/aug/autoaugment.py), one uint8 image
[H, W, 3] with its boxes [N, 4] (normalised ymin, xmin, ymax, xmax) at a time: the box functions (:435-483, :785-835,
:881-919, :978-1025), the detector's Contrast (:267-280), BBox_Cutout's rectangle (:1245-1345) and the policy walk
(:1505-1535, :1632-1667).  The image operations the two reference modules share are tests/randaug_ref.py's.  Every product,
sum and quotient is a single float32 operation in the reference's order; to_int32 truncates.
tests/test_det_autoaugment.py pins this file to the executed reference (tests/golden/reference_det_autoaugment.npz) and
compares the kernels with it bit for bit."""
import math

import numpy as np

from tests import randaug_ref as rr

F = np.float32
NAMES = ('AutoContrast', 'Equalize', 'Posterize', 'Solarize', 'SolarizeAdd', 'Color', 'Contrast', 'Brightness', 'Sharpness',
         'Cutout', 'BBox_Cutout', 'Rotate_BBox', 'TranslateX_BBox', 'TranslateY_BBox', 'ShearX_BBox', 'ShearY_BBox')
SIGNED = ('Rotate_BBox', 'TranslateX_BBox', 'TranslateY_BBox', 'ShearX_BBox', 'ShearY_BBox')
RANDAUG_OPS = ('Equalize', 'Solarize', 'Color', 'Cutout', 'SolarizeAdd', 'TranslateX_BBox', 'TranslateY_BBox', 'ShearX_BBox',
               'ShearY_BBox', 'Rotate_BBox')
POLICIES = {
    'test': [[('TranslateX_BBox', 1.0, 4), ('Equalize', 1.0, 10)]],
    'v2': [
        [('Color', 0.0, 6), ('Cutout', 0.6, 8), ('Sharpness', 0.4, 8)],
        [('Rotate_BBox', 0.4, 8), ('Sharpness', 0.4, 2), ('Rotate_BBox', 0.8, 10)],
        [('TranslateY_BBox', 1.0, 8), ('AutoContrast', 0.8, 2)],
        [('AutoContrast', 0.4, 6), ('ShearX_BBox', 0.8, 8), ('Brightness', 0.0, 10)],
        [('SolarizeAdd', 0.2, 6), ('Contrast', 0.0, 10), ('AutoContrast', 0.6, 0)],
        [('Cutout', 0.2, 0), ('Solarize', 0.8, 8), ('Color', 1.0, 4)],
        [('TranslateY_BBox', 0.0, 4), ('Equalize', 0.6, 8), ('Solarize', 0.0, 10)],
        [('TranslateY_BBox', 0.2, 2), ('ShearY_BBox', 0.8, 8), ('Rotate_BBox', 0.8, 8)],
        [('Cutout', 0.8, 8), ('Brightness', 0.8, 8), ('Cutout', 0.2, 2)],
        [('Color', 0.8, 4), ('TranslateY_BBox', 1.0, 6), ('Rotate_BBox', 0.6, 6)],
        [('Rotate_BBox', 0.6, 10), ('BBox_Cutout', 1.0, 4), ('Cutout', 0.2, 8)],
        [('Rotate_BBox', 0.0, 0), ('Equalize', 0.6, 6), ('ShearY_BBox', 0.6, 8)],
        [('Brightness', 0.8, 8), ('AutoContrast', 0.4, 2), ('Brightness', 0.2, 2)],
        [('TranslateY_BBox', 0.4, 8), ('Solarize', 0.4, 6), ('SolarizeAdd', 0.2, 10)],
        [('Contrast', 1.0, 10), ('SolarizeAdd', 0.2, 8), ('Equalize', 0.2, 4)]],
    'v3': [
        [('Posterize', 0.8, 2), ('TranslateX_BBox', 1.0, 8)],
        [('BBox_Cutout', 0.2, 10), ('Sharpness', 1.0, 8)],
        [('Rotate_BBox', 0.6, 8), ('Rotate_BBox', 0.8, 10)],
        [('Equalize', 0.8, 10), ('AutoContrast', 0.2, 10)],
        [('SolarizeAdd', 0.2, 2), ('TranslateY_BBox', 0.2, 8)],
        [('Sharpness', 0.0, 2), ('Color', 0.4, 8)],
        [('Equalize', 1.0, 8), ('TranslateY_BBox', 1.0, 8)],
        [('Posterize', 0.6, 2), ('Rotate_BBox', 0.0, 10)],
        [('AutoContrast', 0.6, 0), ('Rotate_BBox', 1.0, 6)],
        [('Equalize', 0.0, 4), ('Cutout', 0.8, 10)],
        [('Brightness', 1.0, 2), ('TranslateY_BBox', 1.0, 6)],
        [('Contrast', 0.0, 2), ('ShearY_BBox', 0.8, 0)],
        [('AutoContrast', 0.8, 10), ('Contrast', 0.2, 10)],
        [('Rotate_BBox', 1.0, 10), ('Cutout', 1.0, 10)],
        [('SolarizeAdd', 0.8, 6), ('Equalize', 0.8, 8)]],
}


def to_int32(t):
  """tf.to_int32 of a float32: truncation."""
  return int(np.trunc(F(t)))


def clip_bbox(box):
  """min(max(v, 0), 1), each a compare and select: -0.0 (Rotate makes it: -(0.5 - 0.5)) stays -0.0."""
  out = []
  for v in box:
    v = F(v)
    v = F(0.0) if v < F(0.0) else v
    out.append(F(1.0) if v > F(1.0) else v)
  return out


def check_bbox_area(box, delta=0.05):
  y0, x0, y1, x1 = (F(v) for v in box)
  if y1 - y0 == F(0.0):
    y1, y0 = max(y1, F(0.0 + delta)), min(y0, F(1.0 - delta))
  if x1 - x0 == F(0.0):
    x1, x0 = max(x1, F(0.0 + delta)), min(x0, F(1.0 - delta))
  return [y0, x0, y1, x1]


def finish(box):
  return np.asarray(check_bbox_area(clip_bbox(box)), F)


def matmul_2x4(matrix, coords):
  """A float32 [2, 2] matrix times the transposed corner list [4, 2] -> int32 [2, 4]; every entry is two rounded products and
  one rounded sum."""
  m = np.asarray(matrix, F)
  c = np.asarray(coords, F)
  out = np.zeros((2, 4), np.int64)
  for r in range(2):
    for k in range(4):
      out[r, k] = to_int32(m[r, 0] * c[k, 0] + m[r, 1] * c[k, 1])
  return out


def rotate_bbox(box, h, w, degrees):
  H, W = F(h), F(w)
  angle = F(degrees * (math.pi / 180.0))
  cos, sin = np.cos(angle), np.sin(angle)
  y0 = -to_int32(H * (F(box[0]) - F(0.5)))
  x0 = to_int32(W * (F(box[1]) - F(0.5)))
  y1 = -to_int32(H * (F(box[2]) - F(0.5)))
  x1 = to_int32(W * (F(box[3]) - F(0.5)))
  new = matmul_2x4([[cos, sin], [-sin, cos]], [[y0, x0], [y0, x1], [y1, x0], [y1, x1]])
  return finish([-(F(new[0].max()) / H - F(0.5)), F(new[1].min()) / W + F(0.5),
                 -(F(new[0].min()) / H - F(0.5)), F(new[1].max()) / W + F(0.5)])


def shift_bbox(box, h, w, pixels, horizontal):
  H, W = F(h), F(w)
  p = to_int32(pixels)
  y0, x0, y1, x1 = to_int32(H * F(box[0])), to_int32(W * F(box[1])), to_int32(H * F(box[2])), to_int32(W * F(box[3]))
  if horizontal:
    x0, x1 = max(0, x0 - p), min(w, x1 - p)
  else:
    y0, y1 = max(0, y0 - p), min(h, y1 - p)
  return finish([F(y0) / H, F(x0) / W, F(y1) / H, F(x1) / W])


def shear_bbox(box, h, w, level, horizontal):
  H, W = F(h), F(w)
  y0, x0, y1, x1 = to_int32(H * F(box[0])), to_int32(W * F(box[1])), to_int32(H * F(box[2])), to_int32(W * F(box[3]))
  lv = F(level)
  matrix = [[1, 0], [-lv, 1]] if horizontal else [[1, -lv], [0, 1]]
  new = matmul_2x4(matrix, [[y0, x0], [y0, x1], [y1, x0], [y1, x1]])
  return finish([F(new[0].min()) / H, F(new[1].min()) / W, F(new[0].max()) / H, F(new[1].max()) / W])


def contrast(img, factor):
  """:267-280: the mean grey level, float32(sum) / float32(H W) with the sum exact, clipped and truncated."""
  g = rr.grayscale(img)
  mean = F(int(g.astype(np.int64).sum())) / F(g.size)
  return rr.blend(np.full(img.shape, rr.to_u8(np.asarray(mean, F)), np.uint8), img, factor)


def draw_int(u, lo, hi):
  """tf.random_uniform(minval=lo, maxval=hi, dtype=int32) from u in [0, 1)."""
  return min(lo + int(math.floor(u * (hi - lo))), hi - 1)


def bbox_cutout_rect(boxes, h, w, pad_fraction, box_u, cy_u, cx_u):
  """-> (y1, x1, y2, x2) half-open, the pixels set to 128; no box: nothing."""
  n = len(boxes)
  if n == 0:
    return (0, 0, 0, 0)
  box = boxes[draw_int(box_u, 0, n)]
  H, W = F(h), F(w)
  y0, x0, y1, x1 = to_int32(H * F(box[0])), to_int32(W * F(box[1])), to_int32(H * F(box[2])), to_int32(W * F(box[3]))
  pad_h = int(pad_fraction * ((y1 - y0 + 1) / 2))
  pad_w = int(pad_fraction * ((x1 - x0 + 1) / 2))
  cy, cx = draw_int(cy_u, y0, y1 + 1), draw_int(cx_u, x0, x1 + 1)
  lower, upper = max(0, cy - pad_h), max(0, h - cy - pad_h)
  left, right = max(0, cx - pad_w), max(0, w - cx - pad_w)
  return (lower, left, h - upper, w - right)


def level_to_arg(name, level):
  """:1392-1470 with the hparams of :1620-1626, before the random negation (the restatement's own copy)."""
  r = level / 10.
  return {'AutoContrast': lambda: (), 'Equalize': lambda: (), 'Posterize': lambda: (int(r * 4),),
          'Solarize': lambda: (int(r * 256),), 'SolarizeAdd': lambda: (int(r * 110),), 'Color': lambda: (r * 1.8 + 0.1,),
          'Contrast': lambda: (r * 1.8 + 0.1,), 'Brightness': lambda: (r * 1.8 + 0.1,), 'Sharpness': lambda: (r * 1.8 + 0.1,),
          'Cutout': lambda: (int(r * 100),), 'BBox_Cutout': lambda: (r * 0.75, False), 'Rotate_BBox': lambda: (r * 30.,),
          'TranslateX_BBox': lambda: (r * 250.,), 'TranslateY_BBox': lambda: (r * 250.,), 'ShearX_BBox': lambda: (r * 0.3,),
          'ShearY_BBox': lambda: (r * 0.3,)}[name]()


def apply_op(img, boxes, name, level, sign=1.0, cy_u=0.0, cx_u=0.0, box_u=0.0):
  """One operation on one image and its (valid) boxes [N, 4] -> (image, boxes)."""
  h, w = img.shape[:2]
  boxes = np.asarray(boxes, F).reshape(-1, 4)
  args = level_to_arg(name, float(level))
  if name in SIGNED:
    v = float(sign) * args[0]
    if name == 'Rotate_BBox':
      return rr.rotate(img, v), np.asarray([rotate_bbox(b, h, w, v) for b in boxes], F).reshape(-1, 4)
    if name in ('TranslateX_BBox', 'TranslateY_BBox'):
      hor = name == 'TranslateX_BBox'
      out = rr.translate_x(img, v) if hor else rr.translate_y(img, v)
      return out, np.asarray([shift_bbox(b, h, w, v, hor) for b in boxes], F).reshape(-1, 4)
    hor = name == 'ShearX_BBox'
    out = rr.shear_x(img, v) if hor else rr.shear_y(img, v)
    return out, np.asarray([shear_bbox(b, h, w, v, hor) for b in boxes], F).reshape(-1, 4)
  if name == 'Cutout':
    return rr.cutout(img, args[0], draw_int(cy_u, 0, h), draw_int(cx_u, 0, w)), boxes.copy()
  if name == 'BBox_Cutout':
    y1, x1, y2, x2 = bbox_cutout_rect(boxes, h, w, args[0], box_u, cy_u, cx_u)
    out = img.copy()
    out[max(y1, 0):max(y2, 0), max(x1, 0):max(x2, 0)] = rr.REPLACE
    return out, boxes.copy()
  if name == 'Contrast':
    return contrast(img, *args), boxes.copy()
  return rr.FUNCS[name](img, *args), boxes.copy()


def should_apply(u, prob):
  return bool(np.floor(F(u) + F(prob)) != 0)


def walk(img, boxes, policy, index, apply_u, sign, cy_u, cx_u, box_u, magnitude=None):
  """One image through a policy.  policy: a table name of POLICIES, then index is the sub-policy and the other draws are
  per-layer lists; or 'randaug', then index is the per-layer list of operations over RANDAUG_OPS and apply_u is unused."""
  boxes = np.asarray(boxes, F).reshape(-1, 4)
  if policy == 'randaug':
    steps = [(RANDAUG_OPS[int(op)], None, magnitude) for op in index]
  else:
    steps = POLICIES[policy][int(index)]
  for k, (name, prob, level) in enumerate(steps):
    if prob is not None and not should_apply(apply_u[k], prob):
      continue
    img, boxes = apply_op(img, boxes, name, level, sign[k], cy_u[k], cx_u[k], box_u[k])
  return img, boxes


def distort_batch(images, boxes, counts, policy, draws, magnitude=None):
  """A batch [B, H, W, 3] with padded boxes [B, M, 4] and counts [B] through det_autoaugment.autoaug_draws' draws; rows at or
  past the count come back as they went in."""
  index, apply_u, sign, cy_u, cx_u, box_u = draws
  out = np.array(images, dtype=np.uint8, copy=True)
  bout = np.array(boxes, dtype=F, copy=True)
  for i in range(out.shape[0]):
    n = int(counts[i])
    col = lambda a: None if a is None else np.asarray(a)[:, i]      # noqa: E731
    idx = np.asarray(index)[:, i] if policy == 'randaug' else np.asarray(index)[i]
    out[i], bout[i, :n] = walk(out[i], bout[i, :n], policy, idx, col(apply_u), col(sign), col(cy_u), col(cx_u), col(box_u),
                               magnitude)
  return out, bout
