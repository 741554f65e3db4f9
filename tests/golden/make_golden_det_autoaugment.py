"""Generates tests/golden/reference_det_autoaugment.npz by EXECUTING the reference's efficientdet/aug/autoaugment.py --
unmodified -- on the torch-backed `tf` stand-in (mini_keras.build_tf + make_golden_labels.add_tensor_ops +
make_golden_randaug's leaf operations + the ones below):
  * each of the sixteen NAME_TO_FUNC operations that do not end in _Only_BBoxes through _parse_policy_info at levels 0, 2, 6
    and 10 (both signs where the level is randomly negated) on three small images with four boxes each;
  * distort_image_with_autoaugment for 'test', 'v2' and 'v3': every sub-policy twice, with apply draws under which every
    operation of a probability above 0 runs, and draws under which only those of a probability of at least 0.5 do;
  * distort_image_with_randaugment(num_layers=1, magnitude=15) once per available operation;
  * BBox_Cutout on an image without boxes.

What the fixture pins is the reference's WIRING: the box functions, the detector's Contrast, _cutout_inside_bbox, level_to_arg
with the detector's hparams, the policy tables and the order in which a policy is walked.  The leaf arithmetic added here,
from the documented TensorFlow behaviour:
  * tf.to_float / tf.to_int32: float32; truncation;
  * tf.matmul of a [2, 2] by a [2, 4] float32 matrix: every entry two rounded products and one rounded sum (TensorFlow's own
    kernel is not pinned);
  * an int32 tensor `/` a Python integer: a float64 true division (tf's __truediv__ on integers), so that the pad sizes of
    _cutout_inside_bbox are the reference's double arithmetic;
  * tf.cos / tf.sin of a Python float: numpy's float32 cosine and sine (not pinned, as for the image rotation);
  * tf.reduce_mean: torch's float32 mean; the images here are small enough for every partial sum to be exact;
  * tf.map_fn: the function on each row, stacked; tf.cond is eager, so only the taken branch draws;
  * tf.random_uniform returns values queued by this script; the queues are stored with the outputs.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_det_autoaugment.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mini_keras   # noqa
from mini_keras import ns   # noqa
from make_golden_labels import _Ctx, add_tensor_ops   # noqa
import make_golden_randaug as mgr   # noqa
from make_golden_randaug import QUEUE, R, RT, add_randaug_ops, make_image_ops   # noqa

REF = '/root/reference/efficientdet'
LEVELS = (0, 2, 6, 10)
OPS = ('AutoContrast', 'Equalize', 'Posterize', 'Solarize', 'SolarizeAdd', 'Color', 'Contrast', 'Brightness', 'Sharpness',
       'Cutout', 'BBox_Cutout', 'Rotate_BBox', 'TranslateX_BBox', 'TranslateY_BBox', 'ShearX_BBox', 'ShearY_BBox')
SIGNED = ('Rotate_BBox', 'TranslateX_BBox', 'TranslateY_BBox', 'ShearX_BBox', 'ShearY_BBox')
RANDAUG_OPS = ('Equalize', 'Solarize', 'Color', 'Cutout', 'SolarizeAdd', 'TranslateX_BBox', 'TranslateY_BBox', 'ShearX_BBox',
               'ShearY_BBox', 'Rotate_BBox')


def _true_divide(self, o):      # tf: int / int is a float64 true division
  if not self.is_floating_point():
    return torch.true_divide(self.to(torch.float64), o)
  return torch.Tensor.__truediv__(self, o)


RT.__truediv__ = _true_divide


def _leaf(v):
  if torch.is_tensor(v):
    return v.item() if v.dim() == 0 else [_leaf(e) for e in v]
  if isinstance(v, (list, tuple)):
    return [_leaf(e) for e in v]
  return v


def add_box_ops(tf):
  def stack(xs, axis=0, name=None):
    if all(torch.is_tensor(x) and x.dim() >= 1 for x in xs):
      return R(torch.stack(list(xs), dim=axis))
    a = np.asarray(_leaf(list(xs)))      # scalars (0-d tensors, Python numbers), possibly nested: float32 / int32 as tf does
    return R(torch.from_numpy(a.astype(np.float32 if a.dtype.kind == 'f' else np.int32)))

  def to_float(x):
    return R(x if torch.is_tensor(x) else torch.as_tensor(x)).to(torch.float32)

  def to_int32(x):
    t = R(x if torch.is_tensor(x) else torch.as_tensor(x, dtype=torch.float32 if isinstance(x, float) else None))
    return torch.trunc(t).to(torch.int32) if t.is_floating_point() else t.to(torch.int32)

  def matmul(a, b):
    assert a.shape[1] == 2 and b.shape[0] == 2 and a.dtype == b.dtype == torch.float32
    left = a[:, 0:1] * b[0:1, :]
    right = a[:, 1:2] * b[1:2, :]
    return R(left + right)

  def map_fn(fn, elems):
    rows = [fn(e) for e in elems]
    return R(torch.stack(rows)) if rows else elems

  def reduce_mean(x, axis=None, reduction_indices=None, keepdims=False):
    axis = reduction_indices if reduction_indices is not None else axis
    x = R(x)
    x = x if x.is_floating_point() else x.to(torch.float32)
    return x.mean() if axis is None else x.mean(dim=tuple(axis))

  def squeeze(x, axis=None):
    x = R(x)
    return x.squeeze() if axis is None else x.squeeze(axis[0] if isinstance(axis, (list, tuple)) else axis)

  tf.stack, tf.to_float, tf.to_int32, tf.matmul, tf.map_fn, tf.reduce_mean, tf.squeeze = (
      stack, to_float, to_int32, matmul, map_fn, reduce_mean, squeeze)
  tf.cos = lambda x: R(torch.tensor(np.cos(np.float32(float(x)))))
  tf.sin = lambda x: R(torch.tensor(np.sin(np.float32(float(x)))))
  tf.gather = lambda params, indices, **kw: R(params)[int(indices)] if R(indices).dim() == 0 else R(params)[R(indices).long()]
  tf.logging = ns('logging', info=lambda *a, **k: None)
  tf.device = _Ctx


def images():
  rng = np.random.default_rng(20312)
  a = rng.integers(0, 256, (37, 53, 3)).astype(np.uint8)      # odd-sized
  b = rng.integers(0, 256, (31, 22, 3)).astype(np.uint8)      # taller than wide
  c = np.full((14, 11, 3), 93, np.uint8)                      # all-constant
  return {'a': a, 'b': b, 'c': c}


# interior; touching two borders; pushed fully outside by a translation of 50 pixels either way; zero width
BOXES = np.asarray([[0.25, 0.3, 0.7, 0.8], [0.5, 0.6, 1.0, 1.0], [0.05, 0.02, 0.3, 0.25], [0.2, 0.5, 0.6, 0.5]], np.float32)


def sign_u(sign):
  return 0.75 if sign > 0 else 0.25


def applied(u, prob):
  return bool(np.floor(np.float32(u) + np.float32(prob)) != 0)


def inner_draws(name, n_boxes, box_u, cy_u, cx_u):
  if name == 'Cutout':
    return [cy_u, cx_u]
  if name == 'BBox_Cutout' and n_boxes > 0:
    return [box_u, cy_u, cx_u]
  return []


def policy_queue(table, select, apply_u, signs, box_u, cy_u, cx_u, n_boxes):
  """The tf.random_uniform calls of distort_image_with_autoaugment in the order this stand-in makes them: the random negation
  of every signed operation of the table while it is parsed (:1566-1573), the sub-policy (:1527), then along the selected
  one the apply draw (:1516-1517) and -- where it applies -- the operation's own draws."""
  q = []
  for s, sub in enumerate(table):
    for k, (name, _, _) in enumerate(sub):
      if name in SIGNED:
        q.append(sign_u(signs[k]) if s == select else 0.75)
  q.append((select + 0.5) / len(table))
  for k, (name, prob, _) in enumerate(table[select]):
    q.append(apply_u[k])
    if applied(apply_u[k], prob):
      q += inner_draws(name, n_boxes, box_u[k], cy_u[k], cx_u[k])
  return q


def randaug_queue(op, sign, cy_u, cx_u):
  """distort_image_with_randaugment with one layer (:1654-1666): the operation, then per candidate its `prob`, its random
  negation where it has one and -- for the selected one -- its own draws."""
  q = [(op + 0.5) / len(RANDAUG_OPS)]
  for i, name in enumerate(RANDAUG_OPS):
    q.append(0.5)
    if name in SIGNED:
      q.append(sign_u(sign) if i == op else 0.75)
    if i == op:
      q += inner_draws(name, len(BOXES), 0.0, cy_u, cx_u)
  return q


def main():
  tf = mini_keras.build_tf()
  add_tensor_ops(tf)
  add_randaug_ops(tf)
  add_box_ops(tf)
  mini_keras.install(tf)
  sys.modules['tensorflow_addons'].image = make_image_ops()
  for name in ('hparams_config', 'autoaugment'):
    sys.modules.pop(name, None)
  sys.path.insert(0, REF)
  sys.path.insert(0, os.path.join(REF, 'aug'))
  import autoaugment as ref_aa     # noqa: the reference module
  import hparams_config as ref_hparams    # noqa
  assert ref_aa.__file__.startswith(REF), ref_aa.__file__
  hp = ref_hparams.Config(dict(cutout_max_pad_fraction=0.75, cutout_bbox_replace_with_mean=False, cutout_const=100,
                               translate_const=250, cutout_bbox_const=50, translate_bbox_const=120))      # :1620-1626
  out = {'boxes': BOXES}
  imgs = images()
  for key, img in imgs.items():
    out['image/' + key] = img

  def tensors(key, boxes=BOXES):
    return R(torch.from_numpy(imgs[key].copy())), R(torch.from_numpy(np.array(boxes, np.float32).reshape(-1, 4)))

  # ---- every operation through _parse_policy_info
  stacks, bstacks, names, draws = ({k: [] for k in imgs} for _ in range(4))
  case = 0
  for name in OPS:
    for level in LEVELS:
      for sign in ((1, -1) if name in SIGNED else (1,)):
        for key in imgs:
          case += 1
          box_u, cy_u, cx_u = ((case * 7) % 16 + 0.5) / 16.0, ((case * 5) % 13 + 0.37) / 13.0, ((case * 3) % 11 + 0.81) / 11.0
          QUEUE[:] = [sign_u(sign)] if name in SIGNED else []
          func, _, args = ref_aa._parse_policy_info(name, 0.5, float(level), [128] * 3, hp)
          assert not QUEUE
          QUEUE[:] = inner_draws(name, len(BOXES), box_u, cy_u, cx_u)
          image, boxes = tensors(key)
          res, rbox = func(image, boxes, *args)
          assert not QUEUE, (name, QUEUE)
          res, rbox = res.numpy(), rbox.numpy()
          assert res.dtype == np.uint8 and res.shape == imgs[key].shape and rbox.dtype == np.float32 and rbox.shape == BOXES.shape
          stacks[key].append(res)
          bstacks[key].append(rbox)
          names[key].append('%s/l%d/%s' % (name, level, 'p' if sign > 0 else 'n'))
          draws[key].append([box_u, cy_u, cx_u])
        if sign > 0:
          out['args/%s/l%d' % (name, level)] = np.asarray([float(a) for a in args if not isinstance(a, list)], np.float64)
  for key in imgs:
    out['cases/' + key] = np.stack(stacks[key])
    out['case_boxes/' + key] = np.stack(bstacks[key])
    out['names/' + key] = np.asarray(names[key])
    out['case_draws/' + key] = np.asarray(draws[key], np.float64)

  # ---- BBox_Cutout without boxes
  QUEUE[:] = []
  func, _, args = ref_aa._parse_policy_info('BBox_Cutout', 1.0, 10.0, [128] * 3, hp)
  image, boxes = tensors('a', np.zeros((0, 4), np.float32))
  res, rbox = func(image, boxes, *args)
  assert not QUEUE and tuple(rbox.shape) == (0, 4)
  out['noboxes/out'] = res.numpy()

  # ---- the policies: every sub-policy under two apply draws
  for pname in ('test', 'v2', 'v3'):
    table = getattr(ref_aa, 'policy_v' + pname.replace('v', ''))()
    out['policy/%s/ops' % pname] = np.asarray([['%s' % op for op, _, _ in sub] + [''] * (3 - len(sub)) for sub in table])
    out['policy/%s/prob' % pname] = np.asarray([[p for _, p, _ in sub] + [-1.0] * (3 - len(sub)) for sub in table], np.float64)
    out['policy/%s/level' % pname] = np.asarray([[l for _, _, l in sub] + [-1] * (3 - len(sub)) for sub in table], np.float64)
    runs = []
    for select in range(len(table)):
      for v, au in enumerate((0.999, 0.5)):
        n = len(runs)
        apply_u = [au] * 3
        signs = [1 if (n + k) % 2 == 0 else -1 for k in range(3)]
        box_u = [((n * 3 + k) % 4 + 0.5) / 4.0 for k in range(3)]
        cy_u = [((n * 5 + k) % 9 + 0.3) / 9.0 for k in range(3)]
        cx_u = [((n * 7 + k) % 8 + 0.6) / 8.0 for k in range(3)]
        key = 'a' if n % 3 == 0 else 'b'
        q = policy_queue(table, select, apply_u, signs, box_u, cy_u, cx_u, len(BOXES))
        QUEUE[:] = q
        image, boxes = tensors(key)
        res, rbox = ref_aa.distort_image_with_autoaugment(image, boxes, pname)
        assert not QUEUE, (pname, select, QUEUE)
        tag = 'run/%s/%02d_%d' % (pname, select, v)
        out[tag + '/out'], out[tag + '/boxes'] = res.numpy().astype(np.uint8), rbox.numpy().astype(np.float32)
        out[tag + '/queue'] = np.asarray(q, np.float64)
        out[tag + '/image'] = np.asarray(key)
        out[tag + '/draws'] = np.asarray([[select] * 3, apply_u, signs, cy_u, cx_u, box_u], np.float64)
        runs.append(tag)
    print(pname, len(runs), 'runs')

  # ---- RandAugment as the data loader calls it (dataloader.py:315-316)
  for op, name in enumerate(RANDAUG_OPS):
    sign = 1 if op % 2 == 0 else -1
    cy_u, cx_u = (op * 3 % 7 + 0.4) / 7.0, (op * 5 % 9 + 0.2) / 9.0
    key = 'a' if op % 2 == 0 else 'b'
    q = randaug_queue(op, sign, cy_u, cx_u)
    QUEUE[:] = q
    image, boxes = tensors(key)
    res, rbox = ref_aa.distort_image_with_randaugment(image, boxes, 1, 15)
    assert not QUEUE, (name, QUEUE)
    tag = 'randaug/%d' % op
    out[tag + '/out'], out[tag + '/boxes'] = res.numpy().astype(np.uint8), rbox.numpy().astype(np.float32)
    out[tag + '/queue'] = np.asarray(q, np.float64)
    out[tag + '/image'] = np.asarray(key)
    out[tag + '/draws'] = np.asarray([op, sign, cy_u, cx_u], np.float64)
  path = os.path.join(HERE, 'reference_det_autoaugment.npz')
  np.savez_compressed(path, **out)
  print(path, len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
