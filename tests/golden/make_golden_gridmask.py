"""Generates tests/golden/reference_gridmask.npz by EXECUTING the reference's efficientdet/aug/gridmask.py -- unmodified --
on numpy-backed stand-ins for `tensorflow` and `tensorflow_addons.image`, with the random draws injected: GridMask.mask(h, w)
on its own, and the whole GridMask.__call__ on small uint8 images, for three sizes and a few draws each.

What the fixture pins is the reference's WIRING: the mask side, the length formula, the stripe loop and the order of the two
scatter-and-transpose passes (which start lands on rows), crop, the occurrence branch (a normal draw against prob), the
final multiply with 1 = kept.  The stand-in's `rotate` is tests/gridmask_ref.py's own function, so the fixture says NOTHING
about TensorFlow Addons' rotation (coefficients, bilinear rounding, truncation): that stays unpinned.  tf.random.uniform /
tf.random.normal return values queued by this script; the queues are stored with the outputs.

Needs a checkout of the reference:  python tests/golden/make_golden_gridmask.py <reference>/efficientdet
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gridmask_ref   # noqa: E402

QUEUE = []      # values handed out by tf.random.uniform / tf.random.normal, in call order


class T(np.ndarray):
  """ndarray with the one private method the reference calls on a tensor."""

  def _rank(self):
    return self.ndim


def t(x, dtype=None):
  return np.asarray(x, dtype=dtype).view(T)


def make_tf():
  tf = types.ModuleType('tensorflow')
  tf.float32, tf.int32 = np.float32, np.int32
  tf.function = lambda fn: fn
  tf.cast = lambda x, dtype: t(np.asarray(x).astype(dtype))      # float -> int truncates
  tf.shape = lambda x: t(np.asarray(x).shape, np.int32)
  tf.zeros = lambda shape, dtype=np.float32: t(np.zeros([int(s) for s in shape], dtype))
  tf.ones = lambda shape, dtype=np.float32: t(np.ones([int(s) for s in shape], dtype))
  tf.range = lambda start, limit: t(np.arange(int(start), int(limit), dtype=np.int32))
  tf.reshape = lambda x, shape: t(np.asarray(x).reshape([int(s) for s in shape]))
  tf.transpose = lambda x: t(np.asarray(x).T.copy())
  tf.expand_dims = lambda x, axis: t(np.expand_dims(np.asarray(x), axis))
  tf.cond = lambda pred, true_fn, false_fn: true_fn() if bool(pred) else false_fn()

  def tensor_scatter_nd_update(tensor, indices, updates):
    out = np.asarray(tensor).copy()
    out[np.asarray(indices)[:, 0]] = np.asarray(updates)
    return t(out)
  tf.tensor_scatter_nd_update = tensor_scatter_nd_update
  tf.math = types.SimpleNamespace(maximum=lambda a, b: t(np.maximum(a, b)), minimum=lambda a, b: t(np.minimum(a, b)))

  def uniform(shape, minval=0, maxval=None, dtype=np.float32):
    assert list(shape) == [] and dtype == np.int32
    v = int(QUEUE.pop(0))
    assert int(minval) <= v < int(maxval), (int(minval), v, int(maxval))
    return t(v, np.int32)

  def normal(shape, mean=0.0, stddev=1.0):
    assert list(shape) == []
    return t(QUEUE.pop(0), np.float32)      # the queued value IS the draw from N(mean, stddev)
  tf.random = types.SimpleNamespace(uniform=uniform, normal=normal)
  return tf


def make_image_ops():
  mod = types.ModuleType('tensorflow_addons.image')

  def rotate(images, angles, interpolation='NEAREST'):
    assert interpolation == 'BILINEAR'
    return t(gridmask_ref.rotate(np.asarray(images), np.float32(angles)))
  mod.rotate = rotate
  return mod


# (h, w): draws (d, s1, s2, z1, z2).  d at both ends of int(min(h / 2, 0.3 w)) .. int(max(..)); starts at 0 and at d,
# with S % d == 0 (the empty last stripe); z2 on both sides of prob = 0.5; z1 = 0 is the unrotated mask
CASES = {
    (13, 11): [(3, 0, 3, -1.0, 0.1), (6, 6, 2, 0.0, -0.7), (4, 1, 4, -2.5, 0.49), (5, 2, 0, 1.0, 0.5)],
    (32, 40): [(12, 12, 0, -1.0, -1.2), (16, 3, 16, 0.0, 0.2), (15, 15, 15, 2.5, 0.3), (13, 7, 5, -0.3, 0.9)],
    (64, 48): [(14, 0, 0, -1.0, 0.0), (32, 32, 9, 0.0, 0.4), (24, 24, 24, -2.5, -0.1), (19, 4, 11, 0.7, 2.0)],
}


def main():
  ref = sys.argv[1]
  sys.modules['tensorflow'] = make_tf()
  addons = types.ModuleType('tensorflow_addons')
  addons.image = make_image_ops()
  sys.modules['tensorflow_addons'] = addons
  sys.modules['tensorflow_addons.image'] = addons.image
  sys.path.insert(0, os.path.join(ref, 'aug'))
  ref_gm = importlib.import_module('gridmask')      # the reference module
  rng = np.random.default_rng(20240)
  out = {}
  for (h, w), draws in CASES.items():
    key = '%dx%d' % (h, w)
    image = rng.integers(1, 256, (h, w, 3)).astype(np.uint8)      # no zero byte: a masked pixel is recognisable
    out['image/' + key] = image
    out['draws/' + key] = np.asarray(draws, np.float64)
    masks, results = [], []
    for d, s1, s2, z1, z2 in draws:
      obj = ref_gm.GridMask(prob=0.5, ratio=0.6, rotate=10, gridmask_size_ratio=0.5, fill=1)
      QUEUE[:] = [d, s1, s2]
      mask = np.asarray(obj.mask(h, w))
      assert not QUEUE and mask.dtype == np.int32 and mask.shape[0] == mask.shape[1], (mask.dtype, mask.shape)
      masks.append(mask.astype(np.uint8))
      QUEUE[:] = [d, s1, s2, z1, z2]
      boxes = np.asarray([[0.1, 0.2, 0.3, 0.4]], np.float32)
      res, label = ref_gm.gridmask(t(image.copy()), boxes)
      assert not QUEUE and label is boxes
      res = np.asarray(res)
      assert res.dtype == np.uint8 and res.shape == image.shape, (res.dtype, res.shape)
      results.append(res)
      print(key, (d, s1, s2, z1, z2), 'S', mask.shape[0], 'kept', int(mask.sum()), 'zeroed bytes', int((res == 0).sum()))
    out['mask/' + key] = np.stack(masks)
    out['out/' + key] = np.stack(results)
  path = os.path.join(HERE, 'reference_gridmask.npz')
  np.savez_compressed(path, **out)
  print(path, len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
