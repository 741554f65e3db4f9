"""Generates tests/golden/reference_mosaic.npz by EXECUTING the reference's aug/mosaic.py -- unmodified -- on the torch-backed
`tf` stand-in: Mosaic.__call__ (divide points, _scale_images, _mosaic with its vectorized_map / tensor_scatter_nd_add box
arithmetic, the three concatenations).

The leaf operations it needs beyond mini_keras.build_tf and make_golden_labels.add_tensor_ops:
  tf.image.resize            torch.nn.functional.interpolate(mode='bilinear', align_corners=False, antialias=False) on float32,
                             as in make_golden_preprocess.py (the same half-pixel rule as TF2's bilinear resize, implemented
                             independently of oracle/preprocess_oracle.py)
  tf.vectorized_map          fn applied to every row, the list of results stacked component by component
  tf.tensor_scatter_nd_add   rows idx of the stacked operand += updates
  tf.transpose / tf.concat / tf.constant / tf.shape / tf.cast, tf.function as the identity
  tf.random.uniform          returns values QUEUED by this script (stored with the outputs), and records the bounds it was
                             called with; a queued value may lie outside them -- at these tiny output sizes the reference
                             itself would never draw a seam at 1 or out - 1, which the fixture wants for the placement
  absl.logging               a stub
TensorFlow's integer true division yields float64 (int32 * int32 / int32 in _scale_box); torch's yields the default dtype,
which is therefore float64 while the reference runs.

aug/mosaic.py calls typing.Tuple(int, int) in an annotation, which raises a TypeError at import on this Python (3.10).  For
the duration of the import ONLY, typing.Tuple is replaced by an object that is callable as well as subscriptable; it is put
back before anything else runs.

The reference indexes `images` and reads images.shape[0]; four images of different sizes are handed over as a small
container with exactly that (TensorFlow would need a ragged tensor; the reference's arithmetic per image is the same).

Only inputs, queued draws and outputs are written: no reference text.
Run in the build container only (needs /root/reference):  python tests/golden/make_golden_mosaic.py
"""
import importlib.util
import os
import sys
import typing

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mini_keras   # noqa
from mini_keras import T, ns   # noqa
from make_golden_anchors import REF   # noqa
from make_golden_labels import add_tensor_ops   # noqa

DRAWS = []      # values handed out by tf.random.uniform, in call order
BOUNDS = []     # (minval, maxval) of every call


def add_mosaic_ops(tf):
  def resize(image, size, method=None, **kw):
    x = T(image).to(torch.float32).permute(2, 0, 1)[None]
    y = torch.nn.functional.interpolate(x, size=(int(size[0]), int(size[1])), mode='bilinear', align_corners=False,
                                        antialias=False)
    return T(y[0].permute(1, 2, 0).contiguous())

  def uniform(shape=(), minval=0, maxval=None, dtype=None, seed=None, **kw):
    assert dtype == torch.int32 and list(shape) == [1], (dtype, shape)
    BOUNDS.append((int(minval), int(maxval)))
    return T(torch.tensor([DRAWS.pop(0)], dtype=torch.int32))

  def stacked(x):
    return torch.stack([T(v) for v in x]) if isinstance(x, (list, tuple)) else T(x)

  def vectorized_map(fn, elems):
    rows = [fn(row) for row in T(elems)]
    return [torch.stack([T(r[k]) for r in rows]) for k in range(len(rows[0]))]

  def tensor_scatter_nd_add(tensor, indices, updates):
    out = stacked(tensor).clone()
    idx = T(indices).long().reshape(-1)
    out[idx] += torch.as_tensor(np.asarray(updates)).to(out.dtype)
    return T(out)

  tf.image = ns('image', resize=resize)
  tf.random = ns('random', uniform=uniform)
  tf.vectorized_map = vectorized_map
  tf.tensor_scatter_nd_add = tensor_scatter_nd_add
  tf.transpose = lambda x, perm=None: stacked(x).t()
  tf.function = lambda f: f


class _CallableTuple(object):
  """typing.Tuple that may also be CALLED, as aug/mosaic.py's annotations do."""

  def __init__(self, real):
    self._real = real

  def __getitem__(self, item):
    return self._real[item]

  def __call__(self, *items):
    return self._real[items]


def import_reference():
  spec = importlib.util.spec_from_file_location('reference_aug_mosaic', os.path.join(REF, 'aug', 'mosaic.py'))
  module = importlib.util.module_from_spec(spec)
  real = typing.Tuple
  typing.Tuple = _CallableTuple(real)
  try:
    spec.loader.exec_module(module)
  finally:
    typing.Tuple = real
  return module


class Images(object):
  """Four images of their own sizes: what Mosaic.__call__ reads of `images` is shape[0] and the items."""

  def __init__(self, items):
    self.items = [T(torch.from_numpy(i)) for i in items]
    self.shape = (len(items),)

  def __getitem__(self, k):
    return self.items[k]


RAGGED = ((5, 7), (4, 4), (9, 3), (1, 1))
TINY = ((4, 4),) * 4      # the "tiny images" of the reference's mosaic_test.py
CASES = {   # name: (source sizes, out_size, (x, y), seed)
    'ragged_seam_in_run': (RAGGED, (8, 12), (3, 5), 1),            # the column seam y = 5 inside a run of four pixels
    'ragged_seam_on_run': (RAGGED, (8, 12), (1, 4), 2),            # y = 4 on a run boundary, the row seam at 1
    'ragged_scalar_rows': (RAGGED, (7, 10), (6, 5), 3),            # rows that are no multiple of 4, the row seam at out0 - 1
    'tiny_equal': (TINY, (8, 12), (7, 4), 4),                      # the row seam at out0 - 1
    'tiny_equal_odd': (TINY, (7, 10), (1, 5), 5),
}


def boxes_of(rng, h, w):
  """Two int32 boxes [x1, y1, x2, y2] of an h x w image; the second touches the far corner."""
  x1, y1 = int(rng.integers(0, w)), int(rng.integers(0, h))
  first = [x1, y1, int(rng.integers(x1, w + 1)), int(rng.integers(y1, h + 1))]
  return np.asarray([first, [w // 2, h // 3, w, h]], np.int32)


def main():
  tf = mini_keras.build_tf()
  add_tensor_ops(tf)
  add_mosaic_ops(tf)
  mini_keras.install(tf)
  sys.modules['absl'].logging = sys.modules['absl.logging'] = ns('absl.logging', error=lambda *a, **k: None,
                                                                 info=lambda *a, **k: None)
  ref = import_reference()
  assert typing.Tuple[int, int] is not None and not isinstance(typing.Tuple, _CallableTuple)
  torch.set_default_dtype(torch.float64)      # TensorFlow's integer true division (module docstring)
  out = {}
  for name, (sizes, out_size, (x, y), seed) in CASES.items():
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    boxes = [boxes_of(rng, h, w) for h, w in sizes]
    DRAWS[:], BOUNDS[:] = [x, y], []
    mosaic = ref.Mosaic(out_size=out_size)
    image, mboxes = mosaic(Images(images), [T(torch.from_numpy(b)) for b in boxes])
    assert not DRAWS and tuple(image.shape) == out_size + (3,) and image.dtype == torch.float32, (image.shape, image.dtype)
    assert all(b.dtype == torch.float64 and tuple(b.shape) == (2, 4) for b in mboxes), [(b.dtype, b.shape) for b in mboxes]
    for k in range(4):
      out['%s/image_%d' % (name, k)] = images[k]
    out[name + '/boxes_in'] = np.stack(boxes)
    out[name + '/out_size'] = np.asarray(out_size, np.int32)
    out[name + '/draws'] = np.asarray([x, y], np.int32)
    out[name + '/bounds'] = np.asarray(BOUNDS, np.int32)
    out[name + '/mosaic'] = image.numpy().astype(np.float32)
    out[name + '/boxes'] = np.stack([b.numpy() for b in mboxes]).astype(np.float64)
    print(name, out_size, (x, y), BOUNDS, out[name + '/boxes'].reshape(-1)[:4])
  # the default Mosaic(): the bounds of the two draws, no image work
  DRAWS[:], BOUNDS[:] = [170, 509], []
  px, py = ref.Mosaic()._mosaic_divide_points()
  out['default/out_size'] = np.asarray([680, 680], np.int32)
  out['default/draws'] = np.asarray([int(px[0]), int(py[0])], np.int32)
  out['default/bounds'] = np.asarray(BOUNDS, np.int32)
  print('default', BOUNDS)
  np.savez_compressed(os.path.join(HERE, 'reference_mosaic.npz'), **out)


if __name__ == '__main__':
  main()
