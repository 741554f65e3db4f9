"""Generates tests/golden/reference_legacy.npz by EXECUTING the reference's efficientnetv2/preprocess_legacy.py -- unmodified --
on the torch-backed `tf` stand-in of make_golden_randaug.py, with the reference's own autoaugment.py behind it:
preprocess_image(is_training=False) on images of nine sizes at two target sizes, and preprocess_image(is_training=True) with
augment_name None / 'autoaug' / 'randaug' for queued boxes (a real crop, and the whole image = the "bad" fallback) and both
flip outcomes.

What the fixture pins is the module's WIRING: the sampler's keyword values (:88-98), the "bad" test and its centre-crop
fallback (:99-105), the centre crop's size and offsets (:110-127), flip after resize, the clip / cast in front of the
augmentation (:168-169) and the cast back, AutoAugment 'v0' / RandAugment's arguments, the normalisation constants (:240-243).
Stubs, fed from queues and stored arrays: tf.image.extract_jpeg_shape (the stored image's shape), sample_distorted_bounding_box
(the queued box; its keyword values are stored), decode_and_crop_jpeg (a slice of the stored image; the windows are stored;
an empty window is refused, as TensorFlow's op refuses it), random_flip_left_right (a queued uniform, flipped below 0.5).
tf.image.resize_bicubic is a leaf of this script, written independently of tests/bicubic_ref.py from TensorFlow's published
resize_bicubic_op (legacy: align_corners=False, half_pixel_centers=False, the 1024-entry table with a = -0.75): one output
value at a time in scalar float32 arithmetic.  It cannot be pinned against TensorFlow here.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_legacy.py
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mini_keras   # noqa
import make_golden_randaug as mgr   # noqa
import make_golden_autoaug as mga   # noqa
from make_golden_labels import add_tensor_ops   # noqa

f32 = np.float32
BOXES, FLIPS, WINDOWS, SAMPLER_KW = [], [], [], []
EVAL_SIZES = [(33, 40), (40, 33), (34, 34), (1, 5), (5, 1), (2, 2), (2, 7), (17, 31), (24, 20)]
EVAL_TARGETS = (8, 11)
TRAIN_TARGET = 12
# (name, image size, queued box (y, x, h, w), flip uniform, augment_name)
TRAIN_CASES = [
    ('crop', (33, 40), (3, 5, 20, 17), 0.75, None), ('crop_flip', (33, 40), (0, 23, 33, 17), 0.25, None),
    ('bad', (33, 40), (0, 0, 33, 40), 0.75, None), ('bad_flip', (40, 33), (0, 0, 40, 33), 0.25, None),
    ('one_side_equal', (17, 31), (0, 4, 17, 20), 0.25, None),      # not "bad": only height and channels agree
    ('autoaug', (24, 20), (2, 1, 20, 18), 0.25, 'autoaug'), ('autoaug_bad', (17, 31), (0, 0, 17, 31), 0.75, 'autoaug'),
    ('randaug', (24, 20), (0, 0, 13, 20), 0.75, 'randaug'), ('randaug_flip', (34, 34), (9, 9, 25, 25), 0.25, 'randaug'),
]
AUTOAUG = {'autoaug': (14, (0.999, 0.999), -1), 'autoaug_bad': (21, (0.9, 0.9), 1)}      # sub-policy, apply draws, sign
RANDAUG = {'randaug': (2, 9, [9, 12], [1, -1]), 'randaug_flip': (2, 9, [3, 6], [-1, 1])}      # layers, magnitude, ops, signs


def cubic_table():
  a = -0.75
  t = []
  for i in range(1025):
    x = float(f32(i / 1024.0))
    inner = ((a + 2) * x - (a + 3)) * x * x + 1
    x1 = float(f32(f32(x) + f32(1.0)))
    outer = ((a * x1 - 5 * a) * x1 + 8 * a) * x1 - 4 * a
    t.append((f32(inner), f32(outer)))
  return t


TABLE = cubic_table()


def axis(o, in_n, out_n):
  scale = f32(f32(in_n) / f32(out_n))
  pos = f32(f32(o) * scale)
  base = int(math.floor(float(pos)))
  delta = f32(pos - f32(base))
  off = int(np.rint(f32(delta * f32(1024.0))))
  taps = [min(max(base - 1 + k, 0), in_n - 1) for k in range(4)]
  return taps, [TABLE[off][1], TABLE[off][0], TABLE[1024 - off][0], TABLE[1024 - off][1]]


def resize_bicubic_leaf(image, out_h, out_w):
  img = np.asarray(image, np.float32)
  h, w, ch = img.shape
  out = np.zeros((out_h, out_w, ch), np.float32)
  xs = [axis(x, w, out_w) for x in range(out_w)]
  for y in range(out_h):
    ty, wy = axis(y, h, out_h)
    for x in range(out_w):
      tx, wx = xs[x]
      for c in range(ch):
        cols = []
        for k in range(4):
          s = f32(img[ty[0], tx[k], c] * wy[0])
          for j in range(1, 4):
            s = f32(s + f32(img[ty[j], tx[k], c] * wy[j]))
          cols.append(s)
        v = f32(cols[0] * wx[0])
        for k in range(1, 4):
          v = f32(v + f32(cols[k] * wx[k]))
        out[y, x, c] = v
  return out


class EmptyWindow(Exception):
  pass


def add_legacy_ops(tf, store):
  R = mgr.R

  def extract_jpeg_shape(image_bytes):
    return R(torch.tensor(list(store[image_bytes].shape), dtype=torch.int32))

  def sample_distorted_bounding_box(shape, bounding_boxes=None, **kw):
    y, x, h, w = BOXES.pop(0)
    SAMPLER_KW.append(dict(kw, bounding_boxes=np.asarray(bounding_boxes).tolist()))
    return R(torch.tensor([y, x, 0], dtype=torch.int32)), R(torch.tensor([h, w, -1], dtype=torch.int32)), None

  def decode_and_crop_jpeg(image_bytes, crop_window, channels=3):
    y, x, h, w = (int(v) for v in crop_window)
    WINDOWS.append((y, x, h, w))
    if h < 1 or w < 1:
      raise EmptyWindow((y, x, h, w))
    img = store[image_bytes]
    assert 0 <= y and y + h <= img.shape[0] and 0 <= x and x + w <= img.shape[1], ((y, x, h, w), img.shape)
    return R(torch.from_numpy(img[y:y + h, x:x + w].copy()))

  def resize_bicubic(images, size):
    assert len(images) == 1
    return R(torch.from_numpy(resize_bicubic_leaf(images[0].numpy(), int(size[0]), int(size[1])))[None])

  def random_flip_left_right(image):
    return R(torch.flip(image, dims=[1])) if FLIPS.pop(0) < 0.5 else image

  def convert_image_dtype(image, dtype=None):
    assert image.dtype == torch.float32 and dtype == torch.float32, (image.dtype, dtype)      # (no rescaling between floats)
    return image

  image_ns = tf.image
  for name, fn in (('extract_jpeg_shape', extract_jpeg_shape), ('sample_distorted_bounding_box', sample_distorted_bounding_box),
                   ('decode_and_crop_jpeg', decode_and_crop_jpeg), ('resize_bicubic', resize_bicubic),
                   ('random_flip_left_right', random_flip_left_right), ('convert_image_dtype', convert_image_dtype)):
    setattr(image_ns, name, fn)
  tf.logging = mini_keras.ns('logging', info=lambda *a, **k: None)
  tf.shape = lambda x: R(torch.tensor(list(x.shape), dtype=torch.int32))


def main():
  tf = mini_keras.build_tf()
  add_tensor_ops(tf)
  mgr.add_randaug_ops(tf)
  store = {}
  add_legacy_ops(tf, store)
  mini_keras.install(tf)
  sys.modules['tensorflow_addons'].image = mgr.make_image_ops()
  sys.modules['absl'].logging = mini_keras.ns('logging', info=lambda *a, **k: None)
  sys.modules.pop('hparams', None)
  sys.path.insert(0, mgr.REF)
  import autoaugment as ref_aa     # noqa: the reference module, imported by preprocess_legacy
  import preprocess_legacy as ref_pl     # noqa: the reference module
  rng = np.random.default_rng(20212)
  out = {}
  for h, w in sorted(set(EVAL_SIZES + [c[1] for c in TRAIN_CASES])):
    store['%dx%d' % (h, w)] = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    out['image/%dx%d' % (h, w)] = store['%dx%d' % (h, w)]
  # ---- eval
  out['eval/sizes'] = np.asarray(EVAL_SIZES, np.int32)
  out['eval/targets'] = np.asarray(EVAL_TARGETS, np.int32)
  for target in EVAL_TARGETS:
    windows = []
    for h, w in EVAL_SIZES:
      WINDOWS[:] = []
      try:
        res = ref_pl.preprocess_image('%dx%d' % (h, w), target, is_training=False)
        res = res.numpy()
        assert res.dtype == np.float32 and res.shape == (target, target, 3), (res.dtype, res.shape)
        out['eval/%d/out/%dx%d' % (target, h, w)] = res
      except EmptyWindow:
        pass      # min(h, w) = 1: the reference asks for a window of 0 x 0
      assert len(WINDOWS) == 1
      windows.append(WINDOWS[0])
    out['eval/%d/windows' % target] = np.asarray(windows, np.int32)
  # ---- train
  table = ref_aa.policy_v0()
  names = []
  for name, (h, w), box, flip_u, augment in TRAIN_CASES:
    BOXES[:], FLIPS[:], WINDOWS[:], SAMPLER_KW[:] = [box], [flip_u], [], []
    if augment == 'autoaug':
      sub, apply_u, sign = AUTOAUG[name]
      mgr.QUEUE[:] = mga.queue_of(table, sub, apply_u, sign)
      out['train/%s/autoaug' % name] = np.asarray([sub, apply_u[0], apply_u[1], sign], np.float64)
      kw = {}
    elif augment == 'randaug':
      layers, magnitude, ops, signs = RANDAUG[name]
      mgr.QUEUE[:] = mgr.ra_queue(ops, signs, [(0, 0)] * layers)
      out['train/%s/randaug' % name] = np.asarray([layers, magnitude] + ops + signs, np.float64)
      kw = dict(randaug_num_layers=layers, randaug_magnitude=magnitude)
    else:
      mgr.QUEUE[:] = []
      kw = {}
    res = ref_pl.preprocess_image('%dx%d' % (h, w), TRAIN_TARGET, is_training=True, augment_name=augment, **kw)
    assert not BOXES and not FLIPS and not mgr.QUEUE, (BOXES, FLIPS, mgr.QUEUE)
    res = res.numpy()
    assert res.dtype == np.float32 and res.shape == (TRAIN_TARGET, TRAIN_TARGET, 3), (res.dtype, res.shape)
    names.append(name)
    out['train/%s/out' % name] = res
    out['train/%s/size' % name] = np.asarray([h, w], np.int32)
    out['train/%s/box' % name] = np.asarray(box, np.int32)
    out['train/%s/flip_u' % name] = np.asarray(flip_u, np.float64)
    out['train/%s/windows' % name] = np.asarray(WINDOWS, np.int32)      # the sampler's, then the fallback's when "bad"
    out['train/%s/augment' % name] = np.asarray(augment or '')
    kwv = SAMPLER_KW[0]
    out['train/%s/sampler' % name] = np.asarray([kwv['min_object_covered'], kwv['aspect_ratio_range'][0], kwv['aspect_ratio_range'][1],
                                                 kwv['area_range'][0], kwv['area_range'][1], kwv['max_attempts'],
                                                 float(kwv['use_image_if_no_bounding_boxes'])], np.float64)
    out['train/%s/sampler_boxes' % name] = np.asarray(kwv['bounding_boxes'], np.float64)
  out['train/names'] = np.asarray(names)
  out['train/target'] = np.asarray(TRAIN_TARGET, np.int32)
  try:
    BOXES[:], FLIPS[:] = [(0, 0, 5, 5)], [0.75]
    ref_pl.preprocess_image('24x20', TRAIN_TARGET, is_training=True, augment_name='v0')
    raise AssertionError('augment_name v0 accepted')
  except ValueError as e:
    out['invalid_name_message'] = np.asarray(str(e))
  path = os.path.join(HERE, 'reference_legacy.npz')
  np.savez_compressed(path, **out)
  print(path, len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
