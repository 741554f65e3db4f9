"""Generates tests/golden/reference_det_eval.npz by EXECUTING the reference's evaluation input branch -- unmodified -- on the
torch-backed `tf` stand-in: dataloader.InputReader.dataset_parser(is_training=False) per image, with example_decoder.decode
stubbed to return the arrays and a stub anchor labeler (labelling is pinned by reference_labels.npz), then
InputReader.process_example on the stacked images for the concatenation of groundtruth_data (dataloader.py:253-394).  So
set_scale_factors_to_output_size, resize_and_crop_boxes with its zero-area filter, the source-id parsing, image_scale_to_original,
the four pad_to_fixed_size calls and the concat are all the reference's code.

Stand-in additions made here: strings (tf.constant(''), tf.equal and tf.where on python strings, tf.strings.to_number),
tf.name_scope / tf.control_dependencies as null contexts, and tf.assert_less, which really asserts.

Run where a checkout of the reference is available:  python tests/golden/make_golden_det_eval.py
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mini_keras   # noqa
from mini_keras import T, ns   # noqa
from make_golden_anchors import REF   # noqa
from make_golden_labels import add_tensor_ops   # noqa
from make_golden_preprocess import add_image_ops   # noqa

MAX_INSTANCES = 8
OUTPUT_SIZE = (128, 128)
MEAN = [0.485 * 255, 0.456 * 255, 0.406 * 255]
STD = [0.229 * 255, 0.224 * 255, 0.225 * 255]


def add_eval_ops(tf):
  base_constant, base_equal, base_where, base_cast = tf.constant, getattr(tf, 'equal', None), tf.where, tf.cast
  tf.constant = lambda v, *a, **k: v if isinstance(v, str) else base_constant(v, *a, **k)
  tf.equal = lambda a, b: (a == b) if isinstance(a, str) else base_equal(a, b)

  def where(cond, x=None, y=None):
    if isinstance(cond, bool):
      return x if cond else y
    return base_where(cond) if x is None else base_where(cond, x, y)
  tf.where = where
  tf.strings = ns('strings', to_number=lambda s: T(torch.tensor(np.float32(float(s)))))
  tf.name_scope = lambda *a, **k: contextlib.nullcontext()
  tf.control_dependencies = lambda deps: contextlib.nullcontext()

  def assert_less(x, y, message=None):
    assert int(x) < int(y), message
  tf.assert_less = assert_less
  tf.cast = lambda x, dtype=None: (torch.as_tensor(np.asarray(x)).to(dtype) if isinstance(x, np.ndarray)
                                   else base_cast(x, dtype=dtype))


class Decoder(object):
  def __init__(self, example):
    self.example = example

  def decode(self, value):
    return self.example


class Labeler(object):
  """label_anchors is not what this fixture is about: dataset_parser only hands its results through."""

  def label_anchors(self, boxes, classes):
    return {}, {}, T(torch.tensor(0.0))


def boxes_for(rng, n):
  y0, x0 = rng.uniform(0.0, 0.6, n), rng.uniform(0.0, 0.6, n)
  return np.stack([y0, x0, y0 + rng.uniform(0.15, 0.4, n), x0 + rng.uniform(0.15, 0.4, n)], -1).astype(np.float32)


def cases():
  """name -> (raw height, raw width, box rows M, [per image (count, source id, zero-area rows, crowd rows)])."""
  return {
      # M == max_instances_per_image.  Image 0: a box without area in the middle (row 2) FOLLOWED by a crowd annotation (row
      # 3), so the kept boxes move up a row and the crowd flag does not; image 1: no box and no source id; image 2: 7 of 8
      'rows_at_max': (40, 56, 8, [(6, '139', [2], [3]), (0, '', [], []), (7, '785', [], [6])]),
      # M < max_instances_per_image, another raw size (the height decides the scale); two boxes without area, the first row too
      'rows_below_max': (64, 48, 5, [(5, '42', [0, 3], [1, 4]), (2, '7', [], [])]),
  }


def main():
  tf = mini_keras.build_tf()
  add_tensor_ops(tf)
  add_image_ops(tf)
  add_eval_ops(tf)
  mini_keras.install(tf)
  sys.modules.pop('dataloader', None)          # the real module, not the import stub
  sys.path.insert(0, REF)
  import dataloader as ref_dl     # noqa: the reference module
  params = {'image_size': OUTPUT_SIZE, 'mean_rgb': MEAN, 'stddev_rgb': STD, 'scale_range': False, 'mixed_precision': False,
            'data_format': 'channels_last', 'min_level': 3, 'max_level': 2}      # (no level: the stub labeler has none)
  reader = ref_dl.InputReader(None, is_training=False, max_instances_per_image=MAX_INSTANCES)
  rng = np.random.default_rng(20261)
  out = {'max_instances': np.int32(MAX_INSTANCES), 'output_size': np.asarray(OUTPUT_SIZE, np.int32)}
  for name, (h, w, m, images) in cases().items():
    b = len(images)
    raw = rng.integers(0, 256, (b, h, w, 3)).astype(np.uint8)
    boxes, classes = np.zeros((b, m, 4), np.float32), np.zeros((b, m), np.float32)
    crowds, areas = np.zeros((b, m), np.float32), np.zeros((b, m), np.float32)
    counts, ids, rows = np.zeros(b, np.int32), [], []
    for i, (n, sid, flat, crowd) in enumerate(images):
      counts[i] = n
      boxes[i, :n] = boxes_for(rng, n)
      for r in flat:
        boxes[i, r, 2] = boxes[i, r, 0]      # ymax = ymin: no area
      classes[i, :n] = rng.integers(1, 91, n)
      crowds[i, crowd] = 1
      areas[i, :n] = rng.uniform(10.0, 2000.0, n).astype(np.float32)
      ids.append(sid)
      example = {'source_id': sid, 'image': T(torch.from_numpy(raw[i])),
                 'groundtruth_boxes': T(torch.from_numpy(boxes[i, :n].copy())),
                 'groundtruth_classes': T(torch.from_numpy(classes[i, :n].astype(np.int64))),
                 'groundtruth_area': T(torch.from_numpy(areas[i, :n].copy())),
                 'groundtruth_is_crowd': T(torch.from_numpy(crowds[i, :n] != 0))}
      rows.append(reader.dataset_parser(None, Decoder(example), Labeler(), params))
    (image, cls_t, box_t, npos, source_id, image_scale, gboxes, gcrowds, gareas, gclasses, masks) = [
        [r[k] for r in rows] for k in range(11)]
    stack = lambda ts: T(torch.stack([torch.as_tensor(t) for t in ts]))      # noqa: E731 -- what dataset.batch does
    _, labels = reader.process_example(params, b, stack(image), {}, {}, stack(npos), stack(source_id), stack(image_scale),
                                       stack(gboxes), stack(gcrowds), stack(gareas), stack(gclasses), [])
    gt = labels['groundtruth_data'].numpy()
    assert gt.dtype == np.float32 and gt.shape == (b, MAX_INSTANCES, 7), (gt.dtype, gt.shape)
    out[name + '/raw'], out[name + '/boxes'], out[name + '/classes'], out[name + '/counts'] = raw, boxes, classes, counts
    out[name + '/is_crowds'], out[name + '/areas'] = crowds, areas
    out[name + '/source_id_strings'] = np.asarray(ids)
    out[name + '/groundtruth_data'] = gt
    out[name + '/image_scales'] = labels['image_scales'].numpy().astype(np.float32)
    out[name + '/source_ids'] = labels['source_ids'].numpy().astype(np.float32)
    print(name, gt.shape, out[name + '/image_scales'], out[name + '/source_ids'])
    print(gt[0])
  path = os.path.join(HERE, 'reference_det_eval.npz')
  np.savez_compressed(path, **out)
  print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
