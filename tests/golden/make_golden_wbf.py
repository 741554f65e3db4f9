"""Generates tests/golden/reference_wbf.npz by EXECUTING the reference's efficientdet/tf2/wbf.py -- unmodified -- on the
torch-backed `tf` stand-in (mini_keras.build_tf + make_golden_labels.add_tensor_ops + the leaf operations below): a dozen small
inputs through ensemble_detections with num_models 1, 2 and 3.  Only inputs and outputs are recorded.

Every cluster of these cases has at most two members (asserted: average_detections is watched while the reference runs).  A
float32 sum of two terms has one order, so the fixture pins tests/wbf_ref.py bit for bit without saying anything about
reduce_sum's order for longer sums, which TensorFlow does not pin either.

The leaf arithmetic added here, from the documented TensorFlow behaviour:
  * tf.math.reduce_sum / reduce_mean / reduce_max: torch's float32 sum, mean (sum / n) and max; over one or two terms;
  * tf.stack of nested lists of scalars (0-d tensors and Python numbers): a float32 tensor;
  * tf.gather_nd with the [M, 1] indices of tf.where: the rows;
  * a float32 tensor compared with or multiplied by a Python float: the float converted to float32 first, as tf.convert_to_tensor
    does with the tensor's dtype.
NaN: torch's max returns NaN if any element is one and its argmax the first NaN's index, which is numpy's rule; main() checks it
on a probe and the NaN cases (the reference test's zero-area boxes, the -1e5 padding rows) are in the fixture.  Had the stand-in
disagreed they would have been left out, and 'nan_cases' records which it was.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_wbf.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mini_keras   # noqa
from mini_keras import T, ns   # noqa
from make_golden_labels import add_tensor_ops   # noqa

REF = '/root/reference/efficientdet'
F = np.float32


def _leaf(v):
  if torch.is_tensor(v):
    return v.item() if v.dim() == 0 else [_leaf(e) for e in v]
  if isinstance(v, (list, tuple)):
    return [_leaf(e) for e in v]
  return v


def add_wbf_ops(tf):
  def stack(xs, axis=0, name=None):
    xs = list(xs)
    if all(torch.is_tensor(x) and x.dim() >= 1 for x in xs):
      return T(torch.stack(xs, dim=axis))
    rows = []
    for x in xs:      # rows of scalars: every scalar is float32 already, or a Python number
      assert all((torch.is_tensor(e) and e.dtype == torch.float32) or isinstance(e, (int, float)) for e in x), x
      rows.append(torch.stack([torch.as_tensor(e, dtype=torch.float32) for e in x]))
    return T(torch.stack(rows, dim=axis))

  def gather_nd(params, indices):
    assert indices.dim() == 2 and indices.shape[1] == 1
    return T(params)[indices[:, 0]]

  tf.stack, tf.gather_nd = stack, gather_nd
  tf.math = ns('math', reduce_max=lambda x: T(x).max(), reduce_sum=lambda x: T(x).sum(), reduce_mean=lambda x: T(x).mean())


def pad_rows(image_id, n):
  """The dummy rows of nms_np.per_class_nms through generate_detections: zero box, score -1e5, class 0."""
  return [[image_id, 0, 0, 0, 0, -1e5, 0]] * n


def random_case(seed, num_classes):
  """Up to two jittered copies of five disjoint base boxes per class, shuffled; scores partly multiples of 1/8 (ties), partly
  arbitrary float32; a few rows whose class is dropped (-1, 1.5, num_classes)."""
  rng = np.random.default_rng(seed)
  base = np.array([[10, 10, 60, 50], [100, 20, 180, 90], [30, 120, 70, 200], [200, 200, 260, 230], [300, 10, 340, 100]], F)
  rows = []
  for b in base:
    for cls in range(num_classes):
      for _ in range(int(rng.integers(0, 3))):
        box = b + rng.uniform(-6, 6, 4).astype(F)
        score = rng.integers(1, 8) / 8.0 if rng.random() < 0.6 else rng.uniform(0.05, 0.95)
        rows.append([5.0, box[0], box[1], box[2], box[3], score, cls])
  for cls in (-1.0, 1.5, float(num_classes)):
    rows.append([5.0, 10, 10, 60, 50, 0.875, cls])
  rows = np.asarray(rows, F)
  return rows[rng.permutation(len(rows))]


def cases():
  chain = [[3, 0, 0, 10, 10, .9, 1], [3, 2, 0, 12, 10, .6, 1], [3, 4, 0, 14, 10, .7, 1], [3, 3.5, 0, 13.5, 10, .3, 1]]
  out = [
      # wbf_test.py test_ensemble_boxes: boxes without area, so the IoU of d1 and d2 is 0 / 0
      ('ensemble_boxes', [[1, 2, 1, 10, 1, 0.75, 1], [1, 3, 1, 10, 1, 0.75, 1], [1, 3, 1, 10, 1, 1, 2]], 3, 2, True),
      # the second row moves the first cluster's average so that the third no longer matches it; the fourth joins the second
      ('chain_m1', chain, 2, 1, False), ('chain_m2', chain, 2, 2, False), ('chain_m3', chain, 2, 3, False),
      # the reference's padded shape: real rows, then the dummies (two: one class-0 cluster of two members)
      ('padded', [[7, 10, 10, 50, 60, .8, 1], [7, 12, 9, 51, 62, .6, 1], [7, 100, 100, 150, 160, .5, 2]] + pad_rows(7, 2), 4, 2,
       True),
      ('padded_one', [[7, 10, 10, 50, 60, .8, 2]] + pad_rows(7, 1), 3, 2, False),
      # IoU 220 / 400 rounds to 0.55f: not below the threshold, joins; 218 / 400: founds
      ('threshold', [[0, 0, 0, 20, 20, .5, 0], [0, 0, 0, 20, 11, .25, 0], [0, 100, 0, 120, 20, .5, 0],
                     [0, 100, 0, 120, 10.9, .25, 0]], 1, 2, False),
  ]
  for k, (seed, nc, nm) in enumerate([(1, 4, 1), (2, 4, 2), (3, 4, 3), (4, 2, 2), (5, 3, 3)]):
    out.append(('random_%d' % k, random_case(seed, nc), nc, nm, False))
  return out


def main():
  tf = mini_keras.build_tf()
  add_tensor_ops(tf)
  add_wbf_ops(tf)
  mini_keras.install(tf)
  sys.modules.pop('tf2.wbf', None)
  sys.path.insert(0, REF)
  from tf2 import wbf as ref_wbf     # noqa: the reference module
  assert ref_wbf.__file__.startswith(REF), ref_wbf.__file__

  members = []
  inner = ref_wbf.average_detections

  def watched(detections, num_models):
    members.append(len(detections))
    return inner(detections, num_models)
  ref_wbf.average_detections = watched

  probe = np.array([0.3, np.nan, 0.9, np.nan], F)
  t = T(torch.from_numpy(probe))
  nan_ok = bool(torch.isnan(tf.math.reduce_max(t))) and int(tf.argmax(t)) == int(np.argmax(probe)) == 1 \
      and not bool(tf.math.reduce_max(t) < 0.55)
  out = {'nan_cases': np.asarray('included' if nan_ok else 'left out')}
  names = []
  for name, rows, num_classes, num_models, has_nan in cases():
    if has_nan and not nan_ok:
      continue
    rows = np.asarray(rows, F).reshape(-1, 7)
    del members[:]
    res = ref_wbf.ensemble_detections({'num_classes': num_classes}, T(torch.from_numpy(rows.copy())), num_models)
    assert members and max(members) <= 2, (name, max(members))
    res = res.numpy()
    assert res.dtype == F and res.ndim == 2 and res.shape[1] == 7
    out[name + '/detections'], out[name + '/out'] = rows, res
    out[name + '/num_classes'], out[name + '/num_models'] = np.int32(num_classes), np.int32(num_models)
    names.append(name)
    print(name, rows.shape[0], 'rows ->', res.shape[0], 'clusters, largest', max(members))
  out['names'] = np.asarray(names)
  assert len(names) >= 12 and {int(out[n + '/num_models']) for n in names} == {1, 2, 3}
  path = os.path.join(HERE, 'reference_wbf.npz')
  np.savez_compressed(path, **out)
  print(path, len(out), 'arrays,', os.path.getsize(path), 'bytes; NaN cases', out['nan_cases'])


if __name__ == '__main__':
  main()
