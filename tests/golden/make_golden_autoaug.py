"""Generates tests/golden/reference_autoaug.npz by EXECUTING the reference's efficientnetv2/autoaugment.py -- unmodified -- on
the torch-backed `tf` stand-in of make_golden_randaug.py (its leaf operations, its queue behind tf.random_uniform):
distort_image_with_autoaugment(image, 'v0') for every one of the 25 sub-policies under several apply draws and both signs,
and distort_image_with_autoaugment(image, 'test'), on the 24 x 20 and 17 x 31 images of the RandAugment fixture; and the two
policy tables as the reference returns them.

What the fixture pins is the reference's WIRING of AutoAugment: the tables, the per-operation levels through level_to_arg with
translate_const 250 and cutout_const 100 (:658), floor(u + prob) as the apply rule (:562-563), the random negation, the order
of the two operations.  The leaf arithmetic is make_golden_randaug.py's (its docstring says what of it cannot be pinned).

The tf.random_uniform calls of one distort_image_with_autoaugment, in the order the stand-in's eager tf.cond makes them: while
the policy is parsed, one negation draw per signed table entry in table order (:464-468, u >= 0.5 keeps the sign); then the
sub-policy (:573); then, inside the selected sub-policy, one apply draw per position (:562-563).

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_autoaug.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mini_keras   # noqa
import make_golden_randaug as mgr   # noqa
from make_golden_labels import add_tensor_ops   # noqa

SIGNED = mgr.SIGNED
# (apply draw of position 0, of position 1, sign, image): 0.999 applies everything but a probability 0.0, 0.0 only a
# probability 1.0, 0.5 the probabilities >= 0.5; 0.6 and 0.4 meet 0.4 and 0.6 at the float32 sum 1.0
RUNS = ((0.999, 0.999, 1, 'a'), (0.999, 0.999, -1, 'b'), (0.0, 0.0, 1, 'b'), (0.5, 0.5, -1, 'a'), (0.6, 0.4, 1, 'a'),
        (0.0, 0.999, -1, 'b'))


def queue_of(table, sub, apply_u, sign):
  q = [0.75 if sign > 0 else 0.25 for entries in table for (name, _, _) in entries if name in SIGNED]
  q.append((sub + 0.5) / len(table))
  return q + [float(u) for u in apply_u]


def main():
  tf = mini_keras.build_tf()
  add_tensor_ops(tf)
  mgr.add_randaug_ops(tf)
  mini_keras.install(tf)
  sys.modules['tensorflow_addons'].image = mgr.make_image_ops()
  sys.modules.pop('hparams', None)
  sys.path.insert(0, mgr.REF)
  import autoaugment as ref_aa     # noqa: the reference module
  imgs = mgr.images()
  out = {'image/a': imgs['a'], 'image/b': imgs['b']}
  tables = {'v0': ref_aa.policy_v0(), 'test': ref_aa.policy_vtest()}
  for key, table in tables.items():
    out['policy/%s/names' % key] = np.asarray([[name for name, _, _ in sub] for sub in table])
    out['policy/%s/probs' % key] = np.asarray([[prob for _, prob, _ in sub] for sub in table], np.float64)
    out['policy/%s/levels' % key] = np.asarray([[level for _, _, level in sub] for sub in table], np.float64)
  for key, table in tables.items():
    stacks = {'a': [], 'b': []}
    index = []      # (image is b, sub, sign, position in the image's stack)
    draws = []
    for sub in range(len(table)):
      for u0, u1, sign, image in RUNS:
        q = queue_of(table, sub, (u0, u1), sign)
        mgr.QUEUE[:] = q
        res = ref_aa.distort_image_with_autoaugment(mgr.R(torch.from_numpy(imgs[image].copy())), key)
        assert not mgr.QUEUE, mgr.QUEUE
        res = res.numpy()
        assert res.dtype == np.uint8 and res.shape == imgs[image].shape, (res.dtype, res.shape)
        index.append((int(image == 'b'), sub, sign, len(stacks[image])))
        draws.append((u0, u1))
        stacks[image].append(res)
    out['%s/index' % key] = np.asarray(index, np.int32)
    out['%s/apply_u' % key] = np.asarray(draws, np.float32)
    for image in ('a', 'b'):
      out['%s/out/%s' % (key, image)] = np.stack(stacks[image])
    print(key, len(index), 'runs')
  try:
    ref_aa.distort_image_with_autoaugment(mgr.R(torch.from_numpy(imgs['a'].copy())), 'v1')
    raise AssertionError('v1 accepted')
  except ValueError as e:
    out['invalid_name_message'] = np.asarray(str(e))
  path = os.path.join(HERE, 'reference_autoaug.npz')
  np.savez_compressed(path, **out)
  print(path, len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
