"""Generates tests/golden/reference_iou_loss.npz by EXECUTING the reference's efficientdet/iou_utils.py and
tf2/train_lib.BoxIouLoss.call (with tf2/anchors.py's Anchors and decode_box_outputs) -- all unmodified -- on the torch-backed
`tf` of tests/golden/mini_keras.py plus make_golden_labels.add_tensor_ops, extended below by what these modules touch.

What the stand-in decides about the gradient, and why:
  * maximum(x, y) = where(x >= y, x, y), minimum(x, y) = where(x <= y, x, y): the tie goes to the first argument;
  * divide_no_nan has zero gradient where its denominator is 0;
  * custom_gradient evaluates the wrapped function WITHOUT a tape and hands the gradient function's result to the function's
    ARGUMENTS only.  _get_v is given the target's height and width and closes over the prediction's, so v carries no gradient
    to the prediction.  This is how TensorFlow treats a custom gradient, eagerly and in a graph; no TensorFlow run has
    confirmed it here (none can be made).
Cases are drawn (tests/iou_loss_ref.draw_case) until no positive anchor lies within 1e-3 of a kink of the metric, so none of
the recorded values depends on a tie rule, and at most half of the draws may be rejected (asserted).

Recorded per case: the raw box outputs and targets, the anchors, BoxIouLoss.call's result, the per-anchor losses and the decoded
masked boxes iou_utils.iou_loss was handed (watched while the reference runs), and the autograd gradients of the reduced loss
and of the plain sum of the per-anchor losses with respect to the raw outputs.  Only data is written.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_iou_loss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mini_keras   # noqa
from mini_keras import T, ns   # noqa
from make_golden_labels import add_tensor_ops   # noqa
import iou_loss_ref   # noqa

REF = '/root/reference/efficientdet'
F = np.float32
IMAGE_SIZE, MIN_LEVEL, MAX_LEVEL, NUM_SCALES, ASPECT_RATIOS, ANCHOR_SCALE = 32, 3, 5, 3, [1.0, 2.0, 0.5], 4.0
NUM_POSITIVES = 7.0


def add_iou_ops(tf):
  def tt(x, like=None):
    if torch.is_tensor(x):
      return x
    return torch.as_tensor(x, dtype=like.dtype if torch.is_tensor(like) else torch.float32)

  def divide_no_nan(x, y):
    x, y = tt(x, y), tt(y, x)
    ok = y != 0
    return torch.where(ok, x / torch.where(ok, y, torch.ones_like(y)), torch.zeros_like(x * y))

  def maximum(a, b):
    a, b = tt(a, b), tt(b, a)
    return torch.where(a >= b, a, b)

  def minimum(a, b):
    a, b = tt(a, b), tt(b, a)
    return torch.where(a <= b, a, b)

  def custom_gradient(f):
    def wrapped(*args):
      class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *a):      # (no tape inside forward: what f closes over gets no gradient)
          out, grad_fn = f(*a)
          ctx.grad_fn = grad_fn
          return out

        @staticmethod
        def backward(ctx, dv):
          return tuple(ctx.grad_fn(dv))
      return Fn.apply(*[tt(a) for a in args])
    return wrapped

  def convert_to_tensor(x, dtype=None):
    if torch.is_tensor(x):
      return x.to(dtype) if isinstance(dtype, torch.dtype) else x
    return T(torch.as_tensor(np.asarray(x), dtype=dtype if isinstance(dtype, torch.dtype) else None))

  tf.maximum, tf.minimum = maximum, minimum
  tf.atan = torch.atan
  tf.custom_gradient = custom_gradient
  tf.convert_to_tensor = convert_to_tensor
  tf.squeeze = lambda x, axis=None: x.squeeze() if axis is None else x.squeeze(axis)
  tf.unstack = lambda x, num=None, axis=0: list(torch.unbind(x, dim=axis))
  tf.math = ns('math', divide_no_nan=divide_no_nan, logical_and=torch.logical_and, exp=torch.exp)
  tf.linalg = ns('linalg', norm=lambda x, axis=None: torch.linalg.vector_norm(x, dim=axis))
  tf.executing_eagerly_outside_functions = lambda: True      # tf.compat.v1 is this module


def main():
  tf = mini_keras.build_tf()
  add_tensor_ops(tf)
  add_iou_ops(tf)
  mini_keras.install(tf)
  for m in ('iou_utils', 'tf2.train_lib', 'tf2.anchors'):
    sys.modules.pop(m, None)
  sys.path.insert(0, REF)
  import iou_utils as ref_iou     # noqa: the reference modules
  from tf2 import train_lib as ref     # noqa
  assert ref_iou.__file__.startswith(REF) and ref.__file__.startswith(REF), (ref_iou.__file__, ref.__file__)

  # ---- the reference's own known answers (iou_utils_test.py:32-76), first: the stand-in is trusted only if it gives them
  pb = torch.tensor([[4, 3, 7, 5], [5, 6, 10, 7]], dtype=torch.float32)
  tb = torch.tensor([[3, 4, 6, 8], [14, 14, 15, 15]], dtype=torch.float32)
  known = {'iou': [0.875, 1.0], 'ciou': [0.99931306, 1.6415315], 'diou': [0.9969512, 1.6243094], 'giou': [1.075, 1.933333]}
  for kind, want in known.items():
    np.testing.assert_allclose(ref_iou.iou_loss(pb, tb, kind).numpy(), want, rtol=1e-6, atol=1e-6)
  p, t = pb.clone().requires_grad_(True), tb.clone().requires_grad_(True)
  gp, gt = torch.autograd.grad(ref_iou.iou_loss(p, t, 'ciou').sum(), [p, t])
  np.testing.assert_allclose(float(gp.sum()), -0.14763935, atol=1e-6)
  np.testing.assert_allclose(float(gt.sum()), 0.1476393, atol=1e-6)
  out = {'known/ciou_grad_pred': gp.numpy().astype(F), 'known/ciou_grad_target': gt.numpy().astype(F)}
  print('ciou gradient of the known pair: pred', gp.numpy().tolist(), 'target sum', float(gt.sum()))

  watched = {}
  inner = ref_iou.iou_loss

  def watch(pred_boxes, target_boxes, iou_type='iou'):
    res = inner(pred_boxes, target_boxes, iou_type)
    watched.update(pred=pred_boxes, target=target_boxes, loss=res)
    return res
  ref_iou.iou_loss = watch

  draws = rejected = 0
  for k, kind in enumerate(iou_loss_ref.IOU_TYPES):
    layer = ref.BoxIouLoss(kind, MIN_LEVEL, MAX_LEVEL, NUM_SCALES, ASPECT_RATIOS, ANCHOR_SCALE, IMAGE_SIZE, reduction='none')
    anchors = layer.input_anchors.boxes.numpy().astype(F)
    x, tg, rej = iou_loss_ref.draw_case(100 + k, anchors)
    draws, rejected = draws + rej + 1, rejected + rej
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    loss = layer([torch.tensor(NUM_POSITIVES), T(torch.from_numpy(tg.copy()))], xt)
    grad, = torch.autograd.grad(loss, xt, retain_graph=True)
    grad_sum, = torch.autograd.grad(watched['loss'].sum(), xt)
    pos = (tg != 0).any(-1)
    assert watched['loss'].shape == (x.shape[0],) and 0.15 < pos.mean() < 0.35, (watched['loss'].shape, pos.mean())
    assert ((tg != 0).sum(-1) == 3).sum() == 1      # the row with a single zero target component
    name = 'case_%s/' % kind
    out.update({name + 'box_outputs': x, name + 'box_targets': tg, name + 'anchors': anchors,
                name + 'num_positives': F(NUM_POSITIVES), name + 'loss': F(loss.item()),
                name + 'loss_per_anchor': watched['loss'].detach().numpy().astype(F),
                name + 'decoded_pred': watched['pred'].detach().numpy().astype(F),
                name + 'decoded_target': watched['target'].detach().numpy().astype(F),
                name + 'grad': grad.numpy().astype(F), name + 'grad_sum': grad_sum.numpy().astype(F)})
    print(kind, x.shape[0], 'anchors,', int(pos.sum()), 'positive, loss', float(loss), 'draws rejected', rej,
          'margin %.2e' % iou_loss_ref.kink_margin(x, tg, anchors))
  assert 2 * rejected <= draws, (rejected, draws)
  out['draws'], out['rejected'] = np.int32(draws), np.int32(rejected)
  path = os.path.join(HERE, 'reference_iou_loss.npz')
  np.savez_compressed(path, **out)
  print(path, len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
