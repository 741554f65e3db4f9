"""IoU utils for box regression with IoU losses (efficientdet/iou_utils.py), on the device.

iou_loss is the reference's function by its name and arguments: boxes [..., 4k] of k anchors [ymin, xmin, ymax, xmax] each,
-> 1 - {IoU, GIoU, DIoU, CIoU} per row, summed over the row's anchors, zero for an anchor whose target has no positive height
and width.  One launch of edet_iou_loss whatever the shape; the arithmetic is csrc/iou_impl.h's, the body the training kernels
edet_box_iou_loss / edet_box_iou_loss_eval run after decoding (train_lib.EfficientDetNetTrain.set_iou_loss).

The gradient (return_grad) is the reference's as TensorFlow executes it, not the CIoU paper's: the aspect-ratio term v is a
constant of the backward pass -- its tf.custom_gradient is given the TARGET's height and width as arguments and closes over
the prediction's, and TensorFlow propagates through a custom gradient to its arguments only -- while alpha is differentiated
through iou.  Ties of maximum / minimum go to the first argument as the reference writes them, divide_no_nan has zero
gradient where its denominator is 0, and squared lengths are sums of squares (zero gradient at the zero vector, where
TensorFlow's sqrt gradient is 0 / 0).
"""
import numpy as np
import torch

from automl_amd import _lib
from automl_amd._lib import call, ptr

IOU_TYPES = ('iou', 'giou', 'diou', 'ciou')      # edet_iou_loss's iou_type, by index


def iou_type_id(iou_type):
  """The kernels' number of an IoU type; an unknown one raises the reference's ValueError (iou_utils.py:161-163)."""
  if iou_type not in IOU_TYPES:
    raise ValueError('Unknown loss_type {}, not iou/ciou/diou/giou'.format(iou_type))
  return IOU_TYPES.index(iou_type)


def iou_loss(pred_boxes, target_boxes, iou_type='iou', return_grad=False, device='cuda:0'):
  """pred_boxes, target_boxes: float32 [..., 4k]; device tensors are taken as they are, array-likes are uploaded to `device`.
  -> loss [...]; with return_grad also [..., 4k], the derivative of each row's loss with respect to its pred_boxes."""
  kind = iou_type_id(iou_type)
  if torch.is_tensor(pred_boxes) and pred_boxes.is_cuda:
    device = pred_boxes.device
  elif torch.is_tensor(target_boxes) and target_boxes.is_cuda:
    device = target_boxes.device

  def dev(x):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, np.float32))
    return t.to(device=device, dtype=torch.float32).contiguous()
  pred, target = dev(pred_boxes), dev(target_boxes)
  if pred.shape != target.shape or pred.dim() < 1 or pred.shape[-1] % 4 != 0 or pred.shape[-1] == 0:
    raise ValueError('iou_loss: boxes must be [..., 4k] of one shape, got %s and %s' % (tuple(pred.shape), tuple(target.shape)))
  k = pred.shape[-1] // 4
  rows = pred.numel() // (4 * k)
  loss = torch.empty(pred.shape[:-1], dtype=torch.float32, device=device)
  grad = torch.empty_like(pred) if return_grad else None
  with torch.cuda.device(device):
    call('edet_iou_loss', ptr(pred), ptr(target), rows, k, kind, ptr(loss), ptr(grad) if return_grad else None,
         torch.cuda.current_stream(device).cuda_stream)
  return (loss, grad) if return_grad else loss
