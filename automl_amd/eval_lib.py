"""The detector's evaluation loop on MI355X (mirror of efficientdet/tf2/eval.py:48-125).

``evaluate(model, batches)`` runs a data set through the evaluation input stage, the network, the detections and the COCO
evaluator -- every stage on the device -- and returns the reference's metric dictionary.  Per batch (eval.py:80-90):

  1. ``det_input.DetectionEvalInput``  normalise, resize into the top-left corner, boxes, anchor labels, ground truth
  2. ``model(images, training=False)``
  3. ``postprocess.generate_detections(config, cls, box, labels['image_scales'], labels['source_ids'])``
  4. ``postprocess.transform_detections``
  5. ``evaluator.update_state(labels['groundtruth_data'], detections)``

with ``nms_configs.max_nms_inputs = anchors.MAX_DETECTION_POINTS`` on a copy of the model's config (eval.py:52).  A smaller
last batch is evaluated, not dropped (``drop_remainder = False``, :53): it gets an input stage and an engine of its own shape.
Nothing here waits for the device; the one copy to the host per batch is ``update_state``'s.

Not built: ``testdev_dir``, data-parallel evaluation and merging evaluator states across devices, evaluating the EMA shadows of
a training model in place (``get_ema_weights`` into a second ``EfficientDetNet`` is the way), segmentation.
"""
import copy

import torch

from automl_amd import anchors
from automl_amd import coco_metric
from automl_amd import det_input
from automl_amd import efficientdet_net
from automl_amd import postprocess
from automl_amd import utils


def eval_config(config):
  """A copy of `config` as tf2/eval.py sets it up (:52-53)."""
  config = copy.deepcopy(config)
  config.nms_configs.max_nms_inputs = anchors.MAX_DETECTION_POINTS
  config.drop_remainder = False
  return config


def evaluate(model, batches, evaluator=None, eval_samples=None, max_batches=None):
  """model: an EfficientDetNet, or an EfficientDetNetTrain -- then its CURRENT variables are evaluated, not the EMA shadows.
  batches: an iterable of (raw_images uint8 [B, H, W, 3], boxes [B, M, 4] normalised, classes [B, M], counts [B], is_crowds
  [B, M], areas [B, M], source_ids [B]); the batch size may change, a smaller last batch is evaluated.  raw_images may be the
  pair (raw, sizes) of a canvas batch, as jpeg.JpegDecoder.decode returns it (sizes [B, 2] host data): every image is then
  evaluated at its own size, and one input stage serves every batch on the same canvas.  evaluator: default
  EvaluationMetric(filename=config.val_json_file, label_map=config.label_map); it is NOT reset here.  eval_samples: stop
  after ceil(eval_samples / batch) batches, the batch size being the first batch's (eval.py:104-105); max_batches: a plain
  bound on the batches (COCOCallback's take(count)).
  -> {metric name: value} over evaluator.metric_names, plus 'AP_/<name>' per label_map entry (eval.py:116-124)."""
  config = eval_config(model.config)
  params = config.as_dict()
  if evaluator is None:
    evaluator = coco_metric.EvaluationMetric(filename=getattr(config, 'val_json_file', None),
                                             label_map=getattr(config, 'label_map', None))
  h, w = utils.parse_image_size(config.image_size)
  stages = {}
  limit = max_batches
  for n, batch in enumerate(batches):
    raw, boxes, classes, counts, is_crowds, areas, source_ids = batch
    raw, sizes = det_input.split_raw(raw)
    raw, boxes = torch.as_tensor(raw), torch.as_tensor(boxes)
    b, m = int(raw.shape[0]), int(boxes.shape[1])
    if n == 0 and eval_samples:
      take = (int(eval_samples) + b - 1) // b
      limit = take if limit is None else min(limit, take)
    if limit is not None and n >= limit:
      break
    eng = model._ensure_engine(b, h, w)
    key = (b, int(raw.shape[1]), int(raw.shape[2]), m)
    inp = stages.get(key)
    if inp is None:
      inp = stages[key] = det_input.DetectionEvalInput(config, model.anchors((h, w)), b, key[1], key[2], m, dtype=eng.tdtype,
                                                       device=eng.device)
    images, labels = inp.run(raw, boxes, classes, counts, is_crowds, areas, source_ids, *inp.own_buffers(), sizes=sizes)
    cls_outputs, box_outputs = efficientdet_net.EfficientDetNet.__call__(model, images, False)      # no pre / post-processing
    if hasattr(model, 'train_step'):
      eng._cast_version = -1      # a training step that follows (perhaps the captured one) makes its compute copies again
    detections = postprocess.generate_detections(params, cls_outputs, box_outputs, labels['image_scales'], labels['source_ids'])
    evaluator.update_state(labels['groundtruth_data'], postprocess.transform_detections(detections))
  metrics = evaluator.result()
  metric_dict = {}
  for i, name in enumerate(evaluator.metric_names):
    metric_dict[name] = metrics[i]
  label_map = evaluator.label_map
  if label_map:
    for i, cid in enumerate(sorted(label_map.keys())):
      metric_dict['AP_/%s' % label_map[cid]] = metrics[i + len(evaluator.metric_names)]
  return metric_dict
