"""numpy restatement of the evaluation branch of the detector's input (efficientdet/dataloader.py:331-353, :389) for ONE image:
what automl_amd/csrc/det_eval.hip (edet_pack_groundtruth) and det_input.DetectionEvalInput compute, float32 operation by
operation.  tests/golden/reference_det_eval.npz holds what the executed reference gives for the same inputs."""
import numpy as np

F = np.float32


def scale_factors_to_output_size(height, width, output_size):
  """set_scale_factors_to_output_size (:115-127) -> (image_scale float32, scaled_height, scaled_width)."""
  h, w = F(height), F(width)
  scale = min(F(output_size[1]) / w, F(output_size[0]) / h)
  return F(scale), int(F(h * scale)), int(F(w * scale))


def resize_and_crop_boxes(boxes, classes, scaled_h, scaled_w, output_size):
  """:168-191 with a zero crop offset: pixels of the scaled image, clipped to [0, size - 1], the boxes without area removed
  WITH their classes."""
  b = np.asarray(boxes, F).reshape(-1, 4) * np.asarray([scaled_h, scaled_w, scaled_h, scaled_w], F)
  b = b - np.zeros(4, F)
  hi = np.asarray([output_size[0] - 1, output_size[1] - 1, output_size[0] - 1, output_size[1] - 1], F)
  b = np.clip(b, F(0), hi)
  keep = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) != 0
  return b[keep], np.asarray(classes, F).reshape(-1)[keep]


def pad_to_fixed_size(data, pad_value, rows, columns):
  """:212-233 (rows <= max_instances_per_image: the reference asserts a strict less)."""
  data = np.asarray(data, F).reshape(-1, columns)
  assert data.shape[0] <= rows, 'ERROR: please increase config.max_instances_per_image'
  return np.concatenate([data, F(pad_value) * np.ones((rows - data.shape[0], columns), F)], 0)


def source_id_number(source_id):
  """:340-342."""
  return F(float('-1' if source_id == '' else source_id))


def pack_groundtruth(kept_boxes, kept_classes, is_crowds, areas, image_scale_to_original, max_instances):
  """:344-353 and :389 -> [max_instances, 7] rows [y1, x1, y2, x2, is_crowd, area, class].  kept_boxes / kept_classes are
  resize_and_crop_boxes' (filtered), is_crowds / areas the decoder's (NOT filtered): after a dropped box, columns 4-5 of a
  row belong to another annotation than columns 0-3 and 6 -- as the reference is written."""
  boxes = np.asarray(kept_boxes, F).reshape(-1, 4) * F(image_scale_to_original)
  return np.concatenate([pad_to_fixed_size(boxes, -1, max_instances, 4),
                         pad_to_fixed_size(np.asarray(is_crowds).astype(F), 0, max_instances, 1),
                         pad_to_fixed_size(areas, -1, max_instances, 1),
                         pad_to_fixed_size(kept_classes, -1, max_instances, 1)], 1)


def eval_groundtruth(height, width, output_size, boxes, classes, is_crowds, areas, source_id, max_instances):
  """The ground-truth part of dataset_parser(is_training=False) for one image of height x width ->
  (groundtruth_data [max_instances, 7], image_scale_to_original float32, source id float32)."""
  scale, sh, sw = scale_factors_to_output_size(height, width, output_size)
  kb, kc = resize_and_crop_boxes(boxes, classes, sh, sw, output_size)
  to_original = F(1.0) / scale
  return pack_groundtruth(kb, kc, is_crowds, areas, to_original, max_instances), to_original, source_id_number(source_id)
