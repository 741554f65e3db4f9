"""Inference drivers: ``tf2/infer_lib.py`` ServingDriver :102-252 and KerasDriver :383-421 on the MI355X kernels.

    driver = infer_lib.KerasDriver('/tmp/efficientdet-d0', False, 'efficientdet-d0', batch_size=8)
    boxes, scores, classes, valid_len = driver.serve([np.array(Image.open(f)) for f in files])

The images of a list may have any sizes: a chunk of ``batch_size`` of them goes onto the smallest canvas that holds it
(v2_preprocessing.pad_batch) and every image is processed at its own size and scale (preprocess.preprocess_infer_canvas, as the
reference's ``_preprocess`` runs DetectionInputProcessor per image), so the boxes come back in each image's own pixels.  The
network sees one shape, [batch_size, image_size, 3], whatever the list holds.  Not built: trace files, visualisation, export,
SavedModelDriver and TfliteDriver; each raises ValueError('... is not built')."""
import copy
import time

import numpy as np
import torch

from automl_amd import efficientdet_net
from automl_amd import hparams_config
from automl_amd import postprocess
from automl_amd import preprocess
from automl_amd import util_keras
from automl_amd import v2_preprocessing


def _not_built(what):
  raise ValueError('%s is not built' % what)


def visualize_image(image, boxes, classes, scores, label_map=None, min_score_thresh=0.01, max_boxes_to_draw=1000,
                    line_thickness=2, **kwargs):
  """infer_lib.py:38-76."""
  _not_built('visualize_image')


class ServingDriver(object):
  """A driver for serving single or batch images (infer_lib.py:102-252)."""

  @classmethod
  def create(cls, model_dir, debug, saved_model_dir, *args, **kwargs):
    if saved_model_dir:
      _not_built('serving a saved model (saved_model_dir=%r)' % (saved_model_dir,))
    return KerasDriver(model_dir, debug, *args, **kwargs)

  def __init__(self, model_name, batch_size=1, only_network=False, model_params=None):
    """model_name: such as efficientdet-d0; batch_size: images per network call (None / 0: the whole list at once);
    only_network: the model runs without its pre / post-processing, which the driver does; model_params: overrides of the
    configuration."""
    self.model_name = model_name
    self.batch_size = batch_size
    self.only_network = only_network
    config = hparams_config.get_detection_config(model_name)
    if model_params:      # merged key by key, so {'nms_configs': {'max_output_size': 17}} keeps the other NMS settings
      config.override(model_params, allow_new_keys=True)
    config.override(dict(is_training_bn=False))
    self.params = config.as_dict()
    self.label_map = self.params.get('label_map', None)
    self._decoder = None

  def visualize(self, image, boxes, classes, scores, **kwargs):
    return visualize_image(image, boxes, classes, scores, self.label_map, **kwargs)

  def _benchmark(self, image_arrays, test_func, bm_runs=10, trace_filename=None):
    """Three warm-up runs, then bm_runs timed ones between two device synchronisations (infer_lib.py:181-206)."""
    if trace_filename:
      _not_built('trace_filename')
    for _ in range(3):
      test_func(image_arrays)
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(bm_runs):
      test_func(image_arrays)
    torch.cuda.synchronize()
    end = time.perf_counter()
    inference_time = (end - start) / bm_runs
    fps = (self.batch_size or 1) / inference_time
    print('Per batch inference time: ', inference_time)
    print('FPS: ', fps)
    return {'seconds_per_batch': inference_time, 'fps': fps}

  def predict(self, image_arrays):
    """Feeds the model without extra pre / post-processing."""
    raise NotImplementedError

  def _preprocess(self, image_arrays):
    """(raw, sizes) -> (images [B, H, W, 3] at params['image_size'], image_scale_to_original [B]) (infer_lib.py:219-235)."""
    raw, sizes = image_arrays
    return preprocess.preprocess_infer_canvas(raw, sizes, self.params['image_size'], self.params['mean_rgb'],
                                              self.params['stddev_rgb'], dtype=self._images_dtype())

  def _images_dtype(self):
    return torch.float32

  def _postprocess(self, outputs, scales):
    det_outputs = postprocess.postprocess_global(self.params, outputs[0], outputs[1], scales)
    return det_outputs + tuple(outputs[2:])

  def serve(self, image_arrays):
    raise NotImplementedError

  def export(self, *args, **kwargs):
    _not_built('export')


class SavedModelDriver(ServingDriver):

  def __init__(self, saved_model_dir_or_frozen_graph, *args, **kwargs):
    _not_built('SavedModelDriver')


class TfliteDriver(ServingDriver):

  def __init__(self, tflite_path, *args, **kwargs):
    _not_built('TfliteDriver')


def _is_canvas_pair(image_arrays):
  return (isinstance(image_arrays, tuple) and len(image_arrays) == 2 and hasattr(image_arrays[0], 'shape')
          and len(image_arrays[0].shape) == 4)


def _joined(results):
  """The chunks' (boxes, scores, classes, valid_len) as one."""
  return results[0] if len(results) == 1 else tuple(torch.cat(parts, 0) for parts in zip(*results))


class KerasDriver(ServingDriver):
  """The model of this package behind the serving interface (infer_lib.py:383-421).  ckpt_path None keeps the initial
  variables; dtype, device and seed are EfficientDetNet's."""

  def __init__(self, ckpt_path, debug, model_name, batch_size=1, only_network=False, model_params=None, dtype='bf16',
               device='cuda:0', seed=0):
    super().__init__(model_name, batch_size, only_network, model_params)
    params = copy.deepcopy(self.params)
    config = hparams_config.get_efficientdet_config(self.model_name)
    config.override(params)
    self.model = efficientdet_net.EfficientDetModel(config=config, dtype=dtype, device=device, seed=seed)
    self._dtype = dtype
    if ckpt_path is not None:
      util_keras.restore_ckpt(self.model, ckpt_path, config.moving_average_decay, skip_mismatch=False)
    self.debug = debug

  def _images_dtype(self):
    return torch.bfloat16 if self._dtype in ('bf16', 1) else torch.float32

  def _chunks(self, image_arrays):
    """-> [((raw, sizes), rows)]: canvas batches of batch_size images each, `rows` of them real.  A short last chunk is
    filled with 1 x 1 images, so the network keeps its one shape."""
    if _is_canvas_pair(image_arrays):
      raw, sizes = image_arrays
      raw = torch.from_numpy(raw) if isinstance(raw, np.ndarray) else raw
      sizes = sizes.detach().cpu().numpy() if hasattr(sizes, 'detach') else np.asarray(sizes)
      n = int(raw.shape[0])
      if sizes.shape != (n, 2):
        raise ValueError('sizes must be [batch, 2] for a batch of %d, got %s' % (n, sizes.shape))
      step = self.batch_size or n
      out = []
      for k in range(0, n, step):
        r, s = raw[k:k + step], sizes[k:k + step]
        rows = int(r.shape[0])
        if rows < step:
          r = torch.cat([r, r.new_zeros((step - rows,) + tuple(r.shape[1:]))], 0)
          s = np.concatenate([s, np.ones((step - rows, 2), s.dtype)], 0)
        out.append(((r, s), rows))
      return out
    images = list(image_arrays)
    if not images:
      raise ValueError('serve: no images')
    step = self.batch_size or len(images)
    out = []
    for k in range(0, len(images), step):
      chunk = images[k:k + step]
      rows = len(chunk)
      chunk = chunk + [np.zeros((1, 1, 3), np.uint8)] * (step - rows)
      out.append((v2_preprocessing.pad_batch(chunk), rows))
    return out

  def serve(self, image_arrays):
    """image_arrays: a list of uint8 [h, w, 3] arrays of any sizes (numpy or torch), or a canvas batch (raw uint8 [B, Hc, Wc,
    3], sizes [B, 2]) -> (boxes [B, M, 4] in each image's own pixels, scores [B, M], classes [B, M], valid_len [B]) on the
    device, what EfficientDetModel.__call__ returns.  More than batch_size images are served in chunks."""
    results = []
    for batch, rows in self._chunks(image_arrays):
      scales = None
      if self.only_network:
        batch, scales = self._preprocess(batch)
      outputs = self.predict(batch)
      if self.only_network:
        outputs = self._postprocess(outputs, scales)
      results.append(tuple(o[:rows] for o in outputs))
    return _joined(results)

  def serve_encoded(self, contents, canvas):
    """contents: a list of JPEG files as bytes, decoded on the device onto a canvas = (height, width) that must hold every
    image (jpeg.JpegDecoder, built at the first call for a canvas and kept) -> as serve.  What the decoder refuses raises its
    ValueError."""
    from automl_amd import jpeg
    contents = list(contents)
    if not contents:
      raise ValueError('serve_encoded: no images')
    step = self.batch_size or len(contents)
    key = (step, int(canvas[0]), int(canvas[1]))
    if self._decoder is None or self._decoder[0] != key:
      self._decoder = (key, jpeg.JpegDecoder(*key, device=self.model._device))
    decoder = self._decoder[1]
    results = []
    for k in range(0, len(contents), step):
      chunk = contents[k:k + step]
      rows = len(chunk)
      chunk = chunk + [chunk[-1]] * (step - rows)      # the decoder takes whole batches: the last file again, trimmed below
      raw, sizes = decoder.decode(chunk)
      results.append(tuple(o[:rows] for o in self.serve((raw, sizes))))
    return _joined(results)

  def predict(self, image_arrays):
    if self.only_network:
      cls_outputs, box_outputs = self.model(image_arrays, pre_mode=None, post_mode=None)
      return (cls_outputs, box_outputs)
    return self.model(image_arrays)

  def benchmark(self, image_arrays, bm_runs=10, trace_filename=None):
    return self._benchmark(image_arrays, self.serve, bm_runs, trace_filename)
