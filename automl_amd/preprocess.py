"""Image preprocessing on the GPU: ``EfficientDetModel._preprocessing(mode='infer')`` (efficientdet_keras.py:920-951) and
the training-time ``DetectionInputProcessor`` of the input pipeline (dataloader.py:144-200) for a batch."""
import ctypes

import numpy as np
import torch

from automl_amd import _lib
from automl_amd import utils


def preprocess_infer(raw_images, image_size, mean_rgb, stddev_rgb, dtype=torch.float32):
  """raw_images [B,H,W,3] uint8 or float32 (any device) -> (images [B,h,w,3] `dtype` on the GPU, image_scales [B]
  float32): normalised, resized with the aspect ratio kept into the top-left corner of image_size, zero padded."""
  if raw_images.dim() != 4 or raw_images.shape[-1] != 3:
    raise ValueError('raw images must be [batch, height, width, 3], got %s' % (tuple(raw_images.shape),))
  if raw_images.dtype not in (torch.uint8, torch.float32):
    raw_images = raw_images.to(torch.float32)
  if dtype not in (torch.float32, torch.bfloat16):
    raise ValueError('dtype must be float32 or bfloat16')
  raw = raw_images.cuda().contiguous()
  oh, ow = utils.parse_image_size(image_size)
  b, h, w, _ = raw.shape
  out = torch.empty((b, oh, ow, 3), dtype=dtype, device=raw.device)
  # per-channel lists, or one scalar for all channels (the efficientdet-lite configurations: 127.0 / 128.0)
  mean = (ctypes.c_float * 3)(*[float(v) for v in np.broadcast_to(np.asarray(mean_rgb, np.float32).reshape(-1), (3,))])
  std = (ctypes.c_float * 3)(*[float(v) for v in np.broadcast_to(np.asarray(stddev_rgb, np.float32).reshape(-1), (3,))])
  scale = ctypes.c_float(0.0)
  _lib.call('edet_preprocess_infer', raw.data_ptr(), 1 if raw.dtype == torch.float32 else 0, b, h, w, oh, ow, mean,
            std, out.data_ptr(), ctypes.byref(scale), _lib.EDET_BF16 if dtype == torch.bfloat16 else _lib.EDET_F32,
            torch.cuda.current_stream().cuda_stream)
  return out, torch.full((b,), scale.value, dtype=torch.float32, device=raw.device)


F = np.float32


def infer_canvas_factors(sizes, batch, canvas_h, canvas_w, image_size):
  """The host half of preprocess_infer_canvas, no device touched: sizes checked (utils.canvas_sizes) -> (sizes int32 [B, 2],
  scaled int32 [B, 2] = (scaled_h, scaled_w), image_scales float32 [B] = 1 / scale), each row output_size_scale_factors of
  that image's own size.  An image whose scaled height or width would be 0 raises a ValueError that names it."""
  sizes = utils.canvas_sizes(sizes, batch, canvas_h, canvas_w)
  oh, ow = utils.parse_image_size(image_size)
  scaled = np.zeros((batch, 2), np.int32)
  scales = np.zeros(batch, np.float32)
  for i in range(batch):
    scale, scaled[i] = output_size_scale_factors((oh, ow), int(sizes[i, 0]), int(sizes[i, 1]))
    if int(scaled[i].min()) < 1:
      raise ValueError('image %d: %d x %d scaled into %d x %d is empty (%d x %d)'
                       % (i, int(sizes[i, 0]), int(sizes[i, 1]), oh, ow, int(scaled[i, 0]), int(scaled[i, 1])))
    scales[i] = F(1.0) / scale
  return sizes, scaled, scales


def preprocess_infer_canvas(raw, sizes, image_size, mean_rgb, stddev_rgb, dtype=torch.float32, mirrored=False):
  """preprocess_infer for a CANVAS batch, what jpeg.JpegDecoder.decode and v2_preprocessing.pad_batch return: raw [B, Hc, Wc,
  3] uint8 or float32, image i the top-left sizes[i] = (height, width) of its slot, processed as that image alone would be
  (infer_lib.py:219-235: the input processor per image) -> (images [B, h, w, 3] `dtype` on the GPU, image_scales [B] float32
  on the GPU), each image at its own scale.  mirrored=True -> (images, mirrored_images, image_scales): the second tensor is
  torch.flip(images, dims=[2]), the batch mirrored along the padded width, written by the same launch.  Sizes are HOST data
  (utils.canvas_sizes) and are checked, with the scaled sizes, before anything touches the device."""
  if raw.dim() != 4 or raw.shape[-1] != 3:
    raise ValueError('raw images must be [batch, height, width, 3], got %s' % (tuple(raw.shape),))
  if dtype not in (torch.float32, torch.bfloat16):
    raise ValueError('dtype must be float32 or bfloat16')
  b, hc, wc = (int(v) for v in raw.shape[:3])
  sizes, scaled, scales = infer_canvas_factors(sizes, b, hc, wc, image_size)
  oh, ow = utils.parse_image_size(image_size)
  if raw.dtype not in (torch.uint8, torch.float32):
    raw = raw.to(torch.float32)
  raw = raw.cuda().contiguous()
  # one upload for all three host arrays: int32 [5 B] = sizes [B, 2], scaled [B, 2], the bits of image_scales [B]
  per = torch.from_numpy(np.concatenate([sizes.reshape(-1), scaled.reshape(-1), scales.view(np.int32)])).to(raw.device)
  out = torch.empty((b, oh, ow, 3), dtype=dtype, device=raw.device)
  flipped = torch.empty_like(out) if mirrored else None
  mean = (ctypes.c_float * 3)(*[float(v) for v in np.broadcast_to(np.asarray(mean_rgb, np.float32).reshape(-1), (3,))])
  std = (ctypes.c_float * 3)(*[float(v) for v in np.broadcast_to(np.asarray(stddev_rgb, np.float32).reshape(-1), (3,))])
  _lib.call('edet_preprocess_infer_canvas', raw.data_ptr(), 1 if raw.dtype == torch.float32 else 0, b, hc, wc, per.data_ptr(),
            per.data_ptr() + 8 * b, oh, ow, mean, std, out.data_ptr(), None if flipped is None else flipped.data_ptr(),
            _lib.EDET_BF16 if dtype == torch.bfloat16 else _lib.EDET_F32, torch.cuda.current_stream().cuda_stream)
  image_scales = per[4 * b:].view(torch.float32)
  return (out, flipped, image_scales) if mirrored else (out, image_scales)


MAX_BOXES = 1024      # PREP_MAX_BOXES of csrc/preprocess.hip


def flip_decisions(u):
  """random_horizontal_flip's decision per uniform draw (object_detection/preprocessor.py:113-199): flipped when > 0.5."""
  return (np.asarray(u, np.float32) > F(0.5)).astype(np.int32)


def training_scale_factors(u, scale_min, scale_max, target, output_size, height, width):
  """set_training_random_scale_factors for one image (dataloader.py:66-111), float32 statement by statement, the int casts
  truncating: u = the three uniform [0, 1) float32 values behind (scale factor, offset y, offset x); target, output_size =
  (height, width) pairs -> (image_scale float32, (scaled_h, scaled_w), (offset_y, offset_x)).  DetectionInputProcessor and
  the detector's raw-batch step (det_input.py) both call this."""
  oh, ow = output_size
  factor = F(scale_min) + u[0] * (F(scale_max) - F(scale_min))        # tf.random.uniform([], min, max)
  scaled_y, scaled_x = int(F(factor * F(target[0]))), int(F(factor * F(target[1])))
  h, w = F(height), F(width)
  scale = min(F(scaled_x) / w, F(scaled_y) / h)
  sh, sw = int(F(h * scale)), int(F(w * scale))
  oy = max(F(0), F(sh - oh)) * u[1]
  ox = max(F(0), F(sw - ow)) * u[2]
  return scale, (sh, sw), (int(F(oy)), int(F(ox)))


def output_size_scale_factors(output_size, height, width):
  """set_scale_factors_to_output_size for one raw size (dataloader.py:113-124), float32 statement by statement ->
  (image_scale float32, (scaled_h, scaled_w)).  DetectionInputProcessor and the detector's evaluation input (det_input.py)
  both call this."""
  h, w = F(height), F(width)
  scale = min(F(output_size[1]) / w, F(output_size[0]) / h)
  return scale, (int(F(h * scale)), int(F(w * scale)))


class DetectionInputProcessor(object):
  """``dataloader.DetectionInputProcessor`` (dataloader.py:144-200, base class :36-141) for a BATCH of equally sized raw
  images, same method names and call order as ``InputReader.process_example`` uses them (:321-336)::

      p = DetectionInputProcessor(raw_images, image_size, boxes, classes, counts)
      p.normalize_image(mean_rgb, stddev_rgb)
      p.random_horizontal_flip()                                   # training only
      p.set_training_random_scale_factors(jitter_min, jitter_max, target_size)   # or set_scale_factors_to_output_size()
      images = p.resize_and_crop_image()
      boxes, classes, counts = p.resize_and_crop_boxes()

  The setters only record per-image decisions (host, float32 arithmetic statement by statement as the reference's
  TensorFlow expressions: the int casts truncate); all pixel and box work is ONE call of edet_preprocess_train when the
  first result is asked for.  The random draws come from `rng` (numpy Generator) or are handed in (`draws=`), which is
  how the tests feed the values the reference's fixtures were made with -- TensorFlow's RNG stream cannot be
  reproduced.  boxes [B, max_boxes, 4] normalised (ymin, xmin, ymax, xmax), classes [B, max_boxes] (or [.., 1]), counts
  [B] valid rows per image (None: all rows).

  sizes [B, 2] makes `images` a CANVAS batch, what jpeg.JpegDecoder.decode returns: image i is the top-left sizes[i] =
  (height, width) of its slot and is processed as that image alone would be (edet_preprocess_train_canvas) -- the scale
  factors come from its own size, so image_scale and image_scale_to_original differ per image.  Sizes are host data
  (utils.canvas_sizes: a device tensor is copied to the host, which waits for the device) and are checked here, before any
  draw."""

  def __init__(self, images, output_size, boxes=None, classes=None, counts=None, rng=None, dtype=torch.float32, sizes=None):
    if images.dim() != 4 or images.shape[-1] != 3:
      raise ValueError('raw images must be [batch, height, width, 3], got %s' % (tuple(images.shape),))
    if dtype not in (torch.float32, torch.bfloat16):
      raise ValueError('dtype must be float32 or bfloat16')
    if images.dtype not in (torch.uint8, torch.float32):
      images = images.to(torch.float32)
    self._batch, self._height, self._width = (int(v) for v in images.shape[:3])
    self._sizes = None if sizes is None else utils.canvas_sizes(sizes, self._batch, self._height, self._width)
    self._raw = images.cuda().contiguous()
    self._output_size = utils.parse_image_size(output_size)
    self._dtype = dtype
    self._rng = rng if rng is not None else np.random.default_rng()
    self._mean = self._std = None
    b = self._batch
    self._flip = np.zeros(b, np.int32)
    self._image_scale = np.ones(b, np.float32)
    self._scaled = np.zeros((b, 2), np.int32)
    self._offset = np.zeros((b, 2), np.int32)
    self._scales_set = False
    self._boxes = self._classes = self._counts = None
    if boxes is not None:
      self._boxes = torch.as_tensor(boxes, dtype=torch.float32).reshape(b, -1, 4).cuda().contiguous()
      m = int(self._boxes.shape[1])
      if m > MAX_BOXES:
        raise ValueError('at most %d boxes per image (edet_preprocess_train keeps them in LDS), got %d' % (MAX_BOXES, m))
      if classes is None:      # the reference's constructor allows it (dataloader.py:146): boxes without labels
        classes = torch.zeros(b, m, dtype=torch.float32)
      self._classes = torch.as_tensor(classes, dtype=torch.float32).reshape(b, m).cuda().contiguous()
      self._counts = (torch.full((b,), m, dtype=torch.int32) if counts is None
                      else torch.as_tensor(counts).to(torch.int32)).cuda().contiguous()
    self._result = None

  def normalize_image(self, mean_rgb, stddev_rgb):
    """Records (image - mean) / stddev, applied to the taps of the resize as the reference normalises first (:58-64)."""
    self._mean = np.broadcast_to(np.asarray(mean_rgb, np.float32).reshape(-1), (3,)).copy()
    self._std = np.broadcast_to(np.asarray(stddev_rgb, np.float32).reshape(-1), (3,)).copy()

  def _size(self, i):
    """(height, width) of image i: its own on a canvas batch."""
    return (self._height, self._width) if self._sizes is None else (int(self._sizes[i, 0]), int(self._sizes[i, 1]))

  def _uniform(self, draws, count):
    if draws is None:
      return self._rng.random((self._batch, count)).astype(np.float32)
    d = np.asarray(draws, np.float32).reshape(self._batch, count)
    return d

  def random_horizontal_flip(self, draws=None):
    """preprocessor.random_horizontal_flip (object_detection/preprocessor.py:113-199): one uniform draw per image,
    flipped when it is > 0.5; image and boxes together."""
    self._flip = flip_decisions(self._uniform(draws, 1)[:, 0])
    self._result = None

  def set_training_random_scale_factors(self, scale_min, scale_max, target_size=None, draws=None):
    """dataloader.py:66-111; draws [B, 3] = the uniform [0, 1) values behind (scale factor, offset y, offset x)."""
    target = utils.parse_image_size(target_size) if target_size else self._output_size
    u = self._uniform(draws, 3)
    for i in range(self._batch):
      self._image_scale[i], self._scaled[i], self._offset[i] = training_scale_factors(
          u[i], scale_min, scale_max, target, self._output_size, *self._size(i))
    self._scales_set = True
    self._result = None

  def set_scale_factors_to_output_size(self):
    """dataloader.py:113-124 (evaluation: the whole image into the top-left corner, no offset)."""
    for i in range(self._batch):
      self._image_scale[i], self._scaled[i] = output_size_scale_factors(self._output_size, *self._size(i))
    self._offset[:] = 0
    self._scales_set = True
    self._result = None

  def _run(self):
    if self._result is not None:
      return self._result
    if self._mean is None or not self._scales_set:
      raise RuntimeError('call normalize_image and one of the set_*scale_factors methods first')
    if int(self._scaled.min()) < 1:
      raise ValueError('the scaled image is empty')
    b = self._batch
    oh, ow = self._output_size
    per = np.concatenate([self._flip[:, None], self._scaled, self._offset], 1).astype(np.int32)
    per_dev = torch.from_numpy(np.ascontiguousarray(per)).cuda()
    out = torch.empty((b, oh, ow, 3), dtype=self._dtype, device=self._raw.device)
    mean, std = (ctypes.c_float * 3)(*[float(v) for v in self._mean]), (ctypes.c_float * 3)(*[float(v) for v in self._std])
    m = 0 if self._boxes is None else int(self._boxes.shape[1])
    bo = co = cnt = None
    if m:
      bo = torch.empty_like(self._boxes)
      co = torch.empty_like(self._classes)
      cnt = torch.empty_like(self._counts)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    sizes_dev = None if self._sizes is None else torch.from_numpy(self._sizes).to(self._raw.device)
    tail = (oh, ow, mean, std, per_dev.data_ptr(), out.data_ptr(), p(self._boxes), p(self._classes), p(self._counts), m, p(bo),
            p(co), p(cnt), _lib.EDET_BF16 if self._dtype == torch.bfloat16 else _lib.EDET_F32,
            torch.cuda.current_stream().cuda_stream)
    head = (self._raw.data_ptr(), 1 if self._raw.dtype == torch.float32 else 0, b, self._height, self._width)
    if sizes_dev is None:
      _lib.call('edet_preprocess_train', *head, *tail)
    else:
      _lib.call('edet_preprocess_train_canvas', *head, sizes_dev.data_ptr(), *tail)
    self._keep_alive = (per_dev, sizes_dev)
    self._result = (out, bo, co, cnt)
    return self._result

  def resize_and_crop_image(self):
    """dataloader.py:126-139 -> [B, H, W, 3] on the GPU."""
    return self._run()[0]

  def resize_and_crop_boxes(self):
    """dataloader.py:165-189 -> (boxes [B, max_boxes, 4] in pixels of the output image, classes [B, max_boxes],
    counts [B]): the boxes of non-zero area in their original order, padded with -1."""
    if self._boxes is None:
      raise ValueError('no boxes were given')
    _, bo, co, cnt = self._run()
    return bo, co, cnt

  @property
  def image_scale(self):
    """Scale from the original image to the scaled image, [B] float32 (dataloader.py:191-194)."""
    return torch.from_numpy(self._image_scale.copy())

  @property
  def image_scale_to_original(self):
    """dataloader.py:196-199."""
    return torch.from_numpy((F(1.0) / self._image_scale).astype(np.float32))

  @property
  def offset_x(self):
    return torch.from_numpy(self._offset[:, 1].copy())

  @property
  def offset_y(self):
    return torch.from_numpy(self._offset[:, 0].copy())

  @property
  def scaled_size(self):
    """[B, 2] (scaled_height, scaled_width)."""
    return torch.from_numpy(self._scaled.copy())
