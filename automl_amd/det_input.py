"""The detector's training input on the device, from a raw batch to the train step's static buffers.

Restates the training branch of ``InputReader.dataset_parser`` plus ``process_example`` (dataloader.py:301-338, :369-382)
for a batch of decoded images with padded boxes -- equally sized (a dense batch), or of their own sizes in the top-left
corners of a common canvas with ``sizes=`` (what ``jpeg.JpegDecoder.decode`` returns; see "A canvas batch" below):

  1. ``gridmask.gridmask`` if ``config.grid_mask`` (:308-310)                                  edet_gridmask
  1a. ``distort_image_with_autoaugment`` / ``..._randaugment`` (:312-319) if the ``autoaugment`` switch is on
                                                     edet_autoaug_boxes, edet_randaug_stats, edet_autoaug_contrast_lut,
                                                     edet_randaug_apply per layer (det_autoaugment.py)
  2. ``normalize_image``, 3. ``random_horizontal_flip`` if ``input_rand_hflip``,
  4. ``set_training_random_scale_factors(jitter_min, jitter_max, target_size)``,
  5. ``resize_and_crop_image``, 6. ``resize_and_crop_boxes`` (:321-334)                        edet_preprocess_train
  7. ``anchor_labeler.label_anchors`` (:337-338)                                               edet_label_anchors
  8. ``mean_num_positives``: the batch mean of num_positives tiled to [B, 1] (:371-375)

The launches write into destinations the CALLER supplies -- the captured step's ``input_buffers()`` -- so nothing is
staged; the labelling workspace, the per-image argument arrays, the GridMask scratch image and AutoAugment's scratch images,
boxes, tables and argument buffer are allocated once, here.  The
draws are made on the host (``draw``), turned into the kernels' per-image rows by the same float32 arithmetic as
``preprocess.DetectionInputProcessor`` (``preprocess.training_scale_factors`` is shared) and copied from pinned memory.

A canvas batch: ``run(..., sizes=)`` / ``draw(rng, sizes=)`` with sizes [B, 2] = (height, width) per image, host data.  The
stage is built for the CANVAS (``height``, ``width``) and serves every batch on it: the scratch images stay canvas-sized, a
device ``sizes`` buffer is allocated once and filled by one more small pinned copy per step, and every launch is the
``*_canvas`` sibling, which treats image ``i`` as the dense path treats that image alone, bit for bit -- the reference
processes each image at its own size (dataloader.py:301-353).  The kernels write the scratch images inside the images'
rectangles only; nothing reads the rest.  The draw stream with sizes: flip and scale as without; GridMask's ``d`` comes
from ``rng.integers(lo, hi + 1)`` over the per-image bounds, and everything after it as without -- a stream of its own, not
promised equal to the dense one.

``skip_crowd_during_training`` (:303-306) is the caller's filtering of ``boxes`` / ``counts``: crowd boxes are left out of the
padded rows before they get here.

The box-aware AutoAugment / RandAugment of ``aug/autoaugment.py`` is reached through the constructor's ``autoaugment`` switch
(``EfficientDetNetTrain.set_autoaugment``): ``'randaug'`` (the data loader's num_layers=1, magnitude=15, :315-316), ``'v2'``,
``'v3'`` or ``'test'``.  ``'v0'``, ``'v1'`` and the ``*_Only_BBoxes`` operations they need are not built.  The
``config.autoaugment_policy`` key itself is still refused by ``train_step_raw``.  What is not pinned against TensorFlow
(TFA's rounding rule, float32 sine and cosine, the random streams, ``reduce_mean``'s order beyond a grey sum of 2^24) is
listed in det_autoaugment.py.
"""
import collections
import ctypes

import numpy as np
import torch

from automl_amd import _lib
from automl_amd import det_autoaugment
from automl_amd import gridmask as gridmask_lib
from automl_amd import labeling
from automl_amd import preprocess
from automl_amd import utils
from automl_amd._lib import call, ptr

Draws = collections.namedtuple('Draws', ['flip', 'scale', 'gridmask', 'autoaug'], defaults=(None,))
RANDAUG_NUM_LAYERS, RANDAUG_MAGNITUDE = 1, 15      # dataloader.py:315-316


def input_rng(seed):
  """The generator behind the input draws of a model built with `seed`."""
  return np.random.Generator(np.random.PCG64([int(seed), 0x64657469]))


def mean_num_positives(num_positives):
  """dataloader.py:371-375: reduce_mean over the batch, tiled to [B, 1].  num_positives are integer-valued floats, so their
  sum is exact in any order and the mean is one rounded division (by a tensor: torch turns a division by a host scalar
  into a product with its reciprocal, a second rounding)."""
  b = int(num_positives.shape[0])
  count = torch.full((), float(b), dtype=num_positives.dtype, device=num_positives.device)
  return torch.div(num_positives.sum(), count).reshape(1, 1).expand(b, 1)


class DetectionInput(object):
  """The input launches of one (batch, raw size, box rows) shape for `config` on `device`.  height, width: the size of every
  image of a dense batch, or the canvas of the batches that come with `sizes`."""

  TRAINING = True      # DetectionEvalInput: no GridMask, no AutoAugment, no draws

  def __init__(self, config, anchors, batch, height, width, max_boxes, dtype=torch.float32, device='cuda:0',
               autoaugment=None):
    if dtype not in (torch.float32, torch.bfloat16):
      raise ValueError('dtype must be float32 or bfloat16')
    if not 1 <= int(max_boxes) <= preprocess.MAX_BOXES:
      raise ValueError('between 1 and %d box rows per image (edet_preprocess_train keeps them in LDS), got %d'
                       % (preprocess.MAX_BOXES, max_boxes))
    self.config = config
    self.batch, self.height, self.width, self.max_boxes = int(batch), int(height), int(width), int(max_boxes)
    self.dtype, self.device = dtype, torch.device(device)
    self.output_size = utils.parse_image_size(config.image_size)
    target = getattr(config, 'target_size', None)
    self.target_size = utils.parse_image_size(target) if target else self.output_size
    self.grid_mask = self.TRAINING and bool(getattr(config, 'grid_mask', None))
    if self.grid_mask:
      gridmask_lib.block_range(self.height, self.width)      # a raw size the reference could not mask: raises
    self.autoaugment = autoaugment      # None, 'randaug', 'v2', 'v3' or 'test' (det_autoaugment.available_policy)
    self._aa_policy = det_autoaugment.available_policy(autoaugment) if autoaugment is not None else None
    self.labeler = labeling.AnchorLabeler(anchors, config.num_classes, device=device)
    self.levels = list(self.labeler._levels)
    f = np.float32
    self._mean = (ctypes.c_float * 3)(*[float(v) for v in np.broadcast_to(np.asarray(config.mean_rgb, f).reshape(-1), (3,))])
    self._std = (ctypes.c_float * 3)(*[float(v) for v in np.broadcast_to(np.asarray(config.stddev_rgb, f).reshape(-1), (3,))])
    b, m, dev = self.batch, self.max_boxes, self.device
    # allocated once: argument rows, the masked image, the boxes between the two kernels, the labelling workspace
    self.prep_rows = torch.zeros((b, 5), dtype=torch.int32, device=dev)              # edet_prep_image_t
    self.sizes_dev = torch.zeros((b, 2), dtype=torch.int32, device=dev)              # a canvas batch's (height, width) rows
    self.mask_rows = self.masked = None
    if self.grid_mask:
      self.mask_rows = torch.zeros((b, gridmask_lib.ARGS_BYTES), dtype=torch.uint8, device=dev)      # edet_gridmask_image_t
      self.masked = torch.empty((b, self.height, self.width, 3), dtype=torch.uint8, device=dev)
    self.aa_layers = 0
    if self._aa_policy is not None:
      self.aa_layers = det_autoaugment.num_layers_of(self._aa_policy, RANDAUG_NUM_LAYERS)
      self._aa_layout, nbytes = det_autoaugment.args_layout(self.aa_layers, b)
      self.aa_rows = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)      # one step's arguments, one copy
      self.aa_args = det_autoaugment.unpack_args(self.aa_rows, self._aa_layout)
      shape = (b, self.height, self.width, 3)
      self.aa_images = torch.empty(shape, dtype=torch.uint8, device=dev)
      self.aa_scratch = [torch.empty(shape, dtype=torch.uint8, device=dev) for _ in range(min(self.aa_layers - 1, 2))]
      self.aa_boxes = torch.empty((b, m, 4), dtype=torch.float32, device=dev)
      self.aa_luts = torch.zeros((b, 3, 256), dtype=torch.uint8, device=dev)
    self.boxes = torch.empty((b, m, 4), dtype=torch.float32, device=dev)
    self.classes = torch.empty((b, m), dtype=torch.float32, device=dev)
    self.labels = torch.empty((b, m), dtype=torch.int32, device=dev)
    self.counts = torch.empty((b,), dtype=torch.int32, device=dev)
    self.num_positives = torch.empty((b,), dtype=torch.float32, device=dev)
    need = ctypes.c_size_t(0)
    call('edet_label_anchors_workspace_bytes', b, int(self.labeler._boxes.shape[0]), ctypes.byref(need))
    self._ws_bytes = need.value
    self.workspace = torch.empty((max(need.value, 1),), dtype=torch.uint8, device=dev)
    self._level_anchors = (ctypes.c_int * len(self.levels))(*self.labeler._lanch)
    self._own = None

  # ---- draws ----------------------------------------------------------------------------------------------------------
  def check_sizes(self, sizes):
    """sizes of a canvas batch, checked (utils.canvas_sizes; with grid_mask also gridmask.block_range per image, which names
    the image) -> int32 numpy [B, 2]; None stays None.  Host data: a device tensor is copied to the host once, and that copy
    waits for the device."""
    if sizes is None:
      return None
    sizes = utils.canvas_sizes(sizes, self.batch, self.height, self.width)
    if self.grid_mask:
      f = np.float32
      lo = np.minimum(sizes[:, 0].astype(f) * f(0.5), sizes[:, 1].astype(f) * f(0.3))      # block_range's, for all at once
      for i in np.flatnonzero(lo < 1):
        gridmask_lib.block_range(int(sizes[i, 0]), int(sizes[i, 1]), image=int(i))      # raises
    return sizes

  def _hw(self, sizes):
    """What the argument builders take as (h, w): the stage's two numbers, or the per-image arrays of a canvas batch."""
    return (self.height, self.width) if sizes is None else (sizes[:, 0], sizes[:, 1])

  def draw(self, rng, sizes=None):
    """One step's draws from a numpy generator: flip [B] and scale [B, 3] uniform float32 in [0, 1) (what
    DetectionInputProcessor's setters take as `draws`), gridmask = gridmask_draws' five arrays (None without grid_mask),
    autoaug = det_autoaugment.autoaug_draws' tuple (None without the switch; taken last, so that the stream of a model
    without it does not move).  sizes: a canvas batch's [B, 2], checked before the generator moves; flip and scale are drawn
    as without, GridMask's d over each image's own range (gridmask.gridmask_draws: a stream of its own, not promised equal
    to the dense one), everything after it as without."""
    b = self.batch
    sizes = self.check_sizes(sizes)
    flip = rng.random((b, 1)).astype(np.float32)[:, 0]
    scale = rng.random((b, 3)).astype(np.float32)
    gm = gridmask_lib.gridmask_draws(rng, b, *self._hw(sizes)) if self.grid_mask else None
    aa = None
    if self._aa_policy is not None:
      aa = det_autoaugment.autoaug_draws(rng, b, self._aa_policy, RANDAUG_NUM_LAYERS)
    return Draws(flip, scale, gm, aa)

  def rows(self, draws, sizes=None):
    """draws -> (edet_prep_image_t rows int32 [B, 5], edet_gridmask_image_t rows or None, AutoAugment's packed argument
    arrays uint8 or None -- det_autoaugment.pack_args of autoaug_args), on the host.  sizes: check_sizes' array of a canvas
    batch -- row i is then the row of image i alone at its own size."""
    c = self.config
    hs, ws = self._hw(sizes)
    flip, scale, gm, aa = Draws(*draws)
    u = np.asarray(scale, np.float32).reshape(self.batch, 3)
    per = np.zeros((self.batch, 5), np.int32)
    if c.input_rand_hflip:
      per[:, 0] = preprocess.flip_decisions(np.asarray(flip, np.float32).reshape(self.batch))
    for i in range(self.batch):
      _, per[i, 1:3], per[i, 3:5] = preprocess.training_scale_factors(
          u[i], c.jitter_min, c.jitter_max, self.target_size, self.output_size,
          self.height if sizes is None else int(hs[i]), self.width if sizes is None else int(ws[i]))
    if int(per[:, 1:3].min()) < 1:
      raise ValueError('the scaled image is empty')
    mask = None
    if self.grid_mask:
      if gm is None:
        raise ValueError('config.grid_mask is set: draws need the five GridMask arrays (gridmask.gridmask_draws)')
      mask = gridmask_lib.gridmask_args(gm, hs, ws)      # gridmask.gridmask's defaults (dataloader.py:310)
      if mask.shape[0] != self.batch:
        raise ValueError('GridMask draws for %d images, batch %d' % (mask.shape[0], self.batch))
    packed = None
    if self._aa_policy is not None:
      if aa is None:
        raise ValueError('the autoaugment switch is on (%r): draws need det_autoaugment.autoaug_draws\' tuple' % (self.autoaugment,))
      packed, layout = det_autoaugment.pack_args(det_autoaugment.autoaug_args(
          aa, self._aa_policy, hs, ws, magnitude=RANDAUG_MAGNITUDE))
      if layout != self._aa_layout:
        raise ValueError('AutoAugment draws for %s, want [layers, batch] = %s'
                         % (layout['policy'][1], self._aa_layout['policy'][1]))
    return per, mask, packed

  # ---- destinations ---------------------------------------------------------------------------------------------------
  def label_shapes(self):
    """{label name: (shape, dtype)} of what run() fills, the train step's label layout (dataloader.py:369-382)."""
    b, a = self.batch, self.labeler._a
    out = collections.OrderedDict()
    for level, (h, w) in zip(self.levels, self.labeler._hw):
      out['cls_targets_%d' % level] = ((b, h, w, a), torch.int32)
      out['box_targets_%d' % level] = ((b, h, w, a * 4), torch.float32)
    out['mean_num_positives'] = ((b, 1), torch.float32)
    return out

  def own_buffers(self):
    """(images, labels) buffers of this object's own, allocated at the first call: the destinations of a step that has no
    captured graph's buffers to write into."""
    if self._own is None:
      oh, ow = self.output_size
      images = torch.empty((self.batch, oh, ow, 3), dtype=self.dtype, device=self.device)
      labels = {k: torch.empty(shape, dtype=dt, device=self.device) for k, (shape, dt) in self.label_shapes().items()}
      self._own = (images, labels)
    return self._own

  def _check_destinations(self, images, labels):
    oh, ow = self.output_size
    if tuple(images.shape) != (self.batch, oh, ow, 3) or images.dtype != self.dtype or not images.is_contiguous():
      raise ValueError('images destination must be a dense %s %s, got %s %s'
                       % (self.dtype, (self.batch, oh, ow, 3), images.dtype, tuple(images.shape)))
    for k, (shape, dt) in self.label_shapes().items():
      t = labels.get(k)
      n = int(np.prod(shape))
      if t is None or t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != images.device:
        raise ValueError('labels destination %r must be a dense %s tensor of %d elements on %s'
                         % (k, dt, n, images.device))

  # ---- the launches ---------------------------------------------------------------------------------------------------
  def run(self, raw_images, boxes, classes, counts, draws, images, labels, stream=None, sizes=None):
    """raw_images uint8 [B, H, W, 3], boxes float32 [B, M, 4] normalised (ymin, xmin, ymax, xmax), classes [B, M], counts
    [B] (device tensors, or host arrays that are copied over) -> fills `images` [B, h, w, 3] and `labels`
    {'cls_targets_<l>', 'box_targets_<l>', 'mean_num_positives'} in place, on torch's current stream.  sizes [B, 2]: the
    batch is a canvas batch, image i the top-left sizes[i] = (height, width) of its slot (host data, check_sizes; `draws`
    made for the same sizes); checked before any launch."""
    sizes = self.check_sizes(sizes)
    raw, boxes, classes, counts, stream = self._canonical(raw_images, boxes, classes, counts, stream)
    self._check_destinations(images, labels)
    per, mask, packed = self.rows(draws, sizes)
    self.prep_rows.copy_(torch.from_numpy(per).pin_memory(), non_blocking=True)
    sizes_dev = self._upload_sizes(sizes)
    src = raw
    if self.grid_mask:
      self.mask_rows.copy_(gridmask_lib.args_tensor(mask, pin=True), non_blocking=True)
      src = gridmask_lib.apply_mask(raw, self.masked, self.mask_rows, stream, sizes_dev)
    if self._aa_policy is not None:      # dataloader.py:312-319: after GridMask, on the uint8 image and the boxes
      self.aa_rows.copy_(torch.from_numpy(packed).pin_memory(), non_blocking=True)
      src, boxes = det_autoaugment.apply_layers(src, self.aa_images, boxes, self.aa_boxes, counts, self.aa_args, self.aa_luts,
                                                self.aa_scratch, stream, sizes_dev)
    self._launch(src, boxes, classes, counts, images, labels, stream, sizes_dev)
    return images, labels

  def _upload_sizes(self, sizes):
    """check_sizes' array -> the stage's device buffer, filled by one pinned copy (None stays None)."""
    if sizes is None:
      return None
    self.sizes_dev.copy_(torch.from_numpy(sizes).pin_memory(), non_blocking=True)
    return self.sizes_dev

  def _canonical(self, raw_images, boxes, classes, counts, stream):
    """The arguments run() takes, checked and on the device -> (raw uint8 [B, H, W, 3], boxes float32 [B, M, 4], classes
    float32 [B, M], counts int32 [B], stream handle: torch's current stream unless one was given).  They are kept alive
    until the next call: the launches that read them are asynchronous."""
    b, m, dev = self.batch, self.max_boxes, self.device
    raw = torch.as_tensor(raw_images)
    if raw.dtype != torch.uint8 or tuple(raw.shape) != (b, self.height, self.width, 3):
      raise ValueError('raw images must be uint8 %s, got %s %s' % ((b, self.height, self.width, 3), raw.dtype, tuple(raw.shape)))
    raw = raw.to(dev).contiguous()
    boxes = torch.as_tensor(boxes, dtype=torch.float32).to(dev).reshape(b, m, 4).contiguous()
    classes = torch.as_tensor(classes).to(dev).to(torch.float32).reshape(b, m).contiguous()
    counts = torch.as_tensor(counts).to(dev).to(torch.int32).reshape(b).contiguous()
    if stream is None:
      stream = torch.cuda.current_stream(dev).cuda_stream
    self._keep_alive = (raw, boxes, classes, counts)
    return raw, boxes, classes, counts, stream

  def _launch(self, src, boxes, classes, counts, images, labels, stream, sizes_dev=None):
    """edet_preprocess_train (with sizes_dev its canvas sibling) with the rows in prep_rows, edet_label_anchors,
    mean_num_positives: what the training and the evaluation stage share."""
    b, m = self.batch, self.max_boxes
    tail = (self.output_size[0], self.output_size[1], self._mean, self._std, ptr(self.prep_rows), ptr(images), ptr(boxes),
            ptr(classes), ptr(counts), m, ptr(self.boxes), ptr(self.classes), ptr(self.counts),
            _lib.EDET_BF16 if self.dtype == torch.bfloat16 else _lib.EDET_F32, stream)
    if sizes_dev is None:
      call('edet_preprocess_train', ptr(src), 0, b, self.height, self.width, *tail)
    else:
      call('edet_preprocess_train_canvas', ptr(src), 0, b, self.height, self.width, ptr(sizes_dev), *tail)
    self.labels.copy_(self.classes)      # float class ids (-1 padded) -> int32, as label_anchors_batch takes them
    nlev = len(self.levels)
    cp = (ctypes.c_void_p * nlev)(*[labels['cls_targets_%d' % l].data_ptr() for l in self.levels])
    bp = (ctypes.c_void_p * nlev)(*[labels['box_targets_%d' % l].data_ptr() for l in self.levels])
    call('edet_label_anchors', ptr(self.labeler._boxes), self._level_anchors, nlev, ptr(self.boxes), ptr(self.labels),
         ptr(self.counts), b, m, float(self.labeler._match_threshold), ptr(self.workspace), self._ws_bytes, cp, bp,
         ptr(self.num_positives), stream)
    labels['mean_num_positives'].view(b, 1).copy_(mean_num_positives(self.num_positives))


def split_raw(raw):
  """The raw-images field of a raw batch -> (raw, sizes): `raw` itself with sizes None (a dense batch), or the pair (raw, sizes)
  of a canvas batch, as jpeg.JpegDecoder.decode returns it and the EfficientNetV2 trainer takes it."""
  if isinstance(raw, (tuple, list)) and len(raw) == 2 and np.ndim(raw[0]) == 4:
    return raw[0], raw[1]
  return raw, None


def parse_source_ids(source_ids):
  """dataloader.py:340-342: an empty source id is -1, the others tf.strings.to_number's float32.  Numbers pass through."""
  a = np.asarray(source_ids)
  if a.dtype.kind in 'USO':
    a = np.asarray([float(v) if str(v) != '' else -1.0 for v in a.reshape(-1).tolist()])
  return a.astype(np.float32).reshape(-1)


def check_max_instances(config, max_boxes):
  """-> config.max_instances_per_image (100 when unset); more box ROWS than that raise, on the host (dataloader.py:228,
  pad_to_fixed_size)."""
  max_instances = int(getattr(config, 'max_instances_per_image', None) or 100)
  if int(max_boxes) > max_instances:
    raise ValueError('ERROR: please increase config.max_instances_per_image (%d box rows, max_instances_per_image %d; '
                     'dataloader.pad_to_fixed_size)' % (max_boxes, max_instances))
  return max_instances


def eval_rows(output_size, sizes):
  """sizes int [B, 2] = (height, width) per image -> (edet_prep_image_t rows int32 [B, 5], image_scales float32 [B] =
  image_scale_to_original) on the host: set_scale_factors_to_output_size per image (dataloader.py:113-124), no flip, no
  offset."""
  sizes = np.asarray(sizes)
  per, scales = np.zeros((sizes.shape[0], 5), np.int32), np.zeros(sizes.shape[0], np.float32)
  for i in range(sizes.shape[0]):
    scale, per[i, 1:3] = preprocess.output_size_scale_factors(output_size, int(sizes[i, 0]), int(sizes[i, 1]))
    if int(per[i, 1:3].min()) < 1:
      raise ValueError('image %d: the scaled image is empty' % i)
    scales[i] = np.float32(1.0) / scale
  return per, scales


class DetectionEvalInput(DetectionInput):
  """The evaluation branch of ``InputReader.dataset_parser`` plus ``process_example`` (dataloader.py:321-323, :331-353,
  :369-392) for one (batch, raw size, box rows) shape: ``normalize_image``, ``set_scale_factors_to_output_size`` -- no flip,
  no crop offset, no draws, neither GridMask nor AutoAugment --, ``resize_and_crop_image`` / ``resize_and_crop_boxes``
  (edet_preprocess_train), ``label_anchors`` (edet_label_anchors), ``mean_num_positives``, and the ground truth of the batch
  (edet_pack_groundtruth): 3 launches of this library plus the small copies.  The per-image rows and ``image_scales`` are
  constants of the shape: computed and uploaded once, here.

  ``labels`` gets what the training stage writes plus ``source_ids`` float32 [B] (an empty id is -1, :340-342),
  ``image_scales`` float32 [B] = image_scale_to_original (:345) and ``groundtruth_data`` float32 [B,
  max_instances_per_image, 7], rows [y1, x1, y2, x2, is_crowd, area, class] in pixels of the ORIGINAL image.

  Kept as the reference is written: ``resize_and_crop_boxes`` drops zero-area boxes together with their classes (:186-190)
  but ``is_crowds`` and ``areas`` are not filtered, so after a dropped box columns 4 and 5 of the later rows belong to a
  different annotation than columns 0-3 and 6.  ``pad_to_fixed_size`` asserts instances < max_instances_per_image (:228, a
  strict less); more box ROWS than max_instances_per_image raise here, on the host, and an image that fills every row is
  packed without padding rows instead of failing.

  ``run(..., sizes=)``: a canvas batch (see the module's docstring).  The rows and ``image_scales`` are then computed per call
  from the sizes -- ``set_scale_factors_to_output_size`` per image -- and uploaded; without sizes the constants of the shape are
  used."""

  TRAINING = False

  def __init__(self, config, anchors, batch, height, width, max_boxes, dtype=torch.float32, device='cuda:0'):
    self.max_instances = check_max_instances(config, max_boxes)
    super().__init__(config, anchors, batch, height, width, max_boxes, dtype=dtype, device=device)
    b, m, dev = self.batch, self.max_boxes, self.device
    scale, scaled = preprocess.output_size_scale_factors(self.output_size, self.height, self.width)
    if min(scaled) < 1:
      raise ValueError('the scaled image is empty')
    per = np.zeros((b, 5), np.int32)      # flip 0, offsets 0
    per[:, 1:3] = scaled
    self.prep_rows.copy_(torch.from_numpy(per))
    self.image_scale = scale
    self.image_scales = torch.full((b,), float(np.float32(1.0) / scale), dtype=torch.float32, device=dev)
    self._shape_rows = (per, np.full(b, np.float32(1.0) / scale, np.float32))      # what a dense call puts back after a canvas one
    self._rows_of_shape = True
    self.is_crowds = torch.empty((b, m), dtype=torch.float32, device=dev)
    self.areas = torch.empty((b, m), dtype=torch.float32, device=dev)

  def draw(self, rng, sizes=None):
    raise TypeError('the evaluation input makes no draws')

  def label_shapes(self):
    out = super().label_shapes()
    b = self.batch
    out['source_ids'] = ((b,), torch.float32)
    out['image_scales'] = ((b,), torch.float32)
    out['groundtruth_data'] = ((b, self.max_instances, 7), torch.float32)
    return out

  def run(self, raw_images, boxes, classes, counts, is_crowds, areas, source_ids, images, labels, stream=None, sizes=None):
    """raw_images uint8 [B, H, W, 3], boxes float32 [B, M, 4] normalised (ymin, xmin, ymax, xmax), classes [B, M], counts [B],
    is_crowds [B, M] (bool or 0 / 1), areas [B, M], source_ids [B] (numbers, or strings with '' for none) -> fills `images`
    and `labels` in place, on torch's current stream.  sizes [B, 2]: a canvas batch (host data, check_sizes), checked before
    any launch."""
    b, m = self.batch, self.max_boxes
    sizes = self.check_sizes(sizes)
    raw, boxes, classes, counts, stream = self._canonical(raw_images, boxes, classes, counts, stream)
    self._check_destinations(images, labels)
    if sizes is not None or not self._rows_of_shape:
      per, scales = self._shape_rows if sizes is None else eval_rows(self.output_size, sizes)
      self.prep_rows.copy_(torch.from_numpy(per).pin_memory(), non_blocking=True)
      self.image_scales.copy_(torch.from_numpy(scales).pin_memory(), non_blocking=True)
      self._rows_of_shape = sizes is None
    sizes_dev = self._upload_sizes(sizes)
    self.is_crowds.copy_(torch.as_tensor(is_crowds).reshape(b, m), non_blocking=True)      # tf.cast(is_crowds, float32), :347
    self.areas.copy_(torch.as_tensor(areas).reshape(b, m), non_blocking=True)
    if not torch.is_tensor(source_ids):
      source_ids = torch.from_numpy(parse_source_ids(source_ids))
    labels['source_ids'].view(b).copy_(source_ids.reshape(b), non_blocking=True)
    labels['image_scales'].view(b).copy_(self.image_scales)
    self._launch(raw, boxes, classes, counts, images, labels, stream, sizes_dev)
    call('edet_pack_groundtruth', ptr(self.boxes), ptr(self.classes), ptr(self.counts), ptr(self.is_crowds), ptr(self.areas),
         ptr(counts), ptr(self.image_scales), b, m, self.max_instances, ptr(labels['groundtruth_data']), stream)
    return images, labels
