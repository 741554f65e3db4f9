"""The legacy EfficientNet input pipeline for a canvas batch on the device: the reference's ``efficientnetv2/preprocess_legacy.py``
by its names -- what ``preprocessing.py:133-139`` switches to for every recipe whose ``augname`` starts with ``effnetv1_``
(``efficientnetv2-b0 .. b3``, ``efficientnet-b0 .. b7``).

``preprocess_for_train`` (:136-181) = a random crop (``sample_distorted_bounding_box`` on the whole image as the one box:
area in [0.08, 1], aspect ratio in [3/4, 4/3], 10 attempts, min_object_covered 0.1; the padded centre crop where the sampler
hands back the whole image, :99-105) -> ``tf.image.resize_bicubic`` to the training size -> random left-right flip ->
[clip / cast to uint8 -> AutoAugment v0 or RandAugment] ; ``preprocess_for_eval`` (:184-199) = the padded centre crop
(:110-127) -> the same resize; ``preprocess_image`` (:202-244) = either, then (x - MEAN_RGB) / STDDEV_RGB.  The draws are made
on the host (``legacy_train_rows`` / ``legacy_eval_rows``: edet_crop_image_t rows, as ``v2_preprocessing.train_rows``) and the
pixels are moved by ``edet_crop_resize_bicubic`` (csrc/crop_bicubic.hip), ``edet_randaug_stats`` / ``edet_randaug_apply`` and
``edet_randaug_apply_norm`` (csrc/randaug.hip).  The restatements are tests/bicubic_ref.py and tests/autoaug_ref.py.

What is pinned: the wiring, against the reference module executed unmodified on a stand-in (tests/golden/
make_golden_legacy.py): the "bad" fallback, the centre crop's arithmetic and offsets, the clip / cast, the operation order,
the constants.  What is not: TensorFlow's legacy bicubic itself (tests/bicubic_ref.py is the definition; TensorFlow is not
installed where this project is tested), and the crop sampler's and AutoAugment's random streams (``v2_preprocessing`` and
``autoaugment`` state theirs).

Deliberate difference: the reference normalises in ``image_dtype`` (a bfloat16 image is subtracted and divided in bfloat16).
Here the arithmetic is float32 -- (x - mean) / std, two rounded operations -- and bfloat16 is one final rounding.

Not built: ``resize_method`` other than the default bicubic.
"""
import numpy as np
import torch

from automl_amd import autoaugment
from automl_amd import v2_preprocessing
from automl_amd.v2_preprocessing import _sizes, sample_distorted_bounding_box

CROP_PADDING = 32      # :117
MEAN_RGB = np.array([0.485 * 255, 0.456 * 255, 0.406 * 255], np.float32)        # :240
STDDEV_RGB = np.array([0.229 * 255, 0.224 * 255, 0.225 * 255], np.float32)      # :241
NORM = (MEAN_RGB, STDDEV_RGB)
AUGMENT_NAMES = (None, 'autoaug', 'randaug')
_DTYPES = {None: torch.float32, torch.float32: torch.float32, torch.bfloat16: torch.bfloat16}


def check_augment_name(augment_name):
  """None (or '': the reference tests `if augment_name`), 'autoaug' or 'randaug'; else the reference's ValueError (:178)."""
  if not augment_name:
    return None
  if augment_name not in AUGMENT_NAMES:
    raise ValueError('Invalid value for augment_name: %s' % (augment_name,))
  return augment_name


def center_crop_window(height, width, image_size):
  """_decode_and_center_crop's window (:110-127) -> (y, x, c, c): c = int(float32(image_size / (image_size + 32)) *
  float32(min(h, w))), at (((h - c) + 1) // 2, ((w - c) + 1) // 2).  Where the product truncates to 0 (min(h, w) = 1) the
  crop is the one pixel: the reference's decode_and_crop_jpeg would refuse the empty window."""
  h, w = int(height), int(width)
  ratio = np.float32(image_size / (image_size + CROP_PADDING))
  c = max(int(ratio * np.float32(min(h, w))), 1)
  return ((h - c) + 1) // 2, ((w - c) + 1) // 2, c, c


def train_crop_window(rng, height, width, image_size):
  """_decode_and_random_crop's window (:88-107) for an image of height x width -> (y, x, h, w): the sampler's box, or the
  padded centre crop where that box is the whole image ("bad", :99-105).  The one function behind legacy_train_rows and the
  reader's decode_crop='legacy' windows (effnetv2_datasets)."""
  h, w = int(height), int(width)
  box = sample_distorted_bounding_box(rng, h, w, area_range=(0.08, 1.0), aspect_ratio_range=(3. / 4, 4. / 3.), max_attempts=10,
                                      min_object_covered=0.1)
  if box[2] == h and box[3] == w:
    return center_crop_window(h, w, image_size)
  return box


def _image_size(image_size):
  if int(image_size) != image_size or int(image_size) < 1:
    raise ValueError('image_size %r must be a positive integer' % (image_size,))
  return int(image_size)


def legacy_train_rows(rng, sizes, image_size):
  """preprocess_for_train's draws (:161-162) for images of `sizes` [B, 2] -> int32 [B, 8] in edet_crop_image_t's field order.
  Per image train_crop_window, then the flip bit at probability 1/2."""
  image_size = _image_size(image_size)
  s = _sizes(sizes)
  rows = np.zeros((s.shape[0], 8), np.int32)
  for k, (h, w) in enumerate(s):
    box = train_crop_window(rng, h, w, image_size)
    flip = int(rng.random() < 0.5)
    rows[k] = (h, w) + tuple(box) + (flip, 0)
  return rows


def legacy_flip_rows(rng, sizes):
  """Whole-image rows plus the flip draw: for images that a reader already cut to their windows (decode_crop='legacy')."""
  s = _sizes(sizes)
  rows = np.zeros((s.shape[0], 8), np.int32)
  for k, (h, w) in enumerate(s):
    rows[k] = (h, w, 0, 0, h, w, int(rng.random() < 0.5), 0)
  return rows


def legacy_eval_rows(sizes, image_size):
  """preprocess_for_eval (:184-199) -> int32 [B, 8]: center_crop_window per image, never flipped."""
  image_size = _image_size(image_size)
  s = _sizes(sizes)
  rows = np.zeros((s.shape[0], 8), np.int32)
  for k, (h, w) in enumerate(s):
    rows[k] = (h, w) + center_crop_window(h, w, image_size) + (0, 0)
  return rows


def _raw(raw, sizes):
  x = torch.from_numpy(raw) if isinstance(raw, np.ndarray) else raw
  if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
    raise ValueError('raw must be uint8 [batch, canvas_h, canvas_w, 3], got %s %s' % (x.dtype, tuple(x.shape)))
  b, hc, wc = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
  s = np.tile(np.array([hc, wc], np.int64), (b, 1)) if sizes is None else _sizes(sizes)
  if s.shape[0] != b or (s[:, 0] > hc).any() or (s[:, 1] > wc).any():
    raise ValueError('sizes must be [batch, 2] = (height, width) inside the %d x %d canvas, got %s' % (hc, wc, s.tolist()))
  return x, s


def _dtype(image_dtype):
  if image_dtype not in _DTYPES:
    raise ValueError('image_dtype %r: None / torch.float32 or torch.bfloat16' % (image_dtype,))
  return _DTYPES[image_dtype]


def preprocess_for_train(raw, sizes, image_size, augment_name=None, randaug_num_layers=None, randaug_magnitude=None,
                         image_dtype=None, rng=None, rows=None, draws=None):
  """preprocess_for_train (:136-181) and the normalisation of :239-243 for a canvas batch: raw uint8 [B, Hc, Wc, 3] (numpy or
  torch) with `sizes` [B, 2] (None: every image fills the canvas) -> the normalised batch [B, image_size, image_size, 3] on
  the device, float32 or image_dtype torch.bfloat16.  rows: legacy_train_rows' array, else drawn from `rng` (a numpy
  Generator; default a fresh one); draws: autoaugment.autoaug_draws' / randaug_draws' arrays for the augment_name, else
  drawn from `rng` after the rows.  Without an augment_name the resized float values are normalised as they are; with one
  they are clipped and cast to uint8 first (:168-169)."""
  augment_name = check_augment_name(augment_name)
  dtype = _dtype(image_dtype)
  image_size = _image_size(image_size)
  x, s = _raw(raw, sizes)
  if augment_name == 'randaug':
    layers = 2 if randaug_num_layers is None else int(randaug_num_layers)
    if layers < 0:
      raise ValueError('randaug_num_layers %r must be >= 0' % (randaug_num_layers,))
    magnitude = autoaugment.check_magnitude(15 if randaug_magnitude is None else randaug_magnitude)
  rng = rng if rng is not None else np.random.default_rng()
  if rows is None:
    rows = legacy_train_rows(rng, s, image_size)
  if augment_name is None:
    return v2_preprocessing.crop_resize(x, rows, image_size, dtype, method='bicubic', norm=NORM)
  u8 = v2_preprocessing.crop_resize(x, rows, image_size, torch.uint8, method='bicubic')
  b = int(u8.shape[0])
  if augment_name == 'autoaug':
    table = autoaugment.policy_v0()
    if draws is None:
      draws = autoaugment.autoaug_draws(rng, b, table)
    return autoaugment._run_layers(u8, autoaugment.autoaug_args(draws, image_size, image_size, table), len(table[0]), dtype, NORM)
  if draws is None:
    draws = autoaugment.randaug_draws(rng, b, layers)
  if np.asarray(draws[0]).shape != (layers, b):
    raise ValueError('draws are %s, want [num_layers, batch] = %s' % (np.asarray(draws[0]).shape, (layers, b)))
  return autoaugment._run_layers(u8, autoaugment.randaug_args(draws, magnitude, image_size, image_size), layers, dtype, NORM)


def preprocess_for_eval(raw, sizes, image_size, image_dtype=None, rows=None):
  """preprocess_for_eval (:184-199) and the normalisation of :239-243 for a canvas batch -> the normalised batch on the
  device.  rows: legacy_eval_rows' array (default: computed from the sizes)."""
  dtype = _dtype(image_dtype)
  image_size = _image_size(image_size)
  x, s = _raw(raw, sizes)
  if rows is None:
    rows = legacy_eval_rows(s, image_size)
  return v2_preprocessing.crop_resize(x, rows, image_size, dtype, method='bicubic', norm=NORM)


def preprocess_image(raw, sizes, image_size, is_training=False, image_dtype=None, augment_name=None, randaug_num_layers=None,
                     randaug_magnitude=None, rng=None, rows=None, draws=None):
  """preprocess_image (:202-244) for a canvas batch -> the normalised network input on the device."""
  check_augment_name(augment_name)
  if is_training:
    return preprocess_for_train(raw, sizes, image_size, augment_name, randaug_num_layers, randaug_magnitude, image_dtype, rng,
                                rows, draws)
  return preprocess_for_eval(raw, sizes, image_size, image_dtype, rows)
