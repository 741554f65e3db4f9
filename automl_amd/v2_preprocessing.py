"""The front of the EfficientNetV2 input pipeline for a batch: the reference's ``efficientnetv2/preprocessing.py:22-70``.

``preprocess_for_train`` (:22-55) = random crop (``tf.image.sample_distorted_bounding_box`` without boxes, area in
[0.05, 1], aspect ratio in [0.75, 1.33]) -> bilinear resize to the training size -> random left-right flip;
``preprocess_for_eval`` (:58-70) = centre crop (below 320, or when asked) -> resize.  The draws are made on the host
(``train_rows`` / ``eval_rows``: eight integers per image, the kernel's ``edet_crop_image_t``) and the pixels are moved by
``edet_crop_resize`` (csrc/crop_resize.hip) from a batch of decoded uint8 images, each in the top-left corner of a common
canvas (``pad_batch``).  The numpy restatement the kernel is compared with bit for bit is tests/crop_ref.py.

What cannot be pinned against TensorFlow here (it is not installed, and both pieces are C++ outside the reference tree):

* the crop sampler's random stream and its tie-breaking.  ``sample_distorted_bounding_box`` below implements the published
  algorithm of the op for the reference's call -- per attempt an aspect ratio uniform in its range, a height uniform among
  the integers whose area at that ratio lies in the area range and whose width fits the image, width = round(height *
  ratio), a uniform position, and the whole image after ``max_attempts`` failures -- on a numpy PCG64 generator.  The tests
  pin its properties (inside the image, area and aspect ranges, the fallback rate), not a stream.
* the staircase of ``tf.image.resize`` for scales that float32 does not represent exactly: the kernel computes
  ``(o + 0.5) * (crop_n / out_n) - 0.5`` in float32 as oracle/preprocess_oracle.resize_bilinear and csrc/preprocess.hip do;
  where TensorFlow's own float32 evaluation lands on the other side of an integer the two taps' weights differ by one ulp's
  worth, never the taps' range.
"""
import ctypes
import math

import numpy as np
import torch

from automl_amd import _lib
from automl_amd._lib import call, ptr

ROW_FIELDS = ('height', 'width', 'crop_y', 'crop_x', 'crop_h', 'crop_w', 'flip', 'reserved')      # edet_crop_image_t
_OUT = {None: (_lib.EDET_U8, torch.uint8), torch.uint8: (_lib.EDET_U8, torch.uint8),
        torch.float32: (_lib.EDET_F32, torch.float32), torch.bfloat16: (_lib.EDET_BF16, torch.bfloat16)}


def pad_batch(images, canvas=None):
  """A list of uint8 [h, w, 3] images (numpy or torch) -> (uint8 tensor [B, Hc, Wc, 3], sizes int32 [B, 2] = (h, w)): every
  image in the top-left corner of a zero canvas.  canvas = (Hc, Wc), default the largest height and width of the list; an
  image larger than a given canvas raises.  A fixed canvas keeps the trainer's captured step (TrainableModel.train_step)."""
  if not len(images):
    raise ValueError('pad_batch: no images')
  items = [torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im for im in images]
  for k, im in enumerate(items):
    if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[-1] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
      raise ValueError('pad_batch: image %d must be uint8 [h, w, 3] with h, w >= 1, got %s %s' % (k, im.dtype, tuple(im.shape)))
  sizes = np.array([[int(im.shape[0]), int(im.shape[1])] for im in items], np.int32)
  hc, wc = (int(sizes[:, 0].max()), int(sizes[:, 1].max())) if canvas is None else (int(canvas[0]), int(canvas[1]))
  if sizes[:, 0].max() > hc or sizes[:, 1].max() > wc:
    raise ValueError('pad_batch: an image of %d x %d does not fit the %d x %d canvas' % (sizes[:, 0].max(), sizes[:, 1].max(), hc, wc))
  out = torch.zeros((len(items), hc, wc, 3), dtype=torch.uint8, device=items[0].device)
  for k, im in enumerate(items):
    out[k, :im.shape[0], :im.shape[1]] = im
  return out, sizes


def _round(v):
  """C's lrint in the default rounding mode: halves to even (Python's round)."""
  return int(round(v))


def sample_distorted_bounding_box(rng, height, width, area_range=(0.05, 1.0), aspect_ratio_range=(0.75, 1.33), max_attempts=100,
                                  min_object_covered=0.0):
  """tf.image.sample_distorted_bounding_box for the reference's call (preprocessing.py:32-37: no boxes,
  min_object_covered=0, use_image_if_no_bounding_boxes=True) -> (y, x, h, w) of the crop.  `rng`: a numpy Generator.
  TensorFlow's generator stream and tie-breaking are not reproduced (module docstring).
  min_object_covered: the legacy pipeline's call (preprocess_legacy.py:88-98) hands the op ONE box, the whole image, and
  0.1: a candidate covers the fraction (its area) / (the image's area) of that box, so one whose area is below
  min_object_covered x the image's area is a failed attempt.  At the default 0 nothing changes: the same draws are consumed
  and the same box returned."""
  height, width = int(height), int(width)
  if height < 1 or width < 1:
    raise ValueError('image %d x %d' % (height, width))
  min_area, max_area = area_range[0] * height * width, area_range[1] * height * width
  for _ in range(int(max_attempts)):
    ratio = rng.uniform(aspect_ratio_range[0], aspect_ratio_range[1])
    h_min = _round(math.sqrt(min_area / ratio))
    h_max = _round(math.sqrt(max_area / ratio))
    if _round(h_max * ratio) > width:      # the widest crop that still fits
      h_max = int((width + 0.5 - 1e-7) / ratio)
      if _round(h_max * ratio) > width:
        h_max -= 1
    h_max = min(h_max, height)
    h = min(h_min, h_max)
    if h < h_max:
      h += int(rng.integers(0, h_max - h + 1))
    w = _round(h * ratio)
    # the rounding of either side may have carried the area just outside its range: one step back in
    if w * h < min_area:
      h += 1
      w = _round(h * ratio)
    if w * h > max_area:
      h -= 1
      w = _round(h * ratio)
    if w * h < min_area or w * h > max_area or w > width or h > height or w <= 0 or h <= 0:
      continue
    if w * h < min_object_covered * height * width:      # (never at the default 0)
      continue
    y = int(rng.integers(0, height - h + 1))
    x = int(rng.integers(0, width - w + 1))
    return y, x, h, w
  return 0, 0, height, width


def crop_rng(seed):
  """The generator behind the crop and flip draws of a model built with `seed`."""
  return np.random.Generator(np.random.PCG64([int(seed), 0x63726f70]))


def _sizes(sizes):
  s = np.asarray(sizes)
  if s.ndim != 2 or s.shape[1] != 2 or s.shape[0] < 1 or (s < 1).any():
    raise ValueError('sizes must be [batch, 2] = (height, width) with both >= 1, got %s' % (s.tolist() if s.size < 32 else s.shape,))
  return s.astype(np.int64)


def train_rows(rng, sizes, transformations='crop|flip'):
  """preprocess_for_train's draws (:29-44) for images of `sizes` [B, 2] -> int32 [B, 8] in edet_crop_image_t's field order.
  With 'crop' in `transformations` the box of sample_distorted_bounding_box, else the whole image; with 'flip' one bit per
  image at probability 1/2, else 0.  Per image the crop is drawn before the flip."""
  transformations = 'crop|flip' if transformations is None else transformations
  s = _sizes(sizes)
  rows = np.zeros((s.shape[0], 8), np.int32)
  for k, (h, w) in enumerate(s):
    box = sample_distorted_bounding_box(rng, h, w) if 'crop' in transformations else (0, 0, h, w)
    flip = int(rng.random() < 0.5) if 'flip' in transformations else 0
    rows[k] = (h, w) + tuple(box) + (flip, 0)
  return rows


def eval_rows(sizes, image_size, transformations=None):
  """preprocess_for_eval (:58-70) -> int32 [B, 8]: the centre crop of int(float32(image_size / (image_size + 32)) *
  float32(min(h, w))) pixels at ((h - crop) // 2, (w - crop) // 2) when image_size < 320 or 'crop' is asked for, else the
  whole image; never flipped.  Where that product truncates to 0 (min(h, w) = 1) the crop is the one pixel: the reference's
  crop_to_bounding_box would refuse the empty box."""
  image_size = int(image_size)
  if image_size < 1:
    raise ValueError('image_size %r' % (image_size,))
  if transformations is None or transformations == '':
    transformations = 'crop' if image_size < 320 else ''
  s = _sizes(sizes)
  rows = np.zeros((s.shape[0], 8), np.int32)
  ratio = np.float32(image_size / (image_size + 32))
  for k, (h, w) in enumerate(s):
    if 'crop' in transformations:
      crop = max(int(ratio * np.float32(min(h, w))), 1)
      rows[k] = (h, w, (h - crop) // 2, (w - crop) // 2, crop, crop, 0, 0)
    else:
      rows[k] = (h, w, 0, 0, h, w, 0, 0)
  return rows


def whole_rows(batch, height, width):
  """Rows that take every image whole and unflipped (images that fill their canvas)."""
  return np.tile(np.array([height, width, 0, 0, height, width, 0, 0], np.int32), (int(batch), 1))


def clamp_rows(rows, canvas_h, canvas_w):
  """What edet_crop_resize makes of every field it reads from device memory: height into [1, canvas_h], width into
  [1, canvas_w], crop_y into [0, height - 1], crop_h into [1, height - crop_y], likewise for x, flip != 0 -> int32 [B, 8]."""
  r = np.array(rows, dtype=np.int64).reshape(-1, 8)
  out = np.zeros_like(r)
  out[:, 0] = np.clip(r[:, 0], 1, canvas_h)
  out[:, 1] = np.clip(r[:, 1], 1, canvas_w)
  out[:, 2] = np.clip(r[:, 2], 0, out[:, 0] - 1)
  out[:, 3] = np.clip(r[:, 3], 0, out[:, 1] - 1)
  out[:, 4] = np.clip(r[:, 4], 1, out[:, 0] - out[:, 2])
  out[:, 5] = np.clip(r[:, 5], 1, out[:, 1] - out[:, 3])
  out[:, 6] = r[:, 6] != 0
  return out.astype(np.int32)


METHODS = ('bilinear', 'bicubic')


def mean_std_array(norm):
  """norm = (mean [3], std [3]) -> the six host floats edet_crop_resize_bicubic / edet_randaug_apply_norm read at the call
  (a ctypes array; None stays None)."""
  if norm is None:
    return None
  mean, std = (np.asarray(v, np.float32).reshape(-1) for v in norm)
  if mean.shape != (3,) or std.shape != (3,) or not np.isfinite(mean).all() or not np.isfinite(std).all() or (std == 0).any():
    raise ValueError('norm must be (mean [3], std [3]) of finite floats with no std 0, got %r' % (norm,))
  return (ctypes.c_float * 6)(*[float(v) for v in np.concatenate([mean, std])])


def launch(raw, rows_dev, out, stream, method='bilinear', norm=None):
  """edet_crop_resize (method 'bilinear') or edet_crop_resize_bicubic ('bicubic', with norm = (mean, std) or None) on device
  tensors: raw uint8 [B, Hc, Wc, 3], rows int32 [B, 8], out [B, h, w, 3] uint8 / fp32 / bf16."""
  b, hc, wc = int(raw.shape[0]), int(raw.shape[1]), int(raw.shape[2])
  if method not in METHODS:
    raise ValueError('method %r: one of %s' % (method, ', '.join(METHODS)))
  if method == 'bicubic':
    call('edet_crop_resize_bicubic', ptr(raw), b, hc, wc, ptr(rows_dev), ptr(out), int(out.shape[1]), int(out.shape[2]),
         _OUT[out.dtype][0], mean_std_array(norm), stream, nbytes=out.numel() * out.element_size())
    return out
  if norm is not None:
    raise ValueError("norm needs method='bicubic': the bilinear kernel's float output is (v - 128) / 128")
  # (nbytes: the bytes written; the bytes read are the crop areas, which only the device knows)
  call('edet_crop_resize', ptr(raw), b, hc, wc, ptr(rows_dev), ptr(out), int(out.shape[1]), int(out.shape[2]),
       _OUT[out.dtype][0], stream, nbytes=out.numel() * out.element_size())
  return out


def crop_resize(raw, rows, out_size, out_dtype=None, out=None, stream=None, method='bilinear', norm=None):
  """Crop, resize and flip a canvas batch on the device: raw uint8 [B, Hc, Wc, 3] (numpy or torch), rows [B, 8] (train_rows /
  eval_rows; a device tensor is used as it is) -> [B, out_h, out_w, 3], uint8 (clipped and truncated, RandAugment's input)
  or, with out_dtype torch.float32 / torch.bfloat16, the normalised network input (v - 128) / 128.  out_size: an int or
  (out_h, out_w).  method='bicubic': the legacy pipeline's tf.image.resize_bicubic (edet_crop_resize_bicubic); its float
  output is (v - mean[c]) / std[c] for norm = (mean [3], std [3]), or the resized values as they are for norm=None."""
  if method not in METHODS:
    raise ValueError('method %r: one of %s' % (method, ', '.join(METHODS)))
  if norm is not None and method != 'bicubic':
    raise ValueError("norm needs method='bicubic': the bilinear kernel's float output is (v - 128) / 128")
  mean_std_array(norm)
  if out_dtype not in _OUT:
    raise ValueError('out_dtype %r: None / torch.uint8, torch.float32 or torch.bfloat16' % (out_dtype,))
  x = torch.from_numpy(raw) if isinstance(raw, np.ndarray) else raw
  if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
    raise ValueError('raw must be uint8 [batch, canvas_h, canvas_w, 3], got %s %s' % (x.dtype, tuple(x.shape)))
  x = x.to('cuda').contiguous()
  b = int(x.shape[0])
  oh, ow = (int(out_size), int(out_size)) if np.isscalar(out_size) else (int(out_size[0]), int(out_size[1]))
  if isinstance(rows, torch.Tensor) and rows.is_cuda:
    r = rows
    if r.dtype != torch.int32 or not r.is_contiguous():
      raise ValueError('device rows must be contiguous int32')
  else:
    r = torch.from_numpy(np.ascontiguousarray(np.asarray(rows), dtype=np.int32)).to(x.device)
  if tuple(r.shape) != (b, 8):
    raise ValueError('rows are %s, want [batch, 8] = %s' % (tuple(r.shape), (b, 8)))
  if out is None:
    out = torch.empty((b, oh, ow, 3), dtype=_OUT[out_dtype][1], device=x.device)
  elif tuple(out.shape) != (b, oh, ow, 3) or not out.is_contiguous() or out.dtype not in _OUT:
    raise ValueError('out must be a contiguous [%d, %d, %d, 3] uint8 / float32 / bfloat16 tensor' % (b, oh, ow))
  return launch(x, r, out, torch.cuda.current_stream().cuda_stream if stream is None else stream, method, norm)
