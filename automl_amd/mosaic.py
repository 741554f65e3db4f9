"""Mosaic augmentation on the device: the reference's ``efficientdet/aug/mosaic.py`` and a batch form of this project's own.

``Mosaic`` is the reference's class (mosaic.py:23-251): four images, two divide points ``x`` (it splits the ROWS) and ``y``
(the COLUMNS) drawn in the middle half of the output, every image resized WHOLE with ``tf.image.resize`` (bilinear,
half-pixel centres, no antialiasing, float32) to one quadrant --

    image 0 -> x by y at the top left            image 2 -> x by (out1 - y) to its right
    image 1 -> (out0 - x) by y BELOW image 0     image 3 -> the rest

(the concatenations of :246-250; the reference's variable names ``topright`` / ``bottomleft`` say the opposite) -- and the
boxes ``[x1, y1, x2, y2]`` in pixels scaled by ``sub_w / src_w`` and ``sub_h / src_h`` and moved by their quadrant's offset
(:98-103, :153-217).  The pixels are moved by ``edet_mosaic`` (csrc/mosaic.hip) from decoded uint8 images on a common canvas;
the numpy restatement the kernel is compared with bit for bit is tests/mosaic_ref.py, and the reference's own output on the
torch stand-in is tests/golden/reference_mosaic.npz.

``mosaic_draws`` / ``mosaic_batch`` are THIS PROJECT'S packaging, not the reference's (its data loader never calls Mosaic):
``G`` mosaics from a raw batch in two launches, with boxes, classes and counts in the raw-batch convention of
``EfficientDetNetTrain.train_step_raw``, which takes the result as it is.

Not pinned against TensorFlow (it is not installed): its resize kernel's own float32 evaluation (see v2_preprocessing.py)
and its random stream -- the divide points come from a numpy Generator under the reference's bounds.

Out of scope: a switch in ``DetectionInput`` / the trainer (the caller composes ``mosaic_batch`` and ``train_step_raw``),
``n_images`` other than 4, float source images, and the network-level C ABI.
"""
import numpy as np
import torch

from automl_amd import _lib, utils
from automl_amd._lib import call, ptr

# edet_mosaic_t as 16 int32: the four source indices, the divide points, the sources' heights and widths, two reserved words
ROW_WORDS = 16
INDEX, X, Y, HEIGHT, WIDTH = slice(0, 4), 4, 5, slice(6, 10), slice(10, 14)
_OUT = {'u8': (_lib.EDET_U8, torch.uint8), 'f32': (_lib.EDET_F32, torch.float32),
        torch.uint8: (_lib.EDET_U8, torch.uint8), torch.float32: (_lib.EDET_F32, torch.float32)}
_FOUR = 'Currently Exact 4 Images are supported by Mosaic Aug.'      # mosaic.py:238


def _out_size(out_size):
  if np.isscalar(out_size) or len(out_size) != 2:
    raise ValueError('out_size %r: want (out0, out1) = (rows, columns)' % (out_size,))
  o0, o1 = int(out_size[0]), int(out_size[1])
  if o0 < 2 or o1 < 2:
    raise ValueError('out_size %r: a mosaic needs at least 2 rows and 2 columns' % (out_size,))
  return o0, o1


def divide_point_bounds(out_size=(680, 680), minimum_dim=25):
  """mosaic.py:60-84 -> ((x_lo, x_hi), (y_lo, y_hi)), the half-open ranges of the two draws: int(out * (min / 100)) and
  int(out * ((100 - min) / 100)) -- Python doubles truncated by the cast, as the reference forms them.  A range without a
  value (where tf.random.uniform raises) is a ValueError."""
  o0, o1 = _out_size(out_size)
  if not minimum_dim > 0:
    raise ValueError('Minimum Mosaic image dimension should be above 0')
  out = []
  for name, n in (('x', o0), ('y', o1)):
    lo, hi = int(n * (minimum_dim / 100)), int(n * ((100 - minimum_dim) / 100))
    if lo >= hi:
      raise ValueError('out_size %r with _minimum_mosaic_image_dim %r leaves no divide point %s: [%d, %d) is empty'
                       % ((o0, o1), minimum_dim, name, lo, hi))
    if lo < 1:
      raise ValueError('out_size %r with _minimum_mosaic_image_dim %r allows the divide point %s = %d: an empty sub-image'
                       % ((o0, o1), minimum_dim, name, lo))
    out.append((lo, hi))
  return tuple(out)


def mosaic_divide_points(rng, out_size=(680, 680), minimum_dim=25):
  """Mosaic._mosaic_divide_points on a numpy Generator -> (x, y): x is drawn first, then y, each uniform over the integers
  of divide_point_bounds."""
  (xl, xh), (yl, yh) = divide_point_bounds(out_size, minimum_dim)
  x = int(rng.integers(xl, xh))
  y = int(rng.integers(yl, yh))
  return x, y


def mosaic_draws(rng, groups, batch, out_size, minimum_dim=25):
  """The draws of `groups` mosaics over a batch of `batch` images -> (index int32 [G, 4], points int32 [G, 2] = (x, y)).

  Column 0 of index is arange(G) % batch, so that with G = batch every image is some mosaic's first; columns 1-3 are
  independent uniform draws over the batch (a mosaic may use an image more than once).  The order of the draws is the
  definition: ONE call rng.integers(0, batch, (G, 3)) -- mosaic by mosaic, columns 1, 2, 3 -- then rng.integers over x's
  bounds for all G mosaics, then over y's for all G.  The bounds are checked before the generator moves."""
  groups, batch = int(groups), int(batch)
  if groups < 1 or batch < 1:
    raise ValueError('mosaic_draws: groups %d, batch %d' % (groups, batch))
  (xl, xh), (yl, yh) = divide_point_bounds(out_size, minimum_dim)
  index = np.empty((groups, 4), np.int32)
  index[:, 0] = np.arange(groups) % batch
  index[:, 1:] = rng.integers(0, batch, (groups, 3))
  points = np.empty((groups, 2), np.int32)
  points[:, 0] = rng.integers(xl, xh, groups)
  points[:, 1] = rng.integers(yl, yh, groups)
  return index, points


def mosaic_rows(index, points, sizes):
  """index [G, 4], points [G, 2], sizes [B, 2] = (height, width) per image -> int32 [G, 16], edet_mosaic_t's words."""
  index, points, sizes = np.asarray(index), np.asarray(points), np.asarray(sizes)
  if index.ndim != 2 or index.shape[1] != 4 or points.shape != (index.shape[0], 2):
    raise ValueError('index must be [G, 4] and points [G, 2], got %s and %s' % (index.shape, points.shape))
  if index.min() < 0 or index.max() >= sizes.shape[0]:
    raise ValueError('index holds %d .. %d, the batch has %d images' % (index.min(), index.max(), sizes.shape[0]))
  rows = np.zeros((index.shape[0], ROW_WORDS), np.int32)
  rows[:, INDEX] = index
  rows[:, X], rows[:, Y] = points[:, 0], points[:, 1]
  rows[:, HEIGHT] = sizes[index, 0]
  rows[:, WIDTH] = sizes[index, 1]
  return rows


def clamp_rows(rows, batch, canvas_h, canvas_w, out_h, out_w):
  """What edet_mosaic makes of every field it reads from device memory: the indices into [0, batch - 1], heights into
  [1, canvas_h], widths into [1, canvas_w], x into [1, out_h - 1], y into [1, out_w - 1]; the reserved words 0 -> int32
  [G, 16].  (edet_mosaic_boxes reads the indices and the points, clamped the same.)"""
  r = np.array(rows, dtype=np.int64).reshape(-1, ROW_WORDS)
  out = np.zeros_like(r)
  out[:, INDEX] = np.clip(r[:, INDEX], 0, batch - 1)
  out[:, X] = np.clip(r[:, X], 1, out_h - 1)
  out[:, Y] = np.clip(r[:, Y], 1, out_w - 1)
  out[:, HEIGHT] = np.clip(r[:, HEIGHT], 1, canvas_h)
  out[:, WIDTH] = np.clip(r[:, WIDTH], 1, canvas_w)
  return out.astype(np.int32)


def launch(raw, rows_dev, out, stream):
  """edet_mosaic on device tensors: raw uint8 [B, Hc, Wc, 3], rows int32 [G, 16], out [G, out0, out1, 3] uint8 / float32."""
  call('edet_mosaic', ptr(raw), int(raw.shape[0]), int(raw.shape[1]), int(raw.shape[2]), ptr(rows_dev), int(out.shape[0]),
       ptr(out), int(out.shape[1]), int(out.shape[2]), _OUT[out.dtype][0], stream, nbytes=out.numel() * out.element_size())
  return out


def launch_boxes(boxes, classes, counts, rows_dev, out_size, boxes_out, classes_out, counts_out, stream):
  """edet_mosaic_boxes on device tensors: boxes float32 [B, M, 4], classes float32 [B, M], counts int32 [B], rows int32
  [G, 16] -> boxes_out [G, 4 M, 4], classes_out [G, 4 M], counts_out int32 [G]."""
  call('edet_mosaic_boxes', ptr(boxes), ptr(classes), ptr(counts), int(boxes.shape[0]), int(boxes.shape[1]), ptr(rows_dev),
       int(boxes_out.shape[0]), int(out_size[0]), int(out_size[1]), ptr(boxes_out), ptr(classes_out), ptr(counts_out), stream,
       nbytes=boxes_out.numel() * 4)


def _raw_and_sizes(raw_or_pair, what):
  """The images of a call -> (uint8 tensor [B, Hc, Wc, 3] on the device, sizes int32 numpy [B, 2] checked on the host)."""
  if isinstance(raw_or_pair, (tuple, list)) and len(raw_or_pair) == 2 and np.ndim(raw_or_pair[0]) == 4:
    raw, sizes = raw_or_pair
  else:
    raw, sizes = raw_or_pair, None
  x = torch.from_numpy(np.ascontiguousarray(raw)) if isinstance(raw, np.ndarray) else raw
  if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[-1] != 3:
    raise ValueError('%s: images must be [batch, height, width, 3], got %s' % (what, getattr(x, 'shape', type(x))))
  if x.dtype != torch.uint8:
    raise ValueError('%s: images must be uint8 (the decoded image is the kernel\'s source type), got %s' % (what, x.dtype))
  b, hc, wc = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
  if b < 1 or hc < 1 or wc < 1:
    raise ValueError('%s: empty images %s' % (what, tuple(x.shape)))
  sizes = np.tile(np.asarray([hc, wc], np.int32), (b, 1)) if sizes is None else utils.canvas_sizes(sizes, b, hc, wc)
  return x, sizes


def _rows_tensor(rows, device):
  return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(device)


def mosaic_images(raw_or_pair, index, points, out_size, out_dtype='f32', out=None, stream=None):
  """The image half alone: mosaics [G, out0, out1, 3] (float32: tf.image.resize's values as they are; uint8: clipped to
  [0, 255] and truncated) from a dense batch or a canvas pair, for index [G, 4] and points [G, 2] given."""
  if out_dtype not in _OUT:
    raise ValueError("out_dtype %r: 'u8' / torch.uint8 or 'f32' / torch.float32" % (out_dtype,))
  o0, o1 = _out_size(out_size)
  x, sizes = _raw_and_sizes(raw_or_pair, 'mosaic_images')
  rows = mosaic_rows(index, points, sizes)
  _check_points(rows, o0, o1)
  x = x.to('cuda').contiguous()
  if out is None:
    out = torch.empty((rows.shape[0], o0, o1, 3), dtype=_OUT[out_dtype][1], device=x.device)
  elif tuple(out.shape) != (rows.shape[0], o0, o1, 3) or not out.is_contiguous() or out.dtype not in _OUT:
    raise ValueError('out must be a contiguous [%d, %d, %d, 3] uint8 / float32 tensor' % (rows.shape[0], o0, o1))
  return launch(x, _rows_tensor(rows, x.device), out, torch.cuda.current_stream().cuda_stream if stream is None else stream)


def _check_points(rows, o0, o1):
  bad = np.flatnonzero((rows[:, X] < 1) | (rows[:, X] > o0 - 1) | (rows[:, Y] < 1) | (rows[:, Y] > o1 - 1))
  if bad.size:
    g = int(bad[0])
    raise ValueError('mosaic %d: divide points (%d, %d) leave an empty sub-image of the %d x %d output'
                     % (g, rows[g, X], rows[g, Y], o0, o1))


def mosaic_batch(raw_or_pair, boxes, classes, counts, out_size, draws=None, rng=None, out_dtype='u8', minimum_dim=25):
  """G mosaics of a raw batch in two launches, whatever G (THIS PROJECT'S batch form; module docstring).

  raw_or_pair: uint8 [B, H, W, 3], or the canvas pair (raw [B, Hc, Wc, 3], sizes [B, 2]); boxes float32 [B, M, 4]
  normalised (ymin, xmin, ymax, xmax) with padding rows -1, classes [B, M] float32 padded with -1, counts [B]: the raw-batch
  convention of EfficientDetNetTrain.train_step_raw.  draws = (index [G, 4], points [G, 2]) as mosaic_draws returns them,
  or None: mosaic_draws(rng, B, B, out_size, minimum_dim) -- one mosaic per image -- from the numpy Generator `rng`.
  -> (mosaics [G, out0, out1, 3] uint8 or float32, boxes [G, 4 M, 4], classes [G, 4 M], counts int32 [G]) on the device:
  directly a raw batch for train_step_raw (the caller sets max_instances_per_image to cover 4 M).

  The output rows are the valid rows of source 0, then 1, 2, 3, in their order, the rest -1; a source's rows at or past
  its count are never read into the result.  For a quadrant at offset (oy, ox) of size (qh, qw), in float32 and one
  rounded operation each: ymin' = (float(oy) + ymin * float(qh)) / float(out0), xmin' = (float(ox) + xmin * float(qw)) /
  float(out1), likewise for the maxima.  Nothing is clipped: a mosaic crops nothing.

  The function does not wait for the device.  sizes are host data, checked before the generator moves."""
  if out_dtype not in _OUT:
    raise ValueError("out_dtype %r: 'u8' / torch.uint8 or 'f32' / torch.float32" % (out_dtype,))
  o0, o1 = _out_size(out_size)
  x, sizes = _raw_and_sizes(raw_or_pair, 'mosaic_batch')
  b = int(x.shape[0])
  boxes, classes, counts = torch.as_tensor(boxes), torch.as_tensor(classes), torch.as_tensor(counts)
  if boxes.dim() != 3 or boxes.shape[0] != b or boxes.shape[2] != 4 or boxes.shape[1] < 1 or boxes.dtype != torch.float32:
    raise ValueError('boxes must be float32 [batch %d, max_boxes >= 1, 4], got %s %s' % (b, boxes.dtype, tuple(boxes.shape)))
  m = int(boxes.shape[1])
  if tuple(classes.shape) != (b, m) or tuple(counts.shape) != (b,):
    raise ValueError('classes must be [%d, %d] and counts [%d], got %s and %s' % (b, m, b, tuple(classes.shape),
                                                                                 tuple(counts.shape)))
  if draws is None:
    if rng is None:
      raise ValueError('mosaic_batch: give draws = (index, points) or a numpy Generator rng')
    draws = mosaic_draws(rng, b, b, (o0, o1), minimum_dim)
  rows = mosaic_rows(draws[0], draws[1], sizes)
  _check_points(rows, o0, o1)
  g = rows.shape[0]
  x = x.to('cuda').contiguous()
  dev = x.device
  boxes = boxes.to(dev).contiguous()
  classes = classes.to(device=dev, dtype=torch.float32).contiguous()
  counts = counts.to(device=dev, dtype=torch.int32).contiguous()
  rows_dev = _rows_tensor(rows, dev)
  stream = torch.cuda.current_stream().cuda_stream
  images = torch.empty((g, o0, o1, 3), dtype=_OUT[out_dtype][1], device=dev)
  boxes_out = torch.empty((g, 4 * m, 4), dtype=torch.float32, device=dev)
  classes_out = torch.empty((g, 4 * m), dtype=torch.float32, device=dev)
  counts_out = torch.empty((g,), dtype=torch.int32, device=dev)
  launch(x, rows_dev, images, stream)
  launch_boxes(boxes, classes, counts, rows_dev, (o0, o1), boxes_out, classes_out, counts_out, stream)
  return images, boxes_out, classes_out, counts_out


def _integer_boxes(boxes):
  b = np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes)
  if b.dtype.kind not in 'iu' or b.ndim != 2 or b.shape[1] != 4:
    raise ValueError('boxes must be integers [N, 4] = [x1, y1, x2, y2] in pixels, got %s %s (the reference\'s expression has '
                     'no defined result for float32 boxes times an int32 shape)' % (b.dtype, b.shape))
  return b


def scale_boxes(boxes, src_hw, sub_hw, offset_xy):
  """Mosaic._scale_box and the offsets of :171-217 for one image, in numpy: integer boxes [N, 4] = [x1, y1, x2, y2] in
  pixels of a src_h x src_w image resized to sub_h x sub_w -> float64 [N, 4].  An int32 product, then a true division (what
  TensorFlow makes of int32 * int32 / int32), then the quadrant's integer offset (ox on columns 0 and 2, oy on 1 and 3)."""
  b = _integer_boxes(boxes).astype(np.int32)
  (src_h, src_w), (sub_h, sub_w), (ox, oy) = src_hw, sub_hw, offset_xy
  mul = np.asarray([sub_w, sub_h, sub_w, sub_h], np.int32)
  div = np.asarray([src_w, src_h, src_w, src_h], np.int32)
  return (b * mul) / div + np.asarray([ox, oy, ox, oy], np.int64)


class Mosaic:
  """The reference's Mosaic (aug/mosaic.py:23-251) for four uint8 images, on the device.

  1. Mosaic sub images do not preserve the aspect ratio of the original images.
  2. ``__call__(images, boxes)`` returns (mosaic float32 [out0, out1, 3] on the device, a list of four float64 [N, 4]
     arrays); the divide points come from ``rng`` (a numpy Generator) or are given as ``divide_points=(x, y)``.
  """

  def __init__(self, out_size=(680, 680), n_images=4, _minimum_mosaic_image_dim=25):
    self._n_images = n_images
    self._out_size = out_size
    self._minimum_mosaic_image_dim = _minimum_mosaic_image_dim
    assert (_minimum_mosaic_image_dim > 0), 'Minimum Mosaic image dimension should be above 0'

  @property
  def n_images(self):
    return self._n_images

  @property
  def out_size(self):
    return self._out_size

  def mosaic_divide_points(self, rng):
    return mosaic_divide_points(rng, self._out_size, self._minimum_mosaic_image_dim)

  def __call__(self, images, boxes, rng=None, divide_points=None):
    """images: uint8 [4, h, w, 3] (numpy or torch), or a canvas pair (raw [4, Hc, Wc, 3], sizes [4, 2]); boxes: four integer
    arrays [N, 4] = [x1, y1, x2, y2] in pixels of their image (one array [4, N, 4] will do)."""
    pair = isinstance(images, (tuple, list)) and len(images) == 2 and np.ndim(images[0]) == 4
    first = images[0] if pair else images
    if (first.shape[0] if hasattr(first, 'shape') else len(first)) != 4 or len(boxes) != 4:
      raise ValueError(_FOUR)
    o0, o1 = _out_size(self._out_size)
    x, sizes = _raw_and_sizes(images, 'Mosaic')
    per_image = [_integer_boxes(b) for b in boxes]
    if divide_points is None:
      if rng is None:
        raise ValueError('Mosaic: give a numpy Generator rng or divide_points = (x, y)')
      divide_points = self.mosaic_divide_points(rng)
    px, py = int(divide_points[0]), int(divide_points[1])
    mosaic = mosaic_images((x, sizes), [[0, 1, 2, 3]], [[px, py]], (o0, o1), 'f32')[0]
    subs = ((px, py), (o0 - px, py), (px, o1 - py), (o0 - px, o1 - py))      # (height, width) of the four sub-images
    offsets = ((0, 0), (0, px), (py, 0), (py, px))                           # (ox, oy): image 1 lies below, image 2 to the right
    out = [scale_boxes(per_image[k], sizes[k], subs[k], offsets[k]) for k in range(4)]
    return mosaic, out
