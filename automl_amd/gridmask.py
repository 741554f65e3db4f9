"""GridMask on the device: the reference's ``efficientdet/aug/gridmask.py`` for a whole uint8 batch.

Mirror of the reference module's public names: ``GridMask(prob, ratio, rotate, gridmask_size_ratio, fill)`` called on
``(images, boxes)`` and ``gridmask(images, boxes, ...)`` (:22-136); the boxes come back untouched, as there.  The draws are
made on the host (``gridmask_draws``), turned into the kernel's per-image rows (``gridmask_args``: ``edet_gridmask_image_t``)
and applied by ``edet_gridmask`` (csrc/gridmask.hip), which evaluates the rotated mask per output pixel and never stores it.
The numpy restatement the kernel is compared with bit for bit is tests/gridmask_ref.py; it materialises the mask as the
reference does.

A canvas batch (``sizes=``, what ``jpeg.JpegDecoder.decode`` returns next to the images): image ``i`` is the top-left
``sizes[i]`` of its slot and is masked as that image alone would be -- its own mask side, block range and crop corner
(``edet_gridmask_canvas``).  The kernel writes inside the rectangles only.

As the reference is written, and kept: ``fill=1`` marks what is KEPT (:100, :117), so the image survives on the cross-hatch
of stripes and is zeroed in the square holes between them; the occurrence draw is a NORMAL one, ``N(0, 1) < prob`` (:116),
so ``prob=0.5`` masks about 69 % of the images; the angle is ``rotate * N(-1, 1)`` degrees (:53).

Not pinned against TensorFlow (neither it nor TensorFlow Addons runs here): the rounding of the int32 bilinear blend and its
truncation, the coefficient formulas (``autoaugment.angle_coefficients``), float32 sin / cos (numpy's), and the random streams
of ``tf.random.uniform`` / ``tf.random.normal`` (a numpy PCG64 generator stands in).

Not built, and raising rather than ignored: ``fill != 1``, ``ratio == 1`` (a drawn length, :82-84) and any interpolation
other than ``BILINEAR``.
"""
import numpy as np
import torch

from automl_amd import autoaugment
from automl_amd import utils
from automl_amd._lib import call, ptr

F = np.float32
# edet_gridmask_image_t (include/edet_hip.h)
ARGS_DTYPE = np.dtype([('apply', np.int32), ('size', np.int32), ('d', np.int32), ('l', np.int32), ('s1', np.int32),
                       ('s2', np.int32), ('coef', np.float32, (6,))])
ARGS_BYTES = ARGS_DTYPE.itemsize      # 48


def check_options(ratio=0.6, fill=1, interpolation='BILINEAR'):
  """What is built, or a ValueError that names what the reference would have run."""
  if fill != 1:
    raise ValueError('GridMask fill=%r is not built (gridmask.py:99-101 scatters the fill value into an int32 mask that '
                     'multiplies the image, :117); only fill=1 is' % (fill,))
  if ratio == 1:
    raise ValueError('GridMask ratio=1 is not built (gridmask.py:82-84 draws the stripe length instead of deriving it)')
  if str(interpolation).upper() != 'BILINEAR':
    raise ValueError('GridMask interpolation=%r is not built (gridmask.py:55); only BILINEAR is' % (interpolation,))


def mask_side(h, w, gridmask_size_ratio=0.5):
  """S (gridmask.py:70-73): int(float32(ratio + 1) * max(float32 h, float32 w))."""
  return int(F(F(gridmask_size_ratio + 1) * max(F(h), F(w))))


def block_range(h, w, image=None):
  """The ends of gridblock's range, both included (gridmask.py:76-80).  image: its index in a canvas batch, for the message."""
  a, b = F(F(h) * F(0.5)), F(F(w) * F(0.3))
  lo, hi = int(min(a, b)), int(max(a, b))
  if lo < 1:
    raise ValueError('GridMask on %s %d x %d image: int(min(H / 2, 0.3 W)) = %d < 1, the reference would divide by a zero '
                     'gridblock (gridmask.py:76-80, :95)' % ('a' if image is None else 'image %d, a' % image, h, w, lo))
  return lo, hi


def _per_image(h, w, batch):
  """h, w as gridmask_draws / gridmask_args take them -> None for two numbers (the dense batch), else two int arrays [batch]."""
  if np.ndim(h) == 0 and np.ndim(w) == 0:
    return None
  return np.broadcast_to(np.asarray(h), (batch,)), np.broadcast_to(np.asarray(w), (batch,))


def stripe_length(d, ratio=0.6):
  """gridmask.py:86-90: min(max(int(float32(d) * ratio + 0.5), 1), d - 1)."""
  return min(max(int(F(F(F(d) * F(ratio)) + F(0.5))), 1), int(d) - 1)


def gridmask_rng(seed):
  """The generator behind the GridMask draws of a model built with `seed`."""
  return np.random.Generator(np.random.PCG64([int(seed), 0x67726964]))


def gridmask_draws(rng, batch, h, w):
  """Per image -> (d, s1, s2 int32; z1 ~ N(-1, 1), z2 ~ N(0, 1) float32), each [batch], from a numpy PCG64 generator:
  gridblock uniform in block_range (:76-80), the two stripe starts uniform in [0, d] (:93-94, the first lands on rows),
  the angle's normal (:53) and the occurrence's (:116).  h, w: two numbers, or arrays [batch] for a canvas batch -- then
  gridblock is drawn over each image's own range, in ONE call of rng.integers with the bounds as arrays: a stream of its own,
  not promised equal to the dense one even where every size is the same.  Every range is checked before the generator moves."""
  b = int(batch)
  sizes = _per_image(h, w, b)
  if sizes is None:
    lo, hi = block_range(h, w)
    d = rng.integers(lo, hi + 1, size=b).astype(np.int32)
  else:
    bounds = np.array([block_range(int(sizes[0][i]), int(sizes[1][i]), image=i) for i in range(b)], np.int64).reshape(b, 2)
    d = rng.integers(bounds[:, 0], bounds[:, 1] + 1).astype(np.int32)
  s1 = rng.integers(0, d + 1).astype(np.int32)
  s2 = rng.integers(0, d + 1).astype(np.int32)
  z1 = (rng.standard_normal(b) - 1.0).astype(np.float32)
  z2 = rng.standard_normal(b).astype(np.float32)
  return d, s1, s2, z1, z2


def gridmask_args(draws, h, w, prob=0.5, ratio=0.6, rotate=10, gridmask_size_ratio=0.5):
  """draws of gridmask_draws -> the kernel's rows, a numpy array [batch] of ARGS_DTYPE.  The reference's TensorFlow
  expressions in numpy float32, statement by statement.  h, w: two numbers, or arrays [batch] for a canvas batch: row i is
  then the row of image i alone at its own size."""
  check_options(ratio=ratio)
  d, s1, s2, z1, z2 = (np.asarray(v) for v in draws)
  if not (d.ndim == 1 and d.shape == s1.shape == s2.shape == z1.shape == z2.shape):
    raise ValueError('draws must be five arrays [batch], got shapes %s' % ([np.shape(v) for v in draws],))
  sizes = _per_image(h, w, d.shape[0])
  if sizes is None:
    block_range(h, w)
    sides = [mask_side(h, w, gridmask_size_ratio)] * d.shape[0]
  else:
    for i in range(d.shape[0]):
      block_range(int(sizes[0][i]), int(sizes[1][i]), image=i)
    sides = [mask_side(int(sizes[0][i]), int(sizes[1][i]), gridmask_size_ratio) for i in range(d.shape[0])]
  rows = np.zeros(d.shape[0], ARGS_DTYPE)
  for i in range(d.shape[0]):
    side = sides[i]
    angle = F(rotate) * F(z1[i])                      # self.rotate * tf.random.normal([], -1, 1)
    angle = F(F(F(np.pi) * angle) / F(180))           # math.pi * angle / 180
    rows[i] = (int(F(z2[i]) < F(prob)), side, int(d[i]), stripe_length(int(d[i]), ratio) if int(d[i]) >= 1 else 0,
               int(s1[i]), int(s2[i]), autoaugment.angle_coefficients(angle, side, side))
  return rows


def args_tensor(rows, pin=False):
  """rows of gridmask_args -> a uint8 host tensor [batch, 48] (pinned for an asynchronous copy)."""
  rows = np.ascontiguousarray(rows, dtype=ARGS_DTYPE)
  t = torch.from_numpy(rows.view(np.uint8).reshape(rows.shape[0], ARGS_BYTES))
  return t.pin_memory() if pin else t


def apply_mask(src, out, rows_dev, stream, sizes=None):
  """The launch on device tensors: src uint8 [B, H, W, 3] -> out (another buffer like it); rows_dev uint8 [B, 48].  sizes:
  int32 [B, 2] on the device for a canvas batch -- out is then written inside each image's rectangle only."""
  b, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
  if sizes is None:
    call('edet_gridmask', ptr(src), ptr(out), b, h, w, ptr(rows_dev), stream, nbytes=2 * src.numel())
  else:
    call('edet_gridmask_canvas', ptr(src), ptr(out), b, h, w, ptr(sizes), ptr(rows_dev), stream, nbytes=2 * src.numel())
  return out


def _check_images(images):
  x = torch.from_numpy(images) if isinstance(images, np.ndarray) else images
  if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
    raise ValueError('images must be uint8 [batch, height, width, 3], got %s %s'
                     % (getattr(x, 'dtype', type(x)), tuple(getattr(x, 'shape', ()))))
  return x


class GridMask(object):
  """GridMask class for grid masking augmentation (gridmask.py:22-118), for a batch."""

  def __init__(self, prob=0.6, ratio=0.6, rotate=10, gridmask_size_ratio=0.5, fill=1, interpolation='BILINEAR'):
    check_options(ratio, fill, interpolation)
    self.prob = prob
    self.ratio = ratio
    self.rotate = rotate
    self.gridmask_size_ratio = gridmask_size_ratio
    self.fill = fill
    self.interpolation = interpolation

  def __call__(self, images, label, rng=None, draws=None, sizes=None):
    """images uint8 [B, H, W, 3] (numpy or torch) -> (the masked batch as a device tensor, label as it came).  draws:
    gridmask_draws' arrays, else drawn from `rng` (a numpy Generator; default: a fresh one).  sizes: [B, 2] (height, width)
    of each image on the canvas [H, W] -- host data (utils.canvas_sizes; a device tensor is copied to the host, which waits
    for the device); the result is zero outside the images' rectangles.  Every size is checked before the generator moves."""
    x = _check_images(images)
    b, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    if sizes is not None:
      sizes = utils.canvas_sizes(sizes, b, h, w)
      h, w = sizes[:, 0], sizes[:, 1]
      for i in range(b):
        block_range(int(h[i]), int(w[i]), image=i)
    else:
      block_range(h, w)
    if draws is None:
      draws = gridmask_draws(rng if rng is not None else np.random.default_rng(), b, h, w)
    if np.asarray(draws[0]).shape != (b,):
      raise ValueError('draws are %s, want [batch] = %s' % (np.asarray(draws[0]).shape, (b,)))
    rows = gridmask_args(draws, h, w, self.prob, self.ratio, self.rotate, self.gridmask_size_ratio)
    x = x.to('cuda').contiguous()
    out = torch.empty_like(x) if sizes is None else torch.zeros_like(x)
    apply_mask(x, out, args_tensor(rows).to(x.device), torch.cuda.current_stream().cuda_stream,
               None if sizes is None else torch.from_numpy(sizes).to(x.device))
    return out, label


def gridmask(images, boxes, prob=0.5, ratio=0.6, rotate=10, gridmask_size_ratio=0.5, fill=1, rng=None, draws=None, sizes=None):
  """Callable instance of GridMask and transforms input image (gridmask.py:121-136).  sizes: GridMask.__call__'s."""
  gridmask_obj = GridMask(prob=prob, ratio=ratio, rotate=rotate, gridmask_size_ratio=gridmask_size_ratio, fill=fill)
  return gridmask_obj(images, boxes, rng=rng, draws=draws, sizes=sizes)
