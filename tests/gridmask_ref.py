"""numpy restatement of the reference's aug/gridmask.py that does what the reference does LITERALLY: the S x S int32 mask
by two scatter-and-transpose passes, a generic float32 bilinear projective transform of it (fill 0, truncated), the centre
crop, the multiply.  edet_gridmask (automl_amd/csrc/gridmask.hip) evaluates the same mask per pixel without storing it and
is compared with this bit for bit (tests/test_gridmask.py), as is train_step_raw's first stage (tests/test_det_input.py)."""
import numpy as np

F = np.float32


def build_mask(side, d, l, s1, s2, fill=1):
  """gridmask.py:75, :92-104: rows [d i + start, min(d i + start + l, S)) for i < S // d set to `fill`, transposed; twice."""
  mask = np.zeros((side, side), np.int32)
  for start_w in (s1, s2):
    for i in range(side // d):
      start = d * i + start_w
      end = min(start + l, side)
      rows = np.arange(start, end)                     # (empty where start >= end: s = d with S % d == 0)
      updated = mask.copy()
      updated[rows] = np.ones((rows.shape[0], side), np.int32) * fill
      mask = updated
    mask = mask.T.copy()
  return mask


def projective_bilinear(image, coef):
  """ImageProjectiveTransformV2, BILINEAR, constant fill 0, for one int32 image [H, W] and the six affine coefficients:
  output (y, x) reads (c0 x + c1 y + c2, c3 x + c4 y + c5), float32 left to right; taps floor() and floor() + 1, 0 outside;
  (x_ceil - x) v00 + (x - x_floor) v01 per row, the same between the rows; truncated to the image's type.  A position that
  is not finite reads 0."""
  h, w = image.shape
  c = [F(v) for v in coef]
  ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing='ij')
  with np.errstate(all='ignore'):
    sx = (c[0] * xs + c[1] * ys) + c[2]
    sy = (c[3] * xs + c[4] * ys) + c[5]
    finite = np.isfinite(sx) & np.isfinite(sy)
    sx = np.where(finite, sx, F(-2))
    sy = np.where(finite, sy, F(-2))
    xf, yf = np.floor(sx), np.floor(sy)
    xc, yc = xf + F(1), yf + F(1)
    # (clipped for the integer conversion only: whatever is clipped lies outside the image either way)
    x0 = np.clip(xf, -2, w + 1).astype(np.int64)
    y0 = np.clip(yf, -2, h + 1).astype(np.int64)

    def read(yi, xi):
      ok = (yi >= 0) & (yi < h) & (xi >= 0) & (xi < w)
      return np.where(ok, image[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)], 0).astype(np.float32)

    top = (xc - sx) * read(y0, x0) + (sx - xf) * read(y0, x0 + 1)
    bot = (xc - sx) * read(y0 + 1, x0) + (sx - xf) * read(y0 + 1, x0 + 1)
    out = (yc - sy) * top + (sy - yf) * bot
  assert out.dtype == np.float32
  return np.where(finite, out, F(0)).astype(image.dtype)      # astype truncates


def rotate_coefficients(angle, side):
  """TFA angles_to_projective_transforms(angle, S, S) in float32 (numpy's sin / cos): written out here, independently of
  automl_amd.autoaugment."""
  a = F(angle)
  cos, sin = np.cos(a), np.sin(a)
  m = F(side) - F(1)
  xo = (m - (cos * m - sin * m)) / F(2.0)
  yo = (m - (sin * m + cos * m)) / F(2.0)
  return [cos, -sin, xo, sin, cos, yo]


def rotate(mask, angle):
  """tensorflow_addons.image.rotate(mask, angle, interpolation='BILINEAR') of a square int32 mask."""
  return projective_bilinear(mask, rotate_coefficients(angle, mask.shape[0]))


def crop(mask, h, w):
  """gridmask.py:58-63."""
  hh = ww = mask.shape[0]
  return mask[(hh - h) // 2:(hh - h) // 2 + h, (ww - w) // 2:(ww - w) // 2 + w]


def clamp_row(row):
  """The kernel's stated clamps of one edet_gridmask_image_t row -> (apply, S, d, l, s1, s2, coef)."""
  side = int(np.clip(int(row['size']), 0, 1 << 30))
  d = max(int(row['d']), 1)
  l = int(np.clip(int(row['l']), 0, d))
  s1, s2 = int(np.clip(int(row['s1']), 0, d)), int(np.clip(int(row['s2']), 0, d))
  return int(row['apply']) != 0, side, d, l, s1, s2, np.asarray(row['coef'], np.float32)


def image_mask(row, h, w):
  """The cropped [h, w] int32 mask of one row, by materialising."""
  _, side, d, l, s1, s2, coef = clamp_row(row)
  return crop(projective_bilinear(build_mask(side, d, l, s1, s2), coef), h, w)


def gridmask_batch(images, rows):
  """images uint8 [B, H, W, 3], rows [B] of gridmask.ARGS_DTYPE -> the masked batch (gridmask.py:106-118)."""
  images = np.asarray(images)
  out = images.copy()
  h, w = images.shape[1:3]
  for i in range(images.shape[0]):
    if int(rows[i]['apply']) != 0:
      mask = image_mask(rows[i], h, w).astype(images.dtype).reshape(h, w)
      out[i] = images[i] * mask[..., None]
  return out
