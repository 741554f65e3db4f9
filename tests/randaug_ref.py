"""numpy restatement of the reference's RandAugment operations (efficientnetv2/autoaugment.py:79-441, :471-524, :663-702),
one uint8 image [H, W, 3] at a time, with the arithmetic that csrc/randaug.hip documents: every product and sum a single
float32 operation in the stated order, every float -> uint8 conversion a truncation after the stated clip.
tests/test_randaug.py pins it to the executed reference (tests/golden/reference_randaug.npz) and compares the kernels with it
bit for bit."""
import math

import numpy as np

F = np.float32
OPS = ('AutoContrast', 'Equalize', 'Invert', 'Rotate', 'Posterize', 'Solarize', 'Color', 'Contrast', 'Brightness',
       'Sharpness', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Cutout', 'SolarizeAdd')
SIGNED = ('Rotate', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY')
REPLACE = 128


def to_u8(t):
  """clip to [0, 255], truncate."""
  return np.clip(t, F(0), F(255)).astype(np.uint8)


def blend(a, b, factor):
  """:79-119; factor is the Python double, its float32 value multiplies."""
  if factor == 0.0:
    return a.copy()
  if factor == 1.0:
    return b.copy()
  fa, fb = a.astype(F), b.astype(F)
  t = fa + F(factor) * (fb - fa)
  return t.astype(np.uint8) if 0.0 < factor < 1.0 else to_u8(t)


def grayscale(img):
  """tf.image.rgb_to_grayscale on uint8 -> [H, W]."""
  k = F(1.0) / F(255.0)
  x = img.astype(F) * k
  s = (x[..., 0] * F(0.2989) + x[..., 1] * F(0.5870)) + x[..., 2] * F(0.1140)
  return to_u8(s * F(255.5))


def color(img, factor):
  g = grayscale(img)
  return blend(np.stack([g, g, g], -1), img, factor)


def contrast(img, factor):
  """:196-210 as written: the 'mean' is the pixel count / 256."""
  h, w = img.shape[:2]
  mean = F(h * w) / F(256.0)
  deg = np.full(img.shape, to_u8(np.array(mean, F)), np.uint8)
  return blend(deg, img, factor)


def brightness(img, factor):
  return blend(np.zeros_like(img), img, factor)


def sharpness(img, factor):
  h, w = img.shape[:2]
  deg = img.copy()
  if h > 2 and w > 2:
    x = img.astype(F)
    w1, w5 = F(1.0) / F(13.0), F(5.0) / F(13.0)
    acc = np.zeros((h - 2, w - 2, 3), F)
    for dy in range(3):
      for dx in range(3):
        acc = acc + (w5 if (dy, dx) == (1, 1) else w1) * x[dy:dy + h - 2, dx:dx + w - 2]
    deg[1:-1, 1:-1] = to_u8(acc)
  return blend(deg, img, factor)


def autocontrast(img):
  out = img.copy()
  for c in range(3):
    ch = img[..., c]
    lo, hi = F(ch.min()), F(ch.max())
    if hi > lo:
      scale = F(255.0) / (hi - lo)
      offset = -lo * scale
      out[..., c] = to_u8(ch.astype(F) * scale + offset)
  return out


def equalize(img):
  out = img.copy()
  for c in range(3):
    ch = img[..., c]
    histo = np.bincount(ch.reshape(-1), minlength=256).astype(np.int64)
    nz = histo[histo != 0]
    step = int(nz.sum() - nz[-1]) // 255
    if step == 0:
      continue
    lut = (np.cumsum(histo) + step // 2) // step
    lut = np.clip(np.concatenate([[0], lut[:-1]]), 0, 255)
    out[..., c] = lut[ch].astype(np.uint8)
  return out


def invert(img):
  return (255 - img.astype(np.int32)).astype(np.uint8)


def posterize(img, bits):
  s = 8 - int(bits)
  return (((img.astype(np.int32) >> s) << s) & 255).astype(np.uint8)


def solarize(img, threshold):
  v = img.astype(np.int32)
  return np.where(v < int(threshold), v, 255 - v).astype(np.uint8)


def solarize_add(img, addition, threshold=128):
  v = img.astype(np.int32)
  return np.where(v < threshold, np.clip(v + int(addition), 0, 255), v).astype(np.uint8)


def cutout(img, pad, cy, cx):
  h, w = img.shape[:2]
  out = img.copy()
  out[max(0, cy - pad):min(h, cy + pad), max(0, cx - pad):min(w, cx + pad)] = REPLACE
  return out


def round_away(t):
  """roundf: to the nearest integer, halves away from zero (t - trunc(t) is exact)."""
  r = np.trunc(t)
  return r + np.sign(t) * (np.abs(t - r) >= F(0.5))


def project(img, coef):
  """Nearest-neighbour projective transform with coefficients float32 [a0, a1, a2, b0, b1, b2]; 128 outside."""
  h, w = img.shape[:2]
  a0, a1, a2, b0, b1, b2 = (F(v) for v in coef)
  y, x = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing='ij')
  sx = round_away((a0 * x + a1 * y) + a2)
  sy = round_away((b0 * x + b1 * y) + b2)
  inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
  ix = np.where(inside, sx, 0).astype(np.int64)
  iy = np.where(inside, sy, 0).astype(np.int64)
  return np.where(inside[..., None], img[iy, ix], np.uint8(REPLACE)).astype(np.uint8)


def rotate_coef(degrees, h, w):
  angle = F(degrees * (math.pi / 180.0))
  c, s = np.cos(angle), np.sin(angle)
  wm, hm = F(w - 1), F(h - 1)
  return [c, -s, (wm - (c * wm - s * hm)) / F(2), s, c, (hm - (s * wm + c * hm)) / F(2)]


def rotate(img, degrees):
  return project(img, rotate_coef(degrees, *img.shape[:2]))


def shear_x(img, level):
  return project(img, [1, level, 0, 0, 1, 0])


def shear_y(img, level):
  return project(img, [1, 0, 0, level, 1, 0])


def translate_x(img, pixels):
  return project(img, [1, 0, pixels, 0, 1, 0])


def translate_y(img, pixels):
  return project(img, [1, 0, 0, 0, 1, pixels])


def level_to_arg(name, level, translate_const=100, cutout_const=40):
  """:471-524 before the random negation (the restatement's own copy; the package's is automl_amd.autoaugment's)."""
  r = level / 10.
  if name in ('AutoContrast', 'Equalize', 'Invert'):
    return ()
  return {'Rotate': lambda: (r * 30.,), 'Posterize': lambda: (int(r * 4),), 'Solarize': lambda: (int(r * 256),),
          'SolarizeAdd': lambda: (int(r * 110),), 'Color': lambda: (r * 1.8 + 0.1,), 'Contrast': lambda: (r * 1.8 + 0.1,),
          'Brightness': lambda: (r * 1.8 + 0.1,), 'Sharpness': lambda: (r * 1.8 + 0.1,), 'ShearX': lambda: (r * 0.3,),
          'ShearY': lambda: (r * 0.3,), 'Cutout': lambda: (int(r * cutout_const),),
          'TranslateX': lambda: (r * float(translate_const),), 'TranslateY': lambda: (r * float(translate_const),)}[name]()


FUNCS = {'AutoContrast': autocontrast, 'Equalize': equalize, 'Invert': invert, 'Rotate': rotate, 'Posterize': posterize,
         'Solarize': solarize, 'SolarizeAdd': solarize_add, 'Color': color, 'Contrast': contrast, 'Brightness': brightness,
         'Sharpness': sharpness, 'ShearX': shear_x, 'ShearY': shear_y, 'TranslateX': translate_x, 'TranslateY': translate_y}


def apply_op(img, op, magnitude, sign=1.0, cy=0, cx=0):
  """Operation id `op` (16 or anything outside [0, 16) = identity) at `magnitude`; sign: +1 / -1 for the signed ones;
  (cy, cx): Cutout's centre."""
  if not 0 <= int(op) < len(OPS):
    return img.copy()
  name = OPS[int(op)]
  args = level_to_arg(name, float(magnitude))
  if name == 'Cutout':
    return cutout(img, args[0], int(cy), int(cx))
  if name in SIGNED:
    args = (float(sign) * args[0],)
  return FUNCS[name](img, *args)


def randaugment(images, draws, magnitude):
  """A batch [B, H, W, 3] through the layers of `draws` = (op, sign, cy_u, cx_u), each [L, B] (autoaugment.randaug_draws)."""
  op, sign, cy_u, cx_u = (np.asarray(d) for d in draws)
  out = np.array(images, dtype=np.uint8, copy=True)
  h, w = out.shape[1:3]
  for k in range(op.shape[0]):
    for i in range(out.shape[0]):
      cy, cx = min(int(cy_u[k, i] * h), h - 1), min(int(cx_u[k, i] * w), w - 1)
      out[i] = apply_op(out[i], op[k, i], magnitude, sign[k, i], cy, cx)
  return out


def normalise(images_u8):
  """preprocessing.py:153: (x - 128) / 128, float32 (exact)."""
  return (images_u8.astype(F) - F(128)) / F(128)
