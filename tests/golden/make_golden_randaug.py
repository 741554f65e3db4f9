"""Generates tests/golden/reference_randaug.npz by EXECUTING the reference's efficientnetv2/autoaugment.py -- unmodified --
on the torch-backed `tf` stand-in (mini_keras.build_tf + make_golden_labels.add_tensor_ops + the leaf operations below):
each of the 16 NAME_TO_FUNC operations through _parse_policy_info at magnitudes 0, 5, 10, 15, 20 (both signs where the
level is randomly negated) on three small images, and two distort_image_with_randaugment runs of two layers.

What the fixture pins is the reference's WIRING: level_to_arg, the branches of blend, the Contrast expression, the histogram /
look-up-table logic of AutoContrast and Equalize, wrap / unwrap, the argument and operation order.  The leaf arithmetic is this
script's own, written independently of tests/randaug_ref.py from the documented TensorFlow behaviour:
  * tf.image.rgb_to_grayscale on uint8: convert_image_dtype to float32 (v * (1 / 255)), the weights [0.2989, 0.5870, 0.1140]
    summed left to right, convert_image_dtype back (saturate(v * 255.5), truncated);
  * tf.histogram_fixed_width: bin = clip(floor(nbins * (v - lo) / (hi - lo)), 0, nbins - 1) in float64;
  * tf.nn.depthwise_conv2d 'VALID': the taps accumulated in row-major order in float32 (TensorFlow's own order is not pinned);
  * tensorflow_addons.image rotate / translate / transform: angles_to_projective_transforms /
    translations_to_projective_transforms in float32 (numpy's float32 sin / cos), ImageProjectiveTransformV2 with nearest
    interpolation = the source pixel at (round(x), round(y)), halves away from zero, fill value 0.  Neither that rounding rule
    nor the float32 sin / cos can be pinned against TensorFlow binaries here;
  * `uint8 tensor < Python int` compares as integers (a Solarize threshold >= 256 selects every pixel); TensorFlow's own
    conversion of an out-of-range integer to uint8 is not pinned;
  * tf.random_uniform returns values queued by this script; the queues are stored with the outputs.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_randaug.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mini_keras   # noqa
from mini_keras import KT, ns   # noqa
from make_golden_labels import add_tensor_ops   # noqa

REF = '/root/reference/efficientnetv2'
QUEUE = []     # values in [0, 1) handed out by tf.random_uniform, in call order
MAGNITUDES = (0, 5, 10, 15, 20)
OPS = ('AutoContrast', 'Equalize', 'Invert', 'Rotate', 'Posterize', 'Solarize', 'Color', 'Contrast', 'Brightness',
       'Sharpness', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Cutout', 'SolarizeAdd')
SIGNED = ('Rotate', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY')


class RT(KT):
  """KT with TensorFlow's handling of Python lists and integers next to a uint8 tensor."""

  def __mul__(self, o):
    if isinstance(o, (list, tuple)):
      o = torch.as_tensor(o, dtype=self.dtype)
    return torch.Tensor.__mul__(self, o)

  def __rtruediv__(self, o):      # a true division (torch's own is reciprocal() * o: two roundings)
    return torch.true_divide(torch.as_tensor(o, dtype=self.dtype), self)

  def __lt__(self, o):
    if isinstance(o, int) and not self.is_floating_point():
      return torch.Tensor.__lt__(self.to(torch.int64), o)
    return torch.Tensor.__lt__(self, o)


def R(x, dtype=None):
  t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
  if dtype is not None:
    t = t.to(dtype)
  return t.as_subclass(RT)


def _int(v):
  return int(v)


def add_randaug_ops(tf):
  tf.uint8, tf.int32, tf.int64, tf.bool, tf.float32 = torch.uint8, torch.int32, torch.int64, torch.bool, torch.float32

  def random_uniform(shape=(), minval=0, maxval=None, dtype=torch.float32, **kw):
    u = QUEUE.pop(0)
    if dtype in (torch.int32, torch.int64):
      lo, hi = _int(minval), _int(maxval)
      return R(torch.tensor(min(lo + int(np.floor(u * (hi - lo))), hi - 1), dtype=dtype))
    hi = 1.0 if maxval is None else float(maxval)
    return R(torch.tensor(np.float32(minval) + np.float32(u) * (np.float32(hi) - np.float32(minval))))

  def pad(t, paddings, constant_values=0):
    t = R(t)
    pads = [(_int(a), _int(b)) for a, b in paddings]
    out = torch.full([s + a + b for s, (a, b) in zip(t.shape, pads)], constant_values, dtype=t.dtype)
    out[tuple(slice(a, a + s) for s, (a, b) in zip(t.shape, pads))] = t
    return R(out)

  def concat(xs, axis=0):
    dtype = next(x.dtype for x in xs if torch.is_tensor(x))
    return R(torch.cat([x if torch.is_tensor(x) else torch.as_tensor(x, dtype=dtype) for x in xs], dim=axis))

  def constant(v, dtype=None, shape=None):
    t = torch.as_tensor(v, dtype=dtype)
    return R(t.reshape(shape) if shape is not None else t)

  def histogram_fixed_width(values, value_range, nbins=100):
    lo, hi = float(value_range[0]), float(value_range[1])
    v = R(values).reshape(-1).to(torch.float64)
    idx = torch.clamp(torch.floor(nbins * ((v - lo) / (hi - lo))), 0, nbins - 1).long()
    return R(torch.bincount(idx, minlength=nbins).to(torch.int32))

  def depthwise_conv2d(x, kernel, strides, padding='VALID', rate=None):
    assert padding == 'VALID' and list(strides) == [1, 1, 1, 1]
    kh, kw = kernel.shape[:2]
    oh, ow = x.shape[1] - kh + 1, x.shape[2] - kw + 1
    acc = torch.zeros((x.shape[0], oh, ow, x.shape[3]), dtype=torch.float32)
    for i in range(kh):
      for j in range(kw):
        acc = acc + x[:, i:i + oh, j:j + ow, :] * kernel[i, j, :, 0]
    return R(acc)

  def rgb_to_grayscale(image):
    image = R(image)
    assert image.dtype == torch.uint8
    flt = image.to(torch.float32) * np.float32(1.0 / 255)
    g = flt[..., 0] * np.float32(0.2989)
    g = g + flt[..., 1] * np.float32(0.5870)
    g = g + flt[..., 2] * np.float32(0.1140)
    return R(torch.clamp(g * np.float32(255.5), 0, 255).to(torch.uint8).unsqueeze(-1))

  def clip_by_value(x, lo, hi):
    return torch.clamp(R(x), lo, hi)

  def zeros(shape, dtype=torch.float32):
    return R(torch.zeros([_int(s) for s in shape], dtype=dtype))

  def ones(shape, dtype=torch.float32):
    return R(torch.ones([_int(s) for s in shape], dtype=dtype))

  def slice_(t, begin, size):
    return t[tuple(slice(_int(b), _int(b) + _int(s)) for b, s in zip(begin, size))]

  tf.random_uniform = random_uniform
  tf.pad, tf.concat, tf.constant, tf.clip_by_value, tf.zeros, tf.ones, tf.slice = pad, concat, constant, clip_by_value, zeros, ones, slice_
  tf.histogram_fixed_width = histogram_fixed_width
  tf.nn.depthwise_conv2d = depthwise_conv2d
  tf.image = ns('image', rgb_to_grayscale=rgb_to_grayscale,
                grayscale_to_rgb=lambda g: R(torch.cat([g, g, g], dim=-1)))
  tf.cumsum = lambda x, axis=0: torch.cumsum(x, dim=axis)
  tf.reduce_min = lambda x: R(x).min()
  tf.reduce_max = lambda x, axis=None: R(x).max()
  tf.ones_like = lambda x, dtype=None: R(torch.ones_like(x, dtype=dtype))
  tf.zeros_like = lambda x, dtype=None: R(torch.zeros_like(x, dtype=dtype))
  tf.convert_to_tensor = lambda x, dtype=None: R(x)
  tf.floor = torch.floor
  tf.bitwise = ns('bitwise',
                  right_shift=lambda x, s: R((x.to(torch.int64) // (1 << _int(s))).to(x.dtype)),
                  left_shift=lambda x, s: R(((x.to(torch.int64) * (1 << _int(s))) % 256).to(x.dtype)))


def make_image_ops():
  """tensorflow_addons.image: rotate, translate, transform on one image [H, W, C], nearest interpolation, fill value 0."""
  f = np.float32

  def transform(images, transforms, **kw):
    c = [f(v) for v in transforms]
    h, w = images.shape[0], images.shape[1]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    proj = xs * c[6]
    proj = proj + ys * c[7]
    proj = proj + f(1)
    sx = xs * c[0]
    sx = sx + ys * c[1]
    sx = (sx + c[2]) / proj
    sy = xs * c[3]
    sy = sy + ys * c[4]
    sy = (sy + c[5]) / proj

    def rnd(t):      # std::round, in float64 (t + 0.5 is exact there)
      d = t.to(torch.float64)
      return (torch.sign(d) * torch.floor(d.abs() + 0.5)).long()
    ix, iy = rnd(sx), rnd(sy)
    ok = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    out = images[iy.clamp(0, h - 1), ix.clamp(0, w - 1)]
    return R(torch.where(ok.unsqueeze(-1), out, torch.zeros_like(out)))

  def rotate(images, angles, **kw):
    a = f(float(angles))
    cos, sin = np.cos(a), np.sin(a)
    h, w = f(images.shape[0]), f(images.shape[1])
    xo = ((w - f(1)) - (cos * (w - f(1)) - sin * (h - f(1)))) / f(2.0)
    yo = ((h - f(1)) - (sin * (w - f(1)) + cos * (h - f(1)))) / f(2.0)
    return transform(images, [cos, -sin, xo, sin, cos, yo, 0, 0])

  def translate(images, translations, **kw):
    dx, dy = f(float(translations[0])), f(float(translations[1]))
    return transform(images, [1, 0, -dx, 0, 1, -dy, 0, 0])

  return ns('image', transform=transform, rotate=rotate, translate=translate)


def images():
  rng = np.random.default_rng(20211)
  a = rng.integers(0, 256, (24, 20, 3)).astype(np.uint8)
  b = rng.integers(0, 256, (17, 31, 3)).astype(np.uint8)
  c = rng.integers(40, 200, (9, 7, 3)).astype(np.uint8)
  c[..., 1] = 77                       # a constant channel
  return {'a': a, 'b': b, 'c': c}


def ra_queue(ops, signs, centres):
  """The tf.random_uniform calls of distort_image_with_randaugment (autoaugment.py:688-701) in the order this stand-in's
  eager tf.cond makes them: per layer the operation, then per candidate its `prob`, its random negation where it has one,
  and -- inside the selected branch -- Cutout's centre."""
  q = []
  for op, sg, (uy, ux) in zip(ops, signs, centres):
    q.append((op + 0.5) / len(OPS))
    for i, name in enumerate(OPS):
      q.append(0.5)
      if name in SIGNED:
        q.append(0.75 if (i != op or sg > 0) else 0.25)
      if i == op and name == 'Cutout':
        q += [uy, ux]
  return q


def main():
  tf = mini_keras.build_tf()
  add_tensor_ops(tf)
  add_randaug_ops(tf)
  mini_keras.install(tf)
  sys.modules['tensorflow_addons'].image = make_image_ops()
  sys.modules.pop('hparams', None)
  sys.path.insert(0, REF)
  import autoaugment as ref_aa     # noqa: the reference module
  import hparams as ref_hparams    # noqa
  params = ref_hparams.Config(cutout_const=40, translate_const=100)      # distort_image_with_randaugment's (:682)
  out = {}
  imgs = images()
  for key, img in imgs.items():
    out['image/' + key] = img
  # per image: every case stacked into one array (neighbouring cases that agree then cost next to nothing in the archive)
  stacks, names = {k: [] for k in imgs}, {k: [] for k in imgs}
  for name in OPS:
    for m in MAGNITUDES:
      for sign in ((1, -1) if name in SIGNED else (1,)):
        for key, img in imgs.items():
          h, w = img.shape[:2]
          uy, ux = ((m + 3) % 7) / 7.0, ((m + 5) % 11) / 11.0        # Cutout's centre draws
          QUEUE[:] = ([0.75 if sign > 0 else 0.25] if name in SIGNED else []) + ([uy, ux] if name == 'Cutout' else [])
          func, _, args = ref_aa._parse_policy_info(name, 0.5, float(m), [128] * 3, params)
          res = func(R(torch.from_numpy(img.copy())), *args)
          assert not QUEUE, (name, QUEUE)
          res = res.numpy()
          assert res.dtype == np.uint8 and res.shape == img.shape, (name, res.dtype, res.shape)
          stacks[key].append(res)
          names[key].append('%s/m%d/%s' % (name, m, 'p' if sign > 0 else 'n'))
          if name == 'Cutout':
            out['centre/%s/m%d' % (key, m)] = np.asarray([int(uy * h), int(ux * w)], np.int32)
        if sign > 0:
          out['args/%s/m%d' % (name, m)] = np.asarray([float(a) for a in args if not isinstance(a, list)], np.float64)
  for key in imgs:
    out['cases/' + key] = np.stack(stacks[key])
    out['names/' + key] = np.asarray(names[key])
  runs = {'ra0': ('a', 15, [3, 14], [-1, 1], [(0, 0), (0.3, 0.9)]),
          'ra1': ('b', 10, [1, 10], [1, -1], [(0, 0), (0, 0)])}
  for rname, (key, m, ops, signs, centres) in runs.items():
    q = ra_queue(ops, signs, centres)
    QUEUE[:] = q
    res = ref_aa.distort_image_with_randaugment(R(torch.from_numpy(imgs[key].copy())), len(ops), m)
    assert not QUEUE, QUEUE
    out[rname + '/out'] = res.numpy().astype(np.uint8)
    out[rname + '/queue'] = np.asarray(q, np.float64)
    out[rname + '/magnitude'] = np.asarray(m, np.int32)
    out[rname + '/ops'] = np.asarray(ops, np.int32)
    out[rname + '/signs'] = np.asarray(signs, np.float32)
    out[rname + '/centre_u'] = np.asarray(centres, np.float64)
    out[rname + '/image'] = np.asarray(key)
    print(rname, ops, signs, int((res.numpy() != imgs[key]).sum()), 'bytes changed')
  path = os.path.join(HERE, 'reference_randaug.npz')
  np.savez_compressed(path, **out)
  print(path, len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
