"""RandAugment on the device: the reference's ``efficientnetv2/autoaugment.py`` for a whole uint8 batch.

Mirror of the reference module's public names as far as they are built: ``level_to_arg`` (:471-524), ``distort_image``
(:705-723) with ``aug_name='randaug'`` = ``distort_image_with_randaugment`` (:663-702).  The draws are made on the host
(``randaug_draws``), turned into the kernels' argument arrays (``randaug_args``) and applied by ``edet_randaug_stats`` /
``edet_randaug_apply`` (csrc/randaug.hip), one pair of launches per layer, the operation chosen per image from device
memory.  The numpy restatement the kernels are compared with bit for bit is tests/randaug_ref.py.

As the reference is written, and kept: Contrast blends with the constant uint8(min(H W / 256, 255)) -- its "mean" is
``reduce_sum(hist) / 256`` (:205-206), the pixel count over 256, not the mean grey level.  Solarize compares in int32, so a
threshold >= 256 (``int(level / 10 * 256)`` for a magnitude >= 10, every named EfficientNetV2 model's) leaves the image as
it is; what TensorFlow's conversion of an out-of-range Python integer to uint8 would do is pinned by nothing here.  The
rounding of the geometric operations (nearest source pixel, halves away from zero) and their coefficient formulas follow
the documented TensorFlow Addons / ImageProjectiveTransformV2 behaviour; float32 sin / cos are numpy's.

Not built, and raising rather than ignored: AutoAugment v0 (``'autoaug'``), ``'ra_aa'``, the legacy ``effnetv1_*`` /
``ft*`` preprocessing names.
"""
import math

import numpy as np
import torch

from automl_amd import _lib
from automl_amd._lib import call, ptr

_MAX_LEVEL = 10.
AVAILABLE_OPS = ('AutoContrast', 'Equalize', 'Invert', 'Rotate', 'Posterize', 'Solarize', 'Color', 'Contrast', 'Brightness',
                 'Sharpness', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Cutout', 'SolarizeAdd')      # :683-686
OP_ID = {name: i for i, name in enumerate(AVAILABLE_OPS)}
IDENTITY = len(AVAILABLE_OPS)      # op id 16: a plain copy
SIGNED_OPS = ('Rotate', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY')      # _randomly_negate_tensor (:464-468)
MAX_MAGNITUDE = 20.0      # Posterize keeps int(M / 10 * 4) bits: above 20 its shift 8 - bits would be negative


def check_magnitude(magnitude):
  m = float(magnitude)
  if not 0.0 <= m <= MAX_MAGNITUDE:
    raise ValueError('RandAugment magnitude %r outside [0, %g] (Posterize shifts by 8 - int(M / 10 * 4), '
                     'autoaugment.py:219-222,510)' % (magnitude, MAX_MAGNITUDE))
  return m


def level_to_arg(op_name, magnitude, translate_const=100, cutout_const=40):
  """The reference's argument tuple of `op_name` at `magnitude` before the random negation (autoaugment.py:471-524;
  RandAugment's constants, :682): () / (degrees,) / (bits,) / (threshold,) / (addition,) / (factor,) / (shear level,) /
  (pixels,) / (pad_size,) in Python's own arithmetic (doubles and int())."""
  if op_name not in OP_ID:
    raise ValueError('unknown RandAugment operation %r (autoaugment.py:683-686 has %s)' % (op_name, ', '.join(AVAILABLE_OPS)))
  level = check_magnitude(magnitude)
  if op_name in ('AutoContrast', 'Equalize', 'Invert'):
    return ()
  if op_name == 'Rotate':
    return ((level / _MAX_LEVEL) * 30.,)
  if op_name == 'Posterize':
    return (int((level / _MAX_LEVEL) * 4),)
  if op_name == 'Solarize':
    return (int((level / _MAX_LEVEL) * 256),)
  if op_name == 'SolarizeAdd':
    return (int((level / _MAX_LEVEL) * 110),)
  if op_name in ('Color', 'Contrast', 'Brightness', 'Sharpness'):
    return ((level / _MAX_LEVEL) * 1.8 + 0.1,)
  if op_name in ('ShearX', 'ShearY'):
    return ((level / _MAX_LEVEL) * 0.3,)
  if op_name == 'Cutout':
    return (int((level / _MAX_LEVEL) * cutout_const),)
  return ((level / _MAX_LEVEL) * float(translate_const),)      # TranslateX / TranslateY


def randaug_rng(seed):
  """The generator behind the RandAugment draws of a model built with `seed`."""
  return np.random.Generator(np.random.PCG64([int(seed), 0x72616e64]))


def randaug_draws(rng, batch, num_layers):
  """Per layer and image -> (op int32 in [0, 16), sign float32 in {+1, -1}, cy_u, cx_u float64 in [0, 1)), each
  [num_layers, batch], from a numpy PCG64 generator.  sign is the _randomly_negate_tensor draw (+1 = kept), read by the five
  signed operations; (cy_u, cx_u) place Cutout's centre uniformly over [0, H) x [0, W): cy = int(cy_u H).  The `prob` draw of
  :694 is not made: RandAugment discards it."""
  shape = (int(num_layers), int(batch))
  op = rng.integers(0, len(AVAILABLE_OPS), size=shape).astype(np.int32)
  sign = np.where(rng.random(shape) >= 0.5, 1.0, -1.0).astype(np.float32)
  cy_u, cx_u = rng.random(shape), rng.random(shape)
  return op, sign, cy_u, cx_u


def identity_draws(batch, num_layers):
  """Draws that leave every image as it is (op id 16)."""
  shape = (int(num_layers), int(batch))
  return np.full(shape, IDENTITY, np.int32), np.ones(shape, np.float32), np.zeros(shape), np.zeros(shape)


def rotate_coefficients(degrees, h, w):
  """TFA rotate -> angles_to_projective_transforms in float32: [cos, -sin, xoff, sin, cos, yoff]."""
  return angle_coefficients(np.float32(degrees * (math.pi / 180.0)), h, w)


def angle_coefficients(angle, h, w):
  """angles_to_projective_transforms for a float32 angle in radians (gridmask.py forms its own angle, gridmask.py:53-54)."""
  f = np.float32
  angle = f(angle)
  c, s = np.cos(angle), np.sin(angle)
  wm, hm = f(w - 1), f(h - 1)
  xoff = (wm - (c * wm - s * hm)) / f(2.0)
  yoff = (hm - (s * wm + c * hm)) / f(2.0)
  return [c, -s, xoff, s, c, yoff]


def randaug_args(draws, magnitude, h, w, translate_const=100, cutout_const=40):
  """draws of randaug_draws -> (ops int32 [L, B], iargs int32 [L, B, 4], fargs float32 [L, B, 8]), what the kernels take
  (include/edet_hip.h): the six projective coefficients in numpy float32, the blend factor, Posterize's shift, the
  Solarize threshold / addition, Cutout's box."""
  m = check_magnitude(magnitude)
  op, sign, cy_u, cx_u = (np.asarray(d) for d in draws)
  if not (op.ndim == 2 and op.shape == sign.shape == cy_u.shape == cx_u.shape):
    raise ValueError('draws must be four arrays [num_layers, batch], got shapes %s' % ([np.shape(d) for d in draws],))
  arg = {name: level_to_arg(name, m, translate_const, cutout_const) for name in AVAILABLE_OPS}
  ops = op.astype(np.int32)
  iargs = np.zeros(op.shape + (4,), np.int32)
  fargs = np.zeros(op.shape + (8,), np.float32)
  fargs[..., 6] = 1.0
  f = np.float32
  for idx in np.ndindex(*op.shape):
    k = int(op[idx])
    if not 0 <= k < IDENTITY:
      ops[idx] = IDENTITY
      continue
    name = AVAILABLE_OPS[k]
    sg = float(sign[idx])
    if name == 'Rotate':
      fargs[idx][:6] = rotate_coefficients(sg * arg[name][0], h, w)
    elif name == 'ShearX':
      fargs[idx][:6] = [1, f(sg * arg[name][0]), 0, 0, 1, 0]
    elif name == 'ShearY':
      fargs[idx][:6] = [1, 0, 0, f(sg * arg[name][0]), 1, 0]
    elif name == 'TranslateX':      # translate by [-pixels, 0]: source x = x + pixels
      fargs[idx][:6] = [1, 0, f(sg * arg[name][0]), 0, 1, 0]
    elif name == 'TranslateY':
      fargs[idx][:6] = [1, 0, 0, 0, 1, f(sg * arg[name][0])]
    elif name == 'Posterize':
      iargs[idx][0] = 8 - arg[name][0]
    elif name == 'Solarize':
      iargs[idx][0] = arg[name][0]
    elif name == 'SolarizeAdd':
      iargs[idx][:2] = [arg[name][0], 128]
    elif name == 'Cutout':
      pad = arg[name][0]
      cy, cx = min(int(cy_u[idx] * h), h - 1), min(int(cx_u[idx] * w), w - 1)
      iargs[idx] = [max(0, cy - pad), max(0, cx - pad), min(h, cy + pad), min(w, cx + pad)]
    elif name in ('Color', 'Contrast', 'Brightness', 'Sharpness'):
      fargs[idx][6] = f(arg[name][0])
  return ops, iargs, fargs


UNBUILT = {
    'autoaug': 'AutoAugment v0 (autoaugment.py:33-65,633-660)',
    'ra_aa': "the random choice between AutoAugment and RandAugment (autoaugment.py:712-719)",
}


def check_aug_name(aug_name):
  """'randaug' or a ValueError that names what the reference would have run."""
  if aug_name == 'randaug':
    return aug_name
  name = str(aug_name)
  if name in UNBUILT:
    raise ValueError('aug_name %r is not built: %s; only \'randaug\' is' % (aug_name, UNBUILT[name]))
  if name.startswith('effnetv1_') or name.startswith('ft'):
    raise ValueError('aug_name %r is not built: the legacy / fine-tuning preprocessing (preprocessing.py:112-147); only '
                     '\'randaug\' is' % (aug_name,))
  raise ValueError('Invalid value for aug_name: %s (autoaugment.py:721)' % (aug_name,))


_OUT = {None: (_lib.EDET_U8, torch.uint8), torch.uint8: (_lib.EDET_U8, torch.uint8),
        torch.float32: (_lib.EDET_F32, torch.float32), torch.bfloat16: (_lib.EDET_BF16, torch.bfloat16)}


def apply_layers(src, out, ops, iargs, fargs, luts, scratch, stream):
  """The launches of `ops.shape[0]` RandAugment layers on device tensors: src uint8 [B, H, W, 3] -> out (uint8, or fp32 /
  bf16 = normalised by the last layer).  ops / iargs / fargs: device [L, B(, 4 / 8)]; luts uint8 [B, 3, 256]; scratch: two
  uint8 buffers like src for the layers in between (the kernels never run in place).  L = 0: the (normalising) copy."""
  b, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
  code = _OUT[out.dtype][0]
  layers = 0 if ops is None else int(ops.shape[0])
  if layers == 0:
    call('edet_randaug_apply', ptr(src), ptr(out), b, h, w, None, None, None, None, code, stream,
         nbytes=src.numel() * (1 + out.element_size()))
    return out
  cur = src
  for k in range(layers):
    last = k == layers - 1
    dst = out if last else scratch[k % 2]
    call('edet_randaug_stats', ptr(cur), b, h, w, ptr(ops[k]), ptr(luts), stream, nbytes=cur.numel())
    call('edet_randaug_apply', ptr(cur), ptr(dst), b, h, w, ptr(ops[k]), ptr(iargs[k]), ptr(fargs[k]), ptr(luts),
         code if last else _lib.EDET_U8, stream, nbytes=cur.numel() * (1 + dst.element_size()))
    cur = dst
  return out


def distort_image(images_u8, aug_name, ra_num_layers, ra_magnitude, rng=None, draws=None, out_dtype=None):
  """autoaugment.distort_image for a batch on the device: images_u8 uint8 [B, H, W, 3] (numpy or torch) -> the augmented
  batch as a device tensor, uint8, or with out_dtype torch.float32 / torch.bfloat16 the normalised network input
  (x - 128) / 128.  draws: randaug_draws' arrays, else drawn from `rng` (a numpy Generator; default: a fresh one)."""
  check_aug_name(aug_name)
  layers = int(ra_num_layers)
  if layers < 0:
    raise ValueError('ra_num_layers %r must be >= 0' % (ra_num_layers,))
  check_magnitude(ra_magnitude)
  if out_dtype not in _OUT:
    raise ValueError('out_dtype %r: None / torch.uint8, torch.float32 or torch.bfloat16' % (out_dtype,))
  x = torch.from_numpy(images_u8) if isinstance(images_u8, np.ndarray) else images_u8
  if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
    raise ValueError('images must be uint8 [batch, height, width, 3], got %s %s' % (x.dtype, tuple(x.shape)))
  x = x.to('cuda').contiguous()
  b, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
  if draws is None:
    draws = randaug_draws(rng if rng is not None else np.random.default_rng(), b, layers)
  if np.asarray(draws[0]).shape != (layers, b):
    raise ValueError('draws are %s, want [num_layers, batch] = %s' % (np.asarray(draws[0]).shape, (layers, b)))
  out = torch.empty(x.shape, dtype=_OUT[out_dtype][1], device=x.device)
  stream = torch.cuda.current_stream().cuda_stream
  if layers == 0:
    return apply_layers(x, out, None, None, None, None, None, stream)
  ops, iargs, fargs = (torch.from_numpy(a).to(x.device) for a in randaug_args(draws, ra_magnitude, h, w))
  luts = torch.zeros((b, 3, 256), dtype=torch.uint8, device=x.device)
  scratch = [torch.empty_like(x) for _ in range(min(layers - 1, 2))]
  return apply_layers(x, out, ops, iargs, fargs, luts, scratch, stream)
