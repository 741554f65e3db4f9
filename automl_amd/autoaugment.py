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

AutoAugment v0 (:33-76, :527-660) runs on the same kernels under names of its own: ``policy_v0`` / ``policy_vtest`` (the
tables as plain data), ``autoaug_draws`` (per image the sub-policy, then per position an apply draw and a sign draw -- both
always drawn, so the stream does not depend on the table: the project's definition, not TensorFlow's stream),
``autoaug_args`` (the table's own level per operation, translate_const 250 and cutout_const 100, an operation applied iff
floor(float32(u) + float32(prob)) >= 1, else the copy) and ``distort_image_with_autoaugment``: two layers of
``edet_randaug_stats`` + ``edet_randaug_apply``.  ``apply_layers(norm=(mean, std))`` ends in ``edet_randaug_apply_norm``, the
legacy pipeline's (x - mean) / std (automl_amd/preprocess_legacy.py).  Its restatement is tests/autoaug_ref.py.

Not built, and raising rather than ignored: ``'ra_aa'``, the ``ft*`` fine-tuning preprocessing, and -- through
``check_aug_name`` / ``distort_image`` / ``TrainableModel(augname=...)`` -- the spellings ``'autoaug'`` and ``effnetv1_*``:
those reach the legacy input pipeline, which is selected by ``TrainableModel(preprocessing='legacy', augment_name=...)`` and
``effnetv2_main --legacy_input``, not by ``augname``.
"""
import functools
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


def _fill_op(name, arg, sg, cy_u, cx_u, h, w, iarg, farg):
  """One operation at one level into one image's kernel arguments: `arg` = level_to_arg(name, level, ...), sg the random
  negation (+1 / -1), (cy_u, cx_u) Cutout's centre draws; iarg int32 [4] and farg float32 [8] are written in place.  The one
  filler behind randaug_args and autoaug_args."""
  f = np.float32
  if name == 'Rotate':
    farg[:6] = rotate_coefficients(sg * arg[0], h, w)
  elif name == 'ShearX':
    farg[:6] = [1, f(sg * arg[0]), 0, 0, 1, 0]
  elif name == 'ShearY':
    farg[:6] = [1, 0, 0, f(sg * arg[0]), 1, 0]
  elif name == 'TranslateX':      # translate by [-pixels, 0]: source x = x + pixels
    farg[:6] = [1, 0, f(sg * arg[0]), 0, 1, 0]
  elif name == 'TranslateY':
    farg[:6] = [1, 0, 0, 0, 1, f(sg * arg[0])]
  elif name == 'Posterize':
    iarg[0] = 8 - arg[0]
  elif name == 'Solarize':
    iarg[0] = arg[0]
  elif name == 'SolarizeAdd':
    iarg[:2] = [arg[0], 128]
  elif name == 'Cutout':
    pad = arg[0]
    cy, cx = min(int(cy_u * h), h - 1), min(int(cx_u * w), w - 1)
    iarg[:] = [max(0, cy - pad), max(0, cx - pad), min(h, cy + pad), min(w, cx + pad)]
  elif name in ('Color', 'Contrast', 'Brightness', 'Sharpness'):
    farg[6] = f(arg[0])


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
  for idx in np.ndindex(*op.shape):
    k = int(op[idx])
    if not 0 <= k < IDENTITY:
      ops[idx] = IDENTITY
      continue
    name = AVAILABLE_OPS[k]
    _fill_op(name, arg[name], float(sign[idx]), cy_u[idx], cx_u[idx], h, w, iargs[idx], fargs[idx])
  return ops, iargs, fargs


# ---- AutoAugment v0 (autoaugment.py:33-76, :527-660) on the same kernels ------------------------------------------------------
# (operation, probability, level) per position; a sub-policy per row.  The published policy of the AutoAugment paper as the
# reference tabulates it (:38-64), and its one-row debugging policy (:73-75).
_POLICY_V0 = (
    (('Equalize', 0.8, 1), ('ShearY', 0.8, 4)), (('Color', 0.4, 9), ('Equalize', 0.6, 3)),
    (('Color', 0.4, 1), ('Rotate', 0.6, 8)), (('Solarize', 0.8, 3), ('Equalize', 0.4, 7)),
    (('Solarize', 0.4, 2), ('Solarize', 0.6, 2)), (('Color', 0.2, 0), ('Equalize', 0.8, 8)),
    (('Equalize', 0.4, 8), ('SolarizeAdd', 0.8, 3)), (('ShearX', 0.2, 9), ('Rotate', 0.6, 8)),
    (('Color', 0.6, 1), ('Equalize', 1.0, 2)), (('Invert', 0.4, 9), ('Rotate', 0.6, 0)),
    (('Equalize', 1.0, 9), ('ShearY', 0.6, 3)), (('Color', 0.4, 7), ('Equalize', 0.6, 0)),
    (('Posterize', 0.4, 6), ('AutoContrast', 0.4, 7)), (('Solarize', 0.6, 8), ('Color', 0.6, 9)),
    (('Solarize', 0.2, 4), ('Rotate', 0.8, 9)), (('Rotate', 1.0, 7), ('TranslateY', 0.8, 9)),
    (('ShearX', 0.0, 0), ('Solarize', 0.8, 4)), (('ShearY', 0.8, 0), ('Color', 0.6, 4)),
    (('Color', 1.0, 0), ('Rotate', 0.6, 2)), (('Equalize', 0.8, 4), ('Equalize', 0.0, 8)),
    (('Equalize', 1.0, 4), ('AutoContrast', 0.6, 2)), (('ShearY', 0.4, 7), ('SolarizeAdd', 0.6, 7)),
    (('Posterize', 0.8, 2), ('Solarize', 0.6, 10)), (('Solarize', 0.6, 8), ('Equalize', 0.6, 1)),
    (('Color', 0.8, 6), ('Rotate', 0.4, 5)))
_POLICY_VTEST = ((('TranslateX', 1.0, 4), ('Equalize', 1.0, 10)),)
AUTOAUG_TRANSLATE_CONST, AUTOAUG_CUTOUT_CONST = 250, 100      # distort_image_with_autoaugment's (:658)


def policy_v0():
  """The reference's policy_v0 (:33-65) as plain data: 25 sub-policies of two (operation, probability, level)."""
  return [list(sub) for sub in _POLICY_V0]


def policy_vtest():
  """The reference's policy_vtest (:68-76)."""
  return [list(sub) for sub in _POLICY_VTEST]


AVAILABLE_POLICIES = {'v0': policy_v0, 'test': policy_vtest}


_CHECKED = {}      # name -> the checked table of a named policy: resolved once, read-only from then on


def _policy(policy):
  """A policy by name or as a table -> the table, checked: every sub-policy of the same length, known operations,
  probabilities in [0, 1], levels in check_magnitude's range.  A named policy is resolved and checked once."""
  if isinstance(policy, str):
    if policy not in AVAILABLE_POLICIES:
      raise ValueError('Invalid augmentation_name: {}'.format(policy))
    if policy not in _CHECKED:
      _CHECKED[policy] = _policy(AVAILABLE_POLICIES[policy]())
    return _CHECKED[policy]
  policy = [list(sub) for sub in policy]
  if not policy or not policy[0] or any(len(sub) != len(policy[0]) for sub in policy):
    raise ValueError('a policy is a non-empty list of sub-policies of one length')
  for sub in policy:
    for name, prob, level in sub:
      if name not in OP_ID:
        raise ValueError('unknown AutoAugment operation %r' % (name,))
      if not 0.0 <= float(prob) <= 1.0:
        raise ValueError('probability %r of %s outside [0, 1]' % (prob, name))
      check_magnitude(level)
  return policy


def autoaug_draws(rng, batch, policy='v0'):
  """One step's AutoAugment draws -> (sub int32 [B], apply_u float32 [P, B] in [0, 1), sign float32 [P, B] in {+1, -1}),
  P the sub-policies' length.  Per image: the sub-policy index (select_and_apply_random_policy, :573), then per position its
  apply draw (_apply_func_with_prob, :562-563) and its sign draw (_randomly_negate_tensor, :464-468; +1 = kept).  Both are
  ALWAYS drawn, whatever the operation and its probability, so the stream does not depend on the table: this is the
  project's definition (the reference's graph draws a uniform per branch per image; its stream is TensorFlow's)."""
  table = _policy(policy)
  b, p = int(batch), len(table[0])
  sub = np.zeros(b, np.int32)
  apply_u = np.zeros((p, b), np.float32)
  sign = np.ones((p, b), np.float32)
  for i in range(b):
    sub[i] = min(int(rng.random() * len(table)), len(table) - 1)      # (one uniform, whatever the table's length)
    for k in range(p):
      apply_u[k, i] = rng.random(dtype=np.float32)
      sign[k, i] = 1.0 if rng.random() >= 0.5 else -1.0
  return sub, apply_u, sign


def autoaug_applied(apply_u, prob):
  """should_apply_op of :562-563: floor(float32(u) + float32(prob)) as a boolean."""
  return bool(np.floor(np.float32(apply_u) + np.float32(prob)) >= 1)


@functools.lru_cache(maxsize=4096)
def _entry_args(name, level, sg, h, w):
  """The kernel arguments (iarg [4], farg [8]) of one table entry: they depend on nothing but the operation, its level, the
  sign (+1 for an operation that has none) and the image size, so a step looks them up instead of forming them per image."""
  iarg, farg = np.zeros(4, np.int32), np.zeros(8, np.float32)
  farg[6] = 1.0
  arg = level_to_arg(name, level, AUTOAUG_TRANSLATE_CONST, AUTOAUG_CUTOUT_CONST)
  _fill_op(name, arg, sg, 0.0, 0.0, h, w, iarg, farg)      # (no policy here holds Cutout, whose centre is a draw of its own)
  return iarg, farg


def autoaug_args(draws, h, w, policy='v0'):
  """draws of autoaug_draws -> (ops int32 [P, B], iargs int32 [P, B, 4], fargs float32 [P, B, 8]) in randaug_args' layout:
  position k of image i is operation k of sub-policy sub[i] at the table's own level (level_to_arg with translate_const 250
  and cutout_const 100, :658) where autoaug_applied(apply_u, prob), else IDENTITY; the random negation reaches the five
  signed operations.  A sub-policy index outside the table makes every position of that image IDENTITY."""
  table = _policy(policy)
  sub, apply_u, sign = (np.asarray(d) for d in draws)
  p = len(table[0])
  if not (sub.ndim == 1 and apply_u.shape == sign.shape == (p, sub.shape[0])):
    raise ValueError('draws must be (sub [batch], apply_u [%d, batch], sign [%d, batch]), got shapes %s' % (
        p, p, [np.shape(d) for d in draws]))
  shape = (p, sub.shape[0])
  ops = np.full(shape, IDENTITY, np.int32)
  iargs = np.zeros(shape + (4,), np.int32)
  fargs = np.zeros(shape + (8,), np.float32)
  fargs[..., 6] = 1.0
  h, w = int(h), int(w)
  inside = (sub >= 0) & (sub < len(table))
  probs = np.array([[prob for _, prob, _ in entries] for entries in table], np.float32)[np.where(inside, sub, 0)].T      # [P, B]
  applied = (np.floor(apply_u.astype(np.float32) + probs) >= 1) & inside[None, :]      # autoaug_applied, for every position
  for k, i in zip(*np.nonzero(applied)):
    name, _, level = table[int(sub[i])][k]
    if name == 'Cutout':
      raise ValueError('a policy with Cutout is not built: autoaug_draws has no centre draws for it')
    ops[k, i] = OP_ID[name]
    iargs[k, i], fargs[k, i] = _entry_args(name, level, float(sign[k, i]) if name in SIGNED_OPS else 1.0, h, w)
  return ops, iargs, fargs


UNBUILT = {
    'autoaug': 'AutoAugment v0 (autoaugment.py:33-65,633-660)',      # (built under its own names: LEGACY_HINT)
    'ra_aa': "the random choice between AutoAugment and RandAugment (autoaugment.py:712-719)",
}


# the trailing hint of the refusals that the legacy input pipeline answers under its own switch
LEGACY_HINT = (" through this name (the legacy input pipeline with AutoAugment v0 is TrainableModel(preprocessing='legacy', "
               "augment_name=...), effnetv2_main --legacy_input; autoaugment.distort_image_with_autoaugment)")


def check_aug_name(aug_name):
  """'randaug' or a ValueError that names what the reference would have run."""
  if aug_name == 'randaug':
    return aug_name
  name = str(aug_name)
  if name in UNBUILT:
    raise ValueError('aug_name %r is not built: %s; only \'randaug\' is%s' % (aug_name, UNBUILT[name],
                                                                             LEGACY_HINT if name == 'autoaug' else ''))
  if name.startswith('effnetv1_') or name.startswith('ft'):
    raise ValueError('aug_name %r is not built: the legacy / fine-tuning preprocessing (preprocessing.py:112-147); only '
                     '\'randaug\' is%s' % (aug_name, LEGACY_HINT if name.startswith('effnetv1_') else ''))
  raise ValueError('Invalid value for aug_name: %s (autoaugment.py:721)' % (aug_name,))


_OUT = {None: (_lib.EDET_U8, torch.uint8), torch.uint8: (_lib.EDET_U8, torch.uint8),
        torch.float32: (_lib.EDET_F32, torch.float32), torch.bfloat16: (_lib.EDET_BF16, torch.bfloat16)}


def _apply(src, dst, b, h, w, ops, iargs, fargs, luts, code, mean_std, stream):
  """edet_randaug_apply, or with mean_std (six host floats) edet_randaug_apply_norm."""
  nbytes = src.numel() * (1 + dst.element_size())
  if mean_std is None:
    call('edet_randaug_apply', ptr(src), ptr(dst), b, h, w, ops, iargs, fargs, luts, code, stream, nbytes=nbytes)
  else:
    call('edet_randaug_apply_norm', ptr(src), ptr(dst), b, h, w, ops, iargs, fargs, luts, code, mean_std, stream, nbytes=nbytes)


def apply_layers(src, out, ops, iargs, fargs, luts, scratch, stream, norm=None):
  """The launches of `ops.shape[0]` RandAugment layers on device tensors: src uint8 [B, H, W, 3] -> out (uint8, or fp32 /
  bf16 = normalised by the last layer).  ops / iargs / fargs: device [L, B(, 4 / 8)]; luts uint8 [B, 3, 256]; scratch: two
  uint8 buffers like src for the layers in between (the kernels never run in place).  L = 0: the (normalising) copy.
  norm: None = (x - 128) / 128 (edet_randaug_apply); (mean [3], std [3]) = the legacy pipeline's (x - mean) / std by
  edet_randaug_apply_norm as the last launch."""
  from automl_amd import v2_preprocessing
  b, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
  code = _OUT[out.dtype][0]
  mean_std = v2_preprocessing.mean_std_array(norm)
  layers = 0 if ops is None else int(ops.shape[0])
  if layers == 0:
    _apply(src, out, b, h, w, None, None, None, None, code, mean_std, stream)
    return out
  cur = src
  for k in range(layers):
    last = k == layers - 1
    dst = out if last else scratch[k % 2]
    call('edet_randaug_stats', ptr(cur), b, h, w, ptr(ops[k]), ptr(luts), stream, nbytes=cur.numel())
    _apply(cur, dst, b, h, w, ptr(ops[k]), ptr(iargs[k]), ptr(fargs[k]), ptr(luts), code if last else _lib.EDET_U8,
           mean_std if last else None, stream)
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


def _run_layers(x, host_args, layers, out_dtype, norm):
  """A uint8 device batch through `layers` layers of host argument arrays (ops, iargs, fargs) -> a new device tensor."""
  b = int(x.shape[0])
  out = torch.empty(x.shape, dtype=_OUT[out_dtype][1], device=x.device)
  stream = torch.cuda.current_stream().cuda_stream
  if layers == 0:
    return apply_layers(x, out, None, None, None, None, None, stream, norm=norm)
  ops, iargs, fargs = (torch.from_numpy(a).to(x.device) for a in host_args)
  luts = torch.zeros((b, 3, 256), dtype=torch.uint8, device=x.device)
  scratch = [torch.empty_like(x) for _ in range(min(layers - 1, 2))]
  return apply_layers(x, out, ops, iargs, fargs, luts, scratch, stream, norm=norm)


def distort_image_with_autoaugment(images_u8, augmentation_name, rng=None, draws=None, out_dtype=None, norm=None):
  """autoaugment.distort_image_with_autoaugment (:633-660) for a batch on the device: images_u8 uint8 [B, H, W, 3] (numpy or
  torch), augmentation_name 'v0' or 'test' -> the augmented batch as a device tensor: uint8, or with out_dtype torch.float32
  / torch.bfloat16 the network input, (x - 128) / 128 or, with norm = (mean [3], std [3]), the legacy (x - mean) / std.
  draws: autoaug_draws' arrays, else drawn from `rng` (a numpy Generator; default: a fresh one).  Two layers of
  edet_randaug_stats + edet_randaug_apply: no kernel of its own."""
  if augmentation_name not in AVAILABLE_POLICIES:
    raise ValueError('Invalid augmentation_name: {}'.format(augmentation_name))
  table = AVAILABLE_POLICIES[augmentation_name]()
  if out_dtype not in _OUT:
    raise ValueError('out_dtype %r: None / torch.uint8, torch.float32 or torch.bfloat16' % (out_dtype,))
  x = torch.from_numpy(images_u8) if isinstance(images_u8, np.ndarray) else images_u8
  if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
    raise ValueError('images must be uint8 [batch, height, width, 3], got %s %s' % (x.dtype, tuple(x.shape)))
  x = x.to('cuda').contiguous()
  b, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
  if draws is None:
    draws = autoaug_draws(rng if rng is not None else np.random.default_rng(), b, table)
  return _run_layers(x, autoaug_args(draws, h, w, table), len(table[0]), out_dtype, norm)
