"""Box-aware AutoAugment and RandAugment on the device: the reference's ``efficientdet/aug/autoaugment.py`` for a whole uint8
batch with padded boxes.

Mirror of the reference module's public names as far as they are built: the policy tables (:37-147),
``distort_image_with_autoaugment`` (:1592-1629) for ``'test'``, ``'v2'`` and ``'v3'``, ``distort_image_with_randaugment``
(:1632-1667), ``level_to_arg`` with the detector's constants (:1620-1626).  The draws are made on the host
(``autoaug_draws``), turned into the kernels' argument arrays (``autoaug_args``) and applied per layer by four launches:
``edet_autoaug_boxes`` (the boxes follow the geometric operations; BBox_Cutout's rectangle from a box on the device),
``edet_randaug_stats``, ``edet_autoaug_contrast_lut`` (the detector's Contrast blends with the true mean grey level,
:267-280 -- the classifier's does not) and ``edet_randaug_apply``, the classifier's image kernel, unchanged.  A layer is one
position of a sub-policy: the operation differs per image, chosen from device memory.  The numpy restatement the kernels are
compared with bit for bit is tests/det_autoaug_ref.py.

A canvas batch (``sizes=``, what ``jpeg.JpegDecoder.decode`` returns next to the images): image ``i`` is the top-left
``sizes[i]`` of its slot and is distorted as that image alone would be -- its own height and width in every argument, box and
statistic (the ``*_canvas`` entry points).  The draws do not depend on the sizes.  The kernels write inside the rectangles only.

Not pinned by anything here, as for the classifier's RandAugment (automl_amd/autoaugment.py): TensorFlow Addons' rounding rule
in the geometric image operations and float32 sine / cosine (numpy's, on the host); TensorFlow's random streams (the draws are
numpy's); ``reduce_mean``'s summation order in Contrast for an image whose grey sum reaches 2^24 (more than 65,793 pixels) --
there the kernel's exact integer sum is the definition.

Not built, and raising rather than ignored: the nine ``*_Only_BBoxes`` operations (:503-782), hence ``'v0'`` and ``'v1'``,
which need them; ``cutout_bbox_replace_with_mean=True``.
"""
import collections

import numpy as np
import torch

from automl_amd import _lib
from automl_amd import autoaugment as v2aa
from automl_amd import utils
from automl_amd._lib import call, ptr

_MAX_LEVEL = 10.
CUTOUT_CONST, TRANSLATE_CONST, CUTOUT_MAX_PAD_FRACTION, CUTOUT_BBOX_REPLACE_WITH_MEAN = 100, 250, 0.75, False      # :1620-1626

# NAME_TO_FUNC (:1350-1372) without the *_Only_BBoxes family; the index is the policy id the kernels read
NAMES = ('AutoContrast', 'Equalize', 'Posterize', 'Solarize', 'SolarizeAdd', 'Color', 'Contrast', 'Brightness', 'Sharpness',
         'Cutout', 'BBox_Cutout', 'Rotate_BBox', 'TranslateX_BBox', 'TranslateY_BBox', 'ShearX_BBox', 'ShearY_BBox')
OP_ID = {name: i for i, name in enumerate(NAMES)}
NONE = len(NAMES)      # policy id 16: image and boxes pass through
SIGNED_OPS = ('Rotate_BBox', 'TranslateX_BBox', 'TranslateY_BBox', 'ShearX_BBox', 'ShearY_BBox')      # _randomly_negate_tensor
UNBUILT_OPS = {      # name: where the reference defines it
    'Rotate_Only_BBoxes': 713, 'ShearX_Only_BBoxes': 721, 'ShearY_Only_BBoxes': 729, 'TranslateX_Only_BBoxes': 737,
    'TranslateY_Only_BBoxes': 745, 'Flip_Only_BBoxes': 753, 'Solarize_Only_BBoxes': 761, 'Equalize_Only_BBoxes': 769,
    'Cutout_Only_BBoxes': 777}
RANDAUG_OPS = ('Equalize', 'Solarize', 'Color', 'Cutout', 'SolarizeAdd', 'TranslateX_BBox', 'TranslateY_BBox', 'ShearX_BBox',
               'ShearY_BBox', 'Rotate_BBox')      # available_ops, :1646-1649
# what the image kernel is told (edet_randaug_apply's ids, automl_amd/autoaugment.OP_ID).  Contrast is the copy until
# edet_autoaug_contrast_lut has made the image's table and turned the id into Equalize's, the table look-up
APPLY_ID = {'AutoContrast': 0, 'Equalize': 1, 'Posterize': 4, 'Solarize': 5, 'SolarizeAdd': 15, 'Color': 6,
            'Contrast': v2aa.IDENTITY, 'Brightness': 8, 'Sharpness': 9, 'Cutout': 14, 'BBox_Cutout': 14, 'Rotate_BBox': 3,
            'TranslateX_BBox': 12, 'TranslateY_BBox': 13, 'ShearX_BBox': 10, 'ShearY_BBox': 11}


def policy_v0():
  return [
      [('TranslateX_BBox', 0.6, 4), ('Equalize', 0.8, 10)],
      [('TranslateY_Only_BBoxes', 0.2, 2), ('Cutout', 0.8, 8)],
      [('Sharpness', 0.0, 8), ('ShearX_BBox', 0.4, 0)],
      [('ShearY_BBox', 1.0, 2), ('TranslateY_Only_BBoxes', 0.6, 6)],
      [('Rotate_BBox', 0.6, 10), ('Color', 1.0, 6)],
  ]


def policy_v1():
  return [
      [('TranslateX_BBox', 0.6, 4), ('Equalize', 0.8, 10)],
      [('TranslateY_Only_BBoxes', 0.2, 2), ('Cutout', 0.8, 8)],
      [('Sharpness', 0.0, 8), ('ShearX_BBox', 0.4, 0)],
      [('ShearY_BBox', 1.0, 2), ('TranslateY_Only_BBoxes', 0.6, 6)],
      [('Rotate_BBox', 0.6, 10), ('Color', 1.0, 6)],
      [('Color', 0.0, 0), ('ShearX_Only_BBoxes', 0.8, 4)],
      [('ShearY_Only_BBoxes', 0.8, 2), ('Flip_Only_BBoxes', 0.0, 10)],
      [('Equalize', 0.6, 10), ('TranslateX_BBox', 0.2, 2)],
      [('Color', 1.0, 10), ('TranslateY_Only_BBoxes', 0.4, 6)],
      [('Rotate_BBox', 0.8, 10), ('Contrast', 0.0, 10)],
      [('Cutout', 0.2, 2), ('Brightness', 0.8, 10)],
      [('Color', 1.0, 6), ('Equalize', 1.0, 2)],
      [('Cutout_Only_BBoxes', 0.4, 6), ('TranslateY_Only_BBoxes', 0.8, 2)],
      [('Color', 0.2, 8), ('Rotate_BBox', 0.8, 10)],
      [('Sharpness', 0.4, 4), ('TranslateY_Only_BBoxes', 0.0, 4)],
      [('Sharpness', 1.0, 4), ('SolarizeAdd', 0.4, 4)],
      [('Rotate_BBox', 1.0, 8), ('Sharpness', 0.2, 8)],
      [('ShearY_BBox', 0.6, 10), ('Equalize_Only_BBoxes', 0.6, 8)],
      [('ShearX_BBox', 0.2, 6), ('TranslateY_Only_BBoxes', 0.2, 10)],
      [('SolarizeAdd', 0.6, 8), ('Brightness', 0.8, 10)],
  ]


def policy_vtest():
  return [
      [('TranslateX_BBox', 1.0, 4), ('Equalize', 1.0, 10)],
  ]


def policy_v2():
  return [
      [('Color', 0.0, 6), ('Cutout', 0.6, 8), ('Sharpness', 0.4, 8)],
      [('Rotate_BBox', 0.4, 8), ('Sharpness', 0.4, 2), ('Rotate_BBox', 0.8, 10)],
      [('TranslateY_BBox', 1.0, 8), ('AutoContrast', 0.8, 2)],
      [('AutoContrast', 0.4, 6), ('ShearX_BBox', 0.8, 8), ('Brightness', 0.0, 10)],
      [('SolarizeAdd', 0.2, 6), ('Contrast', 0.0, 10), ('AutoContrast', 0.6, 0)],
      [('Cutout', 0.2, 0), ('Solarize', 0.8, 8), ('Color', 1.0, 4)],
      [('TranslateY_BBox', 0.0, 4), ('Equalize', 0.6, 8), ('Solarize', 0.0, 10)],
      [('TranslateY_BBox', 0.2, 2), ('ShearY_BBox', 0.8, 8), ('Rotate_BBox', 0.8, 8)],
      [('Cutout', 0.8, 8), ('Brightness', 0.8, 8), ('Cutout', 0.2, 2)],
      [('Color', 0.8, 4), ('TranslateY_BBox', 1.0, 6), ('Rotate_BBox', 0.6, 6)],
      [('Rotate_BBox', 0.6, 10), ('BBox_Cutout', 1.0, 4), ('Cutout', 0.2, 8)],
      [('Rotate_BBox', 0.0, 0), ('Equalize', 0.6, 6), ('ShearY_BBox', 0.6, 8)],
      [('Brightness', 0.8, 8), ('AutoContrast', 0.4, 2), ('Brightness', 0.2, 2)],
      [('TranslateY_BBox', 0.4, 8), ('Solarize', 0.4, 6), ('SolarizeAdd', 0.2, 10)],
      [('Contrast', 1.0, 10), ('SolarizeAdd', 0.2, 8), ('Equalize', 0.2, 4)],
  ]


def policy_v3():
  return [
      [('Posterize', 0.8, 2), ('TranslateX_BBox', 1.0, 8)],
      [('BBox_Cutout', 0.2, 10), ('Sharpness', 1.0, 8)],
      [('Rotate_BBox', 0.6, 8), ('Rotate_BBox', 0.8, 10)],
      [('Equalize', 0.8, 10), ('AutoContrast', 0.2, 10)],
      [('SolarizeAdd', 0.2, 2), ('TranslateY_BBox', 0.2, 8)],
      [('Sharpness', 0.0, 2), ('Color', 0.4, 8)],
      [('Equalize', 1.0, 8), ('TranslateY_BBox', 1.0, 8)],
      [('Posterize', 0.6, 2), ('Rotate_BBox', 0.0, 10)],
      [('AutoContrast', 0.6, 0), ('Rotate_BBox', 1.0, 6)],
      [('Equalize', 0.0, 4), ('Cutout', 0.8, 10)],
      [('Brightness', 1.0, 2), ('TranslateY_BBox', 1.0, 6)],
      [('Contrast', 0.0, 2), ('ShearY_BBox', 0.8, 0)],
      [('AutoContrast', 0.8, 10), ('Contrast', 0.2, 10)],
      [('Rotate_BBox', 1.0, 10), ('Cutout', 1.0, 10)],
      [('SolarizeAdd', 0.8, 6), ('Equalize', 0.8, 8)],
  ]


AVAILABLE_POLICIES = {'v0': policy_v0, 'v1': policy_v1, 'v2': policy_v2, 'v3': policy_v3, 'test': policy_vtest}      # :1613-1614


def available_policy(name):
  """'randaug' -> 'randaug'; 'v2' / 'v3' / 'test' -> the table.  'v0' and 'v1' need operations that are not built and raise a
  ValueError naming them; anything else raises the reference's 'Invalid augmentation_name' (:1616)."""
  if name == 'randaug':
    return name
  if not isinstance(name, str) or name not in AVAILABLE_POLICIES:
    raise ValueError('Invalid augmentation_name: {}'.format(name))
  table = AVAILABLE_POLICIES[name]()
  missing = sorted({op for sub in table for op, _, _ in sub if op in UNBUILT_OPS})
  if missing:
    raise ValueError('augmentation_name %r is not built: it needs %s; built are \'randaug\', \'v2\', \'v3\' and \'test\''
                     % (name, ', '.join('%s (aug/autoaugment.py:%d)' % (op, UNBUILT_OPS[op]) for op in missing)))
  return table


def check_op(op_name):
  if op_name in UNBUILT_OPS:
    raise ValueError('operation %r is not built (aug/autoaugment.py:%d)' % (op_name, UNBUILT_OPS[op_name]))
  if op_name not in OP_ID:
    raise ValueError('unknown AutoAugment operation %r (aug/autoaugment.py:1350-1382)' % (op_name,))
  return op_name


def level_to_arg(op_name, level):
  """The reference's argument tuple of `op_name` at `level` before the random negation (:1392-1470 with the hparams of
  :1620-1626), in Python's own arithmetic (doubles and int()): () / (bits,) / (threshold,) / (addition,) / (factor,) /
  (pad_size,) / (pad_fraction, replace_with_mean) / (degrees,) / (pixels,) / (shear level,)."""
  check_op(op_name)
  level = float(level)
  if level < 0.0:
    raise ValueError('level %r must be >= 0' % (level,))
  if op_name in ('AutoContrast', 'Equalize'):
    return ()
  if op_name == 'Posterize':
    bits = int((level / _MAX_LEVEL) * 4)
    if bits > 8:
      raise ValueError('Posterize at level %r would shift by 8 - %d bits (:289-292)' % (level, bits))
    return (bits,)
  if op_name == 'Solarize':
    return (int((level / _MAX_LEVEL) * 256),)
  if op_name == 'SolarizeAdd':
    return (int((level / _MAX_LEVEL) * 110),)
  if op_name in ('Color', 'Contrast', 'Brightness', 'Sharpness'):
    return ((level / _MAX_LEVEL) * 1.8 + 0.1,)
  if op_name == 'Cutout':
    return (int((level / _MAX_LEVEL) * CUTOUT_CONST),)
  if op_name == 'BBox_Cutout':
    return ((level / _MAX_LEVEL) * CUTOUT_MAX_PAD_FRACTION, CUTOUT_BBOX_REPLACE_WITH_MEAN)
  if op_name == 'Rotate_BBox':
    return ((level / _MAX_LEVEL) * 30.,)
  if op_name in ('ShearX_BBox', 'ShearY_BBox'):
    return ((level / _MAX_LEVEL) * 0.3,)
  return ((level / _MAX_LEVEL) * float(TRANSLATE_CONST),)      # TranslateX_BBox / TranslateY_BBox


AutoAugDraws = collections.namedtuple('AutoAugDraws', ['index', 'apply', 'sign', 'cy_u', 'cx_u', 'box_u'])
AutoAugArgs = collections.namedtuple('AutoAugArgs', ['policy', 'ops', 'iargs', 'fargs', 'dargs'])


def _table(policy):
  return available_policy(policy) if isinstance(policy, str) else policy


def num_layers_of(policy, num_layers=1):
  """Layers (launch groups) of a policy: the longest sub-policy of a table, num_layers for 'randaug'."""
  table = _table(policy)
  return int(num_layers) if table == 'randaug' else max(len(sub) for sub in table)


def autoaug_draws(rng, batch, policy, num_layers=1):
  """One batch's draws from a numpy generator.  index: the sub-policy per image [B] (select_and_apply_random_policy, :1527),
  or for 'randaug' the operation over RANDAUG_OPS per layer and image [L, B] (:1655).  Per layer and image [L, B]: apply
  float32 in [0, 1), the reference applies when floor(u + prob) is 1 (:1516-1517; None for 'randaug', whose `prob` draw of
  :1660 is discarded and not made); sign float32 +1 / -1 (_randomly_negate_tensor, +1 = kept); cy_u, cx_u float64 in [0, 1),
  the centre of Cutout over the image and of BBox_Cutout over the chosen box; box_u float64, BBox_Cutout's box (:1324)."""
  table = _table(policy)
  b = int(batch)
  layers = num_layers_of(table, num_layers)
  shape = (layers, b)
  if table == 'randaug':
    index, apply = rng.integers(0, len(RANDAUG_OPS), size=shape).astype(np.int32), None
  else:
    index = rng.integers(0, len(table), size=b).astype(np.int32)
    apply = rng.random(shape).astype(np.float32)
  sign = np.where(rng.random(shape) >= 0.5, 1.0, -1.0).astype(np.float32)
  cy_u, cx_u, box_u = rng.random(shape), rng.random(shape), rng.random(shape)
  return AutoAugDraws(index, apply, sign, cy_u, cx_u, box_u)


def should_apply(u, prob):
  """:1516-1517 in float32: floor(u + prob) cast to bool."""
  return bool(np.floor(np.float32(u) + np.float32(prob)) != 0)


def autoaug_args(draws, policy, h, w, magnitude=None):
  """draws of autoaug_draws -> AutoAugArgs of host arrays, what the kernels take per layer (include/edet_hip.h): policy int32
  [L, B] (the reference's operation, NONE where nothing happens), ops int32 [L, B] / iargs int32 [L, B, 4] / fargs float32
  [L, B, 8] in edet_randaug_apply's layout, dargs float64 [L, B, 4] (BBox_Cutout: pad_fraction and its three draws).  An
  operation that is not applied and a layer past the end of a shorter sub-policy are the identity for image and boxes.
  magnitude: the level of every operation of 'randaug'.  h, w: two numbers, or arrays [batch] for a canvas batch: column i is
  then what image i alone gets at its own size."""
  table = _table(policy)
  d = AutoAugDraws(*draws)
  sign = np.asarray(d.sign)
  if sign.ndim != 2:
    raise ValueError('draws must be arrays [num_layers, batch], got sign %s' % (sign.shape,))
  layers, b = sign.shape
  hs, ws = np.broadcast_to(np.asarray(h), (b,)), np.broadcast_to(np.asarray(w), (b,))
  index = np.asarray(d.index)
  if table == 'randaug':
    if magnitude is None:
      raise ValueError("'randaug' needs a magnitude")
    if index.shape != (layers, b):
      raise ValueError('randaug index draws are %s, want %s' % (index.shape, (layers, b)))
  else:
    if index.shape != (b,) or layers < max(len(sub) for sub in table):
      raise ValueError('draws for %d layers, sub-policy index %s: the table needs [%d, batch] and [batch]'
                       % (layers, index.shape, max(len(sub) for sub in table)))
    apply = np.asarray(d.apply)
  pol = np.full((layers, b), NONE, np.int32)
  ops = np.full((layers, b), v2aa.IDENTITY, np.int32)
  iargs = np.zeros((layers, b, 4), np.int32)
  fargs = np.zeros((layers, b, 8), np.float32)
  fargs[..., 6] = 1.0
  dargs = np.zeros((layers, b, 4), np.float64)
  f = np.float32
  for k in range(layers):
    for i in range(b):
      if table == 'randaug':
        if not 0 <= int(index[k, i]) < len(RANDAUG_OPS):
          continue
        name, level = RANDAUG_OPS[int(index[k, i])], float(magnitude)
      else:
        sub = table[int(index[i])]
        if k >= len(sub) or not should_apply(apply[k, i], sub[k][1]):
          continue
        name, level = sub[k][0], sub[k][2]
      arg = level_to_arg(name, level)
      idx = (k, i)
      pol[idx], ops[idx] = OP_ID[name], APPLY_ID[name]
      sg = float(sign[idx])
      h, w = int(hs[i]), int(ws[i])
      if name == 'Rotate_BBox':
        fargs[idx][:6] = v2aa.rotate_coefficients(sg * arg[0], h, w)
      elif name == 'ShearX_BBox':
        fargs[idx][:6] = [1, f(sg * arg[0]), 0, 0, 1, 0]
      elif name == 'ShearY_BBox':
        fargs[idx][:6] = [1, 0, 0, f(sg * arg[0]), 1, 0]
      elif name == 'TranslateX_BBox':      # translate by [-pixels, 0]: source x = x + pixels
        fargs[idx][:6] = [1, 0, f(sg * arg[0]), 0, 1, 0]
      elif name == 'TranslateY_BBox':
        fargs[idx][:6] = [1, 0, 0, 0, 1, f(sg * arg[0])]
      elif name == 'Posterize':
        iargs[idx][0] = 8 - arg[0]
      elif name == 'Solarize':
        iargs[idx][0] = arg[0]
      elif name == 'SolarizeAdd':
        iargs[idx][:2] = [arg[0], 128]
      elif name == 'Cutout':
        pad = arg[0]
        cy, cx = min(int(d.cy_u[k][i] * h), h - 1), min(int(d.cx_u[k][i] * w), w - 1)
        iargs[idx] = [max(0, cy - pad), max(0, cx - pad), min(h, cy + pad), min(w, cx + pad)]
      elif name == 'BBox_Cutout':      # the rectangle is made on the device, from the box
        if arg[1]:
          raise ValueError('cutout_bbox_replace_with_mean=True is not built')
        dargs[idx] = [arg[0], d.box_u[k][i], d.cy_u[k][i], d.cx_u[k][i]]
      elif name in ('Color', 'Contrast', 'Brightness', 'Sharpness'):
        fargs[idx][6] = f(arg[0])
  return AutoAugArgs(pol, ops, iargs, fargs, dargs)


def pack_args(args):
  """AutoAugArgs -> one uint8 host array (dargs first: 8-byte alignment) and the (offset, shape, dtype) of each field in it,
  so that one copy carries a step's arguments to the device."""
  order = ('dargs', 'fargs', 'iargs', 'ops', 'policy')
  parts, layout, off = [], {}, 0
  for name in order:
    a = np.ascontiguousarray(getattr(args, name))
    layout[name] = (off, a.shape, a.dtype)
    parts.append(a.reshape(-1).view(np.uint8))
    off += a.nbytes
  return np.concatenate(parts), layout


def args_layout(layers, batch):
  """(pack_args' layout, its size in bytes) of the arguments of `layers` x `batch` operations."""
  shape = (int(layers), int(batch))
  host, layout = pack_args(AutoAugArgs(np.zeros(shape, np.int32), np.zeros(shape, np.int32), np.zeros(shape + (4,), np.int32),
                                       np.zeros(shape + (8,), np.float32), np.zeros(shape + (4,), np.float64)))
  return layout, int(host.size)


_TORCH_DTYPE = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}


def unpack_args(buf, layout):
  """Views of a uint8 device tensor `buf` by pack_args' layout -> AutoAugArgs of device tensors."""
  out = {}
  for name, (off, shape, dtype) in layout.items():
    n = int(np.prod(shape)) * dtype.itemsize
    out[name] = buf[off:off + n].view(_TORCH_DTYPE[dtype]).view(*shape)
  return AutoAugArgs(**out)


def apply_layers(src, out, boxes, boxes_out, counts, args, luts, scratch, stream, sizes=None):
  """The launches of `args.policy.shape[0]` layers on device tensors: src uint8 [B, H, W, 3] -> out uint8, boxes float32
  [B, M, 4] -> boxes_out (another buffer: the caller's boxes are not written), counts int32 [B].  args: AutoAugArgs of device
  tensors (the kernels write BBox_Cutout's rectangle into iargs and Contrast's apply id into ops); luts uint8 [B, 3, 256];
  scratch: two uint8 buffers like src for the layers in between (the image kernel never runs in place).  sizes: int32 [B, 2]
  on the device for a canvas batch (args made from the same sizes): out and scratch are then written inside each image's
  rectangle only."""
  b, h, w, m = int(src.shape[0]), int(src.shape[1]), int(src.shape[2]), int(boxes.shape[1])
  layers = int(args.policy.shape[0])
  cur, bcur = src, boxes
  for k in range(layers):
    dst = out if k == layers - 1 else scratch[k % 2]
    if sizes is None:
      call('edet_autoaug_boxes', ptr(bcur), ptr(boxes_out), ptr(counts), b, m, h, w, ptr(args.policy[k]), ptr(args.iargs[k]),
           ptr(args.fargs[k]), ptr(args.dargs[k]), stream, nbytes=2 * bcur.numel() * 4)
      call('edet_randaug_stats', ptr(cur), b, h, w, ptr(args.ops[k]), ptr(luts), stream, nbytes=cur.numel())
      call('edet_autoaug_contrast_lut', ptr(cur), b, h, w, ptr(args.policy[k]), ptr(args.ops[k]), ptr(args.fargs[k]), ptr(luts),
           stream, nbytes=cur.numel())
      call('edet_randaug_apply', ptr(cur), ptr(dst), b, h, w, ptr(args.ops[k]), ptr(args.iargs[k]), ptr(args.fargs[k]), ptr(luts),
           _lib.EDET_U8, stream, nbytes=2 * cur.numel())
    else:
      call('edet_autoaug_boxes_canvas', ptr(bcur), ptr(boxes_out), ptr(counts), b, m, ptr(sizes), ptr(args.policy[k]),
           ptr(args.iargs[k]), ptr(args.fargs[k]), ptr(args.dargs[k]), stream, nbytes=2 * bcur.numel() * 4)
      call('edet_randaug_stats_canvas', ptr(cur), b, h, w, ptr(sizes), ptr(args.ops[k]), ptr(luts), stream, nbytes=cur.numel())
      call('edet_autoaug_contrast_lut_canvas', ptr(cur), b, h, w, ptr(sizes), ptr(args.policy[k]), ptr(args.ops[k]),
           ptr(args.fargs[k]), ptr(luts), stream, nbytes=cur.numel())
      call('edet_randaug_apply_canvas', ptr(cur), ptr(dst), b, h, w, ptr(sizes), ptr(args.ops[k]), ptr(args.iargs[k]),
           ptr(args.fargs[k]), ptr(luts), _lib.EDET_U8, stream, nbytes=2 * cur.numel())
    cur, bcur = dst, boxes_out
  return out, boxes_out


def _distort(images_u8, boxes, counts, policy, num_layers, magnitude, rng, draws, sizes=None):
  x = torch.from_numpy(images_u8) if isinstance(images_u8, np.ndarray) else images_u8
  if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
    raise ValueError('images must be uint8 [batch, height, width, 3], got %s %s' % (x.dtype, tuple(x.shape)))
  b, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
  bx = torch.as_tensor(boxes, dtype=torch.float32)
  if bx.dim() != 3 or bx.shape[0] != b or bx.shape[2] != 4 or bx.shape[1] < 1:
    raise ValueError('boxes must be float32 [batch, max_boxes >= 1, 4], got %s' % (tuple(bx.shape),))
  if sizes is not None:      # (checked before the generator moves)
    sizes = utils.canvas_sizes(sizes, b, h, w)
    h, w = sizes[:, 0], sizes[:, 1]
  x = x.to('cuda').contiguous()
  bx = bx.to(x.device).contiguous()
  cn = torch.as_tensor(counts).to(x.device).to(torch.int32).reshape(b).contiguous()
  layers = num_layers_of(policy, num_layers)
  if layers == 0:
    return x.clone(), bx.clone()
  if draws is None:
    draws = autoaug_draws(rng if rng is not None else np.random.default_rng(), b, policy, num_layers)
  host, layout = pack_args(autoaug_args(draws, policy, h, w, magnitude))
  if layout['policy'][1] != (layers, b):
    raise ValueError('draws are for %s, want [num_layers, batch] = %s' % (layout['policy'][1], (layers, b)))
  args = unpack_args(torch.from_numpy(host).to(x.device), layout)
  out, boxes_out = (torch.empty_like(x) if sizes is None else torch.zeros_like(x)), torch.empty_like(bx)
  luts = torch.zeros((b, 3, 256), dtype=torch.uint8, device=x.device)
  scratch = [torch.empty_like(x) for _ in range(min(layers - 1, 2))]
  return apply_layers(x, out, bx, boxes_out, cn, args, luts, scratch, torch.cuda.current_stream().cuda_stream,
                      None if sizes is None else torch.from_numpy(sizes).to(x.device))


def distort_image_with_autoaugment(images_u8, boxes, counts, augmentation_name, rng=None, draws=None, sizes=None):
  """:1592-1629 for a batch on the device: images_u8 uint8 [B, H, W, 3], boxes float32 [B, M, 4] padded and normalised (ymin,
  xmin, ymax, xmax), counts [B] valid rows (numpy or torch) -> (images uint8, boxes) device tensors; rows at or past
  counts[i] pass through.  draws: autoaug_draws' tuple, else drawn from `rng` (a numpy Generator; default: a fresh one).
  sizes: [B, 2] (height, width) of each image on the canvas [H, W] -- host data (utils.canvas_sizes; a device tensor is copied
  to the host, which waits for the device), checked before the generator moves; the images come back zero outside their
  rectangles."""
  if augmentation_name == 'randaug':
    raise ValueError("Invalid augmentation_name: randaug ('randaug' is distort_image_with_randaugment's)")
  return _distort(images_u8, boxes, counts, available_policy(augmentation_name), 0, None, rng, draws, sizes)


def distort_image_with_randaugment(images_u8, boxes, counts, num_layers, magnitude, rng=None, draws=None, sizes=None):
  """:1632-1667 for a batch on the device; arguments and results as distort_image_with_autoaugment's."""
  if int(num_layers) < 0:
    raise ValueError('num_layers %r must be >= 0' % (num_layers,))
  for name in RANDAUG_OPS:
    level_to_arg(name, magnitude)      # raises for a magnitude no operation could take
  return _distort(images_u8, boxes, counts, 'randaug', int(num_layers), float(magnitude), rng, draws, sizes)
