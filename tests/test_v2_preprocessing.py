"""automl_amd/v2_preprocessing.py and edet_crop_resize (csrc/crop_resize.hip): the host side of the reference's
efficientnetv2/preprocessing.py:22-70 (crop sampler, train / eval rows, the staged schedule of main_tf2.py:256-275) without a
GPU, and the kernel against the numpy restatement tests/crop_ref.py, bit for bit in its three output types."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from automl_amd import _lib, effnetv2_train as et, v2_preprocessing as vp
from tests import crop_ref as cr
from tests import randaug_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the staged schedule ---------------------------------------------------------------------------------------------------
def test_progressive_stages_of_the_named_models():
  s = et.progressive_stages('efficientnetv2-s', 350)
  assert [d['image_size'] for d in s] == [171, 214, 257, 300]
  assert [(d['start_epoch'], d['end_epoch']) for d in s] == [(0, 87), (87, 175), (175, 262), (262, 350)]
  assert np.array_equal([d['ra_magnitude'] for d in s], np.linspace(5, 10, 4))
  assert all(d['mixup_alpha'] == 0 and d['cutmix_alpha'] == 0 for d in s)
  m = et.progressive_stages('efficientnetv2-m', 350)
  assert [d['image_size'] for d in m] == [192, 256, 320, 384]
  assert np.array_equal([d['mixup_alpha'] for d in m], np.linspace(0, 0.2, 4))
  assert np.array_equal([d['cutmix_alpha'] for d in m], np.linspace(0, 0.2, 4))
  assert np.array_equal([d['ra_magnitude'] for d in m], np.linspace(5, 15, 4))
  assert set(m[0]) == {'start_epoch', 'end_epoch', 'image_size', 'ra_magnitude', 'mixup_alpha', 'cutmix_alpha'}


def test_progressive_stages_without_schedule_and_without_stages():
  m = et.progressive_stages('efficientnetv2-m', 350, sched=False)
  assert [d['image_size'] for d in m] == [192, 256, 320, 384]
  assert all(d['ra_magnitude'] == 15 and d['mixup_alpha'] == 0.2 and d['cutmix_alpha'] == 0.2 for d in m)
  one = et.progressive_stages('efficientnetv2-m', 350, stages=0)
  assert one == [dict(start_epoch=0, end_epoch=350, image_size=384, ra_magnitude=15.0, mixup_alpha=0.2, cutmix_alpha=0.2)]
  # a falsy ibase is train_size / 2 (main_tf2.py:258): 150 + 150 * ratio for efficientnetv2-s
  assert [d['image_size'] for d in et.progressive_stages('efficientnetv2-s', 10, ibase=0)] == [187, 225, 262, 300]
  assert [d['image_size'] for d in et.progressive_stages('efficientnetv2-s', 10, stages=2, ibase=100)] == [200, 300]


# ---- preprocess_for_eval ---------------------------------------------------------------------------------------------------
def test_eval_rows():
  # float32(224 / 256) = 0.875; 0.875 * 375 = 328.125 -> 328; (375 - 328) // 2 = 23, (500 - 328) // 2 = 86
  assert vp.eval_rows([[375, 500]], 224).tolist() == [[375, 500, 23, 86, 328, 328, 0, 0]]
  # 384 >= 320: no crop
  assert vp.eval_rows([[375, 500]], 384).tolist() == [[375, 500, 0, 0, 375, 500, 0, 0]]
  # ... unless asked for: float32(384 / 416) = 0.9230769..., * 375 = 346.15 -> 346; (375 - 346) // 2 = 14, (500 - 346) // 2 = 77
  assert vp.eval_rows([[375, 500]], 384, 'crop').tolist() == [[375, 500, 14, 77, 346, 346, 0, 0]]
  # min(h, w) = 1: int(0.875 * 1) = 0, an empty crop that the reference's crop_to_bounding_box refuses; here the one pixel,
  # at ((1 - 1) // 2, (50 - 1) // 2)
  assert vp.eval_rows([[1, 50]], 224).tolist() == [[1, 50, 0, 24, 1, 1, 0, 0]]
  assert vp.eval_rows([[50, 1], [375, 500]], 224).tolist() == [[50, 1, 24, 0, 1, 1, 0, 0], [375, 500, 23, 86, 328, 328, 0, 0]]


# ---- the crop sampler: properties, not a stream ------------------------------------------------------------------------------
SAMPLER_SIZES = [(1, 1), (7, 500), (500, 7), (375, 500), (32, 32)]


@pytest.fixture(scope='module')
def sampled():
  """20 000 draws, 4 000 per size, from one generator -> {size: int array [4000, 4] of (y, x, h, w)}."""
  rng = vp.crop_rng(11)
  return {hw: np.array([vp.sample_distorted_bounding_box(rng, *hw) for _ in range(4000)]) for hw in SAMPLER_SIZES}


@pytest.mark.parametrize('hw', SAMPLER_SIZES)
def test_sampled_boxes_lie_inside_and_within_the_ranges(sampled, hw):
  height, width = hw
  y, x, h, w = sampled[hw].T.astype(np.float64)
  assert (h >= 1).all() and (w >= 1).all() and (y >= 0).all() and (x >= 0).all()
  assert (y + h <= height).all() and (x + w <= width).all()
  whole = (h == height) & (w == width) & (y == 0) & (x == 0)
  area = height * width
  # each side is an integer within one pixel of its real-valued size: area and ratio hold up to that rounding
  area_ok = ((h - 1) * (w - 1) <= 1.0 * area) & ((h + 1) * (w + 1) >= 0.05 * area)
  ratio_ok = ((w - 1) / (h + 1) <= 1.33) & ((w + 1) / np.maximum(h - 1, 1e-9) >= 0.75)
  assert (whole | (area_ok & ratio_ok)).all(), sampled[hw][~(whole | (area_ok & ratio_ok))][:5]


def test_sampler_rarely_falls_back_and_spreads_over_the_areas(sampled):
  y, x, h, w = sampled[(375, 500)].T
  whole = (h == 375) & (w == 500)
  assert whole.mean() < 0.01
  frac = (h * w / (375.0 * 500.0)).mean()
  print('mean area fraction at 375 x 500: %.4f, fallback share %.4f' % (frac, whole.mean()))
  assert 0.3 < frac < 0.75      # a sanity band on "uniform in the height between the two area bounds", not a measurement
  assert len({tuple(b) for b in sampled[(375, 500)]}) > 3900 and x.max() > 250 and y.max() > 180


def test_same_seed_same_rows_and_the_state_round_trip():
  sizes = [[375, 500], [32, 32], [7, 500], [100, 60]]
  a, b = vp.crop_rng(5), vp.crop_rng(5)
  first = vp.train_rows(a, sizes)
  assert np.array_equal(first, vp.train_rows(b, sizes))
  assert first.dtype == np.int32 and first.shape == (4, 8) and np.array_equal(first[:, :2], sizes)
  assert not np.array_equal(first, vp.train_rows(vp.crop_rng(6), sizes))
  words = et._pack_rng_state(a)
  c = vp.crop_rng(99)
  et._unpack_rng_state(c, words)
  assert np.array_equal(vp.train_rows(a, sizes), vp.train_rows(c, sizes))


def test_train_rows_transformations():
  sizes = [[375, 500], [32, 32], [1, 1]]
  rows = vp.train_rows(vp.crop_rng(0), sizes, '')
  assert rows.tolist() == [[375, 500, 0, 0, 375, 500, 0, 0], [32, 32, 0, 0, 32, 32, 0, 0], [1, 1, 0, 0, 1, 1, 0, 0]]
  crop_only = vp.train_rows(vp.crop_rng(0), [[375, 500]] * 64, 'crop')
  assert not crop_only[:, 6].any() and (crop_only[:, 4] < 375).any()
  flips = vp.train_rows(vp.crop_rng(3), [[8, 8]] * 20000, 'flip')
  assert np.array_equal(flips[:, 2:6], np.tile([0, 0, 8, 8], (20000, 1))) and set(flips[:, 6]) == {0, 1}
  assert abs(flips[:, 6].mean() - 0.5) <= 0.02


def test_clamp_rows():
  rows = [[37, 53, -4, 60, 100, 0, 7, 9], [99, 0, 5, 5, 5, 5, 0, 0], [10, 10, 9, 9, 5, 5, -1, 0]]
  assert vp.clamp_rows(rows, 37, 53).tolist() == [[37, 53, 0, 52, 37, 1, 1, 0], [37, 1, 5, 0, 5, 1, 0, 0],
                                                   [10, 10, 9, 9, 1, 1, 1, 0]]


def test_pad_batch():
  rng = np.random.default_rng(0)
  ims = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((5, 9), (7, 3))]
  raw, sizes = vp.pad_batch(ims)
  assert raw.dtype == torch.uint8 and tuple(raw.shape) == (2, 7, 9, 3) and sizes.tolist() == [[5, 9], [7, 3]]
  assert np.array_equal(raw[0, :5, :9].numpy(), ims[0]) and np.array_equal(raw[1, :7, :3].numpy(), ims[1])
  assert int(raw[0, 5:].sum()) == 0 and int(raw[1, :, 3:].sum()) == 0
  assert tuple(vp.pad_batch(ims, (8, 16))[0].shape) == (2, 8, 16, 3)
  with pytest.raises(ValueError, match='does not fit'):
    vp.pad_batch(ims, (6, 16))


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_header_struct_and_stubs():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'edet_hip.h')).read(), flags=re.S)
  m = re.search(r'\bint\s+edet_crop_resize\s*\(([^;]*?)\)\s*;', src, flags=re.S)
  assert m, 'include/edet_hip.h does not declare edet_crop_resize'
  args = [a.strip() for a in m.group(1).split(',')]
  bound = _lib.SIGNATURES['edet_crop_resize']
  assert len(args) == len(bound) == 10
  assert [('*' in a) for a in args] == [t is ctypes.c_void_p for t in bound], args
  fields = re.search(r'typedef struct edet_crop_image \{(.*?)\} edet_crop_image_t;', src, flags=re.S).group(1)
  names = [n.strip() for part in fields.split(';') if part.strip() for n in part.replace('int32_t', '').split(',')]
  assert tuple(names) == tuple(n for n, _ in _lib.CropImage._fields_) == vp.ROW_FIELDS
  assert ctypes.sizeof(_lib.CropImage) == 32


def test_plan_stubs_are_current(tmp_path):
  spec = importlib.util.spec_from_file_location('gen_plan_stubs', os.path.join(ROOT, 'scripts', 'gen_plan_stubs.py'))
  gen = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(gen)
  out = tmp_path / 'plan_stubs.inc'
  out.write_text(gen.generate())
  committed = open(os.path.join(ROOT, 'automl_amd', 'csrc', 'plan_stubs.inc')).read()
  assert out.read_text() == committed
  assert 'edet_crop_resize' in committed


# ---- the kernel against the restatement ------------------------------------------------------------------------------------
CANVAS = (37, 53)
IMAGE_SIZES = [(37, 53), (1, 1), (2, 50), (30, 3), (16, 16)]


def _canvas(sizes, seed):
  """Random images in the top-left corners of a canvas filled with another random pattern (which no valid crop may read)."""
  rng = np.random.default_rng(seed)
  raw = rng.integers(0, 256, (len(sizes),) + CANVAS + (3,)).astype(np.uint8)
  return raw


def _scenarios(sizes):
  """name -> rows [B, 8] (flip 0) for images of `sizes`."""
  whole = [[h, w, 0, 0, h, w, 0, 0] for h, w in sizes]
  one = [[h, w, h - 1, w // 2, 1, 1, 0, 0] for h, w in sizes]
  corner = [[h, w, h // 2, w // 3, h - h // 2, w - w // 3, 0, 0] for h, w in sizes]
  three = [[h, w, max(h - 3, 0) // 2, max(w - 3, 0) // 2, min(h, 3), min(w, 3), 0, 0] for h, w in sizes]
  return {'whole': np.array(whole, np.int32), 'one_pixel': np.array(one, np.int32), 'bottom_right': np.array(corner, np.int32),
          'three': np.array(three, np.int32)}


def _compare(raw, rows, out_hw, what):
  dev = torch.from_numpy(raw).cuda()
  want32 = None
  for kind in cr.KINDS:
    got = vp.crop_resize(dev, rows, out_hw, cr.TORCH_DTYPE[kind])
    torch.cuda.synchronize()
    want = cr.crop_resize_ref(raw, rows, out_hw[0], out_hw[1], kind)
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape)
    same = torch.equal(got.cpu(), want)
    if not same:
      d = (got.cpu().float() - want.float()).abs()
      raise AssertionError('%s, %s, output %s: %d of %d values differ, worst %g at %s' % (
          what, kind, out_hw, int((d != 0).sum()), d.numel(), float(d.max()), np.unravel_index(int(d.argmax()), d.shape)))


# (32, 32): three 4-pixel vector stores per thread; (8, 8): the reduction of the full canvas; (10, 7) and (5, 70): rows that
# are no multiple of 4, one value per store; (1, 1); (3, 261) and (2, 264): rows longer than the 256 pixels one wave covers,
# the second stretch partly and wholly filled, scalar and vector stores
OUT_SIZES = [(32, 32), (8, 8), (10, 7), (5, 70), (1, 1), (3, 261), (2, 264)]


@pytest.mark.gpu
@pytest.mark.parametrize('out_hw', OUT_SIZES, ids=lambda s: '%dx%d' % s)
def test_kernel_equals_the_restatement(out_hw):
  """Batch 5 on a 37 x 53 canvas, every scenario with the flip off, on, and alternating; once more with the images in
  reverse order, so that the crop ending at the bottom-right pixel of the full-canvas image reads the last byte of the batch."""
  for order, sizes in (('forward', IMAGE_SIZES), ('reversed', IMAGE_SIZES[::-1])):
    raw = _canvas(sizes, 7 if order == 'forward' else 8)
    for name, rows in _scenarios(sizes).items():
      for flips in ([0] * 5, [1] * 5, [0, 1, 0, 1, 1]):
        r = rows.copy()
        r[:, 6] = flips
        _compare(raw, r, out_hw, '%s / %s / flip %s' % (order, name, flips))


@pytest.mark.gpu
def test_out_of_range_rows_are_clamped():
  raw = _canvas(IMAGE_SIZES, 9)
  rows = np.array([[37, 53, -5, 4, 20, 20, 0, 0],        # a negative crop_y
                   [1, 1, 0, 0, 1, 1, 1, 0],
                   [2, 50, 1, 10, 40, 45, 5, 0],         # crop_h and crop_w past the image; flip = 5 is "on"
                   [400, 3, 10, -2, 500, 9, 0, 0],       # height above the canvas
                   [16, 16, 99, 99, 0, -3, 1, 0]], np.int32)
  clamped = vp.clamp_rows(rows, *CANVAS)
  assert clamped.tolist() == [[37, 53, 0, 4, 20, 20, 0, 0], [1, 1, 0, 0, 1, 1, 1, 0], [2, 50, 1, 10, 1, 40, 1, 0],
                              [37, 3, 10, 0, 27, 3, 0, 0], [16, 16, 15, 15, 1, 1, 1, 0]]
  dev = torch.from_numpy(raw).cuda()
  for out_hw in ((32, 32), (10, 7)):
    _compare(raw, rows, out_hw, 'out of range')
    for kind in cr.KINDS:
      a = vp.crop_resize(dev, rows, out_hw, cr.TORCH_DTYPE[kind])
      b = vp.crop_resize(dev, clamped, out_hw, cr.TORCH_DTYPE[kind])
      assert torch.equal(a, b), (out_hw, kind)


@pytest.mark.gpu
@pytest.mark.parametrize('hw', [(12, 20), (7, 9), (1, 1)], ids=lambda s: '%dx%d' % s)
def test_identity(hw):
  """Canvas = output size, the whole image, no flip: the input bytes, or their normalisation.  (1 x 1, batch 1: a batch of
  three bytes, read without the 4-byte load.)"""
  batch = 1 if hw == (1, 1) else 3
  raw = np.random.default_rng(4).integers(0, 256, (batch,) + hw + (3,)).astype(np.uint8)
  dev = torch.from_numpy(raw).cuda()
  rows = vp.whole_rows(batch, *hw)
  assert np.array_equal(vp.crop_resize(dev, rows, hw).cpu().numpy(), raw)
  f32 = vp.crop_resize(dev, rows, hw, torch.float32)
  assert np.array_equal(f32.cpu().numpy(), rr.normalise(raw))
  bf16 = vp.crop_resize(dev, rows, hw, torch.bfloat16)
  assert torch.equal(bf16.cpu(), torch.from_numpy(rr.normalise(raw)).to(torch.bfloat16))
  # rows already on the device are used as they are; a given output buffer is filled
  out = torch.empty((batch,) + hw + (3,), dtype=torch.float32, device='cuda')
  assert vp.crop_resize(dev, torch.from_numpy(rows).cuda(), hw, out=out) is out and torch.equal(out, f32)


@pytest.mark.gpu
def test_host_checks():
  dev = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device='cuda')
  rows = torch.from_numpy(vp.whole_rows(2, 4, 4)).cuda()
  out = torch.empty((2, 4, 4, 3), dtype=torch.uint8, device='cuda')
  s = torch.cuda.current_stream().cuda_stream
  for args, what in (((None, 2, 4, 4, rows.data_ptr(), out.data_ptr(), 4, 4, _lib.EDET_U8, s), 'null'),
                     ((dev.data_ptr(), 2, 4, 4, None, out.data_ptr(), 4, 4, _lib.EDET_U8, s), 'null'),
                     ((dev.data_ptr(), 0, 4, 4, rows.data_ptr(), out.data_ptr(), 4, 4, _lib.EDET_U8, s), 'batch 0'),
                     ((dev.data_ptr(), 65536, 4, 4, rows.data_ptr(), out.data_ptr(), 4, 4, _lib.EDET_U8, s), 'batch 65536'),
                     ((dev.data_ptr(), 2, 4, 4, rows.data_ptr(), out.data_ptr(), 0, 4, _lib.EDET_U8, s), 'output 0 x 4'),
                     ((dev.data_ptr(), 2, 30000, 30000, rows.data_ptr(), out.data_ptr(), 4, 4, _lib.EDET_U8, s), 'too large'),
                     ((dev.data_ptr(), 2, 4, 4, rows.data_ptr(), out.data_ptr(), 4, 4, 7, s), 'bad out_dtype')):
    with pytest.raises(_lib.EdetError, match=what):
      _lib.call('edet_crop_resize', *args)
  with pytest.raises(ValueError, match='uint8'):
    vp.crop_resize(dev.float(), rows, 4)
  with pytest.raises(ValueError, match='rows are'):
    vp.crop_resize(dev, rows[:1].contiguous(), 4)
