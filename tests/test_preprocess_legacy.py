"""The legacy EfficientNet input pipeline (automl_amd/preprocess_legacy.py): its rows functions and the restatement chain
(tests/bicubic_ref.py, tests/autoaug_ref.py) against the reference module executed unmodified on a stand-in
(tests/golden/reference_legacy.npz, made by tests/golden/make_golden_legacy.py) without a device; the sampler's
min_object_covered; and preprocess_image on the device against the restatement chain."""
import os

import numpy as np
import pytest
import torch

from automl_amd import autoaugment as aa, preprocess_legacy as pl, v2_preprocessing as vp
from tests import autoaug_ref as ar
from tests import bicubic_ref as br
from tests import randaug_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32


@pytest.fixture(scope='module')
def golden():
  return dict(np.load(os.path.join(HERE, 'golden', 'reference_legacy.npz')))


@pytest.fixture(scope='module')
def v0_table():
  return ar.table_of(dict(np.load(os.path.join(HERE, 'golden', 'reference_autoaug.npz'))), 'v0')


class QueueRng(object):
  """A generator stand-in whose random() hands out queued uniforms (the flip draws of the fixture)."""

  def __init__(self, values):
    self.values = list(values)

  def random(self):
    return self.values.pop(0)


def chain(image, row, target, augment=None, aug=None, table=None):
  """The restatement chain for one image and one edet_crop_image_t row -> float32 [target, target, 3], normalised."""
  raw = image[None]
  v = br.resized_crops(raw, np.asarray(row, np.int32)[None], target, target)[0]
  if augment:
    u8 = np.clip(v, f32(0), f32(255)).astype(np.uint8)
    if augment == 'autoaug':
      u8 = ar.autoaugment(u8[None], aug, table)[0]
    else:
      draws, magnitude = aug
      u8 = rr.randaugment(u8[None], draws, magnitude)[0]
    v = u8.astype(np.float32)
  return (v - pl.MEAN_RGB) / pl.STDDEV_RGB


def test_eval_rows_and_outputs_equal_the_reference(golden):
  sizes = golden['eval/sizes']
  assert {int(min(h, w)) for h, w in sizes} >= {1, 2, 33} and {int(h) % 2 for h, _ in sizes} == {0, 1}
  for target in golden['eval/targets']:
    target = int(target)
    rows = pl.legacy_eval_rows(sizes, target)
    windows = golden['eval/%d/windows' % target]
    for (h, w), row, win in zip(sizes, rows, windows):
      assert row[:2].tolist() == [h, w] and row[6:].tolist() == [0, 0]
      if min(h, w) == 1 or win[2] == 0:
        # the reference asks decode_and_crop_jpeg for an empty window, which the op refuses; here the crop is the one pixel
        assert win[2] == 0 and win[3] == 0 and row[4:6].tolist() == [1, 1]
        assert row[2:4].tolist() == [((h - 1) + 1) // 2, ((w - 1) + 1) // 2]
        continue
      assert row[2:6].tolist() == win.tolist(), (h, w, target)
      want = golden['eval/%d/out/%dx%d' % (target, h, w)]
      assert np.array_equal(chain(golden['image/%dx%d' % (h, w)], row, target), want), (h, w, target)
  # the `+ 1` of the offsets, unlike preprocess_for_eval's of the V2 pipeline: an odd margin rounds up
  row = pl.legacy_eval_rows([[34, 34]], 8)[0]
  c = int(f32(8 / 40) * f32(34))
  assert c == 6 and row[2:6].tolist() == [14, 14, 6, 6]
  row = pl.legacy_eval_rows([[33, 40]], 8)[0]
  assert row[2:6].tolist() == [(33 - 6 + 1) // 2, (40 - 6 + 1) // 2, 6, 6] == [14, 17, 6, 6]
  assert vp.eval_rows([[33, 40]], 8)[0][2:4].tolist() == [13, 17]


def test_train_rows_and_outputs_equal_the_reference(golden, v0_table, monkeypatch):
  target = int(golden['train/target'])
  seen_bad = seen_flip = 0
  for name in golden['train/names']:
    name = str(name)
    g = lambda part: golden['train/%s/%s' % (name, part)]
    h, w = (int(v) for v in g('size'))
    box = tuple(int(v) for v in g('box'))
    calls = []

    def sampler(rng, height, width, **kw):
      calls.append((height, width, kw))
      return box
    monkeypatch.setattr(pl, 'sample_distorted_bounding_box', sampler)
    row = pl.legacy_train_rows(QueueRng([float(g('flip_u'))]), [[h, w]], target)[0]
    # the sampler's keyword values are the reference's (:88-98), on one box: the whole image
    (sh, sw, kw), = calls
    smp = g('sampler')
    assert (sh, sw) == (h, w) and g('sampler_boxes').reshape(-1).tolist() == [0.0, 0.0, 1.0, 1.0]
    assert [kw['min_object_covered'], kw['aspect_ratio_range'][0], kw['aspect_ratio_range'][1], kw['area_range'][0],
            kw['area_range'][1], kw['max_attempts']] == smp[:6].tolist() and smp[6] == 1.0
    windows = g('windows')
    bad = box[2:] == (h, w)
    assert len(windows) == (2 if bad else 1) and windows[0].tolist() == list(box)
    assert row[2:6].tolist() == windows[-1].tolist(), name      # the fallback's window when the box is the whole image
    if bad:
      assert row[2:6].tolist() == list(pl.center_crop_window(h, w, target))
    assert row[6] == int(float(g('flip_u')) < 0.5)
    seen_bad += bad
    seen_flip += int(row[6])
    augment = str(g('augment')) or None
    aug = None
    if augment == 'autoaug':
      sub, u0, u1, sign = g('autoaug')
      aug = (np.array([int(sub)], np.int32), np.array([[u0], [u1]], np.float32), np.full((2, 1), sign, np.float32))
    elif augment == 'randaug':
      r = g('randaug')
      layers = int(r[0])
      aug = ((r[2:2 + layers].astype(np.int32).reshape(layers, 1), r[2 + layers:].astype(np.float32).reshape(layers, 1),
              np.zeros((layers, 1)), np.zeros((layers, 1))), float(r[1]))
    got = chain(golden['image/%dx%d' % (h, w)], row, target, augment, aug, v0_table)
    assert np.array_equal(got, g('out')), name
  assert seen_bad >= 3 and seen_flip >= 4
  assert str(golden['invalid_name_message']) == 'Invalid value for augment_name: v0'


def test_sampler_min_object_covered():
  kw = dict(area_range=(0.08, 1.0), aspect_ratio_range=(3. / 4, 4. / 3.), max_attempts=10)
  # the default consumes and returns exactly what it did: the same boxes, the same generator state afterwards
  a, b = np.random.default_rng(5), np.random.default_rng(5)
  for h, w in [(375, 500), (33, 40), (500, 20), (7, 9)] * 25:
    assert vp.sample_distorted_bounding_box(a, h, w) == vp.sample_distorted_bounding_box(b, h, w, min_object_covered=0.0)
  assert a.bit_generator.state == b.bit_generator.state
  rng = np.random.default_rng(6)
  whole = small = 0
  for k in range(600):
    h, w = (375, 500) if k % 2 else (120, 90)
    y, x, bh, bw = vp.sample_distorted_bounding_box(rng, h, w, min_object_covered=0.1, **kw)
    assert 0 <= y and 0 <= x and bh >= 1 and bw >= 1 and y + bh <= h and x + bw <= w
    if (bh, bw) == (h, w):
      whole += 1
      continue
    assert bh * bw >= 0.1 * h * w - 1e-9 and bh * bw <= h * w
    assert 3. / 4 - 0.02 <= bw / bh <= 4. / 3 + 0.02, (bw, bh)
    small += bh * bw < 0.2 * h * w
  assert small > 20 and whole < 60
  # a range that only min_object_covered can refuse: every attempt fails, the whole image comes back
  assert vp.sample_distorted_bounding_box(np.random.default_rng(1), 100, 100, area_range=(0.08, 0.09), min_object_covered=0.1,
                                          max_attempts=10) == (0, 0, 100, 100)
  assert vp.sample_distorted_bounding_box(np.random.default_rng(1), 100, 100, area_range=(0.08, 0.09), max_attempts=10) != (0, 0, 100, 100)


def test_train_rows_stream_and_fallback():
  sizes = [[375, 500], [33, 40], [1, 1], [2, 2], [500, 375]] * 20
  a = pl.legacy_train_rows(np.random.default_rng(3), sizes, 224)
  b = pl.legacy_train_rows(np.random.default_rng(3), sizes, 224)
  assert np.array_equal(a, b) and a.dtype == np.int32 and a.shape == (100, 8)
  assert np.array_equal(vp.clamp_rows(a, 500, 500), a)
  assert 20 < a[:, 6].sum() < 80
  # a 1 x 1 image can only give the whole image: always the fallback, whose window is the pixel itself
  assert all(r.tolist()[:6] == [1, 1, 0, 0, 1, 1] for r in a[2::5])
  # per image: the window, then the flip -- train_crop_window and rng.random() in turn reproduce the rows
  rng = np.random.default_rng(3)
  for (h, w), row in zip(sizes[:10], a[:10]):
    win = pl.train_crop_window(rng, h, w, 224)
    assert row.tolist() == [h, w] + list(win) + [int(rng.random() < 0.5), 0]
  flips = pl.legacy_flip_rows(np.random.default_rng(4), sizes)
  assert np.array_equal(flips[:, :6], vp.clamp_rows(np.array([[h, w, 0, 0, h, w, 0, 0] for h, w in sizes]), 500, 500)[:, :6])
  assert 20 < flips[:, 6].sum() < 80


def test_value_errors():
  x = np.zeros((2, 8, 8, 3), np.uint8)
  for name in ('v0', 'autoaugment', 'effnetv1_autoaug', 'ra_aa'):
    with pytest.raises(ValueError, match='Invalid value for augment_name: %s' % name):      # (before the device)
      pl.preprocess_image(x, None, 8, is_training=True, augment_name=name)
  with pytest.raises(ValueError, match='image_dtype'):
    pl.preprocess_image(x, None, 8, image_dtype=torch.float16)
  with pytest.raises(ValueError, match='image_size'):
    pl.legacy_eval_rows([[4, 4]], 0)
  with pytest.raises(ValueError, match='inside the 8 x 8 canvas'):
    pl.preprocess_image(x, [[9, 8], [8, 8]], 8)
  with pytest.raises(ValueError, match='uint8'):
    pl.preprocess_image(x.astype(np.float32), None, 8)
  with pytest.raises(ValueError, match='magnitude'):
    pl.preprocess_image(x, None, 8, is_training=True, augment_name='randaug', randaug_magnitude=30)


# ------------------------------------------------------------------------------------ GPU
SIZES = [(40, 56), (33, 20), (12, 56), (40, 9), (25, 31), (1, 1), (38, 50), (17, 17)]


def _batch(seed=9):
  rng = np.random.default_rng(seed)
  raw = rng.integers(0, 256, (len(SIZES), 40, 56, 3)).astype(np.uint8)
  return raw, np.array(SIZES, np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [None, torch.bfloat16])
def test_preprocess_image_equals_the_restatement_chain(v0_table, dtype):
  raw, sizes = _batch()
  target, b = 16, len(SIZES)
  kind = 'bf16' if dtype is torch.bfloat16 else 'f32'
  ms = np.concatenate(pl.NORM)
  # eval
  got = pl.preprocess_image(raw, sizes, target, image_dtype=dtype)
  rows = pl.legacy_eval_rows(sizes, target)
  assert torch.equal(got.cpu(), br.crop_resize_ref(raw, rows, target, target, kind, ms))
  # train, each augment_name; the draws come from the generator: rows first, then the augmentation's
  for augment in (None, 'autoaug', 'randaug'):
    got = pl.preprocess_image(torch.from_numpy(raw), sizes, target, is_training=True, image_dtype=dtype, augment_name=augment,
                              randaug_num_layers=2, randaug_magnitude=9, rng=np.random.default_rng(23))
    rng = np.random.default_rng(23)
    rows = pl.legacy_train_rows(rng, sizes, target)
    assert rows[:, 6].any() and not rows[:, 6].all()
    if augment is None:
      want = br.crop_resize_ref(raw, rows, target, target, kind, ms)
    else:
      u8 = br.crop_resize_ref(raw, rows, target, target, 'u8').numpy()
      if augment == 'autoaug':
        u8 = ar.autoaugment(u8, aa.autoaug_draws(rng, b, 'v0'), v0_table)
      else:
        u8 = rr.randaugment(u8, aa.randaug_draws(rng, b, 2), 9)
      want = br.normalize_u8(u8, kind, ms)
    assert got.dtype == want.dtype and torch.equal(got.cpu(), want), (augment, kind)
  # forced rows and draws
  rows = pl.legacy_train_rows(np.random.default_rng(2), sizes, target)
  draws = aa.autoaug_draws(np.random.default_rng(3), b, 'v0')
  got = pl.preprocess_for_train(raw, sizes, target, 'autoaug', image_dtype=dtype, rows=rows, draws=draws)
  u8 = ar.autoaugment(br.crop_resize_ref(raw, rows, target, target, 'u8').numpy(), draws, v0_table)
  assert torch.equal(got.cpu(), br.normalize_u8(u8, kind, ms))
