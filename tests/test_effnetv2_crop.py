"""Crop, resize and flip on the device in the EfficientNetV2 classifier trainer (effnetv2_train.TrainableModel(image_size=...)
on V2Engine.crop_batch) and the staged sizes: identity rows against today's steps, a real crop against a plain model fed the
restatement's output, graph replay against eager with everything on and a changing canvas, set_image_size against a fresh
model resumed from the saved state, test_step, set_stage.  The tiny configuration of tests/test_effnetv2_randaug.py
(efficientnetv2-b0, 24 classes, batch 8)."""
import math

import numpy as np
import pytest
import torch

from automl_amd import autoaugment as aa, effnetv2_train, v2_preprocessing as vp
from tests import crop_ref as cr
from tests import randaug_ref as rr

MODEL, OVER, SIZE, NC, BATCH = 'efficientnetv2-b0', 'num_classes=24', 32, 24, 8
MIXED_SIZES = [(40, 56), (33, 20), (12, 56), (40, 9), (25, 31), (1, 1), (38, 50), (17, 17)]


def _net(**kw):
  args = dict(learning_rate=0.01, weight_decay=1e-5, label_smoothing=0.1, seed=4)
  args.update(kw)
  return effnetv2_train.TrainableModel(MODEL, OVER, **args)


def _raw(seed, canvas, sizes=None, batch=BATCH):
  """(canvas batch uint8, sizes int32 [B, 2], labels)."""
  rng = np.random.default_rng(seed)
  raw = rng.integers(0, 256, (batch,) + tuple(canvas) + (3,)).astype(np.uint8)
  sizes = np.array(sizes if sizes is not None else [canvas] * batch, np.int32)
  return raw, sizes, rng.integers(0, NC, batch)


def _same_state(a, b, keys=('params_flat', 'velocity', 'adam_v', 'state_flat')):
  for key in keys:
    assert torch.equal(getattr(a.engine.arena, key), getattr(b.engine.arena, key)), key


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_identity_rows_equal_todays_steps(dtype):
  """A 32 x 32 canvas taken whole and unflipped at image_size 32 is the input itself: with RandAugment (identity draws) the
  step is today's uint8 step, without it today's float step on (x - 128) / 128 -- returned dict and arena, bit for bit."""
  raw, sizes, labels = _raw(3, (SIZE, SIZE))
  rows = vp.whole_rows(BATCH, SIZE, SIZE)
  for augname in ('randaug', None):
    crop = _net(use_graph=False, dtype=dtype, augname=augname, image_size=SIZE, transformations='')
    crop.force_crop_rows(rows)
    today = _net(use_graph=False, dtype=dtype, augname=augname)
    if augname:
      crop.force_randaug_draws(aa.identity_draws(BATCH, 2))
      today.force_randaug_draws(aa.identity_draws(BATCH, 2))
    got = crop.train_step(((raw, sizes), labels))
    want = today.train_step((raw if augname else rr.normalise(raw), labels))
    torch.cuda.synchronize()
    assert got == want, (augname, got, want)
    _same_state(crop, today)
    # transformations='' draws exactly these rows by itself
    crop.force_crop_rows(None)
    crop.train_step(({'image': raw}, {'label': labels}))
    assert np.array_equal(crop.engine.crop_rows.cpu().numpy(), rows)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_real_crop_equals_a_plain_step_on_the_restatement(dtype):
  raw, sizes, labels = _raw(5, (40, 56), MIXED_SIZES)
  net = _net(use_graph=False, dtype=dtype, image_size=SIZE)
  got = net.train_step(((raw, sizes), labels))
  torch.cuda.synchronize()
  rows = vp.train_rows(vp.crop_rng(4), sizes)      # what the model's own generator hands its first step
  assert np.array_equal(net.engine.crop_rows.cpu().numpy(), rows)
  assert rows[:, 6].any() and not rows[:, 6].all() and (rows[:, 4] < sizes[:, 0]).any()
  kind = 'f32' if dtype == 'f32' else 'bf16'
  fed = cr.crop_resize_ref(raw, rows, SIZE, SIZE, kind)
  assert torch.equal(net.engine.buf('crop:images', (BATCH, SIZE, SIZE, 3), cr.TORCH_DTYPE[kind]).cpu(), fed)
  plain = _net(use_graph=False, dtype=dtype)
  want = plain.train_step((fed.float().numpy(), labels))
  torch.cuda.synchronize()
  assert got == want, (got, want)
  _same_state(net, plain)


@pytest.mark.gpu
def test_everything_on_graph_equals_eager_over_a_changing_canvas():
  """Crop + RandAugment + mixup + cutmix, bf16, four steps; the canvas changes shape at step 3, so the graph run is
  eager, captured, eager, captured."""
  data = [_raw(20, (40, 56), MIXED_SIZES), _raw(21, (40, 56), MIXED_SIZES), _raw(22, (48, 40)), _raw(23, (48, 40))]
  runs = []
  for use_graph in (True, False):
    net = _net(use_graph=use_graph, image_size=SIZE, augname='randaug', ra_magnitude=9, mixup_alpha=0.4, cutmix_alpha=0.4)
    outs, rows, graphs = [], [], []
    for raw, sizes, labels in data:
      outs.append(net.train_step(((raw, sizes), labels)))
      rows.append(net.engine.crop_rows.cpu().clone())
      graphs.append(None if net._graph is None else (net._graph['steps'], net._graph['graph'] is not None))
    torch.cuda.synchronize()
    runs.append((net, outs, rows, graphs))
  (g, og, rg, gg), (e, oe, re_, ge) = runs
  assert gg == [(1, False), (2, True), (1, False), (2, True)] and ge == [None] * 4
  assert og == oe, (og, oe)
  assert all(math.isfinite(o['loss']) for o in og)
  _same_state(g, e)
  assert all(torch.equal(a, b) for a, b in zip(rg, re_)) and not torch.equal(rg[0], rg[1])
  for key in (('crop:u8', (BATCH, SIZE, SIZE, 3), torch.uint8), ('randaug:images', (BATCH, SIZE, SIZE, 3), torch.bfloat16)):
    assert torch.equal(g.engine.buf(*key), e.engine.buf(*key)), key[0]
  assert torch.equal(g.engine.soft_labels, e.engine.soft_labels)
  images, _ = g.input_buffers()
  assert images.dtype == torch.uint8 and torch.equal(images.cpu(), torch.from_numpy(data[-1][0]))


@pytest.mark.gpu
def test_set_image_size_equals_a_fresh_model_resumed_from_the_state():
  data = [_raw(30 + k, (40, 56), MIXED_SIZES) for k in range(4)]
  step = lambda net, d: net.train_step(((d[0], d[1]), d[2]))
  kw = dict(use_graph=False, image_size=SIZE, augname='randaug', mixup_alpha=0.3)
  net = _net(**kw)
  first = step(net, data[0])
  state1, weights1 = net.get_optimizer_state(), net.get_weights()
  step(net, data[1])
  state, weights = net.get_optimizer_state(), net.get_weights()
  assert 'crop_rng_state' in state and 'randaug_rng_state' in state and 'mix_rng_state' in state
  arena = net.engine.arena
  net.set_image_size(48)
  want = [step(net, d) for d in data[2:]]
  assert net.engine.image_size == (48, 48) and net.engine.arena is arena and net.iterations == 4
  fresh = _net(**dict(kw, image_size=48))
  fresh.set_weights(weights)
  fresh.set_optimizer_state(state)
  got = [step(fresh, d) for d in data[2:]]
  torch.cuda.synchronize()
  assert got == want, (got, want)
  _same_state(net, fresh)
  assert torch.equal(net.engine.crop_rows, fresh.engine.crop_rows)
  # saved and resumed after step 1 at one size: the uninterrupted run
  again = _net(**kw)
  again.set_weights(weights1)
  again.set_optimizer_state(state1)
  step(again, data[1])
  for key, value in again.get_optimizer_state().items():
    assert np.array_equal(np.asarray(value), np.asarray(state[key])), key
  assert math.isfinite(first['loss'])
  # a model built without image_size has no new key and cannot be resized
  plain = _net(use_graph=False)
  plain.train_step((rr.normalise(data[0][0][:, :SIZE, :SIZE]), data[0][2]))
  assert 'crop_rng_state' not in plain.get_optimizer_state() and plain.engine.crop_rows is None
  with pytest.raises(ValueError, match='without image_size'):
    plain.set_image_size(48)


@pytest.mark.gpu
@pytest.mark.parametrize('eval_size', [None, 48])
def test_test_step_on_raw_images(eval_size):
  raw, sizes, labels = _raw(41, (40, 56), MIXED_SIZES)
  net = _net(use_graph=False, dtype='f32', image_size=SIZE, eval_image_size=eval_size, augname='randaug')
  before = effnetv2_train._pack_rng_state(net._crop_rng)
  got = net.test_step(((raw, sizes), labels))
  size = eval_size or SIZE
  rows = vp.eval_rows(sizes, size)
  assert np.array_equal(net.engine.crop_rows.cpu().numpy(), rows) and not rows[:, 6].any()
  assert np.array_equal(effnetv2_train._pack_rng_state(net._crop_rng), before)
  plain = _net(use_graph=False, dtype='f32')
  want = plain.test_step((cr.crop_resize_ref(raw, rows, size, size, 'f32').numpy(), labels))
  assert got == want, (got, want)
  # images that fill the canvas need no sizes
  full = net.test_step((raw, labels))
  assert full == plain.test_step((cr.crop_resize_ref(raw, vp.eval_rows([[40, 56]] * BATCH, size), size, size, 'f32').numpy(), labels))


@pytest.mark.gpu
def test_float_images_raise_and_sizes_are_checked():
  raw, sizes, labels = _raw(43, (40, 56), MIXED_SIZES)
  net = _net(use_graph=False, image_size=SIZE)
  with pytest.raises(ValueError, match=r'preprocessing\.py:22-55'):
    net.train_step(((raw.astype(np.float32), sizes), labels))
  bad = sizes.copy()
  bad[2] = (41, 56)
  with pytest.raises(ValueError, match='inside the 40 x 56 canvas'):
    net.train_step(((raw, bad), labels))
  assert net.iterations == 0


@pytest.mark.gpu
def test_set_stage_changes_size_magnitude_and_alphas_together():
  net = _net(use_graph=True, image_size=SIZE, augname='randaug', ra_magnitude=5)
  raw, sizes, labels = _raw(47, (40, 56), MIXED_SIZES)
  net.train_step(((raw, sizes), labels))
  net.train_step(((raw, sizes), labels))
  assert net._graph['graph'] is not None
  stage = dict(start_epoch=1, end_epoch=2, image_size=48, ra_magnitude=12.5, mixup_alpha=0.1, cutmix_alpha=0.2)
  net.set_stage(stage)
  assert (net.image_size, net.ra_magnitude, net.mixup_alpha, net.cutmix_alpha) == (48, 12.5, 0.1, 0.2) and net._graph is None
  out = net.train_step(((raw, sizes), labels))
  assert math.isfinite(out['loss']) and net.engine.image_size == (48, 48) and net.engine.n_mixup == BATCH // 2
  # a model without RandAugment takes a stage too: the magnitude is not its business
  plain = _net(image_size=SIZE)
  plain.set_stage(stage)
  assert plain.image_size == 48 and plain.mixup_alpha == 0.1
  for d in effnetv2_train.progressive_stages('efficientnetv2-s', 4):
    plain.set_stage(d)
  assert plain.image_size == 300


@pytest.mark.gpu
def test_one_step_at_the_first_stage_size_of_v2s():
  """171 = progressive_stages('efficientnetv2-s', ...)[0]['image_size']: an odd size through every stride-2 layer; batch 2,
  two steps so that the graph run replays its captured step once."""
  size = effnetv2_train.progressive_stages('efficientnetv2-s', 350)[0]['image_size']
  assert size == 171
  data = [_raw(50 + k, (200, 180), [(200, 180), (150, 97)], batch=2) for k in range(2)]
  runs = []
  for use_graph in (True, False):
    net = _net(use_graph=use_graph, image_size=size, augname='randaug')
    runs.append((net, [net.train_step(((raw, sizes), labels)) for raw, sizes, labels in data]))
  torch.cuda.synchronize()
  (g, og), (e, oe) = runs
  assert all(math.isfinite(o['loss']) for o in og + oe), (og, oe)
  assert g._graph['graph'] is not None
  assert og == oe, (og, oe)
  _same_state(g, e)
