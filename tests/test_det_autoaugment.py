"""Box-aware AutoAugment / RandAugment on the detector's input (automl_amd/det_autoaugment.py, csrc/det_autoaug.hip,
det_input.DetectionInput(autoaugment=...), EfficientDetNetTrain.set_autoaugment).

CPU: the numpy restatement tests/det_autoaug_ref.py against the executed reference
(tests/golden/reference_det_autoaugment.npz, written by tests/golden/make_golden_det_autoaugment.py) -- images equal as uint8,
boxes bit for bit as float32 -- and the host side.  GPU: the kernels against the restatement, bit for bit, and train_step_raw
with the switch on.  No tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

from automl_amd import det_autoaugment as daa, det_input, preprocess, train_lib
from tests import det_autoaug_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FIXTURE = []


def fixture():
  if not _FIXTURE:
    _FIXTURE.append(np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_det_autoaugment.npz')))
  return _FIXTURE[0]


def same_boxes(got, want, what):
  got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  off = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
  assert off.size == 0, (what, len(off), [(tuple(i), repr(got[tuple(i)]), repr(want[tuple(i)])) for i in off[:6]])


# ------------------------------------------------------------------------------------ CPU: restatement == executed reference
def test_restatement_reproduces_every_operation_case():
  fx = fixture()
  boxes = fx['boxes']
  seen = set()
  for key in ('a', 'b', 'c'):
    img = fx['image/' + key]
    for name, want, want_boxes, (box_u, cy_u, cx_u) in zip(fx['names/' + key], fx['cases/' + key], fx['case_boxes/' + key],
                                                          fx['case_draws/' + key]):
      op, level, sign = str(name).split('/')
      got, got_boxes = dr.apply_op(img, boxes, op, int(level[1:]), 1.0 if sign == 'p' else -1.0, cy_u, cx_u, box_u)
      assert got.dtype == np.uint8 and np.array_equal(got, want), (key, name, int((got != want).sum()))
      same_boxes(got_boxes, want_boxes, (key, name))
      seen.add((op, level))
  assert seen == {(op, 'l%d' % l) for op in dr.NAMES for l in (0, 2, 6, 10)}
  # the cases are not trivial: a translation pushes box 2 outside (_check_bbox_area fires), the zero-width box is widened
  names = list(fx['names/a'])
  moved = fx['case_boxes/a'][names.index('TranslateX_BBox/l2/p')]
  assert moved[2][1] == 0.0 and moved[2][3] == np.float32(0.05) and moved[0][3] < np.float32(0.8)
  assert not np.array_equal(fx['cases/a'][names.index('Contrast/l6/p')], fx['image/a'])


def test_restatement_reproduces_bbox_cutout_without_boxes():
  fx = fixture()
  got, got_boxes = dr.apply_op(fx['image/a'], np.zeros((0, 4), np.float32), 'BBox_Cutout', 10)
  assert np.array_equal(got, fx['noboxes/out']) and np.array_equal(got, fx['image/a']) and got_boxes.shape == (0, 4)


def policy_runs(fx, pname):
  return sorted({k.rsplit('/', 1)[0] for k in fx.files if k.startswith('run/%s/' % pname)})


@pytest.mark.parametrize('pname', ['test', 'v2', 'v3'])
def test_restatement_reproduces_the_policies(pname):
  fx = fixture()
  runs = policy_runs(fx, pname)
  table = dr.POLICIES[pname]
  assert len(runs) == 2 * len(table)
  applied = set()
  for tag in runs:
    index, apply_u, sign, cy_u, cx_u, box_u = fx[tag + '/draws']
    img = fx['image/' + str(fx[tag + '/image'])]
    got, got_boxes = dr.walk(img, fx['boxes'], pname, int(index[0]), apply_u, sign, cy_u, cx_u, box_u)
    assert np.array_equal(got, fx[tag + '/out']), (tag, int((got != fx[tag + '/out']).sum()))
    same_boxes(got_boxes, fx[tag + '/boxes'], tag)
    applied |= {dr.should_apply(apply_u[k], prob) for k, (_, prob, _) in enumerate(table[int(index[0])])}
  assert applied == ({True} if pname == 'test' else {True, False})      # both branches of _apply_func_with_prob


def test_restatement_reproduces_randaugment():
  fx = fixture()
  for op, name in enumerate(dr.RANDAUG_OPS):
    tag = 'randaug/%d' % op
    index, sign, cy_u, cx_u = fx[tag + '/draws']
    assert int(index) == op
    img = fx['image/' + str(fx[tag + '/image'])]
    got, got_boxes = dr.walk(img, fx['boxes'], 'randaug', [op], None, [sign], [cy_u], [cx_u], [0.0], magnitude=15)
    assert np.array_equal(got, fx[tag + '/out']), (name, int((got != fx[tag + '/out']).sum()))
    same_boxes(got_boxes, fx[tag + '/boxes'], name)


# ------------------------------------------------------------------------------------ CPU: the host side
def test_level_to_arg_and_tables_equal_the_reference():
  fx = fixture()
  for name in daa.NAMES:
    for level in (0, 2, 6, 10):
      want = fx['args/%s/l%d' % (name, level)]
      got = np.asarray([float(v) for v in daa.level_to_arg(name, level)], np.float64)
      assert np.array_equal(got, want), (name, level, got, want)
      assert np.array_equal(np.asarray([float(v) for v in dr.level_to_arg(name, level)], np.float64), want), (name, level)
  for pname in ('test', 'v2', 'v3'):
    table = daa.available_policy(pname)
    assert table == dr.POLICIES[pname]
    ops, prob, level = fx['policy/%s/ops' % pname], fx['policy/%s/prob' % pname], fx['policy/%s/level' % pname]
    assert len(table) == len(ops)
    for s, sub in enumerate(table):
      assert [str(o) for o in ops[s] if str(o)] == [o for o, _, _ in sub]
      assert [p for p in prob[s] if p >= 0] == [p for _, p, _ in sub] and [l for l in level[s] if l >= 0] == [l for _, _, l in sub]
  assert daa.num_layers_of('test') == 2 and daa.num_layers_of('v3') == 2 and daa.num_layers_of('v2') == 3
  assert daa.num_layers_of('randaug', 1) == 1
  assert daa.available_policy('randaug') == 'randaug'
  assert tuple(daa.RANDAUG_OPS) == tuple(dr.RANDAUG_OPS) and tuple(daa.NAMES) == tuple(dr.NAMES)


def test_unbuilt_and_unknown_policies_raise():
  for name in ('v0', 'v1'):
    with pytest.raises(ValueError, match=r'not built.*TranslateY_Only_BBoxes \(aug/autoaugment\.py:745\)'):
      daa.available_policy(name)
  with pytest.raises(ValueError, match=r'Cutout_Only_BBoxes \(aug/autoaugment\.py:777\).*Equalize_Only_BBoxes'):
    daa.available_policy('v1')
  for name in ('v4', '', None, 'autoaug'):
    with pytest.raises(ValueError, match='Invalid augmentation_name'):
      daa.available_policy(name)
  with pytest.raises(ValueError, match='not built'):
    daa.level_to_arg('Flip_Only_BBoxes', 3)
  with pytest.raises(ValueError, match='unknown'):
    daa.level_to_arg('Invert', 3)
  assert len(daa.policy_v0()) == 5 and len(daa.policy_v1()) == 20      # the tables themselves are there: plain data


def test_draws_and_args_shapes():
  rng = np.random.default_rng(1)
  d = daa.autoaug_draws(rng, 5, 'v2')
  assert d.index.shape == (5,) and all(a.shape == (3, 5) for a in d[1:]) and d.apply.dtype == np.float32
  a = daa.autoaug_args(d, 'v2', 37, 53)
  assert a.policy.shape == a.ops.shape == (3, 5) and a.iargs.shape == (3, 5, 4) and a.fargs.shape == (3, 5, 8)
  assert a.dargs.shape == (3, 5, 4) and a.dargs.dtype == np.float64
  d = daa.autoaug_draws(rng, 4, 'randaug', num_layers=2)
  assert d.index.shape == (2, 4) and d.apply is None and int(d.index.max()) < 10
  a = daa.autoaug_args(d, 'randaug', 37, 53, magnitude=15)
  assert not (a.policy == daa.NONE).any()
  # an operation that is not applied and a layer past the end of a shorter sub-policy are the identity
  d = daa.AutoAugDraws(np.asarray([2, 4], np.int32), np.full((3, 2), 0.1, np.float32), np.ones((3, 2), np.float32),
                       np.zeros((3, 2)), np.zeros((3, 2)), np.zeros((3, 2)))
  a = daa.autoaug_args(d, 'v2', 37, 53)      # sub-policy 2 has two operations; 4 = SolarizeAdd 0.2, Contrast 0.0, AutoContrast 0.6
  assert a.policy[:, 0].tolist() == [daa.OP_ID['TranslateY_BBox'], daa.NONE, daa.NONE]
  assert a.policy[:, 1].tolist() == [daa.NONE, daa.NONE, daa.NONE] and (a.ops[:, 1] == 16).all()
  host, layout = daa.pack_args(a)
  assert host.dtype == np.uint8 and layout['dargs'][0] == 0 and host.size == sum(getattr(a, f).nbytes for f in a._fields)


def test_set_autoaugment_needs_no_device():
  from tests.test_det_input import make_config
  net = train_lib.EfficientDetNetTrain(config=make_config(False))
  net.set_autoaugment('v2')
  assert net.autoaugment == 'v2' and net.engine is None
  net.set_autoaugment('randaug')
  net.set_autoaugment(None)
  assert net.autoaugment is None
  for bad in ('v0', 'v1'):
    with pytest.raises(ValueError, match='not built'):
      net.set_autoaugment(bad)
  with pytest.raises(ValueError, match='Invalid augmentation_name'):
    net.set_autoaugment('v9')
  assert net.autoaugment is None


def test_draws_still_construct_from_three_fields():
  d = det_input.Draws(np.zeros(2, np.float32), np.zeros((2, 3), np.float32), None)
  assert d.autoaug is None and len(d) == 4
  flip, scale, gm = d[:3]
  assert gm is None


# ------------------------------------------------------------------------------------ GPU: kernels == restatement
B = 5
CANVASES = ((37, 53), (64, 40))


def batch(h, w, m, seed=0):
  """Five images: random, random, all-constant, random, random; counts 0 and m among them; the padded rows hold values no
  operation may touch."""
  rng = np.random.default_rng(100 + seed + h + m)
  images = rng.integers(0, 256, (B, h, w, 3)).astype(np.uint8)
  images[2] = 93
  y0, x0 = rng.uniform(0.0, 0.6, (B, m)), rng.uniform(0.0, 0.6, (B, m))
  boxes = np.stack([y0, x0, y0 + rng.uniform(0.1, 0.4, (B, m)), x0 + rng.uniform(0.1, 0.4, (B, m))], -1).astype(np.float32)
  fixed = np.asarray([[0.25, 0.3, 0.7, 0.8], [0.5, 0.6, 1.0, 1.0], [0.05, 0.02, 0.3, 0.25], [0.2, 0.5, 0.6, 0.5]], np.float32)
  boxes[:, :min(m, 4)] = fixed[:min(m, 4)]
  counts = np.asarray([m, 0, min(m, 2), m, max(m - 1, 0)], np.int32)
  for i in range(B):
    boxes[i, counts[i]:] = -7.5 - i
  return images, boxes, counts


def single_op_draws(name, level, sign, seed):
  """A one-sub-policy table [(name, 1.0, level)] and draws that apply it to every image."""
  rng = np.random.default_rng(seed)
  table = [[(name, 1.0, level)]]
  d = daa.AutoAugDraws(np.zeros(B, np.int32), np.full((1, B), 0.5, np.float32), np.full((1, B), sign, np.float32),
                       rng.random((1, B)), rng.random((1, B)), rng.random((1, B)))
  return table, d


def ref_table(images, boxes, counts, table, d):
  """The restatement for an explicit table (det_autoaug_ref.walk looks names up in POLICIES)."""
  dr.POLICIES['_case'] = table
  try:
    return dr.distort_batch(images, boxes, counts, '_case', d)
  finally:
    del dr.POLICIES['_case']


def check_device(images, boxes, counts, got, want, what):
  gi, gb = got[0].cpu().numpy(), got[1].cpu().numpy()
  wi, wb = want
  assert gi.dtype == np.uint8 and np.array_equal(gi, wi), (what, 'image bytes off', int((gi != wi).sum()))
  same_boxes(gb, wb, what)
  for i in range(B):      # padded rows untouched
    same_boxes(gb[i, counts[i]:], boxes[i, counts[i]:], (what, 'padding', i))


OP_CASES = [(name, sign) for name in dr.NAMES for sign in ((1.0, -1.0) if name in dr.SIGNED else (1.0,))]


@pytest.mark.gpu
@pytest.mark.parametrize('name,sign', OP_CASES)
def test_kernels_equal_the_restatement_per_operation(name, sign):
  seed = 0
  for h, w in CANVASES:
    for m in (1, 3, preprocess.MAX_BOXES):
      for level in ((2, 6) if m == 3 else (6,)):
        seed += 1
        images, boxes, counts = batch(h, w, m, seed)
        table, d = single_op_draws(name, level, sign, seed)
        got = daa._distort(images, boxes, counts, table, 0, None, None, d)
        torch.cuda.synchronize()
        check_device(images, boxes, counts, got, ref_table(images, boxes, counts, table, d), (name, sign, h, w, m, level))


@pytest.mark.gpu
@pytest.mark.parametrize('policy', ['test', 'v2', 'v3', 'randaug'])
def test_kernels_equal_the_restatement_per_policy(policy):
  for h, w in CANVASES:
    images, boxes, counts = batch(h, w, 3)
    rng = np.random.default_rng(5)
    for rep in range(6):      # fixed draws: with B = 5 every sub-policy of the fifteen is met at least once
      d = daa.autoaug_draws(rng, B, policy, num_layers=1)
      if policy == 'randaug':
        d = d._replace(index=((np.arange(B) + rep * B) % 10).astype(np.int32).reshape(1, B))
        got = daa.distort_image_with_randaugment(images, boxes, counts, 1, 15, draws=d)
        want = dr.distort_batch(images, boxes, counts, 'randaug', d, magnitude=15)
      else:
        n = len(dr.POLICIES[policy])
        d = d._replace(index=((np.arange(B) + rep * B) % n).astype(np.int32))
        got = daa.distort_image_with_autoaugment(images, boxes, counts, policy, draws=d)
        want = dr.distort_batch(images, boxes, counts, policy, d)
      torch.cuda.synchronize()
      check_device(images, boxes, counts, got, want, (policy, h, w, rep))


@pytest.mark.gpu
def test_contrast_blends_with_the_true_mean():
  """Grey sums below 2^24: the constant image (its mean is its grey level, the blend leaves it alone) and an image whose mean
  is x.5 before the truncation (half the pixels at grey level 100, half at 101)."""
  h, w = 64, 40
  images = np.zeros((B, h, w, 3), np.uint8)
  images[0] = 93
  images[1, :, :20] = 100
  images[1, :, 20:] = 101
  images[2:] = np.random.default_rng(3).integers(0, 256, (3, h, w, 3))
  from tests import randaug_ref as rr
  g = rr.grayscale(images[1]).astype(np.int64)
  assert int(g.sum()) * 2 == (2 * int(g.min()) + 1) * g.size and int(g.sum()) < 1 << 24      # mean = min + 0.5
  boxes = np.zeros((B, 1, 4), np.float32)
  counts = np.zeros(B, np.int32)
  for level in (0, 10):
    table, d = single_op_draws('Contrast', level, 1.0, 9)
    got = daa._distort(images, boxes, counts, table, 0, None, None, d)
    torch.cuda.synchronize()
    want = ref_table(images, boxes, counts, table, d)
    check_device(images, boxes, counts, got, want, ('Contrast', level))
    assert np.array_equal(want[0][0], images[0])
    factor = daa.level_to_arg('Contrast', level)[0]
    mean = np.full(images[1].shape, int(g.min()), np.uint8)      # x.5 truncates to x
    assert np.array_equal(want[0][1], rr.blend(mean, images[1], factor))
  from automl_amd import autoaugment as v2aa      # the classifier's Contrast is another operation: H W / 256 = 10
  other = v2aa.distort_image(images, 'randaug', 1, 10, draws=(np.full((1, B), 7, np.int32), np.ones((1, B), np.float32),
                                                             np.zeros((1, B)), np.zeros((1, B))))
  assert not np.array_equal(other.cpu().numpy()[1], want[0][1])


# ------------------------------------------------------------------------------------ GPU: the train step
def _step_batches(steps, seed):
  from tests import test_det_input as tdi
  return [b[0] for b in tdi.batches(False, steps=steps, seed=seed)]


@pytest.mark.gpu
@pytest.mark.parametrize('policy', ['v2', 'randaug'])
def test_raw_step_with_autoaugment_equals_the_pieces(policy):
  """Two steps (the second a graph replay) with set_autoaugment == a second model fed distort_image_with_*'s output through
  plain train_step_raw with the same remaining draws; the generator's state round-trips, so a restored model draws the third
  step's values."""
  from tests import test_det_input as tdi
  config = tdi.make_config(False)
  data = _step_batches(3, 21)
  net = tdi.new_net(config, 'f32', True, stochastic_depth=False)
  net.set_autoaugment(policy)
  plain = tdi.new_net(config, 'f32', True, stochastic_depth=False)
  rng = det_input.input_rng(5)      # new_net's seed: the stream the first model draws from
  losses, want = [], []
  for raw, boxes, classes, counts in data[:2]:
    losses.append(net.train_step_raw((raw, boxes, classes, counts)))
    inp = net._det_input[1]
    d = inp.draw(rng)
    assert d.autoaug is not None
    if policy == 'randaug':
      images, moved = daa.distort_image_with_randaugment(raw, boxes, counts, 1, 15, draws=d.autoaug)
    else:
      images, moved = daa.distort_image_with_autoaugment(raw, boxes, counts, policy, draws=d.autoaug)
    want.append(plain.train_step_raw((images, moved, classes, counts), draws=det_input.Draws(d.flip, d.scale, d.gridmask)))
  torch.cuda.synchronize()
  for i, (x, y) in enumerate(zip(losses, want)):
    for k in tdi.KEYS:
      assert x[k] == y[k], (policy, 'step', i, k, x[k], y[k])
  state, weights = net.get_optimizer_state(), net.get_weights()
  assert np.array_equal(state['input_rng_state'], det_input.utils.pack_rng_state(rng))
  third = net.train_step_raw(data[2])
  other = tdi.new_net(config, 'f32', True, stochastic_depth=False)
  other.set_autoaugment(policy)
  other._ensure_engine(tdi.BATCH, tdi.SIZE, tdi.SIZE)
  other.set_weights(weights)
  other.set_optimizer_state(state)
  again = other.train_step_raw(data[2])
  torch.cuda.synchronize()
  for k in tdi.KEYS:
    assert third[k] == again[k], (policy, 'restored', k, third[k], again[k])


@pytest.mark.gpu
def test_a_model_without_the_switch_keeps_its_stream():
  """Never calling set_autoaugment: the draws are the parent commit's -- flip [B, 1], scale [B, 3] from the seeded generator,
  nothing else taken from it."""
  from tests import test_det_input as tdi
  config = tdi.make_config(False)
  data = _step_batches(2, 22)
  net = tdi.new_net(config, 'f32', True, stochastic_depth=False)
  fed = tdi.new_net(config, 'f32', True, stochastic_depth=False)
  rng = det_input.input_rng(5)
  for d in data:
    a = net.train_step_raw(d)
    flip = rng.random((tdi.BATCH, 1)).astype(np.float32)[:, 0]
    scale = rng.random((tdi.BATCH, 3)).astype(np.float32)
    b = fed.train_step_raw(d, draws=det_input.Draws(flip, scale, None))
    for k in tdi.KEYS:
      assert a[k] == b[k], (k, a[k], b[k])
  torch.cuda.synchronize()
  assert np.array_equal(net.get_optimizer_state()['input_rng_state'], det_input.utils.pack_rng_state(rng))
  assert net._det_input[1].autoaugment is None
