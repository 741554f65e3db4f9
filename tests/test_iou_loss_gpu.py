"""-m gpu: the IoU / GIoU / DIoU / CIoU box loss on the device -- edet_iou_loss (automl_amd.iou_utils.iou_loss), the fused training
and evaluation kernels edet_box_iou_loss / edet_box_iou_loss_eval, and the switch through EfficientDetNetTrain.

The reference of every comparison is the float64 restatement tests/iou_loss_ref.py.  Tolerances, per anchor: the error of a loss
relative to max(1, |loss|), of a gradient component relative to the largest of the anchor's four float64 components.  E32 is that
measure for the restatement run in numpy float32 on the test's own inputs (rounded to bf16 first for bf16 storage), computed
here on the CPU; the kernels get 4 * E32 with a floor of 64 * 2^-24 (fused multiply-adds, expf / atanf / division a unit or two
in the last place from numpy's; the floor is the ~60 roundings of the longest chain), a bf16 gradient 2^-8 of the stored value
on top (one rounding to storage).  Sums: the per-anchor bound times the number of terms, plus (terms + 64) * 2^-24 of the sum of
magnitudes for the additions.  Measured on an MI355X (largest error / bound over all cases): see LABNOTES, "IoU loss".
"""
import os

import numpy as np
import pytest
import torch

from automl_amd import _lib, hparams_config, iou_utils, train_lib
from automl_amd import anchors as anchors_lib
from automl_amd._lib import call, ptr
from tests import gpu_util as gu
from tests import iou_loss_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
DT = {'f32': (_lib.EDET_F32, torch.float32), 'bf16': (_lib.EDET_BF16, torch.bfloat16)}
FLOOR = 64 * 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_iou_loss.npz')
PB = np.array([[4, 3, 7, 5], [5, 6, 10, 7]], F)
TB = np.array([[3, 4, 6, 8], [14, 14, 15, 15]], F)
KNOWN = {'iou': [0.875, 1.0], 'ciou': [0.99931306, 1.6415315], 'diou': [0.9969512, 1.6243094], 'giou': [1.075, 1.933333]}
CIOU_GRAD = np.array([[0.0789376, -0.0424137, 0.0161798, -0.1656677], [0.0303104, 0.0178871, -0.0386740, -0.0441989]])
_CACHE = {}


def measures(loss, grad, loss64, grad64, extra_grad=None):
  """-> (largest loss error relative to max(1, |loss|), largest gradient error relative to the anchor's largest component);
  extra_grad: an absolute allowance per component, taken off the error first (the bf16 storage rounding)."""
  le = np.abs(np.asarray(loss, np.float64) - loss64) / np.maximum(1.0, np.abs(loss64))
  ge = np.abs(np.asarray(grad, np.float64) - grad64)
  if extra_grad is not None:
    ge = np.maximum(ge - extra_grad, 0.0)
  gm = np.abs(grad64).max(-1, keepdims=True)
  ge = ge / np.where(gm > 0, gm, 1.0)
  return float(le.max()) if le.size else 0.0, float(ge.max()) if ge.size else 0.0


def e32_bounds(fn, *inputs):
  """fn(float dtype inputs...) -> (loss, grad): E32 of the float32 run against the float64 run -> (bounds, float64 results)."""
  l64, g64 = fn(*[np.asarray(v, np.float64) for v in inputs])
  l32, g32 = fn(*[np.asarray(v, np.float32) for v in inputs])
  e32 = measures(l32, g32, l64, g64)
  return [max(4 * e, FLOOR) for e in e32], e32, l64, g64


def report(what, got, bound, e32):
  print('%s: E32 loss %.3g grad %.3g; device err / bound loss %.3f grad %.3f' % (what, e32[0], e32[1], got[0] / bound[0], got[1] / bound[1]))


@pytest.fixture(scope='module')
def golden():
  with np.load(GOLDEN) as z:
    return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------------------ edet_iou_loss
@pytest.mark.parametrize('kind', R.IOU_TYPES)
def test_iou_loss_known_answers(kind):
  loss, grad = iou_utils.iou_loss(PB, TB, kind, return_grad=True)
  assert loss.shape == (2,) and grad.shape == (2, 4) and loss.dtype == torch.float32 and loss.is_cuda
  np.testing.assert_allclose(loss.cpu().numpy(), KNOWN[kind], rtol=1e-6, atol=1e-6)
  only = iou_utils.iou_loss(torch.from_numpy(PB).to(gu.DEV), TB, kind)
  assert torch.equal(only, loss)
  z = iou_utils.iou_loss(np.zeros((2, 4), F), np.zeros((2, 4), F), kind, return_grad=True)
  assert not z[0].any() and not z[1].any()
  if kind == 'iou':
    np.testing.assert_allclose(iou_utils.iou_loss(np.tile(PB, [1, 2]), np.tile(TB, [1, 2]), kind).cpu().numpy(), [1.75, 2.0],
                               rtol=1e-6, atol=1e-6)
  pad = np.zeros_like(PB)
  loss, grad = iou_utils.iou_loss(np.concatenate([PB, pad], 1), np.concatenate([TB, pad], 1), kind, return_grad=True)
  np.testing.assert_allclose(loss.cpu().numpy(), KNOWN[kind], rtol=1e-6, atol=1e-6)
  assert not grad[:, 4:].any()      # the zero anchor: exactly no gradient
  if kind == 'ciou':      # v is a constant of the backward pass: the full derivative would start 0.0747623
    np.testing.assert_allclose(grad[:, :4].cpu().numpy(), CIOU_GRAD, rtol=0, atol=1e-6)
    np.testing.assert_allclose(float(grad.double().sum()), -0.14763935, atol=1e-6)
  with pytest.raises(ValueError, match='Unknown loss_type xiou, not iou/ciou/diou/giou'):
    iou_utils.iou_loss(PB, TB, 'xiou')
  with pytest.raises(ValueError, match=r'\[\.\.\., 4k\]'):
    iou_utils.iou_loss(PB[:, :3], TB[:, :3], kind)


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('kind', R.IOU_TYPES)
def test_iou_loss_on_the_fixtures_decoded_boxes(golden, kind, k):
  p, t = golden['case_%s/decoded_pred' % kind], golden['case_%s/decoded_target' % kind]
  n = p.shape[0] // k * k
  p, t = p[:n].reshape(-1, 4 * k), t[:n].reshape(-1, 4 * k)
  bound, e32, l64, g64 = e32_bounds(lambda a, b: R.iou_loss(a, b, kind), p, t)
  loss, grad = iou_utils.iou_loss(p, t, kind, return_grad=True)
  # a row's loss is the sum of k anchors: k times the per-anchor bound; the gradient is per anchor
  got = measures(loss.cpu().numpy(), grad.cpu().numpy().reshape(-1, 4), l64, g64.reshape(-1, 4))
  report('edet_iou_loss %s k=%d' % (kind, k), got, [k * bound[0], bound[1]], e32)
  assert got[0] <= k * bound[0] and got[1] <= bound[1], (got, bound)
  dead = (t.reshape(-1, 4) == 0).all(-1)
  assert dead.any() and not grad.cpu().numpy().reshape(-1, 4)[dead].any()


def test_iou_loss_refuses_bad_arguments():
  a = torch.zeros(8, device=gu.DEV)
  for args in ((None, ptr(a), 2, 1, 0, ptr(a), None), (ptr(a), ptr(a), 2, 1, 4, ptr(a), None), (ptr(a), ptr(a), 2, 0, 0, ptr(a), None),
               (ptr(a) + 4, ptr(a), 1, 1, 0, ptr(a), None)):
    with pytest.raises(_lib.EdetError, match='edet_iou_loss'):
      call('edet_iou_loss', *args, gu.stream())


# ------------------------------------------------------------------------------------------------------- edet_box_iou_loss
SHAPES = {      # (B, h, w, A, ld, workspace)
    'narrow_1x4x4x1_ld8': (1, 4, 4, 1, 8, True),            # the narrowest row
    'odd_2x3x5x9_ld40': (2, 3, 5, 9, 40, True),             # p mod hw across images, the one-anchor last chunk, padding written 0
    'two_wg_2x11x13x9_ld40': (2, 11, 13, 9, 40, True),      # 286 positions > 4 * (256 / 8): two workgroups, ordered partial rows
    'one_wg_2x11x13x9_ld40': (2, 11, 13, 9, 40, False),     # the same without a workspace: ONE workgroup
}
DELTA, NORMALIZER, BOX_W, IOU_W = 0.1, 9.0, 50.0, 1.5
INV = float(F(1.0 / (NORMALIZER * 4.0)))


def workspace():
  if 'ws' not in _CACHE:
    _CACHE['ws'] = torch.empty(1 << 20, dtype=torch.float32, device=gu.DEV)
  return _CACHE['ws']


def problem(shape, name):
  """The inputs of a shape (the generator's recipe and kink margin, |value| <= 2; rounded to the storage type) and what does
  not depend on the IoU type: Huber's float64 values."""
  b, h, w, na, ld, _ = SHAPES[shape]
  key = (b, h, w, na, name)
  if key not in _CACHE:
    anchors = R.make_anchors(h, w, na)
    rows = np.tile(anchors, (b, 1))
    tdt = DT[name][1]
    for seed in range(1000, 1064):      # the margin is asked of the values the kernel sees: after the rounding to storage
      x, tg, _ = R.draw_case(seed + 7 * na + h, rows, zero_component_row=True)
      x = torch.from_numpy(x).to(tdt).float().numpy()
      err = np.abs(x.astype(np.float64) - tg)[tg != 0]
      if R.kink_margin(x, tg, rows) >= 1e-3 and np.abs(err - DELTA).min() > 1e-5:
        break
    else:
      raise AssertionError('no draw')
    e = x.astype(np.float64) - tg
    quad = np.abs(e) <= DELTA
    live = tg != 0
    hub = np.where(live, np.where(quad, 0.5 * e * e, DELTA * np.abs(e) - 0.5 * DELTA * DELTA), 0.0)
    hub_g = np.where(live, np.where(quad, e, np.sign(e) * DELTA), 0.0)
    _CACHE[key] = dict(x=x, tg=tg, anchors=anchors, rows=rows, hub=hub, hub_g=hub_g, cache={})
  return _CACHE[key]


def reference(pr, kind):
  if kind not in pr['cache']:
    pr['cache'][kind] = e32_bounds(lambda x, t, a: R.box_iou_per_anchor(x, t, a, kind), pr['x'], pr['tg'], pr['rows'])
  return pr['cache'][kind]


def launch(shape, name, kind, iou_w=IOU_W, box_w=BOX_W, device_norm=False, which='train'):
  """-> dict of device results of edet_box_iou_loss (which='train'), its _eval twin ('eval') or edet_box_loss ('plain')."""
  b, h, w, na, ld, use_ws = SHAPES[shape]
  edt, tdt = DT[name]
  pr = problem(shape, name)
  nch, pos = 4 * na, b * h * w
  box = torch.full((pos, ld), float('nan'), dtype=torch.float32)
  box[:, :nch] = torch.from_numpy(pr['x'].reshape(pos, nch))
  box = box.to(gu.DEV).to(tdt).contiguous()
  td = torch.from_numpy(pr['tg'].reshape(pos, nch)).to(gu.DEV).contiguous()
  anchors = torch.from_numpy(pr['anchors']).to(gu.DEV).contiguous()
  db = torch.full_like(box, float('nan'))
  dbias = torch.zeros(nch, dtype=torch.float32, device=gu.DEV)
  sums = torch.zeros(4, dtype=torch.float32, device=gu.DEV)
  norm_dev, inv = None, INV
  if device_norm:      # 1 / normalizer on the device, 1 / 4 on the host: the same product
    norm_dev, inv = torch.tensor([1.0 / NORMALIZER], dtype=torch.float32, device=gu.DEV), 0.25
  ws = workspace() if use_ws else None
  wsb = ws.numel() * 4 if use_ws else 0
  kid = iou_utils.iou_type_id(kind)
  if which == 'train':
    call('edet_box_iou_loss', ptr(box), ld, ptr(td), pos, nch, DELTA, inv, box_w, ptr(norm_dev), ptr(db), ptr(dbias), ptr(sums),
         ptr(ws), wsb, edt, gu.stream(), ptr(anchors), h * w, kid, iou_w)
  elif which == 'eval':
    call('edet_box_iou_loss_eval', ptr(box), ld, ptr(td), pos, nch, DELTA, inv, ptr(norm_dev), ptr(sums), ptr(ws), wsb, edt,
         gu.stream(), ptr(anchors), h * w, kid)
  else:
    call('edet_box_loss', ptr(box), ld, ptr(td), pos, nch, DELTA, inv, box_w, ptr(norm_dev), ptr(db), ptr(dbias), ptr(sums),
         ptr(ws), wsb, edt, gu.stream())
  torch.cuda.synchronize()
  return dict(dbox=db, dbias=dbias, sums=sums, inv=1.0 / (NORMALIZER * 4.0) if device_norm else INV)


@pytest.mark.parametrize('name', list(DT))
@pytest.mark.parametrize('kind', R.IOU_TYPES)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_box_iou_loss_against_the_restatement(shape, kind, name):
  b, h, w, na, ld, use_ws = SHAPES[shape]
  nch, pos = 4 * na, b * h * w
  pr = problem(shape, name)
  bound, e32, l64, g64 = reference(pr, kind)
  out = launch(shape, name, kind, device_norm=(shape == 'odd_2x3x5x9_ld40'))
  inv = out['inv']
  dbox = out['dbox'].float().cpu().numpy().astype(np.float64)
  assert not dbox[:, nch:].any() and np.isfinite(dbox).all()      # the padding channels are written 0
  got_g = dbox[:, :nch].reshape(-1, 4)
  want_h = pr['hub_g'] * inv * BOX_W
  want = want_h + g64 * inv * IOU_W
  # per component: Huber's few float32 roundings, the sum's rounding, and for bf16 the one rounding to storage -- taken off
  # before the IoU part's error is measured in the issue's terms (relative to the anchor's largest IoU gradient component)
  allow = 4 * 2.0 ** -24 * np.abs(want_h) + 2.0 ** -24 * np.abs(want) + (2.0 ** -8 * np.abs(want) if name == 'bf16' else 0.0)
  ge = np.maximum(np.abs(got_g - want) - allow, 0.0) / (inv * IOU_W)
  gm = np.abs(g64).max(-1, keepdims=True)
  got = (0.0, float((ge / np.where(gm > 0, gm, 1.0)).max()))
  npos = int((pr['tg'] != 0).any(-1).sum())
  # the IoU sum: per-anchor bound for each term, (terms + 64) roundings of additions on the sum of magnitudes
  s3, want3 = float(out['sums'][3]), float(l64.sum() * inv)
  mag = float(np.maximum(1.0, np.abs(l64))[l64 != 0].sum() * inv)
  tol3 = bound[0] * mag + (npos + 64) * 2.0 ** -24 * mag
  print('%s %s %s: E32 loss %.3g grad %.3g; gradient err / bound %.3f; sums[3] %.8g want %.8g err / bound %.3f'
        % (shape, kind, name, e32[0], e32[1], got[1] / bound[1], s3, want3, abs(s3 - want3) / tol3))
  assert got[1] <= bound[1], (got, bound)
  assert abs(s3 - want3) <= tol3, (s3, want3, tol3)
  dead = (pr['tg'] == 0).all(-1)
  assert not got_g[dead].any()
  # Huber's sum is edet_box_loss's (bit for bit: test_promises) and near its float64 value; sums[0] and [2] are not touched
  want1 = float(pr['hub'].sum() * inv)
  assert abs(float(out['sums'][1]) - want1) <= (pr['hub'] != 0).sum() * 2.0 ** -22 * want1
  assert float(out['sums'][0]) == 0.0 and float(out['sums'][2]) == 0.0
  # dbias: the column sums of the fp32 values dbox was rounded from (as edet_box_loss forms it), added in fp32 -- against the
  # stored values, which for bf16 are each one rounding (2^-8 of the value) away
  col = out['dbox'].float().cpu().numpy().astype(np.float64)[:, :nch]
  db = out['dbias'].cpu().numpy().astype(np.float64)
  stored = 2.0 ** -8 if name == 'bf16' else 0.0
  assert (np.abs(db - col.sum(0)) <= ((pos + 64) * 2.0 ** -24 + stored) * np.abs(col).sum(0) + 1e-30).all()
  if not use_ws:      # against the run with a workspace: the same gradient bits, the sums within the summation bound
    ref = launch('two_wg_2x11x13x9_ld40', name, kind)
    assert torch.equal(out['dbox'][:, :nch], ref['dbox'][:, :nch])
    assert abs(s3 - float(ref['sums'][3])) <= 2 * (npos + 64) * 2.0 ** -24 * mag
    assert (np.abs(db - ref['dbias'].cpu().numpy()) <= 2 * (pos + 64) * 2.0 ** -24 * np.abs(col).sum(0) + 1e-30).all()


@pytest.mark.parametrize('name', list(DT))
@pytest.mark.parametrize('kind', ['giou', 'ciou'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_promises(shape, kind, name):
  b, h, w, na, ld, _ = SHAPES[shape]
  nch = 4 * na
  train, again = launch(shape, name, kind), launch(shape, name, kind)
  plain, off = launch(shape, name, kind, which='plain'), launch(shape, name, kind, iou_w=0.0)
  ev = launch(shape, name, kind, which='eval')
  # a second run on the same inputs: the same bits (no atomics)
  assert torch.equal(train['sums'], again['sums']) and torch.equal(train['dbias'], again['dbias'])
  assert torch.equal(train['dbox'][:, :nch], again['dbox'][:, :nch])
  # sums[1] is edet_box_loss's
  assert torch.equal(train['sums'][1], plain['sums'][1]) and float(plain['sums'][3]) == 0.0 and float(train['sums'][3]) > 0.0
  # iou_grad_scale = 0: the gradient of edet_box_loss, and the IoU sum all the same
  assert torch.equal(off['dbox'][:, :nch], plain['dbox'][:, :nch]) and torch.equal(off['dbias'], plain['dbias'])
  assert not off['dbox'][:, nch:].any() and torch.equal(off['sums'], train['sums'])
  assert not torch.equal(train['dbox'][:, :nch], plain['dbox'][:, :nch])
  # the evaluation twin: both sums of the training kernel, nothing else written
  assert torch.equal(ev['sums'], train['sums'])
  assert torch.isnan(ev['dbox']).all() and not ev['dbias'].any()


def test_box_iou_loss_refuses_bad_arguments():
  a, tg, db, dbias, sums = (torch.zeros(64, device=gu.DEV) for _ in range(5))
  good = [ptr(a), 8, ptr(tg), 4, 4, 0.1, 1.0, 1.0, None, ptr(db), ptr(dbias), ptr(sums), None, 0, _lib.EDET_F32, gu.stream(),
          ptr(a), 4, 0, 1.0]
  call('edet_box_iou_loss', *good)
  for at, bad in ((16, None), (16, ptr(a) + 4), (17, 3), (17, 0), (18, 4), (18, -1), (4, 3)):
    args = list(good)
    args[at] = bad
    with pytest.raises(_lib.EdetError, match='edet_box_iou_loss'):
      call('edet_box_iou_loss', *args)
  ev = good[:7] + [None, ptr(sums), None, 0, _lib.EDET_F32, gu.stream(), ptr(a), 4, 0]
  call('edet_box_iou_loss_eval', *ev)
  for at, bad in ((13, None), (14, 3), (15, 7)):
    args = list(ev)
    args[at] = bad
    with pytest.raises(_lib.EdetError, match='edet_box_iou_loss_eval'):
      call('edet_box_iou_loss_eval', *args)
  torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- through the trainer
SIZE, BATCH, STEPS = 128, 2, 3


def det_config():
  return hparams_config.get_efficientdet_config('efficientdet-d0')


def det_net(iou_loss, use_graph=False):
  from oracle.problems import perturbed_params
  config = det_config()
  return train_lib.EfficientDetNetTrain(config=config, dtype='f32', params=perturbed_params(config, 11), seed=5, use_graph=use_graph,
                                        stochastic_depth=False, steps_per_epoch=10, iou_loss=iou_loss)


def det_data():
  from tests.test_gpu_network import make_labels
  if 'data' not in _CACHE:
    rng = np.random.default_rng(7)
    _CACHE['data'] = [(rng.standard_normal((BATCH, SIZE, SIZE, 3)).astype(F), make_labels(det_config(), BATCH, SIZE, 50 + i))
                      for i in range(STEPS)]
  return _CACHE['data']


def arena_np(arena):
  return {k: getattr(arena, k).detach().cpu().numpy().copy() for k in ('params_flat', 'velocity', 'ema', 'state_flat')}


def restated_sum(eng, labels, kind):
  """The float64 restatement on the engine's stored box outputs and the labels -> (sum of the per-anchor losses / (4 *
  normalizer), number of positive anchors, the bound of the device's sum: 4 * E32 (floor 64 * 2^-24) per term on the sum of
  max(1, |loss|), E32 from the float32 restatement on the same outputs, plus (terms + 64 per level) * 2^-24 of the sum of
  magnitudes for the additions)."""
  c = eng.config
  table = np.asarray(anchors_lib.Anchors(c.min_level, c.max_level, c.num_scales, c.aspect_ratios, c.anchor_scale,
                                         tuple(eng.image_size)).boxes, F)
  _, box = eng.outputs()
  normalizer = float(np.asarray(labels['mean_num_positives'], np.float64).sum()) + 1.0
  total, npos, mag, row, e32 = 0.0, 0, 0.0, 0, 0.0
  for li, out in enumerate(box):
    x = out.detach().float().cpu().numpy().reshape(BATCH, -1, 4)
    tg = np.asarray(labels['box_targets_%d' % (c.min_level + li)], F).reshape(BATCH, -1, 4)
    a = table[row:row + x.shape[1]]
    row += x.shape[1]
    for i in range(BATCH):
      loss, grad = R.box_iou_per_anchor(x[i].astype(np.float64), tg[i], a, kind)
      e32 = max(e32, measures(R.box_iou_per_anchor(x[i], tg[i], a, kind)[0], grad, loss, grad)[0])
      total += float(loss.sum())
      npos += int((tg[i] != 0).any(-1).sum())
      mag += float(np.maximum(1.0, np.abs(loss))[loss != 0].sum())
  assert row == table.shape[0]
  inv = 1.0 / (4.0 * normalizer)
  tol = max(4 * e32, FLOOR) * mag * inv + (npos + 64 * len(box)) * 2.0 ** -24 * mag * inv
  print('restated %s sum: %d positive anchors, E32 %.3g, bound %.3g' % (kind, npos, e32, tol))
  return total * inv, npos, tol


def test_weight_zero_moves_exactly_what_the_model_without_it_moves():
  data = det_data()
  plain, zero = det_net(None), det_net(dict(type='giou', weight=0.0))
  a, b = plain.train_step(data[0]), zero.train_step(data[0])
  torch.cuda.synchronize()
  assert zero.engine.iou_loss == (1, 'giou', 0.0) and plain.engine.iou_loss is None
  for k, want in arena_np(plain.engine.arena).items():
    got = arena_np(zero.engine.arena)[k]
    assert np.array_equal(got, want), '%s: %d elements differ' % (k, int((got != want).sum()))
  assert 'box_iou_loss' not in a and b['box_iou_loss'] > 0
  assert a['cls_loss'] == b['cls_loss'] and a['box_loss'] == b['box_loss'] and a['det_loss'] == b['det_loss']
  assert plain.engine.loss_keys == plain.engine.LOSS_KEYS and zero.engine.loss_keys[-1] == 'box_iou_loss'


@pytest.fixture(scope='module')
def ciou_eager():
  """STEPS eager steps with ciou, weight 1 -> (net, the loss values of every step, the arena after the last)."""
  net = det_net(dict(type='ciou', weight=1.0))
  values = []
  for d in det_data():
    values.append(net.train_step(d))
    if len(values) == 1:
      torch.cuda.synchronize()
      values[0]['restated'] = restated_sum(net.engine, d[1], 'ciou')
      values[0]['sums'] = net.engine.loss_sums.detach().cpu().numpy().copy()
  torch.cuda.synchronize()
  return net, values, arena_np(net.engine.arena)


def test_trainer_reports_the_restated_loss(ciou_eager):
  net, values, _ = ciou_eager
  v = values[0]
  want, npos, tol = v['restated']
  print('box_iou_loss %.8g, restated %.8g, err / bound %.3f (%d positive anchors)' % (v['box_iou_loss'], want, abs(v['box_iou_loss'] - want) / tol, npos))
  assert npos > 50 and abs(v['box_iou_loss'] - want) <= tol
  s = v['sums']
  c = net.config
  det = F(F(s[0] + F(c.box_loss_weight) * s[1]) + F(1.0) * s[3])      # D5 in float32
  assert v['det_loss'] == float(det) and v['box_iou_loss'] == float(s[3]) and v['loss'] == float(det) + float(s[2])
  vec = net.engine.loss_vector(torch.from_numpy(s).to(gu.DEV), torch.zeros(6, device=gu.DEV)).cpu().numpy()
  assert [float(x) for x in vec] == [float(F(v[k])) for k in net.engine.loss_keys]


def test_graph_replay_equals_eager(ciou_eager):
  _, values, want = ciou_eager
  net = det_net(dict(type='ciou', weight=1.0), use_graph=True)
  outs = [net.train_step(d) for d in det_data()]
  torch.cuda.synchronize()
  assert net._graph['graphs'] is not None and net.engine.arena.step_count == STEPS
  got = arena_np(net.engine.arena)
  for k in want:
    assert np.array_equal(got[k], want[k]), '%s: %d elements differ' % (k, int((got[k] != want[k]).sum()))
  for a, b in zip(outs, values):
    assert all(a[k] == b[k] for k in net.engine.loss_keys)


def test_test_step_reports_the_training_kernels_sum_and_moves_nothing(ciou_eager):
  net, _, _ = ciou_eager
  eng = net.engine
  before = arena_np(eng.arena)
  data = det_data()[0]
  out = net.test_step(data)
  torch.cuda.synchronize()
  for k, want in before.items():
    assert np.array_equal(arena_np(eng.arena)[k], want), k
  # the training kernels on the outputs of that forward pass, with the evaluation step's normalizer
  labels = net._labels_to_device(data[1], eng)
  sums = torch.zeros(4, dtype=torch.float32, device=gu.DEV)
  na, row = eng.spec.num_anchors, 0
  table = eng._iou_anchors()
  ws = workspace()
  for li, bv in enumerate(eng.box_views):
    rb = bv.raw
    bt = labels['box_targets_%d' % (eng.config.min_level + li)]
    edt = _lib.EDET_F32 if rb.data.dtype == torch.float32 else _lib.EDET_BF16
    hw = rb.rows // BATCH
    dbox, dbias = torch.empty_like(rb.data), torch.zeros(4 * na, device=gu.DEV)      # scratch: the gradient is not looked at
    call('edet_box_iou_loss', ptr(rb.data), rb.ld, ptr(bt), rb.rows, 4 * na, eng.config.delta, 0.25, 1.0, ptr(eng.eval_inv_norm),
         ptr(dbox), ptr(dbias), ptr(sums), ptr(ws), ws.numel() * 4, edt, gu.stream(), table.data_ptr() + 16 * row, hw, 3, 1.0)
    torch.cuda.synchronize()
    row += hw * na
  torch.cuda.synchronize()
  s = sums.cpu().numpy()
  assert out['box_iou_loss'] == float(s[3]) and out['box_loss'] == float(s[1]) and s[3] > 0
  assert out['det_loss'] == float(F(F(F(out['cls_loss']) + F(eng.config.box_loss_weight) * s[1]) + F(1.0) * s[3]))
  want, npos, tol = restated_sum(eng, data[1], 'ciou')
  assert abs(out['box_iou_loss'] - want) <= tol


def test_recording_a_plan_is_refused(ciou_eager):
  from automl_amd import plan
  net, _, _ = ciou_eager
  images, labels = det_data()[0]
  with pytest.raises(ValueError, match='is not built'):
    plan.record_network(net, torch.from_numpy(images).to(gu.DEV), labels, path=os.devnull)
