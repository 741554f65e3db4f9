"""The IoU / GIoU / DIoU / CIoU box loss without a device: the numpy restatement (tests/iou_loss_ref.py) against the reference's
own test values, against central differences of itself and against the executed reference (tests/golden/reference_iou_loss.npz,
made by tests/golden/make_golden_iou_loss.py), and the wiring of the switch through the trainer, the CLI and the state file."""
import os

import numpy as np
import pytest

from automl_amd import hparams_config, iou_utils, train, train_lib
from tests import iou_loss_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_iou_loss.npz')
F = np.float32
PB = np.array([[4, 3, 7, 5], [5, 6, 10, 7]], F)
TB = np.array([[3, 4, 6, 8], [14, 14, 15, 15]], F)
KNOWN = {'iou': [0.875, 1.0], 'ciou': [0.99931306, 1.6415315], 'diou': [0.9969512, 1.6243094], 'giou': [1.075, 1.933333]}
# the gradient of sum(ciou loss) with respect to PB with v a constant of the backward pass (torch autograd, float32); the full
# derivative would start 0.0747623
CIOU_GRAD = np.array([[0.0789376, -0.0424137, 0.0161798, -0.1656677], [0.0303104, 0.0178871, -0.0386740, -0.0441989]])


@pytest.fixture(scope='module')
def golden():
  with np.load(GOLDEN) as z:
    return {k: z[k] for k in z.files}


def case(golden, kind):
  return {k.split('/', 1)[1]: v for k, v in golden.items() if k.startswith('case_%s/' % kind)}


def error_measures(loss, grad, loss64, grad64):
  """The issue's per-anchor measures -> (loss error relative to max(1, |loss|), gradient error relative to the largest of the
  anchor's four float64 components), each the maximum over the anchors."""
  le = np.abs(loss.astype(np.float64) - loss64) / np.maximum(1.0, np.abs(loss64))
  gm = np.abs(grad64).max(-1, keepdims=True)
  ge = np.abs(grad.astype(np.float64) - grad64) / np.where(gm > 0, gm, 1.0)
  return float(le.max()), float(ge.max())


FLOOR = 64 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------- the reference's test values
@pytest.mark.parametrize('kind', R.IOU_TYPES)
def test_reference_test_values(kind):
  loss, _ = R.iou_loss(PB, TB, kind)
  assert loss.dtype == F
  np.testing.assert_allclose(loss, KNOWN[kind], rtol=1e-6, atol=1e-6)
  zero, _ = R.iou_loss(np.zeros((2, 4), F), np.zeros((2, 4), F), kind)
  assert (zero == 0).all()


def test_reference_test_values_multiple_anchors():
  np.testing.assert_allclose(R.iou_loss(np.tile(PB, [1, 2]), np.tile(TB, [1, 2]), 'iou')[0], [1.75, 2.0], rtol=1e-6, atol=1e-6)
  pad = np.zeros_like(PB)
  loss, grad = R.iou_loss(np.concatenate([PB, pad], 1), np.concatenate([TB, pad], 1), 'iou')
  np.testing.assert_allclose(loss, [0.875, 1.0], rtol=1e-6, atol=1e-6)
  assert (grad[:, 4:] == 0).all()


def test_ciou_grad_is_the_executed_one_not_the_papers(golden):
  _, grad = R.iou_loss(PB, TB, 'ciou')
  np.testing.assert_allclose(float(grad.sum(dtype=np.float64)), -0.14763935, atol=1e-6)
  np.testing.assert_allclose(grad, CIOU_GRAD, rtol=0, atol=1e-6)
  assert abs(grad[0, 0] - 0.0747623) > 1e-3      # the full derivative (v differentiated) is told apart
  # the zero anchor of a padded pair gets exactly no gradient
  pad = np.zeros_like(PB)
  _, g2 = R.iou_loss(np.concatenate([PB, pad], 1), np.concatenate([TB, pad], 1), 'ciou')
  np.testing.assert_allclose(g2[:, :4], CIOU_GRAD, rtol=0, atol=1e-6)
  assert (g2[:, 4:] == 0).all()
  # and what the executed reference gave for the same pair
  np.testing.assert_allclose(golden['known/ciou_grad_pred'], CIOU_GRAD, rtol=0, atol=1e-6)
  np.testing.assert_allclose(float(golden['known/ciou_grad_target'].sum(dtype=np.float64)), 0.1476393, atol=1e-6)


def test_unknown_type_raises_the_references_message():
  for fn in (lambda: R.iou_loss(PB, TB, 'xiou'), lambda: iou_utils.iou_type_id('xiou'),
             lambda: iou_utils.iou_loss(PB, TB, 'xiou')):
    with pytest.raises(ValueError, match='Unknown loss_type xiou, not iou/ciou/diou/giou'):
      fn()
  assert [iou_utils.iou_type_id(k) for k in ('iou', 'giou', 'diou', 'ciou')] == [0, 1, 2, 3]


# ---------------------------------------------------------------------------------------------- finite differences
@pytest.mark.parametrize('kind', R.IOU_TYPES)
def test_gradient_equals_central_differences(golden, kind):
  """float64, h = 1e-6, relative 1e-6: the fixture keeps every positive anchor 1e-3 away from a kink, truncation h^2 and
  cancellation 2^-53 / h stay far below the bound.  CIoU's v is held at its value, as the backward pass holds it."""
  c = case(golden, kind)
  x, tg, a = c['box_outputs'].astype(np.float64), c['box_targets'].astype(np.float64), c['anchors'].astype(np.float64)
  assert R.kink_margin(x, tg, a) >= 1e-3
  pos = (tg != 0).any(-1)
  p, t = R.decoded_pair(x, tg, a)
  v = R.ciou_v(p, t) if kind == 'ciou' else None
  _, grad = R.box_iou_per_anchor(x, tg, a, kind)
  h = 1e-6
  fd = np.zeros_like(x)
  for k in range(4):
    e = np.zeros(4)
    e[k] = h
    fd[:, k] = (R.box_iou_per_anchor(x + e, tg, a, kind, v)[0] - R.box_iou_per_anchor(x - e, tg, a, kind, v)[0]) / (2 * h)
  scale = np.maximum(np.abs(grad).max(-1, keepdims=True), 1.0)
  assert (np.abs(fd - grad) / scale)[pos].max() <= 1e-6, (np.abs(fd - grad) / scale)[pos].max()
  assert (grad[~pos] == 0).all() and (fd[~pos] == 0).all()


# ---------------------------------------------------------------------------------------------- the executed reference
@pytest.mark.parametrize('kind', R.IOU_TYPES)
def test_restatement_against_the_executed_reference(golden, kind):
  """The float32 restatement and the reference run on the torch-backed stand-in, both against the float64 restatement: each
  within 4 * E32 (floor 64 * 2^-24), E32 being the float32 restatement's own error -- so the two agree within twice that."""
  c = case(golden, kind)
  x, tg, a = c['box_outputs'], c['box_targets'], c['anchors']
  pos = (tg != 0).any(-1)
  loss64, grad64 = R.box_iou_per_anchor(x.astype(np.float64), tg, a, kind)
  loss32, grad32 = R.box_iou_per_anchor(x, tg, a, kind)
  e32 = error_measures(loss32, grad32, loss64, grad64)
  bound = [max(4 * e, FLOOR) for e in e32]
  got = error_measures(c['loss_per_anchor'], c['grad_sum'], loss64, grad64)
  print(kind, 'E32 loss %.3g grad %.3g; executed reference: loss %.3g grad %.3g' % (e32 + got))
  assert got[0] <= bound[0] and got[1] <= bound[1], (got, bound)
  assert (c['loss_per_anchor'][~pos] == 0).all() and (c['grad_sum'][~pos] == 0).all() and (c['grad'][~pos] == 0).all()
  assert (loss32[~pos] == 0).all() and (grad32[~pos] == 0).all()
  # the decoded, masked boxes the reference handed to iou_loss, and its reduction (train_lib.py:457,463)
  p, t = R.decoded_pair(x, tg, a)
  np.testing.assert_allclose(c['decoded_pred'][pos], p[pos], rtol=1e-5, atol=1e-4)
  np.testing.assert_allclose(c['decoded_target'][pos], t[pos], rtol=1e-5, atol=1e-4)
  red, gred = R.box_iou_loss(x.astype(np.float64), tg, a, kind, float(c['num_positives']))
  n = int(pos.sum())
  assert abs(float(c['loss']) - red) <= (n + 2) * 2.0 ** -24 * abs(red) + max(bound[0], FLOOR) * n / (4 * float(c['num_positives']))
  assert error_measures(np.zeros(len(x), F), c['grad'], np.zeros(len(x)), gred)[1] <= bound[1] + 2.0 ** -23


def test_fixture_cases(golden):
  assert 2 * int(golden['rejected']) <= int(golden['draws'])
  for kind in R.IOU_TYPES:
    c = case(golden, kind)
    tg = c['box_targets']
    assert c['anchors'].shape == (189, 4) and 0.15 < (tg != 0).any(-1).mean() < 0.35
    assert ((tg != 0).sum(-1) == 3).sum() == 1 and np.abs(tg).max() <= 2 and np.abs(c['box_outputs']).max() <= 2
    p, t = R.decoded_pair(c['box_outputs'].astype(np.float64), tg, c['anchors'])
    pos = (tg != 0).all(-1)
    ih = np.minimum(p[pos, 2], t[pos, 2]) - np.maximum(p[pos, 0], t[pos, 0])
    iw = np.minimum(p[pos, 3], t[pos, 3]) - np.maximum(p[pos, 1], t[pos, 1])
    inside = ((p[pos, :2] >= t[pos, :2]) & (p[pos, 2:] <= t[pos, 2:])).all(-1) | ((p[pos, :2] <= t[pos, :2]) & (p[pos, 2:] >= t[pos, 2:])).all(-1)
    assert ((ih > 0) & (iw > 0)).any() and ((ih < 0) | (iw < 0)).any() and inside.any()      # overlapping, disjoint, nested


# ---------------------------------------------------------------------------------------------- wiring, no device
def d0():
  return hparams_config.get_efficientdet_config('efficientdet-d0')


def test_config_key_still_raises_and_names_the_switch():
  config = d0()
  config.override('iou_loss_type=ciou')
  with pytest.raises(ValueError, match='not built') as e:
    train_lib.EfficientDetNetTrain(config=config)
  assert 'iou_loss=' in str(e.value) and 'set_iou_loss' in str(e.value)


def test_set_iou_loss_validates_and_is_fixed_once_an_engine_exists(monkeypatch):
  model = train_lib.EfficientDetNetTrain(config=d0())
  assert model._iou_loss is None and model._loss_keys() == ('cls_loss', 'box_loss', 'det_loss', 'reg_l2_loss', 'loss')
  model.set_iou_loss('ciou')
  assert model._iou_loss == ('ciou', 1.0)      # config.iou_loss_weight
  assert model._loss_keys()[-1] == 'box_iou_loss' and len(model._loss_keys()) == 6
  model.set_iou_loss('giou', weight=0.25)
  assert model._iou_loss == ('giou', 0.25)
  with pytest.raises(ValueError, match='Unknown loss_type xiou, not iou/ciou/diou/giou'):
    model.set_iou_loss('xiou')
  with pytest.raises(ValueError, match='not finite'):
    model.set_iou_loss('iou', weight=float('nan'))
  assert model._iou_loss == ('giou', 0.25)
  model.set_iou_loss(None)
  assert model._iou_loss is None
  kw = train_lib.EfficientDetNetTrain(config=d0(), iou_loss=dict(type='diou', weight=None))
  assert kw._iou_loss == ('diou', 1.0)
  monkeypatch.setattr(kw, 'engine', object())
  with pytest.raises(ValueError, match='set_iou_loss after the first engine was made'):
    kw.set_iou_loss('ciou')
  with pytest.raises(ValueError, match='set_iou_loss after the first engine was made'):
    kw.set_iou_loss(None)


def test_engine_gets_the_switch(monkeypatch):
  from automl_amd import efficientdet_net
  seen = []

  class FakeEngine(object):
    def __init__(self, *args, **kwargs):
      seen.append(kwargs)
      raise RuntimeError('no device in this test')
  monkeypatch.setattr(efficientdet_net.engine_lib, 'Engine', FakeEngine)
  for model, want in ((train_lib.EfficientDetNetTrain(config=d0()), None),
                      (train_lib.EfficientDetNetTrain(config=d0(), iou_loss=dict(type='ciou', weight=2.0)), ('ciou', 2.0))):
    with pytest.raises(RuntimeError, match='no device'):
      efficientdet_net.EfficientDetNet._ensure_engine(model, 1, 64, 64)
    assert seen[-1].get('iou_loss') == want and (want is not None or 'iou_loss' not in seen[-1])


def test_cli_flags(tmp_path):
  flags = train.parse_flags(['--iou_loss_type=ciou'])
  assert train.iou_loss_of(flags) == {'type': 'ciou', 'weight': None}
  flags = train.parse_flags(['--iou_loss_type', 'giou', '--iou_loss_weight', '0.5'])
  assert train.iou_loss_of(flags) == {'type': 'giou', 'weight': 0.5}
  assert train.iou_loss_of(train.parse_flags([])) is None
  with pytest.raises(ValueError, match='--iou_loss_weight needs --iou_loss_type'):
    train.iou_loss_of(train.parse_flags(['--iou_loss_weight=2']))
  with pytest.raises(SystemExit):
    train.parse_flags(['--iou_loss_type=xiou'])
  argv = ['--model_dir=%s' % tmp_path, '--mode=train', '--train_file_pattern=%s' % (tmp_path / 'none-*')]
  with pytest.raises(ValueError, match='not built') as e:
    train.main(argv + ['--hparams=iou_loss_type=ciou'])
  assert '--iou_loss_type' in str(e.value)
  with pytest.raises(ValueError, match='matches no file'):      # the flag gets as far as the data
    train.main(argv + ['--iou_loss_type=ciou'])


def test_train_state_carries_the_switch(tmp_path):
  from tests.test_train_driver import HandMadeModel, hand_made_state
  config = d0()
  off, on = HandMadeModel(config, hand_made_state(config), {}), HandMadeModel(config, hand_made_state(config), {})
  on._iou_loss = ('ciou', 1.0)
  p_off, p_on = str(tmp_path / 'off.train_state.npz'), str(tmp_path / 'on.train_state.npz')
  train_lib.save_train_state(off, p_off)
  train_lib.save_train_state(on, p_on)
  assert 'iou_loss' not in train_lib.load_train_state(p_off)[0]      # off: the file as it was
  assert train_lib.load_train_state(p_on)[0]['iou_loss'] == {'type': 'ciou', 'weight': 1.0}
  same = train_lib.EfficientDetNetTrain(config=d0(), iou_loss=dict(type='ciou'))
  assert train_lib.restore_train_state(same, p_on)['iou_loss'] == {'type': 'ciou', 'weight': 1.0}
  train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=d0()), p_off)
  with pytest.raises(ValueError, match=r"another model: the file has iou_loss type 'ciou', this model 'giou'"):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=d0(), iou_loss=dict(type='giou')), p_on)
  with pytest.raises(ValueError, match=r'another model: the file has iou_loss weight 1.0, this model 0.5'):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=d0(), iou_loss=dict(type='ciou', weight=0.5)), p_on)
  with pytest.raises(ValueError, match=r'another model: the file has iou_loss \{.*\}, this model None'):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=d0()), p_on)
  with pytest.raises(ValueError, match=r'another model: the file has iou_loss None, this model \{'):
    train_lib.restore_train_state(same, p_off)
