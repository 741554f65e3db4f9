"""Lion (lion/lion_tf2.py) without a GPU: the numpy float32 restatement tests/lion_ref.py against the two executed reference
runs of tests/golden/reference_lion.npz (make_golden_lion.py), and the configuration surface -- Update, both trainers, both
command lines, the plan properties and the training-state files."""
import json
import struct

import numpy as np
import pytest

from automl_amd import effnetv2_main, effnetv2_train, hparams_config, layer_engine, plan, train, train_lib
from automl_amd.layer_engine import Update
from tests import lion_ref
from tests.test_plan import _FakeRecorder

GOLDEN = 'tests/golden/reference_lion.npz'
F = np.float32


@pytest.fixture(scope='module')
def golden():
  import os
  with np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), GOLDEN), allow_pickle=False) as z:
    return {k: z[k] for k in z.files}


def _cases(g):
  nvar, steps = len(g['shapes']), int(g['steps'])
  for h in (0, 1):
    b1, b2, wd = (float(x) for x in g['h%d/hyper' % h])
    yield h, b1, b2, wd, nvar, steps


def _replay(g, h, how, b1, b2, wd, nvar, steps):
  """lion_ref over the fixture's inputs -> [(w list, m list, c list)] per step."""
  w = [g['h%d/w0_%d' % (h, v)].copy() for v in range(nvar)]
  m = [np.zeros_like(x) for x in w]
  out = []
  for t in range(steps):
    lr = float(g['h%d/lr' % h][t])
    c = []
    for v in range(nvar):
      grad = g['h%d/g_%d_%d' % (h, t, v)]
      c.append(lion_ref.interpolation(m[v], grad, b1, how))
      w[v], m[v], _ = lion_ref.lion_step(w[v], m[v], grad, lr, b1, b2, wd, how=how)
    out.append(([x.copy() for x in w], [x.copy() for x in m], c))
  return out


def test_fixture_holds_the_cases(golden):
  g = golden
  assert list(g['shapes']) == ['(7,)', '(5, 3)', '(1,)'] and int(g['steps']) == 4
  assert [tuple(g['h%d/hyper' % h]) for h in (0, 1)] == [(0.9, 0.99, 0.0), (0.95, 0.98, 0.1)]
  for h in (0, 1):
    assert len(set(g['h%d/lr' % h].tolist())) == 4      # a different rate each step
    assert sum(int((g['h%d/g_0_%d' % (h, v)] == 0).sum()) for v in range(3)) == 4      # sign(0) = 0 on step one
    assert all(g[k].dtype == F for k in g if '/w_' in k or '/m_' in k or '/g_' in k or '/w0_' in k)


def test_fixture_keeps_every_c_off_zero(golden):
  """The condition under which two implementations cannot differ in a sign: every |c| is exactly 0 or at least 1e-3 of the
  largest |g| of its tensor."""
  g = golden
  zeros = 0
  for h, b1, b2, wd, nvar, steps in _cases(g):
    for how in ('tf2', 'torch'):
      for t, (_, _, cs) in enumerate(_replay(g, h, how, b1, b2, wd, nvar, steps)):
        for v, c in enumerate(cs):
          bound = float(g['margin']) * np.abs(g['h%d/g_%d_%d' % (h, t, v)]).max()
          assert (((c == 0) | (np.abs(c) >= bound))).all(), (h, how, t, v, c, bound)
          zeros += int((c == 0).sum())
  assert zeros == 2 * 2 * 4


def test_restatement_equals_the_executed_tf2_run(golden):
  g = golden
  for h, b1, b2, wd, nvar, steps in _cases(g):
    for t, (ws, ms, _) in enumerate(_replay(g, h, 'tf2', b1, b2, wd, nvar, steps)):
      for v in range(nvar):
        assert np.array_equal(ws[v], g['h%d/tf2/w_%d_%d' % (h, t, v)]), (h, t, v)
        assert np.array_equal(ms[v], g['h%d/tf2/m_%d_%d' % (h, t, v)]), (h, t, v)


def _ulps(a, b):
  """Distance in float32 units in the last place (same-sign finite values; 0 for equal ones)."""
  a, b = np.asarray(a, F), np.asarray(b, F)
  ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
  assert (np.signbit(a) == np.signbit(b)).all() or np.array_equal(a, b)
  return int(np.abs(ia - ib).max()) if a.size else 0


def test_restatement_against_the_executed_pytorch_run(golden):
  """torch multiplies the decay in (p *= 1 - lr wd) and its add_(alpha=) may fuse: equal signs always, equal variables
  with wd = 0, two float32 ulp otherwise."""
  g = golden
  for h, b1, b2, wd, nvar, steps in _cases(g):
    w_prev = [g['h%d/w0_%d' % (h, v)] for v in range(nvar)]
    for t, (ws, ms, cs) in enumerate(_replay(g, h, 'torch', b1, b2, wd, nvar, steps)):
      lr = float(g['h%d/lr' % h][t])
      for v in range(nvar):
        tw, tm = g['h%d/torch/w_%d_%d' % (h, t, v)], g['h%d/torch/m_%d_%d' % (h, t, v)]
        # the sign torch applied, recovered from its own step: (decayed w - w') / lr
        tw_prev = w_prev[v]
        applied = np.sign(np.round((tw_prev.astype(np.float64) * (1 - lr * wd) - tw.astype(np.float64)) / lr))
        assert np.array_equal(applied, lion_ref.sign(cs[v]).astype(np.float64)), (h, t, v)
        if wd == 0:
          assert np.array_equal(ws[v], tw), (h, t, v)
        else:
          assert _ulps(ws[v], tw) <= 2, (h, t, v, _ulps(ws[v], tw))
        assert _ulps(ms[v], tm) <= 2, (h, t, v, _ulps(ms[v], tm))
      w_prev = [g['h%d/torch/w_%d_%d' % (h, t, v)] for v in range(nvar)]


def test_one_minus_switch_and_sign():
  assert lion_ref.one_minus(0.9, 'tf2') == F(1) - F(0.9) and lion_ref.one_minus(0.9, 'torch') == F(1.0 - 0.9)
  assert lion_ref.one_minus(0.9, 'tf2') != lion_ref.one_minus(0.9, 'torch')      # the two differ by an ulp here
  s = lion_ref.sign(np.array([-2.0, -0.0, 0.0, 3.0, np.nan], F))
  assert np.array_equal(s[:4], [-1, 0, 0, 1]) and np.isnan(s[4])
  w, m, ema = lion_ref.lion_step(np.array([1.0, -0.0], F), np.zeros(2, F), np.array([0.0, 0.0], F), 0.5, wd=0.0,
                                 ema=np.array([2.0, 2.0], F), decay=0.5)
  assert np.array_equal(w, [1.0, 0.0]) and np.array_equal(m, [0, 0]) and np.array_equal(ema, [1.5, 1.0])


# ---- configuration -----------------------------------------------------------------------------------------------------
def test_update_keeps_its_positional_forms():
  assert Update('sgd', 0.9) == ('sgd', 0.9, None, None, None, None)
  assert Update('adam', 0.9, 0.999, 1e-7) == ('adam', 0.9, 0.999, 1e-7, None, None)
  assert Update('rmsprop', 0.9, epsilon=0.001, rho=0.9) == ('rmsprop', 0.9, None, 0.001, 0.9, None)
  assert Update('rmsprop', 0.9, None, 0.001, 0.9).wd is None
  u = Update('lion', 0.9, 0.99, wd=0.1)
  assert (u.kind, u.momentum, u.beta2, u.wd, u.epsilon, u.rho) == ('lion', 0.9, 0.99, 0.1, None, None)
  assert Update._fields == ('kind', 'momentum', 'beta2', 'epsilon', 'rho', 'wd')


def test_classifier_constructs_with_lion():
  net = effnetv2_train.TrainableModel('efficientnetv2-b0', 'num_classes=24', optimizer='lion')
  assert net.engine is None and net.optimizer == 'lion' and net.update == Update('lion', 0.9, 0.99, wd=0.0)
  net = effnetv2_train.TrainableModel('efficientnetv2-b0', 'num_classes=24', optimizer='Lion', momentum=0.95, lion_beta2=0.98,
                                      lion_wd=0.1)
  assert net.update == Update('lion', 0.95, 0.98, wd=0.1)
  assert 'lion' in effnetv2_train.OPTIMIZERS and effnetv2_train.build_update('lion', 0.9).kind == 'lion'
  assert effnetv2_train.build_update('rmsprop', 0.9) == Update('rmsprop', 0.9, epsilon=0.001, rho=0.9)      # as before
  for bad in (dict(lion_beta2=1.0), dict(lion_wd=-0.1), dict(momentum=1.0)):
    with pytest.raises(ValueError, match='lion'):
      effnetv2_train.TrainableModel('efficientnetv2-b0', 'num_classes=24', optimizer='lion', **bad)


def _det_config(optimizer='lion'):
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  config.override('optimizer=%s' % optimizer)
  return config


def test_detector_constructs_with_lion_and_set_lion_is_refused_once_an_engine_exists():
  net = train_lib.EfficientDetNetTrain(config=_det_config())
  assert net.engine is None and net.update == Update('lion', 0.9, 0.99, wd=0.0)      # beta_1 = config.momentum
  net.set_lion(wd=0.1)
  assert net.update == Update('lion', 0.9, 0.99, wd=0.1)
  net.set_lion(beta_2=0.98)      # None keeps a value
  assert net.update == Update('lion', 0.9, 0.98, wd=0.1)
  net = train_lib.EfficientDetNetTrain(config=_det_config(), lion=dict(beta_2=0.98, wd=0.05))
  assert net.update == Update('lion', 0.9, 0.98, wd=0.05) and net._lion == {'beta_2': 0.98, 'wd': 0.05}
  with pytest.raises(ValueError, match='beta_2'):
    net.set_lion(beta_2=1.5)
  with pytest.raises(ValueError, match='unknown option'):
    layer_engine.lion_options({'beta_3': 1})
  net.engine = object()      # what the first step leaves
  with pytest.raises(ValueError, match='after the first engine was made'):
    net.set_lion(wd=0.2)
  assert net.update.wd == 0.05
  # another optimizer has no Lion options; rmsprop keeps raising for the detector
  with pytest.raises(ValueError, match='set_lion needs config.optimizer = lion'):
    train_lib.EfficientDetNetTrain(config=_det_config('sgd'), lion=dict(wd=0.1))
  assert train_lib.EfficientDetNetTrain(config=_det_config('adam')).update == Update('adam', 0.9, 0.999, 1e-7)
  with pytest.raises(ValueError, match='rmsprop'):
    train_lib.EfficientDetNetTrain(config=_det_config('rmsprop'))


def test_command_lines_parse_the_lion_flags():
  flags = train.parse_flags(['--model_dir=/tmp/x', '--hparams=optimizer=lion', '--lion_beta2=0.98', '--lion_wd=0.1'])
  config = train.build_config(flags)
  assert config.optimizer == 'lion' and train.lion_of(flags, config) == {'beta_2': 0.98, 'wd': 0.1}
  plain = train.parse_flags(['--model_dir=/tmp/x'])
  assert plain.lion_beta2 is None and plain.lion_wd is None and train.lion_of(plain, train.build_config(plain)) is None
  with pytest.raises(ValueError, match='need --hparams=optimizer=lion'):
    train.lion_of(train.parse_flags(['--lion_wd=0.1']), train.build_config(plain))
  v2 = effnetv2_main.parse_flags(['--hparam_str=train.optimizer=lion,data.augname=None', '--lion_beta2=0.97', '--lion_wd=0.01'])
  assert (v2.lion_beta2, v2.lion_wd) == (0.97, 0.01)
  assert effnetv2_main.build_config(v2).train.optimizer == 'lion'
  none = effnetv2_main.parse_flags([])
  assert none.lion_beta2 is None and none.lion_wd is None


def test_classifier_command_line_builds_a_lion_model():
  flags = effnetv2_main.parse_flags(['--hparam_str=train.optimizer=lion,data.augname=None', '--lion_beta2=0.97', '--lion_wd=0.01'])
  config = effnetv2_main.build_config(flags)
  model = effnetv2_main.build_model(flags, config, effnetv2_main.plan_of(config))
  assert model.update == Update('lion', 0.9, 0.97, wd=0.01) and model.engine is None
  other = effnetv2_main.parse_flags(['--hparam_str=data.augname=None', '--lion_wd=0.01'])
  config = effnetv2_main.build_config(other)
  with pytest.raises(ValueError, match='need train.optimizer=lion'):
    effnetv2_main.build_model(other, config, effnetv2_main.plan_of(config))


def test_plan_properties_round_trip(tmp_path):
  props = plan.optimizer_props(Update('lion', 0.95, 0.98, wd=0.1), 7)
  assert props['optimizer'] == 2 and props['iterations'] == 7
  assert sorted(props) == ['iterations', 'lion_beta1_bits', 'lion_beta2_bits', 'lion_wd_bits', 'optimizer']
  rec = _FakeRecorder()
  rec.begin('forward', main_stream=0)
  rec.on_call('edet_zero', (0x10000 + 128, 256, 0))
  rec.end()
  rec.names['params'] = (0x20000, 4096)
  rec.props.update(props)
  path = str(tmp_path / 'lion.plan')
  rec.write(path)
  for got in (plan.read_plan(path), plan.read_summary(path)):
    names = got['names']
    assert names['optimizer'][:2] == (plan.NULL_BUF, 2) and names['iterations'][1] == 7
    for key, want in (('lion_beta1_bits', 0.95), ('lion_beta2_bits', 0.98), ('lion_wd_bits', 0.1)):
      assert plan.bits_double(names[key][1]) == want == struct.unpack('<d', struct.pack('<Q', names[key][1]))[0]
  # the other kinds write what they wrote before
  assert plan.optimizer_props(Update('sgd', 0.9), 3) == {'optimizer': 0, 'iterations': 3}
  adam = plan.optimizer_props(Update('adam', 0.9, 0.999, 1e-7), 0)
  assert adam['optimizer'] == 1 and sorted(adam) == ['adam_beta1_bits', 'adam_beta2_bits', 'adam_epsilon_bits', 'iterations',
                                                     'optimizer']
  assert plan.bits_double(adam['adam_epsilon_bits']) == 1e-7
  with pytest.raises(ValueError, match='rmsprop'):
    plan.optimizer_props(Update('rmsprop', 0.9, epsilon=0.001, rho=0.9), 0)


# ---- training-state files ----------------------------------------------------------------------------------------------
class _HandMadeDetector(object):
  """What train_lib.save_train_state reads of a model."""
  _engines = {}

  def __init__(self, config, lion=None):
    self.config = config
    self.update = train_lib.EfficientDetNetTrain(config=config, lion=lion).update
    n = train_lib.arena_length(self)
    self.state = {'velocity': np.full(n, 0.25, F), 'ema': np.zeros(n, F), 'iterations': 3}

  def get_optimizer_state(self):
    return self.state


def _meta(path):
  with np.load(path, allow_pickle=False) as z:
    return json.loads(z['meta'].tobytes().decode('utf-8')), sorted(z.files)


def test_detector_train_state_carries_lion_and_refuses_a_mismatch(tmp_path):
  path = str(tmp_path / 'ckpt-1.train_state.npz')
  train_lib.save_train_state(_HandMadeDetector(_det_config(), dict(beta_2=0.98, wd=0.1)), path)
  meta, members = _meta(path)
  assert meta['optimizer'] == 'lion' and meta['lion'] == {'beta_2': 0.98, 'wd': 0.1}
  assert members == ['ema', 'meta', 'velocity']      # one slot: no second arena in the file
  same = train_lib.EfficientDetNetTrain(config=_det_config(), lion=dict(beta_2=0.98, wd=0.1))
  train_lib.restore_train_state(same, path)
  assert same.iterations == 3 and float(same._pending_state['velocity'][0]) == 0.25
  with pytest.raises(ValueError, match='the file has lion as optimizer, this model sgd'):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=_det_config('sgd')), path)
  with pytest.raises(ValueError, match=r"the file has lion wd 0\.1, this model 0\.0"):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=_det_config(), lion=dict(beta_2=0.98)), path)
  with pytest.raises(ValueError, match=r"lion beta_2 0\.98, this model 0\.99; lion wd 0\.1, this model 0\.0"):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=_det_config()), path)
  # and the reverse: an SGD state into a Lion model
  sgd = str(tmp_path / 'sgd.train_state.npz')
  train_lib.save_train_state(_HandMadeDetector(_det_config('sgd')), sgd)
  assert 'lion' not in _meta(sgd)[0]
  with pytest.raises(ValueError, match='the file has sgd as optimizer, this model lion'):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=_det_config()), sgd)


def test_classifier_train_state_carries_lion_and_refuses_a_mismatch(tmp_path):
  def small(**kw):
    return effnetv2_train.TrainableModel('efficientnetv2-b0', 'num_classes=24', **kw)
  src = small(optimizer='lion', lion_wd=0.1)
  n = train_lib.arena_length(src)
  src._pending_state = {'velocity': np.full(n, 0.5, F), 'ema': np.zeros(n, F), 'iterations': 5}
  path = str(tmp_path / 'ckpt-5.train_state.npz')
  effnetv2_train.save_train_state(src, path)
  meta, members = _meta(path)
  assert meta['optimizer'] == 'lion' and meta['lion'] == {'beta_2': 0.99, 'wd': 0.1} and 'rms' not in members
  dst = small(optimizer='lion', lion_wd=0.1)
  effnetv2_train.restore_train_state(dst, path)
  assert dst.iterations == 5
  with pytest.raises(ValueError, match='the file has lion as optimizer, this model momentum'):
    effnetv2_train.restore_train_state(small(optimizer='momentum'), path)
  with pytest.raises(ValueError, match=r'the file has lion wd 0\.1, this model 0\.0'):
    effnetv2_train.restore_train_state(small(optimizer='lion'), path)
  with pytest.raises(ValueError, match=r'the file has lion beta_2 0\.99, this model 0\.9$'):
    effnetv2_train.restore_train_state(small(optimizer='lion', lion_beta2=0.9, lion_wd=0.1), path)
