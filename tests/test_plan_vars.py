"""The variable table of a step plan, state files and Adam's bias-corrected rate (include/edet_net.h: edet_net_variable_info,
edet_net_save_state, edet_train_step), the parts that need no GPU: writer and reader of automl_amd/plan.py agree, a bad
file is refused, and the operation order the C runtime follows for alpha is the Python engine's."""
import math
import struct

import numpy as np
import pytest

from automl_amd import engine, plan
from tests.test_plan import _FakeRecorder


def _bits(x):
  return struct.unpack('<Q', struct.pack('<d', x))[0]


def _record(rec):
  rec.begin('forward', main_stream=0)
  rec.on_call('edet_zero', (0x10000 + 128, 256, 0))
  rec.end()
  rec.names['params'] = (0x20000, 4096)
  rec.props['batch'] = 2


VARS = [('class_net/class-predict/bias', (810,), True, 0, 810),
        ('stem/conv2d/kernel', (3, 3, 3, 32), True, 812, 864),
        ('fpn_cells/cell_0/fnode0/WSM', (), True, 1676, 1),
        ('stem/tpu_batch_normalization/moving_mean', (32,), False, 0, 32)]


def test_variable_table_and_optimizer_properties_round_trip(tmp_path):
  rec = _FakeRecorder()
  _record(rec)
  rec.variables = list(VARS)
  rec.props.update({'optimizer': 1, 'iterations': 7, 'adam_beta1_bits': _bits(0.9),
                    'adam_beta2_bits': _bits(engine.Engine.ADAM_BETA2), 'adam_epsilon_bits': _bits(engine.Engine.ADAM_EPSILON)})
  path = str(tmp_path / 'vars.plan')
  rec.write(path)
  for got in (plan.read_plan(path), plan.read_summary(path)):
    assert [(v['name'], v['shape'], v['trainable'], v['offset'], v['count']) for v in got['variables']] == VARS
    names = got['names']
    assert names['num_variables'][:2] == (plan.NULL_BUF, len(VARS))
    assert names['optimizer'][1] == 1 and names['iterations'][1] == 7
    for key, want in (('adam_beta1_bits', 0.9), ('adam_beta2_bits', 0.999), ('adam_epsilon_bits', 1e-7)):
      assert struct.unpack('<d', struct.pack('<Q', names[key][1]))[0] == want
  assert plan.read_plan(path)['ops']['forward'][0][1] == 'edet_zero'


def test_plan_without_a_table_reads_as_before_plus_an_empty_table(tmp_path):
  rec = _FakeRecorder()
  _record(rec)
  path = str(tmp_path / 'plain.plan')
  rec.write(path)
  got = plan.read_plan(path)
  assert got['variables'] == [] and plan.read_summary(path)['variables'] == []
  assert set(got['names']) == {'params', 'batch'}      # no property announces a table
  assert got['names']['params'] == (1, 0, 4096) and got['names']['batch'][:2] == (plan.NULL_BUF, 2)
  assert set(got) == {'version', 'entry_points', 'buffers', 'names', 'streams', 'events', 'programs', 'device_relocations',
                      'ops', 'device_relocation_table', 'variables'}
  # the same recording with a table differs from it by the table and its property only: what was there stays byte for byte
  rec2 = _FakeRecorder()
  _record(rec2)
  rec2.variables = list(VARS)
  path2 = str(tmp_path / 'table.plan')
  rec2.write(path2)
  with_table = plan.read_plan(path2)
  assert with_table['ops'] == got['ops'] and with_table['buffers'] == got['buffers']


def test_a_table_that_is_announced_and_missing_is_refused(tmp_path):
  rec = _FakeRecorder()
  _record(rec)
  rec.props['num_variables'] = 3      # the property without the section
  path = str(tmp_path / 'bad.plan')
  rec.write(path)
  with pytest.raises(ValueError, match='variable table'):
    plan.read_plan(path)


def test_state_file_round_trip_and_refusals(tmp_path):
  rng = np.random.default_rng(3)
  values = {'class_net/class-predict/bias': rng.standard_normal((810,)).astype(np.float32),
            'stem/conv2d/kernel': rng.standard_normal((3, 3, 3, 32)).astype(np.float32),
            'fpn_cells/cell_0/fnode0/WSM': np.float32(0.75).reshape(()),
            'stem/tpu_batch_normalization/moving_mean': rng.standard_normal((32,)).astype(np.float32)}
  train = {k: v for k, v in values.items() if 'moving' not in k}
  ema = {k: v * 2 for k, v in train.items()}
  mom = {k: v * 3 for k, v in train.items()}
  adam_v = {k: v * v for k, v in train.items()}
  path = str(tmp_path / 'net.state')
  plan.write_state(path, values, ema=ema, momentum=mom, adam_v=adam_v, iterations=12345678901)
  got = plan.read_state(path)
  assert got['iterations'] == 12345678901
  for key, want in (('variables', values), ('ema', ema), ('momentum', mom), ('adam_v', adam_v)):
    assert list(got[key]) == list(want)
    for name, w in want.items():
      assert got[key][name].shape == w.shape and got[key][name].dtype == np.float32, (key, name)
      assert np.array_equal(got[key][name].view(np.uint32), np.asarray(w).view(np.uint32)), (key, name)
  assert got['variables']['fpn_cells/cell_0/fnode0/WSM'].shape == ()
  # SGD state: no second moments
  plan.write_state(path, values, ema=ema, momentum=mom, iterations=3)
  assert plan.read_state(path)['adam_v'] == {} and plan.read_state(path)['iterations'] == 3
  raw = open(path, 'rb').read()
  for cut in (4, 12, 30, len(raw) // 2, len(raw) - 1):
    bad = tmp_path / ('cut%d.state' % cut)
    bad.write_bytes(raw[:cut])
    with pytest.raises(ValueError):
      plan.read_state(str(bad))
  bad = tmp_path / 'magic.state'
  bad.write_bytes(b'EDETPLAN' + raw[8:])
  with pytest.raises(ValueError, match='not a state file'):
    plan.read_state(str(bad))
  bad = tmp_path / 'tail.state'
  bad.write_bytes(raw + b'\0')
  with pytest.raises(ValueError, match='after the last record'):
    plan.read_state(str(bad))


def test_alpha_in_the_runtimes_operation_order_is_the_engines():
  """csrc/net_runtime.cpp: alpha = (double)lr * sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t)), then (float).  Here with
  math.pow / math.sqrt (the same libm functions) against Engine.set_hyper's expression, t = 1 .. 50, beta1 = 0.9."""
  b1, b2 = 0.9, engine.Engine.ADAM_BETA2
  for lr in (float(np.float32(0.003)), float(np.float32(0.08)), 0.015625):
    for t in range(1, 51):
      transcribed = np.float32(lr * math.sqrt(1.0 - math.pow(b2, float(t))) / (1.0 - math.pow(b1, float(t))))
      engine_expr = np.float32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))      # engine.py: Engine.set_hyper
      assert transcribed.view(np.uint32) == engine_expr.view(np.uint32), (lr, t)
  # what the issue is about: at t = 1 the corrected rate is about a third of the raw one
  assert 0.3 < math.sqrt(1.0 - b2) / (1.0 - b1) < 0.33
