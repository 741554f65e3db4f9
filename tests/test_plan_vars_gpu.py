"""Variables by name, saved state and Adam steps through the network-level C ABI (include/edet_net.h) against the Python
host, BIT FOR BIT (uint32 views; both sides are this code base's own hosts): the variable table equals the arena,
edet_get_variable / edet_set_variable, the refusals, the Adam replay with the runtime's own bias-corrected rate, resuming
from a state file in a fresh process of a C99 host (tests/c_host/edet_vars_host.c), and plans without their inputs."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from automl_amd import _lib, hparams_config, net_c, plan, train_lib
from tests.test_gpu_network import make_labels, perturbed_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 256
LR, DECAY = float(np.float32(0.02)), float(np.float32(0.9))
HOST_LR, HOST_DECAY = 0.015625, 0.875      # LEARNING_RATE / EMA_DECAY of tests/c_host/edet_vars_host.c
BIAS = 'class_net/class-predict/bias'
STATE_KEYS = ('params', 'ema', 'velocity', 'bn_state', 'loss_sums')


def _record(tmp_path_factory, tag, override):
  d = tmp_path_factory.mktemp('plan_' + tag)
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  if override:
    config.override(override)
  net = train_lib.EfficientDetNetTrain(config=config, dtype='bf16', params=perturbed_params(config, 11), seed=5)
  rng = np.random.default_rng(97)
  images = torch.from_numpy(rng.standard_normal((2, SIZE, SIZE, 3)).astype(np.float32))
  labels = make_labels(config, 2, SIZE, 101)
  path = str(d / ('d0_256_b2_%s.plan' % tag))
  summary, expected = plan.record_network(net, images, labels, path, learning_rate=LR, ema_decay=DECAY, keep_inputs=False)
  eng = net._ensure_engine(2, SIZE, SIZE)
  dimages = net._to_device_images(images, eng)
  dl = net._labels_to_device(labels, eng)
  inputs = {'images': dimages.view(torch.uint8).cpu().numpy().reshape(-1)}
  inputs.update({k: t.cpu().numpy() for k, t in dl.items() if torch.is_tensor(t)})
  return {'path': path, 'summary': summary, 'expected': expected, 'net': net, 'eng': eng, 'images': images, 'labels': labels,
          'dimages': dimages, 'dl': dl, 'inputs': inputs, 'dir': str(d), 'config': config}


@pytest.fixture(scope='module')
def sgd(tmp_path_factory):
  return _record(tmp_path_factory, 'sgd', None)


@pytest.fixture(scope='module')
def adam(tmp_path_factory):
  return _record(tmp_path_factory, 'adam', 'optimizer=adam')


def _open(rec):
  cnet = net_c.CNet(rec['path'])
  for k, a in rec['inputs'].items():
    cnet.write(k, a)
  return cnet


def _u32(a):
  return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _logits(cnet, config, kind):
  out = []
  for level in range(config.min_level, config.max_level + 1):
    name = '%s_outputs_%d' % (kind, level)
    eb, ld, ch = cnet.prop(name + '.elem_bytes'), cnet.prop(name + '.ld'), cnet.prop(name + '.channels')
    out.append(cnet.read(name).reshape(-1, ld * eb)[:, :ch * eb].copy())
  return out


def _state_equal(cnet, eng, keys, what):
  torch.cuda.synchronize()
  tensors = {'params': eng.params_flat, 'ema': eng.ema, 'velocity': eng.velocity, 'bn_state': eng.state_flat,
             'loss_sums': eng.loss_sums, 'adam_v': getattr(eng.arena, 'adam_v', None)}
  for k in keys:
    got, want = cnet.read(k).view(np.uint32), _u32(tensors[k].detach().cpu().numpy())
    print('%s, %s: %d of %d elements differ' % (what, k, int((got != want).sum()), want.size))
    assert np.array_equal(got, want), '%s, %s: %d of %d elements differ' % (what, k, int((got != want).sum()), want.size)


def test_variable_table_equals_the_arena_and_get_variable_reads_every_slot(sgd):
  eng, exp = sgd['eng'], sgd['expected']
  cnet = _open(sgd)
  try:
    offsets = eng.arena.offsets
    table = cnet.variables()
    assert len(table) == 709
    assert [(n, tuple(s), t) for n, s, t in table] == [(n, tuple(o[2]), o[3]) for n, o in offsets.items()]
    assert cnet.prop('optimizer') == 0 and cnet.iterations == cnet.prop('iterations') >= 1
    assert 'adam_v' not in cnet.names()
    before = cnet.iterations
    cnet.train_step(LR, DECAY)      # = the recorded step
    assert cnet.iterations == before + 1
    for name, (off, n, shape, tr) in offsets.items():
      slots = ((net_c.SLOT_VALUE, 'params'), (net_c.SLOT_EMA, 'ema'), (net_c.SLOT_MOMENTUM, 'velocity')) if tr else \
          ((net_c.SLOT_VALUE, 'bn_state'),)
      for slot, key in slots:
        got = cnet.get_variable(name, slot)
        assert got.shape == tuple(shape), name
        assert np.array_equal(_u32(got), _u32(exp[key][off:off + n])), (name, key)
  finally:
    cnet.close()


def test_set_variable_by_name_equals_set_weights_on_the_python_host(sgd):
  """Runs after the recorded step on both sides (the Python engine is one step past the plan's snapshot)."""
  net, eng, config = sgd['net'], sgd['eng'], sgd['config']
  cnet = _open(sgd)
  try:
    cnet.train_step(LR, DECAY)
    _state_equal(cnet, eng, ('params', 'bn_state'), 'before the write')
    cnet.forward()
    cls0, box0 = _logits(cnet, config, 'cls'), _logits(cnet, config, 'box')
    v = np.random.default_rng(5).standard_normal(cnet.get_variable(BIAS).shape).astype(np.float32)
    old = eng.get_params([BIAS])[BIAS].copy()
    ema_before = cnet.get_variable(BIAS, net_c.SLOT_EMA)
    cnet.set_variable(BIAS, v)
    assert np.array_equal(_u32(cnet.get_variable(BIAS)), _u32(v))
    assert np.array_equal(_u32(cnet.get_variable(BIAS, net_c.SLOT_EMA)), _u32(ema_before)), 'iterations > 0: no EMA seeding'
    net.set_weights({BIAS: v})
    try:
      cnet.forward()
      eng.forward(sgd['dimages'], training=False)
      torch.cuda.synchronize()
      cls1, box1 = _logits(cnet, config, 'cls'), _logits(cnet, config, 'box')
      for li, (cv, bv) in enumerate(zip(eng.cls_views, eng.box_views)):
        for got, view in ((cls1[li], cv), (box1[li], bv)):
          r = view.raw
          eb = r.data.element_size()
          want = r.data.detach().view(torch.uint8).cpu().numpy().reshape(-1, r.ld * eb)[:, :r.c * eb]
          assert np.array_equal(got, want), 'level %d: %d bytes differ' % (li, int((got != want).sum()))
        assert not np.array_equal(cls1[li], cls0[li]), 'class logits of level %d did not move' % li
        assert np.array_equal(box1[li], box0[li]), 'box logits of level %d moved' % li
    finally:
      net.set_weights({BIAS: old})
    # iterations == 0: the moving average follows the variable (ParamArena.set_params)
    cnet.iterations = 0
    cnet.set_variable(BIAS, v * 2)
    assert np.array_equal(_u32(cnet.get_variable(BIAS, net_c.SLOT_EMA)), _u32(v * 2))
  finally:
    cnet.close()


def test_refusals_name_the_variable_and_leave_the_network_intact(sgd):
  exp = sgd['expected']
  cnet = _open(sgd)
  lib = cnet.lib
  buf = np.zeros(4096, np.float32)
  mean = next(n for n, o in sgd['eng'].arena.offsets.items() if n.endswith('/moving_mean'))
  try:
    cases = [('get unknown', lambda: lib.edet_get_variable(cnet.h, b'no/such/variable', 0, buf.ctypes.data, buf.size), 'no/such/variable'),
             ('set unknown', lambda: lib.edet_set_variable(cnet.h, b'no/such/variable', 0, buf.ctypes.data, 4), 'no/such/variable'),
             ('set wrong count', lambda: lib.edet_set_variable(cnet.h, BIAS.encode(), 0, buf.ctypes.data, 809), BIAS),
             ('get small capacity', lambda: lib.edet_get_variable(cnet.h, BIAS.encode(), 0, buf.ctypes.data, 809), BIAS),
             ('adam_v on sgd', lambda: lib.edet_get_variable(cnet.h, BIAS.encode(), net_c.SLOT_ADAM_V, buf.ctypes.data, buf.size), BIAS),
             ('set adam_v on sgd', lambda: lib.edet_set_variable(cnet.h, BIAS.encode(), net_c.SLOT_ADAM_V, buf.ctypes.data, 810), BIAS),
             ('ema of a moving mean', lambda: lib.edet_get_variable(cnet.h, mean.encode(), net_c.SLOT_EMA, buf.ctypes.data, buf.size), mean),
             ('set ema of a moving mean', lambda: lib.edet_set_variable(cnet.h, mean.encode(), net_c.SLOT_EMA, buf.ctypes.data,
                                                                        cnet.get_variable(mean).size), mean)]
    for what, fn, name in cases:
      assert fn() != 0, what
      assert name in lib.edet_last_error().decode(), (what, lib.edet_last_error())
    with pytest.raises(_lib.EdetError, match='no/such/variable'):
      cnet.get_variable('no/such/variable')
    cnet.train_step(LR, DECAY)
    for k in STATE_KEYS:
      assert np.array_equal(cnet.read(k).view(np.uint32), _u32(exp[k])), k
  finally:
    cnet.close()


def test_adam_replay_forms_the_bias_corrected_rate_itself(adam):
  """The C replay (graph mode) of the recorded step and of three more steps with three rates equals plan.train_pass on the
  Python engine after every step: the runtime takes the RAW rate and forms alpha from its own iteration count.
  (Before plans named "adam_v" and carried the optimizer, this failed at the first read of "adam_v" -- and the step was
  taken with the raw rate, about 3x alpha at t = 1.)"""
  eng, exp = adam['eng'], adam['expected']
  assert eng.adam
  keys = STATE_KEYS + ('adam_v',)
  cnet = _open(adam)
  try:
    assert cnet.prop('optimizer') == 1 and 'adam_v' in cnet.names()
    t0 = cnet.iterations
    assert t0 == eng.arena.step_count - 1
    cnet.use_graph(True)
    st = torch.cuda.Stream()
    cnet.train_step(LR, DECAY, st.cuda_stream)      # = the recorded step
    st.synchronize()
    for k in keys:
      got, want = cnet.read(k).view(np.uint32), _u32(exp[k])
      print('recorded step, %s: %d of %d elements differ' % (k, int((got != want).sum()), want.size))
      assert np.array_equal(got, want), 'recorded step, %s: %d elements differ' % (k, int((got != want).sum()))
    for step, rate in enumerate((0.003, 0.01, 0.0007)):
      lr = float(np.float32(rate))
      plan.train_pass(eng, adam['dimages'], adam['dl'], lr, DECAY)
      cnet.train_step(lr, DECAY, st.cuda_stream)
      st.synchronize()
      _state_equal(cnet, eng, keys, 'step %d' % step)
      assert cnet.iterations == eng.arena.step_count == t0 + 2 + step
    name = next(iter(eng.arena.offsets))
    off, n = eng.arena.offsets[name][:2]
    assert np.array_equal(_u32(cnet.get_variable(name, net_c.SLOT_ADAM_V)), _u32(eng.arena.adam_v[off:off + n].cpu().numpy()))
  finally:
    cnet.close()


def _build_host(workdir):
  gcc = shutil.which('gcc')
  if gcc is None or not os.path.exists('/opt/rocm/include/hip/hip_runtime_api.h'):
    pytest.skip('no C toolchain / HIP headers on this box')
  libdir = os.path.join(ROOT, 'automl_amd')
  exe = os.path.join(workdir, 'edet_vars_host')
  cmd = [gcc, '-std=c99', '-O1', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include',
         os.path.join(ROOT, 'tests', 'c_host', 'edet_vars_host.c'), '-o', exe, '-L' + libdir, '-ledet_hip', '-L/opt/rocm/lib',
         '-lamdhip64', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib']
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  return exe


def _host(exe, args, rec=None, out=None):
  if out is not None:
    os.makedirs(out, exist_ok=True)
    for k, a in rec['inputs'].items():
      np.ascontiguousarray(a).tofile(os.path.join(out, k.replace('/', '_').replace(':', '_') + '.in'))
  env = {k: v for k, v in os.environ.items() if not k.startswith('PYTHON')}
  r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
  assert r.returncode == 0, (args, r.stdout, r.stderr)
  assert 'ok' in r.stdout
  return r.stdout


def _dumps(out, keys):
  got = {k: np.fromfile(os.path.join(out, k + '.bin'), dtype=np.uint32) for k in keys}
  got['iterations'] = int(open(os.path.join(out, 'iterations.txt')).read())
  return got


@pytest.mark.parametrize('which', ['sgd', 'adam'])
def test_c_host_resumes_from_a_state_file_in_a_fresh_process(which, request):
  rec = request.getfixturevalue(which)
  exe = _build_host(rec['dir'])
  keys = STATE_KEYS + (('adam_v',) if which == 'adam' else ())
  d = rec['dir']
  listing = _host(exe, ['list', rec['path']]).splitlines()
  assert len(listing) == 709 + 1 and '%s 1 810 1' % BIAS in listing
  full, half, rest = (os.path.join(d, 'out_' + n) for n in ('full', 'half', 'rest'))
  state = os.path.join(d, 'half.state')
  _host(exe, ['train', rec['path'], full, 4], rec, full)
  _host(exe, ['train', rec['path'], half, 2, '-', state], rec, half)
  _host(exe, ['train', rec['path'], rest, 2, state], rec, rest)
  a, b, h = _dumps(full, keys), _dumps(rest, keys), _dumps(half, keys)
  t0 = plan.read_summary(rec['path'])['names']['iterations'][1]
  assert a['iterations'] == b['iterations'] == t0 + 4 and h['iterations'] == t0 + 2
  for k in keys:
    assert np.array_equal(a[k], b[k]), '%s, %s: %d elements differ' % (which, k, int((a[k] != b[k]).sum()))
    if k != 'bn_state' and k != 'loss_sums':
      assert not np.array_equal(a[k], h[k]), k      # the last two steps did something
  # the saved state carries the run to the Python host: a fresh network takes the same next two steps
  saved = plan.read_state(state)
  assert saved['iterations'] == t0 + 2 and set(saved['variables']) == set(rec['eng'].arena.offsets)
  net = train_lib.EfficientDetNetTrain(config=rec['config'], dtype='bf16', params=perturbed_params(rec['config'], 3), seed=9)
  eng = net._ensure_engine(2, SIZE, SIZE)
  net.set_weights(saved['variables'])
  flat = {}
  for key, slot in (('ema', 'ema'), ('velocity', 'momentum')) + ((('adam_v', 'adam_v'),) if which == 'adam' else ()):
    arr = np.zeros(eng.params_flat.numel(), np.float32)
    for name, (off, n, shape, tr) in eng.arena.offsets.items():
      if tr:
        arr[off:off + n] = saved[slot][name].reshape(-1)
    flat[key] = arr
  flat['iterations'] = saved['iterations']
  net.set_optimizer_state(flat)
  dimages = net._to_device_images(rec['images'], eng)
  dl = net._labels_to_device(rec['labels'], eng)
  for _ in range(2):
    plan.train_pass(eng, dimages, dl, HOST_LR, HOST_DECAY)
  torch.cuda.synchronize()
  tensors = {'params': eng.params_flat, 'ema': eng.ema, 'velocity': eng.velocity, 'bn_state': eng.state_flat,
             'loss_sums': eng.loss_sums, 'adam_v': getattr(eng.arena, 'adam_v', None)}
  for k in keys:
    want = _u32(tensors[k].detach().cpu().numpy())
    assert np.array_equal(b[k], want), '%s, python resume, %s: %d elements differ' % (which, k, int((b[k] != want).sum()))
  assert eng.arena.step_count == b['iterations']
  # a state of the other optimizer, or of nothing, is refused and changes nothing
  cnet = _open(rec)
  try:
    bad = os.path.join(d, 'short.state')
    some = dict(list(saved['variables'].items())[:-1])
    plan.write_state(bad, some, ema=saved['ema'], momentum=saved['momentum'], adam_v=saved['adam_v'], iterations=1)
    missing = list(saved['variables'])[-1]
    with pytest.raises(_lib.EdetError, match=re.escape(missing)):
      cnet.load_state(bad)
    assert cnet.iterations == t0
  finally:
    cnet.close()


def test_c_host_sets_a_variable_by_name(sgd):
  exe = _build_host(sgd['dir'])
  out = os.path.join(sgd['dir'], 'out_setvar')
  _host(exe, ['setvar', sgd['path'], out, BIAS, '0.5'], sgd, out)
  cnet = _open(sgd)
  try:
    cnet.forward()
    before = [cnet.read('cls_outputs_%d' % l) for l in range(3, 8)]
    cnet.set_variable(BIAS, np.full((810,), 0.5, np.float32))
    cnet.forward()
    after = [cnet.read('cls_outputs_%d' % l) for l in range(3, 8)]
  finally:
    cnet.close()
  for i, level in enumerate(range(3, 8)):
    b = np.fromfile(os.path.join(out, 'cls_outputs_%d.before.bin' % level), dtype=np.uint8)
    a = np.fromfile(os.path.join(out, 'cls_outputs_%d.after.bin' % level), dtype=np.uint8)
    ld, ch = (810 + 7) // 8 * 8, 810
    eb = b.size // (2 * (SIZE >> level) ** 2 * ld)
    cut = lambda x: x.reshape(-1, ld * eb)[:, :ch * eb]
    assert np.array_equal(cut(b), cut(before[i])) and np.array_equal(cut(a), cut(after[i])), level
    assert not np.array_equal(cut(a), cut(b)), level


def test_keep_inputs_false_drops_the_input_bytes_and_computes_the_same(sgd, tmp_path):
  """The default plan (inputs recorded) against the module's keep_inputs=False plan of the same network state."""
  config = sgd['config']
  net = train_lib.EfficientDetNetTrain(config=config, dtype='bf16', params=perturbed_params(config, 11), seed=5)
  path = str(tmp_path / 'with_inputs.plan')
  plan.record_network(net, sgd['images'], sgd['labels'], path, learning_rate=LR, ema_decay=DECAY)
  input_bytes = sum(np.ascontiguousarray(a).nbytes for a in sgd['inputs'].values())
  assert os.path.getsize(path) - os.path.getsize(sgd['path']) >= input_bytes
  s_def, s_lean = plan.read_summary(path), plan.read_summary(sgd['path'])
  assert set(s_def['names']) == set(s_lean['names'])
  full = net_c.CNet(path)
  lean = net_c.CNet(sgd['path'])
  try:
    assert not lean.read('images').any(), 'no recorded inputs in the keep_inputs=False plan'
    assert full.read('images').any()
    for k, a in sgd['inputs'].items():
      lean.write(k, a)
    full.forward()
    lean.forward()
    for kind in ('cls', 'box'):
      for li, (g, w) in enumerate(zip(_logits(lean, config, kind), _logits(full, config, kind))):
        assert np.array_equal(g, w), (kind, li)
    for k in STATE_KEYS:      # and the same recorded step from the same state
      assert np.array_equal(lean.read(k), full.read(k)), k
    full.train_step(LR, DECAY)
    lean.train_step(LR, DECAY)
    for k in STATE_KEYS:
      assert np.array_equal(lean.read(k), full.read(k)), k
  finally:
    full.close()
    lean.close()
