"""Lion on the device: edet_opt_lion_ema against tests/lion_ref.py bit for bit, the update wired into both trainers (one
step ahead of the restatement, eager and replayed, state round trip), a sanity learning run, and a Lion plan replayed by the
C host."""
import os

import numpy as np
import pytest
import torch

from automl_amd import _lib, effnetv2_configs, effnetv2_model, effnetv2_train, hparams_config, net_c, plan, train_lib
from automl_amd._lib import call, ptr
from tests import gpu_util as gu
from tests import lion_ref
from tests import test_effnetv2_train as v2t
from tests import test_plan_vars_gpu as pv
from tests.test_gpu_network import make_labels, perturbed_params

pytestmark = pytest.mark.gpu
F = np.float32


def same(got, want):
  """array_equal with NaN equal to NaN (a diverged element must be NaN on both sides)."""
  got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
  return np.array_equal(got, np.asarray(want), equal_nan=True)


# ---- the kernel --------------------------------------------------------------------------------------------------------
SIZES = [1, 3, 1023, 1024, 1025, 4099, 64]      # 4099: the segments behind it start off a 16-byte boundary (scalar walk)
FLAGS = [1, 0, 1, 0, 1, 0, _lib.SEG_FROZEN]


def _kernel_problem():
  rng = np.random.default_rng(23)
  offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
  tot = int(offs[-1])
  w = rng.standard_normal(tot).astype(F)
  m = (rng.standard_normal(tot) * 0.05).astype(F)
  ema = rng.standard_normal(tot).astype(F)
  g = rng.standard_normal(tot).astype(F)
  a = int(offs[5])      # inside the 4099 segment (vector path): the special values
  m[a:a + 8] = 0.0
  g[a:a + 8] = 0.0                        # c == 0 with m == 0: the variable moves by the decay alone
  g[a + 2], m[a + 3] = -0.0, -0.0           # negative zeros: sign(-0) = 0
  w[a + 4], w[a + 5] = 0.0, -0.0            # and zero variables under them
  g[a + 9] = np.nan                       # one diverged element
  b = int(offs[2]) + 1021                 # the scalar tail of the 1023 segment
  m[b], g[b] = 0.0, 0.0
  g[int(offs[6]) - 1] = np.nan            # and one in the scalar walk of the last live segment
  fac = rng.uniform(0.2, 1.0, len(SIZES)).astype(F)
  return offs, w, m, ema, g, fac


@pytest.mark.parametrize('wd', [0.0, 0.1])
@pytest.mark.parametrize('use_factor', [True, False], ids=['factor', 'no_factor'])
@pytest.mark.parametrize('use_ema', [True, False], ids=['ema', 'no_ema'])
def test_kernel_equals_the_restatement(use_ema, use_factor, wd):
  offs, w, m, ema, g, fac = _kernel_problem()
  assert int(offs[6]) % 4 != 0 and int(offs[3]) % 4 != 0      # unaligned starts are in the layout
  b1, b2 = 0.9, 0.99
  hyper = np.array([0.01, 0.95], F)
  wdev, md, ed, gd = (torch.from_numpy(t.copy()).to(gu.DEV) for t in (w, m, ema, g))
  od = torch.from_numpy(offs).to(gu.DEV)
  fd = torch.tensor(FLAGS, dtype=torch.int32, device=gu.DEV)
  facd = torch.from_numpy(fac).to(gu.DEV)
  hd = torch.from_numpy(hyper).to(gu.DEV)
  for step in (1, 2):
    call('edet_opt_lion_ema', ptr(wdev), ptr(gd), ptr(md), ptr(ed) if use_ema else None, ptr(od),
         ptr(facd) if use_factor else None, ptr(fd), len(SIZES), ptr(hd), b1, b2, wd, gu.stream())
    torch.cuda.synchronize()
    w2, m2, ema2 = lion_ref.lion_arena(w, m, g, offs, FLAGS, hyper, b1, b2, wd, fac if use_factor else None,
                                       ema if use_ema else None, frozen_flag=_lib.SEG_FROZEN)
    for what, got, want in (('w', wdev, w2), ('m', md, m2), ('ema', ed, ema2 if use_ema else ema)):
      g_np = got.cpu().numpy()
      bad = ~((g_np == want) | (np.isnan(g_np) & np.isnan(want)))
      assert same(got, want), 'step %d, %s: %d of %d elements differ, first at %s' % (step, what, int(bad.sum()), bad.size,
                                                                                     np.flatnonzero(bad)[:5])
    w, m = w2, m2
    ema = ema2 if use_ema else ema
  a = int(offs[5])
  assert np.isnan(w[a + 9]) and np.isnan(m[a + 9]) and np.isfinite(w[a + 8]) and np.isfinite(w[a + 10])      # the NaN stays put
  assert int(np.isnan(w).sum()) == 2
  # the frozen segment: nothing of it was touched (gradient included)
  fr = slice(int(offs[6]), int(offs[7]))
  start = _kernel_problem()
  for got, was in ((wdev, start[1]), (md, start[2]), (ed, start[3]), (gd, start[4])):
    assert same(got[fr], was[fr])
  # zero gradient and zero momentum: the variable moved by the decay alone, the momentum stayed zero
  lr = hyper[0]
  w0 = start[1][a:a + 2]
  once = (w0 - lr * (F(0) + w0 * F(wd))).astype(F)
  assert np.array_equal(w[a:a + 2], (once - lr * (F(0) + once * F(wd))).astype(F)) and not m[a:a + 2].any()


def test_kernel_refuses_bad_arguments():
  t = torch.zeros(8, device=gu.DEV)
  offs = torch.tensor([0, 8], dtype=torch.int64, device=gu.DEV)
  with pytest.raises(_lib.EdetError, match='edet_opt_lion_ema'):
    call('edet_opt_lion_ema', ptr(t), ptr(t), None, None, ptr(offs), None, None, 1, ptr(t), 0.9, 0.99, 0.0, gu.stream())


# ---- the detector --------------------------------------------------------------------------------------------------------
DET_SIZE, DET_BATCH, DET_STEPS = 128, 2, 3
DET_LION = dict(beta_2=0.98, wd=0.05)


def _det_config():
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  config.override('optimizer=lion')
  return config


def _det_data(config):
  rng = np.random.default_rng(7)
  return [(rng.standard_normal((DET_BATCH, DET_SIZE, DET_SIZE, 3)).astype(F), make_labels(config, DET_BATCH, DET_SIZE, 50 + i))
          for i in range(DET_STEPS)]


def _det_net(config, use_graph):
  return train_lib.EfficientDetNetTrain(config=config, dtype='f32', params=perturbed_params(config, 11), seed=5,
                                        use_graph=use_graph, stochastic_depth=False, steps_per_epoch=10, lion=DET_LION)


def _arena_np(arena):
  return {k: getattr(arena, k).detach().cpu().numpy().copy() for k in ('params_flat', 'velocity', 'ema', 'state_flat')}


def _one_step_ahead(eng, before, use_ema):
  """lion_ref applied to what the step left behind (gradient with its L2 term, clip factors, the step's scalars) on the
  state from before the step -> the state the step must have left."""
  torch.cuda.synchronize()
  u = eng.update
  hyper = eng.hyper.cpu().numpy()[:2]
  return lion_ref.lion_arena(before['params_flat'], before['velocity'], eng.grads_flat.cpu().numpy(),
                             eng.seg_offsets.cpu().numpy(), eng.seg_flags.cpu().numpy(), hyper, u.momentum, u.beta2, u.wd,
                             eng.seg_factor.cpu().numpy(), before['ema'] if use_ema else None, frozen_flag=_lib.SEG_FROZEN)


@pytest.fixture(scope='module')
def det_eager():
  """Three eager steps, each one held to the restatement; -> (net, the state after every step, the optimizer state and
  weights after step two)."""
  config = _det_config()
  data = _det_data(config)
  net = _det_net(config, False)
  states, mid = [], None
  for i, d in enumerate(data):
    if net.engine is None:
      net._ensure_engine(DET_BATCH, DET_SIZE, DET_SIZE)
    before = _arena_np(net.engine.arena)
    out = net.train_step(d)
    assert np.isfinite(out['loss'])
    eng = net.engine
    assert eng.update == ('lion', 0.9, 0.98, None, None, 0.05) and eng.arena.adam_v is None      # one slot, no second arena
    w, m, ema = _one_step_ahead(eng, before, True)
    after = _arena_np(eng.arena)
    for what, got, want in (('variables', after['params_flat'], w), ('slot', after['velocity'], m), ('shadows', after['ema'], ema)):
      assert np.array_equal(got, want), 'step %d, %s: %d elements differ' % (i, what, int((got != want).sum()))
    assert float(np.abs(after['params_flat'] - before['params_flat']).max()) > 0 and np.abs(after['velocity']).max() > 0
    states.append(after)
    if i == 1:
      mid = (net.get_optimizer_state(), net.get_weights())
  return net, states, mid, data, config


def test_detector_steps_equal_the_restatement(det_eager):
  net, states, _, _, _ = det_eager
  assert net.engine.arena.step_count == DET_STEPS and len(states) == DET_STEPS
  # wd reaches the BatchNorm scales too: they are segments of the arena like any other, and none is frozen here
  name = next(n for n in net.engine.arena.offsets if n.endswith('/gamma'))
  assert net.engine.arena.offsets[name][3] and not int((net.engine.seg_flags & _lib.SEG_FROZEN).sum())


def test_detector_graph_replay_equals_eager(det_eager):
  _, states, _, data, config = det_eager
  net = _det_net(config, True)
  for d in data:
    net.train_step(d)
  torch.cuda.synchronize()
  assert net._graph['graphs'] is not None and net.engine.arena.step_count == DET_STEPS
  got = _arena_np(net.engine.arena)
  for k, want in states[-1].items():
    assert np.array_equal(got[k], want), '%s: %d elements differ' % (k, int((got[k] != want).sum()))


def test_detector_state_round_trip(det_eager):
  _, states, (state, weights), data, config = det_eager
  assert state['iterations'] == 2 and 'adam_v' not in state and 'rms' not in state
  other = _det_net(config, False)
  other._ensure_engine(DET_BATCH, DET_SIZE, DET_SIZE)
  other.set_weights(weights)
  other.set_optimizer_state(state)
  other.train_step(data[2])
  torch.cuda.synchronize()
  got = _arena_np(other.engine.arena)
  for k, want in states[-1].items():
    assert np.array_equal(got[k], want), '%s: %d elements differ' % (k, int((got[k] != want).sum()))
  assert other.iterations == 3 and other.engine.arena.step_count == 3
  with pytest.raises(ValueError, match='after the first engine was made'):
    other.set_lion(wd=0.0)


# ---- the classifier ------------------------------------------------------------------------------------------------------
V2 = dict(model_name='efficientnetv2-b0', over='num_classes=24', size=64, batch=4, steps=3)


def _v2_net(use_graph):
  spec = effnetv2_model.V2Spec(effnetv2_configs.model_config(V2['model_name'], V2['over']))
  sched = effnetv2_train.WarmupLearningRateSchedule(0.001, steps_per_epoch=2, lr_decay_type='cosine', total_steps=10,
                                                    warmup_epochs=1)
  return effnetv2_train.TrainableModel(V2['model_name'], V2['over'], dtype='f32', params=v2t._perturbed(spec, 3),
                                       use_graph=use_graph, learning_rate=sched, weight_decay=1e-5, label_smoothing=0.1,
                                       optimizer='lion', momentum=0.95, lion_beta2=0.98, lion_wd=0.02, ema_decay=0.99, seed=4)


def _v2_data():
  rng = np.random.default_rng(29)
  return [(rng.standard_normal((V2['batch'], V2['size'], V2['size'], 3)).astype(F), rng.integers(0, 24, V2['batch']))
          for _ in range(V2['steps'])]


def test_classifier_steps_equal_the_restatement_and_the_replay():
  data = _v2_data()
  net = _v2_net(False)
  for i, d in enumerate(data):
    if net.engine is None:
      net._ensure_engine(V2['batch'], V2['size'], V2['size'])
    before = _arena_np(net.engine.arena)
    out = net.train_step(d)
    eng = net.engine
    assert eng.update == ('lion', 0.95, 0.98, None, None, 0.02) and eng.arena.adam_v is None
    w, m, ema = _one_step_ahead(eng, before, True)
    after = _arena_np(eng.arena)
    for what, got, want in (('variables', after['params_flat'], w), ('slot', after['velocity'], m), ('shadows', after['ema'], ema)):
      assert np.array_equal(got, want), 'step %d, %s: %d elements differ' % (i, what, int((got != want).sum()))
    assert float(np.float32(out['learning_rate'])) == float(eng.hyper[0]) and float(eng.hyper[1]) == float(np.float32(0.99))
  state = net.get_optimizer_state()
  assert state['iterations'] == 3 and 'rms' not in state and 'adam_v' not in state
  replayed = _v2_net(True)
  for d in data:
    replayed.train_step(d)
  torch.cuda.synchronize()
  assert replayed._graph['graph'] is not None
  got = _arena_np(replayed.engine.arena)
  for k, want in after.items():
    assert np.array_equal(got[k], want), '%s: %d elements differ' % (k, int((got[k] != want).sum()))


def test_it_learns_with_lion():
  """test_effnetv2_train.test_it_learns' problem (its LEARN set-up, imported) with optimizer='lion' at a tenth of its RMSprop
  rate: the training-mode loss after the same number of steps is below the first one's.  A sanity floor, not a tuned number."""
  learn = v2t.LEARN
  vals, images, labels = v2t._learn_problem()
  net = effnetv2_train.TrainableModel(learn['model_name'], learn['over'], dtype='f32', params=vals, learning_rate=learn['lr'] / 10,
                                      label_smoothing=learn['smoothing'], weight_decay=0.0, optimizer='lion')
  losses = [net.train_step((images, labels))['loss'] for _ in range(learn['steps'])]
  print('training-mode loss with Lion: step 1 %.4f, step 11 %.4f, step %d %.4f' % (losses[0], losses[10], len(losses), losses[-1]))
  assert np.isfinite(losses).all()
  assert losses[-1] < losses[0], (losses[0], losses[-1])


# ---- the plan ------------------------------------------------------------------------------------------------------------
def test_lion_plan_replayed_by_the_c_host(tmp_path_factory):
  """A Lion D0 plan recorded at the C host's rate and decay: its two replayed steps (edet_train_step, from a fresh process)
  equal the Python host's -- the recorded step and one more -- bit for bit, the saved state has the one slot, and the
  second-moment slot is refused as it is for SGD."""
  d = tmp_path_factory.mktemp('plan_lion')
  config = _det_config()
  net = train_lib.EfficientDetNetTrain(config=config, dtype='bf16', params=perturbed_params(config, 11), seed=5, lion=DET_LION)
  rng = np.random.default_rng(97)
  images = torch.from_numpy(rng.standard_normal((2, DET_SIZE, DET_SIZE, 3)).astype(F))
  labels = make_labels(config, 2, DET_SIZE, 101)
  path = str(d / 'd0_128_b2_lion.plan')
  _, expected = plan.record_network(net, images, labels, path, learning_rate=pv.HOST_LR, ema_decay=pv.HOST_DECAY, keep_inputs=False)
  eng = net._ensure_engine(2, DET_SIZE, DET_SIZE)
  dimages, dl = net._to_device_images(images, eng), net._labels_to_device(labels, eng)
  inputs = {'images': dimages.view(torch.uint8).cpu().numpy().reshape(-1)}
  inputs.update({k: t.cpu().numpy() for k, t in dl.items() if torch.is_tensor(t)})
  rec = {'path': path, 'inputs': inputs}
  names = plan.read_summary(path)['names']
  assert names['optimizer'][1] == 2 and 'adam_v' not in names
  for key, want in (('lion_beta1_bits', 0.9), ('lion_beta2_bits', 0.98), ('lion_wd_bits', 0.05)):
    assert plan.bits_double(names[key][1]) == want
  t0 = names['iterations'][1]
  # the Python host: the recorded step was the first, one more makes two
  plan.train_pass(eng, dimages, dl, pv.HOST_LR, pv.HOST_DECAY)
  torch.cuda.synchronize()
  want = {'params': eng.params_flat, 'ema': eng.ema, 'velocity': eng.velocity, 'bn_state': eng.state_flat, 'loss_sums': eng.loss_sums}
  exe = pv._build_host(str(d))
  out, state = os.path.join(str(d), 'out'), os.path.join(str(d), 'two.state')
  pv._host(exe, ['train', path, out, 2, '-', state], rec, out)
  got = pv._dumps(out, pv.STATE_KEYS)
  assert got['iterations'] == t0 + 2 == eng.arena.step_count
  for k in pv.STATE_KEYS:
    w = pv._u32(want[k].detach().cpu().numpy())
    assert np.array_equal(got[k], w), 'C host, %s: %d of %d elements differ' % (k, int((got[k] != w).sum()), w.size)
  saved = plan.read_state(state)
  assert saved['iterations'] == t0 + 2 and not saved['adam_v'] and set(saved['momentum']) == set(saved['ema'])
  name = next(iter(eng.arena.offsets))
  off, n = eng.arena.offsets[name][:2]
  assert np.array_equal(pv._u32(saved['momentum'][name]), pv._u32(eng.velocity[off:off + n].cpu().numpy()))
  cnet = pv._open(rec)
  try:
    assert cnet.prop('optimizer') == 2 and 'adam_v' not in cnet.names()
    cnet.train_step(pv.HOST_LR, pv.HOST_DECAY, torch.cuda.current_stream().cuda_stream)      # = the recorded step
    torch.cuda.synchronize()
    for k in ('params', 'velocity', 'ema'):
      assert np.array_equal(cnet.read(k).view(np.uint32), pv._u32(expected[k])), k
    with pytest.raises(_lib.EdetError, match='not Adam'):
      cnet.get_variable(name, net_c.SLOT_ADAM_V)
  finally:
    cnet.close()
