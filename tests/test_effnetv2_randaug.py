"""RandAugment in the EfficientNetV2 classifier trainer (effnetv2_train.TrainableModel(augname='randaug') on
V2Engine.randaug_batch): the uint8 train step against the float step, the fp32 oracle fed the restatement's augmented batch,
graph replay against eager, the magnitude between steps and the state round trip.  The tiny configuration of
tests/test_effnetv2_train.py (efficientnetv2-b0, 24 classes), batch 8, images 32 x 32."""
import numpy as np
import pytest
import torch

from automl_amd import autoaugment as aa, effnetv2_configs, effnetv2_model, effnetv2_train
from tests import gpu_util as gu
from tests import randaug_ref as rr
from tests.test_effnetv2_train import EPSILON, _perturbed, oracle_train_step, rmsprop_step, topk_rows

MODEL, OVER, SIZE, NC, BATCH = 'efficientnetv2-b0', 'num_classes=24', 32, 24, 8


def _data(seed, steps):
  rng = np.random.default_rng(seed)
  return [(rng.integers(0, 256, (BATCH, SIZE, SIZE, 3)).astype(np.uint8), rng.integers(0, NC, BATCH)) for _ in range(steps)]


def _net(**kw):
  args = dict(learning_rate=0.01, weight_decay=1e-5, label_smoothing=0.1, seed=4, augname='randaug', ra_num_layers=2,
              ra_magnitude=15)
  args.update(kw)
  return effnetv2_train.TrainableModel(MODEL, OVER, **args)


def _same_state(a, b, keys=('params_flat', 'velocity', 'adam_v', 'state_flat')):
  for key in keys:
    assert torch.equal(getattr(a.engine.arena, key), getattr(b.engine.arena, key)), key


def _draws_of(net):
  e = net.engine
  return tuple(t.cpu().clone() for t in (e.ra_ops, e.ra_iargs, e.ra_fargs))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_identity_draws_equal_the_float_step(dtype):
  """Draws forced to the identity: the uint8 step is, bit for bit in loss and updated variables, the existing float step on
  (x - 128) / 128 -- the normalisation is exact in fp32 and bf16 and the launches behind it are the same."""
  (images, labels), = _data(3, 1)
  aug = _net(use_graph=False, dtype=dtype)
  aug.force_randaug_draws(aa.identity_draws(BATCH, 2))
  plain = _net(use_graph=False, dtype=dtype, augname=None)
  got = aug.train_step((images, labels))
  want = plain.train_step((rr.normalise(images), labels))
  torch.cuda.synchronize()
  assert got == want, (got, want)
  _same_state(aug, plain)
  assert int((aug.engine.ra_ops != 16).sum()) == 0
  # test_step never augments: uint8 in, normalised only
  aug.force_randaug_draws(None)
  assert aug.test_step((images, labels)) == plain.test_step((rr.normalise(images), labels))
  assert aug.test_step((rr.normalise(images), labels)) == plain.test_step((rr.normalise(images), labels))
  with pytest.raises(ValueError, match='uint8'):
    aug.train_step((rr.normalise(images), labels))


@pytest.mark.gpu
def test_randaug_step_matches_oracle_fp32():
  """One eager RMSprop step with RandAugment, fp32 storage, against test_effnetv2_train's oracle step fed the restatement's
  augmented and normalised batch, with that test's own tolerances: the same network arithmetic, only the input differs."""
  lr, wd, smoothing = 0.01, 1e-4, 0.1
  spec = effnetv2_model.V2Spec(effnetv2_configs.model_config(MODEL, OVER))
  vals = _perturbed(spec, 9)
  (images, labels), = _data(13, 1)
  net = _net(dtype='f32', params=vals, use_graph=False, learning_rate=lr, weight_decay=wd, label_smoothing=smoothing, seed=1)
  draws = aa.randaug_draws(aa.randaug_rng(1), BATCH, 2)      # what the model's own generator hands its first step
  out = net.train_step((images, labels))
  torch.cuda.synchronize()
  eng = net.engine
  ops, iargs, fargs = aa.randaug_args(draws, 15, SIZE, SIZE)
  assert np.array_equal(eng.ra_ops.cpu().numpy(), ops) and np.array_equal(eng.ra_iargs.cpu().numpy(), iargs)
  assert np.array_equal(eng.ra_fargs.cpu().numpy(), fargs)
  augmented = rr.randaugment(images, draws, 15)
  assert not np.array_equal(augmented, images)
  fed = rr.normalise(augmented)
  assert np.array_equal(eng.buf('randaug:images', (BATCH, SIZE, SIZE, 3), torch.float32).cpu().numpy(), fed)
  drop_scale = {k[:-len(':out')]: m[:, 0].detach().cpu().clone() for k, (m, p) in eng.drop_masks.items()}
  loss, l2, grads, moving, logits = oracle_train_step(MODEL, OVER, vals, fed, labels, smoothing, wd, drop_scale,
                                                      eng.dropout_mask.cpu().clone())
  print('randaug step: loss %.6f (oracle %.6f), L2 %.6f (%.6f)' % (out['loss'] - out['reg_l2_loss'], loss, out['reg_l2_loss'], l2))
  assert abs(out['loss'] - out['reg_l2_loss'] - loss) <= 1e-3 * abs(loss), (out, loss)
  assert abs(out['reg_l2_loss'] - l2) <= 1e-3 * l2, (out, l2)
  assert out['acc_top1'] == topk_rows(logits, torch.as_tensor(labels), 1) / BATCH
  assert out['acc_top5'] == topk_rows(logits, torch.as_tensor(labels), 5) / BATCH
  got_g = eng.get_grads()
  new = net.get_weights()
  gmax = max(float(np.abs(g).max()) for g in grads.values())
  bad_g, bad_w = [], []
  for name, g in grads.items():
    bound = 1e-2 * max(float(np.abs(g).max()), 1e-4 * gmax)
    e = float(np.abs(np.asarray(got_g[name]).reshape(g.shape) - g).max())
    if not e <= bound:
      bad_g.append((name, e / bound))
    w, ms, mom = vals[name].copy(), np.zeros_like(g), np.zeros_like(g)
    rmsprop_step(w, g, ms, mom, lr)
    e = float(np.abs(new[name].reshape(w.shape) - w).max())
    if not e <= lr / np.sqrt(EPSILON) * bound:
      bad_w.append((name, e / (lr / np.sqrt(EPSILON) * bound)))
  assert not bad_g, 'gradient mismatch in %d/%d tensors, worst %s' % (len(bad_g), len(grads), sorted(bad_g, key=lambda t: -t[1])[:8])
  assert not bad_w, 'update mismatch in %d/%d tensors, worst %s' % (len(bad_w), len(grads), sorted(bad_w, key=lambda t: -t[1])[:8])
  worst = max(float(np.abs(new[k] - v).max()) / max(float(np.abs(v).max()), 1e-6) for k, v in moving.items())
  assert worst <= 1e-3, 'moving statistics differ: %g' % worst


@pytest.mark.gpu
@pytest.mark.parametrize('mix', [0.0, 0.4], ids=['plain', 'mixup_cutmix'])
def test_graph_replay_equals_eager(mix):
  """bf16 storage, three steps: one eager and two replays of the captured step (the RandAugment launches are its first,
  reading the static argument buffers; with mixup + cutmix on, the mix kernels follow them) leave exactly the state and the
  losses of three eager steps; the draws differ from step to step."""
  data = _data(29, 3)
  runs = []
  for use_graph in (True, False):
    net = _net(use_graph=use_graph, mixup_alpha=mix, cutmix_alpha=mix)
    outs, draws = [], []
    for d in data:
      outs.append(net.train_step(d))
      draws.append(_draws_of(net))
    torch.cuda.synchronize()
    runs.append((net, outs, draws))
  (g, og, dg), (e, oe, de) = runs
  assert g._graph['graph'] is not None and g._graph['steps'] == 3 and e._graph is None
  assert og == oe, (og, oe)
  _same_state(g, e)
  for a, b in zip(dg, de):
    assert all(torch.equal(x, y) for x, y in zip(a, b))
  assert all(not torch.equal(dg[i][0], dg[i + 1][0]) for i in range(2)), 'the operations did not change between steps'
  images, _ = g.input_buffers()
  assert images.dtype == torch.uint8 and torch.equal(images.cpu(), torch.from_numpy(data[-1][0]))
  key = ('randaug:images', (BATCH, SIZE, SIZE, 3), torch.bfloat16)
  assert torch.equal(g.engine.buf(*key), e.engine.buf(*key))
  if mix:
    assert torch.equal(g.engine.soft_labels, e.engine.soft_labels) and g.engine.n_mixup == BATCH // 2


@pytest.mark.gpu
def test_set_randaug_keeps_the_graph_and_changes_the_result():
  data = _data(31, 3)
  a, b = _net(use_graph=True), _net(use_graph=True)
  for net in (a, b):
    net.train_step(data[0])
    net.train_step(data[1])
  _same_state(a, b)
  graph = a._graph['graph']
  assert graph is not None
  a.set_randaug(5)
  oa, ob = a.train_step(data[2]), b.train_step(data[2])
  torch.cuda.synchronize()
  assert a._graph['graph'] is graph and a._graph['steps'] == 3, 'set_randaug dropped the captured step'
  assert torch.equal(a.engine.ra_ops, b.engine.ra_ops), 'the same operations at another magnitude'
  assert not torch.equal(a.engine.ra_fargs, b.engine.ra_fargs) or not torch.equal(a.engine.ra_iargs, b.engine.ra_iargs)
  assert oa['loss'] != ob['loss']
  # the replayed step at magnitude 5 is the eager step at magnitude 5
  c = _net(use_graph=False)
  c.train_step(data[0])
  c.train_step(data[1])
  c.set_randaug(5)
  assert c.train_step(data[2]) == oa
  _same_state(a, c)


@pytest.mark.gpu
def test_state_round_trip_and_no_new_key_without_augname():
  """State and weights after step 2 -> a fresh model: its steps 3 and 4 are the uninterrupted ones bit for bit, the
  RandAugment draws included.  Without augname the state has no new key, and a uint8 batch is what it always was: the
  byte values cast to the network's type."""
  data = _data(37, 4)
  net = _net(use_graph=False)
  net.train_step(data[0])
  net.train_step(data[1])
  state, weights = net.get_optimizer_state(), net.get_weights()
  assert 'randaug_rng_state' in state and 'mix_rng_state' in state and 'rng_state' in state
  other = _net(use_graph=False)
  other.set_weights(weights)
  other.set_optimizer_state(state)
  for d in data[2:]:
    want = net.train_step(d)
    got = other.train_step(d)
    assert got == want
    assert all(torch.equal(x, y) for x, y in zip(_draws_of(net), _draws_of(other)))
  torch.cuda.synchronize()
  _same_state(net, other)
  plain = [_net(use_graph=False, augname=None) for _ in range(2)]
  images, labels = data[0]
  got = plain[0].train_step((images, labels))
  want = plain[1].train_step((images.astype(np.float32), labels))
  torch.cuda.synchronize()
  assert got == want
  _same_state(plain[0], plain[1])
  state = plain[0].get_optimizer_state()
  assert 'randaug_rng_state' not in state and 'mix_rng_state' in state
  assert plain[0].engine.ra_ops is None and 'randaug:images' not in plain[0].engine._bufs
