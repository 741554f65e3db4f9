"""EfficientNetV2 classifier training (automl_amd/effnetv2_train.py on edet_softmax_xent, edet_dropout_cast and
edet_opt_rmsprop_ema): the learning-rate schedule and the loss restatement on the CPU, the three kernels and the whole
train step against fp32 restatements on the GPU.

The restatements live here: `xent` (tf.keras.losses.CategoricalCrossentropy(label_smoothing, from_logits=True), mean over
the batch -- pinned against torch.nn.functional.cross_entropy below), `rmsprop_step` (TensorFlow's ApplyRMSProp with
momentum, as documented; TensorFlow is not installed where this suite runs) and `oracle_train_step` (oracle.effnetv2_oracle
forward with the device's stochastic-depth draws and dropout mask -> xent -> autograd -> L2 -> rmsprop_step)."""
import numpy as np
import pytest
import torch

from automl_amd import _lib, effnetv2_configs, effnetv2_model, effnetv2_train, netspec
from automl_amd._lib import call, ptr
from oracle import effnetv2_oracle as v2orc
from tests import gpu_util as gu

RHO, MOMENTUM, EPSILON = 0.9, 0.9, 0.001      # build_tf2_optimizer, efficientnetv2/main_tf2.py:36-52


# ------------------------------------------------------------------------------------ restatements
def xent(logits, labels, smoothing):
  """-> (mean loss, per-row loss): y = (1 - s) onehot + s / C, loss_row = logsumexp(x) - sum_c y_c x_c."""
  c = logits.shape[1]
  y = torch.nn.functional.one_hot(labels.long(), c).to(logits.dtype) * (1.0 - smoothing) + smoothing / c
  rows = torch.logsumexp(logits, dim=1) - (y * logits).sum(1)
  return rows.mean(), rows


def topk_rows(logits, labels, k):
  """Rows whose label is in the top k: fewer than k logits strictly greater than the label's."""
  xl = logits.gather(1, labels.long().view(-1, 1))
  return int(((logits > xl).sum(1) < k).sum())


def rmsprop_step(w, g, ms, mom, lr, rho=RHO, momentum=MOMENTUM, eps=EPSILON):
  """numpy float32, in place: ms += (1 - rho)(g^2 - ms); mom = momentum mom + lr g / sqrt(ms + eps); w -= mom."""
  f = np.float32
  ms += (g * g - ms) * (f(1) - f(rho))
  mom[...] = f(momentum) * mom + (f(lr) * g) / np.sqrt(ms + f(eps))
  w -= mom


# ------------------------------------------------------------------------------------ CPU
def test_schedule_known_answers():
  """WarmupLearningRateSchedule (efficientnetv2/utils.py:101-131), by hand: initial 0.8, 10 steps per epoch, 2 warm-up
  epochs (20 steps: lr = 0.8 step / 20 below step 20, the decayed value from step 20 on)."""
  S = effnetv2_train.WarmupLearningRateSchedule
  kw = dict(steps_per_epoch=10, warmup_epochs=2)
  # exponential, staircase: decay_steps = 10 * 2.4 = 24, 0.8 * 0.5 ^ floor(step / 24)
  e = S(0.8, lr_decay_type='exponential', decay_factor=0.5, decay_epochs=2.4, **kw)
  assert e(0) == 0.0
  assert e(19) == pytest.approx(0.8 * 19 / 20) and e(20) == pytest.approx(0.8)
  assert e(23) == pytest.approx(0.8) and e(24) == pytest.approx(0.4)          # the staircase boundary
  assert e(47) == pytest.approx(0.4) and e(48) == pytest.approx(0.2)
  # cosine over 100 steps: 0.4 (1 + cos(pi step / 100))
  c = S(0.8, lr_decay_type='cosine', total_steps=100, **kw)
  assert c(19) == pytest.approx(0.76) and c(20) == pytest.approx(0.4 * (1 + np.cos(np.pi * 0.2)))
  assert c(50) == pytest.approx(0.4) and c(100) == pytest.approx(0.0, abs=1e-12)
  # linear over 100 steps: 0.8 (1 - step / 100)
  l = S(0.8, lr_decay_type='linear', total_steps=100, **kw)
  assert l(19) == pytest.approx(0.76) and l(20) == pytest.approx(0.64) and l(75) == pytest.approx(0.2)
  # constant
  k = S(0.8, lr_decay_type='constant', **kw)
  assert k(19) == pytest.approx(0.76) and k(20) == 0.8 and k(10 ** 6) == 0.8
  # the floor applies to the decayed value, not to the warm-up ramp (utils.py:121-129: maximum first, then the cond)
  for sched, step in ((S(0.8, lr_decay_type='exponential', decay_factor=0.5, decay_epochs=2.4, minimal_lr=0.3, **kw), 48),
                      (S(0.8, lr_decay_type='cosine', total_steps=100, minimal_lr=0.3, **kw), 90),
                      (S(0.8, lr_decay_type='linear', total_steps=100, minimal_lr=0.3, **kw), 90),
                      (S(0.2, lr_decay_type='constant', minimal_lr=0.3, **kw), 30)):
    assert sched(step) == 0.3
    assert sched(5) == pytest.approx(sched.initial_lr * 5 / 20)
  # no warm-up
  assert S(0.8, lr_decay_type='linear', total_steps=100, steps_per_epoch=10, warmup_epochs=0)(0) == 0.8
  with pytest.raises(ValueError):
    S(0.8, lr_decay_type='polynomial')


@pytest.mark.parametrize('smoothing', [0.0, 0.1, 0.3])
def test_loss_restatement_equals_torch_cross_entropy(smoothing):
  """xent() above is what the GPU tests compare with: the same definition as torch's cross_entropy(label_smoothing)."""
  rng = np.random.default_rng(3)
  for b, c in ((1, 5), (8, 24), (64, 1000), (7, 1001)):
    x = torch.from_numpy(rng.standard_normal((b, c)) * 4).double().requires_grad_(True)
    y = torch.from_numpy(rng.integers(0, c, b))
    mine, _ = xent(x, y, smoothing)
    g_mine, = torch.autograd.grad(mine, x)
    want = torch.nn.functional.cross_entropy(x, y, label_smoothing=smoothing)
    g_want, = torch.autograd.grad(want, x)
    assert abs(float(mine.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    assert float((g_mine - g_want).abs().max()) <= 1e-14


def test_trainer_options():
  """No GPU needed: the constructor's checks and the host side of the state."""
  t = effnetv2_train.TrainableModel('efficientnetv2-b0', 'num_classes=24')
  assert t.optimizer == 'rmsprop' and t.momentum == 0.9 and t.cfg_model.dropout_rate > 0
  assert effnetv2_train.TrainableModel('efficientnetv2-b0', optimizer='sgd').momentum == 0.0
  with pytest.raises(ValueError):
    effnetv2_train.TrainableModel('efficientnetv2-b0', optimizer='lamb')
  with pytest.raises(ValueError):
    effnetv2_train.TrainableModel('efficientnetv2-b0', 'conv_dropout=0.1')
  for name in ('edet_softmax_xent', 'edet_dropout_cast', 'edet_opt_rmsprop_ema'):
    assert name in _lib.SIGNATURES


# ------------------------------------------------------------------------------------ GPU: kernels
def _xent_problem(name, tdt, b, nc, seed):
  rng = np.random.default_rng(seed)
  x = rng.standard_normal((b, nc)) * 2
  for r in range(0, b, 3):      # some rows with max x ~ 80: without the max subtraction exp() overflows
    i = int(np.abs(x[r]).argmax())
    x[r] *= 80.0 / x[r, i]
  logits = torch.from_numpy(x.astype(np.float32)).to(tdt).float()
  labels = torch.from_numpy(rng.integers(0, nc, b).astype(np.int32))
  # a row with tied logits: the label's logit also sits in two other columns, and is the row maximum
  r = b - 1
  l = int(labels[r])
  top = float(logits[r].max()) + 1.0
  top = float(torch.tensor(top).to(tdt).float())
  logits[r, l] = top
  logits[r, (l + 1) % nc] = top
  logits[r, (l + 2) % nc] = top
  return logits, labels


@pytest.mark.gpu
@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('nc', [5, 24, 1000, 1001])
@pytest.mark.parametrize('b', [1, 8, 256])
@pytest.mark.parametrize('smoothing', [0.0, 0.1], ids=['hard', 'ls0.1'])
def test_softmax_xent(dt, nc, b, smoothing):
  name, edt, tdt = dt
  logits, labels = _xent_problem(name, tdt, b, nc, gu.seed_of(nc, b, smoothing))
  assert float(logits.max()) > 75
  xq = logits.double().requires_grad_(True)
  want, _ = xent(xq, labels, smoothing)
  gscale = 1.0 if nc != 24 else 0.37      # grad_scale multiplies the gradient only: the loss sum stays unscaled
  (want * gscale).backward()
  ld = gu.to_dev(logits.view(b, 1, 1, nc), tdt)
  ld[..., nc:] = 7.0                       # padding columns may hold anything
  dl = torch.full_like(ld, float('nan'))
  sums = torch.zeros(4, dtype=torch.float32, device=gu.DEV)
  lab = labels.to(gu.DEV)
  wsp = torch.empty(4096, dtype=torch.float32, device=gu.DEV)

  def run(ws):
    sums.zero_()
    call('edet_softmax_xent', ptr(ld), ld.shape[-1], ptr(lab), b, nc, smoothing, gscale, ptr(dl), ptr(sums),
         ptr(ws), ws.numel() * 4 if ws is not None else 0, edt, gu.stream())
    torch.cuda.synchronize()
    return sums.cpu().clone(), dl.clone()
  s, d = run(wsp)
  s2, d2 = run(wsp)
  assert torch.equal(s, s2) and torch.equal(d.view(torch.uint8), d2.view(torch.uint8)), 'run-to-run difference'
  s3, d3 = run(None)                       # no workspace: one workgroup walks the rows
  loss = float(want.detach())
  print('softmax_xent %s nc=%d b=%d ls=%g: loss %.6f vs %.6f' % (name, nc, b, smoothing, float(s[0]), loss))
  for got in (s, s3):
    assert abs(float(got[0]) - loss) <= 1e-3 * abs(loss) + 1e-5, (float(got[0]), loss)
    assert int(got[1]) == topk_rows(logits, labels, 1) and int(got[2]) == topk_rows(logits, labels, 5), got
  # the tied row: two other logits equal the label's, none is strictly greater -> in the top 1
  assert topk_rows(logits[-1:], labels[-1:], 1) == 1
  for got in (d, d3):
    gu.check(got.view(b, -1)[:, :nc], xq.grad.float(), name, 'dlogits', rtol=1e-2 if name == 'bf16' else 1e-4)
    assert ld.shape[-1] == nc or float(got[..., nc:].abs().max()) == 0.0


@pytest.mark.gpu
def test_softmax_xent_refuses_bad_arguments():
  x = torch.zeros(2, 8, device=gu.DEV)
  lab = torch.zeros(2, dtype=torch.int32, device=gu.DEV)
  s = torch.zeros(4, device=gu.DEV)
  with pytest.raises(_lib.EdetError):
    call('edet_softmax_xent', ptr(x), 8, ptr(lab), 2, 9, 0.0, 1.0, ptr(x), ptr(s), None, 0, _lib.EDET_F32, gu.stream())
  with pytest.raises(_lib.EdetError):
    call('edet_softmax_xent', ptr(x), 8, ptr(lab), 2, 8, 1.5, 1.0, ptr(x), ptr(s), None, 0, _lib.EDET_F32, gu.stream())


@pytest.mark.gpu
@pytest.mark.parametrize('use_ema', [True, False], ids=['ema', 'no_ema'])
@pytest.mark.parametrize('use_factor', [True, False], ids=['factor', 'no_factor'])
def test_optimizer_rmsprop(use_ema, use_factor):
  """edet_opt_rmsprop_ema on the segment layout of test_gpu_kernels.test_optimizer (unaligned, multi-slice and frozen
  segments), non-zero starting slots, two steps."""
  rng = np.random.default_rng(17)
  sizes = [7, 64, 1, 1000, 33, 4096, 40003, 3, 65536]
  flags = [1, 0, 0, 1, _lib.SEG_FROZEN, 0, 1, _lib.SEG_FROZEN, 1]
  offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  tot = int(offs[-1])
  p = rng.standard_normal(tot).astype(np.float32)
  ms = (rng.standard_normal(tot) ** 2).astype(np.float32)
  mom = (rng.standard_normal(tot) * 0.1).astype(np.float32)
  ema = rng.standard_normal(tot).astype(np.float32)
  start = [t.copy() for t in (p, ms, mom, ema)]
  fac = rng.uniform(0.2, 1.0, len(sizes)).astype(np.float32)
  lr, decay = 0.05, np.float32(0.95)
  pd, sd, md, ed = (torch.from_numpy(t.copy()).to(gu.DEV) for t in (p, ms, mom, ema))
  od = torch.from_numpy(offs).to(gu.DEV)
  fd = torch.tensor(flags, dtype=torch.int32, device=gu.DEV)
  facd = torch.from_numpy(fac).to(gu.DEV)
  hyper = torch.tensor([lr, float(decay)], dtype=torch.float32, device=gu.DEV)
  for step in (1, 2):
    g = (rng.standard_normal(tot) * 3).astype(np.float32)
    gd = torch.from_numpy(g).to(gu.DEV)
    call('edet_opt_rmsprop_ema', ptr(pd), ptr(gd), ptr(sd), ptr(md), ptr(ed) if use_ema else None, ptr(od),
         ptr(facd) if use_factor else None, ptr(fd), len(sizes), ptr(hyper), RHO, MOMENTUM, EPSILON, gu.stream())
    torch.cuda.synchronize()
    for i in range(len(sizes)):
      sl = slice(int(offs[i]), int(offs[i + 1]))
      if flags[i] == _lib.SEG_FROZEN:
        continue
      gs = g[sl] * fac[i] if use_factor else g[sl]
      rmsprop_step(p[sl], gs, ms[sl], mom[sl], lr)
      if use_ema:
        ema[sl] = ema[sl] - (np.float32(1) - decay) * (ema[sl] - p[sl])
    for what, got, want in (('params', pd, p), ('ms', sd, ms), ('mom', md, mom), ('ema', ed, ema)):
      gu.check(got, torch.from_numpy(want), 'f32', 'rmsprop %s, step %d' % (what, step), rtol=1e-5, atol=1e-6)
  for i in (4, 7):      # frozen: value, both slots and the shadow bit for bit
    sl = slice(int(offs[i]), int(offs[i + 1]))
    for got, was in zip((pd, sd, md, ed), start):
      assert torch.equal(got[sl].cpu(), torch.from_numpy(was[sl]))
  if not use_ema:
    assert torch.equal(ed.cpu(), torch.from_numpy(start[3]))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
def test_dropout_cast(dt):
  name, edt, tdt = dt
  rng = np.random.default_rng(23)
  n, c, rate = 6, 1280, 0.2
  pooled = torch.from_numpy((rng.standard_normal((n, c)) * 30).astype(np.float32)).to(gu.DEV)
  mask = torch.from_numpy(((rng.random((n, c)) >= rate) / (1.0 - rate)).astype(np.float32)).to(gu.DEV)
  out = torch.empty(n, c, dtype=tdt, device=gu.DEV)
  call('edet_dropout_cast', ptr(pooled), ptr(mask), ptr(out), n * c, edt, gu.stream())
  torch.cuda.synchronize()
  assert torch.equal(out, (pooled * mask).to(tdt))
  assert 0 < int((out == 0).sum()) < n * c
  # rate 0 (a mask of ones) and no mask at all: edet_cast bit for bit
  plain = torch.empty_like(out)
  call('edet_cast', ptr(pooled), ptr(plain), n * c, edt, gu.stream())
  for m in (torch.ones_like(mask), None):
    out.fill_(3.0)
    call('edet_dropout_cast', ptr(pooled), ptr(m), ptr(out), n * c, edt, gu.stream())
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.uint8), plain.view(torch.uint8))
  # in place, fp32: the backward pass's use
  d = pooled.clone()
  call('edet_dropout_cast', ptr(d), ptr(mask), ptr(d), n * c, _lib.EDET_F32, gu.stream())
  torch.cuda.synchronize()
  assert torch.equal(d, pooled * mask)


# ------------------------------------------------------------------------------------ GPU: the train step
def _perturbed(spec, seed):
  """Reference initialisers with every BatchNorm variable / bias perturbed (the problem of test_effnetv2.py's backward test)."""
  vals = effnetv2_model.init_params(spec, seed)
  rng = np.random.default_rng(seed + 1)
  for p in spec.params:
    v = vals[p.name]
    if p.name.endswith(('/gamma', '/beta', '/moving_mean')):
      v += 0.2 * rng.standard_normal(v.shape).astype(np.float32)
    elif p.name.endswith('/moving_variance'):
      v *= rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
    elif p.name.endswith('/bias'):
      v += 0.1 * rng.standard_normal(v.shape).astype(np.float32)
    vals[p.name] = v
  return vals


def oracle_train_step(model_name, over, vals, images, labels, smoothing, weight_decay, drop_scale=None, dropout_mask=None):
  """One training forward + loss + autograd of the fp32 oracle -> (loss without L2, L2 loss, {name: gradient incl. the L2
  term}, new moving statistics).  drop_scale / dropout_mask: the device's draws (inputs of the oracle)."""
  params = {k: torch.from_numpy(np.array(v, dtype=np.float32)).requires_grad_(not k.endswith(('moving_mean', 'moving_variance')))
            for k, v in vals.items()}
  oracle = v2orc.V2Oracle(model_name, over, params=params)
  oracle.drop_scale = drop_scale or {}
  ends = oracle.forward(torch.as_tensor(images, dtype=torch.float32), True)
  n = oracle.mconfig.model_name
  pooled = ends['pooled_features']
  if dropout_mask is not None:
    pooled = pooled * dropout_mask       # tf.keras.layers.Dropout between pooling and the dense layer
  logits = pooled @ params[n + '/head/dense/kernel'] + params[n + '/head/dense/bias']
  loss, _ = xent(logits, torch.as_tensor(labels), smoothing)
  l2 = sum((0.5 * weight_decay * (p * p).sum() for k, p in params.items()
            if p.requires_grad and netspec.is_l2_regularised(k)), torch.zeros(()))
  (loss + l2).backward()
  grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).numpy() for k, p in params.items() if p.requires_grad}
  return float(loss.detach()), float(l2.detach()), grads, {k: v.numpy() for k, v in oracle.new_moving.items()}, logits.detach()


@pytest.mark.gpu
@pytest.mark.parametrize('model_name,size', [('efficientnetv2-b0', 64), ('efficientnetv2-s', 96)])
def test_train_step_matches_oracle_fp32(model_name, size):
  """One RMSprop train_step with the DEFAULT dropout rate and stochastic depth, fp32 storage, against the oracle that is
  handed the device's draws: loss 1e-3; every gradient within 1e-2 * max(|g|_max of the tensor, 1e-4 g_max) (the bound of
  test_model_backward_matches_oracle_fp32); every updated variable within lr / sqrt(epsilon) times that gradient bound (the
  largest slope of the RMSprop update from zero slots, reached at g = 0); moving statistics within 1e-3."""
  over, batch, lr, wd, smoothing = 'num_classes=24', 4, 0.01, 1e-4, 0.1
  spec = effnetv2_model.V2Spec(effnetv2_configs.model_config(model_name, over))
  assert spec.mconfig.dropout_rate > 0 and spec.mconfig.survival_prob > 0
  vals = _perturbed(spec, 9)
  rng = np.random.default_rng(13)
  images = rng.standard_normal((batch, size, size, 3)).astype(np.float32)
  labels = rng.integers(0, 24, batch)
  net = effnetv2_train.TrainableModel(model_name, over, dtype='f32', params=vals, use_graph=False, learning_rate=lr,
                                      weight_decay=wd, label_smoothing=smoothing)
  out = net.train_step((images, labels))
  torch.cuda.synchronize()
  eng = net.engine
  assert eng.dropout_mask is not None and eng.drop_masks
  drop_scale = {k[:-len(':out')]: m[:, 0].detach().cpu().clone() for k, (m, p) in eng.drop_masks.items()}
  loss, l2, grads, moving, logits = oracle_train_step(model_name, over, vals, images, labels, smoothing, wd, drop_scale,
                                                      eng.dropout_mask.cpu().clone())
  print('%s@%d: loss %.6f (oracle %.6f), L2 %.6f (%.6f), gradient norm %.4f' % (
      model_name, size, out['loss'] - out['reg_l2_loss'], loss, out['reg_l2_loss'], l2, out['gradient_norm']))
  assert abs(out['loss'] - out['reg_l2_loss'] - loss) <= 1e-3 * abs(loss), (out, loss)
  assert abs(out['reg_l2_loss'] - l2) <= 1e-3 * l2, (out, l2)
  assert abs(out['loss'] - (loss + l2)) <= 1e-3 * (loss + l2)
  assert out['acc_top1'] == topk_rows(logits, torch.as_tensor(labels), 1) / batch
  assert out['acc_top5'] == topk_rows(logits, torch.as_tensor(labels), 5) / batch
  assert out['learning_rate'] == lr
  gn = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads.values())))
  assert abs(out['gradient_norm'] - gn) <= 1e-2 * gn
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
  state = net.get_optimizer_state()
  assert state['iterations'] == 1 and 'rms' in state and 'adam_v' not in state and float(state['rms'].max()) > 0


@pytest.mark.gpu
def test_dropout_is_on_in_training_only():
  model_name, over, size, batch = 'efficientnetv2-b0', 'num_classes=24', 64, 4
  rng = np.random.default_rng(5)
  images = rng.standard_normal((batch, size, size, 3)).astype(np.float32)
  labels = rng.integers(0, 24, batch)
  net = effnetv2_train.TrainableModel(model_name, over, dtype='f32', use_graph=False, learning_rate=0.0)
  rate = net.cfg_model.dropout_rate
  net.train_step((images, labels))
  m1 = net.engine.dropout_mask.cpu().clone()
  values = np.unique(m1.numpy()).tolist()
  assert len(values) == 2 and values[0] == 0.0 and abs(values[1] - 1.0 / (1.0 - rate)) <= 1e-6, values
  frac = float((m1 == 0).float().mean())
  assert abs(frac - rate) < 0.05, frac
  # learning rate 0: the variables stay, the moving statistics do not -- freeze them out of the comparison below
  t1 = net.test_step((images, labels))
  net.train_step((images, labels))
  m2 = net.engine.dropout_mask.cpu().clone()
  assert not torch.equal(m1, m2), 'two consecutive steps drew the same dropout mask'
  # test_step does not see the mask: the same inference result under two different masks
  state = net.get_weights()
  net.engine.dropout_mask.copy_(m1.to(gu.DEV))
  a = net.test_step((images, labels))
  net.engine.dropout_mask.copy_(m2.to(gu.DEV))
  b = net.test_step((images, labels))
  assert a == b and np.isfinite(a['loss']) and set(a) == {'loss', 'reg_l2_loss', 'acc_top1', 'acc_top5'}
  assert all(np.array_equal(v, net.get_weights()[k]) for k, v in state.items()), 'test_step changed a variable'
  assert np.isfinite(t1['loss'])
  # EffNetV2Model's own call keeps refusing dropout, and labels out of range never reach the device
  with pytest.raises(ValueError):
    net(torch.from_numpy(images), training=True)
  with pytest.raises(ValueError):
    net.train_step((images, np.array([0, 1, 24, 2])))


def _steps(use_graph, optimizer='rmsprop', ema_decay=None, steps=4):
  model_name, over, size, batch = 'efficientnetv2-b0', 'num_classes=24', 64, 4
  spec = effnetv2_model.V2Spec(effnetv2_configs.model_config(model_name, over))
  vals = _perturbed(spec, 3)
  rng = np.random.default_rng(29)
  sched = effnetv2_train.WarmupLearningRateSchedule(0.01, steps_per_epoch=2, lr_decay_type='cosine', total_steps=10,
                                                    warmup_epochs=1)
  net = effnetv2_train.TrainableModel(model_name, over, params=vals, use_graph=use_graph, learning_rate=sched,
                                      weight_decay=1e-5, label_smoothing=0.1, optimizer=optimizer, ema_decay=ema_decay, seed=4)
  outs = []
  for _ in range(steps):
    images = rng.standard_normal((batch, size, size, 3)).astype(np.float32)
    labels = rng.integers(0, 24, batch)
    outs.append(net.train_step((images, labels)))
  torch.cuda.synchronize()
  return net, outs


@pytest.mark.gpu
@pytest.mark.parametrize('optimizer', ['rmsprop', 'momentum', 'adam'])
def test_graph_replay_equals_eager(optimizer):
  """bf16 storage (the default): four steps -- the first eager, as the trainer always runs it, then three replays of the
  captured hipGraph, so that two replays follow a replay -- leave exactly the state of four eager steps -- variables, both slot arenas, EMA shadows, moving statistics, and the same metrics."""
  g, og = _steps(True, optimizer, 0.99)
  e, oe = _steps(False, optimizer, 0.99)
  assert g._graph['graph'] is not None and g._graph['steps'] == 4 and e._graph is None
  assert og == oe, (og, oe)
  assert og[0]['learning_rate'] == 0.0 and og[1]['learning_rate'] > 0
  a, b = g.engine.arena, e.engine.arena
  assert a.step_count == b.step_count == 4
  for key in ('params_flat', 'velocity', 'ema', 'state_flat'):
    assert torch.equal(getattr(a, key), getattr(b, key)), key
  if optimizer != 'momentum':
    assert torch.equal(a.adam_v, b.adam_v) and float(a.adam_v.abs().max()) > 0
  assert torch.equal(g.engine.dropout_mask, e.engine.dropout_mask)
  assert not torch.equal(a.ema, a.params_flat)


@pytest.mark.gpu
def test_test_step_between_replayed_steps_changes_nothing():
  """An eager inference pass (test_step) on the buffers of the captured engine, between replayed steps: the training run
  ends in exactly the state of the run without it, and test_step leaves the gradient arena of the last train_step alone."""
  model_name, over, size, batch = 'efficientnetv2-b0', 'num_classes=24', 64, 4
  rng = np.random.default_rng(41)
  data = [(rng.standard_normal((batch, size, size, 3)).astype(np.float32), rng.integers(0, 24, batch)) for _ in range(4)]
  nets = []
  for with_eval in (False, True):
    net = effnetv2_train.TrainableModel(model_name, over, use_graph=True, learning_rate=0.01, weight_decay=1e-4,
                                        label_smoothing=0.1, seed=6)
    for i, d in enumerate(data):
      net.train_step(d)
      if with_eval and i >= 1:
        grads = net.engine.grads_flat.clone()
        gnorm, fac = net.engine.gnorm.clone(), net.engine.seg_factor.clone()
        out = net.test_step(d)
        assert np.isfinite(out['loss']) and out['reg_l2_loss'] > 0
        assert torch.equal(net.engine.grads_flat, grads) and torch.equal(net.engine.gnorm, gnorm)
        assert torch.equal(net.engine.seg_factor, fac)
    torch.cuda.synchronize()
    nets.append(net)
  a, b = nets[0].engine.arena, nets[1].engine.arena
  for key in ('params_flat', 'velocity', 'adam_v', 'state_flat'):
    assert torch.equal(getattr(a, key), getattr(b, key)), key
  # the evaluation L2 term is the training one (same variables, same weight decay), from another summation order
  l2_eval = nets[1].test_step(data[0])['reg_l2_loss']
  l2_train = nets[1].train_step(data[0])['reg_l2_loss']
  assert abs(l2_eval - l2_train) <= 1e-3 * l2_train, (l2_eval, l2_train)
  # device labels: unchecked by default, checked on request
  bad = torch.tensor([0, 1, 24, 2], device=gu.DEV)
  strict = effnetv2_train.TrainableModel(model_name, over, use_graph=False, check_device_labels=True)
  with pytest.raises(ValueError):
    strict.train_step((data[0][0], bad))
  # one optimizer per arena
  with pytest.raises(ValueError):
    nets[1].engine.arena.use_second_slot('adam_v')


@pytest.mark.gpu
def test_state_round_trip():
  """get_optimizer_state after two steps -> a fresh TrainableModel -> set_optimizer_state + weights -> its third step is
  the uninterrupted third step bit for bit (slots, iteration count for the schedule, and the generator behind the draws)."""
  model_name, over, size, batch = 'efficientnetv2-b0', 'num_classes=24', 64, 4
  rng = np.random.default_rng(31)
  data = [(rng.standard_normal((batch, size, size, 3)).astype(np.float32), rng.integers(0, 24, batch)) for _ in range(3)]
  sched = effnetv2_train.WarmupLearningRateSchedule(0.01, steps_per_epoch=1, lr_decay_type='linear', total_steps=10,
                                                    warmup_epochs=1)
  kw = dict(use_graph=False, learning_rate=sched, weight_decay=1e-5, label_smoothing=0.1, seed=2)
  net = effnetv2_train.TrainableModel(model_name, over, **kw)
  net.train_step(data[0])
  net.train_step(data[1])
  state, weights = net.get_optimizer_state(), net.get_weights()
  assert state['iterations'] == 2 and 'rms' in state and 'rng_state' in state
  want = net.train_step(data[2])
  other = effnetv2_train.TrainableModel(model_name, over, **kw)
  other.set_weights(weights)
  other.set_optimizer_state(state)
  got = other.train_step(data[2])
  torch.cuda.synchronize()
  assert got == want and got['learning_rate'] == sched(2)
  a, b = net.engine.arena, other.engine.arena
  for key in ('params_flat', 'velocity', 'adam_v', 'state_flat'):
    assert torch.equal(getattr(a, key), getattr(b, key)), key
  assert other.iterations == 3 and b.step_count == 3
  assert torch.equal(net.engine.dropout_mask, other.engine.dropout_mask)


LEARN = dict(model_name='efficientnetv2-b0', over='num_classes=24,survival_prob=0,dropout_rate=0', size=64, lr=1e-3,
             smoothing=0.1, steps=30)


def _learn_problem():
  spec = effnetv2_model.V2Spec(effnetv2_configs.model_config(LEARN['model_name'], LEARN['over']))
  vals = effnetv2_model.init_params(spec, 0)
  rng = np.random.default_rng(0)
  images = rng.standard_normal((8, LEARN['size'], LEARN['size'], 3)).astype(np.float32)
  return vals, images, np.arange(8)


def oracle_learning_curve(steps=None):
  """The fp32 restatement of test_it_learns' run on the CPU -> the training-mode loss of every step."""
  vals, images, labels = _learn_problem()
  vals = {k: v.copy() for k, v in vals.items()}
  slots = {}
  losses = []
  for _ in range(steps or LEARN['steps']):
    loss, _, grads, moving, _ = oracle_train_step(LEARN['model_name'], LEARN['over'], vals, images, labels, LEARN['smoothing'], 0.0)
    losses.append(loss)
    for k, g in grads.items():
      ms, mom = slots.setdefault(k, (np.zeros_like(g), np.zeros_like(g)))
      rmsprop_step(vals[k], g, ms, mom, LEARN['lr'])
    vals.update({k: v.copy() for k, v in moving.items()})
  return losses


@pytest.mark.gpu
def test_it_learns():
  """A fixed batch of 8 standard-normal 64 px images with the labels 0..7, efficientnetv2-b0 (24 classes, no stochastic
  depth, no dropout) from init_params(spec, 0), fp32 storage, RMSprop at a constant 1e-3, label smoothing 0.1, no weight
  decay: the training-mode loss of the 30th train_step is below half of the first one's.  The fp32 oracle restatement of
  exactly this run (oracle_learning_curve above, CPU) gives 4.1716 at step 1, 2.2924 at step 11 and 0.8720 at step 30.
  The test_step loss is NOT asserted on: thirty steps at BatchNorm momentum 0.9 on 8 images whose last maps are 2 x 2 leave
  the moving statistics far from the batch statistics, so the reference's own inference-mode loss rises over this run."""
  vals, images, labels = _learn_problem()
  net = effnetv2_train.TrainableModel(LEARN['model_name'], LEARN['over'], dtype='f32', params=vals, learning_rate=LEARN['lr'],
                                      label_smoothing=LEARN['smoothing'], weight_decay=0.0, optimizer='rmsprop')
  losses = [net.train_step((images, labels))['loss'] for _ in range(LEARN['steps'])]
  print('training-mode loss: step 1 %.4f, step 11 %.4f, step 30 %.4f' % (losses[0], losses[10], losses[-1]))
  assert np.isfinite(losses).all()
  assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
