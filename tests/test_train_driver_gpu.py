"""The detector training driver on the device: EfficientDetNetTrain.fit / evaluate, ModelCheckpoint with the training-state
file, exact resume, the validation pass and automl_amd.train.main, all bit for bit against the pieces called by hand.

Shards are written here from the small JPEGs of tests/golden/jpeg_cases.npz (at most 37 x 53) with a few boxes each; the model
is efficientdet-d0 at image_size=128, batch 2, canvas 64 x 64, ten training records in two shards -- the smallest shapes that
still pass through every stage (reader, JPEG decoder, input stage, captured step, checkpoint)."""
import os

import numpy as np
import pytest
import torch

from automl_amd import dataloader, eval_lib, hparams_config, tf_checkpoint, train, train_lib, util_keras
from oracle.problems import perturbed_params
from tests.test_dataloader import CANVAS, GOLDEN, IMAGES, record, write_shards

pytestmark = pytest.mark.gpu
SEED = 13
KEYS = train_lib.engine_lib.Engine.LOSS_KEYS
_PARAMS = {}


@pytest.fixture(scope='module')
def jpegs():
  g = np.load(GOLDEN)
  return [g[n + '/bytes'].tobytes() for n in IMAGES]


def train_shards(jpegs, folder):
  folder.mkdir(exist_ok=True)
  records = [record(jpegs[k % len(jpegs)], k, 1 + k % 4) for k in range(10)]
  return write_shards(folder, [records[:5], records[5:]], name='train')


def val_shards(jpegs, folder):
  folder.mkdir(exist_ok=True)
  records = [record(jpegs[(k + 2) % len(jpegs)], 50 + k, 1 + k % 3, source_id=str(200 + k), crowd=[0] * (1 + k % 3),
                    area=[400.0 + k] * (1 + k % 3)) for k in range(6)]
  return write_shards(folder, [records[:3], records[3:]], name='val')


def make_config(name='efficientdet-d0', **kw):
  config = hparams_config.get_efficientdet_config(name)
  config.override('image_size=128')
  config.override(kw, True)
  return config


def reader_of(config, pattern, is_training=True, seed=SEED):
  p = config.as_dict()
  p['tf_random_seed'] = seed
  if not is_training:
    p['drop_remainder'] = False
  return dataloader.InputReader(pattern, is_training=is_training).reader(p, batch_size=2, canvas=CANVAS)


def new_net(config, use_graph=True, autoaugment=None, fresh=False, cls=train_lib.EfficientDetNetTrain):
  """fresh: its own initial values and another seed -- a model that is about to be restored."""
  if not fresh and config.name not in _PARAMS:
    _PARAMS[config.name] = perturbed_params(config, 3)
  net = cls(config=config, dtype='bf16', params=None if fresh else _PARAMS[config.name], seed=99 if fresh else 5,
            steps_per_epoch=3, global_batch_size=64, use_graph=use_graph)
  if autoaugment:
    net.set_autoaugment(autoaugment)
  return net


def full_state(net, reader=None):
  """Every piece of the training state, on the host."""
  torch.cuda.synchronize()
  state = {'weights': net.get_weights(), 'shadows': net.get_ema_weights(), 'optimizer': net.get_optimizer_state(),
           'drop_rng': {key: eng.drop_rng_state() for key, eng in net._engines.items()}, 'iterations': net.iterations}
  if reader is not None:
    state['reader'] = reader.get_state()
  return state


def assert_state_equal(a, b, what):
  assert sorted(a) == sorted(b), what
  assert a['iterations'] == b['iterations'], what
  assert a.get('reader') == b.get('reader'), (what, 'reader')
  for part in ('weights', 'shadows', 'optimizer', 'drop_rng'):
    assert sorted(a[part]) == sorted(b[part]), (what, part, sorted(a[part]), sorted(b[part]))
    for k in a[part]:
      x, y = np.asarray(a[part][k]), np.asarray(b[part][k])
      assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8)), \
          (what, part, k)
  assert any('moving_mean' in k for k in a['weights'])      # the BatchNorm moving statistics are among the variables


def step_order_mean(values, key):
  """Keras' Mean in float32: the sum in step order, divided by the count."""
  total = np.float32(0)
  for v in values:
    total = np.float32(total + np.float32(v[key]))
  return float(np.float32(total / np.float32(len(values))))


# --------------------------------------------------------------------------------------------------------------- fit
@pytest.mark.parametrize('use_graph, momentum', [(True, 0.9), (False, None)], ids=['graph-positives_momentum', 'eager'])
def test_fit_is_the_hand_loop(jpegs, tmp_path, use_graph, momentum):
  config = make_config(positives_momentum=momentum)
  pattern = train_shards(jpegs, tmp_path / 'data')
  fitted, by_hand = new_net(config, use_graph), new_net(config, use_graph)
  r_fit, r_hand = reader_of(config, pattern), reader_of(config, pattern)
  history = fitted.fit(r_fit, epochs=2, steps_per_epoch=3, verbose=0)
  values = [by_hand.train_step_raw(next(r_hand)) for _ in range(6)]
  got, want = full_state(fitted, r_fit), full_state(by_hand, r_hand)
  r_fit.close()
  r_hand.close()
  assert_state_equal(got, want, 'fit against six steps')
  assert got['iterations'] == 6 and got['optimizer']['iterations'] == 6 and 'input_rng_state' in got['optimizer']
  assert ('moving_normalizer' in got['optimizer']) == bool(momentum)
  assert history.epoch == [0, 1] and sorted(history.history) == sorted(KEYS + ('learning_rate',))
  for e in range(2):
    for k in KEYS:
      want_mean = step_order_mean(values[3 * e:3 * e + 3], k)
      print(use_graph, e, k, history.history[k][e], want_mean)
      assert history.history[k][e] == want_mean and np.isfinite(want_mean), (e, k, history.history[k][e], want_mean)
    assert history.history['learning_rate'][e] == values[3 * e + 2]['learning_rate']
  assert history.history['cls_loss'][0] > 0 and history.history['loss'][0] != history.history['loss'][1]


class Spy(train_lib.EfficientDetNetTrain):
  """Records the arguments of train_step_raw and the reads of the loss accumulator."""
  calls, reads = None, 0

  def train_step_raw(self, data, sync_loss=True, draws=None):
    self.calls = (self.calls or []) + [(sync_loss, draws)]
    return super().train_step_raw(data, sync_loss=sync_loss, draws=draws)

  def _read_losses(self, acc):
    self.reads += 1
    return super()._read_losses(acc)


def test_fit_does_not_wait_per_step(jpegs, tmp_path, monkeypatch):
  """sync_loss=False on every step, the per-step values never read (Engine.loss_values is not called), the accumulator read
  once per epoch -- and once per batch only for a batch-level callback that accesses a device value."""
  config = make_config()
  pattern = train_shards(jpegs, tmp_path / 'data')
  net = new_net(config, cls=Spy)
  reader = reader_of(config, pattern)
  host_reads = []
  monkeypatch.setattr(train_lib.engine_lib.Engine, 'loss_values', lambda self: host_reads.append(1))
  seen = []

  class HostOnly(object):
    def on_train_batch_end(self, step, logs):
      seen.append((step, logs['learning_rate'], logs['step'], 'loss' in logs))
  net.fit(reader, epochs=2, steps_per_epoch=2, callbacks=[HostOnly()], verbose=0)
  assert net.calls == [(False, None)] * 4 and net.reads == 2 and not host_reads
  assert [s[0] for s in seen] == [0, 1, 0, 1] and [s[2] for s in seen] == [1, 2, 3, 4] and all(s[3] for s in seen)
  running = []

  class Asks(object):
    def on_train_batch_end(self, step, logs):
      running.append((logs['loss'], logs['cls_loss']))
  history = net.fit(reader, epochs=3, initial_epoch=2, steps_per_epoch=2, callbacks=[Asks()], verbose=0)
  reader.close()
  assert net.reads == 2 + 2 + 1 and len(net.calls) == 6 and not host_reads
  assert history.epoch == [2] and history.history['loss'] == [running[-1][0]]      # the running mean after the last batch


# ------------------------------------------------------------------------------------------------------------- resume
@pytest.mark.parametrize('case', ['plain', 'augment', 'd1'])
def test_resume_is_exact(jpegs, tmp_path, case):
  """A: two epochs of three steps with checkpoints.  B: one epoch; then a NEW model with its own initial values and seed and a
  new reader with another seed, both restored from B's model_dir; then the second epoch.  'augment' has grid_mask and
  AutoAugment v2, so the input generator matters; 'd1' is efficientdet-d1 at the same size, whose backbone has the
  stochastic-depth masks, so the engine's generator matters."""
  config = make_config('efficientdet-d1' if case == 'd1' else 'efficientdet-d0', grid_mask=(case == 'augment'))
  policy = 'v2' if case == 'augment' else None
  pattern = train_shards(jpegs, tmp_path / 'data')

  def run(net, reader, model_dir, **kw):
    p = config.as_dict()
    p['model_dir'] = str(model_dir)
    history = net.fit(reader, steps_per_epoch=3, callbacks=train_lib.get_callbacks(p), verbose=0, **kw)
    state = full_state(net, reader)
    reader.close()
    return history, state
  hist_a, state_a = run(new_net(config, autoaugment=policy), reader_of(config, pattern), tmp_path / 'a', epochs=2)
  run(new_net(config, autoaugment=policy), reader_of(config, pattern), tmp_path / 'b', epochs=1)
  latest = tf_checkpoint.latest_checkpoint(str(tmp_path / 'b'))
  assert os.path.basename(latest) == 'emackpt-1'
  net, reader = new_net(config, autoaugment=policy, fresh=True), reader_of(config, pattern, seed=999)
  util_keras.restore_ckpt(net, latest, config.moving_average_decay, skip_mismatch=False)
  meta = train_lib.restore_train_state(net, train_lib.train_state_path(latest), reader=reader)
  assert net.engine is None and net.iterations == 3 and meta['iterations'] == 3      # restored before anything was built
  hist_b, state_b = run(net, reader, tmp_path / 'b', epochs=2, initial_epoch=1)
  assert_state_equal(state_b, state_a, 'resumed against uninterrupted')
  assert state_a['iterations'] == 6 and state_a['reader']['emitted'] == 2 and state_a['reader']['epoch'] == 1
  assert state_a['drop_rng'] and all(v.size == 16 for v in state_a['drop_rng'].values())
  if case == 'd1':
    assert net.engine.drop_masks      # the generator was used: its restored state mattered
    fresh = new_net(config, fresh=True)
    assert train_lib.arena_length(fresh) == net.engine.arena.velocity.numel()
  assert hist_b.epoch == [1] and hist_a.epoch == [0, 1]
  for k in KEYS + ('learning_rate',):
    assert hist_b.history[k] == hist_a.history[k][1:], k
  # and the files of the second epoch are the same files
  names = sorted(os.listdir(tmp_path / 'a'))
  assert names == sorted(['checkpoint'] + ['emackpt-%d%s' % (e, s) for e in (1, 2)
                                          for s in ('.index', '.data-00000-of-00001', '.train_state.npz')])
  assert sorted(os.listdir(tmp_path / 'b')) == names
  for s in ('.index', '.data-00000-of-00001'):
    assert (tmp_path / 'a' / ('emackpt-2' + s)).read_bytes() == (tmp_path / 'b' / ('emackpt-2' + s)).read_bytes(), s
  (meta_a, arrays_a), (meta_b, arrays_b) = (train_lib.load_train_state(str(tmp_path / d / 'emackpt-2.train_state.npz')) for d in 'ab')
  assert meta_a == meta_b and sorted(arrays_a) == sorted(arrays_b) and all(np.array_equal(arrays_a[k], arrays_b[k]) for k in arrays_a)


# --------------------------------------------------------------------------------------------- evaluate and traineval
def test_evaluate_is_the_mean_of_the_test_steps(jpegs, tmp_path):
  config = make_config()
  val = train_lib.RepeatableReader(reader_of(config, val_shards(jpegs, tmp_path / 'val'), is_training=False))
  net = new_net(config)
  got = net.evaluate(val, steps=3)
  values = [net.test_step_raw(batch)[0] for batch in val]      # replays of the pass evaluate ran eagerly, captured and replayed
  assert len(values) == 3 and sorted(got) == sorted(KEYS)
  for k in KEYS:
    assert got[k] == step_order_mean(values, k), k
  assert got['cls_loss'] > 0 and len({v['loss'] for v in values}) == 3
  assert net.evaluate(val, steps=2) == {k: step_order_mean(values[:2], k) for k in KEYS}
  assert net.evaluate(val) == got      # every batch of the data
  val.close()
  assert net.iterations == 0 and net.get_optimizer_state()['iterations'] == 0 and 'input_rng_state' not in net.get_optimizer_state()


def test_traineval_logs_and_training_state(jpegs, tmp_path):
  config = make_config(map_freq=1)
  train_reader = reader_of(config, train_shards(jpegs, tmp_path / 'data'))
  val = train_lib.RepeatableReader(reader_of(config, val_shards(jpegs, tmp_path / 'val'), is_training=False))
  net = new_net(config)
  after_last_step = []

  class Snapshot(object):
    def on_train_batch_end(self, step, logs):
      if step == 1:
        after_last_step.append(full_state(net, train_reader))
  p = config.as_dict()
  p['model_dir'] = str(tmp_path / 'run')
  callbacks = [Snapshot()] + train_lib.get_callbacks(p, val)
  assert [type(c).__name__ for c in callbacks] == ['Snapshot', 'ModelCheckpoint', 'COCOCallback']
  history = net.fit(train_reader, epochs=1, steps_per_epoch=2, callbacks=callbacks, validation_data=val, validation_steps=2, verbose=0)
  logs = {k: v[0] for k, v in history.history.items()}
  # the validation pass and the COCO pass moved nothing of the training state
  assert_state_equal(full_state(net, train_reader), after_last_step[0], 'after validation')
  train_reader.close()
  losses = net.evaluate(val, steps=2)
  metrics = eval_lib.evaluate(net, val)
  val.close()
  names = ['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'ARmax1', 'ARmax10', 'ARmax100', 'ARs', 'ARm', 'ARl']
  assert sorted(logs) == sorted(KEYS + ('learning_rate',) + tuple('val_' + k for k in KEYS) + tuple(names))
  for k in KEYS:
    assert logs['val_' + k] == losses[k] and np.isfinite(losses[k]), k
  for k in names:
    assert logs[k] == metrics[k], k
  assert logs['val_reg_l2_loss'] != logs['reg_l2_loss']      # the variables after the epoch, not the mean over its steps
  assert os.path.exists(train_lib.train_state_path(str(tmp_path / 'run' / 'emackpt-1')))


# ----------------------------------------------------------------------------------------------------------------- main
def test_main_trains_continues_and_evaluates(jpegs, tmp_path, capsys):
  model_dir = tmp_path / 'run'
  common = ['--model_dir=%s' % model_dir, '--batch_size=2', '--num_examples_per_epoch=4', '--hparams=image_size=128',
            '--canvas=%dx%d' % CANVAS, '--tf_random_seed=7', '--train_file_pattern=%s' % train_shards(jpegs, tmp_path / 'data'),
            '--val_file_pattern=%s' % val_shards(jpegs, tmp_path / 'val')]

  def files(epochs):
    return sorted(['checkpoint', 'config.yaml'] + ['emackpt-%d%s' % (e, s) for e in epochs
                                                   for s in ('.index', '.data-00000-of-00001', '.train_state.npz')])
  first = train.main(common + ['--mode=train', '--num_epochs=1'])
  assert first.epoch == [0] and sorted(os.listdir(model_dir)) == files([1])
  config_yaml = (model_dir / 'config.yaml').read_text()
  second = train.main(common + ['--mode=train', '--num_epochs=2'])      # picks the run up where the checkpoint left it
  assert second.epoch == [1] and sorted(os.listdir(model_dir)) == files([1, 2])
  assert (model_dir / 'config.yaml').read_text() == config_yaml
  meta, _ = train_lib.load_train_state(str(model_dir / 'emackpt-2.train_state.npz'))
  assert meta['iterations'] == 4 and meta['reader']['epoch'] == 0 and meta['reader']['emitted'] == 8
  assert all(np.isfinite(v[0]) for v in list(first.history.values()) + list(second.history.values()))
  done = train.main(common + ['--mode=train', '--num_epochs=2'])      # nothing is left to do
  assert done.epoch == [] and sorted(os.listdir(model_dir)) == files([1, 2])
  capsys.readouterr()
  metrics = train.main(common + ['--mode=eval'])
  assert sorted(metrics) == sorted(['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'ARmax1', 'ARmax10', 'ARmax100', 'ARs', 'ARm', 'ARl'])
  assert all(np.isfinite(v) for v in metrics.values()) and 'emackpt-2' in capsys.readouterr().out
  assert sorted(os.listdir(model_dir)) == files([1, 2])
  # traineval goes on from there: a third epoch with the validation pass and, at map_freq=1, the COCO pass in its logs
  third = train.main(common + ['--mode=traineval', '--num_epochs=3', '--hparams=image_size=128,map_freq=1', '--eval_samples=4'])
  assert third.epoch == [2] and sorted(os.listdir(model_dir)) == files([1, 2, 3])
  assert {'loss', 'val_loss', 'val_cls_loss', 'AP', 'ARl', 'learning_rate'} <= set(third.history)
  assert np.isfinite(third.history['val_loss'][0]) and third.history['val_loss'][0] != third.history['loss'][0]
