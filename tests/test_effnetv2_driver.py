"""The classifier training driver without a device: the stage fit applies per epoch against progressive_stages, the epoch-log
arithmetic from a given accumulator, fit's loop (callbacks, lazy batch logs, early end, validation) over a model whose steps are
replaced by host stand-ins, the training-state file through a model without an engine, effnetv2_main's refusals -- each before
a model exists -- and its configuration assembly for the EfficientNetV2-S recipe.  The runs are in
tests/test_effnetv2_driver_gpu.py."""
import json
import os
import types

import numpy as np
import pytest
import torch

from automl_amd import effnetv2_main as main_lib, effnetv2_train as et, train_lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_v2_driver.json')


def small(**kw):
  args = dict(learning_rate=0.01, augname='randaug', ra_magnitude=9, mixup_alpha=0.1, cutmix_alpha=0.2, image_size=48, seed=3)
  args.update(kw)
  return et.TrainableModel('efficientnetv2-b0', 'num_classes=24', **args)


class HostSteps(et.TrainableModel):
  """TrainableModel whose steps run nothing: train_step / test_step put step-numbered sums where the engine's cls_sums are
  (on the host) and record what the model was set to."""

  def __init__(self, *args, **kwargs):
    super().__init__(*args, **kwargs)
    self.seen, self.tested = [], 0

  def _sums(self, k):
    self.engine = types.SimpleNamespace(batch=4, cls_sums=torch.tensor([1.0 + 0.1 * k, k % 5, 4.0, 0.3], dtype=torch.float32))

  def train_step(self, data, sync_loss=True):
    assert sync_loss is False
    self.seen.append((data, self.iterations, self.image_size, self.ra_magnitude, self.mixup_alpha, self.cutmix_alpha))
    self._sums(self.iterations)
    self.iterations += 1
    return {'learning_rate': 0.5 / self.iterations}

  def test_step(self, data, sync_loss=True):
    assert sync_loss is False
    self.tested += 1
    self._sums(100 + data)
    return {}


def host_sums(ks):
  acc = np.zeros(4, np.float32)
  for k in ks:
    acc += np.array([1.0 + 0.1 * k, k % 5, 4.0, 0.3], np.float32)
  return acc


# ---------------------------------------------------------------------------------------------------------- the stages
def test_stage_of_epoch_equals_progressive_stages():
  for name, epochs in (('efficientnetv2-s', 10), ('efficientnetv2-m', 7), ('efficientnetv2-s', 350)):
    stages = et.progressive_stages(name, epochs)
    assert len(stages) == 4
    for epoch in range(epochs):
      holding = [s for s in stages if s['start_epoch'] <= epoch < s['end_epoch']]
      assert len(holding) == 1 and et.stage_of_epoch(stages, epoch) is holding[0]
    assert et.stage_of_epoch(stages, epochs) is None
  # the plain-values form is the same arithmetic
  assert et.stage_list(300, 10, 4, True, 128, 10, 0, 0) == et.progressive_stages('efficientnetv2-s', 10)
  assert et.stage_list(384, 7, 4, True, 128, 15, 0.2, 0.2) == et.progressive_stages('efficientnetv2-m', 7)
  assert et.stage_list(300, 10, 0, True, 128, 10, 0, 0) == et.progressive_stages('efficientnetv2-s', 10, stages=0)


@pytest.mark.parametrize('initial_epoch', [0, 1, 3, 4, 5])
def test_fit_applies_the_stage_of_every_epoch(initial_epoch):
  stages = et.progressive_stages('efficientnetv2-m', 6, stages=3)      # epochs [0, 2), [2, 4), [4, 6)
  assert [(s['start_epoch'], s['end_epoch']) for s in stages] == [(0, 2), (2, 4), (4, 6)]
  model = HostSteps('efficientnetv2-b0', 'num_classes=24', learning_rate=0.01, augname='randaug', image_size=384, seed=3)
  model.iterations = 2 * initial_epoch
  calls = []
  set_stage = model.set_stage
  model.set_stage = lambda stage: (calls.append(stage), set_stage(stage))
  history = model.fit(iter(range(1000)), epochs=6, steps_per_epoch=2, initial_epoch=initial_epoch, stages=stages, verbose=0)
  assert history.epoch == list(range(initial_epoch, 6))
  for data, iteration, size, ram, mixup, cutmix in model.seen:
    s = stages[(iteration // 2) // 2]
    assert (size, ram, mixup, cutmix) == (s['image_size'], s['ra_magnitude'], s['mixup_alpha'], s['cutmix_alpha'])
  assert [d for d, *_ in model.seen] == list(range(2 * (6 - initial_epoch)))      # one iterator, never restarted
  # set_stage only where the stage differs from the model's: once per stage entered, never again inside it
  assert calls == [s for s in stages if s['end_epoch'] > initial_epoch]
  # a model that already is in the stage (a restored one) is left alone
  model2 = HostSteps('efficientnetv2-b0', 'num_classes=24', learning_rate=0.01, augname='randaug', image_size=384, seed=3)
  model2.set_stage(stages[1])
  model2.set_stage = lambda stage: calls.append('again')
  model2.fit(iter(range(4)), epochs=4, steps_per_epoch=2, initial_epoch=2, stages=stages, verbose=0)
  assert 'again' not in calls


# ------------------------------------------------------------------------------------------------------------- the logs
def test_epoch_logs_from_an_accumulator():
  acc = np.array([7.25, 9.0, 11.0, 0.75], np.float32)
  got = et.metrics_from_sums(acc, 3, 4)
  f = np.float32
  assert got == {'loss': float((f(7.25) + f(0.75)) / f(3)), 'reg_l2_loss': float(f(0.75) / f(3)), 'acc_top1': float(f(9) / f(12)),
                 'acc_top5': float(f(11) / f(12))}
  assert got['loss'] == float(np.float32(8.0) / np.float32(3.0)) != 8.0 / 3.0      # float32 arithmetic, as Keras' Mean
  assert set(et.metrics_from_sums(acc, 3, 4, prefix='val_')) == {'val_' + k for k in et.METRIC_KEYS}
  # one step in float64 is what train_step / test_step report
  s = np.array([1.3, 2.0, 3.0, 0.1], np.float32)
  one = et.metrics_from_sums(s, 1, 4, np.float64)
  assert one == {'loss': float(s[0]) + float(s[3]), 'reg_l2_loss': float(s[3]), 'acc_top1': float(s[1]) / 4, 'acc_top5': float(s[2]) / 4}


def test_fit_loop_logs_callbacks_and_early_end():
  model = HostSteps('efficientnetv2-b0', 'num_classes=24', learning_rate=0.01, seed=3)
  events = []

  class Callback(object):
    def set_model(self, m):
      events.append(('set_model', m is model))

    def on_train_begin(self, logs):
      events.append(('begin',))

    def on_epoch_begin(self, epoch, logs):
      events.append(('epoch_begin', epoch))

    def on_epoch_end(self, epoch, logs):
      events.append(('epoch_end', epoch, dict(logs)))

    def on_train_end(self, logs):
      events.append(('end', dict(logs)))

  class Batch(object):
    reads = []

    def on_train_batch_end(self, step, logs):
      assert isinstance(logs, train_lib.LazyLogs) and set(logs) == set(et.METRIC_KEYS) | {'learning_rate', 'step'}
      logs['learning_rate'], logs['step']      # host values: nothing is read
      if step == 1:
        self.reads.append((logs['step'], logs['loss'], logs['acc_top1']))

  reads = []
  read = model._epoch_metrics
  model._epoch_metrics = lambda *a, **k: (reads.append(1), read(*a, **k))[1]
  history = model.fit(iter(range(8)), epochs=5, steps_per_epoch=3, callbacks=[Callback(), Batch()], validation_data=[0, 1, 2],
                      validation_steps=2, verbose=0)
  # 8 batches: two epochs of 3, a third of 2, and fit ends early
  assert history.epoch == [0, 1, 2] and model.iterations == 8 and model.fit_input is not None
  for epoch, ks in enumerate(([0, 1, 2], [3, 4, 5], [6, 7])):
    want = et.metrics_from_sums(host_sums(ks), len(ks), 4)
    want['learning_rate'] = 0.5 / (ks[-1] + 1)
    want.update(et.metrics_from_sums(host_sums([100, 101]), 2, 4, prefix='val_'))
    got = {k: v[epoch] for k, v in history.history.items()}
    assert got == want, epoch
  assert model.tested == 3 * 2
  assert [e[0] for e in events] == ['set_model', 'begin'] + ['epoch_begin', 'epoch_end'] * 3 + ['end']
  assert events[-1][1] == events[-2][2]
  # the batch callback read once per epoch (step 1), the running values of that epoch so far
  assert Batch.reads[0] == (2, ) + tuple(et.metrics_from_sums(host_sums([0, 1]), 2, 4)[k] for k in ('loss', 'acc_top1'))
  assert len(Batch.reads) == 3 and len(reads) == 3 + 3 + 3      # batch reads, epoch reads, validation reads
  # stop_training ends the run after the epoch; an empty iterator ends it at once
  class Stop(object):
    def on_epoch_end(self, epoch, logs):
      model.stop_training = True
  assert model.fit(iter(range(100)), epochs=5, steps_per_epoch=2, callbacks=[Stop()], verbose=0).epoch == [0]
  assert model.fit(iter(()), epochs=5, steps_per_epoch=2, verbose=0).epoch == []
  with pytest.raises(ValueError, match='holds no batch'):
    model.evaluate([])


# ------------------------------------------------------------------------------------------------------ the state file
def hand_state(model, seed):
  rng = np.random.default_rng(seed)
  n = train_lib.arena_length(model)
  state = {'velocity': rng.standard_normal(n).astype(np.float32), 'ema': rng.standard_normal(n).astype(np.float32),
           'rms': rng.random(n).astype(np.float32), 'iterations': 7, 'rng_state': rng.integers(0, 256, 16).astype(np.uint8),
           'mix_rng_state': rng.integers(0, 2 ** 63, 6).astype(np.uint64), 'randaug_rng_state': rng.integers(0, 2 ** 63, 6).astype(np.uint64),
           'crop_rng_state': rng.integers(0, 2 ** 63, 6).astype(np.uint64)}
  return state


class Reader(object):
  def __init__(self):
    self.state = {'epoch': 1, 'buffer': [[0, 1], [2, 3]], 'rng': {'state': {'state': 2 ** 100 + 1}}}

  def get_state(self):
    return self.state

  def set_state(self, state):
    self.state = state


def test_train_state_round_trip_through_a_model_without_an_engine(tmp_path):
  src = small()
  state = hand_state(src, 5)
  src.set_optimizer_state(state)      # no engine: kept until the first one exists
  assert src.engine is None and src.iterations == 7
  src.set_stage({'image_size': 32, 'ra_magnitude': 6.5, 'mixup_alpha': 0.05, 'cutmix_alpha': 0.0})
  path = str(tmp_path / 'ckpt-2.train_state.npz')
  assert et.save_train_state(src, path, Reader()) == path and not os.path.exists(path + '.tmp')
  with np.load(path, allow_pickle=False) as z:
    meta = json.loads(z['meta'].tobytes().decode('utf-8'))
    assert sorted(z.files) == sorted(['meta'] + [k for k in state if k != 'iterations'])
  assert meta['iterations'] == 7 and meta['optimizer'] == 'rmsprop' and meta['kind'] == 'effnetv2'
  assert meta['stage'] == {'image_size': 32, 'ra_magnitude': 6.5, 'mixup_alpha': 0.05, 'cutmix_alpha': 0.0}
  dst, reader = small(), Reader()
  reader.state = None
  assert dst.current_stage() == {'image_size': 48, 'ra_magnitude': 9.0, 'mixup_alpha': 0.1, 'cutmix_alpha': 0.2}
  et.restore_train_state(dst, path, reader)
  assert dst.iterations == 7 and dst.engine is None and dst.current_stage() == meta['stage']
  assert reader.state == Reader().state
  pending = dst._pending_state
  assert sorted(pending) == sorted(state)
  for k, v in state.items():
    assert np.array_equal(np.asarray(pending[k]), np.asarray(v)) and np.asarray(pending[k]).dtype == np.asarray(v).dtype, k
  # and out again, unchanged
  again = str(tmp_path / 'again.npz')
  et.save_train_state(dst, again)
  with np.load(again, allow_pickle=False) as a, np.load(path, allow_pickle=False) as b:
    for k in state:
      if k != 'iterations':
        assert np.array_equal(a[k], b[k]), k
  with pytest.raises(ValueError, match='holds no reader state'):
    et.restore_train_state(small(), again, Reader())
  with pytest.raises(RuntimeError, match='not been built'):
    et.save_train_state(small(), again)      # nothing to save yet


def test_another_models_state_is_refused_with_the_difference_named(tmp_path):
  src = small()
  src.set_optimizer_state(hand_state(src, 1))
  path = str(tmp_path / 's.npz')
  et.save_train_state(src, path)
  with pytest.raises(ValueError, match=r'another model: the file has \d+ variables, this model \d+; \d+ arena elements, this model \d+$'):
    et.restore_train_state(et.TrainableModel('efficientnetv2-b1', 'num_classes=24'), path)
  with pytest.raises(ValueError, match=r'another model: the file has \d+ arena elements, this model \d+$'):
    et.restore_train_state(et.TrainableModel('efficientnetv2-b0', 'num_classes=25'), path)
  with pytest.raises(ValueError, match='another model: the file has rmsprop as optimizer, this model adam$'):
    et.restore_train_state(small(optimizer='adam'), path)
  # the detector's file is not a classifier's
  meta = {'format': train_lib.TRAIN_STATE_FORMAT, 'num_variables': 1, 'arena_length': 4, 'optimizer': 'sgd', 'iterations': 0}
  other = str(tmp_path / 'det.npz')
  np.savez(other, meta=np.frombuffer(json.dumps(meta).encode(), np.uint8))
  with pytest.raises(ValueError, match='not a classifier training state'):
    et.restore_train_state(small(), other)


def test_model_checkpoint_is_the_detectors_callback_with_this_trainers_files():
  cb = et.ModelCheckpoint('/x/ckpt-{epoch:d}')
  assert isinstance(cb, train_lib.ModelCheckpoint) and cb.save_freq == 'epoch' and cb.on_train_batch_end is None
  assert callable(et.ModelCheckpoint('/x/ckpt-{epoch:d}', save_freq=3).on_train_batch_end)
  assert cb.filepath.format(epoch=4) == '/x/ckpt-4'


# -------------------------------------------------------------------------------------------------------------- the CLI
def test_flags_keep_the_reference_names():
  f = main_lib.parse_flags([])
  want = dict(model_name='efficientnetv2-b0', dataset_cfg='Imagenet', hparam_str='', data_dir=None, model_dir=None, mode='train',
              sweeps='', use_tpu=False, tpu=None, export_to_tpu=False, canvas=(512, 512), dtype=None, seed=0)
  for k, v in want.items():
    assert getattr(f, k) == v, k
  f = main_lib.parse_flags(['--mode=traineval', '--canvas=56x64', '--dtype=f32', '--use_tpu=false', '--seed=4'])
  assert f.mode == 'traineval' and f.canvas == (56, 64) and f.dtype == 'f32' and f.seed == 4
  for bad in (['--mode=infer'], ['--canvas=64'], ['--dtype=fp8']):
    with pytest.raises(SystemExit):
      main_lib.parse_flags(bad)


OK_HPARAMS = 'data.augname=randaug'


@pytest.mark.parametrize('argv, reason', [
    (['--hparam_str=runtime.strategy=tpu,' + OK_HPARAMS], "runtime.strategy='tpu' is not built"),
    (['--hparam_str=runtime.strategy=gpus,' + OK_HPARAMS], "runtime.strategy='gpus' is not built"),
    (['--tpu=grpc://1.2.3.4:8470'], 'no TPU path'), (['--tpu_zone=z'], 'no TPU path'), (['--gcp_project=p'], 'no TPU path'),
    (['--use_tpu=true'], 'no TPU path'), (['--use_tpu'], 'no TPU path'), (['--export_to_tpu'], 'no TPU path'),
    (['--sweeps=train.lr_base=0.1*0.2'], 'sweeping is not built'),
    (['--dataset_cfg=cifar10ft'], 'is not built: .*tensorflow_datasets'), (['--dataset_cfg=imagenet21k'], 'is not built: .*sigmoid'),
    (['--hparam_str=data.ds_name=imagenettfds,' + OK_HPARAMS], 'is not built: .*tensorflow_datasets'),
    ([], "aug_name 'effnetv1_autoaug' is not built.*--hparam_str=data.augname=randaug"),      # efficientnetv2-b0's own recipe
    (['--dataset_cfg=imagenetft'], "aug_name 'ft' is not built.*--hparam_str=data.augname=randaug"),
    (['--hparam_str=data.augname=autoaug'], 'is not built.*data.augname'),
])
def test_every_refusal_comes_before_a_model(argv, reason, tmp_path, monkeypatch):
  made = []

  class Recorder(et.TrainableModel):
    def __init__(self, *args, **kwargs):
      made.append(self)
      super().__init__(*args, **kwargs)
  monkeypatch.setattr(et, 'TrainableModel', Recorder)
  base = ['--model_dir=%s' % (tmp_path / 'run'), '--data_dir=%s' % tmp_path, '--mode=train']
  with pytest.raises(ValueError, match=reason):
    main_lib.main(base + argv)
  assert not made and not os.path.exists(tmp_path / 'run')      # no model, so no engine; nothing written
  # the same command without what is refused gets as far as the model and stops at the data, still without an engine
  with pytest.raises(ValueError, match='matches no file'):
    main_lib.main(base + ['--hparam_str=' + OK_HPARAMS])
  assert len(made) == 1 and made[0].engine is None and os.path.exists(tmp_path / 'run' / 'config.yaml')
  with pytest.raises(ValueError, match='model_dir'):
    main_lib.main(['--mode=train'])


def test_ft_init_ckpt_leaves_the_classification_layer_alone(tmp_path):
  from automl_amd import tf_checkpoint, util_keras
  model = small()
  rng = np.random.default_rng(2)
  tensors = {p.name: rng.standard_normal(tuple(p.shape)).astype(np.float32) for p in model.spec.params}
  prefix = str(tmp_path / 'pretrained')
  tf_checkpoint.write_checkpoint(prefix, tensors)
  util_keras.restore_ckpt(main_lib._WithoutHead(model), prefix, ema_decay=0, skip_mismatch=True)
  head = sorted(n for n in tensors if '/head/dense/' in n)
  assert [n.rsplit('/', 1)[1] for n in head] == ['bias', 'kernel']
  assert sorted(model._init_params) == sorted(n for n in tensors if n not in head)      # kept until the first engine exists
  assert all(np.array_equal(model._init_params[n], tensors[n]) for n in model._init_params)


def test_configuration_assembly_for_v2_s(tmp_path):
  with open(FIXTURE) as f:
    golden = json.load(f)
  base = main_lib.base_config().as_dict()
  for section in ('train', 'eval', 'data'):
    assert base[section] == golden['base_config'][section], section
  # the one restated value that differs on purpose: the reference's default strategy is 'tpu' (hparams.py:311)
  assert golden['base_config']['runtime']['strategy'] == 'tpu' and base['runtime']['strategy'] is None
  assert {k: v for k, v in base['runtime'].items() if k != 'strategy'} == {k: v for k, v in golden['base_config']['runtime'].items() if k != 'strategy'}

  flags = main_lib.parse_flags(['--model_name=efficientnetv2-s', '--dataset_cfg=imagenet', '--model_dir=%s' % tmp_path,
                                '--hparam_str=train.batch_size=512,train.epochs=10'])
  config = main_lib.build_config(flags)
  assert config.model.model_name == 'efficientnetv2-s' and config.model.num_classes == config.data.num_classes == 1000
  assert config.train.isize == 300 and config.eval.isize == 384 and config.train.stages == 4 and config.data.ram == 10
  assert config.train.label_smoothing == 0.1 and config.train.lr_sched == 'exponential' and config.eval.batch_size == 8
  plan = main_lib.plan_of(config)
  assert plan['steps_per_epoch'] == 1256144 // 512 == 2453 and plan['total_steps'] == 24530
  assert plan['scaled_lr'] == 0.016 * (512 / 256.0) == 0.032 and plan['scaled_lr_min'] == 0
  assert plan['train_size'] == 300 and plan['eval_size'] == 384 and plan['validation_steps'] == 50000 // 8
  assert plan['stages'] == et.progressive_stages('efficientnetv2-s', 10)
  assert [s['image_size'] for s in plan['stages']] == [171, 214, 257, 300]
  # train_size from a fraction (main_tf2.py:161-162), num_images overridden, stages off
  config = main_lib.build_config(main_lib.parse_flags([
      '--model_name=efficientnetv2-s', '--hparam_str=train.isize=0.8,train.stages=0,data.splits.train.num_images=100,'
      'data.splits.minival.num_images=9,eval.split=minival,train.batch_size=8,eval.batch_size=4,train.lr_min=0.001']))
  plan = main_lib.plan_of(config)
  assert plan['train_size'] == int(384 * 0.8) // 16 * 16 == 304 and plan['steps_per_epoch'] == 12 and plan['validation_steps'] == 2
  assert plan['scaled_lr_min'] == 0.001 * (8 / 256.0) and len(plan['stages']) == 1 and plan['stages'][0]['image_size'] == 304
  with pytest.raises(ValueError, match='holds no batch'):
    main_lib.plan_of(main_lib.build_config(main_lib.parse_flags(['--model_name=efficientnetv2-s', '--hparam_str=data.splits.train.num_images=5'])))
  with pytest.raises(KeyError, match='no_such_key'):
    main_lib.build_config(main_lib.parse_flags(['--model_name=efficientnetv2-s', '--hparam_str=train.no_such_key=1']))
  # from the configuration to the model: the schedule, the loss and the input stage
  model = main_lib.build_model(flags, main_lib.build_config(flags), main_lib.plan_of(main_lib.build_config(flags)))
  assert model.engine is None and model.optimizer == 'rmsprop' and model.weight_decay == 1e-5 and model.label_smoothing == 0.1
  assert model.learning_rate.get_config() == dict(initial_lr=0.032, steps_per_epoch=2453, lr_decay_type='exponential', decay_factor=0.97,
                                                  decay_epochs=2.4, total_steps=24530, warmup_epochs=5, minimal_lr=0)
  assert (model.augname, model.ra_num_layers, model.ra_magnitude, model.image_size, model.eval_image_size) == ('randaug', 2, 10, 300, 384)
  assert model.ema_decay is None and model._dtype == 'bf16' and model.spec.num_classes == 1000
  # config.yaml is plain data
  import yaml
  path = main_lib.save_config(main_lib.build_config(flags), str(tmp_path / 'm'))
  loaded = yaml.safe_load(open(path))
  assert loaded['train']['batch_size'] == 512 and loaded['data']['splits']['train']['slice'] == [20, None]
  assert loaded['model']['blocks_args'][0]['kernel_size'] == 3 and loaded['runtime']['strategy'] is None
