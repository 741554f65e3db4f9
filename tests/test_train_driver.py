"""The detector training driver without a device: automl_amd/train.py's flags, arithmetic, config.yaml and refusals,
train_lib.get_callbacks, the training-state file (save_train_state / restore_train_state) on a hand-made state, and the lazy
batch logs of fit.  The runs themselves are in tests/test_train_driver_gpu.py."""
import json
import os
import zipfile

import numpy as np
import pytest

from automl_amd import _lib, dataloader, hparams_config, train, train_lib
from tests.test_dataloader import numbered, params as reader_params, take, write_shards

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_cases.npz')


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


# ------------------------------------------------------------------------------------------------------------ the flags
def test_flags_keep_the_reference_names_and_defaults():
  f = train.parse_flags([])
  want = dict(model_name='efficientdet-d0', model_dir=None, pretrained_ckpt=None, hparams='', batch_size=64, eval_samples=5000,
              train_file_pattern=None, val_file_pattern=None, val_json_file=None, mode='traineval', num_examples_per_epoch=120000,
              num_epochs=None, use_fake_data=False, debug=False, tf_random_seed=None, canvas=(640, 640), dtype='bf16',
              strategy='', steps_per_execution=1, use_xla=False, profile=False, hub_module_url=None, tpu=None)
  for k, v in want.items():
    assert getattr(f, k) == v, k
  f = train.parse_flags(['--use_fake_data', '--debug=true', '--mode=eval', '--canvas=480x640', '--dtype=f32', '--strategy=',
                         '--steps_per_execution=1', '--use_xla=false', '--tf_random_seed', '3'])
  assert f.use_fake_data is True and f.debug is True and f.mode == 'eval' and f.canvas == (480, 640) and f.dtype == 'f32'
  assert f.tf_random_seed == 3
  for bad in (['--mode=infer'], ['--canvas=640'], ['--dtype=fp8'], ['--debug=perhaps']):
    with pytest.raises(SystemExit):
      train.parse_flags(bad)


def test_flags_enter_the_config(tmp_path):
  f = train.parse_flags(['--model_name=efficientdet-d1', '--hparams=image_size=128,moving_average_decay=0,grid_mask=true',
                         '--num_epochs=7', '--batch_size=16', '--num_examples_per_epoch=1000', '--model_dir=%s' % tmp_path,
                         '--tf_random_seed=11', '--eval_samples=48', '--val_json_file=v.json'])
  c = train.build_config(f)
  assert c.name == 'efficientdet-d1' and c.backbone_name == 'efficientnet-b1' and c.image_size == 128 and c.grid_mask is True
  assert c.moving_average_decay == 0 and c.num_epochs == 7 and c.batch_size == 16 and c.steps_per_epoch == 62
  assert c.model_dir == str(tmp_path) and c.tf_random_seed == 11 and c.eval_samples == 48 and c.val_json_file == 'v.json'
  assert c.steps_per_execution == 1 and c.strategy == '' and c.num_shards == 1 and c.model_name == 'efficientdet-d1'
  # without --num_epochs the config's own 300 stays (tf2/train.py:157-158)
  assert train.build_config(train.parse_flags([])).num_epochs == 300
  with pytest.raises(KeyError, match='no_such_key'):
    train.build_config(train.parse_flags(['--hparams=no_such_key=1']))


def test_steps_per_epoch_and_initial_epoch():
  assert train.steps_per_epoch_of(train.parse_flags([])) == 120000 // 64 == 1875
  assert train.steps_per_epoch_of(train.parse_flags(['--num_examples_per_epoch=7', '--batch_size=2'])) == 3
  with pytest.raises(ValueError, match='holds no batch'):
    train.steps_per_epoch_of(train.parse_flags(['--num_examples_per_epoch=7', '--batch_size=8']))
  assert [train.initial_epoch_of(i, 3) for i in (0, 2, 3, 5, 6, 7)] == [0, 0, 1, 1, 2, 2]


def test_config_yaml_is_written_once(tmp_path):
  import yaml
  model_dir = tmp_path / 'run' / 'a'      # made on the way
  c = train.build_config(train.parse_flags(['--model_dir=%s' % model_dir, '--num_epochs=2']))
  path = train.init_experimental(c)
  assert path == str(model_dir / 'config.yaml')
  first = (model_dir / 'config.yaml').read_text()
  loaded = yaml.safe_load(first)
  assert loaded['num_epochs'] == 2 and loaded['name'] == 'efficientdet-d0' and loaded['nms_configs']['max_output_size'] == 100
  c2 = train.build_config(train.parse_flags(['--model_dir=%s' % model_dir, '--num_epochs=5']))
  train.init_experimental(c2)
  assert (model_dir / 'config.yaml').read_text() == first      # a continued run leaves the first run's record


def test_get_callbacks(tmp_path):
  p = hparams_config.get_efficientdet_config('efficientdet-d0').as_dict()
  p['model_dir'] = str(tmp_path)
  assert p['moving_average_decay'] and p['map_freq'] == 5 and p['save_freq'] == 'epoch'
  val = [object()]
  cbs = train_lib.get_callbacks(p, val)
  assert [type(c) for c in cbs] == [train_lib.ModelCheckpoint, train_lib.COCOCallback]
  assert cbs[0].filepath == os.path.join(str(tmp_path), 'emackpt-{epoch:d}') and cbs[0].filepath.format(epoch=3).endswith('emackpt-3')
  assert cbs[0].save_freq == 'epoch' and cbs[0].on_train_batch_end is None      # no batch-level work where none is asked for
  assert cbs[1].test_dataset is val and cbs[1].update_freq == 5
  assert [type(c) for c in train_lib.get_callbacks(p)] == [train_lib.ModelCheckpoint]
  assert [type(c) for c in train_lib.get_callbacks(dict(p, map_freq=0), val)] == [train_lib.ModelCheckpoint]
  assert [type(c) for c in train_lib.get_callbacks(dict(p, map_freq=None), val)] == [train_lib.ModelCheckpoint]
  plain = train_lib.get_callbacks(dict(p, moving_average_decay=0, save_freq=4), val)
  assert plain[0].filepath == os.path.join(str(tmp_path), 'ckpt-{epoch:d}') and plain[0].save_freq == 4
  assert callable(plain[0].on_train_batch_end) and len(plain) == 2
  with pytest.raises(ValueError, match='is not built'):
    train_lib.get_callbacks(dict(p, sample_image='x.jpg'))
  with pytest.raises(ValueError, match='save_freq'):
    train_lib.get_callbacks(dict(p, save_freq='batch'))
  assert train_lib.train_state_path('/a/ckpt-2') == '/a/ckpt-2.train_state.npz'


@pytest.mark.parametrize('flag, reason', [('--strategy=gpus', 'data-parallel fit is not built'), ('--strategy=tpu', 'strategy'),
                                          ('--tpu=grpc://1.2.3.4:8470', 'no TPU path'), ('--tpu_zone=z', 'no TPU path'),
                                          ('--gcp_project=p', 'no TPU path'), ('--hub_module_url=u', 'hub_module_url'),
                                          ('--use_xla', 'XLA'), ('--profile', 'profile'),
                                          ('--steps_per_execution=2', 'steps_per_execution=2')])
def test_what_is_not_built_is_refused_before_a_model_exists(flag, reason, tmp_path, monkeypatch):
  made = []

  class Recorder(train_lib.EfficientDetNetTrain):
    def __init__(self, *args, **kwargs):
      made.append(self)
      super().__init__(*args, **kwargs)
  monkeypatch.setattr(train_lib, 'EfficientDetNetTrain', Recorder)
  argv = ['--model_dir=%s' % tmp_path, '--mode=train', '--train_file_pattern=%s' % (tmp_path / 'none-*'), flag]
  with pytest.raises(ValueError, match=reason):
    train.main(argv)
  assert not made and not os.listdir(tmp_path)      # no model, so no engine; nothing written
  # the same command without the flag gets as far as the model and stops at the data, still without an engine
  with pytest.raises(ValueError, match='matches no file'):
    train.main(argv[:-1])
  assert len(made) == 1 and made[0].engine is None
  with pytest.raises(ValueError, match='model_dir'):
    train.main(['--mode=train'])


# ------------------------------------------------------------------------------------------------------ the state file
class HandMadeModel(object):
  """What save_train_state reads of a model: the config (for the variable list), the optimizer state, the engines."""

  class Eng(object):
    def __init__(self, state):
      self.state = state

    def drop_rng_state(self):
      return self.state

  def __init__(self, config, state, drop):
    self.config, self.state = config, state
    self._engines = {key: self.Eng(v) for key, v in drop.items()}

  def get_optimizer_state(self):
    return self.state


def hand_made_state(config, adam=False):
  n = train_lib.arena_length(HandMadeModel(config, None, {}))
  rng = np.random.default_rng(5)
  state = {'velocity': rng.standard_normal(n).astype(np.float32), 'ema': rng.standard_normal(n).astype(np.float32),
           'iterations': 7, 'moving_normalizer': float(np.float32(12.345678)),
           'input_rng_state': np.array([2**64 - 1, 2**63 + 5, 3, 2**64 - 2, 1, 2**32 - 1], np.uint64)}
  if adam:
    state['adam_v'] = rng.random(n).astype(np.float32)
  return state


def test_state_file_round_trip(lib, tmp_path):
  g = np.load(GOLDEN)
  sizes = [40, 30, 50]
  pattern = write_shards(tmp_path, numbered(g['s8x9_420_q75/bytes'].tobytes(), sizes))
  ir = dataloader.InputReader(pattern, is_training=True)
  reader = ir.host_reader(reader_params(), 8)
  take(reader, 5)
  reader_state = reader.get_state()      # mid-epoch: 64 records wait in the shuffle buffer, files are half read
  assert reader_state['live'] and len(reader_state['buffer']) == 64 and reader_state['rng']['state']['state'] >= 2**64
  rest = [b.index for b in take(reader, 6)]
  reader.close()

  class Held(object):
    def get_state(self):
      return reader_state
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  config.optimizer = 'adam'
  state = hand_made_state(config, adam=True)
  drop = {(2, 128, 128): np.arange(240, 256, dtype=np.uint8), (1, 128, 128): np.arange(16, dtype=np.uint8)}      # 128 bits each
  path = str(tmp_path / 'ckpt-3.train_state.npz')
  assert train_lib.save_train_state(HandMadeModel(config, state, drop), path, Held()) == path
  assert not os.path.exists(path + '.tmp')
  # arrays are npz members, everything else one JSON member; nothing in it is pickled
  with zipfile.ZipFile(path) as z:
    assert sorted(z.namelist()) == sorted(k + '.npy' for k in ('velocity', 'ema', 'adam_v', 'input_rng_state', 'meta',
                                                               'drop_rng.2x128x128', 'drop_rng.1x128x128'))
  with np.load(path, allow_pickle=False) as z:
    assert all(z[k].dtype != object for k in z.files)
    meta = json.loads(z['meta'].tobytes().decode('utf-8'))
  assert meta['iterations'] == 7 and meta['optimizer'] == 'adam' and meta['moving_normalizer'] == state['moving_normalizer']
  assert meta['arena_length'] == state['velocity'].size and meta['reader']['rng'] == reader_state['rng']
  # into a model that has no engine: kept until the first one is made, the step count at once
  net = train_lib.EfficientDetNetTrain(config=config)
  resumed = ir.host_reader(reader_params(tf_random_seed=999), 8)
  train_lib.restore_train_state(net, path, reader=resumed)
  assert net.engine is None and net.iterations == 7
  kept = net._pending_state
  assert sorted(kept) == sorted(state)
  for k, v in state.items():
    assert np.array_equal(np.asarray(kept[k]), np.asarray(v)) and np.asarray(kept[k]).dtype == np.asarray(v).dtype, k
  assert sorted(net._pending_drop_rng) == ['1x128x128', '2x128x128']
  assert np.array_equal(net._pending_drop_rng['2x128x128'], drop[(2, 128, 128)])
  assert [b.index for b in take(resumed, 6)] == rest      # the reader goes on where the saved one was
  resumed.close()
  # the reader's part is asked for and the file has none
  bare = str(tmp_path / 'bare.train_state.npz')
  train_lib.save_train_state(HandMadeModel(config, state, {}), bare)
  train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=config), bare)
  with pytest.raises(ValueError, match='holds no reader state'):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=config), bare, reader=resumed)


def test_state_of_another_model_is_refused(tmp_path):
  d0 = hparams_config.get_efficientdet_config('efficientdet-d0')
  path = str(tmp_path / 'ckpt-1.train_state.npz')
  train_lib.save_train_state(HandMadeModel(d0, hand_made_state(d0), {}), path)
  d1 = hparams_config.get_efficientdet_config('efficientdet-d1')
  n0, n1 = (len(hparams_config_variables(c)) for c in (d0, d1))
  assert n0 != n1
  with pytest.raises(ValueError, match=r'another model: the file has %d variables, this model %d; \d+ arena elements, this model \d+'
                     % (n0, n1)):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=d1), path)
  adam = hparams_config.get_efficientdet_config('efficientdet-d0')
  adam.optimizer = 'adam'
  with pytest.raises(ValueError, match='the file has sgd as optimizer, this model adam'):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=adam), path)
  # the same variable list with another head width: the count agrees, the arena does not
  wide = hparams_config.get_efficientdet_config('efficientdet-d0')
  wide.num_classes = 20
  with pytest.raises(ValueError, match='arena elements'):
    train_lib.restore_train_state(train_lib.EfficientDetNetTrain(config=wide), path)
  # a file that is not this format's
  other = str(tmp_path / 'other.npz')
  np.savez(other, meta=np.frombuffer(json.dumps({'format': 99}).encode(), np.uint8))
  with pytest.raises(ValueError, match='format 99'):
    train_lib.load_train_state(other)


def hparams_config_variables(config):
  from automl_amd import util_keras
  return util_keras.model_variables(HandMadeModel(config, None, {}))


# ------------------------------------------------------------------------------------------------------ the batch logs
def test_batch_logs_read_device_values_only_when_one_is_accessed():
  class Device(object):
    reads = 0

    def read(self):
      self.reads += 1
      return {k: float(i) for i, k in enumerate(train_lib.engine_lib.Engine.LOSS_KEYS)}
  dev = Device()
  logs = train_lib.LazyLogs({'learning_rate': 0.01, 'step': 4}, train_lib.engine_lib.Engine.LOSS_KEYS, dev.read)
  assert logs['learning_rate'] == 0.01 and logs['step'] == 4 and logs.get('step') == 4
  assert 'loss' in logs and 'AP' not in logs and len(logs) == 7
  assert sorted(logs) == sorted(('cls_loss', 'box_loss', 'det_loss', 'reg_l2_loss', 'loss', 'learning_rate', 'step'))
  assert logs.get('AP') is None
  with pytest.raises(KeyError):
    logs['AP']
  assert dev.reads == 0      # keys, membership and host values: nothing read
  assert logs['loss'] == 4.0 and dev.reads == 1
  assert logs['cls_loss'] == 0.0 and dict(logs)['det_loss'] == 2.0 and dev.reads == 1      # one read serves the batch


def test_history_is_a_dict_of_lists():
  h = train_lib.History()
  h.append(1, {'loss': 2.0, 'learning_rate': 0.1})
  h.append(2, {'loss': 1.5, 'learning_rate': 0.2, 'AP': 0.0})
  assert h.epoch == [1, 2] and h.history == {'loss': [2.0, 1.5], 'learning_rate': [0.1, 0.2], 'AP': [0.0]}


def test_data_parallel_fit_is_refused_before_the_device():
  net = train_lib.EfficientDetNetTrain(config=hparams_config.get_efficientdet_config('efficientdet-d0'), use_dist=True)
  with pytest.raises(ValueError, match='data-parallel fit is not built'):
    net.fit(iter(()))
  assert net.engine is None
