"""reader(decode_crop=True) of the ImageNet reader and --decode_crop of the classifier's CLI, without a device
(automl_amd/effnetv2_datasets.py, effnetv2_main.py): on a tiny shard written with tfrecord.TFRecordWriter the windows equal a
restated draw sequence -- a PCG64 stream derived from the seed, one sample_distorted_bounding_box per readable header, in batch
order -- and the records are those of the reader without decode_crop; get_state() taken mid-epoch and given to a new reader
reproduces the following batches' windows and records; the state-key mismatches raise and name the key; evaluation refuses
decode_crop; with max_ratio the ratio and the covering window are choose_window_ratio's; and the flag reaches the reader and the
model."""
import os

import numpy as np
import pytest

from automl_amd import _lib, effnetv2_datasets as ds, effnetv2_main as main_lib, jpeg, tfrecord, v2_preprocessing as vp
from tests import jpeg_ref as jr
from tests import v2_datasets_ref as ref

SEED, BATCH, CLASSES = 5, 4, 24
CFG = {'num_classes': CLASSES, 'splits': {'train': {'num_images': 22, 'files': 'train*', 'slice': [0, None]}}}
JUNK = (1, 3)      # (file, record) whose image is not a JPEG stream


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


@pytest.fixture(scope='module')
def shard(tmp_path_factory, lib):
  """Two training files of 11 records over the reference's fixture images, one record with bytes that are no JPEG."""
  folder = tmp_path_factory.mktemp('imagenet')
  jpegs = ref.load_jpegs()
  for f in range(2):
    with tfrecord.TFRecordWriter(folder / ('train-%05d-of-00002' % f)) as w:
      for r in range(11):
        image = b'junk, not a stream' if (f, r) == JUNK else jpegs[(3 * f + r) % len(jpegs)]
        w.write(tfrecord.encode_example({'image/encoded': image, 'image/class/label': [(f * 11 + r) % CLASSES + 1]}))
  return str(folder)


def _input(shard, is_training=True, seed=SEED):
  return ds.ImageNetInput(is_training, shard, seed=seed, cfg=CFG)


def _restated_rng(seed):
  return np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(0x77696E646F77,))))


def _restate(batches, rng):
  """The windows and header sizes of HostBatches, drawn again: one draw per readable header, in order."""
  out = []
  for hb in batches:
    windows, sizes = np.zeros((len(hb.images), 4), np.int32), np.zeros((len(hb.images), 2), np.int32)
    for i, image in enumerate(hb.images):
      try:
        fr = jr.info(bytes(image))
      except jr.Refused:
        continue
      sizes[i] = (fr.height, fr.width)
      windows[i] = vp.sample_distorted_bounding_box(rng, fr.height, fr.width)
    out.append((windows, sizes))
  return out


def test_windows_equal_a_restated_draw_sequence_and_the_records_do_not_change(shard):
  crop = _input(shard).host_reader(BATCH, decode_crop=True)
  plain = _input(shard).host_reader(BATCH)
  got = [next(crop) for _ in range(7)]      # past the end of the first epoch (22 records, 5 batches)
  want = [next(plain) for _ in range(7)]
  crop.close()
  plain.close()
  junk = 0
  for a, b, (windows, sizes) in zip(got, want, _restate(got, _restated_rng(SEED))):
    assert a.index == b.index and np.array_equal(a.labels, b.labels) and b.windows is None and b.image_sizes is None
    assert [bytes(x) for x in a.images] == [bytes(x) for x in b.images]
    assert a.windows.dtype == np.int32 and np.array_equal(a.windows, windows) and np.array_equal(a.image_sizes, sizes)
    for i, pair in enumerate(a.index):
      y, x, h, w = a.windows[i]
      if tuple(pair) == JUNK:      # no draw: the decoder is to say what is wrong with it
        junk += 1
        assert not a.windows[i].any() and not a.image_sizes[i].any()
      else:
        assert 0 <= y and 0 <= x and h >= 1 and w >= 1 and y + h <= sizes[i, 0] and x + w <= sizes[i, 1]
    # the order's part of the state is the plain reader's; the generator's travels under its own key
    assert ds.WINDOW_KEY == 'window_rng' and ds.WINDOW_KEY in a.state and ds.WINDOW_KEY not in b.state
    assert {k: v for k, v in a.state.items() if k != ds.WINDOW_KEY}.keys() == b.state.keys()
    assert repr({k: v for k, v in a.state.items() if k != ds.WINDOW_KEY}) == repr(b.state)
  assert junk >= 1
  assert len({tuple(w) for hb in got for w in hb.windows}) > 20      # the windows differ from image to image and epoch to epoch
  # another seed: other windows
  other = _input(shard, seed=SEED + 1).host_reader(BATCH, decode_crop=True)
  assert not np.array_equal(np.concatenate([next(other).windows for _ in range(3)]), np.concatenate([hb.windows for hb in got[:3]]))
  other.close()


def test_resume_mid_epoch_reproduces_windows_and_records(shard):
  first = _input(shard).host_reader(BATCH, decode_crop=True)
  next(first)
  next(first)
  state = first.get_state()
  want = [next(first) for _ in range(5)]
  first.close()
  again = _input(shard, seed=SEED + 17).host_reader(BATCH, decode_crop=True)      # (the state carries both generators)
  again.set_state(state)
  got = [next(again) for _ in range(5)]
  assert again.get_state()[ds.WINDOW_KEY] == want[-1].state[ds.WINDOW_KEY]
  again.close()
  for a, b in zip(got, want):
    assert a.index == b.index and np.array_equal(a.windows, b.windows) and np.array_equal(a.labels, b.labels)
    assert np.array_equal(a.image_sizes, b.image_sizes)


def test_state_key_mismatches_raise_and_name_the_key(shard):
  crop = _input(shard).host_reader(BATCH, decode_crop=True)
  plain = _input(shard).host_reader(BATCH)
  with pytest.raises(ValueError, match="no key 'window_rng'.*with decode_crop"):
    crop.set_state(plain.get_state())
  with pytest.raises(ValueError, match="the key 'window_rng'.*without decode_crop"):
    plain.set_state(crop.get_state())
  plain.set_state(plain.get_state())
  crop.set_state(crop.get_state())
  crop.close()
  plain.close()


def test_evaluation_refuses_decode_crop(shard, tmp_path):
  with tfrecord.TFRecordWriter(tmp_path / 'val-00000-of-00001') as w:
    w.write(tfrecord.encode_example({'image/encoded': ref.load_jpegs()[0], 'image/class/label': [1]}))
  ev = ds.ImageNetInput(False, str(tmp_path), seed=SEED, cfg={'num_classes': CLASSES})
  with pytest.raises(ValueError, match='decode_crop is for training'):
    ev.reader(1, canvas=(64, 64), decode_crop=True)
  with pytest.raises(ValueError, match='decode_crop is for training'):
    ev.host_reader(1, decode_crop=True)
  ev.reader(1, canvas=(64, 64)).close()


class HostDecoder(object):
  """jpeg.JpegDecoder with the device stage left out: the window host stage alone; it records how it was built and called."""
  built, calls = [], []

  def __init__(self, batch, canvas_h, canvas_w, depth=2, threads=None, max_ratio=1, windowed=False):
    self.batch, self.hc, self.wc, self.threads, self.max_ratio = batch, canvas_h, canvas_w, threads or min(16, batch), max_ratio
    HostDecoder.built.append((max_ratio, windowed))

  def decode(self, contents, fallback=None, windows=None, ratios=None):
    b = self.batch
    HostDecoder.calls.append((np.array(windows), None if ratios is None else list(ratios)))
    coef = np.zeros(64 * 8192, np.int16)
    images, wins = np.zeros(b * jpeg.IMAGE_BYTES, np.uint8), np.zeros(b * jpeg.WINDOW_BYTES, np.uint8)
    qtables, status = np.zeros((b, 4, 64), np.uint16), np.zeros(b, np.int32)
    jpeg.entropy_decode_window(contents, self.hc, self.wc, self.max_ratio, ratios, windows, coef, images, wins, qtables, status,
                               self.threads)
    sizes = np.zeros((b, 2), np.int32)
    for i, (d, w) in enumerate(zip(jpeg.descriptors(images, b), jpeg.window_descriptors(wins, b))):
      if d.status and fallback is None:
        raise ValueError('contents[%d] is not decoded: %s (status %d)' % (i, jpeg.REASONS.get(int(d.status), '?'), d.status))
      sizes[i] = (1, 1) if d.status else (w.h, w.w)
    return None, sizes


def test_the_device_reader_hands_the_decoder_windows_and_ratios(shard, monkeypatch):
  monkeypatch.setattr(jpeg, 'JpegDecoder', HostDecoder)
  host = _input(shard).host_reader(BATCH, decode_crop=True)
  batches = [next(host) for _ in range(4)]
  host.close()
  # a canvas every window fits: ratio 1, the windows as they were drawn, `sizes` the window sizes
  HostDecoder.built, HostDecoder.calls = [], []
  reader = _input(shard).reader(BATCH, canvas=(64, 288), decode_crop=True, fallback=lambda data: np.zeros((1, 1, 3), np.uint8))
  for hb in batches:
    (_, sizes), labels = next(reader)
    windows, ratios = HostDecoder.calls[-1]
    assert ratios is None and np.array_equal(labels, hb.labels)
    for i, pair in enumerate(hb.index):
      if tuple(pair) == JUNK:
        assert windows[i].tolist() == [0, 0, 1, 1] and sizes[i].tolist() == [1, 1]      # (the fallback's image)
      else:
        assert np.array_equal(windows[i], hb.windows[i]) and np.array_equal(sizes[i], hb.windows[i, 2:])
  assert HostDecoder.built == [(1, True)]
  assert reader.get_state()[ds.WINDOW_KEY] == batches[-1].state[ds.WINDOW_KEY]
  reader.close()
  # a small canvas and max_ratio=8: per image the smallest ratio whose covering window fits, else max_ratio (TOO_LARGE)
  HostDecoder.built, HostDecoder.calls = [], []
  canvas = (6, 9)
  reader = _input(shard).reader(BATCH, canvas=canvas, decode_crop=True, max_ratio=8, fallback=lambda data: np.zeros((1, 1, 3), np.uint8))
  seen = set()
  for hb in batches:
    (_, sizes), _ = next(reader)
    windows, ratios = HostDecoder.calls[-1]
    for i, pair in enumerate(hb.index):
      if tuple(pair) == JUNK:
        assert ratios[i] == 1 and windows[i].tolist() == [0, 0, 1, 1]
        continue
      h, w = hb.image_sizes[i]
      want = jpeg.choose_window_ratio(hb.windows[i], h, w, canvas[0], canvas[1], 8)
      if want is None:
        want = (8, jpeg.covering_window(hb.windows[i], 8))
        assert sizes[i].tolist() == [1, 1]      # the decoder's TOO_LARGE went to the fallback
      else:
        assert sizes[i].tolist() == list(want[1][2:])
      seen.add(want[0])
      assert ratios[i] == want[0] and tuple(windows[i]) == tuple(want[1])
  assert HostDecoder.built == [(8, True)] and len(seen) >= 3, seen
  reader.close()
  # without a fallback the refused record is named
  reader = _input(shard).reader(BATCH, canvas=(64, 288), decode_crop=True)
  with pytest.raises(ValueError, match=r'train-00001-of-00002 record 3: contents\[\d\] is not decoded: a malformed'):
    for _ in range(6):
      next(reader)
  reader.close()


def test_the_cli_flag_reaches_the_reader_and_the_model(monkeypatch):
  assert main_lib.parse_flags([]).decode_crop is False and main_lib.parse_flags(['--decode_crop']).decode_crop is True
  calls = []

  class Input(object):
    def __call__(self, batch, **kw):
      calls.append((batch, kw))
      return 'reader'

  monkeypatch.setattr(ds, 'build_dataset_input', lambda *a, **kw: Input())
  config = main_lib.build_config(main_lib.parse_flags(['--hparam_str=data.augname=randaug']))
  plan = {'train_split': 'train', 'eval_split': 'eval'}
  flags = main_lib.parse_flags(['--decode_crop', '--canvas=56x64', '--data_dir=/nowhere'])
  assert main_lib.get_dataset(flags, config, plan, True) == 'reader'
  assert main_lib.get_dataset(flags, config, plan, False) == 'reader'      # evaluation: no decode_crop
  assert calls == [(config.train.batch_size, {'canvas': (56, 64), 'max_ratio': 1, 'decode_crop': True}),
                   (config.eval.batch_size, {'canvas': (56, 64), 'max_ratio': 1})]
  # the model: transformations='flip' with the flag, the default without
  from automl_amd import effnetv2_train
  made = []
  monkeypatch.setattr(effnetv2_train, 'TrainableModel', lambda *a, **kw: made.append(kw) or 'model')
  monkeypatch.setattr(effnetv2_train, 'WarmupLearningRateSchedule', lambda *a, **kw: 'schedule')
  full = {'scaled_lr': 0.1, 'steps_per_epoch': 10, 'total_steps': 100, 'scaled_lr_min': 0.0, 'train_size': 32, 'eval_size': 32}
  for argv, want in ((['--decode_crop'], 'flip'), ([], None)):
    made.clear()
    flags = main_lib.parse_flags(argv + ['--data_dir=/nowhere'])
    assert main_lib.build_model(flags, config, full) == 'model'
    assert made[0].get('transformations') == want, argv
