"""automl_amd/effnetv2_datasets.py without a device: the split table and the dataset configurations against the fixture
tests/golden/reference_v2_driver.json (made by tests/golden/make_golden_v2_driver.py, which executes the reference's hparams.py
and datasets.py), the slicing of the file list, everything that is refused, label - 1 and the labels that raise, and the host
reader's order, sharding, drop_remainder, single evaluation pass and mid-epoch resume against the restatement
tests/v2_datasets_ref.py.  The decoder's refusals are checked with the device stage replaced by a host stand-in that runs the
real Huffman stage (jpeg.entropy_decode) and raises as jpeg.JpegDecoder.decode does."""
import json
import os

import numpy as np
import pytest

from automl_amd import _lib, effnetv2_datasets as ds, jpeg, tfrecord
from tests import v2_datasets_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'reference_v2_driver.json')
CLASSES = 24
SEED = 7
TRAIN_SIZES = [3, 5, 2, 4, 6, 1, 3, 5, 4, 2, 3, 6, 5, 4, 3, 2, 1, 4, 5, 3, 7, 5, 6, 4, 9]      # 25 files: train = [20:]
VAL_SIZES = [5, 4, 6]


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


@pytest.fixture(scope='module')
def golden():
  with open(FIXTURE) as f:
    return json.load(f)


@pytest.fixture(scope='module')
def data(lib, tmp_path_factory):
  folder = tmp_path_factory.mktemp('imagenet')
  content = ref.write_shards(folder, ref.load_jpegs(), TRAIN_SIZES, VAL_SIZES, CLASSES, tfrecord.TFRecordWriter, tfrecord.encode_example)
  return str(folder), content


def cfg(**kw):
  c = {'num_classes': CLASSES}
  c.update(kw)
  return c


def take(reader, n):
  out = []
  for batch in reader:
    out.append(batch)
    if len(out) == n:
      break
  return out


def named(reader, batches):
  return [[(os.path.basename(reader.files[f]), r) for f, r in b.index] for b in batches]


def want(names, sizes_of, batch, training, seed, epochs, **kw):
  sizes = [sizes_of[n] for n in names]
  return [[(names[f], r) for f, r in b] for b in ref.batches(sizes, batch, training, seed, epochs, **kw)]


def test_tables_equal_the_reference(golden):
  assert ds.ImageNetInput.cfg.as_dict() == golden['imagenet_input']
  assert ds.ImageNetInput.cfg.num_classes == 1000 and sorted(ds.ImageNetInput.cfg.splits.keys()) == ['eval', 'minival', 'train', 'trainval']
  assert ds.get_dataset_config('imagenet').as_dict() == golden['dataset_configs']['imagenet']
  assert ds.get_dataset_config('Imagenet').as_dict() == golden['dataset_configs']['imagenet']      # the flag's default spelling
  got, expect = ds.get_dataset_config('imagenetft').as_dict(), golden['dataset_configs']['imagenetft']
  assert sorted(got) == sorted(expect) == ['data', 'model', 'train']
  assert got['model'] == expect['model'] and got['train'] == expect['train']
  # the deliberate difference: the reference's recipe reads 'imagenettfds' through tfds, this one the ImageNet TFRecords
  assert expect['data']['ds_name'] == 'imagenettfds' and got['data']['ds_name'] == 'imagenet'
  for key in ('augname', 'mixup_alpha', 'cutmix_alpha', 'num_classes', 'multiclass'):
    assert got['data'][key] == expect['data'][key], key
  assert got['data']['splits'] == golden['imagenet_input']['splits']
  assert ds.get_dataset_class('imagenet') is ds.ImageNetInput and ds.get_dataset_class('imagenetft') is ds.ImageNetInput


def test_what_is_not_built_raises_with_its_reason(golden, tmp_path):
  assert sorted(list(golden['unbuilt']) + ['imagenet']) == golden['dataset_classes']      # every other class of the reference
  for name, table in golden['unbuilt'].items():
    with pytest.raises(ValueError, match='is not built: ') as e:
      ds.get_dataset_class(name)
    # the reason is the sigmoid loss for the multiclass table and tfds for every table that names a tfds data set
    assert ('sigmoid' in str(e.value)) == bool(table['multiclass']) and ('tensorflow_datasets' in str(e.value)) == bool(table['tfds_name'])
    with pytest.raises(ValueError, match='is not built: '):
      ds.build_dataset_input(True, 224, None, str(tmp_path), 'train', {'ds_name': name})
  for name in ('imagenet21k', 'cifar10ft', 'cifar100ft', 'flowersft', 'tfflowersft', 'carsft'):
    with pytest.raises(ValueError, match='is not built: '):
      ds.get_dataset_config(name)
  with pytest.raises(ValueError, match='not registered'):
    ds.get_dataset_config('mnist')
  for null in (None, '', 'null'):
    with pytest.raises(ValueError, match='is not built.*all-zero'):
      ds.ImageNetInput(True, null)
    with pytest.raises(ValueError, match='is not built'):
      ds.build_dataset_input(True, 224, None, null, None, ds.get_dataset_config('imagenet').data)


def test_split_defaults_and_slicing(lib, data, tmp_path):
  folder, content = data
  assert ds.ImageNetInput(True, folder).split == 'train' and ds.ImageNetInput(False, folder).split == 'eval'
  assert ds.ImageNetInput(True, folder).num_images == 1256144 and ds.ImageNetInput(False, folder, 'minival').num_images == 25021
  for split in ('train', 'minival', 'eval', 'trainval'):
    got = ds.ImageNetInput(True, folder, split).files()
    assert [os.path.basename(f) for f in got] == ref.split_files(content, split), split
  assert len(ds.ImageNetInput(True, folder).files()) == 5 and len(ds.ImageNetInput(True, folder, 'minival').files()) == 20
  assert [os.path.basename(f) for f in ds.ImageNetInput(True, folder).files(shard=(2, 1))] == ref.split_files(content, 'train', (2, 1))
  with pytest.raises(ValueError, match='shard'):
    ds.ImageNetInput(True, folder).files(shard=(8, 6))
  # Python's own slicing: 20 files leave 'train' empty, and an empty list raises; so does a pattern that matches nothing
  few = tmp_path / 'few'
  few.mkdir()
  ref.write_shards(few, ref.load_jpegs(), [1] * 20, [], CLASSES, tfrecord.TFRecordWriter, tfrecord.encode_example)
  assert len(ds.ImageNetInput(True, str(few), 'minival').files()) == 20 and len(ds.ImageNetInput(True, str(few), 'trainval').files()) == 20
  with pytest.raises(ValueError, match='none is left'):
    ds.ImageNetInput(True, str(few)).files()
  with pytest.raises(ValueError, match='matches no file'):
    ds.ImageNetInput(False, str(few)).files()
  with pytest.raises(ValueError, match='split'):
    ds.ImageNetInput(True, folder, 'test')
  # a data section handed in (build_dataset_input) replaces the table's entries
  inp = ds.build_dataset_input(True, 224, None, folder, 'train', {'ds_name': 'imagenet', 'num_classes': CLASSES,
                                                                   'splits': {'train': {'num_images': 31}}})
  assert inp.num_classes == CLASSES and inp.num_images == 31 and inp.split_info['files'] == 'train*' and inp.split_info['slice'] == [20, None]


def test_labels_and_images(lib, data):
  folder, content = data
  reader = ds.ImageNetInput(False, folder, cfg=cfg()).host_reader(4)
  got = list(reader)
  names = ref.split_files(content, 'eval')
  assert named(reader, got) == want(names, {n: len(content[n]) for n in names}, 4, False, None, 1) and len(got) == 3
  for b in got:
    assert b.labels.dtype == np.int32 and b.labels.shape == (4,)
    for (f, r), image, label in zip(b.index, b.images, b.labels):
      record = bytes(tfrecord.TFRecordFile(reader.files[f])[r])
      assert isinstance(image, memoryview) and bytes(image) == ref.image_of(record) == content[os.path.basename(reader.files[f])][r][0]
      assert int(label) == ref.class_id(record, CLASSES) == content[os.path.basename(reader.files[f])][r][1]


@pytest.mark.parametrize('label, what', [(None, "no 'image/class/label'"), (0, 'outside 1 .. 24'), (CLASSES + 1, 'outside 1 .. 24')])
def test_a_label_the_reference_would_zero_raises(lib, tmp_path, label, what):
  jpegs = ref.load_jpegs()
  path = tmp_path / 'val-00000-of-00001'
  good = tfrecord.encode_example({'image/encoded': jpegs[1], 'image/class/label': [3]})
  feats = {'image/encoded': jpegs[2]}
  if label is not None:
    feats['image/class/label'] = [label]
  with tfrecord.TFRecordWriter(path) as w:
    for r in (good, good, tfrecord.encode_example(feats), good):
      w.write(r)
  with pytest.raises(ValueError):
    ref.class_id(tfrecord.encode_example(feats), CLASSES)
  assert ref.class_id(good, CLASSES) == 2
  reader = ds.ImageNetInput(False, str(tmp_path), cfg=cfg()).host_reader(4)
  with pytest.raises(tfrecord.TFRecordError, match=what) as e:
    next(reader)
  offset = tfrecord.TFRecordFile(str(path)).offset(2)
  assert e.value.path == str(path) and e.value.record == 2 and e.value.offset == offset
  assert str(path) in str(e.value) and 'record 2 at byte offset %d' % offset in str(e.value)
  # the largest label is fine
  with tfrecord.TFRecordWriter(path) as w:
    w.write(tfrecord.encode_example({'image/encoded': jpegs[1], 'image/class/label': [CLASSES]}))
  assert next(ds.ImageNetInput(False, str(tmp_path), cfg=cfg()).host_reader(1)).labels.tolist() == [CLASSES - 1]


def test_order_sharding_and_resume(lib, data):
  folder, content = data
  sizes_of = {n: len(rows) for n, rows in content.items()}
  # training on 'trainval' (25 files: more than the 16 open ones, 98 records: more than the shuffle buffer), two epochs
  names = ref.split_files(content, 'trainval')
  expect = want(names, sizes_of, 4, True, SEED, 2)
  assert len(expect) == 2 * (sum(TRAIN_SIZES) // 4) and sum(TRAIN_SIZES) % 4      # a remainder is dropped in each epoch
  reader = ds.ImageNetInput(True, folder, 'trainval', seed=SEED, cfg=cfg()).host_reader(4)
  got = take(reader, len(expect) + 1)      # it goes on into a third epoch
  assert named(reader, got[:-1]) == expect
  first = [p for b in expect[:len(expect) // 2] for p in b]
  assert len(set(first)) == len(first) and expect[:len(expect) // 2] != expect[len(expect) // 2:]
  assert expect[0] != want(names, sizes_of, 4, False, None, 1)[0]
  reader.close()
  other = ds.ImageNetInput(True, folder, 'trainval', seed=SEED + 1, cfg=cfg()).host_reader(4)
  assert named(other, take(other, 3)) != expect[:3]
  other.close()
  # the 'train' split is files [20:], and shard=(2, 1) every second of those
  for shard in (None, (2, 1)):
    names = ref.split_files(content, 'train', shard)
    reader = ds.ImageNetInput(True, folder, seed=SEED, cfg=cfg()).host_reader(3, shard=shard, threads=2)
    expect = want(names, sizes_of, 3, True, SEED, 2)
    assert named(reader, take(reader, len(expect))) == expect
    reader.close()
  # evaluation, and debug=True: file order, one pass, the remainder dropped
  names = ref.split_files(content, 'eval')
  for batch, count in ((4, 3), (7, 2), (16, 0)):
    reader = ds.ImageNetInput(False, folder, cfg=cfg()).host_reader(batch)
    got = list(reader)
    assert named(reader, got) == want(names, sizes_of, batch, False, None, 1) and len(got) == count
  assert want(names, sizes_of, 4, False, None, 1)[0] == [(names[0], 0), (names[1], 0), (names[2], 0), (names[0], 1)]      # by hand
  names = ref.split_files(content, 'minival')
  reader = ds.ImageNetInput(True, folder, 'minival', debug=True, seed=SEED, cfg=cfg()).host_reader(4)
  got = list(reader)
  assert named(reader, got) == want(names, sizes_of, 4, False, None, 1) and len(got) == sum(TRAIN_SIZES[:20]) // 4
  # a state taken in the middle of an epoch and put into a fresh reader goes on with the same stream
  names = ref.split_files(content, 'trainval')
  expect = want(names, sizes_of, 4, True, SEED, 2)
  reader = ds.ImageNetInput(True, folder, 'trainval', seed=SEED, cfg=cfg()).host_reader(4, depth=3)
  take(reader, 7)
  state = json.loads(json.dumps(reader.get_state()))      # as the training-state file stores it
  reader.close()
  fresh = ds.ImageNetInput(True, folder, 'trainval', seed=SEED + 5, cfg=cfg()).host_reader(4)
  fresh.set_state(state)
  got = take(fresh, len(expect) - 7)
  assert named(fresh, got) == expect[7:]
  for b in got[:3]:
    for (f, r), label in zip(b.index, b.labels):
      assert int(label) == content[os.path.basename(fresh.files[f])][r][1]
  fresh.close()


class HostDecoder(object):
  """jpeg.JpegDecoder with the device stage left out: the real Huffman stage on host arrays, and JpegDecoder.decode's
  handling of a refused stream."""

  def __init__(self, batch, canvas_h, canvas_w, depth=2, threads=None):
    self.batch, self.hc, self.wc, self.threads = batch, canvas_h, canvas_w, threads or min(16, batch)

  def decode(self, contents, fallback=None):
    b = self.batch
    coef = np.zeros(b * jpeg.worst_blocks(self.hc, self.wc) * 64, np.int16)
    images, qtables, status = np.zeros(b * jpeg.IMAGE_BYTES, np.uint8), np.zeros((b, 4, 64), np.uint16), np.zeros(b, np.int32)
    jpeg.entropy_decode(contents, self.hc, self.wc, coef, images, qtables, status, self.threads)
    sizes = np.zeros((b, 2), np.int32)
    for i, d in enumerate(jpeg.descriptors(images, b)):
      if d.status and fallback is None:
        raise ValueError('contents[%d] is not decoded: %s (status %d)' % (i, jpeg.REASONS.get(int(d.status), '?'), d.status))
      sizes[i] = fallback(contents[i]).shape[:2] if d.status else (d.height, d.width)
    return None, sizes


@pytest.mark.parametrize('case, reason', [('s24x280_420_q75', jpeg.REASONS[jpeg.TOO_LARGE]), ('big_480x640_420', jpeg.REASONS[jpeg.TOO_LARGE]),
                                          ('progressive_17x33', jpeg.REASONS[jpeg.PROGRESSIVE]), ('cmyk_16x16', jpeg.REASONS[jpeg.COMPONENTS])])
def test_what_the_decoder_refuses_names_the_record(lib, tmp_path, monkeypatch, case, reason):
  jpegs = ref.load_jpegs()
  bad = ref.load_jpegs((case,))[0]
  for f in range(2):
    with tfrecord.TFRecordWriter(tmp_path / ('val-%05d-of-00002' % f)) as w:
      for r in range(4):
        w.write(tfrecord.encode_example({'image/encoded': bad if (f, r) == (1, 2) else jpegs[r + 1], 'image/class/label': [r + 1]}))
  monkeypatch.setattr(jpeg, 'JpegDecoder', HostDecoder)
  reader = ds.ImageNetInput(False, str(tmp_path), cfg=cfg())(4, canvas=(56, 56))
  (_, sizes), labels = next(reader)      # (0, 0), (1, 0), (0, 1), (1, 1)
  assert labels.tolist() == [0, 0, 1, 1] and sizes.tolist()[0] == sizes.tolist()[1]
  with pytest.raises(ValueError) as e:      # (0, 2), (1, 2), (0, 3), (1, 3)
    next(reader)
  assert reason in str(e.value) and '%s record 2: contents[1]' % (tmp_path / 'val-00001-of-00002') in str(e.value)
  reader.close()
  # with a fallback the status passes through: the slot is the fallback's
  reader = ds.ImageNetInput(False, str(tmp_path), cfg=cfg())(4, canvas=(56, 56), fallback=lambda data: np.zeros((5, 6, 3), np.uint8))
  next(reader)
  (_, sizes), _ = next(reader)
  assert sizes[1].tolist() == [5, 6]
  reader.close()
  with pytest.raises(ValueError, match='canvas'):
    ds.ImageNetInput(False, str(tmp_path), cfg=cfg())(4)
