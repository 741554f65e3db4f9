"""dataloader.InputReader (automl_amd/dataloader.py): TFRecord shards -> the raw batches of train_step_raw / test_step_raw.

Without a device: the (file, record) order of the host half against the restatement tests/tfrecord_ref.py -- evaluation, two
training epochs at a seed, a data set larger than the shuffle buffer, sharding, a state saved in the middle of an epoch and
put into a fresh reader, use_fake_data --, the padded arrays against the restatement's, and everything that is refused.

On the device (marked gpu): the reader's batches equal the tuples built by hand from JpegDecoder.decode of the same bytes
and the restatement's arrays, bit for bit; test_step_raw and train_step_raw fed by the reader equal the same steps fed by
hand; and five batches iterated without a synchronisation in between equal the same five with one after each.  The images are
the small cases of tests/golden/jpeg_cases.npz."""
import gzip
import os

import numpy as np
import pytest
import torch

from automl_amd import _lib, dataloader, hparams_config, tfrecord
from tests import tfrecord_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
IMAGES = ('s8x9_420_q75', 's16x16_444_q75', 's17x33_422_q75', 's31x22_420_q75', 's37x53_444_q75', 'grey_16x16_q75')
CANVAS = (64, 64)
SEED = 13


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


@pytest.fixture(scope='module')
def jpegs():
  g = np.load(GOLDEN)
  return [g[n + '/bytes'].tobytes() for n in IMAGES]


def params(**kw):
  p = hparams_config.get_efficientdet_config('efficientdet-d0').as_dict()
  p.update(tf_random_seed=SEED, batch_size=4)
  p.update(kw)
  return p


def record(jpeg, k, boxes, crowd=None, area=None, source_id=None, stored_size=None):
  """One detection Example: `boxes` rows drawn from a generator seeded by k."""
  rng = np.random.default_rng(1000 + k)
  lo = (rng.random((boxes, 2)) * 0.5).astype(np.float32)
  hi = lo + (0.2 + rng.random((boxes, 2)) * 0.3).astype(np.float32)
  feats = {'image/encoded': jpeg, 'image/object/bbox/ymin': lo[:, 0], 'image/object/bbox/xmin': lo[:, 1],
           'image/object/bbox/ymax': hi[:, 0], 'image/object/bbox/xmax': hi[:, 1],
           'image/object/class/label': rng.integers(1, 91, boxes)}
  if crowd is not None:
    feats['image/object/is_crowd'] = crowd
  if area is not None:
    feats['image/object/area'] = np.asarray(area, np.float32)
  if source_id is not None:
    feats['image/source_id'] = source_id
  if stored_size is not None:
    feats['image/height'], feats['image/width'] = stored_size
  return tfrecord.encode_example(feats)


def write_shards(folder, shards, name='part'):
  """shards: lists of records -> the files part-00000.tfrecord ... in `folder`; returns the pattern."""
  for i, records in enumerate(shards):
    with tfrecord.TFRecordWriter(folder / ('%s-%05d.tfrecord' % (name, i))) as w:
      for r in records:
        w.write(r)
  return str(folder / (name + '-*.tfrecord'))


def numbered(jpeg, sizes):
  """Shards of `sizes` records whose source id is 1000 file + record, with (file + record) % 4 boxes."""
  return [[record(jpeg, 100 * f + r, (f + r) % 4, source_id=str(1000 * f + r), crowd=[(f + r + i) % 2 for i in range((f + r) % 4)])
           for r in range(n)] for f, n in enumerate(sizes)]


def take(reader, n):
  out = []
  for batch in reader:
    out.append(batch)
    if len(out) == n:
      break
  return out


def check_content(batch, shards, is_training, skip_crowd=True):
  decoded = [ref.decode(shards[f][r]) for f, r in batch.index]
  want = ref.pad_batch(decoded, is_training, skip_crowd)
  got = (batch.boxes, batch.classes, batch.counts, batch.is_crowds, batch.areas, batch.source_ids)
  for g, w, name in zip(got, want, ('boxes', 'classes', 'counts', 'is_crowds', 'areas', 'source_ids')):
    if is_training and name in ('is_crowds', 'areas', 'source_ids'):
      continue
    assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), name
  assert [bytes(v) for v in batch.images] == [d['image'] for d in decoded]
  if not is_training:
    assert batch.source_ids.tolist() == [float(1000 * f + r) for f, r in batch.index]


def test_order_of_three_shards(lib, jpegs, tmp_path):
  sizes = [5, 1, 9]
  shards = numbered(jpegs[0], sizes)
  pattern = write_shards(tmp_path, shards)
  # evaluation: one pass in interleave order; the remainder is kept or dropped as params say
  for drop in (False, True):
    reader = dataloader.InputReader(pattern, is_training=False).host_reader(params(drop_remainder=drop), 4)
    got = list(reader)
    want = ref.batches(sizes, 4, False, SEED, 1, drop)
    assert [b.index for b in got] == want and len(want) == (3 if drop else 4)
    for b in got:
      check_content(b, shards, False)
  assert want[0] == [(0, 0), (1, 0), (2, 0), (0, 1)] and want[1] == [(2, 1), (0, 2), (2, 2), (0, 3)]      # by hand
  # training: two epochs at a seed, each permuted and shuffled, never a batch across the epoch's end
  for drop in (True, False):
    reader = dataloader.InputReader(pattern, is_training=True).host_reader(params(drop_remainder=drop), 4)
    want = ref.batches(sizes, 4, True, SEED, 2, drop)
    got = take(reader, len(want) + 1)      # it goes on into a third epoch
    reader.close()
    assert [b.index for b in got[:-1]] == want and len(want) == (6 if drop else 8)
    first = sorted(p for b in want[:len(want) // 2] for p in b)
    assert len(set(first)) == len(first) and (drop or first == sorted((f, r) for f, n in enumerate(sizes) for r in range(n)))
    assert want[:len(want) // 2] != want[len(want) // 2:] and want[0] != ref.batches(sizes, 4, False, SEED, 1, drop)[0]
    for b in got:
      check_content(b, shards, True)
  other = dataloader.InputReader(pattern, is_training=True).host_reader(params(tf_random_seed=SEED + 1), 4)
  assert [b.index for b in take(other, 3)] != want[:3]
  other.close()
  # debug: training without any shuffling, repeated
  reader = dataloader.InputReader(pattern, is_training=True, debug=True).host_reader(params(), 4)
  plain = ref.batches(sizes, 4, False, SEED, 1, True)
  assert [b.index for b in take(reader, 6)] == plain + plain
  reader.close()
  # batch_size from params; shard=(2, 1) keeps files[1::2]
  ir = dataloader.InputReader(pattern, is_training=False)
  assert [len(b.index) for b in ir.host_reader(params(batch_size=7, drop_remainder=False))] == [7, 7, 1]
  files = ir.files()
  assert [os.path.basename(f) for f in files] == ['part-%05d.tfrecord' % i for i in range(3)]
  assert ir.files(shard=(2, 1)) == files[1::2] and ir.files(shard=(2, 0)) == files[0::2]
  got = list(ir.host_reader(params(drop_remainder=False), 4, shard=(2, 0)))
  assert [b.index for b in got] == ref.batches([5, 9], 4, False, SEED, 1, False)
  assert got[0].source_ids.tolist() == [0.0, 2000.0, 1.0, 2001.0]
  assert [b.index for b in ir.host_reader(params(drop_remainder=False), 4, shard=(2, 1))] == [[(0, 0)]]


def test_order_with_more_records_than_the_shuffle_buffer_and_a_resumed_state(lib, jpegs, tmp_path):
  sizes = [40, 0, 30, 50]      # (an empty shard among them)
  shards = numbered(jpegs[0], sizes)
  pattern = write_shards(tmp_path, shards)
  want = ref.batches(sizes, 8, True, SEED, 2, True)
  assert len(want) == 30
  ir = dataloader.InputReader(pattern, is_training=True)
  reader = ir.host_reader(params(), 8)
  got = take(reader, 7)
  state = reader.get_state()      # after 56 records: 64 wait in the buffer, the thread is `depth` batches ahead
  assert len(state['buffer']) == 64 and state['live'] and state['epoch'] == 0
  rest = take(reader, 23)
  reader.close()
  assert [b.index for b in got + rest] == want
  for b in got[:2] + rest[-2:]:
    check_content(b, shards, True)
  resumed = ir.host_reader(params(tf_random_seed=999), 8)      # its own seed is replaced with the state
  resumed.set_state(state)
  again = take(resumed, 23)
  assert resumed.get_state()['epoch'] == 1
  resumed.close()
  assert [b.index for b in again] == [b.index for b in rest]
  for a, b in zip(again, rest):
    assert np.array_equal(a.boxes, b.boxes) and np.array_equal(a.counts, b.counts) and [bytes(v) for v in a.images] == [bytes(v) for v in b.images]
  # a state is the reader's own again after it was used: resuming twice gives the same stream
  resumed.set_state(state)
  assert [b.index for b in take(resumed, 3)] == [b.index for b in rest[:3]]
  resumed.close()
  # use_fake_data: batch 0 again and again
  fake = dataloader.InputReader(pattern, is_training=True, use_fake_data=True).host_reader(params(), 8)
  first = take(fake, 4)
  assert first[0].index == want[0] and all(b is first[0] for b in first)
  assert fake._thread is None      # nothing is left running


def test_rows_are_padded_crowds_skipped_and_too_many_rows_refused(lib, jpegs, tmp_path):
  shards = [[record(jpegs[1], 1, 100, crowd=[0] * 99 + [1], area=np.arange(100), source_id='17'),
             record(jpegs[0], 2, 3, crowd=[1, 0, 1]), record(jpegs[2], 3, 0, stored_size=(5, 6))]]
  pattern = write_shards(tmp_path, shards)
  ev, = list(dataloader.InputReader(pattern, is_training=False).host_reader(params(drop_remainder=False), 4))
  decoded = [ref.decode(r) for r in shards[0]]
  for got, want in zip(ev[2:8], ref.pad_batch(decoded, False, True)):
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
  assert ev.boxes.shape == (3, 100, 4) and ev.counts.tolist() == [100, 3, 0] and ev.source_ids.tolist() == [17.0, -1.0, -1.0]
  assert ev.is_crowds[1, :4].tolist() == [1, 0, 1, 0] and ev.areas[1, 3] == -1 and ev.classes[2, 0] == -1 and ev.boxes[1, 3, 0] == -1
  for skip, counts in ((True, [99, 1, 0]), (False, [100, 3, 0])):
    tr = dataloader.InputReader(pattern, is_training=True, debug=True).host_reader(
        params(drop_remainder=False, skip_crowd_during_training=skip), 3)
    batch = next(tr)
    tr.close()
    assert batch.counts.tolist() == counts
    for got, want in zip(batch[2:5], ref.pad_batch(decoded, True, skip)):
      assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
  assert np.array_equal(batch.boxes[1, 1], decoded[1]['groundtruth_boxes'][1])
  small = dataloader.InputReader(pattern, is_training=False, max_instances_per_image=8).host_reader(params(), 1)
  with pytest.raises(ValueError, match=r'please increase config.max_instances_per_image \(.*part-00000.tfrecord: record 0 at byte '
                                       r'offset 12 has 100 rows'):
    next(small)
  # 101 rows against the default of 100; the crowd row is skipped first when training, and then it fits
  (tmp_path / 'big').mkdir()
  big = write_shards(tmp_path / 'big', [[record(jpegs[0], 5, 2), record(jpegs[0], 4, 101, crowd=[1] + [0] * 100)]])
  reader = dataloader.InputReader(big, is_training=False).host_reader(params(), 1)
  assert next(reader).counts.tolist() == [2]
  with pytest.raises(tfrecord.TFRecordError, match=r'part-00000.tfrecord: record 1 at byte offset \d+ has 101 rows') as e:
    next(reader)
  assert e.value.record == 1 and e.value.path.endswith('part-00000.tfrecord')
  with pytest.raises(StopIteration):
    next(reader)
  fits = dataloader.InputReader(big, is_training=True, debug=True).host_reader(params(), 2)
  assert next(fits).counts.tolist() == [2, 100]
  fits.close()
  # a record that is not an Example, inside a well-framed file: the file, the record and the offset
  (tmp_path / 'bad').mkdir()
  bad = write_shards(tmp_path / 'bad', [[shards[0][1], shards[0][1][:-2]]])
  with pytest.raises(tfrecord.TFRecordError, match=r'part-00000.tfrecord: record 1 at byte offset \d+: record 1 is not a tf.train.Example'):
    list(dataloader.InputReader(bad, is_training=False).host_reader(params(drop_remainder=False), 4))


def test_image_spans_reach_the_huffman_stage_where_they_lie(lib, jpegs, tmp_path):
  """The hand-off copies no image byte: what the reader yields are memoryviews inside the mapped file, and the address the
  JPEG host stage is given for each is the address of that span in the mapping; the stage decodes them to what it decodes
  from bytes."""
  from automl_amd import jpeg
  shards = [[record(jpegs[k], k, 1) for k in range(3)]]
  pattern = write_shards(tmp_path, shards)
  reader = dataloader.InputReader(pattern, is_training=False).host_reader(params(drop_remainder=False), 4)
  batch = next(reader)
  reader.close()
  assert reader.files == [str(tmp_path / 'part-00000.tfrecord')]
  whole = tfrecord.TFRecordFile(reader.files[0])
  data = (tmp_path / 'part-00000.tfrecord').read_bytes()
  for k, view in enumerate(batch.images):
    assert isinstance(view, memoryview) and view.readonly and bytes(view) == jpegs[k]
    at = data.index(jpegs[k])
    keep, address, size = jpeg._buffer(view)
    assert size == len(jpegs[k]) and np.shares_memory(keep, np.frombuffer(view, np.uint8))
    mapped = np.frombuffer(reader._producer._file(0)._view, np.uint8)
    assert address == mapped.ctypes.data + at      # inside the reader's mapping, at the span's offset in the file
    assert bytes(whole[k][at - whole.offset(k):][:size]) == jpegs[k]

  def host(datas):
    n = len(datas)
    coef = np.zeros(n * jpeg.worst_blocks(*CANVAS) * 64, np.int16)
    images, qt, status = np.zeros(n * jpeg.IMAGE_BYTES, np.uint8), np.zeros((n, 4, 64), np.uint16), np.full(n, -1, np.int32)
    jpeg.entropy_decode(datas, CANVAS[0], CANVAS[1], coef, images, qt, status, 2)
    return coef, images, qt, status
  want = host(jpegs[:3])
  strided = memoryview(np.repeat(np.frombuffer(jpegs[2], np.uint8), 2))[::2]      # not contiguous: the one case that is copied
  assert not strided.c_contiguous
  for datas in (batch.images, [bytearray(j) for j in jpegs[:3]], [np.frombuffer(j, np.uint8) for j in jpegs[:3]],
                [memoryview(jpegs[0]), jpegs[1], strided]):
    for g, w in zip(host(datas), want):
      assert np.array_equal(g, w)
  assert not want[3].any() and jpeg.jpeg_info(batch.images[1]) == jpeg.jpeg_info(jpegs[1])
  assert host([memoryview(b''), jpegs[1]])[3].tolist() == [jpeg.MALFORMED, 0]


def test_what_the_reader_refuses(lib, jpegs, tmp_path):
  pattern = write_shards(tmp_path, numbered(jpegs[0], [2]))
  ir = dataloader.InputReader(pattern, is_training=False)
  with pytest.raises(ValueError, match='sstable'):
    ir.host_reader(params(dataset_type='sstable'))
  with pytest.raises(ValueError, match='segmentation'):
    ir.reader(params(heads=['object_detection', 'segmentation']), canvas=CANVAS)
  with pytest.raises(ValueError, match='regenerate_source_id=True is not built'):
    ir.host_reader(params(regenerate_source_id=True))
  with pytest.raises(ValueError, match='matches no file'):
    dataloader.InputReader(str(tmp_path / 'nothing-*'), is_training=False).host_reader(params())
  with pytest.raises(ValueError, match=r'canvas=\(Hc, Wc\)'):
    ir.reader(params())
  with pytest.raises(ValueError, match='shard'):
    ir.host_reader(params(), shard=(2, 2))
  (tmp_path / 'z').mkdir()
  packed = tmp_path / 'z' / 'part-00000.tfrecord'
  packed.write_bytes(gzip.compress((tmp_path / 'part-00000.tfrecord').read_bytes()))
  with pytest.raises(ValueError, match=r'z/part-00000.tfrecord: record 0 at byte offset 0: .*compressed TFRecord files are not read'):
    dataloader.InputReader(str(packed), is_training=False).host_reader(params())
  # a damaged second file is met on the thread and raised on the consumer's side, once
  (tmp_path / 'd').mkdir()
  pattern = write_shards(tmp_path / 'd', numbered(jpegs[0], [2, 2]))
  second = tmp_path / 'd' / 'part-00001.tfrecord'
  data = bytearray(second.read_bytes())
  data[-1] ^= 1      # the stored checksum of its last record: the records themselves are whole
  second.write_bytes(bytes(data))
  reader = dataloader.InputReader(pattern, is_training=False).host_reader(params(), 2)
  with pytest.raises(tfrecord.TFRecordError, match=r'part-00001.tfrecord: record 1 at byte offset \d+: the checksum of the record'):
    list(reader)
  assert reader._thread is None and list(reader) == []
  # a source id that is not text: the file, the record and the offset, as for every other record that cannot be used
  (tmp_path / 'u').mkdir()
  odd = write_shards(tmp_path / 'u', [[record(jpegs[0], 1, 1, source_id='5'), record(jpegs[0], 2, 1, source_id=b'\xff\xfe')]])
  with pytest.raises(tfrecord.TFRecordError, match=r"u/part-00000.tfrecord: record 1 at byte offset \d+: record 1: 'image/source_id' is not UTF-8") as e:
    list(dataloader.InputReader(odd, is_training=False).host_reader(params(), 2))
  assert e.value.record == 1 and e.value.path.endswith('part-00000.tfrecord') and e.value.offset > 12
  got = list(dataloader.InputReader(pattern, is_training=False).host_reader(params(), 2, verify=False))
  assert [b.index for b in got] == [[(0, 0), (1, 0)], [(0, 1), (1, 1)]]


# ------------------------------------------------------------------------------------------------------------ the device
def gpu_shards(jpegs, folder):
  """Six records in two shards of three: 0 to 5 boxes, one crowd row (record 1 of shard 0), empty and stored areas, empty and
  numeric source ids, one stored size."""
  spec = [dict(boxes=2, source_id='11', area=[100.0, 2500.0], crowd=[0, 0]), dict(boxes=3, crowd=[0, 1, 0], source_id=''),
          dict(boxes=0, source_id='13'), dict(boxes=5, source_id='14', stored_size=(31, 22)), dict(boxes=1, crowd=[]),
          dict(boxes=4, source_id='16', area=[])]
  records = [record(jpegs[k], k, **s) for k, s in enumerate(spec)]
  shards = [records[:3], records[3:]]
  return shards, write_shards(folder, shards)


def by_hand(shards, index, is_training, skip_crowd=True):
  from automl_amd import jpeg
  decoded = [ref.decode(shards[f][r]) for f, r in index]
  raw, sizes = jpeg.JpegDecoder(len(index), *CANVAS).decode([d['image'] for d in decoded])
  boxes, classes, counts, is_crowds, areas, ids = ref.pad_batch(decoded, is_training, skip_crowd)
  if is_training:
    return ((raw, sizes), boxes, classes, counts)
  return ((raw, sizes), boxes, classes, counts, is_crowds, areas, ids)


def assert_batches_equal(got, want, what):
  assert len(got) == len(want), what
  (raw, sizes), (want_raw, want_sizes) = got[0], want[0]
  assert raw.dtype == torch.uint8 and raw.is_cuda and torch.equal(raw, want_raw), what
  assert isinstance(sizes, np.ndarray) and sizes.dtype == np.int32 and np.array_equal(sizes, want_sizes), what
  for k, (g, w) in enumerate(zip(got[1:], want[1:])):
    assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k)


@pytest.mark.gpu
def test_evaluation_reader_equals_the_batches_built_by_hand(jpegs, tmp_path):
  shards, pattern = gpu_shards(jpegs, tmp_path)
  # drop_remainder=False, as tf2/eval.py sets it (eval_lib.eval_config): the short last batch is evaluated
  reader = dataloader.InputReader(pattern, is_training=False).reader(params(drop_remainder=False), batch_size=4, canvas=CANVAS)
  got = list(reader)
  order = ref.batches([3, 3], 4, False, SEED, 1, False)
  assert [len(b) for b in order] == [4, 2] and len(got) == 2
  for k, (batch, index) in enumerate(zip(got, order)):
    assert_batches_equal(batch, by_hand(shards, index, False), k)
  torch.cuda.synchronize()
  assert tuple(got[0][0][0].shape) == (4, 64, 64, 3) and tuple(got[1][0][0].shape) == (2, 64, 64, 3)
  assert got[0][0][1].tolist() == [[8, 9], [31, 22], [16, 16], [37, 53]] and got[0][6].tolist() == [11.0, 14.0, -1.0, -1.0]
  assert got[0][3].tolist() == [2, 5, 3, 1] and got[0][4][2, :3].tolist() == [0, 1, 0]
  g = np.load(GOLDEN)
  assert np.array_equal(got[1][0][0][1, :16, :16].cpu().numpy(), g['grey_16x16_q75/rgb'])      # the pixels are Pillow's
  assert not got[1][0][0][1, 16:].any()
  # an image larger than the canvas: refused with the files of the batch, or handed to the fallback
  small = dataloader.InputReader(pattern, is_training=False).reader(params(), batch_size=4, canvas=(32, 32))
  with pytest.raises(ValueError, match=r'contents\[3\] is not decoded: an image larger than the canvas.*part-00001.tfrecord record 1'):
    next(small)
  small.close()
  seen = []

  def fallback(data):
    seen.append(bytes(data))
    return np.full((5, 7, 3), 9, np.uint8)
  lenient = dataloader.InputReader(pattern, is_training=False).reader(params(), batch_size=4, canvas=(32, 32), fallback=fallback)
  (raw, sizes) = next(lenient)[0]
  lenient.close()
  assert seen == [jpegs[4]] and sizes.tolist() == [[8, 9], [31, 22], [16, 16], [5, 7]] and int(raw[3, :5, :7].min()) == 9
  assert not raw[3, 5:].any() and not raw[3, :, 7:].any()


def eval_net():
  from automl_amd import train_lib
  from oracle.problems import perturbed_params
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  config.override('image_size=128')
  return config, train_lib.EfficientDetNetTrain(config=config, dtype='f32', params=perturbed_params(config, 3), seed=5,
                                                steps_per_epoch=10, global_batch_size=64, use_graph=False)


@pytest.mark.gpu
def test_evaluation_step_from_the_reader_equals_the_step_from_the_batch_built_by_hand(jpegs, tmp_path):
  shards, pattern = gpu_shards(jpegs, tmp_path)
  config, net = eval_net()
  p = config.as_dict()
  p['tf_random_seed'] = SEED
  batch = next(dataloader.InputReader(pattern, is_training=False).reader(p, batch_size=4, canvas=CANVAS))
  results = []
  for data in (batch, by_hand(shards, ref.batches([3, 3], 4, False, SEED, 1, False)[0], False)):
    values, labels = net.test_step_raw(data)
    torch.cuda.synchronize()
    results.append((values, {k: v.clone() for k, v in labels.items()}))      # the buffers are the next call's too
  (values, labels), (want_values, want_labels) = results
  assert values == want_values and np.isfinite(values['loss']) and values['cls_loss'] > 0
  assert sorted(labels) == sorted(want_labels) and {'source_ids', 'image_scales', 'groundtruth_data'} <= set(labels)
  for k in labels:
    assert torch.equal(labels[k].view(torch.uint8), want_labels[k].view(torch.uint8)), k
  assert labels['source_ids'].tolist() == [11.0, 14.0, -1.0, -1.0]
  assert float(labels['groundtruth_data'][2, 1, 4]) == 1.0 and float(labels['groundtruth_data'][0, 1, 5]) == 2500.0


@pytest.mark.gpu
def test_training_steps_from_the_reader_equal_the_steps_from_batches_built_by_hand(jpegs, tmp_path):
  from automl_amd import train_lib
  from oracle.problems import perturbed_params
  from tests.test_det_input import assert_same, snapshot
  shards, pattern = gpu_shards(jpegs, tmp_path)
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  config.override('image_size=128')
  assert config.skip_crowd_during_training
  p = config.as_dict()
  p['tf_random_seed'] = SEED
  nets = [train_lib.EfficientDetNetTrain(config=config, dtype='bf16', params=perturbed_params(config, 3), seed=5, steps_per_epoch=10,
                                         global_batch_size=64, use_graph=True) for _ in range(2)]
  order = ref.batches([3, 3], 2, True, SEED, 1, True)
  assert len(order) == 3 and (0, 1) in order[0] + order[1]      # the record with the crowd row is among the two steps
  reader = dataloader.InputReader(pattern, is_training=True).reader(p, batch_size=2, canvas=CANVAS)
  got, want = [], []
  for step in range(2):      # the second step is a replay
    batch = next(reader)
    hand = by_hand(shards, order[step], True)
    assert_batches_equal(batch, hand, step)
    got.append(nets[0].train_step_raw(batch))
    want.append(nets[1].train_step_raw(hand))
  reader.close()
  step = 0 if (0, 1) in order[0] else 1
  assert ref.pad_batch([ref.decode(shards[0][1])], True, True)[2].tolist() == [2]      # three boxes, one of them a crowd
  assert ref.pad_batch([ref.decode(shards[f][r]) for f, r in order[step]], True, True)[2][order[step].index((0, 1))] == 2
  assert_same(snapshot(nets[0], got), snapshot(nets[1], want), 'reader to step')
  assert all(np.isfinite(v['loss']) and v['cls_loss'] > 0 for v in got)


@pytest.mark.gpu
def test_batches_iterated_without_a_synchronisation_equal_the_synchronised_ones(jpegs, tmp_path):
  """depth=2: the decoder's two sets of pinned arenas are written again for batches 2, 3 and 4 while earlier copies may still
  be in flight; the events behind them, not a synchronisation of ours, keep the bytes apart."""
  shards, pattern = gpu_shards(jpegs, tmp_path)
  runs = []
  for sync in (False, True):
    reader = dataloader.InputReader(pattern, is_training=True).reader(params(), batch_size=2, canvas=CANVAS, depth=2)
    batches = []
    for batch in reader:
      batches.append(batch)
      if sync:
        torch.cuda.synchronize()
      if len(batches) == 5:
        break
    reader.close()
    runs.append(batches)
  torch.cuda.synchronize()
  order = ref.batches([3, 3], 2, True, SEED, 2, True)
  for k, (a, b) in enumerate(zip(*runs)):
    assert_batches_equal(a, b, k)
    assert a[0][1].tolist() == [[ref.decode(shards[f][r])[key] for key in ('height', 'width')] for f, r in order[k]]
  assert len({tuple(a[0][1].reshape(-1).tolist()) for a in runs[0]}) > 1
