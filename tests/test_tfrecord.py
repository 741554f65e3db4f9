"""TFRecord framing, CRC-32C and tf.train.Example parsing without a device (automl_amd/tfrecord.py and tf_example_decoder.py
on csrc/tfrecord_host.cpp, called through ctypes on the built library): the CRC's known answers and tf_checkpoint.crc32c; a
file assembled byte by byte; the parser and the decoder against the pure-Python restatement tests/tfrecord_ref.py on every
encoding protobuf allows for these messages; every status of the two entry points reached by a constructed input; and a
stand-alone program that runs the host stage over prefixes and corruptions under the address and undefined-behaviour
sanitizers.  Everything is exact: there is no tolerance anywhere."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from automl_amd import _lib, tf_checkpoint, tf_example_decoder, tfrecord
from tests import tfrecord_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


@pytest.fixture(scope='module')
def jpegs():
  g = np.load(GOLDEN)
  return {n: g[n + '/bytes'].tobytes() for n in ('s8x9_420_q75', 's17x33_422_q75', 'grey_16x16_q75')}


def test_crc32c_known_answers_and_the_restatement(lib):
  assert tfrecord.crc32c(b'123456789') == 0xE3069283
  assert tfrecord.crc32c(bytes(32)) == 0x8A9136AA
  assert tfrecord.crc32c(b'\xff' * 32) == 0x62A8AB43
  rng = np.random.default_rng(11)
  for n in list(range(0, 40)) + [63, 64, 65, 1023, 1024, 4099] + [int(v) for v in rng.integers(0, 4100, 40)]:
    data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    want = tf_checkpoint.crc32c(data)
    assert tfrecord.crc32c(data) == want, n
    cut = int(rng.integers(0, n + 1))
    assert tfrecord.crc32c(data[cut:], tfrecord.crc32c(data[:cut])) == want, (n, cut)
    assert tfrecord.crc32c(memoryview(data)[cut:], tf_checkpoint.crc32c(data[:cut])) == want, (n, cut)
  for c in (0, 1, 0x7fff, 0x8000, 0xE3069283, 0xffffffff, 0x5d7d1528):
    assert tfrecord.mask_crc(c) == tf_checkpoint.mask_crc(c)


def test_a_file_assembled_by_hand_reads_back_and_the_writer_writes_it(lib, tmp_path):
  records = [b'first record', b'']
  by_hand = b''
  for r in records:
    head = struct.pack('<Q', len(r))
    by_hand += head + struct.pack('<I', tf_checkpoint.mask_crc(tf_checkpoint.crc32c(head)))
    by_hand += r + struct.pack('<I', tf_checkpoint.mask_crc(tf_checkpoint.crc32c(r)))
  path = tmp_path / 'hand.tfrecord'
  path.write_bytes(by_hand)
  f = tfrecord.TFRecordFile(path)
  got = list(f)
  assert all(isinstance(v, memoryview) for v in got) and [bytes(v) for v in got] == records
  assert len(f) == 2 and bytes(f[1]) == b'' and f.offset(0) == 12 and f.offset(1) == 12 + 12 + 4 + 12
  with pytest.raises(IndexError):
    f[2]
  with tfrecord.TFRecordWriter(tmp_path / 'written.tfrecord') as w:
    for r in records:
      w.write(r)
  assert (tmp_path / 'written.tfrecord').read_bytes() == by_hand
  (tmp_path / 'empty.tfrecord').write_bytes(b'')
  assert len(tfrecord.TFRecordFile(tmp_path / 'empty.tfrecord')) == 0
  # more records than one indexing call takes
  with tfrecord.TFRecordWriter(tmp_path / 'many.tfrecord') as w:
    for i in range(tfrecord.INDEX_CHUNK + 3):
      w.write(struct.pack('<I', i))
  many = tfrecord.TFRecordFile(tmp_path / 'many.tfrecord')
  assert bytes(many[tfrecord.INDEX_CHUNK + 2]) == struct.pack('<I', tfrecord.INDEX_CHUNK + 2) and len(many) == tfrecord.INDEX_CHUNK + 3


def test_encode_example_is_sorted_and_packed(lib):
  a = tfrecord.encode_example({'b': np.array([1.5, -0.0], np.float32), 'a': 'text', 'c': [3, -1], 'd': []})
  b = tfrecord.encode_example({'d': np.zeros(0, np.int64), 'c': np.array([3, -1]), 'a': b'text', 'b': [1.5, -0.0]})
  assert a == b
  want = ref.example([('a', ref.feature(1, ref.bytes_list([b'text']))),
                      ('b', ref.feature(2, ref.float_list([0x3fc00000, 0x80000000]))),
                      ('c', ref.feature(3, ref.int64_list([3, -1]))), ('d', ref.feature(0, b''))])
  assert a == want


F = {'zero': 0x00000000, 'negzero': 0x80000000, 'denormal': 0x00000001, 'negdenormal': 0x807fffff, 'nan': 0x7fc00001,
     'signalling': 0x7f800001, 'negnan': 0xffc00000, 'inf': 0x7f800000, 'half': 0x3f000000, 'max': 0x7f7fffff}
INT_EXTREMES = [0, 1, -1, 2 ** 63 - 1, -2 ** 63, 127, 128, -129, 2 ** 32, -2 ** 31]
SPEC = [('bytes', 'bytes', 3), ('floats', 'float', 12), ('ints', 'int64', 12), ('absent', 'float', 2), ('empty', 'int64', 2),
        ('', 'int64', 2)]


def _examples():
  bits = list(F.values())
  group = (ref.varint(13 << 3 | 3) + ref.varint(14 << 3 | 0) + ref.varint(5) + ref.varint(15 << 3 | 3) + ref.varint(15 << 3 | 4) +
           ref.ld(16, b'in') + ref.varint(1 << 3 | 5) + bytes(4) + ref.varint(13 << 3 | 4))      # with a group and fields inside
  unknown = (ref.varint(9 << 3 | 0) + ref.varint(2 ** 64 - 1) + ref.varint(10 << 3 | 1) + bytes(8) + ref.ld(11, b'xyz') +
             ref.varint(12 << 3 | 5) + bytes(4) + group)      # one unknown field of each wire type
  out = {}
  for mode in ('packed', 'unpacked', 'mixed'):
    out[mode] = ref.example([('bytes', ref.feature(1, ref.bytes_list([b'one', b'', b'three']))),
                             ('floats', ref.feature(2, ref.float_list(bits, mode))),
                             ('ints', ref.feature(3, ref.int64_list(INT_EXTREMES, mode))),
                             ('unwanted', ref.feature(3, ref.int64_list([5]))), ('empty', ref.feature(0, b''))])
  out['duplicate key'] = ref.example([('ints', ref.feature(3, ref.int64_list([1, 2, 3]))), ('floats', ref.feature(2, ref.float_list(bits[:2]))),
                                      ('ints', ref.feature(3, ref.int64_list([7])))])
  out['unknown fields'] = ref.example([('ints', unknown + ref.feature(3, unknown + ref.int64_list([4, 5]) + unknown) + unknown)],
                                      unknown=unknown, features_unknown=unknown)
  out['member twice'] = ref.example([('ints', ref.feature(3, ref.int64_list([1])) + ref.feature(3, ref.int64_list([2], 'unpacked')))])
  out['another member first'] = ref.example([('ints', ref.feature(2, ref.float_list([1])) + ref.feature(3, ref.int64_list([9])))])
  out['empty lists'] = ref.example([('floats', ref.feature(2, b'')), ('ints', ref.feature(3, ref.ld(1, b''))), ('bytes', ref.feature(1, b''))])
  out['empty key'] = ref.example([('', ref.feature(3, ref.int64_list([6])))])
  out['entry without value'] = ref.example([]) + ref.ld(1, ref.ld(1, ref.ld(1, b'ints')))
  out['two features fields'] = ref.example([('ints', ref.feature(3, ref.int64_list([1])))]) + ref.example([('floats', ref.feature(2, ref.float_list([7])))])
  out['ten byte varint'] = ref.example([('ints', ref.feature(3, ref.varint(1 << 3) + b'\xff' * 9 + b'\x7f'))])
  nest = lambda n: b''.join(ref.varint(20 << 3 | 3) for _ in range(n)) + b''.join(ref.varint(20 << 3 | 4) for _ in range(n))      # noqa: E731
  out['groups 32 deep'] = nest(32) + ref.example([('ints', ref.feature(3, ref.int64_list([8])))])
  out['nothing'] = b''
  return out


def _compare(parsed, i, record, spec, name):
  want = ref.parse_example(record, spec)
  for key, kind, cap in spec:
    count = int(parsed.counts[key][i])
    if want[key] is None:
      assert count == -1, (name, key)
      continue
    assert count == len(want[key]), (name, key, count, want[key])
    got = parsed.values[key][i, :count]
    if kind == 'float':
      assert got.dtype == np.float32 and got.view(np.uint32).tolist() == want[key], (name, key)
    elif kind == 'int64':
      assert got.dtype == np.int64 and got.tolist() == want[key], (name, key)
    else:
      assert [tuple(v) for v in got.tolist()] == want[key], (name, key)


def test_parse_examples_equals_the_restatement(lib):
  examples = _examples()
  names = sorted(examples)
  records = [examples[n] for n in names]
  parsed = tfrecord.parse_examples(records, SPEC)
  assert parsed.status.tolist() == [0] * len(records), dict(zip(names, parsed.status.tolist()))
  for i, name in enumerate(names):
    _compare(parsed, i, records[i], SPEC, name)
  # what the restatement itself gives, by hand, where it matters most
  i = names.index('packed')
  assert parsed.values['floats'][i, :10].view(np.uint32).tolist() == list(F.values())
  assert parsed.values['ints'][i, :10].tolist() == INT_EXTREMES
  assert [records[i][o:o + n] for o, n in parsed.values['bytes'][i].tolist()] == [b'one', b'', b'three']
  assert parsed.counts['absent'][i] == -1 and parsed.counts['empty'][i] == 0
  assert parsed.values['ints'][names.index('duplicate key'), :1].tolist() == [7] and parsed.counts['ints'][names.index('duplicate key')] == 1
  assert parsed.values['ints'][names.index('member twice'), :2].tolist() == [1, 2]
  assert parsed.values['ints'][names.index('another member first'), :1].tolist() == [9]
  assert parsed.values['ints'][names.index('ten byte varint'), :1].tolist() == [-1]
  assert parsed.counts[''][names.index('empty key')] == 1 and parsed.counts['ints'][names.index('entry without value')] == 0
  # memoryviews as TFRecordFile yields them, and every thread count, give the same arrays
  for threads in (1, 3, 16):
    again = tfrecord.parse_examples([memoryview(r) for r in records], SPEC, threads)
    assert again.status.tolist() == parsed.status.tolist()
    for key in parsed.values:
      assert np.array_equal(again.values[key].view(np.uint8), parsed.values[key].view(np.uint8)), (threads, key)
      assert np.array_equal(again.counts[key], parsed.counts[key]), (threads, key)
  empty = tfrecord.parse_examples([], SPEC)
  assert empty.status.shape == (0,) and empty.values['floats'].shape == (0, 12)
  for threads in (0, 17):
    with pytest.raises(ValueError):
      tfrecord.parse_examples(records, SPEC, threads)


def test_every_parse_status_is_reached(lib):
  good = _examples()['mixed']
  ints = lambda payload: ref.example([('ints', ref.feature(3, payload))])      # noqa: E731
  cases = {
      'eleven byte varint': (ints(ref.varint(1 << 3) + b'\xff' * 10 + b'\x01'), tfrecord.E_VARINT),
      'varint cut off': (ints(ref.varint(1 << 3) + b'\xff'), tfrecord.E_VARINT),
      'tag cut off': (b'\x8a', tfrecord.E_VARINT),
      'length past the end': (good[:-1], tfrecord.E_LENGTH),
      'inner length past the end': (ints(ref.varint(1 << 3 | 2) + ref.varint(5) + b'\x01'), tfrecord.E_LENGTH),
      'packed floats of 7 bytes': (ref.example([('floats', ref.feature(2, ref.ld(1, bytes(7))))]), tfrecord.E_LENGTH),
      'fixed32 cut off': (ref.example([('floats', ref.feature(2, ref.varint(1 << 3 | 5) + bytes(3)))]), tfrecord.E_LENGTH),
      'unknown fixed64 cut off': (ref.varint(9 << 3 | 1) + bytes(7), tfrecord.E_LENGTH),
      'features as a varint': (ref.varint(1 << 3 | 0) + ref.varint(3), tfrecord.E_WIRE_TYPE),
      'float value as a varint': (ref.example([('floats', ref.feature(2, ref.varint(1 << 3 | 0) + ref.varint(3)))]), tfrecord.E_WIRE_TYPE),
      'int value as fixed32': (ints(ref.varint(1 << 3 | 5) + bytes(4)), tfrecord.E_WIRE_TYPE),
      'bytes value as a varint': (ref.example([('bytes', ref.feature(1, ref.varint(1 << 3 | 0) + ref.varint(3)))]), tfrecord.E_WIRE_TYPE),
      'an end-group tag that closes nothing': (ref.varint(9 << 3 | 4), tfrecord.E_WIRE_TYPE),
      'a group closed by another number': (ref.varint(9 << 3 | 3) + ref.varint(8 << 3 | 4), tfrecord.E_WIRE_TYPE),
      'a group without its end': (ref.varint(9 << 3 | 3) + ref.varint(1 << 3 | 0) + ref.varint(1), tfrecord.E_LENGTH),
      'features as a group': (ref.varint(1 << 3 | 3) + ref.varint(1 << 3 | 4), tfrecord.E_WIRE_TYPE),
      'groups 33 deep': (b''.join(ref.varint(20 << 3 | 3) for _ in range(33)) + b''.join(ref.varint(20 << 3 | 4) for _ in range(33)),
                         tfrecord.E_WIRE_TYPE),
      'wire type 7': (ints(ref.varint(5 << 3 | 7)), tfrecord.E_WIRE_TYPE),
      'thirteen ints': (ints(ref.int64_list(range(13))), tfrecord.E_CAPACITY),
      'thirteen floats, mixed': (ref.example([('floats', ref.feature(2, ref.float_list(range(13), 'mixed')))]), tfrecord.E_CAPACITY),
      'four byte strings': (ref.example([('bytes', ref.feature(1, ref.bytes_list([b'a'] * 4)))]), tfrecord.E_CAPACITY),
      'floats under an int key': (ref.example([('ints', ref.feature(2, ref.float_list([1])))]), tfrecord.E_KIND),
      'an empty bytes list under a float key': (ref.example([('floats', ref.feature(1, b''))]), tfrecord.E_KIND),
  }
  names = sorted(cases)
  records = [good] + [cases[n][0] for n in names] + [good]      # the good ones around them stay good
  parsed = tfrecord.parse_examples(records, SPEC, 4)
  assert parsed.status[0] == 0 and parsed.status[-1] == 0
  for i, name in enumerate(names):
    assert parsed.status[i + 1] == cases[name][1], (name, parsed.status[i + 1])
    assert ref.status_of(cases[name][0], SPEC) == cases[name][1], name
  assert {c[1] for c in cases.values()} == set(tfrecord.PARSING)
  _compare(parsed, len(records) - 1, good, SPEC, 'the last')


def _index(data, verify=True, capacity=8):
  offsets, lengths, status, consumed = tfrecord.index_buffer(np.frombuffer(data, np.uint8), verify, capacity)
  return offsets.tolist(), lengths.tolist(), status, consumed


def test_every_framing_status_is_reached_and_named(lib, tmp_path):
  recs = [b'abc', b'defgh', b'']
  data = b''.join(ref.frame(r, tfrecord.crc32c, tfrecord.mask_crc) for r in recs)
  assert _index(data) == ([12, 31, 52], [3, 5, 0], tfrecord.OK, len(data))
  assert _index(data[:5])[2:] == (tfrecord.TRUNCATED_HEADER, 0)
  assert _index(data[:19 + 7]) == ([12], [3], tfrecord.TRUNCATED_HEADER, 19)
  assert _index(data[:19 + 14]) == ([12], [3], tfrecord.TRUNCATED_PAYLOAD, 19)
  assert _index(data[:19 + 14], verify=False)[2:] == (tfrecord.LENGTH_RANGE, 19)
  flip = lambda at: data[:at] + bytes([data[at] ^ 0x40]) + data[at + 1:]      # noqa: E731
  assert _index(flip(19 + 2))[2:] == (tfrecord.LENGTH_CRC, 19)
  assert _index(flip(19 + 9))[2:] == (tfrecord.LENGTH_CRC, 19)
  assert _index(flip(19 + 13))[2:] == (tfrecord.DATA_CRC, 19)
  assert _index(flip(19 + 12 + 5 + 1))[2:] == (tfrecord.DATA_CRC, 19)
  assert _index(flip(19 + 13), verify=False)[2] == tfrecord.OK
  huge = struct.pack('<Q', 2 ** 63)
  huge += struct.pack('<I', tfrecord.mask_crc(tfrecord.crc32c(huge))) + b'abc' + bytes(4)
  assert _index(huge)[2:] == (tfrecord.TRUNCATED_PAYLOAD, 0) and _index(huge, verify=False)[2:] == (tfrecord.LENGTH_RANGE, 0)
  # capacity reached, and the walk continued from `consumed`
  off, ln, status, consumed = _index(data, capacity=2)
  assert (off, ln, status, consumed) == ([12, 31], [3, 5], tfrecord.CAPACITY, 40)
  offsets, _, status, consumed = tfrecord.index_buffer(np.frombuffer(data, np.uint8), True, 2, base=consumed)
  assert (offsets.tolist(), status, consumed) == ([52], tfrecord.OK, len(data))
  # the Python layer names the file, the record and the byte offset
  path = tmp_path / 'damaged.tfrecord'
  path.write_bytes(flip(19 + 13))
  with pytest.raises(tfrecord.TFRecordError) as e:
    list(tfrecord.TFRecordFile(path))
  assert (e.value.path, e.value.record, e.value.offset, e.value.status) == (str(path), 1, 19, tfrecord.DATA_CRC)
  assert str(path) in str(e.value) and 'record 1' in str(e.value) and 'byte offset 19' in str(e.value)
  assert [bytes(v) for v in tfrecord.TFRecordFile(path, verify=False)] == recs[:1] + [flip(19 + 13)[31:36]] + recs[2:]
  import gzip
  import zlib
  for name, packed in (('gz', gzip.compress(data)), ('zlib', zlib.compress(data))):
    (tmp_path / name).write_bytes(packed)
    with pytest.raises(ValueError, match='compressed TFRecord files are not read'):
      len(tfrecord.TFRecordFile(tmp_path / name))


def _detection(jpeg, **kw):
  feats = {'image/encoded': jpeg}
  feats.update(kw)
  return tfrecord.encode_example(feats)


def _box_lists(n, rng):
  lo = rng.random((n, 2)).astype(np.float32) * np.float32(0.5)
  hi = lo + rng.random((n, 2)).astype(np.float32) * np.float32(0.5)
  return {'image/object/bbox/ymin': lo[:, 0], 'image/object/bbox/xmin': lo[:, 1], 'image/object/bbox/ymax': hi[:, 0],
          'image/object/bbox/xmax': hi[:, 1], 'image/object/class/label': rng.integers(1, 91, n)}


def _same(got, want, name):
  assert set(got) == set(want), name
  assert bytes(got['image']) == want['image'] and isinstance(got['image'], memoryview), name
  assert (got['source_id'], got['height'], got['width']) == (want['source_id'], want['height'], want['width']), name
  for key, dt in (('groundtruth_boxes', np.float32), ('groundtruth_area', np.float32), ('groundtruth_classes', np.int64),
                  ('groundtruth_is_crowd', np.bool_)):
    assert got[key].dtype == dt and got[key].shape == want[key].shape, (name, key, got[key].shape, want[key].shape)
    assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), (name, key)


def test_decoder_equals_the_restatement(lib, jpegs):
  rng = np.random.default_rng(3)
  j = list(jpegs.values())
  odd = np.array(list(F.values()), np.uint32).view(np.float32)
  records = {
      'no boxes, no optional keys': _detection(j[0]),
      'one box': _detection(j[1], **{'image/source_id': '139', 'image/height': 17, 'image/width': 33, 'image/object/area': [12.5],
                                     'image/object/is_crowd': [1], **_box_lists(1, rng)}),
      'a hundred boxes': _detection(j[2], **{'image/source_id': b'7', 'image/object/is_crowd': rng.integers(0, 2, 100),
                                             'image/object/area': rng.random(100).astype(np.float32), **_box_lists(100, rng)}),
      'empty area and crowd lists': _detection(j[0], **{'image/object/area': [], 'image/object/is_crowd': [], **_box_lists(5, rng)}),
      'a stored height alone': _detection(j[1], **{'image/height': 99, **_box_lists(2, rng)}),
      'crowd flags that are not 0 or 1': _detection(j[0], **{**_box_lists(3, rng), 'image/object/is_crowd': [2, 0, -1]}),
      'float bit patterns': _detection(j[0], **{'image/object/bbox/ymin': odd, 'image/object/bbox/xmin': odd[::-1], 'image/object/bbox/ymax': odd,
                                                'image/object/bbox/xmax': odd, 'image/object/class/label': np.array(INT_EXTREMES),
                                                'image/object/area': odd}),
      'an empty source id': _detection(j[2], **{'image/source_id': '', **_box_lists(1, rng)}),
      'unpacked, with a duplicate key': ref.example(
          [('image/object/class/label', ref.feature(3, ref.int64_list([9, 9, 9]))), ('image/encoded', ref.feature(1, ref.bytes_list([j[0]]))),
           ('image/object/bbox/ymin', ref.feature(2, ref.float_list([F['half'], F['zero']], 'unpacked'))),
           ('image/object/bbox/xmin', ref.feature(2, ref.float_list([F['zero'], F['half']], 'mixed'))),
           ('image/object/bbox/ymax', ref.feature(2, ref.float_list([F['max'], F['half']]))),
           ('image/object/bbox/xmax', ref.feature(2, ref.float_list([F['half'], F['half']], 'unpacked'))),
           ('image/object/class/label', ref.feature(3, ref.int64_list([4, 5], 'unpacked'))), ('image/object/mask', ref.feature(1, b''))],
          unknown=ref.ld(7, b'ignored')),
  }
  names = sorted(records)
  dec = tf_example_decoder.TfExampleDecoder()
  got = dec.decode([memoryview(records[n]) for n in names])
  for name, g in zip(names, got):
    _same(g, ref.decode(records[name]), name)
  by = dict(zip(names, got))
  assert (by['no boxes, no optional keys']['height'], by['no boxes, no optional keys']['width']) == (8, 9)
  assert by['no boxes, no optional keys']['groundtruth_boxes'].shape == (0, 4) and by['no boxes, no optional keys']['source_id'] == ''
  assert (by['a stored height alone']['height'], by['a stored height alone']['width']) == (17, 33)      # both from the image
  assert by['a hundred boxes']['groundtruth_boxes'].shape == (100, 4) and by['a hundred boxes']['source_id'] == '7'
  assert by['crowd flags that are not 0 or 1']['groundtruth_is_crowd'].tolist() == [True, False, True]
  assert by['unpacked, with a duplicate key']['groundtruth_classes'].tolist() == [4, 5]
  one = by['one box']
  assert one['groundtruth_area'].tolist() == [12.5] and one['groundtruth_is_crowd'].tolist() == [True]
  five = by['empty area and crowd lists']
  b = five['groundtruth_boxes']
  assert np.array_equal(five['groundtruth_area'], (b[:, 3] - b[:, 1]) * (b[:, 2] - b[:, 0])) and not five['groundtruth_is_crowd'].any()
  # lists longer than the first pass's capacity are parsed again, not refused
  long = _detection(j[0], **_box_lists(tf_example_decoder.LIST_CAPACITY + 5, rng))
  both = dec.decode([records['one box'], long])
  _same(both[1], ref.decode(long), 'a long record')
  _same(both[0], ref.decode(records['one box']), 'the record beside it')


def test_decoder_refuses(lib, jpegs):
  j = jpegs['s8x9_420_q75']
  rng = np.random.default_rng(4)
  dec = tf_example_decoder.TfExampleDecoder()
  good = _detection(j, **_box_lists(2, rng))
  with pytest.raises(ValueError, match="record 1 has no 'image/encoded'"):
    dec.decode([good, tfrecord.encode_example({'image/source_id': '5'})])
  lists = _box_lists(3, rng)
  lists['image/object/bbox/xmax'] = lists['image/object/bbox/xmax'][:2]
  with pytest.raises(ValueError, match='record 0: the box lists have 3, 3, 3 and 2'):
    dec.decode([_detection(j, **lists)])
  with pytest.raises(ValueError, match='2 crowd flags for 3 classes'):
    dec.decode([_detection(j, **{**_box_lists(3, rng), 'image/object/is_crowd': [0, 1]})])
  with pytest.raises(tfrecord.TFRecordError, match='record 1 is not a tf.train.Example') as e:
    dec.decode([good, good[:-3]])
  assert e.value.status == tfrecord.E_LENGTH and e.value.record == 1
  with pytest.raises(tfrecord.TFRecordError, match="record 1: 'image/source_id' is not UTF-8 text") as e:
    dec.decode([good, _detection(j, **{'image/source_id': b'\xff\xfe1'})])
  assert e.value.record == 1
  with pytest.raises(ValueError, match='another kind of list'):
    dec.decode([_detection(j, **{'image/height': [2.5]})])
  with pytest.raises(ValueError, match='no frame header'):
    dec.decode([_detection(b'not a jpeg')])
  with pytest.raises(ValueError, match=r'include_mask=True is not built.*tf_example_decoder\.py:49'):
    tf_example_decoder.TfExampleDecoder(include_mask=True)
  with pytest.raises(ValueError, match=r'regenerate_source_id=True is not built.*tf_example_decoder\.py:22'):
    tf_example_decoder.TfExampleDecoder(regenerate_source_id=True)


def _cxx():
  return shutil.which('g++') or next((p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/bin/amdclang++') if os.path.exists(p)), None)


def test_host_stage_under_sanitizers(tmp_path):
  """tests/c_host/tfrecord_host_check.cpp + csrc/tfrecord_host.cpp, built with -fsanitize=address,undefined and run as a child
  process (see the program's header for its inputs).  Skips only where the host compiler cannot build a trivial sanitized
  program."""
  cxx = _cxx()
  flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-pthread']
  trivial = tmp_path / 'trivial.cpp'
  trivial.write_text('int main() { return 0; }\n')
  if cxx is None or subprocess.run([cxx] + flags + [str(trivial), '-o', str(tmp_path / 'trivial')],
                                   capture_output=True).returncode != 0 or \
      subprocess.run([str(tmp_path / 'trivial')], capture_output=True).returncode != 0:
    pytest.skip('the host compiler cannot build a sanitized program')
  exe = str(tmp_path / 'tfrecord_host_check')
  r = subprocess.run([cxx] + flags + ['-Wall', '-Wextra', os.path.join(ROOT, 'tests', 'c_host', 'tfrecord_host_check.cpp'),
                                      os.path.join(ROOT, 'automl_amd', 'csrc', 'tfrecord_host.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  r = subprocess.run([exe], capture_output=True, text=True, errors='replace', timeout=600)
  assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
  assert ' 0 failures' in r.stdout, r.stdout
