"""TFRecord files and tf.train.Example messages, read and written without TensorFlow (csrc/tfrecord_host.cpp through ctypes;
host only, no device needed).  The reference starts here: dataloader.InputReader reads TFRecord shards of Example protos
written by dataset/create_coco_tfrecord.py (dataloader.py:404-460, object_detection/tf_example_decoder.py).

  TFRecordFile(path)       the records of one file as memoryviews into its mmap: nothing is copied
  TFRecordWriter(path)     writes such a file; encode_example(dict) serializes one Example, keys sorted
  parse_examples(records, spec)   the wanted keys of a batch of Examples as numpy arrays and spans, on up to 16 threads
  crc32c / mask_crc        the checksum of the framing (the library's slicing tables; tf_checkpoint.crc32c is the restatement)

Both formats are read by their specifications, as tf_checkpoint.py reads its own: no TensorFlow-written file has been read
here.  Not built: compressed records (GZIP / ZLIB options of TFRecordWriter), SequenceExample."""
import collections
import ctypes
import mmap
import os
import struct

import numpy as np

from automl_amd import _lib

OK, TRUNCATED_HEADER, TRUNCATED_PAYLOAD, LENGTH_CRC, DATA_CRC, LENGTH_RANGE, CAPACITY = range(7)
FRAMING = {
    TRUNCATED_HEADER: 'the file ends inside a record header',
    TRUNCATED_PAYLOAD: 'the file ends inside a record',
    LENGTH_CRC: 'the checksum of the length field does not match',
    DATA_CRC: 'the checksum of the record does not match',
    LENGTH_RANGE: 'a record length (not verified) that runs past the end of the file',
}
BYTES, FLOAT, INT64 = 1, 2, 3
E_OK, E_VARINT, E_LENGTH, E_WIRE_TYPE, E_CAPACITY, E_KIND = range(6)
PARSING = {
    E_VARINT: 'a malformed varint',
    E_LENGTH: 'a length that runs past the end of its message',
    E_WIRE_TYPE: 'a wrong wire type',
    E_CAPACITY: 'a list longer than its capacity',
    E_KIND: 'a wanted key holds another kind of list',
}
MAX_THREADS = 16
INDEX_CHUNK = 256       # records indexed (and their CRCs checked) per call while a file is walked
PARSE_RECORDS_PER_THREAD = 64

Spec = collections.namedtuple('Spec', 'key kind capacity')
Parsed = collections.namedtuple('Parsed', 'values counts status')


class TFRecordError(ValueError):
  """A file that cannot be read as records, or a record that cannot be read as an Example: .path, .record, .offset, .status."""

  def __init__(self, message, path=None, record=None, offset=None, status=None):
    super().__init__(message)
    self.path, self.record, self.offset, self.status = path, record, offset, status


def crc32c(data, crc=0):
  """CRC-32C of bytes-like `data`, continuing from `crc` (edet_crc32c)."""
  buf = np.frombuffer(memoryview(data).cast('B'), np.uint8)
  c = ctypes.c_uint32(int(crc) & 0xffffffff)
  _lib.call('edet_crc32c', buf.ctypes.data if buf.size else None, buf.size, ctypes.byref(c))
  return int(c.value)


def mask_crc(crc):
  """crc32c::Mask, as the record framing stores its checksums."""
  return (((crc >> 15) | (crc << 17)) + 0xa282ead8) & 0xffffffff


def index_buffer(buf, verify=True, capacity=INDEX_CHUNK, base=0):
  """edet_tfrecord_index on a uint8 array from byte `base` on -> (offsets, lengths, status, consumed): the payload offsets
  (absolute) and lengths of up to `capacity` records, the status the walk ended with, and the offset it is about."""
  lib = _lib.load()
  offsets, lengths = np.zeros(capacity, np.uint64), np.zeros(capacity, np.uint64)
  count, consumed = ctypes.c_size_t(0), ctypes.c_size_t(0)
  n = buf.size - base
  status = lib.edet_tfrecord_index(buf.ctypes.data + base if n > 0 else None, max(n, 0), int(bool(verify)), offsets.ctypes.data,
                                   lengths.ctypes.data, capacity, ctypes.byref(count), ctypes.byref(consumed))
  if status < 0:
    raise _lib.EdetError('edet_tfrecord_index failed: %s' % lib.edet_last_error().decode())
  return offsets[:count.value] + np.uint64(base), lengths[:count.value], status, base + consumed.value


class TFRecordFile(object):
  """The records of one TFRecord file.  The file is mapped, not read: iterating yields a read-only memoryview of each payload
  inside the mapping, and record i is file[i].  The framing is walked, and with `verify` both checksums of every record are
  checked, INDEX_CHUNK records at a time as far as the records asked for; len() walks to the end.  A file that is not
  well-formed raises TFRecordError naming the file, the record index and the byte offset."""

  def __init__(self, path, verify=True):
    self.path, self.verify = str(path), bool(verify)
    self._offsets, self._lengths = [], []
    self._pos, self._done = 0, False
    size = os.path.getsize(self.path)
    with open(self.path, 'rb') as f:
      self._map = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if size else None
    self._view = memoryview(self._map) if size else memoryview(b'')
    self._array = np.frombuffer(self._view, np.uint8)
    self._done = size == 0

  def _more(self):
    offsets, lengths, status, consumed = index_buffer(self._array, self.verify, INDEX_CHUNK, self._pos)
    self._offsets.extend(int(v) for v in offsets)
    self._lengths.extend(int(v) for v in lengths)
    self._pos = consumed
    if status == OK:
      self._done = True
    elif status != CAPACITY:
      record = len(self._offsets)
      what = FRAMING[status]
      if status in (LENGTH_CRC, LENGTH_RANGE) and record == 0 and bytes(self._view[:2]) in (b'\x1f\x8b', b'\x78\x01', b'\x78\x5e', b'\x78\x9c', b'\x78\xda'):
        what += ': the file starts like a gzip or zlib stream, and compressed TFRecord files are not read'
      raise TFRecordError('%s: record %d at byte offset %d: %s' % (self.path, record, consumed, what), self.path, record,
                          consumed, status)

  def __len__(self):
    while not self._done:
      self._more()
    return len(self._offsets)

  def __getitem__(self, i):
    i = int(i)
    while i >= len(self._offsets) and not self._done:
      self._more()
    if i < 0 or i >= len(self._offsets):
      raise IndexError('%s: record %d of %d' % (self.path, i, len(self._offsets)))
    return self._view[self._offsets[i]:self._offsets[i] + self._lengths[i]]

  def has(self, i):
    """Whether record i exists, walking no further than needed."""
    while i >= len(self._offsets) and not self._done:
      self._more()
    return i < len(self._offsets)

  def offset(self, i):
    """The byte offset of record i's payload."""
    self[i]
    return self._offsets[i]

  def __iter__(self):
    i = 0
    while self.has(i):
      yield self[i]
      i += 1

  def close(self):
    """Unmaps the file; memoryviews handed out before must have been released (else the mapping stays until they are)."""
    self._array = None
    try:
      self._view.release()
      if self._map is not None:
        self._map.close()
    except BufferError:
      pass
    self._map = None

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()


# ---------------------------------------------------------------------------------------------------------- writing
def _varint(out, v):
  v &= (1 << 64) - 1
  while v >= 0x80:
    out.append((v & 0x7f) | 0x80)
    v >>= 7
  out.append(v)


def _field(out, number, payload):
  """One length-delimited field."""
  _varint(out, (number << 3) | 2)
  _varint(out, len(payload))
  out += payload


def encode_feature(value):
  """One Feature message: bytes / str, or a list of them -> bytes_list; a float array or list -> packed float_list (float32
  bits as given); an integer or bool array or list -> packed int64_list.  An empty list is a Feature with no member set."""
  if isinstance(value, str):
    value = value.encode('utf-8')
  if isinstance(value, (bytes, bytearray, memoryview)):
    value = [bytes(value)]
  if isinstance(value, (list, tuple)) and value and all(isinstance(v, (bytes, bytearray, memoryview, str)) for v in value):
    inner = bytearray()
    for v in value:
      _field(inner, 1, v.encode('utf-8') if isinstance(v, str) else bytes(v))
    out = bytearray()
    _field(out, 1, inner)
    return bytes(out)
  a = np.asarray(value)
  if a.size == 0:
    return b''
  if a.dtype.kind == 'f':
    inner = bytearray()
    _field(inner, 1, a.astype('<f4').reshape(-1).tobytes())
    out = bytearray()
    _field(out, 2, inner)
    return bytes(out)
  if a.dtype.kind in 'iub':
    packed = bytearray()
    for v in a.reshape(-1).tolist():
      _varint(packed, int(v))
    inner = bytearray()
    _field(inner, 1, packed)
    out = bytearray()
    _field(out, 3, inner)
    return bytes(out)
  raise ValueError('a feature is bytes, str, or a float or integer array, got %s' % (a.dtype,))


def encode_example(features):
  """{key: value} -> a serialized tf.train.Example (encode_feature per value), the keys in sorted order so that equal
  dictionaries give equal bytes."""
  feats = bytearray()
  for key in sorted(features):
    entry = bytearray()
    _field(entry, 1, key.encode('utf-8') if isinstance(key, str) else bytes(key))
    _field(entry, 2, encode_feature(features[key]))
    _field(feats, 1, entry)
  out = bytearray()
  _field(out, 1, feats)
  return bytes(out)


class TFRecordWriter(object):
  """Writes records in the TFRecord framing: write(record) takes bytes (encode_example's, or anything else)."""

  def __init__(self, path):
    self.path = str(path)
    self._f = open(self.path, 'wb')

  def write(self, record):
    record = bytes(record)
    head = struct.pack('<Q', len(record))
    self._f.write(head + struct.pack('<I', mask_crc(crc32c(head))) + record + struct.pack('<I', mask_crc(crc32c(record))))

  def close(self):
    if self._f is not None:
      self._f.close()
      self._f = None

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()


# ---------------------------------------------------------------------------------------------------------- parsing
_KINDS = {'bytes': BYTES, 'float': FLOAT, 'int64': INT64, BYTES: BYTES, FLOAT: FLOAT, INT64: INT64}
_DTYPES = {BYTES: np.int64, FLOAT: np.float32, INT64: np.int64}


def parse_examples(records, spec, threads=None):
  """records: serialized Examples (bytes, or memoryviews such as TFRecordFile yields; contiguous); spec: (key, kind,
  capacity) triples, kind 'bytes', 'float' or 'int64' -> Parsed(values, counts, status): values[key] is int64 [n, capacity,
  2] (offset, length) spans into the record for bytes, float32 / int64 [n, capacity] otherwise; counts[key] int32 [n], -1
  where the record does not have the key; status int32 [n], E_* per record -- nothing raises for a malformed record here.
  threads: 1 .. 16, never taken from the machine's core count; default one per PARSE_RECORDS_PER_THREAD records -- the image
  bytes are skipped, not read, so a detection record costs about a microsecond and a thread's start many times that."""
  lib = _lib.load()
  spec = [Spec(k.encode('utf-8') if isinstance(k, str) else bytes(k), _KINDS[kind], int(cap)) for k, kind, cap in spec]
  n, ns = len(records), len(spec)
  if threads is None:
    threads = max(1, min(MAX_THREADS, n // PARSE_RECORDS_PER_THREAD))
  threads = int(threads)
  if threads < 1 or threads > MAX_THREADS:
    raise ValueError('threads %d outside 1 .. %d' % (threads, MAX_THREADS))
  arrays = [np.frombuffer(memoryview(r).cast('B'), np.uint8) for r in records]      # views, not copies
  ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrays])
  sizes = (ctypes.c_size_t * max(n, 1))(*[a.size for a in arrays])
  cspec = (_lib.ExampleSpec * max(ns, 1))()
  values = []
  for k, s in enumerate(spec):
    cspec[k].key, cspec[k].key_len, cspec[k].kind, cspec[k].capacity = s.key, len(s.key), s.kind, s.capacity
    values.append(np.zeros((n, s.capacity, 2) if s.kind == BYTES else (n, s.capacity), _DTYPES[s.kind]))
  vptrs = (ctypes.c_void_p * max(ns, 1))(*[v.ctypes.data if v.size else None for v in values])
  counts = np.full((n, ns), -1, np.int32)
  status = np.zeros(n, np.int32)
  rc = lib.edet_example_parse(ptrs, sizes, n, cspec, ns, threads, vptrs, counts.ctypes.data, status.ctypes.data)
  if rc != 0:
    raise _lib.EdetError('edet_example_parse failed (%d): %s' % (rc, lib.edet_last_error().decode()))
  names = [s.key.decode('utf-8') for s in spec]
  return Parsed(dict(zip(names, values)), {name: counts[:, k] for k, name in enumerate(names)}, status)
