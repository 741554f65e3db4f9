"""Pure-Python restatement of the TFRecord input path, for tests/test_tfrecord.py and tests/test_dataloader.py: the
tf.train.Example parser over tf_checkpoint._parse_proto, the rules of object_detection/tf_example_decoder.py:30-169, the
padding of dataloader.py:289-306, :345-353, and the record order automl_amd/dataloader.py defines.  Nothing here calls the
library.  Floats are carried as their uint32 bit patterns."""
import struct

import numpy as np

from automl_amd import tf_checkpoint as tc
from tests import jpeg_ref

BYTES, FLOAT, INT64 = 1, 2, 3
OK, VARINT, LENGTH, WIRE_TYPE, CAPACITY, KIND = range(6)
KIND_OF = {'bytes': BYTES, 'float': FLOAT, 'int64': INT64}


class Refused(Exception):
  def __init__(self, status):
    super().__init__(status)
    self.status = status


MAX_GROUP_DEPTH = 32


def _skip_group(data, pos, number, depth=0):
  """pos: behind a start-group tag of field `number` -> the position behind its end-group tag.  Protobuf skips an unknown
  group field by field; _parse_proto does not know groups, so they are cut out in front of it (without_groups)."""
  if depth >= MAX_GROUP_DEPTH:
    raise Refused(WIRE_TYPE)
  while True:
    if pos >= len(data):
      raise Refused(LENGTH)      # the message ends inside the group
    try:
      tag, pos = tc._get_varint(data, pos)
      field, wt = tag >> 3, tag & 7
      if wt == 4:
        if field != number:
          raise Refused(WIRE_TYPE)
        return pos
      if wt == 0:
        _, pos = tc._get_varint(data, pos)
      elif wt == 2:
        n, pos = tc._get_varint(data, pos)
    except (IndexError, ValueError):
      raise Refused(VARINT)
    if wt == 3:
      pos = _skip_group(data, pos, field, depth + 1)
    elif wt in (1, 2, 5):
      width = 8 if wt == 1 else 4 if wt == 5 else n
      if width > len(data) - pos:
        raise Refused(LENGTH)
      pos += width
    elif wt != 0:
      raise Refused(WIRE_TYPE)


def without_groups(buf):
  """The message with its groups cut out; what is left is what _parse_proto reads."""
  out = []
  for field, wt, start, n, at, end in _walk(bytes(buf)):
    if wt != 3:
      out.append(bytes(buf)[at:end])
  return b''.join(out)


def fields(buf):
  """tf_checkpoint._parse_proto with its failures named as the library names them."""
  buf = without_groups(buf)
  try:
    return tc._parse_proto(bytes(buf))
  except IndexError:
    raise Refused(VARINT)      # a varint cut off by the end of the message
  except struct.error:
    raise Refused(LENGTH)
  except ValueError as e:
    raise Refused(VARINT if 'varint' in str(e) else LENGTH if 'truncated' in str(e) else WIRE_TYPE)


def _signed(v):
  return tc._signed64(v & ((1 << 64) - 1))


def _list(buf, kind, base):
  """One BytesList / FloatList / Int64List -> its values: (offset, length) spans, uint32 bits, or signed integers.  `base` is
  where buf starts inside the record."""
  out = []
  if kind == BYTES:      # _parse_proto copies payloads; the spans come from the walk that keeps positions
    for field, wt, start, n in _spans(buf, base):
      if field == 1:
        if wt != 2:
          raise Refused(WIRE_TYPE)
        out.append((start, n))
    return out
  for field, wt, v in fields(buf):
    if field != 1:
      continue
    if kind == FLOAT and wt == 5:
      out.append(v)
    elif kind == FLOAT and wt == 2:
      if len(v) % 4:
        raise Refused(LENGTH)
      out.extend(struct.unpack('<%dI' % (len(v) // 4), v))
    elif kind == INT64 and wt == 0:
      out.append(_signed(v))
    elif kind == INT64 and wt == 2:
      pos = 0
      while pos < len(v):
        try:
          x, pos = tc._get_varint(v, pos)
        except (IndexError, ValueError):
          raise Refused(VARINT)
        out.append(_signed(x))
    else:
      raise Refused(WIRE_TYPE)
  return out


def _walk(data):
  """The fields of one message: (field, wire type, payload start, payload length, field start, field end); start and length
  are None unless the field is length-delimited.  A group comes as one entry of wire type 3."""
  pos = 0
  while pos < len(data):
    at = pos
    try:
      tag, pos = tc._get_varint(data, pos)
      field, wt = tag >> 3, tag & 7
      if wt == 0:
        _, pos = tc._get_varint(data, pos)
        yield field, wt, None, None, at, pos
        continue
      if wt == 2:
        n, pos = tc._get_varint(data, pos)
    except (IndexError, ValueError):
      raise Refused(VARINT)
    if wt == 1 or wt == 5:
      width = 8 if wt == 1 else 4
      if len(data) - pos < width:
        raise Refused(LENGTH)
      pos += width
      yield field, wt, None, None, at, pos
    elif wt == 2:
      if n > len(data) - pos:
        raise Refused(LENGTH)
      pos += n
      yield field, wt, pos - n, n, at, pos
    elif wt == 3:
      pos = _skip_group(data, pos, field)
      yield field, wt, None, None, at, pos
    else:
      raise Refused(WIRE_TYPE)


def _spans(buf, base):
  """The fields of one message with the positions _parse_proto does not keep: [(field, wire type, start in the record,
  length)], start and length None for the wire types that are not length-delimited (a group is one such entry)."""
  return [(field, wt, None if start is None else base + start, n) for field, wt, start, n, _, _ in _walk(bytes(buf))]


def parse_example(record, spec):
  """record: one serialized Example; spec: [(key, kind name, capacity)] -> {key: list of values, or None for an absent key}.
  Raises Refused(status).  The walk is the library's: fields in stream order, a wanted key's Feature parsed where it stands,
  an unwanted one skipped unread, the last entry of a repeated key winning."""
  record = bytes(record)
  want = {(k.encode() if isinstance(k, str) else k): (k, KIND_OF[kind], cap) for k, kind, cap in spec}
  out = {k: None for k, _, _ in spec}
  for field, wt, start, n in _spans(record, 0):
    if field != 1:
      continue
    if wt != 2:
      raise Refused(WIRE_TYPE)
    for field2, wt2, start2, n2 in _spans(record[start:start + n], start):
      if field2 != 1:
        continue
      if wt2 != 2:
        raise Refused(WIRE_TYPE)
      key, value = b'', (start2, 0)
      for field3, wt3, start3, n3 in _spans(record[start2:start2 + n2], start2):
        if field3 not in (1, 2):
          continue
        if wt3 != 2:
          raise Refused(WIRE_TYPE)
        if field3 == 1:
          key = record[start3:start3 + n3]
        else:
          value = (start3, n3)
      if key not in want:
        continue
      name, kind, cap = want[key]
      values, member = [], 0
      for field4, wt4, start4, n4 in _spans(record[value[0]:value[0] + value[1]], value[0]):
        if field4 not in (1, 2, 3):
          continue
        if wt4 != 2:
          raise Refused(WIRE_TYPE)
        if field4 != member:
          values = []
        member = field4
        if field4 == kind:
          values += _list(record[start4:start4 + n4], kind, start4)
          if len(values) > cap:
            raise Refused(CAPACITY)
      if member and member != kind:
        raise Refused(KIND)
      out[name] = values
  return out


def status_of(record, spec):
  try:
    parse_example(record, spec)
    return OK
  except Refused as e:
    return e.status


# ------------------------------------------------------------------------------------------------ the decoder's rules
KEYS = (('image/encoded', 'bytes'), ('image/source_id', 'bytes'), ('image/height', 'int64'), ('image/width', 'int64'),
        ('image/object/bbox/xmin', 'float'), ('image/object/bbox/xmax', 'float'), ('image/object/bbox/ymin', 'float'),
        ('image/object/bbox/ymax', 'float'), ('image/object/class/label', 'int64'), ('image/object/area', 'float'),
        ('image/object/is_crowd', 'int64'))


def _f32(bits):
  return np.asarray(bits or [], np.uint32).view(np.float32)


def decode(record):
  """tf_example_decoder.TfExampleDecoder.decode of one record, the image left encoded (bytes)."""
  record = bytes(record)
  p = parse_example(record, [(k, kind, len(record) + 1) for k, kind in KEYS])
  if not p['image/encoded']:
    raise ValueError("no 'image/encoded'")
  o, n = p['image/encoded'][0]
  image = record[o:o + n]
  source_id = ''
  if p['image/source_id']:
    o, n = p['image/source_id'][0]
    source_id = record[o:o + n].decode('utf-8')
  height = p['image/height'][0] if p['image/height'] else -1
  width = p['image/width'][0] if p['image/width'] else -1
  if height == -1 or width == -1:
    info = jpeg_ref.info(image)
    height, width = info.height, info.width
  ymin, xmin, ymax, xmax = (_f32(p['image/object/bbox/' + k]) for k in ('ymin', 'xmin', 'ymax', 'xmax'))
  if len({ymin.size, xmin.size, ymax.size, xmax.size}) != 1:
    raise ValueError('box lists of unequal lengths')
  classes = np.asarray(p['image/object/class/label'] or [], np.int64)
  crowd = np.asarray(p['image/object/is_crowd'] or [], np.int64)
  if crowd.size == 0:
    crowd = np.zeros(classes.shape, bool)
  elif crowd.size != classes.size:
    raise ValueError('crowd flags and classes of unequal lengths')
  else:
    crowd = crowd != 0
  area = _f32(p['image/object/area'])
  if area.size == 0:
    area = (xmax - xmin) * (ymax - ymin)
  return {'image': image, 'source_id': source_id, 'height': int(height), 'width': int(width), 'groundtruth_classes': classes,
          'groundtruth_is_crowd': crowd, 'groundtruth_area': area.astype(np.float32),
          'groundtruth_boxes': np.stack([ymin, xmin, ymax, xmax], -1)}


def pad_batch(decoded, is_training, skip_crowd, max_instances=100):
  """dataloader.py:289-306, :340-353 on decoded records -> (boxes, classes, counts, is_crowds, areas, source_ids)."""
  b, m = len(decoded), max_instances
  boxes, classes = np.full((b, m, 4), -1, np.float32), np.full((b, m), -1, np.float32)
  is_crowds, areas, counts = np.zeros((b, m), np.float32), np.full((b, m), -1, np.float32), np.zeros(b, np.int32)
  ids = np.zeros(b, np.float32)
  for i, d in enumerate(decoded):
    bx, cl = d['groundtruth_boxes'], d['groundtruth_classes']
    if is_training and skip_crowd:
      keep = [k for k in range(cl.size) if not d['groundtruth_is_crowd'][k]]
      bx, cl = bx[keep], cl[keep]
    if bx.shape[0] > m:
      raise ValueError('more rows than max_instances_per_image')
    for k in range(bx.shape[0]):
      boxes[i, k] = bx[k]
      classes[i, k] = np.float32(cl[k])
    counts[i] = bx.shape[0]
    if not is_training:
      is_crowds[i, :cl.size] = d['groundtruth_is_crowd'].astype(np.float32)
      areas[i, :cl.size] = d['groundtruth_area']
    ids[i] = np.float32(-1.0 if d['source_id'] == '' else float(d['source_id']))
  return boxes, classes, counts, is_crowds, areas, ids


# ------------------------------------------------------------------------------------------------ the order
def epoch_interleave(files, sizes, cycle=16):
  """files: the epoch's file list; sizes[f]: records of file f -> the round-robin sequence of (file, record)."""
  slots = [[f, 0] for f in files[:min(cycle, len(files))]]
  waiting = list(files[len(slots):])
  out = []
  turn = 0
  while any(s is not None for s in slots):
    s = slots[turn]
    if s is not None and s[1] >= sizes[s[0]]:      # ended: the next file of the list takes its place and its turn
      slots[turn] = s = [waiting.pop(0), 0] if waiting else None
      if s is not None:
        continue
    if s is not None:
      out.append((s[0], s[1]))
      s[1] += 1
    turn = (turn + 1) % len(slots)
  return out


def batches(sizes, batch, training, seed, epochs, drop_remainder, buffer=64):
  """The [(file, record)] lists of `epochs` epochs (one pass when not training: no permutation, no shuffle buffer)."""
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(epochs if training else 1):
    files = [int(v) for v in rng.permutation(len(sizes))] if training else list(range(len(sizes)))
    seq = epoch_interleave(files, sizes)
    if training:
      held, rest, emitted = seq[:buffer], seq[buffer:], []
      while held:
        j = int(rng.integers(len(held)))
        emitted.append(held[j])
        if rest:
          held[j] = rest.pop(0)
        else:
          held[j] = held[-1]
          held.pop()
      seq = emitted
    for at in range(0, len(seq), batch):
      if at + batch <= len(seq) or not drop_remainder:
        out.append(seq[at:at + batch])
  return out


# ------------------------------------------------------------------------------------------------ hand encoders for the tests
def varint(v):
  out = bytearray()
  tc._put_varint(out, v)
  return bytes(out)


def ld(field, payload):
  """One length-delimited field."""
  return varint(field << 3 | 2) + varint(len(payload)) + bytes(payload)


def float_list(bits, mode='packed'):
  """A FloatList of uint32 bit patterns: 'packed', 'unpacked', or 'mixed' (the first half packed, the rest one by one)."""
  bits = [int(b) for b in bits]
  cut = {'packed': len(bits), 'unpacked': 0, 'mixed': len(bits) // 2}[mode]
  out = ld(1, struct.pack('<%dI' % cut, *bits[:cut])) if cut or mode == 'packed' else b''
  for b in bits[cut:]:
    out += varint(1 << 3 | 5) + struct.pack('<I', b)
  return out


def int64_list(values, mode='packed'):
  values = [int(v) for v in values]
  cut = {'packed': len(values), 'unpacked': 0, 'mixed': len(values) // 2}[mode]
  out = ld(1, b''.join(varint(v) for v in values[:cut])) if cut or mode == 'packed' else b''
  for v in values[cut:]:
    out += varint(1 << 3 | 0) + varint(v)
  return out


def bytes_list(values):
  return b''.join(ld(1, v) for v in values)


def feature(member, payload):
  """member: 1 bytes_list, 2 float_list, 3 int64_list, 0 a Feature with nothing set."""
  return ld(member, payload) if member else b''


def example(entries, unknown=b'', features_unknown=b''):
  """entries: [(key, Feature bytes)] in the order given (a key may repeat); unknown / features_unknown: raw fields put in
  front of the features field and in front of the map entries."""
  feats = features_unknown + b''.join(ld(1, ld(1, k.encode() if isinstance(k, str) else k) + ld(2, f)) for k, f in entries)
  return unknown + ld(1, feats)


def frame(record, crc32c, mask_crc):
  """One record in the TFRecord framing, by the CRC functions handed in."""
  head = struct.pack('<Q', len(record))
  return head + struct.pack('<I', mask_crc(crc32c(head))) + record + struct.pack('<I', mask_crc(crc32c(record)))
