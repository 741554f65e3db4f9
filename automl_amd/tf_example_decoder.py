"""object_detection/tf_example_decoder.py:30-169 for batches of serialized tf.train.Example records, on the host
(tfrecord.parse_examples on csrc/tfrecord_host.cpp): the detection keys of the reference's shards -> per record the encoded
image bytes (a span inside the record, not a copy, and NOT decoded: jpeg.JpegDecoder takes it from here), source id, height,
width, boxes, classes, crowd flags and areas, by the reference's rules:

  image/encoded                required; a record without it is an error naming the key
  image/source_id              default ''
  image/height, image/width    default -1, and then BOTH are read from the image's frame header (jpeg.jpeg_info; :129-138)
  image/object/bbox/{ymin,xmin,ymax,xmax}   stacked [n, 4] float32, the stored bits; four lists of one length, else an error
  image/object/class/label     int64 [n]
  image/object/is_crowd        the list != 0, of the classes' length; an empty list is all False (:140-143)
  image/object/area            the stored list when it is not empty, else (xmax - xmin) * (ymax - ymin) in float32 (:84-92)

A deliberate difference: for an empty source id the reference stores a FarmHash fingerprint of the image bytes
(_get_source_id_from_encoded_image, :22-27, :147-150).  That fingerprint is not built; the id stays '', which
det_input.parse_source_ids maps to -1.  Not built, refused by name: include_mask (PNG instance masks, :49-53, :67-82) and
regenerate_source_id (:144-145)."""
import numpy as np

from automl_amd import jpeg
from automl_amd import tfrecord

KEYS = (('image/encoded', 'bytes'), ('image/source_id', 'bytes'), ('image/height', 'int64'), ('image/width', 'int64'),
        ('image/object/bbox/xmin', 'float'), ('image/object/bbox/xmax', 'float'), ('image/object/bbox/ymin', 'float'),
        ('image/object/bbox/ymax', 'float'), ('image/object/class/label', 'int64'), ('image/object/area', 'float'),
        ('image/object/is_crowd', 'int64'))
SCALARS = ('image/encoded', 'image/source_id', 'image/height', 'image/width')
LIST_CAPACITY = 128      # rows per list of the first pass; a record with longer lists is parsed again at its own bound


class TfExampleDecoder(object):
  """decode(records) -> one dictionary per record: 'image' (memoryview of the encoded bytes), 'source_id' (str), 'height',
  'width' (int), 'groundtruth_classes' int64 [n], 'groundtruth_is_crowd' bool [n], 'groundtruth_area' float32 [n],
  'groundtruth_boxes' float32 [n, 4] (ymin, xmin, ymax, xmax).  A record that cannot be decoded raises tfrecord.TFRecordError
  (a ValueError) whose .record is its index in the batch."""

  def __init__(self, include_mask=False, regenerate_source_id=False):
    if include_mask:
      raise ValueError('include_mask=True is not built: instance masks are PNG files decoded per object '
                       '(object_detection/tf_example_decoder.py:49-53, :67-82)')
    if regenerate_source_id:
      raise ValueError('regenerate_source_id=True is not built: the id would be a FarmHash fingerprint of the image bytes '
                       '(object_detection/tf_example_decoder.py:22-27, :144-145)')

  def _parse(self, records, threads):
    spec = [(k, kind, 1 if k in SCALARS else LIST_CAPACITY) for k, kind in KEYS]
    parsed = tfrecord.parse_examples(records, spec, threads)
    again = [i for i, s in enumerate(parsed.status) if s == tfrecord.E_CAPACITY]
    out = [(parsed, i) for i in range(len(records))]
    for i in again:      # a value takes at least one byte of its record
      bound = max(len(records[i]), 1)
      one = tfrecord.parse_examples([records[i]], [(k, kind, 1 if k in SCALARS else bound) for k, kind in KEYS], 1)
      out[i] = (one, 0)
    return out

  def decode(self, records, threads=None):
    records = list(records)
    result = []
    for i, (p, at) in enumerate(self._parse(records, threads)):
      status = int(p.status[at])
      if status != tfrecord.E_OK:
        raise tfrecord.TFRecordError('record %d is not a tf.train.Example that can be read: %s (status %d)'
                                     % (i, tfrecord.PARSING[status], status), record=i, status=status)

      def values(key):
        n = int(p.counts[key][at])
        return p.values[key][at, :max(n, 0)]
      if p.counts['image/encoded'][at] < 1:
        raise tfrecord.TFRecordError("record %d has no 'image/encoded' feature" % i, record=i)
      offset, length = (int(v) for v in p.values['image/encoded'][at, 0])
      image = memoryview(records[i]).cast('B')[offset:offset + length]
      source_id = ''
      if p.counts['image/source_id'][at] >= 1:
        o, n = (int(v) for v in p.values['image/source_id'][at, 0])
        try:
          source_id = bytes(memoryview(records[i]).cast('B')[o:o + n]).decode('utf-8')
        except UnicodeDecodeError as e:
          raise tfrecord.TFRecordError("record %d: 'image/source_id' is not UTF-8 text: %s" % (i, e), record=i)
      height = int(values('image/height')[0]) if p.counts['image/height'][at] >= 1 else -1
      width = int(values('image/width')[0]) if p.counts['image/width'][at] >= 1 else -1
      if height == -1 or width == -1:
        try:
          info = jpeg.jpeg_info(image)
        except ValueError as e:
          raise tfrecord.TFRecordError("record %d stores no 'image/height' / 'image/width' and its image has no frame "
                                       'header to take them from: %s' % (i, e), record=i)
        height, width = info.height, info.width
      ymin, xmin, ymax, xmax = (values('image/object/bbox/' + k) for k in ('ymin', 'xmin', 'ymax', 'xmax'))
      if not ymin.size == xmin.size == ymax.size == xmax.size:
        raise tfrecord.TFRecordError('record %d: the box lists have %d, %d, %d and %d entries (ymin, xmin, ymax, xmax)'
                                     % (i, ymin.size, xmin.size, ymax.size, xmax.size), record=i)
      boxes = np.stack([ymin, xmin, ymax, xmax], axis=-1)
      classes = values('image/object/class/label').copy()
      crowd = values('image/object/is_crowd')
      if crowd.size == 0:
        is_crowd = np.zeros(classes.shape, bool)
      elif crowd.size != classes.size:
        raise tfrecord.TFRecordError('record %d: %d crowd flags for %d classes' % (i, crowd.size, classes.size), record=i)
      else:
        is_crowd = crowd != 0
      area = values('image/object/area')
      area = area.copy() if area.size else (xmax - xmin) * (ymax - ymin)
      result.append({'image': image, 'source_id': source_id, 'height': height, 'width': width, 'groundtruth_classes': classes,
                     'groundtruth_is_crowd': is_crowd, 'groundtruth_area': area, 'groundtruth_boxes': boxes})
    return result
