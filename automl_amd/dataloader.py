"""dataloader.InputReader (dataloader.py:236-460) on MI355X: TFRecord shards of tf.train.Example protos -> the raw batches
that train_step_raw, test_step_raw and eval_lib.evaluate take.

  reader = InputReader('/data/coco/train-*.tfrecord', is_training=True)
  for batch in reader(config.as_dict(), batch_size=128, canvas=(640, 640)):
    model.train_step_raw(batch)

The stage is split as the JPEG decoder is.  File reads (mmap), record framing, CRC-32C and protobuf parsing are serial byte
work: they run on the host (tfrecord.py, tf_example_decoder.py on csrc/tfrecord_host.cpp), on ONE background thread that
stays up to `depth` batches ahead (ctypes releases the GIL); `threads` bounds the workers of a batch's parse and of the
decoder's Huffman stage (1 .. 16, never the machine's core count).  Everything behind them is the device's and stays on the
consumer's thread: the reader owns one jpeg.JpegDecoder(batch, Hc, Wc, depth=depth), hands it the image spans as memoryviews
into the mapped files -- the Huffman workers read them where they lie, no image byte is copied on the way -- and yields its
(raw, sizes) with the padded annotation arrays.  Iterating makes no HIP call of its own.  The one wait for the device is the
decoder's own: a set of pinned arenas is written again only behind the event of its last copy, `depth` batches earlier.

Batches.  Training: ((raw, sizes), boxes [B, M, 4], classes [B, M], counts [B]).  Evaluation: ((raw, sizes), boxes, classes,
counts, is_crowds [B, M], areas [B, M], source_ids [B]).  M = max_instances_per_image or 100; boxes float32 normalised (ymin,
xmin, ymax, xmax) padded with -1, classes float32 padded with -1, is_crowds float32 padded with 0, areas float32 padded with -1
(dataloader.py:345-353), counts int32, source_ids float32 with -1 for an empty id (:340-342).  With is_training and
params['skip_crowd_during_training'] the crowd rows leave boxes and classes first, in order (:303-306).  More than M rows
raise, naming the file and the record.  params['drop_remainder'] decides about a short last batch; a short batch gets a
decoder of its own size.  Training repeats for ever, batches never straddle an epoch (batch before repeat, :449-454);
evaluation makes one pass.  use_fake_data yields the first batch again and again (:455-459).

Ordering is this project's definition -- tf.data's shuffle, interleave and AUTOTUNE order is pinned nowhere:
  files      sorted(glob(file_pattern)); shard=(n, i) keeps files[i::n] of it (dataset.shard on the file list, :424-426)
  epochs     when training, the list is permuted per epoch by one numpy generator seeded from params['tf_random_seed']
  interleave min(16, len(files)) files are open; they are read round-robin, one record each; a file that has ended is
             replaced by the next of the list at once, and that file takes the turn
  shuffle    when training, 64 records: the buffer is filled, an index drawn uniformly from the same generator, that record
             emitted and its place taken by the next one (by the last of the buffer once the files have ended)
  Evaluation, and debug=True, is the interleave order of the sorted list with no shuffling at all.
get_state() / set_state() of the iterator return and restore the epoch, the file list and positions, the buffer by (file,
record) and the generator's state as of the last batch it yielded, so a resumed run goes on with the same stream.

Refused with a reason: dataset_type='sstable', a 'segmentation' head (instance masks are not built), compressed TFRecord
files, a pattern that matches nothing, regenerate_source_id."""
import collections
import copy
import glob
import queue
import threading

import numpy as np

from automl_amd import det_input
from automl_amd import tf_example_decoder
from automl_amd import tfrecord

CYCLE_LENGTH = 16
SHUFFLE_BUFFER = 64
MAX_OPEN_FILES = 2 * CYCLE_LENGTH

HostBatch = collections.namedtuple('HostBatch', 'index images boxes classes counts is_crowds areas source_ids state')


class RecordOrder(object):
  """The (file, record) stream of the module's docstring.  has(file, record) tells whether a file has that record; next() is
  the next pair, or None at the end of each epoch (`finished` is then set unless the stream repeats)."""

  def __init__(self, num_files, has, shuffle, seed, repeat):
    self.num_files, self.has, self.shuffle, self.repeat = int(num_files), has, bool(shuffle), bool(repeat)
    self.rng = np.random.default_rng(seed)
    self.epoch = 0
    self.live = False      # inside an epoch
    self.finished = False
    self.perm, self.slots, self.buffer = [], [], []
    self.next_file = self.turn = self.emitted = 0
    self.drained = False

  def _begin(self):
    n = self.num_files
    self.perm = [int(v) for v in self.rng.permutation(n)] if self.shuffle else list(range(n))
    cycle = min(CYCLE_LENGTH, n)
    self.slots = [[self.perm[k], 0] for k in range(cycle)]
    self.next_file, self.turn, self.emitted = cycle, 0, 0
    self.buffer, self.drained, self.live = [], False, True

  def _sequential(self):
    """The interleave alone: the next pair of this epoch, None once every file has ended."""
    left = sum(s is not None for s in self.slots)
    while left:
      s = self.slots[self.turn]
      if s is not None:
        if self.has(s[0], s[1]):
          s[1] += 1
          self.turn = (self.turn + 1) % len(self.slots)
          return (s[0], s[1] - 1)
        if self.next_file < len(self.perm):
          self.slots[self.turn] = [self.perm[self.next_file], 0]
          self.next_file += 1
          continue      # the new file takes this turn
        self.slots[self.turn] = None
        left -= 1
      self.turn = (self.turn + 1) % len(self.slots)
    return None

  def next(self):
    if self.finished:
      return None
    if not self.live:
      self._begin()
    if not self.shuffle:
      out = self._sequential()
    else:
      while len(self.buffer) < SHUFFLE_BUFFER and not self.drained:
        r = self._sequential()
        if r is None:
          self.drained = True
        else:
          self.buffer.append(r)
      out = None
      if self.buffer:
        j = int(self.rng.integers(len(self.buffer)))
        out = self.buffer[j]
        r = None if self.drained else self._sequential()
        if r is None:
          self.drained = True
          self.buffer[j] = self.buffer[-1]
          self.buffer.pop()
        else:
          self.buffer[j] = r
    if out is None:
      if not self.emitted:
        raise ValueError('the files hold no record')
      self.live = False
      self.epoch += 1
      self.finished = not self.repeat
    else:
      self.emitted += 1
    return out

  def get_state(self):
    return copy.deepcopy({'epoch': self.epoch, 'live': self.live, 'finished': self.finished, 'perm': self.perm, 'slots': self.slots,
                          'buffer': self.buffer, 'next_file': self.next_file, 'turn': self.turn, 'emitted': self.emitted,
                          'drained': self.drained, 'rng': self.rng.bit_generator.state})

  def set_state(self, state):
    state = copy.deepcopy(state)
    self.rng.bit_generator.state = state.pop('rng')
    self.buffer = [tuple(r) for r in state.pop('buffer')]
    for k, v in state.items():
      setattr(self, k, v)


class _Producer(object):
  """The host half: the order, the open files, the decoder's parse and the padding; run() is the background thread's body.
  It refers to nothing of the iterator that owns it, so that iterator can be collected while the thread is alive."""

  def __init__(self, files, batch, is_training, shuffle, seed, skip_crowd, drop_remainder, max_instances, threads, verify):
    self.files, self.batch, self.is_training = files, int(batch), bool(is_training)
    self.skip_crowd, self.drop_remainder, self.max_instances = bool(skip_crowd), bool(drop_remainder), int(max_instances)
    self.threads, self.verify = threads, verify
    self.decoder = tf_example_decoder.TfExampleDecoder()
    self.open = collections.OrderedDict()
    self.views = {}      # (file, record) -> memoryview of records the shuffle buffer holds
    self.order = RecordOrder(len(files), self._has, shuffle, seed, repeat=is_training)

  def _file(self, f):
    got = self.open.get(f)
    if got is None:
      got = self.open[f] = tfrecord.TFRecordFile(self.files[f], self.verify)
      while len(self.open) > MAX_OPEN_FILES:
        self.open.popitem(last=False)[1].close()
    else:
      self.open.move_to_end(f)
    return got

  def open_first(self):
    """Opens the first file and walks to its first record, so that a compressed or damaged file is refused where the reader
    is made, not on the thread; the file and its index stay open for the thread."""
    self._file(0).has(0)

  def _has(self, f, r):
    file = self._file(f)
    if not file.has(r):
      return False
    self.views[(f, r)] = file[r]
    return True

  def _view(self, f, r):
    v = self.views.pop((f, r), None)
    return self._file(f)[r] if v is None else v      # (None: a buffer entry that came with set_state)

  def _where(self, f, r):
    return '%s: record %d at byte offset %d' % (self.files[f], r, self._file(f).offset(r))

  def next_batch(self):
    """The next HostBatch, None at the end of the stream."""
    order = self.order
    while True:
      index = []
      while len(index) < self.batch:
        pair = order.next()
        if pair is None:
          break
        index.append(pair)
      if len(index) == self.batch or (index and not self.drop_remainder):
        return self._assemble(index)
      for pair in index:      # a dropped remainder
        self.views.pop(pair, None)
      if order.finished:
        return None

  def _assemble(self, index):
    b, m = len(index), self.max_instances
    views = [self._view(f, r) for f, r in index]
    try:
      decoded = self.decoder.decode(views, self.threads)
    except tfrecord.TFRecordError as e:
      if e.record is None:
        raise
      f, r = index[e.record]
      raise tfrecord.TFRecordError('%s: %s' % (self._where(f, r), e), self.files[f], r, self._file(f).offset(r), e.status)
    boxes = np.full((b, m, 4), -1, np.float32)
    classes = np.full((b, m), -1, np.float32)
    is_crowds = np.zeros((b, m), np.float32)
    areas = np.full((b, m), -1, np.float32)
    counts = np.zeros(b, np.int32)
    for i, d in enumerate(decoded):
      bx, cl, cr, ar = d['groundtruth_boxes'], d['groundtruth_classes'], d['groundtruth_is_crowd'], d['groundtruth_area']
      if not bx.shape[0] == cl.size == ar.size:
        raise tfrecord.TFRecordError('%s: %d boxes, %d classes and %d areas' % (self._where(*index[i]), bx.shape[0], cl.size, ar.size),
                                     self.files[index[i][0]], index[i][1])
      if self.is_training and self.skip_crowd:      # dataloader.py:303-306, in front of everything else
        keep = np.logical_not(cr)
        bx, cl = bx[keep], cl[keep]
      n = max(bx.shape[0], 0 if self.is_training else cr.size)
      if n > m:
        raise tfrecord.TFRecordError('ERROR: please increase config.max_instances_per_image (%s has %d rows, max_instances_per_image '
                                     '%d; dataloader.pad_to_fixed_size)' % (self._where(*index[i]), n, m),
                                     self.files[index[i][0]], index[i][1])
      boxes[i, :bx.shape[0]] = bx
      classes[i, :cl.size] = cl.astype(np.float32)
      counts[i] = bx.shape[0]
      if not self.is_training:
        is_crowds[i, :cr.size] = cr.astype(np.float32)
        areas[i, :ar.size] = ar
    try:
      source_ids = det_input.parse_source_ids([d['source_id'] for d in decoded])
    except ValueError as e:
      raise tfrecord.TFRecordError('a source id that is not a number in one of %s: %s' % ([self._where(*p) for p in index], e))
    return HostBatch(index, [d['image'] for d in decoded], boxes, classes, counts, is_crowds, areas, source_ids,
                     self.order.get_state())

  def run(self, out, stop):
    def put(item):
      while not stop.is_set():
        try:
          out.put(item, timeout=0.05)
          return
        except queue.Full:
          pass
    try:
      while not stop.is_set():
        batch = self.next_batch()
        put(batch)
        if batch is None:
          return
    except BaseException as e:      # handed to the consumer, raised there
      put(e)


class HostReader(object):
  """Iterator over HostBatch: the host half alone, up to `depth` batches ahead on one background thread.  Needs no device.
  .index of a batch is its [(file, record)] list, .images the spans of the encoded images; get_state() / set_state() as the
  module's docstring says."""

  def __init__(self, producer, depth, fake):
    self._producer, self._depth, self._fake = producer, max(int(depth), 1), bool(fake)
    self.files = list(producer.files)      # what .index of a batch points into
    self._thread = self._queue = self._stop = None
    self._state = producer.order.get_state()
    self._first = None
    self._ended = False

  def _start(self):
    self._queue, self._stop = queue.Queue(self._depth), threading.Event()
    self._thread = threading.Thread(target=self._producer.run, args=(self._queue, self._stop), daemon=True)
    self._thread.start()

  def close(self):
    if self._thread is not None:
      self._stop.set()
      self._thread.join()
      self._thread = None

  def __del__(self):
    stop = getattr(self, '_stop', None)
    if stop is not None:
      stop.set()

  def __iter__(self):
    return self

  def __next__(self):
    if self._fake and self._first is not None:
      return self._first
    if self._ended:
      raise StopIteration
    if self._thread is None:
      self._start()
    item = self._queue.get()
    if item is None or isinstance(item, BaseException):
      self._ended = True
      self.close()
      if item is None:
        raise StopIteration
      raise item
    self._state = item.state
    if self._fake:
      self._first = item
      self.close()
    return item

  def get_state(self):
    return copy.deepcopy(self._state)

  def set_state(self, state):
    self.close()
    self._producer.views.clear()
    self._producer.order.set_state(state)
    self._state, self._first, self._ended = copy.deepcopy(state), None, False


class DeviceReader(object):
  """Iterator over the raw batches of the module's docstring: HostReader's batches through the reader's own JpegDecoder."""

  def __init__(self, host, files, is_training, canvas, depth, threads, fallback, fake, jpeg_entropy='host'):
    self._host, self._files, self._is_training, self._canvas = host, files, is_training, (int(canvas[0]), int(canvas[1]))
    self._depth, self._threads, self._fallback, self._fake = depth, threads, fallback, fake
    self._entropy = jpeg_entropy
    self._decoders = {}
    self._issued = {}      # device entropy: per decoder and set of arenas, (batch number, HostBatch.index) of its last batch
    self._count = 0
    self._first = None

  def _decoder(self, batch):
    from automl_amd import jpeg
    if batch not in self._decoders:      # the reader's batch, and the short last one where it is kept
      mode = {} if self._entropy == 'host' else {'entropy': self._entropy}
      self._decoders[batch] = jpeg.JpegDecoder(batch, self._canvas[0], self._canvas[1], depth=self._depth,
                                               threads=None if self._threads is None else min(int(self._threads), batch), **mode)
      self._issued[batch] = [None] * self._decoders[batch].depth
    return self._decoders[batch]

  def _check_scans(self, batch, ahead=0):
    """Device entropy: a stream damaged inside its scan is found on the device, behind decode()'s back.  Asked here, for the
    batch that last used the set of arenas the next decode() takes, where decode() waits for that set anyway."""
    dec = self._decoders[batch]
    at = (dec._next + ahead) % dec.depth
    failed = dec.scan_failures(ahead)
    if failed and self._issued[batch][at] is not None:
      number, index = self._issued[batch][at]
      self._issued[batch][at] = None
      raise ValueError('batch %d: the scan of image %s is malformed or truncated (found on the device, behind decode): %s'
                       % (number, failed, ['%s record %d' % (self._files[index[i][0]], index[i][1]) for i in failed]))

  def __iter__(self):
    return self

  def __next__(self):
    if self._first is not None:
      return self._first
    try:
      hb = next(self._host)
    except StopIteration:
      for batch in self._decoders if self._entropy == 'device' else ():      # the batches still in flight
        for ahead in range(self._decoders[batch].depth):
          self._check_scans(batch, ahead)
      raise
    dec = self._decoder(len(hb.images))
    if self._entropy == 'device':
      self._check_scans(len(hb.images))
      self._issued[len(hb.images)][dec._next] = (self._count, hb.index)
    self._count += 1
    try:
      raw, sizes = dec.decode(hb.images, fallback=self._fallback)
    except ValueError as e:
      raise ValueError('%s; the batch holds %s' % (e, ['%s record %d' % (self._files[f], r) for f, r in hb.index]))
    if self._is_training:
      batch = ((raw, sizes), hb.boxes, hb.classes, hb.counts)
    else:
      batch = ((raw, sizes), hb.boxes, hb.classes, hb.counts, hb.is_crowds, hb.areas, hb.source_ids)
    if self._fake:
      self._first = batch
    return batch

  def get_state(self):
    return self._host.get_state()

  def set_state(self, state):
    self._host.set_state(state)
    self._first = None

  def close(self):
    self._host.close()


class InputReader(object):
  """dataloader.py:236-460.  reader(params, ...) -- also reader_obj(params, ...), as the reference calls it -- returns the
  iterator of raw batches; host_reader(params, ...) the host half alone (HostBatch, no device)."""

  def __init__(self, file_pattern, is_training, use_fake_data=False, max_instances_per_image=None, debug=False,
               jpeg_entropy='host'):
    if jpeg_entropy not in ('host', 'device'):
      raise ValueError("jpeg_entropy=%r: 'host' or 'device' (jpeg.JpegDecoder's entropy=)" % (jpeg_entropy,))
    self._jpeg_entropy = jpeg_entropy
    self._file_pattern = file_pattern
    self._is_training = bool(is_training)
    self._use_fake_data = bool(use_fake_data)
    self._max_instances_per_image = max_instances_per_image or 100
    self._debug = bool(debug)

  def files(self, shard=None):
    """The sorted files of the pattern, files[i::n] of them for shard=(n, i)."""
    files = sorted(glob.glob(self._file_pattern))
    if not files:
      raise ValueError('file_pattern %r matches no file' % (self._file_pattern,))
    if shard is not None:
      n, i = int(shard[0]), int(shard[1])
      if n < 1 or not 0 <= i < n:
        raise ValueError('shard=(%d, %d): (number of shards, index below it)' % (n, i))
      if i >= len(files):
        raise ValueError('shard %d of %d gets none of the %d files of %r' % (i, n, len(files), self._file_pattern))
      files = files[i::n]
    return files

  def host_reader(self, params, batch_size=None, shard=None, depth=2, threads=None, verify=True):
    params = params.as_dict() if hasattr(params, 'as_dict') else params
    if params.get('dataset_type', None) == 'sstable':
      raise ValueError("dataset_type='sstable' is not built: SSTable is not a public format (dataloader.py:429-431)")
    if 'segmentation' in (params.get('heads', None) or ()):
      raise ValueError("heads contains 'segmentation': instance masks (PNG, include_mask) are not built "
                       '(dataloader.py:410-411, object_detection/tf_example_decoder.py:49-53)')
    if params.get('regenerate_source_id', False):
      tf_example_decoder.TfExampleDecoder(regenerate_source_id=True)      # raises, with the reason
    batch = int(batch_size or params['batch_size'])
    if batch < 1:
      raise ValueError('batch_size %d < 1' % batch)
    files = self.files(shard)
    producer = _Producer(files, batch, self._is_training, self._is_training and not self._debug, params.get('tf_random_seed', None),
                         self._is_training and params.get('skip_crowd_during_training', False),
                         params.get('drop_remainder', True), self._max_instances_per_image, threads, verify)
    producer.open_first()
    return HostReader(producer, depth, self._use_fake_data)

  def reader(self, params, batch_size=None, canvas=None, shard=None, depth=2, threads=None, fallback=None, verify=True):
    if canvas is None or len(canvas) != 2:
      raise ValueError('canvas=(Hc, Wc) is needed: the slot every decoded image is written into (jpeg.JpegDecoder)')
    host = self.host_reader(params, batch_size, shard, depth, threads, verify)
    return DeviceReader(host, host.files, self._is_training, canvas, depth, threads, fallback, self._use_fake_data,
                        self._jpeg_entropy)

  __call__ = reader
