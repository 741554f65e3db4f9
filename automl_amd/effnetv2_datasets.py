"""efficientnetv2/datasets.py on MI355X, as far as it can exist here: the ImageNet TFRecord reader (:72-448), the dataset
training configurations (:646-729) and ``build_dataset_input`` -> the batches TrainableModel.train_step / test_step take.

  reader = ImageNetInput(True, '/data/imagenet', seed=1)(256, canvas=(512, 512))
  for batch in reader:            # ((raw uint8 [B, Hc, Wc, 3] on the device, sizes int32 [B, 2]), labels int32 [B])
    model.train_step(batch)       # TrainableModel(image_size=...): crop, resize, flip, RandAugment, mixing on the device

Pinned to the reference: the split table (``ImageNetInput.cfg``, :78-91), split = 'train' / 'eval' by is_training (:140), the
files sorted(glob(data_dir / files))[slice] with Python's own slicing (:342-344: 'train' of fewer than 21 files is empty, and an
empty list raises), the two keys of a record -- 'image/encoded' (bytes) and 'image/class/label' (int64), class id = label - 1
(:309-320) -- and drop_remainder=True in both modes (:406-407).

This project's definition (tf.data's 128 K-element shuffle and non-deterministic interleave are pinned nowhere): the order is
dataloader.RecordOrder's -- training: the file list permuted per epoch by a generator seeded by `seed`, round-robin over at
most 16 open files, a 64-record shuffle buffer, repeating; evaluation, and debug=True: file order, one pass (no permutation, no
shuffle, no repeat).  shard=(n, i) keeps files[i::n] of the sliced list (:352).
get_state() / set_state() of a reader resume the same stream.

The structure is dataloader.InputReader's: ONE background thread reads, verifies and parses up to `depth` batches ahead
(tfrecord.parse_examples with a two-entry spec); the reader's jpeg.JpegDecoder and every HIP call stay on the consumer's thread,
and the image bytes go to the Huffman workers as memoryviews into the mapped files.  Worker threads are 1 .. 16, never the
machine's core count.  The labels stay on the host: train_step range-checks host labels before any launch.

Deliberate differences.  (1) A missing label (the reference's default -1), label 0 or a label above num_classes becomes an
all-zero one-hot row in the reference, which then trains on it; here such a record raises tfrecord.TFRecordError naming the
file, the record number and its byte offset, as the detector's reader does for a malformed record.  (2) The reference
decodes, crops and augments inside its input pipeline at the stage's image size; here the reader delivers decoded canvases
and TrainableModel does the rest on the device, so ONE reader serves every progressive stage (image_size / image_dtype of
build_dataset_input are accepted and unused).  (3) ImagenetFt names the tfds data set 'imagenettfds' in the reference; here
the fine-tuning recipe reads the ImageNet TFRecords, the only reader that is built.

What the decoder refuses passes through unchanged: ImageNet holds a few CMYK JPEGs and a PNG, and jpeg.JpegDecoder's statuses
and ``fallback=`` (a callable from the bytes to uint8 [h, w, 3]) apply as they are; without a fallback the error names the
file and the record.  An image larger than the canvas is the decoder's TOO_LARGE and goes the same way with max_ratio=1, the
default.  Full-size ImageNet has images of several thousand pixels a side: reader(..., max_ratio=8) decodes such an image at
the smallest tf.io.decode_jpeg ratio (2, 4 or 8: libjpeg's reduced-size decode, jpeg.choose_ratio) whose output fits the
canvas, and `sizes` are then the output sizes, so nothing behind the decoder changes.  The ratio is a function of the file's
header and the canvas alone: the order of the records and get_state() / set_state() are what they are without it.
Deliberate difference (4): the reference decodes every image at full size and crops and resizes from that; with a ratio, the
crop and the bicubic / bilinear resize start from libjpeg's reduced image, for the images larger than the canvas only.  An
image that is still too large at max_ratio, or a batch whose files have more 8x8 blocks than the decoder's coefficient arena
(jpeg.JpegDecoder's coef_blocks), is TOO_LARGE as before.

Window decode (tf.image.decode_and_crop_jpeg, preprocess_legacy.py:53-68): reader(..., decode_crop=True), training only.  The
background thread reads each image's size from its header and draws ONE crop window per image with
v2_preprocessing.sample_distorted_bounding_box at train_rows' defaults; the decoder stores, copies and transforms only the
blocks that window needs (jpeg.JpegDecoder(windowed=True)), and the batches are ((raw, sizes), labels) as before with each
window at the top-left of its slot and `sizes` the window sizes.  The model is then built with transformations='flip': its
step takes the whole "image" and only draws the flip.  The windows come from a generator of their own, a PCG64 stream derived
from the reader's seed, whose state travels with get_state() / set_state() under the key 'window_rng' -- present only with
decode_crop, and a state with or without it given to a reader that is the other way round raises.  An image whose header
cannot be read gets no draw and is left to the decoder's status and `fallback`; a stream that goes to `fallback` comes back
whole.  With max_ratio > 1 each image is decoded at the smallest ratio at which the window's covering output window fits the
canvas (jpeg.choose_window_ratio); one that fits at no ratio is the decoder's TOO_LARGE.  Deliberate difference (5): the
reference decodes the window at full size whatever its size; and the order of the draws is this project's, as for the crop in
the step.  Without decode_crop nothing changes, the reader's state and the order of its records included.
reader(..., decode_crop='legacy', crop_image_size=N): the same, with the LEGACY pipeline's window in place of the V2 sampler's
-- preprocess_legacy.train_crop_window, the one function behind preprocess_legacy.legacy_train_rows: the box of area
[0.08, 1], aspect ratio [3/4, 4/3], 10 attempts and min_object_covered 0.1, or the padded centre crop for training size N
where the sampler hands back the whole image (preprocess_legacy.py:88-127) -- drawn from the header size on the same
'window_rng' stream; the model is then TrainableModel(preprocessing='legacy', transformations='flip').  decode_crop=True
keeps its sampler, stream and state.  A legacy reader's state carries 'window_sampler': 'legacy' beside the stream, and a
state given to a reader with the other sampler raises: the stream never goes on silently under another sampler.

Not built, raising ValueError('... is not built: ...'): every tfds-backed configuration (cifar10, cifar100, flowers,
tfflowers, cars, imagenettfds: tensorflow_datasets is not available and its on-disk format is not read), imagenet21k (its
multiclass labels need the sigmoid loss, which train_step does not have), and the null input of data_dir None / '' / 'null'
(black images with all-zero label rows, :305-307: train_step's labels are class ids or one-hot rows, an all-zero row is
neither).  cache, transpose_image and file_buffer_size_m have no counterpart."""
import collections
import copy
import glob
import os
import re

import numpy as np

from automl_amd import dataloader
from automl_amd import hparams_config
from automl_amd import tfrecord

Config = hparams_config.Config

SPEC = (('image/encoded', 'bytes', 1), ('image/class/label', 'int64', 1))

# windows / image_sizes (decode_crop only): int32 [B, 4] = (y, x, h, w) in full-size pixels and int32 [B, 2] from the headers;
# an image whose header cannot be read has zeros in both
HostBatch = collections.namedtuple('HostBatch', 'index images labels state windows image_sizes', defaults=(None, None))
WINDOW_KEY = 'window_rng'
SAMPLER_KEY = 'window_sampler'      # only in the state of a decode_crop='legacy' reader: which function draws from that stream

# datasets.py:78-91; a slice is [start, stop] so that the table stays plain data (config.yaml)
IMAGENET_CFG = dict(
    data_dir=None, num_classes=1000, multiclass=False, tfds_split=None,
    splits=dict(train=dict(num_images=1256144, files='train*', slice=[20, None]),
                minival=dict(num_images=25021, files='train*', slice=[0, 20]),
                eval=dict(num_images=50000, files='val*', slice=[0, None]),
                trainval=dict(num_images=1281167, files='train*', slice=[0, None])))

_TFDS = 'it is read through tensorflow_datasets, which is not available, and its on-disk format is not read'
UNBUILT_DATASETS = {
    'imagenet21k': 'its labels are multiclass (several classes per image) and need the sigmoid loss, which train_step does '
                   'not have (datasets.py:451-503)',
    'imagenettfds': _TFDS, 'cifar10': _TFDS, 'cifar100': _TFDS, 'flowers': _TFDS, 'tfflowers': _TFDS, 'cars': _TFDS,
}
# the dataset training configurations (datasets.py:646-760) -> the data set each of them names
_UNBUILT_CONFIGS = {'imagenet21k': 'imagenet21k', 'cifar10ft': 'cifar10', 'cifar100ft': 'cifar100', 'flowersft': 'flowers',
                    'tfflowersft': 'tfflowers', 'carsft': 'cars'}

# datasets.py:646-663
IMAGENET_TRAIN_CFG = dict(
    data=dict(ds_name='imagenet', multiclass=False),
    train=dict(epochs=350, lr_base=0.016, lr_warmup_epoch=5, lr_sched='exponential', label_smoothing=0.1),
    eval=dict(batch_size=8))
# datasets.py:699-727 (fine-tuning: less regularisation); ds_name: the module's docstring, difference (3)
IMAGENETFT_TRAIN_CFG = dict(
    model=dict(dropout_rate=0.000001, survival_prob=0.8),
    train=dict(batch_size=512, stages=0, epochs=15, optimizer='rmsprop', lr_sched='constant', lr_base=0.0005,
               lr_warmup_epoch=1, ema_decay=0.9996, weight_decay=1e-5, label_smoothing=0.1, min_steps=10000, isize=1.0),
    data=dict(ds_name='imagenet', augname='ft', mixup_alpha=0, cutmix_alpha=0))


def _not_built(name, reason):
  return ValueError('dataset %r is not built: %s' % (name, reason))


def get_dataset_class(ds_name):
  """datasets.py:631-641; 'imagenet' (and the fine-tuning configuration's name 'imagenetft') -> ImageNetInput."""
  name = str(ds_name).lower()
  if name in ('imagenet', 'imagenetft'):
    return ImageNetInput
  if name in UNBUILT_DATASETS:
    raise _not_built(ds_name, UNBUILT_DATASETS[name])
  raise ValueError('unknown dataset %r (datasets.py:631-641 has imagenet, imagenet21k, imagenettfds, cifar10, cifar100, '
                   'flowers, tfflowers, cars)' % (ds_name,))


def get_dataset_config(name):
  """datasets.py:764-768: the training configuration 'imagenet' or 'imagenetft' with the data set's own table merged into
  its data section -> a Config with data / train / eval ('imagenet') or model / train / data ('imagenetft')."""
  key = str(name).lower()
  if key in _UNBUILT_CONFIGS:
    raise _not_built(name, UNBUILT_DATASETS[_UNBUILT_CONFIGS[key]])
  if key == 'imagenet':
    cfg = Config(copy.deepcopy(IMAGENET_TRAIN_CFG))
  elif key == 'imagenetft':
    cfg = Config(copy.deepcopy(IMAGENETFT_TRAIN_CFG))      # (the class's own table: nothing of ImageNet's is inherited)
  else:
    raise ValueError('ds:%s not registered: imagenet, imagenetft (built); %s (not built)' % (key, ', '.join(_UNBUILT_CONFIGS)))
  cfg.data.update(get_dataset_class(cfg.data.ds_name).cfg)
  return cfg


def build_dataset_input(is_training, image_size, image_dtype, data_dir, split, ds_cfg, seed=None, debug=False):
  """datasets.py:23-45 -> an ImageNetInput on ds_cfg (the data section of a configuration: ds_name, num_classes, splits).
  image_size and image_dtype are accepted and unused: crop, resize, augmentation and the cast are TrainableModel's."""
  del image_size, image_dtype
  ds_cfg = ds_cfg.as_dict() if hasattr(ds_cfg, 'as_dict') else dict(ds_cfg)
  return get_dataset_class(ds_cfg.get('ds_name', 'imagenet'))(is_training, data_dir, split, debug=debug, seed=seed, cfg=ds_cfg)


def window_rng(seed):
  """The generator behind the crop windows of reader(decode_crop=True): a PCG64 stream of its own, derived from the reader's
  seed (None: numpy's entropy)."""
  return np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(0x77696E646F77,))))


class _Order(object):
  """dataloader.RecordOrder with the window generator's state next to its own: what the producer and HostReader know as the
  order.  rng None (no decode_crop): RecordOrder's state as it is."""

  def __init__(self, order, rng, sampler=None):
    self.order, self.rng, self.sampler = order, rng, sampler      # sampler: None (the V2 box) or 'legacy'

  def next(self):
    return self.order.next()

  @property
  def finished(self):
    return self.order.finished

  def get_state(self):
    state = self.order.get_state()
    if self.rng is not None:
      state[WINDOW_KEY] = copy.deepcopy(self.rng.bit_generator.state)
      if self.sampler is not None:
        state[SAMPLER_KEY] = self.sampler
    return state

  def set_state(self, state):
    if (WINDOW_KEY in state) != (self.rng is not None):
      raise ValueError('this state has %s key %r and the reader was made with%s decode_crop: a state resumes a reader made the '
                       'same way' % (('the', WINDOW_KEY, 'out') if WINDOW_KEY in state else ('no', WINDOW_KEY, '')))
    state = dict(state)
    sampler = state.pop(SAMPLER_KEY, None)
    if sampler != self.sampler:
      kind = lambda s: "decode_crop='legacy'" if s == 'legacy' else 'decode_crop=True'
      raise ValueError('this state was saved by a reader made with %s and the reader was made with %s: the %r stream would go on '
                       'under another sampler; a state resumes a reader made the same way' % (kind(sampler), kind(self.sampler),
                                                                                                WINDOW_KEY))
    if self.rng is not None:
      self.rng.bit_generator.state = copy.deepcopy(state.pop(WINDOW_KEY))
    self.order.set_state(state)


class _Producer(dataloader._Producer):
  """The host half for classification records: dataloader._Producer's order, open files and thread body with the two-key
  parse in place of the detection decoder."""

  def __init__(self, files, batch, shuffle, seed, num_classes, threads, verify, decode_crop=False, crop_image_size=None):      # pylint: disable=super-init-not-called
    self.files, self.batch = files, int(batch)
    self.drop_remainder, self.num_classes = True, int(num_classes)
    self.threads, self.verify = threads, verify
    self.open = collections.OrderedDict()
    self.views = {}
    self.order = _Order(dataloader.RecordOrder(len(files), self._has, shuffle, seed, repeat=shuffle),
                        window_rng(seed) if decode_crop else None, 'legacy' if decode_crop == 'legacy' else None)
    self.legacy_size = int(crop_image_size) if decode_crop == 'legacy' else None

  def _error(self, pair, what, status=None):
    f, r = pair
    return tfrecord.TFRecordError('%s: %s' % (self._where(f, r), what), self.files[f], r, self._file(f).offset(r), status)

  def _assemble(self, index):
    views = [self._view(f, r) for f, r in index]
    parsed = tfrecord.parse_examples(views, SPEC, self.threads)
    images, labels = [], np.zeros(len(index), np.int32)
    for i, pair in enumerate(index):
      status = int(parsed.status[i])
      if status != tfrecord.E_OK:
        raise self._error(pair, 'not a tf.train.Example that can be read: %s (status %d)' % (tfrecord.PARSING[status], status), status)
      if parsed.counts['image/encoded'][i] < 1:
        raise self._error(pair, "no 'image/encoded' feature")
      if parsed.counts['image/class/label'][i] < 1:
        raise self._error(pair, "no 'image/class/label' feature (the reference's default -1 would train on an all-zero label row)")
      label = int(parsed.values['image/class/label'][i, 0])
      if not 1 <= label <= self.num_classes:
        raise self._error(pair, "'image/class/label' %d outside 1 .. %d (0 is the background; the reference would train on an "
                          'all-zero label row)' % (label, self.num_classes))
      labels[i] = label - 1      # datasets.py:317-320
      offset, length = (int(v) for v in parsed.values['image/encoded'][i, 0])
      images.append(views[i][offset:offset + length])
    if self.order.rng is None:
      return HostBatch(index, images, labels, self.order.get_state())
    from automl_amd import jpeg, preprocess_legacy, v2_preprocessing
    sizes = jpeg.jpeg_sizes(images)
    windows = np.zeros((len(index), 4), np.int32)
    for i, (h, w) in enumerate(sizes):
      if h >= 1 and w >= 1 and self.legacy_size is not None:
        windows[i] = preprocess_legacy.train_crop_window(self.order.rng, int(h), int(w), self.legacy_size)
      elif h >= 1 and w >= 1:      # (else: no draw; the decoder says what is wrong with the stream)
        windows[i] = v2_preprocessing.sample_distorted_bounding_box(self.order.rng, int(h), int(w))
      else:
        sizes[i] = 0
    return HostBatch(index, images, labels, self.order.get_state(), windows, sizes)


class DeviceReader(object):
  """Iterator over ((raw, sizes), labels): dataloader.HostReader's batches through the reader's own jpeg.JpegDecoder."""

  def __init__(self, host, canvas, depth, threads, fallback, max_ratio=1, decode_crop=False):
    self._host, self._canvas, self._decode_crop = host, (int(canvas[0]), int(canvas[1])), bool(decode_crop)
    self._depth, self._threads, self._fallback, self._max_ratio = depth, threads, fallback, max_ratio
    self._decoder = None
    self.files = host.files

  def __iter__(self):
    return self

  def __next__(self):
    hb = next(self._host)
    if self._decoder is None:
      from automl_amd import jpeg
      threads = None if self._threads is None else min(int(self._threads), len(hb.images))
      ratio = {} if self._max_ratio == 1 else {'max_ratio': self._max_ratio}      # (1: the decoder as it is built without it)
      if self._decode_crop:
        ratio['windowed'] = True
      self._decoder = jpeg.JpegDecoder(len(hb.images), self._canvas[0], self._canvas[1], depth=self._depth, threads=threads,
                                       **ratio)
    try:
      if self._decode_crop:
        ratios, windows = self._output_windows(hb)
        raw, sizes = self._decoder.decode(hb.images, fallback=self._fallback, windows=windows,
                                          ratios=None if self._max_ratio == 1 else ratios)
      else:
        raw, sizes = self._decoder.decode(hb.images, fallback=self._fallback)
    except ValueError as e:
      raise ValueError(name_refused(str(e), hb.index, self.files))
    return (raw, sizes), hb.labels

  def _output_windows(self, hb):
    """The ratio of every image and its window in the output at that ratio (jpeg.choose_window_ratio).  A window that fits
    the canvas at no ratio goes to the decoder at max_ratio, which calls it TOO_LARGE; an image without a readable header goes
    with a one-pixel window, and the decoder gives the stream's own status."""
    from automl_amd import jpeg
    ratios, windows = [], np.zeros((len(hb.images), 4), np.int32)
    for i, (window, (h, w)) in enumerate(zip(hb.windows, hb.image_sizes)):
      if h < 1:
        ratios.append(1)
        windows[i] = (0, 0, 1, 1)
        continue
      got = jpeg.choose_window_ratio(window, int(h), int(w), self._canvas[0], self._canvas[1], self._max_ratio)
      if got is None:
        got = self._max_ratio, jpeg.covering_window(window, self._max_ratio)
      ratios.append(got[0])
      windows[i] = got[1]
    return ratios, windows

  def get_state(self):
    return self._host.get_state()

  def set_state(self, state):
    self._host.set_state(state)

  def close(self):
    self._host.close()


def name_refused(message, index, files):
  """The decoder's message about contents[i] of a batch with that record named: '<file> record <r>: <message>'."""
  m = re.search(r'contents\[(\d+)\]', message)
  if m is None or int(m.group(1)) >= len(index):
    return '%s; the batch holds %s' % (message, ['%s record %d' % (files[f], r) for f, r in index])
  f, r = index[int(m.group(1))]
  return '%s record %d: %s' % (files[f], r, message)


class ImageNetInput(object):
  """datasets.py:72-448.  reader(batch_size, canvas=(Hc, Wc), ...) -- also input_obj(batch_size, ...) -- returns the iterator
  of ((raw, sizes), labels); host_reader(batch_size, ...) the host half alone (HostBatch: index, images, labels; no device).
  seed: the generator behind the training order (None: numpy's entropy).  cfg: the data section to use instead of the class
  table (num_classes, splits.<split>.num_images / files / slice), as build_dataset_input passes it."""
  cfg = Config(copy.deepcopy(IMAGENET_CFG))

  def __init__(self, is_training, data_dir, split=None, debug=False, seed=None, cfg=None):
    if data_dir is None or data_dir in ('', 'null'):
      raise ValueError("data_dir=%r: the null input is not built: the reference then feeds black images with all-zero label "
                       "rows (datasets.py:305-307, :338-340), and train_step's labels are class ids or one-hot rows -- an "
                       'all-zero row is neither' % (data_dir,))
    self.is_training, self.data_dir, self.debug, self.seed = bool(is_training), str(data_dir), bool(debug), seed
    self.split = split or ('train' if is_training else 'eval')      # datasets.py:140
    table = self.cfg.as_dict()
    if cfg is not None:
      given = cfg.as_dict() if hasattr(cfg, 'as_dict') else cfg
      table = Config(table)
      table.update({k: v for k, v in given.items() if k in ('num_classes', 'splits')})
      table = table.as_dict()
    if self.split not in table['splits']:
      raise ValueError('split %r: one of %s' % (self.split, ', '.join(table['splits'])))
    self.num_classes = int(table['num_classes'])
    self.split_info = table['splits'][self.split]
    if not self.split_info.get('files'):
      raise ValueError('split %r of this data configuration names no files' % (self.split,))

  @property
  def num_images(self):
    return self.split_info['num_images']

  def files(self, shard=None):
    """sorted(glob(data_dir / files))[slice] (datasets.py:342-344), files[i::n] of them for shard=(n, i) (:352)."""
    pattern = os.path.join(self.data_dir, self.split_info['files'])
    found = sorted(glob.glob(pattern))
    if not found:
      raise ValueError('%r matches no file (split %r)' % (pattern, self.split))
    start, stop = self.split_info.get('slice') or (None, None)
    files = found[slice(start, stop)]
    if not files:
      raise ValueError('split %r keeps files[%s:%s] of %r, and only %d match: none is left' % (
          self.split, '' if start is None else start, '' if stop is None else stop, pattern, len(found)))
    if shard is not None:
      n, i = int(shard[0]), int(shard[1])
      if n < 1 or not 0 <= i < n:
        raise ValueError('shard=(%d, %d): (number of shards, index below it)' % (n, i))
      if i >= len(files):
        raise ValueError('shard %d of %d gets none of the %d files of split %r' % (i, n, len(files), self.split))
      files = files[i::n]
    return files

  @staticmethod
  def _check_decode_crop(decode_crop, crop_image_size):
    """decode_crop: False / True / 'legacy'; 'legacy' needs crop_image_size (the training size its centre-crop fallback is
    made for), and nothing else takes one."""
    if decode_crop not in (False, True, None, 'legacy'):
      raise ValueError("decode_crop=%r: False, True or 'legacy'" % (decode_crop,))
    if decode_crop == 'legacy':
      if crop_image_size is None or int(crop_image_size) != crop_image_size or int(crop_image_size) < 1:
        raise ValueError("decode_crop='legacy' needs crop_image_size, the training size (a positive integer): the centre-crop "
                         'fallback of preprocess_legacy.py:110-127 depends on it; got %r' % (crop_image_size,))
    elif crop_image_size is not None:
      raise ValueError("crop_image_size belongs to decode_crop='legacy'")

  def host_reader(self, batch_size, shard=None, depth=2, threads=None, verify=True, decode_crop=False, crop_image_size=None):
    batch = int(batch_size)
    if batch < 1:
      raise ValueError('batch_size %d < 1' % batch)
    if threads is not None and not 1 <= int(threads) <= tfrecord.MAX_THREADS:
      raise ValueError('threads %d outside 1 .. %d' % (threads, tfrecord.MAX_THREADS))
    self._check_decode_crop(decode_crop, crop_image_size)
    if decode_crop and not self.is_training:
      raise ValueError('decode_crop is for training: evaluation takes the whole image or its centre crop (eval_rows)')
    producer = _Producer(self.files(shard), batch, self.is_training and not self.debug, self.seed, self.num_classes, threads,
                         verify, 'legacy' if decode_crop == 'legacy' else bool(decode_crop), crop_image_size)
    producer.open_first()
    return dataloader.HostReader(producer, depth, False)

  def reader(self, batch_size, canvas=None, shard=None, depth=2, threads=None, fallback=None, verify=True, max_ratio=1,
             decode_crop=False, crop_image_size=None):
    if canvas is None or len(canvas) != 2:
      raise ValueError('canvas=(Hc, Wc) is needed: the slot every decoded image is written into (jpeg.JpegDecoder)')
    if max_ratio not in (1, 2, 4, 8):
      raise ValueError('max_ratio=%r: 1, 2, 4 or 8 (jpeg.JpegDecoder)' % (max_ratio,))
    return DeviceReader(self.host_reader(batch_size, shard, depth, threads, verify, decode_crop, crop_image_size), canvas, depth,
                        threads, fallback, max_ratio, decode_crop)

  __call__ = reader
