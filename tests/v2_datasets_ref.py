"""Pure-Python restatement of automl_amd/effnetv2_datasets.py for the tests (in the manner of tests/tfrecord_ref.py): the file
list of a split, the class id of a record, and the (file, record) batches of the reader's order -- plus the helper that writes
the small ImageNet-style shards the host and the device tests read.  Nothing here imports the module under test."""
import os

import numpy as np

from tests import tfrecord_ref

SPLITS = {'train': ('train*', 20, None), 'minival': ('train*', 0, 20), 'eval': ('val*', 0, None), 'trainval': ('train*', 0, None)}
IMAGES = ('s1x1_444_q75', 's8x9_420_q75', 's16x16_444_q75', 's17x33_422_q75', 's31x22_420_q75', 's37x53_444_q75',
          'grey_16x16_q75', 'grey_19x13_q90', 's37x53_420_q30')      # 4:4:4, 4:2:2, 4:2:0 and greyscale, odd sizes, 1 x 1
OVERSIZE = ('s24x280_420_q75', 'big_480x640_420')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_cases.npz')


def load_jpegs(names=IMAGES):
  g = np.load(GOLDEN)
  return [g[n + '/bytes'].tobytes() for n in names]


def split_files(names, split, shard=None):
  """names: the file names of data_dir -> those of the split, in order (datasets.py:342-344, :352)."""
  prefix, start, stop = SPLITS[split]
  files = sorted(n for n in names if n.startswith(prefix[:-1]))[start:stop]
  return files if shard is None else files[shard[1]::shard[0]]


def class_id(record, num_classes):
  """datasets.py:309-320 with this project's refusal: label - 1, ValueError for a missing label or one outside 1 .. C."""
  p = tfrecord_ref.parse_example(record, [('image/encoded', 'bytes', 1), ('image/class/label', 'int64', 1)])
  label = p['image/class/label'][0] if p['image/class/label'] else -1
  if not 1 <= label <= num_classes:
    raise ValueError('label %d' % label)
  return label - 1


def image_of(record):
  p = tfrecord_ref.parse_example(record, [('image/encoded', 'bytes', 1)])
  o, n = p['image/encoded'][0]
  return bytes(record)[o:o + n]


def _round_robin(files, sizes, cycle):
  """One epoch's interleave: `cycle` files open, one record each in turn; an ended file's slot and turn go to the next file."""
  open_, waiting, out, turn = [[f, 0] for f in files[:cycle]], list(files[cycle:]), [], 0
  while any(s is not None for s in open_):
    s = open_[turn]
    while s is not None and s[1] >= sizes[s[0]]:
      s = open_[turn] = [waiting.pop(0), 0] if waiting else None
    if s is not None:
      out.append((s[0], s[1]))
      s[1] += 1
    turn = (turn + 1) % len(open_)
  return out


def batches(sizes, batch, training, seed, epochs, cycle=16, buffer=64):
  """The [(file, record)] batches of `epochs` epochs, the remainder of each epoch dropped.  training=False (evaluation, and
  debug): one pass, no permutation, no shuffle buffer."""
  shuffle = training
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(epochs if training else 1):
    files = [int(v) for v in rng.permutation(len(sizes))] if shuffle else list(range(len(sizes)))
    seq = _round_robin(files, sizes, min(cycle, len(files)))
    if shuffle:
      held, at, emitted = seq[:buffer], buffer, []
      while held:
        j = int(rng.integers(len(held)))
        emitted.append(held[j])
        if at < len(seq):
          held[j] = seq[at]
          at += 1
        else:
          held[j] = held[-1]
          del held[-1]
      seq = emitted
    out += [seq[k:k + batch] for k in range(0, len(seq) - batch + 1, batch)]
  return out


def write_shards(folder, jpegs, train_sizes, val_sizes, num_classes, writer, encode):
  """train-00000 .. and val-00000 .. in `folder`, file f holding sizes[f] records; record r of file f carries image
  jpegs[(3 f + r) % len] and label 1 + (5 f + 7 r) % num_classes.  writer / encode: tfrecord.TFRecordWriter / encode_example.
  -> {file name: [(image bytes, class id)]}."""
  content = {}
  for prefix, sizes in (('train', train_sizes), ('val', val_sizes)):
    for f, n in enumerate(sizes):
      name = '%s-%05d-of-%05d' % (prefix, f, len(sizes))
      rows = [(jpegs[(3 * f + r) % len(jpegs)], (5 * f + 7 * r) % num_classes) for r in range(n)]
      with writer(os.path.join(str(folder), name)) as w:
        for image, cls in rows:
          w.write(encode({'image/encoded': image, 'image/class/label': [cls + 1]}))
      content[name] = rows
  return content
