#!/usr/bin/env python3
"""TrainableModel.fit over effnetv2_datasets.ImageNetInput on one MI355X, for LABNOTES.md "Classifier training driver" (NOT the
bench.py line, and nothing here is read by bench.py).  The workload: EfficientNetV2-S, bf16, training size `--image_size`,
batch `--batch`, a `--canvas` x `--canvas` canvas, the step replayed from its hipGraph with crop, resize and flip on the
device.  The script writes its own shards into a temporary folder: `--images` records in `--shards` files, every image the
640 x 480 file of tests/golden/jpeg_cases.npz cut to the canvas and encoded again with Pillow (quality 90, 4:2:0); where Pillow
is not importable the file goes in whole and the canvas is widened to hold it, which the JSON line says.

  --mode fit    fit over the reader.  After a warm-up fit of three steps (eager, capture, replay) one fit runs `--rounds` + 1
                epochs of `--steps` steps; an epoch is timed from on_epoch_begin to on_epoch_end (fit reads its accumulator in
                between, which waits for the device); the first epoch is not kept.  Also the reader alone: records/s of the
                host half (CRC, parse) and images/s of reader + decoder, so that a gap can be placed.
  --mode hand   the hand loop train_step(batch, sync_loss=False) fed from memory with the same canvases (two batches decoded
                once, alternating), `--rounds` + 1 rounds of `--steps` steps ending in one synchronisation.  `--root DIR` takes
                the package from DIR: a checkout of the parent commit, whose train_step is the same code and which has
                neither fit nor the reader.

  --mode hand_reader   the same hand loop fed by the reader (this tree): what the decode costs the step without fit.

`--decode_crop` (modes fit and hand_reader): the reader draws the crop and decodes only that window of each file
(reader(decode_crop=True)), and the model is built with transformations='flip', as effnetv2_main --decode_crop does.

Prints one JSON line: images/s as the median of the rounds with the spread (max - min) beside it.  The comparison -- three
processes of each mode, alternating -- is the caller's; no ratio is asserted here."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLASSES = 1000


def stats(rates):
  return {'median': round(float(np.median(rates)), 1), 'spread': round(float(max(rates) - min(rates)), 1), 'rounds': len(rates)}


def make_jpeg(canvas):
  """-> (bytes, canvas side that holds it, what it is)."""
  g = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz'))
  whole = g['big_480x640_420/bytes'].tobytes()
  try:
    from PIL import Image
  except ImportError:
    return whole, max(canvas, 640), 'fixture big_480x640_420 whole (no Pillow to cut it)'
  image = Image.open(io.BytesIO(whole)).convert('RGB').crop((0, 0, min(640, canvas), min(480, canvas)))
  buf = io.BytesIO()
  image.save(buf, 'JPEG', quality=90, subsampling=2)
  return buf.getvalue(), canvas, 'fixture big_480x640_420 cut to %d x %d, Pillow quality 90' % image.size[::-1]


class EpochTimer(object):
  def __init__(self):
    self.seconds = []

  def on_epoch_begin(self, epoch, logs=None):
    self._t0 = time.perf_counter()

  def on_epoch_end(self, epoch, logs=None):
    self.seconds.append(time.perf_counter() - self._t0)


def main(args):
  sys.path.insert(0, os.path.abspath(args.root))
  import torch
  from automl_amd import effnetv2_train, jpeg
  if not torch.cuda.is_available():
    sys.exit('bench_v2_fit.py needs an MI355X')
  data, canvas, source = make_jpeg(args.canvas)
  n, b = args.images, args.batch
  out = {'mode': args.mode, 'model': args.model, 'images': n, 'shards': args.shards, 'batch': b, 'canvas': canvas, 'jpeg': source,
         'jpeg_bytes': len(data), 'image_size': args.image_size, 'dtype': 'bf16', 'rounds': args.rounds, 'steps_per_round': args.steps,
         'root': os.path.relpath(os.path.abspath(args.root), ROOT)}
  net = effnetv2_train.TrainableModel(args.model, learning_rate=0.016, weight_decay=1e-5, label_smoothing=0.1, dtype='bf16', seed=0,
                                      use_graph=True, image_size=args.image_size,
                                      **({'transformations': 'flip'} if args.decode_crop else {}))
  crop = {'decode_crop': True} if args.decode_crop else {}
  out['decode_crop'] = bool(args.decode_crop)
  if args.decode_crop and args.mode == 'hand':
    sys.exit('--decode_crop needs the reader: --mode fit or hand_reader')
  rng = np.random.default_rng(args.seed)
  labels = rng.integers(0, CLASSES, n)

  if args.mode == 'hand':
    decoder = jpeg.JpegDecoder(b, canvas, canvas, depth=1, threads=args.threads)
    batches = []
    for k in range(2):
      raw, sizes = decoder.decode([data] * b)
      batches.append(((raw.clone(), sizes.copy()), labels[k * b:(k + 1) * b].astype(np.int32)))
    torch.cuda.synchronize()
    for k in range(3):      # eager, capture, replay
      net.train_step(batches[k % 2], sync_loss=False)
    torch.cuda.synchronize()
    rates = []
    for _ in range(args.rounds + 1):
      t0 = time.perf_counter()
      for k in range(args.steps):
        net.train_step(batches[k % 2], sync_loss=False)
      torch.cuda.synchronize()
      rates.append(args.steps * b / (time.perf_counter() - t0))
    out['hand_images_per_s'] = stats(rates[1:])
    out['rates'] = [round(r, 1) for r in rates[1:]]
    print(json.dumps(out))
    return

  from automl_amd import effnetv2_datasets, tfrecord
  with tempfile.TemporaryDirectory() as tmp:
    per = (n + args.shards - 1) // args.shards
    for s in range(args.shards):
      with tfrecord.TFRecordWriter(os.path.join(tmp, 'train-%05d-of-%05d' % (s, args.shards))) as w:
        for i in range(s * per, min(n, (s + 1) * per)):
          w.write(tfrecord.encode_example({'image/encoded': data, 'image/class/label': [int(labels[i]) + 1]}))
    inp = effnetv2_datasets.ImageNetInput(True, tmp, 'trainval', seed=args.seed)
    if args.mode == 'hand_reader':
      reader = inp(b, canvas=(canvas, canvas), depth=2, threads=args.threads, **crop)
      for _ in range(3):      # eager, capture, replay
        net.train_step(next(reader), sync_loss=False)
      torch.cuda.synchronize()
      rates = []
      for _ in range(args.rounds + 1):
        t0 = time.perf_counter()
        for _ in range(args.steps):
          net.train_step(next(reader), sync_loss=False)
        torch.cuda.synchronize()
        rates.append(args.steps * b / (time.perf_counter() - t0))
      reader.close()
      out['hand_reader_images_per_s'] = stats(rates[1:])
      out['rates'] = [round(r, 1) for r in rates[1:]]
      print(json.dumps(out))
      return
    # ---- the reader alone: the host half, then reader + decoder
    host, rates = inp.host_reader(b, depth=2, threads=args.threads, **crop), []
    for _ in range(args.rounds + 1):
      t0 = time.perf_counter()
      for _ in range(args.steps):
        next(host)
      rates.append(args.steps * b / (time.perf_counter() - t0))
    host.close()
    out['host_records_per_s'] = stats(rates[1:])
    reader, rates = inp(b, canvas=(canvas, canvas), depth=2, threads=args.threads, **crop), []
    for _ in range(args.rounds + 1):
      t0 = time.perf_counter()
      for _ in range(args.steps):
        next(reader)
      torch.cuda.synchronize()
      rates.append(args.steps * b / (time.perf_counter() - t0))
    reader.close()
    out['reader_images_per_s'] = stats(rates[1:])
    # ---- fit over the reader
    reader = inp(b, canvas=(canvas, canvas), depth=2, threads=args.threads, **crop)
    net.fit(reader, epochs=1, steps_per_epoch=3, verbose=0)      # eager, capture, replay
    timer = EpochTimer()
    history = net.fit(reader, epochs=args.rounds + 1, steps_per_epoch=args.steps, callbacks=[timer], verbose=0)
    reader.close()
  rates = [args.steps * b / s for s in timer.seconds[1:]]
  out['fit_images_per_s'] = stats(rates)
  out['rates'] = [round(r, 1) for r in rates]
  out['last_loss'] = history.history['loss'][-1]
  print(json.dumps(out))


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--mode', choices=['fit', 'hand', 'hand_reader'], default='fit')
  ap.add_argument('--root', default=ROOT, help='where the package is taken from (--mode hand: a checkout of the parent commit)')
  ap.add_argument('--model', default='efficientnetv2-s')
  ap.add_argument('--images', type=int, default=2048)
  ap.add_argument('--shards', type=int, default=8)
  ap.add_argument('--batch', type=int, default=256)
  ap.add_argument('--canvas', type=int, default=512)
  ap.add_argument('--image_size', type=int, default=224)
  ap.add_argument('--threads', type=int, default=16)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--steps', type=int, default=8)
  ap.add_argument('--seed', type=int, default=0)
  ap.add_argument('--decode_crop', action='store_true', help='the reader draws the crop and decodes only that window')
  main(ap.parse_args())
