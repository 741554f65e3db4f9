#!/usr/bin/env python3
"""EfficientDetNetTrain.fit on one MI355X, for LABNOTES.md "Detector training driver" (NOT the bench.py line, and nothing here is
read by bench.py).  The workload is the `step` figure of scripts/bench_tfrecord.py, side A: the same `--images` records in
`--shards` shards (its make_jpegs / make_annotations, the same seed), D0 at `--image_size`, batch `--batch`, bf16, the step
replayed from its hipGraph, fed by dataloader.InputReader on a 480 x 640 canvas -- but driven by fit instead of a hand loop.

After a warm-up fit of three steps (eager, capture, replay) one fit runs `--rounds` + 1 epochs of `--steps` steps.  An epoch
is timed from on_epoch_begin to on_epoch_end: fit reads its loss accumulator in between, which waits for the device, so the
interval holds the epoch's steps as the hand loop's round holds them between two synchronisations.  The first epoch is not
kept.  Prints one JSON line: images/s as the median of the epochs with the spread (max - min) beside it, as bench_tfrecord.py
does.  The comparison -- this against bench_tfrecord.py's A_reader on the parent commit, processes alternating -- is the
caller's; no ratio is asserted here."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bench_tfrecord      # noqa: E402  (the data of its step figure)


class EpochTimer(object):
  def __init__(self):
    self.seconds = []

  def on_epoch_begin(self, epoch, logs=None):
    self._t0 = time.perf_counter()

  def on_epoch_end(self, epoch, logs=None):
    self.seconds.append(time.perf_counter() - self._t0)


def main(args):
  sys.path.insert(0, ROOT)
  import torch
  from automl_amd import dataloader, hparams_config, tfrecord, train_lib
  if not torch.cuda.is_available():
    sys.exit('bench_fit.py needs an MI355X')
  jpegs, source = bench_tfrecord.make_jpegs(args.distinct, args.seed)
  n, b = args.images, args.batch
  boxes, classes = bench_tfrecord.make_annotations(n, args.seed)
  with tempfile.TemporaryDirectory() as tmp:
    per = (n + args.shards - 1) // args.shards
    for s in range(args.shards):
      with tfrecord.TFRecordWriter(os.path.join(tmp, 'train-%05d-of-%05d.tfrecord' % (s, args.shards))) as w:
        for i in range(s * per, min(n, (s + 1) * per)):
          w.write(tfrecord.encode_example({
              'image/encoded': jpegs[i % len(jpegs)], 'image/source_id': str(i), 'image/height': 480, 'image/width': 640,
              'image/object/bbox/ymin': boxes[i, :, 0], 'image/object/bbox/xmin': boxes[i, :, 1],
              'image/object/bbox/ymax': boxes[i, :, 2], 'image/object/bbox/xmax': boxes[i, :, 3],
              'image/object/class/label': classes[i], 'image/object/is_crowd': np.zeros(8, np.int64),
              'image/object/area': np.ones(8, np.float32)}))
    config = hparams_config.get_efficientdet_config('efficientdet-d0')
    config.override('image_size=%d' % args.image_size)
    params = config.as_dict()
    params['tf_random_seed'] = args.seed
    reader = dataloader.InputReader(os.path.join(tmp, 'train-*.tfrecord'), is_training=True).reader(
        params, batch_size=b, canvas=(480, 640), depth=2, threads=args.threads)
    net = train_lib.EfficientDetNetTrain(config=config, dtype='bf16', seed=0, global_batch_size=b, steps_per_epoch=1000, use_graph=True)
    net.fit(reader, epochs=1, steps_per_epoch=3, verbose=0)      # eager, capture, replay
    timer = EpochTimer()
    history = net.fit(reader, epochs=args.rounds + 1, steps_per_epoch=args.steps, callbacks=[timer], verbose=0)
    reader.close()
  rates = [args.steps * b / s for s in timer.seconds[1:]]
  print(json.dumps({'images': n, 'shards': args.shards, 'batch': b, 'jpeg': source, 'rounds': args.rounds, 'steps_per_round': args.steps,
                    'image_size': args.image_size, 'dtype': 'bf16', 'fit_images_per_s': bench_tfrecord.stats(rates),
                    'rates': [round(r, 1) for r in rates], 'last_loss': history.history['loss'][-1]}))


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--images', type=int, default=1024)
  ap.add_argument('--shards', type=int, default=4)
  ap.add_argument('--distinct', type=int, default=16)
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--threads', type=int, default=16)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--steps', type=int, default=8)
  ap.add_argument('--image_size', type=int, default=640)
  ap.add_argument('--seed', type=int, default=0)
  main(ap.parse_args())
