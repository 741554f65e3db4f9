#!/usr/bin/env python3
"""edet_crop_resize_bicubic beside edet_crop_resize on one MI355X, for LABNOTES.md "Legacy EfficientNet input" (NOT the
bench.py line, and nothing here is read by bench.py).

  --mode kernel   (default) both kernels on the same rows: batch `--batch` on a `--canvas` x `--canvas` canvas of random bytes,
                  image sizes cycling through an ImageNet-like mix (SIZE_MIX below: the common 500 x 375 / 375 x 500 and their
                  neighbours, one square, one small image; cut to the canvas), rows = preprocess_legacy.legacy_train_rows at
                  the output size from a fixed seed; outputs `--sizes` (192 and 224), uint8 and bf16 (bicubic bf16 with the
                  mean / stddev normalisation, as the step runs it).  Per configuration `--rounds` rounds ALTERNATING the two
                  kernels, each round `--launches` launches between two device events after a warm-up; the line has the median
                  microseconds per launch of each kernel with the spread (max - min) over the rounds, their ratio, the bytes
                  each launch writes and -- counted on the host from the rows -- the source bytes inside the crops, so that a
                  bandwidth figure can be named for what it is.
  --mode step     one efficientnetv2-b0 training step, size `--image_size` (192), batch `--batch`, bf16, replayed from its
                  hipGraph: the legacy front (preprocessing='legacy', augment_name='autoaug') and the V2 front
                  (augname='randaug', magnitude 15), in ONE process, alternating `--rounds` rounds of `--steps` steps, each
                  round ending in one synchronisation; milliseconds per step, median and spread.  `--front NAME` runs one
                  front alone, so that a kernel trace of the process belongs to it.

Prints one JSON line per configuration.  No threshold is asserted here."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIZE_MIX = [(375, 500), (500, 375), (333, 500), (500, 333), (400, 500), (480, 512), (500, 500), (281, 500), (512, 384), (150, 200)]


def stats(values, digits=2):
  return {'median': round(float(np.median(values)), digits), 'spread': round(float(max(values) - min(values)), digits),
          'rounds': len(values)}


def kernel_mode(args):
  import torch
  from automl_amd import preprocess_legacy as pl, v2_preprocessing as vp
  b, c = args.batch, args.canvas
  rng = np.random.default_rng(args.seed)
  raw = torch.from_numpy(rng.integers(0, 256, (b, c, c, 3), dtype=np.uint8)).cuda()
  sizes = np.array([(min(h, c), min(w, c)) for h, w in (SIZE_MIX[i % len(SIZE_MIX)] for i in range(b))], np.int32)
  stream = torch.cuda.current_stream().cuda_stream
  for size in args.sizes:
    rows = pl.legacy_train_rows(np.random.default_rng(args.seed + 1), sizes, size)
    rows_dev = torch.from_numpy(rows).cuda()
    crop_bytes = int((rows[:, 4].astype(np.int64) * rows[:, 5]).sum()) * 3
    for dtype in (torch.uint8, torch.bfloat16):
      out = torch.empty((b, size, size, 3), dtype=dtype, device='cuda')
      runs = {'bilinear': lambda: vp.launch(raw, rows_dev, out, stream),
              'bicubic': lambda: vp.launch(raw, rows_dev, out, stream, 'bicubic', None if dtype is torch.uint8 else pl.NORM)}
      for fn in runs.values():
        for _ in range(args.warmup):
          fn()
      torch.cuda.synchronize()
      us = {name: [] for name in runs}
      for _ in range(args.rounds):
        for name, fn in runs.items():      # alternating
          start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          start.record()
          for _ in range(args.launches):
            fn()
          end.record()
          end.synchronize()
          us[name].append(start.elapsed_time(end) * 1000.0 / args.launches)
      line = {'mode': 'kernel', 'batch': b, 'canvas': c, 'out_size': size, 'out_dtype': str(dtype).replace('torch.', ''),
              'launches_per_round': args.launches, 'written_bytes': out.numel() * out.element_size(), 'crop_bytes': crop_bytes,
              'bilinear_us': stats(us['bilinear']), 'bicubic_us': stats(us['bicubic'])}
      line['ratio'] = round(line['bicubic_us']['median'] / line['bilinear_us']['median'], 3)
      print(json.dumps(line), flush=True)


def step_mode(args):
  import torch
  from automl_amd import effnetv2_train
  b, c, size = args.batch, args.canvas, args.image_size
  rng = np.random.default_rng(args.seed)
  sizes = np.array([(min(h, c), min(w, c)) for h, w in (SIZE_MIX[i % len(SIZE_MIX)] for i in range(b))], np.int32)
  batches = [((torch.from_numpy(rng.integers(0, 256, (b, c, c, 3), dtype=np.uint8)).cuda(), sizes), rng.integers(0, 1000, b).astype(np.int32))
             for _ in range(2)]
  common = dict(learning_rate=0.016, weight_decay=1e-5, label_smoothing=0.1, dtype='bf16', seed=0, use_graph=True, image_size=size)
  make = {'legacy_autoaug': lambda: effnetv2_train.TrainableModel(args.model, preprocessing='legacy', augment_name='autoaug', **common),
          'v2_randaug': lambda: effnetv2_train.TrainableModel(args.model, augname='randaug', ra_magnitude=15, **common)}
  nets = {name: fn() for name, fn in make.items() if args.front in ('both', name)}      # (one front: for a kernel trace)
  for net in nets.values():
    for k in range(3):      # eager, capture, replay
      net.train_step(batches[k % 2], sync_loss=False)
  torch.cuda.synchronize()
  ms = {name: [] for name in nets}
  for _ in range(args.rounds):
    for name, net in nets.items():      # alternating
      t0 = time.perf_counter()
      for k in range(args.steps):
        net.train_step(batches[k % 2], sync_loss=False)
      torch.cuda.synchronize()
      ms[name].append((time.perf_counter() - t0) * 1000.0 / args.steps)
  line = {'mode': 'step', 'model': args.model, 'batch': b, 'canvas': c, 'image_size': size, 'dtype': 'bf16', 'steps_per_round': args.steps}
  for name in nets:
    line[name + '_ms'] = stats(ms[name], 3)
  if len(nets) == 2:
    line['ratio'] = round(line['legacy_autoaug_ms']['median'] / line['v2_randaug_ms']['median'], 4)
  print(json.dumps(line), flush=True)


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--mode', default='kernel', choices=['kernel', 'step'])
  ap.add_argument('--batch', type=int, default=256)
  ap.add_argument('--canvas', type=int, default=512)
  ap.add_argument('--sizes', type=int, nargs='+', default=[192, 224])
  ap.add_argument('--image_size', type=int, default=192)
  ap.add_argument('--model', default='efficientnetv2-b0')
  ap.add_argument('--front', default='both', choices=['both', 'legacy_autoaug', 'v2_randaug'],
                  help='--mode step: time both fronts alternating, or run one alone (under a profiler)')
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--launches', type=int, default=200)
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=20)
  ap.add_argument('--seed', type=int, default=0)
  args = ap.parse_args()
  sys.path.insert(0, ROOT)
  import torch
  if not torch.cuda.is_available():
    sys.exit('bench_crop.py needs an MI355X')
  (kernel_mode if args.mode == 'kernel' else step_mode)(args)


if __name__ == '__main__':
  main()
