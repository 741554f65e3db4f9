#!/usr/bin/env python3
"""The detector's input stage on one MI355X, for LABNOTES.md (NOT the bench.py line).  One phase per process, one JSON line each:
  gridmask  edet_gridmask alone on a `--batch` x `--height` x `--width` uint8 batch with one step's drawn rows, every image
            masked: HIP events around `--launches` launches, `--reps` repetitions -> median, spread, bytes read + written,
            implied GB/s and its share of the measured float4 copy rate (6.29 TB/s).  With `--rotate N` the launches walk over
            N batches (N x 2 x batch bytes: larger than the 256 MiB Infinity Cache when N is large enough); with the default 1
            they reuse one batch of 126 MB in and 126 MB out, which the cache holds -- say which one a figure is;
  step      ms per EfficientDetNetTrain step of `--model` at its own image size, batch `--batch`, bf16, hipGraph replay:
            train_step_raw from a raw uint8 batch of `--height` x `--width` with `--boxes` box rows per image (GridMask on with
            `--grid-mask`, the box-aware AutoAugment with `--autoaugment v2`), next to train_step fed from input_buffers() (no input work at all), alternating, `--reps`
            repetitions of `--steps` steps each -> medians and spreads.
With `--canvas` both phases run on a CANVAS batch of `--height` x `--width` with per-image sizes (edet_gridmask_canvas;
train_step_raw fed ((raw, sizes), ...)): `--sizes full` (default) makes every size equal to the canvas -- the same bytes and
the same work as the dense run, which is what the two are compared on -- and `--sizes mix` draws them from SIZE_MIX below with
a fixed seed.  The gridmask phase then counts the bytes of the images' own sizes, not of the canvas."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from automl_amd import gridmask as gm, hparams_config, train_lib  # noqa: E402

COPY_RATE = 6.29e12      # bytes / s: the float4 copy of the microarchitecture notes
# `--sizes mix`: (height, width, weight), drawn with seed 3 and clipped into the canvas.  Shaped like COCO's image sizes -- the
# longer side 640 for most, 4:3 landscape the most common, then 3:2 landscape, portrait and a few smaller ones -- but the
# weights are round numbers, not measured from the data set.
SIZE_MIX = ((480, 640, 0.45), (427, 640, 0.25), (640, 480, 0.15), (640, 427, 0.05), (375, 500, 0.05), (360, 640, 0.05))


def canvas_sizes(args):
  """None without --canvas, else int32 [batch, 2] inside the --height x --width canvas."""
  if not args.canvas:
    return None
  if args.sizes == 'full':
    return np.tile(np.asarray([args.height, args.width], np.int32), (args.batch, 1))
  pick = np.random.default_rng(3).choice(len(SIZE_MIX), size=args.batch, p=[m[2] for m in SIZE_MIX])
  sizes = np.asarray([SIZE_MIX[k][:2] for k in pick], np.int32)
  return np.minimum(sizes, np.asarray([args.height, args.width], np.int32))


def bench_gridmask(args):
  b, h, w = args.batch, args.height, args.width
  rng = np.random.default_rng(2)
  one = torch.from_numpy(rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)).to('cuda:0')
  srcs = [one] + [one.clone() for _ in range(args.rotate - 1)]
  dsts = [torch.empty_like(one) for _ in range(args.rotate)]
  sizes = canvas_sizes(args)
  hs, ws = (h, w) if sizes is None else (sizes[:, 0], sizes[:, 1])
  rows = gm.gridmask_args(gm.gridmask_draws(gm.gridmask_rng(0), b, hs, ws), hs, ws, prob=1e9)      # every image masked
  dev_rows = gm.args_tensor(rows).to('cuda:0')
  dev_sizes = None if sizes is None else torch.from_numpy(sizes).to('cuda:0')
  st = torch.cuda.current_stream().cuda_stream
  k = 0
  for _ in range(3 * args.rotate):
    gm.apply_mask(srcs[k % args.rotate], dsts[k % args.rotate], dev_rows, st, dev_sizes)
    k += 1
  torch.cuda.synchronize()
  times = []
  for _ in range(args.reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.launches):
      gm.apply_mask(srcs[k % args.rotate], dsts[k % args.rotate], dev_rows, st, dev_sizes)
      k += 1
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) / args.launches)
  med = float(np.median(times))
  nbytes = 2 * one.numel() if sizes is None else 2 * 3 * int((sizes[:, 0].astype(np.int64) * sizes[:, 1]).sum())
  rate = nbytes / (med * 1e-3)
  kept = float((dsts[0] != 0).float().mean())
  print(json.dumps({'phase': 'gridmask', 'batch': b, 'height': h, 'width': w, 'canvas': bool(args.canvas),
                    'sizes': args.sizes if args.canvas else None, 'launches': args.launches, 'reps': args.reps,
                    'buffers_walked': args.rotate, 'footprint_bytes': args.rotate * nbytes,
                    'cache_resident': args.rotate * nbytes <= 256 << 20, 'median_ms': round(med, 5),
                    'spread_ms': round(max(times) - min(times), 5), 'min_ms': round(min(times), 5), 'bytes_per_launch': nbytes,
                    'GBps': round(rate / 1e9, 1), 'share_of_float4_copy_rate': round(rate / COPY_RATE, 3),
                    'bytes_kept_fraction': round(kept, 3)}))


def bench_step(args):
  config = hparams_config.get_efficientdet_config(args.model)
  if args.grid_mask:
    config.override('grid_mask=true')
  net = train_lib.EfficientDetNetTrain(config=config, dtype='bf16', steps_per_epoch=1000, global_batch_size=args.batch,
                                       use_graph=True)
  if args.autoaugment:
    net.set_autoaugment(args.autoaugment)
  b, m = args.batch, args.boxes
  rng = np.random.default_rng(2)
  raw = torch.from_numpy(rng.integers(0, 256, (b, args.height, args.width, 3), dtype=np.uint8)).to('cuda:0')
  y0, x0 = rng.uniform(0.0, 0.6, (b, m)), rng.uniform(0.0, 0.6, (b, m))
  boxes = torch.from_numpy(np.stack([y0, x0, y0 + rng.uniform(0.1, 0.4, (b, m)), x0 + rng.uniform(0.1, 0.4, (b, m))], -1)
                           .astype(np.float32)).to('cuda:0')
  classes = torch.from_numpy(rng.integers(1, config.num_classes + 1, (b, m)).astype(np.float32)).to('cuda:0')
  counts = torch.from_numpy(rng.integers(0, m + 1, b).astype(np.int32)).to('cuda:0')
  sizes = canvas_sizes(args)
  data = (raw if sizes is None else (raw, sizes), boxes, classes, counts)
  first = net.train_step_raw(data)
  for _ in range(max(args.warmup, 2)):
    net.train_step_raw(data, sync_loss=False)
  torch.cuda.synchronize()
  fed = net.input_buffers()

  def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
      fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.steps
  times = {'train_step_raw': [], 'train_step': []}
  for _ in range(args.reps):
    times['train_step_raw'].append(timed(lambda: net.train_step_raw(data, sync_loss=False)))
    times['train_step'].append(timed(lambda: net.train_step(fed, sync_loss=False)))
  out = {'phase': 'step', 'model': args.model, 'batch': b, 'image_size': config.image_size, 'raw': [args.height, args.width],
         'canvas': bool(args.canvas), 'sizes': args.sizes if args.canvas else None,
         'box_rows': m, 'grid_mask': bool(args.grid_mask), 'autoaugment': args.autoaugment or None, 'steps': args.steps, 'reps': args.reps,
         'first_loss': round(float(first['loss']), 4)}
  for name, t in times.items():
    out[name] = {'median_ms': round(float(np.median(t)), 3), 'spread_ms': round(max(t) - min(t), 3), 'min_ms': round(min(t), 3)}
  out['input_stage_ms'] = round(out['train_step_raw']['median_ms'] - out['train_step']['median_ms'], 3)
  print(json.dumps(out))


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('phase', choices=['gridmask', 'step'])
  ap.add_argument('--model', default='efficientdet-d0')
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--width', type=int, default=640)
  ap.add_argument('--boxes', type=int, default=100)
  ap.add_argument('--grid-mask', action='store_true')
  ap.add_argument('--autoaugment', default='')
  ap.add_argument('--canvas', action='store_true')
  ap.add_argument('--sizes', choices=['full', 'mix'], default='full')
  ap.add_argument('--rotate', type=int, default=1)
  ap.add_argument('--launches', type=int, default=20)
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('bench_det_input.py needs an MI355X: nothing is measured without one')
  {'gridmask': bench_gridmask, 'step': bench_step}[a.phase](a)
