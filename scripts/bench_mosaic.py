#!/usr/bin/env python3
"""Mosaic on one MI355X, for LABNOTES.md (NOT the bench.py line).  One process, one JSON line.

Workload: `--groups` mosaics of `--out` x `--out` from a `--batch`-image canvas batch of `--height` x `--width` (every image
fills its canvas), drawn by mosaic_draws with a fixed seed; `--boxes` box rows per image for the box kernel.  Timed with HIP
events around `--launches` launches, `--reps` rounds, the candidates ALTERNATING inside every round:
  edet_mosaic        uint8 output and float32 output
  edet_mosaic_boxes
  edet_crop_resize   the yardstick on the same commit: the same number of output pixels (`--groups` images of `--out` x `--out`)
                     from the same canvas, every image resized whole -- the same taps and stores per pixel, one source per image
  edet_crop_resize x 4   the same canvas resized whole to `--out`/2 x `--out`/2, four launches into four buffers: the same number
                     of output pixels again, and -- like a mosaic, whose four quadrants each shrink a WHOLE source image --
                     four passes over the source bytes instead of one
-> per candidate the median, the spread (max - min over the rounds) and the minimum; the ratio of edet_mosaic to
edet_crop_resize per output kind; and the byte floor: the source bytes read once plus the output bytes written, at HBM_RATE.
The sources (`--batch` x `--height` x `--width` x 3 bytes) and a uint8 output fit the 256 MiB Infinity Cache together at the
default sizes only in part; the float32 output (629 MB) does not.  Nothing is rotated: say so with the figures."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from automl_amd import mosaic as mz, v2_preprocessing as vp  # noqa: E402

HBM_RATE = 8.0e12      # bytes / s: the HBM peak README.md's rooflines use


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--groups', type=int, default=128)
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--width', type=int, default=640)
  ap.add_argument('--out', type=int, default=640)
  ap.add_argument('--boxes', type=int, default=100)
  ap.add_argument('--launches', type=int, default=20)
  ap.add_argument('--reps', type=int, default=9)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('bench_mosaic.py needs an MI355X: nothing is measured without one')
  g, b, h, w, o, m = a.groups, a.batch, a.height, a.width, a.out, a.boxes
  rng = np.random.default_rng(2)
  raw = torch.from_numpy(rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)).to('cuda:0')
  index, points = mz.mosaic_draws(np.random.default_rng(3), g, b, (o, o))
  rows = torch.from_numpy(mz.mosaic_rows(index, points, np.tile(np.asarray([h, w], np.int32), (b, 1)))).to('cuda:0')
  crop_rows = torch.from_numpy(vp.whole_rows(b, h, w)[np.arange(g) % b]).to('cuda:0')
  crop_src = raw if g == b else raw[torch.arange(g) % b].contiguous()
  y0, x0 = rng.uniform(0.0, 0.6, (b, m)), rng.uniform(0.0, 0.6, (b, m))
  boxes = torch.from_numpy(np.stack([y0, x0, y0 + rng.uniform(0.1, 0.4, (b, m)), x0 + rng.uniform(0.1, 0.4, (b, m))], -1)
                           .astype(np.float32)).to('cuda:0')
  classes = torch.from_numpy(rng.integers(1, 91, (b, m)).astype(np.float32)).to('cuda:0')
  counts = torch.from_numpy(rng.integers(0, m + 1, b).astype(np.int32)).to('cuda:0')
  out = {k: torch.empty((g, o, o, 3), dtype=t, device='cuda:0') for k, t in (('u8', torch.uint8), ('f32', torch.float32))}
  bo = torch.empty((g, 4 * m, 4), dtype=torch.float32, device='cuda:0')
  co = torch.empty((g, 4 * m), dtype=torch.float32, device='cuda:0')
  no = torch.empty((g,), dtype=torch.int32, device='cuda:0')
  st = torch.cuda.current_stream().cuda_stream
  half = o // 2
  quarter = {k: [torch.empty((g, half, half, 3), dtype=t, device='cuda:0') for _ in range(4)]
             for k, t in (('u8', torch.uint8), ('f32', torch.float32))}

  def four(kind):
    for q in quarter[kind]:
      vp.launch(crop_src, crop_rows, q, st)
  runs = {
      'edet_mosaic_u8': lambda: mz.launch(raw, rows, out['u8'], st),
      'edet_crop_resize_u8': lambda: vp.launch(crop_src, crop_rows, out['u8'], st),
      'edet_mosaic_f32': lambda: mz.launch(raw, rows, out['f32'], st),
      'edet_crop_resize_f32': lambda: vp.launch(crop_src, crop_rows, out['f32'], st),
      'edet_crop_resize_x4_u8': lambda: four('u8'),
      'edet_crop_resize_x4_f32': lambda: four('f32'),
      'edet_mosaic_boxes': lambda: mz.launch_boxes(boxes, classes, counts, rows, (o, o), bo, co, no, st),
  }
  for fn in runs.values():
    for _ in range(3):
      fn()
  torch.cuda.synchronize()
  times = {k: [] for k in runs}
  for _ in range(a.reps):
    for name, fn in runs.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(a.launches):
        fn()
      e1.record()
      torch.cuda.synchronize()
      times[name].append(e0.elapsed_time(e1) / a.launches)
  res = {'groups': g, 'batch': b, 'canvas': [h, w], 'out': [o, o], 'box_rows': m, 'launches': a.launches, 'reps': a.reps,
         'hbm_rate_TBps': HBM_RATE / 1e12, 'buffers_rotated': False}
  for name, t in times.items():
    res[name] = {'median_ms': round(float(np.median(t)), 5), 'spread_ms': round(max(t) - min(t), 5), 'min_ms': round(min(t), 5)}
  src_bytes = raw.numel()
  for kind, size in (('u8', 1), ('f32', 4)):
    nbytes = src_bytes + g * o * o * 3 * size
    floor_ms = nbytes / HBM_RATE * 1e3
    med = res['edet_mosaic_' + kind]['median_ms']
    res['mosaic_over_crop_resize_' + kind] = round(med / res['edet_crop_resize_' + kind]['median_ms'], 4)
    res['mosaic_over_crop_resize_x4_' + kind] = round(med / res['edet_crop_resize_x4_' + kind]['median_ms'], 4)
    res['floor_' + kind] = {'bytes': nbytes, 'floor_ms': round(floor_ms, 5), 'fraction_of_floor_rate': round(floor_ms / med, 4),
                            'GBps': round(nbytes / (med * 1e-3) / 1e9, 1)}
  print(json.dumps(res))


if __name__ == '__main__':
  main()
