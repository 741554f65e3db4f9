#!/usr/bin/env python3
"""Times EvaluationMetric.result() (automl_amd/coco_metric.py) on a synthetic state of COCO val's size: 5,000 images x 100
detections, about 7 ground truths per image, 80 classes, fed as device tensors in batches.  Prints one JSON line: the median
and the fastest of --repeats evaluations (each from update_state's tensors to the float32 result on the host), the time of the
two kernels alone, and, with --host-images N, the time of the numpy restatement (tests/coco_ref.py) on the first N images for
scale.  No time is required of it: nothing earlier exists to compare with."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from automl_amd import _lib, coco_metric as cm      # noqa: E402


def synthetic(images, dets, gts_mean, classes, seed):
  """groundtruth_data [images, 32, 7] and detections [images, dets, 7]: about half of the detection rows are jittered copies
  of a ground truth of their image with a high score, the rest is low-score clutter of random classes."""
  rng = np.random.default_rng(seed)
  m = 32
  count = np.clip(rng.poisson(gts_mean, images), 1, m)
  y, x = rng.uniform(0, 500, (2, images, m))
  h, w = np.exp(rng.uniform(np.log(8), np.log(300), (2, images, m)))
  cls = rng.integers(1, classes + 1, (images, m)).astype(np.float64)
  cls[np.arange(m)[None, :] >= count[:, None]] = -1
  gt = np.stack([y, x, y + h, x + w, rng.random((images, m)) < 0.05, h * w, cls], -1).astype(np.float32)
  src = rng.integers(0, m, (images, dets)) % count[:, None]
  take = lambda a: np.take_along_axis(a, src, 1)
  hit = rng.random((images, dets)) < 0.5
  jit = rng.normal(0, 0.08, (4, images, dets))
  dx = np.where(hit, take(x) + jit[0] * take(w), rng.uniform(0, 500, (images, dets)))
  dy = np.where(hit, take(y) + jit[1] * take(h), rng.uniform(0, 500, (images, dets)))
  dw = np.where(hit, take(w) * np.exp(jit[2]), np.exp(rng.uniform(np.log(8), np.log(300), (images, dets))))
  dh = np.where(hit, take(h) * np.exp(jit[3]), np.exp(rng.uniform(np.log(8), np.log(300), (images, dets))))
  dc = np.where(hit, take(cls), rng.integers(1, classes + 1, (images, dets)))
  score = np.where(hit, rng.uniform(0.3, 1.0, (images, dets)), rng.uniform(0.0, 0.4, (images, dets)))
  det = np.stack([np.full((images, dets), -1.0), dx, dy, dw, dh, score, dc], -1).astype(np.float32)
  return gt, det


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--images', type=int, default=5000)
  ap.add_argument('--dets', type=int, default=100)
  ap.add_argument('--gts', type=float, default=7.0)
  ap.add_argument('--classes', type=int, default=80)
  ap.add_argument('--batch', type=int, default=100)
  ap.add_argument('--repeats', type=int, default=30)
  ap.add_argument('--host-images', type=int, default=0)
  args = ap.parse_args()
  _lib.load()
  gt, det = synthetic(args.images, args.dets, args.gts, args.classes, 0)
  metric = cm.EvaluationMetric()
  for i in range(0, args.images, args.batch):
    metric.update_state(torch.from_numpy(gt[i:i + args.batch]).cuda(), torch.from_numpy(det[i:i + args.batch]).cuda())
  torch.cuda.synchronize()
  times, kernel_ms, stats = [], [], None
  for _ in range(args.repeats + 1):      # the first one warms up
    metric.metric_values = None
    prof = _lib.Profiler({'edet_coco_match', 'edet_coco_accumulate'})
    _lib.profiler = prof
    t0 = time.perf_counter()
    stats = metric.result()
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
    _lib.profiler = None
    kernel_ms.append({k: round(v[1], 3) for k, v in prof.summary().items()})
  times = sorted(times[1:])
  out = {'images': args.images, 'dets_per_image': args.dets, 'classes': args.classes,
         'result_ms_median': round(1e3 * times[len(times) // 2], 2), 'result_ms_min': round(1e3 * times[0], 2),
         'kernel_ms': kernel_ms[-1], 'AP': round(float(stats[0]), 4), 'AR100': round(float(stats[8]), 4)}
  if args.host_images:
    from tests import coco_ref
    n = args.host_images
    host = cm.EvaluationMetric()
    host.update_state(gt[:n], det[:n])
    _, dt, g, cats = host.packed_state('cpu')
    t0 = time.perf_counter()
    coco_ref.evaluate(dt.numpy(), g.numpy(), cats.numpy())
    out['restatement_images'] = n
    out['restatement_s'] = round(time.perf_counter() - t0, 2)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
