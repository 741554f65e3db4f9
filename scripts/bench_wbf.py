#!/usr/bin/env python3
"""Times wbf.ensemble_detections_batch (automl_amd/wbf.py) on a synthetic flip test-time-augmentation batch: 64 images x 200
rows (two passes of 100), 90 classes.  The second pass's rows are jittered copies of the first's; each pass ends in -1e5
padding rows of class 0.  Prints one JSON line: the median and the fastest of --repeats calls (device tensors in, device
tensors out, one synchronisation at the end), the time of the two kernels alone, and, with --host-images N, the time of the
numpy restatement (tests/wbf_ref.py) on the first N images for scale.  No time is required of it: nothing earlier exists to
compare with."""
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

from automl_amd import _lib, wbf      # noqa: E402


def synthetic(images, rows, classes, seed):
  """detections [images, rows, 7]: rows // 2 rows of a plain pass, of which the last tenth is padding, then a mirrored pass
  whose real rows are the plain ones moved by a few percent of their size, three in four with the same class."""
  rng = np.random.default_rng(seed)
  half = rows // 2
  real = half - half // 10
  x, y = rng.uniform(0, 500, (2, images, half))
  w, h = np.exp(rng.uniform(np.log(8), np.log(300), (2, images, half)))
  cls = rng.integers(1, classes, (images, half)).astype(np.float64)
  score = rng.uniform(0.05, 1.0, (images, half))
  ids = np.repeat(np.arange(images, dtype=np.float64)[:, None], half, 1)
  plain = np.stack([ids, x, y, x + w, y + h, score, cls], -1)
  jit = rng.normal(0, 0.04, (4, images, half))
  same = rng.random((images, half)) < 0.75
  other = np.stack([ids, x + jit[0] * w, y + jit[1] * h, x + w + jit[2] * w, y + h + jit[3] * h,
                    score * rng.uniform(0.7, 1.0, (images, half)),
                    np.where(same, cls, rng.integers(1, classes, (images, half)))], -1)
  for p in (plain, other):
    p[:, real:, 1:5] = 0
    p[:, real:, 5] = -1e5
    p[:, real:, 6] = 0
  return np.concatenate([plain, other], 1).astype(np.float32)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--images', type=int, default=64)
  ap.add_argument('--rows', type=int, default=200)
  ap.add_argument('--classes', type=int, default=90)
  ap.add_argument('--repeats', type=int, default=30)
  ap.add_argument('--host-images', type=int, default=0)
  args = ap.parse_args()
  _lib.load()
  params = {'num_classes': args.classes}
  det = synthetic(args.images, args.rows, args.classes, 0)
  dev = torch.from_numpy(det).cuda()
  torch.cuda.synchronize()
  times, kernel_ms, counts = [], [], None
  for _ in range(args.repeats + 1):      # the first one warms up
    prof = _lib.Profiler({'edet_wbf_cluster', 'edet_wbf_order'})
    _lib.profiler = prof
    t0 = time.perf_counter()
    _, counts = wbf.ensemble_detections_batch(params, dev, 2)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
    _lib.profiler = None
    kernel_ms.append({k: round(v[1], 4) for k, v in prof.summary().items()})
  times = sorted(times[1:])
  counts = counts.cpu().numpy()
  out = {'images': args.images, 'rows_per_image': args.rows, 'classes': args.classes,
         'call_ms_median': round(1e3 * times[len(times) // 2], 3), 'call_ms_min': round(1e3 * times[0], 3),
         'kernel_ms': kernel_ms[-1], 'clusters_per_image': round(float(counts.mean()), 1)}
  if args.host_images:
    from tests import wbf_ref
    n = min(args.host_images, args.images)
    t0 = time.perf_counter()
    _, host_counts = wbf_ref.ensemble_detections_batch(params, det[:n], 2)
    out['restatement_images'] = n
    out['restatement_s'] = round(time.perf_counter() - t0, 3)
    out['restatement_counts_agree'] = bool(np.array_equal(host_counts, counts[:n]))
  print(json.dumps(out))


if __name__ == '__main__':
  main()
