#!/usr/bin/env python3
"""Lion against SGD-momentum on one MI355X, for LABNOTES.md (NOT the bench.py line).  One phase per process, one JSON line each:
  opt   edet_opt_lion_ema and edet_opt_sgd_ema on the EfficientDet-D0 arena (the same seven arrays per element): HIP events
        around `--launches` launches each, alternating, `--reps` repetitions -> medians, spreads (max - min), implied GB/s;
  step  ms per EfficientDetNetTrain.train_step of bench.py's workload (D0, 640 x 640, batch 128, bf16, hipGraph replay, its
        synthetic batch) with `--optimizer sgd|lion`.  Run the two in alternation, three processes each, and compare the
        medians with the spread."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from automl_amd import _lib, engine as engine_lib, hparams_config, netspec, train_lib  # noqa: E402
from automl_amd._lib import call, ptr  # noqa: E402


def bench_opt(args):
  config = hparams_config.get_efficientdet_config(args.model)
  spec = netspec.NetSpec(config)
  a = engine_lib.ParamArena(spec, 'cuda:0', netspec.init_params(spec, 0))
  n = a.n_train_elems
  a.grads_flat.copy_(torch.randn(n, device='cuda:0') * 1e-2)
  hyper = torch.tensor([1e-6, 0.9999], dtype=torch.float32, device='cuda:0')
  st = torch.cuda.current_stream().cuda_stream
  common = (ptr(a.ema), ptr(a.seg_offsets), ptr(a.seg_factor), ptr(a.seg_flags), a.nseg, ptr(hyper))

  def sgd():
    call('edet_opt_sgd_ema', ptr(a.params_flat), ptr(a.grads_flat), ptr(a.velocity), *common, 0.9, st)

  def lion():
    call('edet_opt_lion_ema', ptr(a.params_flat), ptr(a.grads_flat), ptr(a.velocity), *common, 0.9, 0.99, 0.0, st)
  rules = (('sgd', sgd), ('lion', lion))
  times = {name: [] for name, _ in rules}
  for _, fn in rules:
    for _ in range(5):
      fn()
  torch.cuda.synchronize()
  for _ in range(args.reps):
    for name, fn in rules:
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(args.launches):
        fn()
      e1.record()
      torch.cuda.synchronize()
      times[name].append(e0.elapsed_time(e1) / args.launches)
  out = {'phase': 'opt', 'model': args.model, 'arena_elems': n, 'segments': a.nseg, 'launches': args.launches, 'reps': args.reps}
  nbytes = 7 * 4 * n      # reads g, w, the slot, ema; writes w, the slot, ema
  for name, t in times.items():
    med = float(np.median(t))
    out[name] = {'median_ms': round(med, 5), 'spread_ms': round(max(t) - min(t), 5), 'min_ms': round(min(t), 5),
                 'bytes_per_launch': nbytes, 'GBps': round(nbytes / (med * 1e-3) / 1e9, 1)}
  out['lion_within_sgd_plus_spread'] = out['lion']['median_ms'] <= out['sgd']['median_ms'] + out['sgd']['spread_ms']
  print(json.dumps(out))


def bench_step(args):
  import bench      # the flagship's synthetic batch
  config = hparams_config.get_efficientdet_config(args.model)
  config.override('image_size=%d' % args.size)
  config.override('optimizer=%s' % args.optimizer)
  net = train_lib.EfficientDetNetTrain(config=config, dtype='bf16', seed=0, global_batch_size=args.batch, steps_per_epoch=1000,
                                       use_graph=True)
  eng = net._ensure_engine(args.batch, args.size, args.size)
  images, labels = bench.synth_batch(config, args.batch, args.size, 3, 'cuda:0', eng.tdtype)
  labels.pop('normalizer')
  first = net.train_step((images, labels))
  for _ in range(max(args.warmup, 3)):
    net.train_step((images, labels), sync_loss=False)
  images, labels = net.input_buffers()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(args.steps):
    net.train_step((images, labels), sync_loss=False)
  torch.cuda.synchronize()
  dt = (time.perf_counter() - t0) / args.steps
  last = net.train_step((images, labels))
  print(json.dumps({'phase': 'step', 'workload': '%s %dx%d batch %d bf16 train_step, optimizer=%s, hipGraph replay' % (
      args.model, args.size, args.size, args.batch, args.optimizer), 'ms_per_step': round(dt * 1e3, 3),
      'images_per_sec': round(args.batch / dt, 1), 'first_loss': first['loss'], 'last_loss': last['loss'], 'steps': args.steps}))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('phase', choices=['opt', 'step'])
  ap.add_argument('--model', default='efficientdet-d0')
  ap.add_argument('--optimizer', default='lion', choices=['sgd', 'lion'])
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--size', type=int, default=640)
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--launches', type=int, default=20)
  ap.add_argument('--reps', type=int, default=11)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_lion.py needs an MI355X: there is no CPU path and no CPU timing')
  _lib.load()
  {'opt': bench_opt, 'step': bench_step}[args.phase](args)


if __name__ == '__main__':
  main()
