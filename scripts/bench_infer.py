#!/usr/bin/env python3
"""Inference preprocessing and flip test-time augmentation on one MI355X, for LABNOTES.md (NOT the bench.py line).  One phase per
process, one JSON line each:
  kernel  the preprocessing launch alone, `--batch` raw uint8 images on a `--height` x `--width` canvas into `--out` x `--out`
          `--dtype` images: HIP events around `--launches` launches, `--reps` rounds; inside a round the variants run one after
          the other, so every variant sees the same machine state -> per variant median, min and spread (max - min) of the ms
          per launch, the bytes the launch has to move (the images' own raw bytes once, every output written once) and the
          implied GB/s.  Variants: dense (edet_preprocess_infer of this tree), canvas_full (edet_preprocess_infer_canvas, every
          size the canvas), canvas_mix (sizes drawn from bench_det_input.SIZE_MIX, seed 3), canvas_full_mirrored /
          canvas_mix_mirrored (both outputs), dense_plus_flip (dense + torch.flip, what the mirrored output replaces), and, with
          `--parent-lib` (a libedet_hip.so built from the parent commit), parent_dense: the same dense call through that library.
          At the default shape the raw batch is 126 MB and one bf16 output 315 MB: more than the 256 MiB Infinity Cache, so the
          figures are streaming figures.
  tta     EfficientDetModel.detect_flip_tta of `--model` at image_size `--out`, end to end (preprocess, two forward passes, two
          generate_detections, WBF), host clock around `--steps` calls that end in a device synchronise, `--reps` rounds
          alternating: dense (the torch.flip path, the parent's code), pair_full and pair_mix (a (raw, sizes) pair: the mirrored
          output), and with `--parent-lib` parent_dense (the dense path with the parent's preprocessing kernel)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from automl_amd import _lib, efficientdet_net, hparams_config, preprocess  # noqa: E402
from bench_det_input import SIZE_MIX  # noqa: E402


def mixed_sizes(args):
  pick = np.random.default_rng(3).choice(len(SIZE_MIX), size=args.batch, p=[m[2] for m in SIZE_MIX])
  sizes = np.asarray([SIZE_MIX[k][:2] for k in pick], np.int32)
  return np.minimum(sizes, np.asarray([args.height, args.width], np.int32))


def full_sizes(args):
  return np.tile(np.asarray([args.height, args.width], np.int32), (args.batch, 1))


def parent_library(path):
  """Another build of the library (the parent commit's) -> (call(name, *args) of its edet_preprocess_infer, a stand-in for
  preprocess.preprocess_infer that goes through it: the same Python, the parent's kernel)."""
  lib = ctypes.CDLL(os.path.abspath(path))
  fn = lib.edet_preprocess_infer
  fn.restype = ctypes.c_int
  fn.argtypes = _lib.SIGNATURES['edet_preprocess_infer']

  def call(name, *args):
    assert name == 'edet_preprocess_infer'
    rc = fn(*args)
    if rc:
      raise RuntimeError('the parent library refused edet_preprocess_infer (%d)' % rc)

  def wrapper(raw_images, image_size, mean_rgb, stddev_rgb, dtype=torch.float32):
    raw = raw_images.cuda().contiguous()
    oh, ow = (image_size, image_size) if isinstance(image_size, int) else image_size
    b, h, w, _ = raw.shape
    out = torch.empty((b, oh, ow, 3), dtype=dtype, device=raw.device)
    mean = (ctypes.c_float * 3)(*[float(v) for v in mean_rgb])
    std = (ctypes.c_float * 3)(*[float(v) for v in stddev_rgb])
    scale = ctypes.c_float(0.0)
    call('edet_preprocess_infer', raw.data_ptr(), 1 if raw.dtype == torch.float32 else 0, b, h, w, oh, ow, mean, std,
         out.data_ptr(), ctypes.byref(scale), _lib.EDET_BF16 if dtype == torch.bfloat16 else _lib.EDET_F32,
         torch.cuda.current_stream().cuda_stream)
    return out, torch.full((b,), scale.value, dtype=torch.float32, device=raw.device)
  return call, wrapper


def summary(times):
  return {'median_ms': round(float(np.median(times)), 4), 'min_ms': round(min(times), 4),
          'spread_ms': round(max(times) - min(times), 4)}


def bench_kernel(args, parent):
  b, h, w, o = args.batch, args.height, args.width, args.out
  tdt = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
  config = hparams_config.get_efficientdet_config(args.model)
  mean, std = config.mean_rgb, config.stddev_rgb
  raw = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (b, h, w, 3), dtype=np.uint8)).to('cuda:0')
  full, mix = full_sizes(args), mixed_sizes(args)
  # the entry points themselves on buffers made once: no allocation and no upload inside the timed window
  out_a, out_b = torch.empty((b, o, o, 3), dtype=tdt, device='cuda:0'), torch.empty((b, o, o, 3), dtype=tdt, device='cuda:0')
  c3 = ctypes.c_float * 3
  cmean, cstd = c3(*[float(v) for v in mean]), c3(*[float(v) for v in std])
  code = _lib.EDET_BF16 if tdt == torch.bfloat16 else _lib.EDET_F32
  st = torch.cuda.current_stream().cuda_stream
  scale = ctypes.c_float(0.0)
  per = {}
  for key, sizes in (('full', full), ('mix', mix)):
    _, scaled, _ = preprocess.infer_canvas_factors(sizes, b, h, w, o)
    per[key] = torch.from_numpy(np.concatenate([sizes, scaled], 0)).to('cuda:0')

  def dense(lib_call):
    lib_call('edet_preprocess_infer', raw.data_ptr(), 0, b, h, w, o, o, cmean, cstd, out_a.data_ptr(), ctypes.byref(scale), code,
             st)

  def canvas(key, mirrored):
    _lib.call('edet_preprocess_infer_canvas', raw.data_ptr(), 0, b, h, w, per[key].data_ptr(), per[key].data_ptr() + 8 * b, o, o,
              cmean, cstd, out_a.data_ptr(), out_b.data_ptr() if mirrored else None, code, st)
  variants = {
      'dense': lambda: dense(_lib.call),
      'canvas_full': lambda: canvas('full', False),
      'canvas_mix': lambda: canvas('mix', False),
      'canvas_full_mirrored': lambda: canvas('full', True),
      'canvas_mix_mirrored': lambda: canvas('mix', True),
      'dense_plus_flip': lambda: (dense(_lib.call), torch.flip(out_a, dims=[2])),      # what the mirrored output replaces
  }
  if parent is not None:
    variants['parent_dense'] = lambda: dense(parent)
    bits = torch.int16 if tdt == torch.bfloat16 else torch.int32
    dense(parent)
    theirs = out_a.clone()
    dense(_lib.call)
    same = torch.equal(theirs.view(bits), out_a.view(bits))
    del theirs
  order = sorted(variants)
  for name in order:      # every shape once before the timed window: code objects, the allocator's blocks
    for _ in range(3):
      variants[name]()
  torch.cuda.synchronize()
  times = {name: [] for name in order}
  for _ in range(args.reps):
    for name in order:
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(args.launches):
        variants[name]()
      e1.record()
      torch.cuda.synchronize()
      times[name].append(e0.elapsed_time(e1) / args.launches)
  esize = 2 if tdt == torch.bfloat16 else 4
  one_out = b * o * o * 3 * esize
  raw_bytes = {'full': b * h * w * 3, 'mix': 3 * int((mix[:, 0].astype(np.int64) * mix[:, 1]).sum())}
  moved = {'dense': raw_bytes['full'] + one_out, 'parent_dense': raw_bytes['full'] + one_out,
           'canvas_full': raw_bytes['full'] + one_out, 'canvas_mix': raw_bytes['mix'] + one_out,
           'canvas_full_mirrored': raw_bytes['full'] + 2 * one_out, 'canvas_mix_mirrored': raw_bytes['mix'] + 2 * one_out,
           'dense_plus_flip': raw_bytes['full'] + 3 * one_out}      # the flip reads the output and writes its copy
  out = {'phase': 'kernel', 'batch': b, 'canvas': [h, w], 'out': [o, o], 'dtype': args.dtype, 'launches': args.launches,
         'reps': args.reps}
  if parent is not None:
    out['parent_dense_bits_equal_dense'] = bool(same)
  for name in order:
    out[name] = summary(times[name])
    out[name]['bytes'] = moved[name]
    out[name]['GBps'] = round(moved[name] / (out[name]['median_ms'] * 1e-3) / 1e9, 1)
  print(json.dumps(out))


def bench_tta(args, parent):
  b, h, w = args.batch, args.height, args.width
  config = hparams_config.get_efficientdet_config(args.model)
  config.override('image_size=%d' % args.out)
  model = efficientdet_net.EfficientDetModel(config=config, dtype=args.dtype, seed=5)
  raw = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (b, h, w, 3), dtype=np.uint8)).to('cuda:0')
  full, mix = full_sizes(args), mixed_sizes(args)
  ours = preprocess.preprocess_infer

  def with_parent():
    preprocess.preprocess_infer = parent
    try:
      return model.detect_flip_tta(raw)
    finally:
      preprocess.preprocess_infer = ours
  variants = {'dense': lambda: model.detect_flip_tta(raw), 'pair_full': lambda: model.detect_flip_tta((raw, full)),
              'pair_mix': lambda: model.detect_flip_tta((raw, mix))}
  if parent is not None:
    variants['parent_dense'] = with_parent
  order = sorted(variants)
  first = {}
  for name in order:
    for _ in range(max(args.warmup, 2)):
      first[name] = variants[name]()
  torch.cuda.synchronize()
  same = {name: bool(torch.equal(first[name][0].view(torch.int32), first['dense'][0].view(torch.int32)))
          for name in order if name not in ('dense', 'pair_mix')}
  times = {name: [] for name in order}
  for _ in range(args.reps):
    for name in order:
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(args.steps):
        variants[name]()
      torch.cuda.synchronize()
      times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
  out = {'phase': 'tta', 'model': args.model, 'batch': b, 'canvas': [h, w], 'image_size': args.out, 'dtype': args.dtype,
         'steps': args.steps, 'reps': args.reps, 'detections_bits_equal_dense': same}
  for name in order:
    out[name] = summary(times[name])
  print(json.dumps(out))


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('phase', choices=['kernel', 'tta'])
  ap.add_argument('--model', default='efficientdet-d0')
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--height', type=int, default=512)
  ap.add_argument('--width', type=int, default=640)
  ap.add_argument('--out', type=int, default=640)
  ap.add_argument('--dtype', choices=['bf16', 'f32'], default='bf16')
  ap.add_argument('--parent-lib', default='')
  ap.add_argument('--launches', type=int, default=20)
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--steps', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=2)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('bench_infer.py needs an MI355X: nothing is measured without one')
  _lib.load()
  parent_fns = parent_library(a.parent_lib) if a.parent_lib else (None, None)
  {'kernel': bench_kernel, 'tta': bench_tta}[a.phase](a, parent_fns[0 if a.phase == 'kernel' else 1])
