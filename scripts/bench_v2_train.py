#!/usr/bin/env python3
"""EfficientNetV2 classifier training on one MI355X, for LABNOTES.md (NOT the bench.py line).  One phase per process
(scripts/bench_v2_train.sh chains them under time limits), one JSON line each:
  opt    edet_opt_sgd_ema, edet_opt_rmsprop_ema and edet_opt_adam_ema on the model's arena (the last two move the same
         bytes): HIP events around `--launches` launches each, alternating, `--reps` repetitions -> medians, spreads
         (max - min), implied GB/s;
  step   ms per TrainableModel.train_step (RMSprop, default dropout and stochastic depth, hipGraph replay); with
         `--mix ALPHA` mixup and cutmix are on at that alpha (half the batch each) and the static image buffer is refilled
         from the caller's batch every step, as a mixing step needs; with `--randaug` RandAugment is on at the model's own
         magnitude (uint8 images, refilled every step); with `--crop CANVAS` the step takes decoded uint8 images on a
         CANVAS x CANVAS canvas and crops, resizes and flips them to `--size` on the device first (image_size = --size);
  mix    the mix pass alone (edet_mix_images + edet_mix_labels on the step's buffers): HIP events around `--launches`
         passes, `--reps` repetitions -> median, spread, bytes moved and implied GB/s;
  randaug the RandAugment pass alone (V2Engine.randaug_batch: the layers' edet_randaug_stats + edet_randaug_apply, the last
         one storing the normalised bf16 input) with the drawn mix of operations, then the whole batch one operation for each
         of the 16: HIP events around `--launches` passes, `--reps` repetitions -> median, spread, bytes moved, implied GB/s;
  crop   the crop / resize / flip pass alone (V2Engine.crop_batch: edet_crop_resize from a `--crop CANVAS` canvas to `--size`,
         with one step's drawn rows), into uint8 (what RandAugment reads) and into the normalised bf16 input: HIP events
         around `--launches` passes, `--reps` repetitions -> median, spread, bytes read (sum of the crop areas x 3) and
         written, implied GB/s and its share of the 8 TB/s HBM peak;
  fwdbwd ms per forward(training) + backward of EffNetV2Model with dropout_rate=0, launched eagerly: what the step had
         before the loss, the dropout and the update existed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from automl_amd import _lib, autoaugment, effnetv2_configs, effnetv2_model, effnetv2_train, engine as engine_lib  # noqa: E402
from automl_amd import v2_preprocessing  # noqa: E402
from automl_amd._lib import call, ptr  # noqa: E402


def bench_opt(args):
  spec = effnetv2_model.V2Spec(effnetv2_configs.model_config(args.model))
  a = engine_lib.ParamArena(spec, 'cuda:0', effnetv2_model.init_params(spec, 0))
  n = a.n_train_elems
  a.grads_flat.copy_(torch.randn(n, device='cuda:0') * 1e-2)
  slot2 = a.second_moment()
  hyper = torch.tensor([1e-6, 0.9999], dtype=torch.float32, device='cuda:0')
  st = torch.cuda.current_stream().cuda_stream
  common = (ptr(a.ema), ptr(a.seg_offsets), ptr(a.seg_factor), ptr(a.seg_flags), a.nseg, ptr(hyper))

  def sgd():
    call('edet_opt_sgd_ema', ptr(a.params_flat), ptr(a.grads_flat), ptr(a.velocity), *common, 0.9, st)

  def rms():
    call('edet_opt_rmsprop_ema', ptr(a.params_flat), ptr(a.grads_flat), ptr(slot2), ptr(a.velocity), *common, 0.9, 0.9, 1e-3, st)

  def adam():
    call('edet_opt_adam_ema', ptr(a.params_flat), ptr(a.grads_flat), ptr(a.velocity), ptr(slot2), *common, 0.9, 0.999, 1e-7, st)
  rules = (('sgd', sgd), ('rmsprop', rms), ('adam', adam))
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
  out = {'phase': 'opt', 'model': args.model, 'arena_elems': n, 'segments': a.nseg, 'launches': args.launches,
         'reps': args.reps}
  for name, t in times.items():
    med = float(np.median(t))
    # reads g, w, the slots, ema; writes w, the slots, ema: 9 arrays with two slots, 7 with SGD's one
    nbytes = (7 if name == 'sgd' else 9) * 4 * n
    out[name] = {'median_ms': round(med, 5), 'spread_ms': round(max(t) - min(t), 5), 'min_ms': round(min(t), 5),
                 'bytes_per_launch': nbytes, 'GBps': round(nbytes / (med * 1e-3) / 1e9, 1)}
  allow = max(out['rmsprop']['spread_ms'], out['adam']['spread_ms'])
  out['rmsprop_within_adam_plus_spread'] = out['rmsprop']['median_ms'] <= out['adam']['median_ms'] + allow
  print(json.dumps(out))


def _data(args):
  rng = np.random.default_rng(2)
  images = torch.from_numpy(rng.standard_normal((args.batch, args.size, args.size, 3)).astype(np.float32))
  return images.to('cuda:0', torch.bfloat16).contiguous(), torch.from_numpy(rng.integers(0, 1000, args.batch)).to('cuda:0', torch.int32)


def _data_u8(args):
  rng = np.random.default_rng(2)
  images = torch.from_numpy(rng.integers(0, 256, (args.batch, args.size, args.size, 3)).astype(np.uint8))
  return images.to('cuda:0').contiguous(), torch.from_numpy(rng.integers(0, 1000, args.batch)).to('cuda:0', torch.int32)


def _data_raw(args):
  """Decoded images that fill a --crop x --crop canvas."""
  rng = np.random.default_rng(2)
  images = torch.from_numpy(rng.integers(0, 256, (args.batch, args.crop, args.crop, 3), dtype=np.uint8))
  return images.to('cuda:0').contiguous(), torch.from_numpy(rng.integers(0, 1000, args.batch)).to('cuda:0', torch.int32)


HBM_PEAK = 8e12      # bytes / s


def bench_step(args):
  extra = {}
  if args.crop:
    extra['image_size'] = args.size
  if args.randaug:
    name, layers, ram = effnetv2_train.randaug_params(args.model)
    extra.update(augname=name, ra_num_layers=layers, ra_magnitude=ram)
  net = effnetv2_train.TrainableModel(args.model, dtype='bf16', learning_rate=1e-4, weight_decay=1e-5, label_smoothing=0.1,
                                      use_graph=True, mixup_alpha=args.mix, cutmix_alpha=args.mix, **extra)
  images, labels = _data_raw(args) if args.crop else _data_u8(args) if args.randaug else _data(args)
  first = net.train_step((images, labels))
  for _ in range(max(args.warmup, 2)):
    net.train_step((images, labels), sync_loss=False)
  if not args.mix and not args.randaug and not args.crop:      # (a mixing step mixes the static buffer in place: it is refilled from `images` every step)
    images, labels = net.input_buffers()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(args.steps):
    net.train_step((images, labels), sync_loss=False)
  torch.cuda.synchronize()
  dt = (time.perf_counter() - t0) / args.steps
  last = net.train_step((images, labels))
  print(json.dumps({'phase': 'step', 'workload': '%s %dx%d batch %d bf16 train_step (rmsprop, dropout %g, stochastic depth), '
                    'hipGraph replay%s' % (args.model, args.size, args.size, args.batch, net.cfg_model.dropout_rate,
                                          (', mixup + cutmix alpha %g' % args.mix if args.mix else '') +
                                          (', RandAugment %d layers M=%g' % (extra['ra_num_layers'], extra['ra_magnitude'])
                                           if args.randaug else '') +
                                          (', crop / resize / flip from a %dx%d uint8 canvas' % (args.crop, args.crop) if args.crop else '')),
                    'ms_per_step': round(dt * 1e3, 3), 'images_per_sec': round(args.batch / dt, 1),
                    'first_loss': first['loss'], 'last_loss': last['loss'], 'steps': args.steps}))


def bench_mix(args):
  alpha = args.mix or 0.4
  net = effnetv2_train.TrainableModel(args.model, dtype='bf16', use_graph=False, mixup_alpha=alpha, cutmix_alpha=alpha)
  images, labels = _data(args)
  eng = net._ensure_engine(args.batch, args.size, args.size)
  n_mixup = effnetv2_train.mix_split(args.batch, alpha, alpha)
  weights, boxes = effnetv2_train.draw_mix(net._mix_rng, args.batch, args.size, args.size, alpha, alpha)
  eng.set_mix_draws(weights, boxes, n_mixup)
  for _ in range(3):
    eng.mix_batch(images, labels)
  torch.cuda.synchronize()
  times = []
  for _ in range(args.reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.launches):
      eng.mix_batch(images, labels)
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) / args.launches)
  # mixup rows: read and written once; cutmix: the image rows of each pair's two boxes, read and written in both images
  row = args.size * 3 * 2
  moved = 2 * n_mixup * args.size * row
  m = args.batch - n_mixup
  for k in range(m // 2):
    i, p = n_mixup + k, args.batch - 1 - k
    spans = [(b[0], b[2]) for b in (boxes[i], boxes[p]) if b[2] > b[0] and b[3] > b[1]]
    if spans:
      moved += 2 * 2 * (max(s[1] for s in spans) - min(s[0] for s in spans)) * row
  moved += args.batch * eng.soft_labels.shape[1] * 4
  med = float(np.median(times))
  print(json.dumps({'phase': 'mix', 'workload': '%s %dx%d batch %d bf16 mix pass (mixup rows %d, cutmix rows %d, alpha %g)' % (
      args.model, args.size, args.size, args.batch, n_mixup, m, alpha), 'median_ms': round(med, 5),
      'spread_ms': round(max(times) - min(times), 5), 'min_ms': round(min(times), 5), 'bytes_per_pass': int(moved),
      'GBps': round(moved / (med * 1e-3) / 1e9, 1), 'launches': args.launches, 'reps': args.reps}))


def bench_randaug(args):
  name, layers, ram = effnetv2_train.randaug_params(args.model)
  net = effnetv2_train.TrainableModel(args.model, dtype='bf16', use_graph=False, augname=name, ra_num_layers=layers, ra_magnitude=ram)
  images, _ = _data_u8(args)
  eng = net._ensure_engine(args.batch, args.size, args.size)
  n = images.numel()
  # per layer: the apply launch reads and writes the batch (uint8; the last layer writes bf16), the statistics launch reads
  # the images whose operation is AutoContrast or Equalize once more
  def moved(ops):
    stats = int(np.isin(ops, (0, 1)).sum()) * (n // args.batch)
    return stats + n * (2 * (layers - 1) + 1 + 2)

  def measure(draws):
    ops, iargs, fargs = autoaugment.randaug_args(draws, ram, args.size, args.size)
    eng.set_randaug_draws(ops, iargs, fargs)
    for _ in range(3):
      eng.randaug_batch(images)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(args.launches):
        eng.randaug_batch(images)
      e1.record()
      torch.cuda.synchronize()
      times.append(e0.elapsed_time(e1) / args.launches)
    med, b = float(np.median(times)), moved(ops)
    return {'median_ms': round(med, 5), 'spread_ms': round(max(times) - min(times), 5), 'min_ms': round(min(times), 5),
            'bytes_per_pass': int(b), 'GBps': round(b / (med * 1e-3) / 1e9, 1)}
  out = {'phase': 'randaug', 'workload': '%s %dx%d batch %d, %d RandAugment layers at M=%g + normalisation to bf16' % (
      args.model, args.size, args.size, args.batch, layers, ram), 'launches': args.launches, 'reps': args.reps}
  out['drawn'] = measure(autoaugment.randaug_draws(net._ra_rng, args.batch, layers))
  shape = (layers, args.batch)
  rng = np.random.default_rng(3)
  for k, op_name in enumerate(autoaugment.AVAILABLE_OPS):
    sign = np.where(rng.random(shape) >= 0.5, 1.0, -1.0).astype(np.float32)
    out[op_name] = measure((np.full(shape, k, np.int32), sign, rng.random(shape), rng.random(shape)))
  print(json.dumps(out))


def bench_crop(args):
  if not args.crop:
    raise SystemExit('the crop phase needs --crop CANVAS')
  net = effnetv2_train.TrainableModel(args.model, dtype='bf16', use_graph=False, image_size=args.size)
  images, _ = _data_raw(args)
  eng = net._ensure_engine(args.batch, args.size, args.size)
  rows = v2_preprocessing.train_rows(net._crop_rng, [[args.crop, args.crop]] * args.batch)
  eng.set_crop_rows(rows)
  read = int((rows[:, 4].astype(np.int64) * rows[:, 5]).sum()) * 3
  out = {'phase': 'crop', 'workload': '%s batch %d, crop / resize / flip from a %dx%d uint8 canvas to %dx%d' % (
      args.model, args.batch, args.crop, args.crop, args.size, args.size), 'launches': args.launches, 'reps': args.reps,
      'bytes_read': read, 'mean_crop_area_fraction': round(read / 3 / (args.batch * args.crop * args.crop), 4)}
  for key, to_u8, esize in (('to_uint8', True, 1), ('to_bf16', False, 2)):
    for _ in range(3):
      eng.crop_batch(images, to_u8)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(args.launches):
        eng.crop_batch(images, to_u8)
      e1.record()
      torch.cuda.synchronize()
      times.append(e0.elapsed_time(e1) / args.launches)
    med, written = float(np.median(times)), args.batch * args.size * args.size * 3 * esize
    out[key] = {'median_ms': round(med, 5), 'spread_ms': round(max(times) - min(times), 5), 'min_ms': round(min(times), 5),
                'bytes_written': written, 'GBps': round((read + written) / (med * 1e-3) / 1e9, 1),
                'share_of_hbm_peak': round((read + written) / (med * 1e-3) / HBM_PEAK, 4)}
  print(json.dumps(out))


def bench_fwdbwd(args):
  net = effnetv2_model.EffNetV2Model(args.model, 'dropout_rate=0', dtype='bf16')
  images, _ = _data(args)
  eng = net._ensure_engine(args.batch, args.size, args.size)
  dlog = torch.randn(args.batch, net.spec.num_classes, device='cuda:0') * 1e-3

  def one():
    eng.forward(images, training=True)
    eng.backward(dlog)
  for _ in range(max(args.warmup, 2)):
    one()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(args.steps):
    one()
  torch.cuda.synchronize()
  dt = (time.perf_counter() - t0) / args.steps
  print(json.dumps({'phase': 'fwdbwd', 'workload': '%s %dx%d batch %d bf16 forward(training) + backward, dropout_rate=0, eager '
                    'launches' % (args.model, args.size, args.size, args.batch), 'ms_per_pass': round(dt * 1e3, 3),
                    'steps': args.steps}))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('phase', choices=['opt', 'step', 'mix', 'randaug', 'crop', 'fwdbwd'])
  ap.add_argument('--model', default='efficientnetv2-s')
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--size', type=int, default=224)
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--launches', type=int, default=20)
  ap.add_argument('--reps', type=int, default=11)
  ap.add_argument('--mix', type=float, default=0.0, help='mixup_alpha = cutmix_alpha of the step / mix phases (0 = off)')
  ap.add_argument('--randaug', action='store_true', help='step phase: RandAugment on, at the named model\'s layers and magnitude')
  ap.add_argument('--crop', type=int, default=0, metavar='CANVAS',
                  help='step / crop phases: decoded uint8 images on a CANVAS x CANVAS canvas, cropped and resized to --size on the device')
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_v2_train.py needs an MI355X: there is no CPU path and no CPU timing')
  _lib.load()
  {'opt': bench_opt, 'step': bench_step, 'mix': bench_mix, 'randaug': bench_randaug, 'crop': bench_crop, 'fwdbwd': bench_fwdbwd}[args.phase](args)


if __name__ == '__main__':
  main()
