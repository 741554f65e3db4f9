#!/usr/bin/env python3
"""Times the evaluation step's kernels against what they are cut from.  Prints one JSON line.

  loss kernels   edet_focal_loss + edet_box_loss against edet_focal_loss_eval + edet_box_loss_eval over the five head levels of
                 efficientdet-d0 at 640 x 640, batch --batch (bf16 logits, rows of 816 and 40 elements), and edet_l2_loss
                 against edet_opt_l2_norms + edet_opt_clip_factors on the model's own arena.
  test_step      EfficientDetNetTrain.test_step (eager, and replayed from its captured graph) against the forward half of a
                 training step, eng.forward(images, training=True), on the same engine.

Medians of --repeats timed runs between two events.  No time is required of it: these are measurements."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from automl_amd import _lib, hparams_config, netspec, train_lib      # noqa: E402
from automl_amd._lib import call, ptr      # noqa: E402


def timed(fn, repeats):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  out = []
  for _ in range(repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    out.append(a.elapsed_time(b))
  return float(np.median(out))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--size', type=int, default=640)
  ap.add_argument('--repeats', type=int, default=20)
  ap.add_argument('--skip-network', action='store_true')
  args = ap.parse_args()
  _lib.load()
  dev = 'cuda:0'
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  config.override('image_size=%d' % args.size)
  spec = netspec.NetSpec(config)
  na, nc = spec.num_anchors, config.num_classes
  rng = np.random.default_rng(0)
  st = torch.cuda.current_stream().cuda_stream
  levels = []
  sizes = spec.feat_sizes(args.size)
  for level in range(config.min_level, config.max_level + 1):
    pos = args.batch * sizes[level]['height'] * sizes[level]['width']
    logits = torch.randn((pos, (na * nc + 7) // 8 * 8), device=dev).to(torch.bfloat16)
    box = (torch.randn((pos, (4 * na + 7) // 8 * 8), device=dev) * 0.3).to(torch.bfloat16)
    ct = torch.from_numpy(np.where(rng.random((pos, na)) < 0.01, rng.integers(0, nc, (pos, na)), -1).astype(np.int32)).to(dev)
    bt = torch.zeros((pos, 4 * na), device=dev)
    bt[torch.rand((pos, 4 * na), device=dev) < 0.01] = 0.2
    levels.append((pos, logits, box, ct, bt, torch.empty_like(logits), torch.empty_like(box)))
  sums = torch.zeros(4, device=dev)
  dbc, dbb = torch.zeros(na * nc, device=dev), torch.zeros(4 * na, device=dev)
  wsp = torch.empty(16 * 1024 * 1024, dtype=torch.float32, device=dev)
  wsb = wsp.numel() * 4
  inv = torch.tensor([1.0 / 37.0], device=dev)

  def train_losses():
    for pos, logits, box, ct, bt, dl, db in levels:
      call('edet_focal_loss', ptr(logits), logits.shape[1], ptr(ct), pos, na, nc, 0.25, 1.5, 1.0, ptr(inv), ptr(dl), ptr(dbc),
           ptr(sums), ptr(wsp), wsb, _lib.EDET_BF16, st)
      call('edet_box_loss', ptr(box), box.shape[1], ptr(bt), pos, 4 * na, 0.1, 0.25, 50.0, ptr(inv), ptr(db), ptr(dbb), ptr(sums),
           ptr(wsp), wsb, _lib.EDET_BF16, st)

  def eval_losses():
    for pos, logits, box, ct, bt, dl, db in levels:
      call('edet_focal_loss_eval', ptr(logits), logits.shape[1], ptr(ct), pos, na, nc, 0.25, 1.5, 0.0, 1.0, ptr(inv), ptr(sums),
           ptr(wsp), wsb, _lib.EDET_BF16, st)
      call('edet_box_loss_eval', ptr(box), box.shape[1], ptr(bt), pos, 4 * na, 0.1, 0.25, ptr(inv), ptr(sums), ptr(wsp), wsb,
           _lib.EDET_BF16, st)

  out = {'batch': args.batch, 'size': args.size,
         'loss_train_ms': timed(train_losses, args.repeats), 'loss_eval_ms': timed(eval_losses, args.repeats)}
  out['logit_bytes'] = int(sum(l[1].numel() * 2 + l[2].numel() * 2 for l in levels))
  del levels
  if not args.skip_network:
    net = train_lib.EfficientDetNetTrain(config=config, dtype='bf16', use_graph=True, global_batch_size=64)
    images = torch.randn((args.batch, args.size, args.size, 3), device=dev).to(torch.bfloat16)
    labels = {'mean_num_positives': np.full((args.batch,), 5.0, np.float32)}
    for level in range(config.min_level, config.max_level + 1):
      h, w = sizes[level]['height'], sizes[level]['width']
      ct = np.full((args.batch, h, w, na), -1, np.int32)
      ct[:, ::2, ::2, 0] = 3
      bt = np.zeros((args.batch, h, w, 4 * na), np.float32)
      bt[:, ::2, ::2, :4] = 0.1
      labels['cls_targets_%d' % level], labels['box_targets_%d' % level] = ct, bt
    eng = net._ensure_engine(args.batch, args.size, args.size)
    dl = net._labels_to_device(labels, eng)
    out['forward_training_ms'] = timed(lambda: eng.forward(images, training=True), args.repeats)
    net.use_graph = False
    out['test_step_eager_ms'] = timed(lambda: net.test_step((images, dl), sync_loss=False), args.repeats)
    net.use_graph = True
    out['test_step_graph_ms'] = timed(lambda: net.test_step((images, dl), sync_loss=False), args.repeats)
    a = eng.arena
    sq, fac = torch.zeros_like(a.seg_sqnorm), torch.zeros_like(a.seg_factor)
    l2, gn = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    seg_l2 = torch.zeros(a.nseg * _lib.OPT_SPLIT, device=dev)

    def train_l2():
      call('edet_opt_l2_norms', ptr(a.grads_flat), ptr(a.params_flat), ptr(a.seg_offsets), ptr(a.seg_flags), a.nseg, 4e-5, ptr(sq), st)
      call('edet_opt_clip_factors', ptr(sq), a.nseg, 10.0, ptr(fac), ptr(gn), ptr(l2), st)
    out['l2_train_ms'] = timed(train_l2, args.repeats)
    out['l2_eval_ms'] = timed(lambda: call('edet_l2_loss', ptr(a.params_flat), ptr(a.seg_offsets), ptr(a.seg_flags), a.nseg, 4e-5,
                                           ptr(seg_l2), ptr(l2), st), args.repeats)
    out['test_step'] = net.test_step((images, dl))
  print(json.dumps(out))


if __name__ == '__main__':
  main()
