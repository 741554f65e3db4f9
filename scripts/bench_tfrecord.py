#!/usr/bin/env python3
"""The TFRecord input path on one MI355X and its host, for LABNOTES.md "TFRecord input" (NOT the bench.py line, and nothing here
is read by bench.py).  Writes `--shards` synthetic shards of `--images` records into a temporary folder -- 640 x 480 4:2:0 JPEGs
(`--distinct` different smooth-noise images encoded with Pillow where it is importable, else the 640 x 480 file of
tests/golden/jpeg_cases.npz, which is mostly flat tiles), eight boxes each -- and prints one JSON line:
  host           records/s of index + CRC-32C + Example parse + decoder rules alone (no device), at 1 and at 16 parse threads,
                 with the two halves timed apart: `index_crc` (one thread, always) and `parse`; files are in the page cache;
  decode         images/s of reader + JpegDecoder (A) against JpegDecoder fed the same bytes from memory (B);
  step           D0 `--batch` train_step_raw images/s fed by the reader (A) against the same step fed from memory (B).
A and B alternate, `--rounds` rounds each of `--steps` batches ending in one synchronisation; each figure is the median of
its rounds with the spread (max - min) beside it.  `--memory-only --root DIR` runs the B sides alone on the package under DIR
(a checkout of the parent commit, which has no reader).  No ratio is asserted: the numbers are the result."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BOXES = 100


def make_jpegs(distinct, seed):
  try:
    from PIL import Image
  except ImportError:
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz'))
    return [g['big_480x640_420/bytes'].tobytes()], 'fixture big_480x640_420'
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(distinct):
    coarse = rng.normal(128, 50, (60, 80, 3))
    img = np.kron(coarse, np.ones((8, 8, 1))) + rng.normal(0, 12, (480, 640, 3))      # blocks with grain: a photograph's order of size
    buf = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), 'RGB').save(buf, 'JPEG', quality=90, subsampling=2)
    out.append(buf.getvalue())
  return out, 'Pillow quality 90, %d distinct' % distinct


def make_annotations(n, seed):
  rng = np.random.default_rng(seed + 1)
  lo = (rng.random((n, 8, 2)) * 0.5).astype(np.float32)
  hi = lo + (0.2 + rng.random((n, 8, 2)) * 0.3).astype(np.float32)
  boxes = np.concatenate([lo, hi], -1)      # ymin, xmin, ymax, xmax
  classes = rng.integers(1, 91, (n, 8))
  return boxes, classes


def stats(rates):
  return {'median': round(float(np.median(rates)), 1), 'spread': round(float(max(rates) - min(rates)), 1), 'rounds': len(rates)}


def main(args):
  sys.path.insert(0, os.path.abspath(args.root))
  import torch
  from automl_amd import hparams_config, jpeg, train_lib
  if not torch.cuda.is_available() and not args.host_only:
    sys.exit('bench_tfrecord.py needs an MI355X for its decode and step figures (--host-only measures the host half alone)')
  jpegs, source = make_jpegs(args.distinct, args.seed)
  n, b = args.images, args.batch
  boxes, classes = make_annotations(n, args.seed)
  out = {'images': n, 'shards': args.shards, 'batch': b, 'jpeg': source, 'jpeg_bytes_mean': int(np.mean([len(j) for j in jpegs])),
         'rounds': args.rounds, 'steps_per_round': args.steps, 'root': os.path.relpath(os.path.abspath(args.root), ROOT)}

  def memory_batches():
    """Batches from memory for ever: the bytes and the padded arrays of `b` consecutive records."""
    k = 0
    bx = np.full((b, MAX_BOXES, 4), -1, np.float32)
    cl = np.full((b, MAX_BOXES), -1, np.float32)
    counts = np.full(b, 8, np.int32)
    while True:
      idx = [(k + i) % n for i in range(b)]
      k = (k + b) % n
      bx[:, :8], cl[:, :8] = boxes[idx], classes[idx]
      yield [jpegs[i % len(jpegs)] for i in idx], bx.copy(), cl.copy(), counts

  with tempfile.TemporaryDirectory() as tmp:
    reader_of = None
    if not args.memory_only:
      from automl_amd import dataloader, tf_example_decoder, tfrecord
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
      pattern = os.path.join(tmp, 'train-*.tfrecord')
      files = sorted(os.path.join(tmp, f) for f in os.listdir(tmp))
      out['file_bytes'] = sum(os.path.getsize(f) for f in files)
      # ---- the host half alone
      decoder = tf_example_decoder.TfExampleDecoder()
      out['host'] = {}
      for threads in (1, 16):
        rates, index_ms, parse_ms = [], [], []
        for _ in range(args.rounds + 1):
          t_index = t_parse = 0.0
          for path in files:
            t0 = time.perf_counter()
            f = tfrecord.TFRecordFile(path, verify=True)
            count = len(f)
            t1 = time.perf_counter()
            for at in range(0, count, b):
              decoder.decode([f[i] for i in range(at, min(count, at + b))], threads)
            t_parse += time.perf_counter() - t1
            t_index += t1 - t0
            f.close()
          rates.append(n / (t_index + t_parse))
          index_ms.append(t_index * 1e3)
          parse_ms.append(t_parse * 1e3)
        out['host'][str(threads)] = {'records_per_s': stats(rates[1:]), 'index_crc_ms': round(float(np.median(index_ms[1:])), 2),
                                     'parse_ms': round(float(np.median(parse_ms[1:])), 2),
                                     'crc_GBps': round(out['file_bytes'] / (float(np.median(index_ms[1:])) * 1e-3) / 1e9, 2)}
      config_params = hparams_config.get_efficientdet_config('efficientdet-d0').as_dict()
      config_params['tf_random_seed'] = args.seed

      def reader_of():
        return dataloader.InputReader(pattern, is_training=True).reader(config_params, batch_size=b, canvas=(480, 640), depth=2,
                                                                         threads=args.threads)
    if args.host_only:
      print(json.dumps(out))
      return
    # ---- reader + decoder against the decoder fed from memory
    dec = jpeg.JpegDecoder(b, 480, 640, threads=args.threads, depth=2)
    mem = memory_batches()
    reader = reader_of() if reader_of else None

    def decode_a():
      next(reader)

    def decode_b():
      dec.decode(next(mem)[0])

    def rounds(sides, steps):
      """sides: {'A': fn, 'B': fn} -> {name: images/s per round}, alternating, one warm-up round each that is not kept."""
      rates = {k: [] for k in sides}
      for r in range(args.rounds + 1):
        for name, fn in sides.items():
          torch.cuda.synchronize()
          t0 = time.perf_counter()
          for _ in range(steps):
            fn()
          torch.cuda.synchronize()
          if r:
            rates[name].append(steps * b / (time.perf_counter() - t0))
      return {k: stats(v) for k, v in rates.items()}
    sides = {'B_memory': decode_b} if reader is None else {'A_reader': decode_a, 'B_memory': decode_b}
    out['decode_images_per_s'] = rounds(sides, args.steps)
    # ---- the D0 step
    if not args.no_step:
      config = hparams_config.get_efficientdet_config('efficientdet-d0')
      config.override('image_size=%d' % args.image_size)
      net = train_lib.EfficientDetNetTrain(config=config, dtype='bf16', seed=0, global_batch_size=b, steps_per_epoch=1000, use_graph=True)

      def step_a():
        net.train_step_raw(next(reader), sync_loss=False)

      def step_b():
        datas, bx, cl, counts = next(mem)
        net.train_step_raw((dec.decode(datas), bx, cl, counts), sync_loss=False)
      for _ in range(3):      # eager, capture, replay
        step_b()
      sides = {'B_memory': step_b} if reader is None else {'A_reader': step_a, 'B_memory': step_b}
      out['step_images_per_s'] = dict(rounds(sides, args.steps), image_size=args.image_size, dtype='bf16')
    if reader is not None:
      reader.close()
  print(json.dumps(out))


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
  ap.add_argument('--root', default=ROOT, help='where the automl_amd package to measure lies')
  ap.add_argument('--memory-only', dest='memory_only', action='store_true')
  ap.add_argument('--host-only', dest='host_only', action='store_true')
  ap.add_argument('--no-step', dest='no_step', action='store_true')
  main(ap.parse_args())
