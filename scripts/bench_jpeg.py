#!/usr/bin/env python3
"""The JPEG decoder on one MI355X and its host, for LABNOTES.md (NOT the bench.py line).  A batch of `--batch` copies of the
640x480 4:2:0 file of tests/golden/jpeg_cases.npz -- or of `--file`, any JPEG the decoder takes: the fixture is mostly flat
tiles (16 KB), so its Huffman stage is far shorter than a photograph's --, one JSON line:
  host_ms        the host stage alone (edet_jpeg_entropy_decode into pinned memory) at 1, 4 and 16 threads: wall clock,
                 median and spread of `--reps` batches;
  copy_ms        the three host-to-device copies of one batch, HIP events;
  idct_ms, color_ms   each kernel alone, HIP events around `--launches` launches;
  end_to_end     JpegDecoder(depth=2).decode in a loop at `--threads` threads, the device stage of one batch under the host
                 stage of the next: wall clock per batch with one synchronisation at the end -> images per second;
  pillow         where Pillow is importable: Image.open(...).convert('RGB') of the same bytes on a pool of as many worker
                 threads (its decoder releases the interpreter lock), the independent baseline -> images per second.
`--ratio` 2, 4 or 8 decodes every image at that tf.io.decode_jpeg ratio into a canvas of the reduced size, through the three
*_scaled entry points (csrc/jpeg_scaled.hip); `--max_ratio` alone (with --ratio 1) runs full-size images through the same
entry points.  With both at 1, the default, the full-size entry points are measured as before.  The host stage and the copy
move the file's coefficients whatever the ratio; only the two kernels shrink.
`--window` decodes a crop window of every image through edet_jpeg_entropy_decode_window, edet_jpeg_idct_scaled on the kept
grids and edet_jpeg_color_window (csrc/jpeg_window.hip): `--window` or `--window sampled` draws one window per image with
v2_preprocessing.sample_distorted_bounding_box from a fixed seed (at --ratio above 1: its covering output window),
`--window whole` takes the whole image through the same path.  The canvas stays the whole output's size.  window_area is the
mean share of the output's pixels the windows cover, kept_blocks the mean share of the file's blocks stored and copied.
`--entropy device` measures JpegDecoder(entropy='device') on the same batch, full size only: host_ms is then
edet_jpeg_scan_prepare (the marker walk and the byte-copy pass) at 1, 4 and 16 threads, copy_ms the copies of the scan arena,
its segment, table and descriptor arrays, entropy_ms edet_jpeg_entropy_device alone at `--subseq_bits`, with `rounds` read
back from the scan descriptors after the run; the other keys keep their meaning.  The host mode measured in the same run is
the yardstick.
No ratio between two timings is asserted: the numbers are the result."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from automl_amd import jpeg  # noqa: E402
from automl_amd._lib import call, ptr  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')


def stats(times):
  return {'median_ms': round(float(np.median(times)), 3), 'spread_ms': round(max(times) - min(times), 3),
          'min_ms': round(min(times), 3)}


def events(fn, launches, reps):
  times = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
      fn()
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) / launches)
  return stats(times)


def main_device(args, data, rgb, h, w, out):
  """--entropy device: the keys of main(), with edet_jpeg_scan_prepare as the host stage and the entropy kernel beside the two
  others."""
  b = args.batch
  datas = [data] * b
  dec = jpeg.JpegDecoder(b, h, w, threads=args.threads, depth=2, entropy='device', subseq_bits=args.subseq_bits,
                         scan_bytes=b * ((len(data) + 79) // 16 * 16))
  slot = dec._slots[0]
  out['entropy'], out['subseq_bits'] = 'device', args.subseq_bits
  used = None

  def host_stage(threads):
    return jpeg.scan_prepare(datas, h, w, 1, None, dec.blocks * 64, args.subseq_bits, slot.scan_host, slot.segments_host,
                             slot.unit_capacity, slot.tables_host, slot.scans_host, slot.images_host, slot.qtables_host,
                             slot.status, threads)
  out['host_ms'] = {}
  for threads in (1, 4, 16):
    times = []
    for _ in range(args.reps + 1):
      t0 = time.perf_counter()
      used = host_stage(threads)
      times.append((time.perf_counter() - t0) * 1e3)
    out['host_ms'][str(threads)] = dict(stats(times[1:]), images_per_s=round(b / (float(np.median(times[1:])) * 1e-3), 1))
  assert not slot.status.any()
  desc = jpeg.descriptors(slot.images_host, b)
  most = max(d.total_blocks for d in desc)
  nbytes, nseg = used[0], used[1] * jpeg.SEGMENT_BYTES
  out['scan_bytes'], out['segments'], out['units'] = used
  out['copied_bytes'] = nbytes + nseg + slot.tables_host.numel() + slot.scans_host.numel() + slot.images_host.numel() + \
      slot.qtables_host.numel() * 2
  out['blocks_per_image'] = most

  def copy():
    slot.scan[:nbytes].copy_(slot.scan_host[:nbytes], non_blocking=True)
    slot.segments[:nseg].copy_(slot.segments_host[:nseg], non_blocking=True)
    slot.tables.copy_(slot.tables_host, non_blocking=True)
    slot.scans.copy_(slot.scans_host, non_blocking=True)
    slot.images.copy_(slot.images_host, non_blocking=True)
    slot.qtables.copy_(slot.qtables_host, non_blocking=True)
  raw = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dec.device)
  st = torch.cuda.current_stream().cuda_stream
  copy()
  torch.cuda.synchronize()
  out['copy_ms'] = events(copy, 1, args.reps)
  out['copy_GBps'] = round(out['copied_bytes'] / (out['copy_ms']['median_ms'] * 1e-3) / 1e9, 1)
  out['entropy_ms'] = events(lambda: call('edet_jpeg_entropy_device', ptr(slot.scan), dec.scan_bytes, ptr(slot.segments),
                                          dec.segments, ptr(slot.tables), ptr(slot.scans), ptr(slot.images), b, args.subseq_bits,
                                          ptr(slot.units), slot.unit_capacity, ptr(slot.dc), ptr(slot.coef), dec.blocks * 64,
                                          ptr(slot.scan_status), st), args.launches, args.reps)
  rounds = [d.rounds for d in jpeg.scan_descriptors(slot.scans.cpu(), b)]
  assert not slot.scan_status.cpu().numpy().any()
  out['rounds'] = {'min': int(min(rounds)), 'max': int(max(rounds))}
  out['units_per_image'] = used[2] // b
  out['idct_ms'] = events(lambda: call('edet_jpeg_idct', ptr(slot.coef), ptr(slot.images), ptr(slot.qtables), b, most,
                                       ptr(slot.planes), dec.blocks * 64, st), args.launches, args.reps)
  out['color_ms'] = events(lambda: call('edet_jpeg_color', ptr(slot.planes), ptr(slot.images), b, h, w, dec.blocks * 64,
                                        ptr(raw), st), args.launches, args.reps)
  if rgb is not None:
    assert np.array_equal(raw[b - 1].cpu().numpy(), rgb), 'the decoded batch differs from the fixture'
  else:      # any other file: the host mode is the yardstick
    want = jpeg.JpegDecoder(1, h, w, depth=1).decode([data])[0]
    assert torch.equal(raw[b - 1], want[0]), 'the device entropy mode differs from the host mode'
  sizes = np.zeros((b, 2), np.int32)
  for _ in range(2):
    dec.decode(datas, out=raw, sizes_out=sizes)
  torch.cuda.synchronize()
  times = []
  for _ in range(args.reps):
    t0 = time.perf_counter()
    for _ in range(args.batches):
      dec.decode(datas, out=raw, sizes_out=sizes)
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3 / args.batches)
  assert not dec.scan_status().any()
  out['end_to_end'] = dict(stats(times), threads=args.threads, depth=2, batches_per_rep=args.batches,
                           images_per_s=round(b / (float(np.median(times)) * 1e-3), 1))
  print(json.dumps(out))


def main(args):
  if args.file:
    data = open(args.file, 'rb').read()
    info = jpeg.jpeg_info(data)
    rgb, h, w = None, info.height, info.width
  else:
    g = np.load(GOLDEN)
    data = g['big_480x640_420/bytes'].tobytes()
    rgb = g['big_480x640_420/rgb']
    h, w = rgb.shape[:2]
  b = args.batch
  datas = [data] * b
  ratio, max_ratio = args.ratio, max(args.ratio, args.max_ratio)
  scaled = max_ratio > 1 or bool(args.window)
  ratios = [ratio] * b if max_ratio > 1 else None
  out = {'batch': b, 'height': h, 'width': w, 'file': os.path.basename(args.file) if args.file else 'big_480x640_420',
         'file_bytes': len(data), 'reps': args.reps, 'ratio': ratio, 'max_ratio': max_ratio,
         'entry_points': 'scaled' if scaled else 'full size'}
  file_blocks = jpeg.worst_blocks(h, w)
  h, w = jpeg.scaled_size(h, w, ratio)      # the canvas: the output, exactly
  out['canvas'] = [h, w]
  if args.entropy == 'device':
    if scaled:
      sys.exit('--entropy device is measured at full size: no --ratio, --max_ratio or --window with it')
    return main_device(args, data, rgb, h, w, out)
  out['entropy'] = 'host'
  windows = None
  if args.window:
    from automl_amd import v2_preprocessing
    rng = np.random.default_rng(args.window_seed)
    full = [v2_preprocessing.sample_distorted_bounding_box(rng, out['height'], out['width']) if args.window == 'sampled'
            else (0, 0, out['height'], out['width']) for _ in range(b)]
    windows = np.array([jpeg.covering_window(win, ratio) for win in full], np.int32)
    out['entry_points'] = 'window'
    out['window'] = args.window
    out['window_area'] = round(float(np.mean(windows[:, 2] * windows[:, 3])) / (h * w), 4)
    dec = jpeg.JpegDecoder(b, h, w, threads=args.threads, depth=2, max_ratio=max_ratio, windowed=True,
                           coef_blocks=min(b * file_blocks, max_ratio ** 2 * b * jpeg.worst_window_blocks(h, w)))
  elif scaled:
    dec = jpeg.JpegDecoder(b, h, w, threads=args.threads, depth=2, max_ratio=max_ratio, coef_blocks=b * file_blocks)
  else:
    dec = jpeg.JpegDecoder(b, h, w, threads=args.threads, depth=2)
  slot = dec._slots[0]
  idct, color = ('edet_jpeg_idct_scaled', 'edet_jpeg_color_scaled') if scaled else ('edet_jpeg_idct', 'edet_jpeg_color')

  def host_stage(threads):
    if windows is not None:
      jpeg.entropy_decode_window(datas, h, w, max_ratio, ratios, windows, slot.coef_host, slot.images_host, slot.windows_host,
                                 slot.qtables_host, slot.status, threads)
    elif scaled:
      jpeg.entropy_decode_scaled(datas, h, w, max_ratio, ratios, slot.coef_host, slot.images_host, slot.qtables_host,
                                 slot.status, threads)
    else:
      jpeg.entropy_decode(datas, h, w, slot.coef_host, slot.images_host, slot.qtables_host, slot.status, threads)
  out['host_ms'] = {}
  for threads in (1, 4, 16):
    times = []
    for _ in range(args.reps + 1):
      t0 = time.perf_counter()
      host_stage(threads)
      times.append((time.perf_counter() - t0) * 1e3)
    out['host_ms'][str(threads)] = dict(stats(times[1:]), images_per_s=round(b / (float(np.median(times[1:])) * 1e-3), 1))
  desc = jpeg.descriptors(slot.images_host, b)
  assert not slot.status.any()
  used = max(d.first_block[0] + d.total_blocks for d in desc)
  most = max(d.total_blocks for d in desc)
  out['coefficient_bytes'] = used * 128
  out['blocks_per_image'] = most
  if windows is not None:
    out['kept_blocks'] = round(used / float(b * jpeg.window_grid(jpeg.jpeg_info(data), (0, 0, h, w), ratio)[1]), 4)

  def copy():
    slot.coef[:used * 64].copy_(slot.coef_host[:used * 64], non_blocking=True)
    slot.images.copy_(slot.images_host, non_blocking=True)
    slot.qtables.copy_(slot.qtables_host, non_blocking=True)
    if windows is not None:
      slot.windows.copy_(slot.windows_host, non_blocking=True)
  raw = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dec.device)
  st = torch.cuda.current_stream().cuda_stream
  copy()
  torch.cuda.synchronize()
  out['copy_ms'] = events(copy, 1, args.reps)
  out['copy_GBps'] = round(used * 128 / (out['copy_ms']['median_ms'] * 1e-3) / 1e9, 1)
  out['idct_ms'] = events(lambda: call(idct, ptr(slot.coef), ptr(slot.images), ptr(slot.qtables), b, most,
                                       ptr(slot.planes), dec.blocks * 64, st), args.launches, args.reps)
  if windows is not None:
    out['color_ms'] = events(lambda: call('edet_jpeg_color_window', ptr(slot.planes), ptr(slot.images), ptr(slot.windows), b, h,
                                          w, dec.blocks * 64, ptr(raw), st), args.launches, args.reps)
  else:
    out['color_ms'] = events(lambda: call(color, ptr(slot.planes), ptr(slot.images), b, h, w, dec.blocks * 64,
                                          ptr(raw), st), args.launches, args.reps)
  out['idct_ns_per_block'] = round(out['idct_ms']['median_ms'] * 1e6 / (b * most), 3)
  if windows is not None and rgb is not None and ratio == 1:
    y, x, wh, ww = windows[b - 1]
    want = np.zeros_like(rgb)
    want[:wh, :ww] = rgb[y:y + wh, x:x + ww]
    assert np.array_equal(raw[b - 1].cpu().numpy(), want), 'the decoded window differs from the fixture'
  assert windows is not None or rgb is None or ratio > 1 or np.array_equal(raw[b - 1].cpu().numpy(), rgb), \
      'the decoded batch differs from the fixture'
  sizes = np.zeros((b, 2), np.int32)
  for _ in range(2):
    dec.decode(datas, out=raw, sizes_out=sizes, ratios=ratios, windows=windows)
  torch.cuda.synchronize()
  times = []
  for _ in range(args.reps):
    t0 = time.perf_counter()
    for _ in range(args.batches):
      dec.decode(datas, out=raw, sizes_out=sizes, ratios=ratios, windows=windows)
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3 / args.batches)
  out['end_to_end'] = dict(stats(times), threads=args.threads, depth=2, batches_per_rep=args.batches,
                           images_per_s=round(b / (float(np.median(times)) * 1e-3), 1))
  try:
    from PIL import Image
  except ImportError:
    out['pillow'] = None
  else:
    def one(d):
      im = Image.open(io.BytesIO(d))
      if ratio > 1:
        im.draft('RGB', (im.size[0] // ratio, im.size[1] // ratio))      # libjpeg's scale_denom
      return np.asarray(im.convert('RGB'))
    with ThreadPoolExecutor(max_workers=args.threads) as pool:
      times = []
      for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        done = list(pool.map(one, datas))
        times.append((time.perf_counter() - t0) * 1e3)
    # (draft mode does not reach a ratio larger than the image's smaller side: then the sizes differ and nothing is compared)
    assert windows is not None or done[0].shape != tuple(raw[0].shape) or np.array_equal(done[0], raw[0].cpu().numpy()), 'Pillow and the decoder differ'
    out['pillow'] = dict(stats(times[1:]), threads=args.threads,
                         images_per_s=round(b / (float(np.median(times[1:])) * 1e-3), 1))
  print(json.dumps(out))


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--file', default='')
  ap.add_argument('--ratio', type=int, default=1, choices=[1, 2, 4, 8], help='decode every image at this ratio')
  ap.add_argument('--max_ratio', type=int, default=1, choices=[1, 2, 4, 8],
                  help="the decoder's max_ratio; above 1 the *_scaled entry points run, also for --ratio 1")
  ap.add_argument('--window', nargs='?', const='sampled', default='', choices=['sampled', 'whole'],
                  help='decode a crop window of every image: sampled (sample_distorted_bounding_box, the default) or whole')
  ap.add_argument('--window_seed', type=int, default=0)
  ap.add_argument('--entropy', default='host', choices=['host', 'device'], help="where the Huffman stage runs (JpegDecoder's entropy=)")
  ap.add_argument('--subseq_bits', type=int, default=4096, help='--entropy device: the bits of a unit')
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--threads', type=int, default=16)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--launches', type=int, default=10)
  ap.add_argument('--batches', type=int, default=6)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('bench_jpeg.py needs an MI355X: nothing is measured without one')
  main(a)
