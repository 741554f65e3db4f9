"""The device entropy decoder on the device (automl_amd/jpeg.py: JpegDecoder(entropy='device') on csrc/jpeg_entropy.hip).
edet_jpeg_entropy_device alone writes, for all 39 decodable fixtures in one batch and at three subsequence sizes, the very
coefficient arena edet_jpeg_entropy_decode writes -- element for element, padding blocks included, canaries behind every
buffer intact; JpegDecoder(entropy='device').decode equals JpegDecoder().decode byte for byte (full size, forced ratios, slot
reuse, a batch of one); a stream truncated inside its scan gives a zero canvas, MALFORMED in scan_status, ValueError or the
fallback under check_scan=True; header-level refusals raise before anything is enqueued; decode_jpeg and InputReader take the
switch.  array_equal throughout: there is no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

from automl_amd import dataloader, hparams_config, jpeg, tfrecord
from automl_amd._lib import call, ptr
from tests import gpu_util as gu
from tests import jpeg_entropy_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
MIXED = ['s17x33_420_q75', 'grey_19x13_q90', 's31x22_422_q75', 's37x53_444_q100', 's1x1_420_q75', 'restart_24x280_420',
         's8x9_422_q75', 'optimize_31x22_420', 's37x53_420_q100', 'grey_16x16_q75', 's1x1_444_q75', 'const_20x20_420']
CANVAS = (40, 288)
CANARY = 1024


@pytest.fixture(scope='module')
def cases():
  g = np.load(GOLDEN)
  ok = {str(n): g[str(n) + '/bytes'].tobytes() for n in g['names']}
  refused = {str(n): (g[str(n) + '/bytes'].tobytes(), int(g[str(n) + '/status'])) for n in g['refused']}
  return ok, refused


@pytest.fixture(scope='module')
def host_arena(cases):
  """All 39 decodable fixtures as one batch through the host stage, computed once: names, streams, the coefficient arena
  (0x5A5A where nothing is written), its descriptors and the blocks in use."""
  names = sorted(cases[0])
  datas = [cases[0][n] for n in names]
  n = len(datas)
  assert n == 39
  probe = np.zeros(n * jpeg.worst_blocks(480, 640) * 64, np.int16)
  images = np.zeros(n * jpeg.IMAGE_BYTES, np.uint8)
  qt = np.zeros((n, 4, 64), np.uint16)
  status = np.zeros(n, np.int32)
  jpeg.entropy_decode(datas, 480, 640, probe, images, qt, status)
  assert not status.any()
  desc = jpeg.descriptors(images, n)
  used = max(d.first_block[0] + d.total_blocks for d in desc)
  coef = np.full(used * 64, 0x5A5A, np.int16)      # an arena of exactly the blocks in use: the next block would be TOO_LARGE
  jpeg.entropy_decode(datas, 480, 640, coef, images, qt, status)
  assert not status.any() and np.array_equal(coef, probe[:used * 64])
  return dict(names=names, datas=datas, coef=coef, images=images.copy(), used=used)


def _canaried(count, dtype, fill):
  return torch.full((count + CANARY,), fill, dtype=dtype, device=gu.DEV)


@pytest.mark.gpu
@pytest.mark.parametrize('bits', [64, 128, 1024])
def test_entropy_device_equals_the_host_stage(host_arena, bits):
  h = host_arena
  n, used = len(h['datas']), h['used']
  scan = np.zeros(1 << 20, np.uint8)
  segments = np.zeros(4096 * jpeg.SEGMENT_BYTES, np.uint8)
  tables = np.zeros(n * jpeg.TABLES * jpeg.TABLE_BYTES, np.uint8)
  scans = np.zeros(n * jpeg.SCAN_BYTES, np.uint8)
  images = np.zeros(n * jpeg.IMAGE_BYTES, np.uint8)
  qt = np.zeros((n, 4, 64), np.uint16)
  status = np.zeros(n, np.int32)
  nbytes, nseg, nunits = jpeg.scan_prepare(h['datas'], 480, 640, 1, None, used * 64, bits, scan, segments, 1 << 22, tables,
                                           scans, images, qt, status)
  assert not status.any() and np.array_equal(images, h['images'])
  sd = jpeg.scan_descriptors(scans, n)
  at = h['names'].index('s37x53_444_q100')
  if bits == 64:
    assert sd[at].units > 256      # more units than the workgroup has threads
  # every buffer the kernel writes is exactly as large as the host says it must be, with a canary behind it
  coef = _canaried(used * 64, torch.int16, 0x5A5A)
  units = _canaried(nunits * jpeg.UNIT_WORDS, torch.int32, 0x5A5A5A5A)
  dc = _canaried(used, torch.int16, 0x5A5A)
  status_dev = _canaried(n, torch.int32, 0x5A5A5A5A)
  scans_dev = torch.cat([torch.from_numpy(scans), torch.full((CANARY,), 0x5A, dtype=torch.uint8)]).to(gu.DEV)
  images_dev = torch.cat([torch.from_numpy(images), torch.full((CANARY,), 0x5A, dtype=torch.uint8)]).to(gu.DEV)
  scan_dev = torch.from_numpy(scan[:nbytes]).to(gu.DEV)
  seg_dev = torch.from_numpy(segments[:nseg * jpeg.SEGMENT_BYTES]).to(gu.DEV)
  tables_dev = torch.from_numpy(tables).to(gu.DEV)
  call('edet_jpeg_entropy_device', ptr(scan_dev), nbytes, ptr(seg_dev), nseg, ptr(tables_dev), ptr(scans_dev), ptr(images_dev), n,
       bits, ptr(units), nunits, ptr(dc), ptr(coef), used * 64, ptr(status_dev), gu.stream())
  torch.cuda.synchronize()
  got = coef.cpu().numpy()
  assert np.array_equal(got[:used * 64], h['coef'])      # element for element, padding blocks included
  assert (got[used * 64:] == 0x5A5A).all()
  assert (units.cpu().numpy()[nunits * jpeg.UNIT_WORDS:] == 0x5A5A5A5A).all() and (dc.cpu().numpy()[used:] == 0x5A5A).all()
  st = status_dev.cpu().numpy()
  assert not st[:n].any() and (st[n:] == 0x5A5A5A5A).all()
  assert np.array_equal(images_dev.cpu().numpy()[:images.size], images) and (images_dev.cpu().numpy()[images.size:] == 0x5A).all()
  back = scans_dev.cpu().numpy()
  assert (back[scans.size:] == 0x5A).all()
  rounds = [d.rounds for d in jpeg.scan_descriptors(back[:scans.size], n)]
  assert all(1 <= r <= max(d.units, 1) for r, d in zip(rounds, sd)), rounds
  # the rounds are the restatement's (one small and noisy stream: hundreds of them at 64 bits)
  want = er.decode(er.prepare(h['datas'][at], subseq_bits=bits), bits)[2]
  assert rounds[at] == want and (bits != 64 or want > 100), (rounds[at], want)


def _both(datas, canvas, device_kw=None, **kw):
  """decode() of one batch by a host-mode and a device-mode decoder, each into a destination pre-filled with 0xFF."""
  n = len(datas)
  outs = []
  for mode in ({}, dict(entropy='device', **(device_kw or {}))):
    dec = jpeg.JpegDecoder(n, canvas[0], canvas[1], **kw.get('ctor', {}), **mode)
    out = torch.full((n, canvas[0], canvas[1], 3), 0xFF, dtype=torch.uint8, device=gu.DEV)
    raw, sizes = dec.decode(datas, out=out, **kw.get('decode', {}))
    torch.cuda.synchronize()
    outs.append((raw.cpu().numpy(), sizes.copy(), dec))
  return outs


@pytest.mark.gpu
@pytest.mark.parametrize('bits', [64, 1024])
def test_decoder_equals_the_host_mode(cases, bits):
  ok, _ = cases
  datas = [ok[n] for n in MIXED]
  (want, wsizes, _), (got, gsizes, dec) = _both(datas, CANVAS, dict(subseq_bits=bits))
  assert np.array_equal(got, want) and np.array_equal(gsizes, wsizes)
  assert not dec.scan_status().any() and dec.scan_failures(dec.depth - 1) == []
  assert (dec.scan_rounds() >= 1).all()
  # a batch of one (noise at quality 100: more than the default 64 bytes a block), and the real image
  with pytest.raises(ValueError, match=r'contents\[0\] is not decoded: no room left .* scan_bytes=6720 bytes.*\(status 6\)'):
    jpeg.JpegDecoder(1, 37, 53, entropy='device').decode([ok['s37x53_444_q100']])
  for name, canvas in (('s37x53_444_q100', (37, 53)), ('big_480x640_420', (480, 640))):
    (want, wsizes, _), (got, gsizes, _) = _both([ok[name]], canvas, dict(subseq_bits=bits, scan_bytes=len(ok[name])))
    assert np.array_equal(got, want) and np.array_equal(gsizes, wsizes), name


@pytest.mark.gpu
def test_decoder_equals_the_host_mode_at_forced_ratios(cases):
  ok, _ = cases
  datas = [ok[n] for n in MIXED]
  ratios = [(1, 2, 4, 8)[i % 4] for i in range(len(datas))]
  kw = dict(ctor=dict(max_ratio=8), decode=dict(ratios=ratios))
  (want, wsizes, _), (got, gsizes, _) = _both(datas, CANVAS, dict(subseq_bits=128), **kw)
  assert np.array_equal(got, want) and np.array_equal(gsizes, wsizes)
  assert gsizes[MIXED.index('restart_24x280_420')].tolist() == [12, 140]      # ratio 2
  # chosen ratios: a canvas the big image fits at ratio 8 only
  (want, wsizes, _), (got, gsizes, _) = _both([ok['big_480x640_420'], ok['s17x33_420_q75']], (60, 80), **dict(ctor=dict(max_ratio=8, coef_blocks=8000)))
  assert np.array_equal(got, want) and gsizes.tolist() == wsizes.tolist() == [[60, 80], [17, 33]]


@pytest.mark.gpu
def test_slot_reuse_over_three_batches(cases):
  ok, _ = cases
  host = jpeg.JpegDecoder(len(MIXED), *CANVAS, depth=2)
  dev = jpeg.JpegDecoder(len(MIXED), *CANVAS, depth=2, entropy='device', subseq_bits=128)
  rng = np.random.default_rng(3)
  got, want = [], []
  for _ in range(3):      # no synchronisation in between: the third batch takes the first one's set
    datas = [ok[MIXED[i]] for i in rng.permutation(len(MIXED))]
    want.append(host.decode(datas))
    got.append(dev.decode(datas))
  torch.cuda.synchronize()
  for (g, gs), (w, ws) in zip(got, want):
    assert np.array_equal(g.cpu().numpy(), w.cpu().numpy()) and np.array_equal(gs, ws)
  assert not np.array_equal(got[0][1], got[2][1])      # (the orders differed)


@pytest.mark.gpu
def test_a_stream_truncated_inside_its_scan(cases):
  """The refusal path of the kernel: a segment that ends early completes fewer blocks than its share.  Bounded loops and
  checked reads take it there; nothing else happens to the batch."""
  ok, refused = cases
  names = ['s17x33_420_q75', 'truncated_17x33', 's37x53_444_q100', 'restart_24x280_420']
  datas = [ok[n] if n in ok else refused[n][0] for n in names]
  good = [0, 2, 3]
  host = jpeg.JpegDecoder(4, *CANVAS)
  with pytest.raises(ValueError, match=r'contents\[1\] is not decoded: a malformed or truncated stream \(status 7\)'):
    host.decode(datas)
  fill = np.full((5, 7, 3), 9, np.uint8)
  want, wsizes = host.decode(datas, fallback=lambda data: fill)
  dev = jpeg.JpegDecoder(4, *CANVAS, entropy='device', subseq_bits=64)
  out = torch.full((4,) + CANVAS + (3,), 0xFF, dtype=torch.uint8, device=gu.DEV)
  raw, sizes = dev.decode(datas, out=out)      # not reported here: check_scan is False
  status = dev.scan_status()
  assert status.tolist() == [0, jpeg.MALFORMED, 0, 0] and dev.scan_status(wait=False).tolist() == status.tolist()
  got = raw.cpu().numpy()
  assert np.array_equal(got[good], want.cpu().numpy()[good]) and not got[1].any()
  assert sizes.tolist() == [[17, 33], [17, 33], [37, 53], [24, 280]]      # the header's size
  with pytest.raises(ValueError, match=r'contents\[1\] is not decoded: a malformed or truncated stream \(status 7\)'):
    dev.decode(datas, check_scan=True)
  seen = []

  def fallback(data):
    seen.append(bytes(data))
    return fill
  out.fill_(0xFF)
  raw, sizes = dev.decode(datas, out=out, fallback=fallback, check_scan=True)
  torch.cuda.synchronize()
  assert seen == [datas[1]] and np.array_equal(raw.cpu().numpy(), want.cpu().numpy()) and np.array_equal(sizes, wsizes)
  assert dev.scan_status().tolist() == [0, jpeg.MALFORMED, 0, 0]


@pytest.mark.gpu
def test_header_level_refusals_raise_on_the_host(cases):
  ok, refused = cases
  dev = jpeg.JpegDecoder(2, *CANVAS, entropy='device')
  host = jpeg.JpegDecoder(2, *CANVAS)
  for name in ('progressive_17x33', 'cmyk_16x16', 'huffman_17x33'):
    messages = []
    for dec in (host, dev):
      with pytest.raises(ValueError) as e:
        dec.decode([ok['s8x9_420_q75'], refused[name][0]])
      messages.append(str(e.value))
    assert messages[0] == messages[1] and 'contents[1]' in messages[0] and '(status %d)' % refused[name][1] in messages[0], name
  fill = np.full((3, 4, 3), 200, np.uint8)
  raw, sizes = dev.decode([refused['cmyk_16x16'][0], ok['s8x9_420_q75']], fallback=lambda data: fill)
  want, wsizes = host.decode([refused['cmyk_16x16'][0], ok['s8x9_420_q75']], fallback=lambda data: fill)
  torch.cuda.synchronize()
  assert np.array_equal(raw.cpu().numpy(), want.cpu().numpy()) and sizes.tolist() == wsizes.tolist() == [[3, 4], [8, 9]]
  assert dev.scan_status().tolist() == [jpeg.COMPONENTS, 0] and dev.scan_failures(dev.depth - 1) == []


@pytest.mark.gpu
def test_decode_jpeg_takes_the_switch(cases):
  ok, refused = cases
  for name in ('s37x53_422_q75', 's37x53_444_q100', 'restart_24x280_420', 'grey_19x13_q90', 's1x1_422_q75'):
    for ratio in (1, 4):
      want = jpeg.decode_jpeg(ok[name], ratio=ratio)
      got = jpeg.decode_jpeg(ok[name], ratio=ratio, entropy='device')
      assert got.shape == want.shape and torch.equal(got, want), (name, ratio)
  with pytest.raises(ValueError, match='a malformed or truncated stream'):
    jpeg.decode_jpeg(refused['truncated_17x33'][0], entropy='device')


def _record(data, k, boxes, **more):
  """One detection Example, as tests/test_dataloader.py builds it: `boxes` rows drawn from a generator seeded by k."""
  rng = np.random.default_rng(1000 + k)
  lo = (rng.random((boxes, 2)) * 0.5).astype(np.float32)
  hi = lo + (0.2 + rng.random((boxes, 2)) * 0.3).astype(np.float32)
  feats = {'image/encoded': data, 'image/object/bbox/ymin': lo[:, 0], 'image/object/bbox/xmin': lo[:, 1],
           'image/object/bbox/ymax': hi[:, 0], 'image/object/bbox/xmax': hi[:, 1],
           'image/object/class/label': rng.integers(1, 91, boxes)}
  for key, name in (('crowd', 'image/object/is_crowd'), ('source_id', 'image/source_id')):
    if key in more:
      feats[name] = more[key]
  if 'area' in more:
    feats['image/object/area'] = np.asarray(more['area'], np.float32)
  if 'stored_size' in more:
    feats['image/height'], feats['image/width'] = more['stored_size']
  return tfrecord.encode_example(feats)


def _shards(folder, records, name='part'):
  for i, part in enumerate(records):
    with tfrecord.TFRecordWriter(folder / ('%s-%05d.tfrecord' % (name, i))) as w:
      for r in part:
        w.write(r)
  return str(folder / (name + '-*.tfrecord'))


@pytest.mark.gpu
def test_input_reader_takes_the_switch(cases, tmp_path):
  ok, refused = cases
  images = ('s8x9_420_q75', 's16x16_444_q75', 's17x33_422_q75', 's31x22_420_q75', 's37x53_444_q75', 'grey_16x16_q75')
  spec = [dict(boxes=2, source_id='11', area=[100.0, 2500.0], crowd=[0, 0]), dict(boxes=3, crowd=[0, 1, 0], source_id=''),
          dict(boxes=0, source_id='13'), dict(boxes=5, source_id='14', stored_size=(31, 22)), dict(boxes=1, crowd=[]),
          dict(boxes=4, source_id='16', area=[])]
  records = [_record(ok[name], k, **s) for k, (name, s) in enumerate(zip(images, spec))]
  pattern = _shards(tmp_path, [records[:3], records[3:]])
  params = hparams_config.get_efficientdet_config('efficientdet-d0').as_dict()
  params.update(tf_random_seed=13, batch_size=4, drop_remainder=False)
  for is_training, count in ((False, 2), (True, 3)):
    readers = [dataloader.InputReader(pattern, is_training=is_training, **mode).reader(params, batch_size=4, canvas=(64, 64))
               for mode in ({}, dict(jpeg_entropy='device'))]
    batches = [[], []]
    for k in range(count):
      for which, reader in enumerate(readers):
        batches[which].append(next(reader))
    if not is_training:
      for reader in readers:
        with pytest.raises(StopIteration):
          next(reader)
    torch.cuda.synchronize()
    for reader in readers:
      reader.close()
    for want, got in zip(*batches):
      assert torch.equal(got[0][0], want[0][0]) and np.array_equal(got[0][1], want[0][1])
      for g, w in zip(got[1:], want[1:]):
        assert g.dtype == w.dtype and np.array_equal(g, w)
  # a record whose scan is truncated: the host mode names it at once, the device mode when the set of arenas comes round again
  (tmp_path / 'bad').mkdir()
  bad = [_record(ok[images[k % 6]] if k != 5 else refused['truncated_17x33'][0], k, 1) for k in range(8)]
  pattern = _shards(tmp_path / 'bad', [bad])
  with pytest.raises(ValueError, match=r'contents\[1\] is not decoded.*record 5'):
    list(dataloader.InputReader(pattern, is_training=False).reader(params, batch_size=4, canvas=(64, 64)))
  reader = dataloader.InputReader(pattern, is_training=False, jpeg_entropy='device').reader(params, batch_size=4, canvas=(64, 64))
  first = next(reader)
  (raw, sizes) = next(reader)[0]
  assert not raw[1].any() and sizes[1].tolist() == [17, 33] and first[0][1][0].tolist() == [8, 9]
  with pytest.raises(ValueError, match=r'batch 1: the scan of image \[1\] is malformed or truncated.*part-00000.tfrecord record 5'):
    next(reader)
  reader.close()
