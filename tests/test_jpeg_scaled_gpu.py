"""JPEG decode at reduced size on the device (automl_amd/jpeg.py on csrc/jpeg_scaled.hip): edet_jpeg_idct_scaled equals the
planes of the numpy restatement tests/jpeg_scaled_ref.py, padding blocks included, with nothing written outside them;
edet_jpeg_color_scaled, fed the restatement's planes, equals its image; JpegDecoder(max_ratio=8).decode of one mixed batch
equals v2_preprocessing.pad_batch of the pixels Pillow decoded in draft mode (tests/golden/jpeg_scaled_cases.npz) byte for byte
-- the restatement's where Pillow has no answer; the 640x480 stream at ratio 2 and 8; forced ratios and the fallback; arena
rotation; max_ratio=1 and ratio=1 against the full-size path; and TrainableModel.test_step fed the decoder's pair.
array_equal throughout."""
import os

import numpy as np
import pytest
import torch

from automl_amd import effnetv2_train, jpeg, v2_preprocessing as vp
from automl_amd._lib import call, ptr
from tests import gpu_util as gu
from tests import jpeg_ref as jr
from tests import jpeg_scaled_ref as js

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
SCALED = os.path.join(ROOT, 'tests', 'golden', 'jpeg_scaled_cases.npz')
SIZES = ('1x1', '8x9', '16x16', '17x33', '31x22', '37x53', '24x280')
# the canvas 10 x 36 gives these ratios 2, 4, 8, 1, 1, 4, 2, 8, 2, 1, 4
MIXED = ['s17x33_420_q75', 's37x53_444_q75', 's24x280_420_q75', 's8x9_422_q75', 's1x1_420_q75', 's31x22_422_q75',
         's16x16_422_q100', 's64x64_420_q75', 'grey_19x13_q90', 's8x9_444_q75', 's37x53_422_q75']
MIXED_CANVAS = (10, 36)
MIXED_RATIOS = [2, 4, 8, 1, 1, 4, 2, 8, 2, 1, 4]


@pytest.fixture(scope='module')
def cases():
  """name -> (bytes, {ratio: pixels}; ratio 1: the full-size fixture's), the (name/rN) Pillow has no answer for, a refused
  stream, and the 640x480 stream."""
  g, s = np.load(GOLDEN), np.load(SCALED)
  names = [str(n) for n in s['names']]
  ok = {n: (g[n + '/bytes'].tobytes(), {1: g[n + '/rgb']}) for n in names}
  ok.update({str(n): (s[str(n) + '/bytes'].tobytes(), {}) for n in s['new']})
  for n, (data, pixels) in ok.items():
    pixels.update({int(r): s['%s/r%d' % (n, r)] for r in s['ratios']})
    if 1 not in pixels:
      pixels[1] = jr.decode(data)      # (make_golden_jpeg_scaled.py compared it with Pillow)
  return ok, set(str(n) for n in s['restated']), g['truncated_17x33/bytes'].tobytes(), g['big_480x640_420/bytes'].tobytes()


@pytest.fixture(scope='module')
def small(cases):
  """Every size, sampling and ratio as ONE batch -- together with ratio-1 images and one refused stream: the names and
  ratios, the host stage's arrays and the restatement's planes and images."""
  ok = cases[0]
  jobs = [('s%s_%s_q75' % (size, sub), r) for size in SIZES for sub in ('444', '422', '420') for r in (2, 4, 8)]
  jobs += [(n, r) for n in ('grey_16x16_q75', 'grey_19x13_q90', 's16x16_422_q100', 's64x64_420_q75') for r in (2, 4, 8)]
  jobs += [('s17x33_420_q75', 1), ('s37x53_422_q75', 1), ('grey_19x13_q90', 1), ('s24x280_444_q75', 1)]
  jobs.insert(20, ('refused', 2))
  datas = [cases[2] if n == 'refused' else ok[n][0] for n, _ in jobs]
  canvas = (40, 288)
  parsed = {n: jr.parse(ok[n][0]) for n in set(n for n, _ in jobs) if n != 'refused'}
  blocks = sum(sum(b.size // 64 for b in parsed[n].coefs) for n, _ in jobs if n != 'refused') + 64
  coef = np.zeros(blocks * 64, np.int16)
  images = np.zeros(len(jobs) * jpeg.IMAGE_BYTES, np.uint8)
  qt = np.zeros((len(jobs), 4, 64), np.uint16)
  status = np.zeros(len(jobs), np.int32)
  jpeg.entropy_decode_scaled(datas, canvas[0], canvas[1], 8, [r for _, r in jobs], coef, images, qt, status)
  assert [int(v) for v in status] == [jpeg.MALFORMED if n == 'refused' else 0 for n, _ in jobs]
  desc = jpeg.descriptors(images, len(jobs))
  planes = [None if n == 'refused' else js.planes(parsed[n], r) for n, r in jobs]
  rgb = [None if n == 'refused' else js.color(parsed[n], r, pl) for (n, r), pl in zip(jobs, planes)]
  for (n, r), img in zip(jobs, rgb):      # the restatement's images are the fixture's
    assert n == 'refused' or np.array_equal(img, ok[n][1][r]), (n, r)
  return dict(jobs=jobs, coef=coef, images=images, qt=qt, desc=desc, planes=planes, rgb=rgb, blocks=blocks)


def _dev(a):
  return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gu.DEV)


@pytest.mark.gpu
def test_idct_equals_the_restatement(small):
  s = small
  live = [d for d in s['desc'] if not d.status]
  used = max(d.first_block[0] + d.total_blocks for d in live)
  assert used <= s['blocks'] and max(d.total_blocks for d in live) > 4 * 32 and max(d.blocks_w[0] for d in live) > 32
  canary = 4096
  planes = torch.full((s['blocks'] * 64 + canary,), 0xA5, dtype=torch.uint8, device=gu.DEV)
  coef, images, qt = _dev(s['coef']), _dev(s['images']), _dev(s['qt'])
  call('edet_jpeg_idct_scaled', ptr(coef), ptr(images), ptr(qt), len(s['jobs']), max(d.total_blocks for d in live),
       ptr(planes), s['blocks'] * 64, gu.stream())
  got = planes.cpu().numpy()
  for (name, ratio), d, want in zip(s['jobs'], s['desc'], s['planes']):
    if want is None:
      assert d.status and d.total_blocks == 0
      continue
    assert d.reserved == ratio
    sizes = js.sample_sizes(d.components, d.h_max, d.v_max, ratio)
    for c in range(d.components):
      h, w = d.blocks_h[c] * sizes[c], d.blocks_w[c] * sizes[c]
      assert want[c].shape == (h, w), (name, ratio, c)
      at = d.first_block[c] * 64
      assert np.array_equal(got[at:at + h * w].reshape(h, w), want[c]), (name, ratio, c)
      end = at + 64 * d.blocks_h[c] * d.blocks_w[c]      # the slot the full-size plane had
      assert (got[at + h * w:end] == 0xA5).all(), (name, ratio, c)      # its unused tail
  assert (got[used * 64:] == 0xA5).all()      # nothing behind the last block of the batch


@pytest.mark.gpu
@pytest.mark.parametrize('canvas', [(40, 288), (41, 283)])      # three words per four pixels / bytes (width % 4 != 0)
def test_color_equals_the_restatement(small, canvas):
  s = small
  n = len(s['jobs'])
  # the cases the replication rule is about: two chroma columns at 4:2:2 (ratio 4: 16x16 and 8x9), and 4:2:2 at ratio 8
  for job in (('s16x16_422_q75', 4), ('s16x16_422_q100', 4), ('s8x9_422_q75', 4), ('s37x53_422_q75', 8), ('s24x280_422_q75', 8)):
    assert job in s['jobs']
  arena = np.zeros(s['blocks'] * 64, np.uint8)
  for d, pl in zip(s['desc'], s['planes']):
    for c in range(d.components):
      arena[d.first_block[c] * 64:d.first_block[c] * 64 + pl[c].size] = pl[c].reshape(-1)
  images = s['images'].copy()
  rows = images.view(np.int32).reshape(n, 20)
  bad = s['jobs'].index(('s17x33_444_q75', 4))
  rows[bad, 0] = jpeg.MALFORMED      # a refused image in between: an all-zero canvas
  odd = s['jobs'].index(('s31x22_420_q75', 2))
  rows[odd, 19] = 3      # a denominator the host stage never writes: refused too
  raw = torch.full((n, canvas[0], canvas[1], 3), 0xFF, dtype=torch.uint8, device=gu.DEV)
  tail = torch.full((4096,), 0xA5, dtype=torch.uint8, device=gu.DEV)
  arena_dev, images_dev = _dev(arena), _dev(images)      # (held until the result has been read back)
  call('edet_jpeg_color_scaled', ptr(arena_dev), ptr(images_dev), n, canvas[0], canvas[1], s['blocks'] * 64, ptr(raw),
       gu.stream())
  got = raw.cpu().numpy()
  for i, ((name, ratio), d, rgb) in enumerate(zip(s['jobs'], s['desc'], s['rgb'])):
    want = np.zeros((canvas[0], canvas[1], 3), np.uint8)
    if rgb is not None and i not in (bad, odd):
      assert rgb.shape == (d.height, d.width, 3)
      want[:d.height, :d.width] = rgb
    assert np.array_equal(got[i], want), (name, ratio)
  assert (tail.cpu().numpy() == 0xA5).all()


@pytest.mark.gpu
def test_decoder_equals_pad_batch_of_pillows_pixels(cases):
  ok, restated, _, _ = cases
  canvas = MIXED_CANVAS
  dec = jpeg.JpegDecoder(len(MIXED), canvas[0], canvas[1], threads=3, max_ratio=8)
  out = torch.full((len(MIXED), canvas[0], canvas[1], 3), 0xFF, dtype=torch.uint8, device=gu.DEV)
  sizes_out = np.full((len(MIXED), 2), -1, np.int32)
  ratios_out = np.full(len(MIXED), -1, np.int32)
  raw, sizes = dec.decode([ok[n][0] for n in MIXED], out=out, sizes_out=sizes_out, ratios_out=ratios_out)
  assert raw is out and sizes is sizes_out
  assert ratios_out.tolist() == MIXED_RATIOS == [jpeg.choose_ratio(*(ok[n][1][1].shape[:2] + canvas)) for n in MIXED]
  assert not any('%s/r%d' % (n, r) in restated for n, r in zip(MIXED, MIXED_RATIOS))      # Pillow's pixels, all of them
  want, want_sizes = vp.pad_batch([ok[n][1][r] for n, r in zip(MIXED, MIXED_RATIOS)], canvas)
  assert sizes.dtype == want_sizes.dtype and np.array_equal(sizes, want_sizes)
  assert raw.dtype == torch.uint8 and raw.shape == want.shape and torch.equal(raw.cpu(), want)
  # where Pillow has no answer the restatement is the definition: 1x1 at every ratio, forced
  names = ['s1x1_444_q75', 's1x1_422_q75', 's1x1_420_q75', 's8x9_420_q75']
  for ratio in (2, 4, 8):
    assert all('%s/r%d' % (n, ratio) in restated for n in names[:3])
    raw, sizes = jpeg.JpegDecoder(4, 8, 12, max_ratio=8).decode([ok[n][0] for n in names], ratios=[ratio] * 4)
    want, want_sizes = vp.pad_batch([js.decode(ok[n][0], ratio) for n in names], (8, 12))
    assert np.array_equal(sizes, want_sizes) and torch.equal(raw.cpu(), want), ratio
  # every family of the fixture, one image at a time, at every ratio
  for name, (data, pixels) in ok.items():
    for ratio in (2, 4, 8):
      got = jpeg.decode_jpeg(data, channels=0 if name.startswith('grey') else 3, ratio=ratio)
      assert np.array_equal(got.cpu().numpy(), pixels[ratio]), (name, ratio)


@pytest.fixture(scope='module')
def big(cases):
  return cases[3], jr.parse(cases[3])


@pytest.mark.gpu
@pytest.mark.parametrize('canvas, ratio', [((240, 320), 2), ((100, 100), 8)])      # an exact fit; 60 x 80 inside 100 x 100
def test_whole_size_image(cases, big, canvas, ratio):
  data, parsed = big
  small = cases[0]['s37x53_422_q75']
  # (two 640x480 files have more blocks than the default arena of a 100 x 100 canvas: four full-size batches)
  dec = jpeg.JpegDecoder(3, canvas[0], canvas[1], max_ratio=8, coef_blocks=3 * jpeg.worst_blocks(480, 640))
  ratios = np.zeros(3, np.int32)
  raw, sizes = dec.decode([data, small[0], data], ratios_out=ratios)
  size = jpeg.scaled_size(480, 640, ratio)
  assert ratios.tolist() == [ratio, 1, ratio] and sizes.tolist() == [list(size), [37, 53], list(size)]
  want, _ = vp.pad_batch([js.color(parsed, ratio), small[1][1]], canvas)
  assert torch.equal(raw[:2].cpu(), want) and torch.equal(raw[2], raw[0])


@pytest.mark.gpu
def test_forced_ratios_and_the_fallback(cases):
  ok, _, refused, _ = cases
  canvas = MIXED_CANVAS
  datas = [ok[n][0] for n in MIXED]
  dec = jpeg.JpegDecoder(len(MIXED), canvas[0], canvas[1], max_ratio=8)
  chosen, sizes = dec.decode(datas)
  forced, forced_sizes = dec.decode(datas, ratios=MIXED_RATIOS)
  assert torch.equal(forced, chosen) and np.array_equal(forced_sizes, sizes)
  # a larger ratio than needed is honoured; one whose output does not fit goes to the fallback, as a refused stream does
  ratios = list(MIXED_RATIOS)
  ratios[0], ratios[1] = 8, 2      # 17x33 at 1/8: 3 x 5; 37x53 at 1/2: 19 x 27, too high
  with pytest.raises(ValueError, match=r'contents\[1\].*canvas'):
    dec.decode(datas, ratios=ratios)
  seen = []
  fill = np.arange(9 * 11 * 3, dtype=np.uint8).reshape(9, 11, 3)

  def fallback(data):
    seen.append(data)
    return fill
  got_ratios = np.zeros(len(MIXED), np.int32)
  raw, sizes = dec.decode(datas[:2] + [refused] + datas[3:], ratios=ratios, fallback=fallback, ratios_out=got_ratios)
  assert seen == [datas[1], refused] and got_ratios.tolist() == [8, 1, 1] + MIXED_RATIOS[3:]
  images = [ok[n][1][r] for n, r in zip(MIXED, ratios)]
  images[1] = images[2] = fill
  want, want_sizes = vp.pad_batch(images, canvas)
  assert torch.equal(raw.cpu(), want) and np.array_equal(sizes, want_sizes)
  for bad in ([1] * 3, [3] * len(MIXED), [16] * len(MIXED)):
    with pytest.raises(ValueError, match='ratios'):
      dec.decode(datas, ratios=bad)
  with pytest.raises(ValueError, match='ratios'):
    jpeg.JpegDecoder(len(MIXED), canvas[0], canvas[1], max_ratio=2).decode(datas, ratios=[4] * len(MIXED))
  # an arena too small for the batch: the image that no longer fits names coef_blocks
  blocks = [sum(b.size // 64 for b in jr.parse(d).coefs) for d in datas[:3]]
  tight = jpeg.JpegDecoder(3, canvas[0], canvas[1], max_ratio=8, coef_blocks=sum(blocks) - 1)
  with pytest.raises(ValueError, match=r'contents\[2\].*coef_blocks'):
    tight.decode(datas[:3])
  raw, sizes = tight.decode(datas[:3], fallback=fallback)
  assert sizes.tolist() == [[9, 17], [10, 14], [9, 11]] and torch.equal(raw[:2], chosen[:2])


@pytest.mark.gpu
def test_arena_rotation(cases):
  ok = cases[0]
  canvas = MIXED_CANVAS
  first, second, third = ([ok[n][0] for n in MIXED[k:k + 3]] for k in (0, 3, 6))
  dec = jpeg.JpegDecoder(3, *canvas, depth=2, max_ratio=8)
  a, sa = dec.decode(first)
  b, sb = dec.decode(second)
  c, sc = dec.decode(third)      # the first set again, behind its event
  for got, got_sizes, k in ((a, sa, 0), (b, sb, 3), (c, sc, 6)):
    want, want_sizes = vp.pad_batch([ok[n][1][r] for n, r in zip(MIXED[k:k + 3], MIXED_RATIOS[k:k + 3])], canvas)
    assert torch.equal(got.cpu(), want) and np.array_equal(got_sizes, want_sizes), k
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  d, _ = dec.decode(second, stream=side)
  side.synchronize()
  assert torch.equal(d, b)


@pytest.mark.gpu
def test_ratio_one_is_the_full_size_path(cases):
  ok = cases[0]
  names = ['s37x53_420_q75', 's31x22_422_q75', 's24x280_444_q75', 'grey_16x16_q75']
  datas = [ok[n][0] for n in names]
  canvas = (40, 284)
  full, full_sizes = jpeg.JpegDecoder(4, *canvas).decode(datas)
  assert torch.equal(full.cpu(), vp.pad_batch([ok[n][1][1] for n in names], canvas)[0])
  one = jpeg.JpegDecoder(4, *canvas, max_ratio=1)
  assert one.blocks == 4 * jpeg.worst_blocks(*canvas)      # the allocations are today's
  ratios = np.zeros(4, np.int32)
  got, sizes = one.decode(datas, ratios=[1] * 4, ratios_out=ratios)
  assert torch.equal(got, full) and np.array_equal(sizes, full_sizes) and ratios.tolist() == [1] * 4
  # the reduced-size kernels on images that all fit: the same bytes
  got, sizes = jpeg.JpegDecoder(4, *canvas, max_ratio=8).decode(datas, ratios_out=ratios)
  assert torch.equal(got, full) and np.array_equal(sizes, full_sizes) and ratios.tolist() == [1] * 4
  for name in names[:2]:
    assert torch.equal(jpeg.decode_jpeg(ok[name][0], ratio=1), jpeg.decode_jpeg(ok[name][0]))
    assert np.array_equal(jpeg.decode_jpeg(ok[name][0], 3, 1).cpu().numpy(), ok[name][1][1])


@pytest.mark.gpu
def test_test_step_on_the_scaled_pair(cases):
  """The smallest V2 model, batch 2: test_step fed decode()'s (raw, sizes) at ratios 2 and 1 and fed pad_batch of the same
  pixels."""
  ok = cases[0]
  names, ratios = ['s64x64_420_q75', 's31x22_422_q75'], [2, 1]
  canvas = (40, 56)
  labels = np.array([3, 17])

  def net():
    return effnetv2_train.TrainableModel('efficientnetv2-b0', 'num_classes=24', learning_rate=0.01, seed=4, use_graph=False,
                                         dtype='f32', image_size=32)
  got_ratios = np.zeros(2, np.int32)
  raw, sizes = jpeg.JpegDecoder(2, *canvas, max_ratio=8).decode([ok[n][0] for n in names], ratios_out=got_ratios)
  assert got_ratios.tolist() == ratios and sizes.tolist() == [[32, 32], [31, 22]]
  got = net().test_step(((raw, sizes), labels))
  want = net().test_step((vp.pad_batch([ok[n][1][r] for n, r in zip(names, ratios)], canvas), labels))
  assert got == want and np.isfinite(got['loss']), (got, want)
