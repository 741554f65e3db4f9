"""The JPEG decoder on the device (automl_amd/jpeg.py on csrc/jpeg.hip): edet_jpeg_idct equals the planes of the numpy
restatement tests/jpeg_ref.py, padding blocks included; edet_jpeg_color, fed the restatement's planes, equals its image;
JpegDecoder.decode of one mixed batch equals v2_preprocessing.pad_batch of the pixels Pillow decoded
(tests/golden/jpeg_cases.npz; Pillow itself is not needed here) byte for byte, zero padding included; arena rotation, the
fallback, the 640x480 case, decode_jpeg, and TrainableModel.test_step fed the decoder's pair.  array_equal throughout."""
import os

import numpy as np
import pytest
import torch

from automl_amd import _lib, effnetv2_train, jpeg, v2_preprocessing as vp
from automl_amd._lib import call, ptr
from tests import gpu_util as gu
from tests import jpeg_ref as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
MIXED = ['s17x33_420_q75', 'grey_19x13_q90', 's31x22_422_q75', 's37x53_444_q75', 's1x1_420_q75', 'restart_24x280_420',
         's8x9_422_q75', 'optimize_31x22_420', 's37x53_420_q100', 'grey_16x16_q75', 's16x16_420_q75', 'const_20x20_420']


@pytest.fixture(scope='module')
def cases():
  g = np.load(GOLDEN)
  ok = {str(n): (g[str(n) + '/bytes'].tobytes(), g[str(n) + '/rgb']) for n in g['names']}
  refused = {str(n): (g[str(n) + '/bytes'].tobytes(), int(g[str(n) + '/status'])) for n in g['refused']}
  return ok, refused


@pytest.fixture(scope='module')
def small(cases):
  """Every case but the 640x480 one, as one batch: names, the host stage's arrays and the restatement's planes."""
  names = sorted(n for n in cases[0] if not n.startswith('big'))
  datas = [cases[0][n][0] for n in names]
  canvas = (40, 288)
  blocks = len(names) * jpeg.worst_blocks(*canvas)
  coef = np.zeros(blocks * 64, np.int16)
  images = np.zeros(len(names) * jpeg.IMAGE_BYTES, np.uint8)
  qt = np.zeros((len(names), 4, 64), np.uint16)
  status = np.zeros(len(names), np.int32)
  jpeg.entropy_decode(datas, canvas[0], canvas[1], coef, images, qt, status)
  assert not status.any()
  desc = jpeg.descriptors(images, len(names))
  planes = [jr.planes(jr.parse(d)) for d in datas]
  return dict(names=names, coef=coef, images=images, qt=qt, desc=desc, planes=planes, blocks=blocks)


def _dev(a):
  return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gu.DEV)


@pytest.mark.gpu
def test_idct_equals_the_restatement(small):
  s = small
  used = max(d.first_block[0] + d.total_blocks for d in s['desc'])
  assert used > 4 * 32 and max(d.blocks_w[0] for d in s['desc']) > 32      # more than one workgroup, a block row of > 32
  canary = 4096
  planes = torch.full((s['blocks'] * 64 + canary,), 0xA5, dtype=torch.uint8, device=gu.DEV)
  coef, images, qt = _dev(s['coef']), _dev(s['images']), _dev(s['qt'])
  call('edet_jpeg_idct', ptr(coef), ptr(images), ptr(qt), len(s['names']), max(d.total_blocks for d in s['desc']),
       ptr(planes), s['blocks'] * 64, gu.stream())
  got = planes.cpu().numpy()
  for name, d, want in zip(s['names'], s['desc'], s['planes']):
    for c in range(d.components):
      h, w = d.blocks_h[c] * 8, d.blocks_w[c] * 8
      assert want[c].shape == (h, w), (name, c)
      at = d.first_block[c] * 64
      assert np.array_equal(got[at:at + h * w].reshape(h, w), want[c]), (name, c)
  assert (got[used * 64:] == 0xA5).all()      # nothing behind the last block of the batch


@pytest.mark.gpu
@pytest.mark.parametrize('canvas', [(40, 288), (41, 283)])      # three words per four pixels / bytes (width % 4 != 0)
def test_color_equals_the_restatement(small, canvas):
  s = small
  n = len(s['names'])
  arena = np.zeros(s['blocks'] * 64, np.uint8)
  for d, pl in zip(s['desc'], s['planes']):
    for c in range(d.components):
      arena[d.first_block[c] * 64:d.first_block[c] * 64 + pl[c].size] = pl[c].reshape(-1)
  images = s['images'].copy()
  bad = s['names'].index('s17x33_444_q75')
  images.view(np.int32).reshape(n, 20)[bad, 0] = jpeg.MALFORMED      # a refused image in between: an all-zero canvas
  raw = torch.full((n, canvas[0], canvas[1], 3), 0xFF, dtype=torch.uint8, device=gu.DEV)
  tail = torch.full((4096,), 0xA5, dtype=torch.uint8, device=gu.DEV)
  call('edet_jpeg_color', ptr(_dev(arena)), ptr(_dev(images)), n, canvas[0], canvas[1], s['blocks'] * 64, ptr(raw),
       gu.stream())
  got = raw.cpu().numpy()
  for i, (name, d, pl) in enumerate(zip(s['names'], s['desc'], s['planes'])):
    want = np.zeros((canvas[0], canvas[1], 3), np.uint8)
    if i != bad:
      dec = jr.Decoded(jr.Frame(d.height, d.width, d.components, 8, 0, 0, 0xC0, (), (), (), (), 1, -1), d.h_max, d.v_max,
                       list(d.blocks_w), list(d.blocks_h), None, None)
      want[:d.height, :d.width] = jr.color(dec, pl)
    assert np.array_equal(got[i], want), name
  assert (tail.cpu().numpy() == 0xA5).all()


@pytest.mark.gpu
def test_decoder_equals_pad_batch_of_pillows_pixels(cases):
  ok, _ = cases
  canvas = (48, 300)
  dec = jpeg.JpegDecoder(len(MIXED), canvas[0], canvas[1], threads=3)
  out = torch.full((len(MIXED), canvas[0], canvas[1], 3), 0xFF, dtype=torch.uint8, device=gu.DEV)
  sizes_out = np.full((len(MIXED), 2), -1, np.int32)
  raw, sizes = dec.decode([ok[n][0] for n in MIXED], out=out, sizes_out=sizes_out)
  assert raw is out and sizes is sizes_out
  want, want_sizes = vp.pad_batch([ok[n][1] for n in MIXED], canvas)
  assert sizes.dtype == want_sizes.dtype and np.array_equal(sizes, want_sizes)
  assert raw.dtype == torch.uint8 and raw.shape == want.shape and torch.equal(raw.cpu(), want)
  # every family of the fixture, one image at a time
  for name, (data, rgb) in ok.items():
    if name not in MIXED and not name.startswith('big'):
      got = jpeg.decode_jpeg(data, channels=0 if name.startswith('grey') else 3)
      assert np.array_equal(got.cpu().numpy(), rgb), name


@pytest.mark.gpu
def test_arena_rotation(cases):
  ok, _ = cases
  first = [ok[n][0] for n in MIXED[:4]]
  second = [ok[n][0] for n in MIXED[4:8]]
  canvas = (40, 284)
  dec = jpeg.JpegDecoder(4, *canvas, depth=2)
  a, _ = dec.decode(first)
  b, sb = dec.decode(second)
  c, _ = dec.decode(first)      # the first set again, behind its event
  a2, _ = jpeg.JpegDecoder(4, *canvas, depth=1).decode(first)
  b2, sb2 = jpeg.JpegDecoder(4, *canvas, depth=1).decode(second)
  assert torch.equal(a, a2) and torch.equal(b, b2) and torch.equal(c, a2) and np.array_equal(sb, sb2)
  assert torch.equal(a.cpu(), vp.pad_batch([ok[n][1] for n in MIXED[:4]], canvas)[0])
  with pytest.raises(ValueError):
    dec.decode(first[:3])
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  d, _ = dec.decode(second, stream=side)
  side.synchronize()
  assert torch.equal(d, b2)


@pytest.mark.gpu
def test_refused_streams_and_the_fallback(cases):
  ok, refused = cases
  canvas = (40, 64)
  datas = [ok['s37x53_420_q75'][0], refused['progressive_17x33'][0], ok['s31x22_444_q75'][0], refused['truncated_17x33'][0]]
  dec = jpeg.JpegDecoder(4, *canvas)
  with pytest.raises(ValueError, match=r'contents\[1\].*progressive'):
    dec.decode(datas)
  with pytest.raises(ValueError, match='canvas'):
    jpeg.JpegDecoder(1, 16, 16).decode([ok['s37x53_420_q75'][0]])
  with pytest.raises(ValueError, match='CMYK'):
    jpeg.decode_jpeg(refused['cmyk_16x16'][0])
  seen = []
  fill = np.arange(17 * 33 * 3, dtype=np.uint8).reshape(17, 33, 3)

  def fallback(data):
    seen.append(data)
    return fill
  raw, sizes = dec.decode(datas, fallback=fallback)
  assert seen == [datas[1], datas[3]]
  want, want_sizes = vp.pad_batch([ok['s37x53_420_q75'][1], fill, ok['s31x22_444_q75'][1], fill], canvas)
  assert torch.equal(raw.cpu(), want) and np.array_equal(sizes, want_sizes)


@pytest.mark.gpu
def test_whole_size_image(cases):
  data, rgb = cases[0]['big_480x640_420']
  dec = jpeg.JpegDecoder(3, 480, 640)
  raw, sizes = dec.decode([data, cases[0]['s37x53_422_q75'][0], data])
  assert sizes.tolist() == [[480, 640], [37, 53], [480, 640]]
  assert np.array_equal(raw[0].cpu().numpy(), rgb) and torch.equal(raw[2], raw[0])
  assert torch.equal(raw[1].cpu(), vp.pad_batch([cases[0]['s37x53_422_q75'][1]], (480, 640))[0][0])


@pytest.mark.gpu
def test_test_step_on_the_decoders_pair(cases):
  """The smallest V2 model, batch 2: test_step fed decode()'s (raw, sizes) and fed pad_batch of the same pixels."""
  ok, _ = cases
  names = ['s37x53_420_q75', 's31x22_422_q75']
  canvas = (40, 56)
  labels = np.array([3, 17])

  def net():
    return effnetv2_train.TrainableModel('efficientnetv2-b0', 'num_classes=24', learning_rate=0.01, seed=4, use_graph=False,
                                         dtype='f32', image_size=32)
  raw, sizes = jpeg.JpegDecoder(2, *canvas).decode([ok[n][0] for n in names])
  got = net().test_step(((raw, sizes), labels))
  want = net().test_step((vp.pad_batch([ok[n][1] for n in names], canvas), labels))
  assert got == want and np.isfinite(got['loss']), (got, want)
