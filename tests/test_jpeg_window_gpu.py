"""JPEG decode of a crop window on the device (automl_amd/jpeg.py on csrc/jpeg_window.hip): edet_jpeg_color_window, fed the
planes of the numpy restatement tests/jpeg_window_ref.py on the kept grids the host stage describes, equals the restatement's
windows -- every window of the CPU tests' set, ratios 1, 2, 4 and 8, a word-store and a byte-store canvas and canvases of
exactly the window's size; JpegDecoder(windowed=True).decode(windows=...) of one mixed batch equals the fixtures' pixels
cropped, zero padding included, with a refused stream that comes back whole through `fallback`; arena rotation; windows=None
against the plain decoder; decode_and_crop_jpeg on the 640x480 stream; and two train steps of the classifier fed the decoded
windows equal two steps fed the full decodes and the same crops.  array_equal throughout."""
import numpy as np
import pytest
import torch

from automl_amd import effnetv2_train, jpeg, v2_preprocessing as vp
from automl_amd._lib import call, ptr
from tests import gpu_util as gu
from tests import jpeg_ref as jr
from tests import jpeg_scaled_ref as js
from tests import jpeg_window_ref as jw
from tests.test_jpeg_window import GOLDEN, load_streams

KERNEL_STREAMS = ('s37x53_444_q75', 's37x53_422_q75', 's37x53_420_q75', 's8x9_420_q75', 's1x1_420_q75', 'grey_19x13_q90')
RATIOS = (1, 2, 4, 8)


@pytest.fixture(scope='module')
def streams():
  return load_streams()


@pytest.fixture(scope='module')
def small(streams):
  """Every stream of KERNEL_STREAMS x ratio x window of the window set as ONE batch: the host stage's arrays, and the
  restatement's kept planes and windows."""
  jobs = [(n, r, win) for n in KERNEL_STREAMS for r in RATIOS for win in jw.windows_for(*streams[n][1][r].shape[:2])]
  canvas = (40, 288)
  parsed = [jw.parse(streams[n][0], win, r) for n, r, win in jobs]
  blocks = sum(sum(c.size // 64 for c in p.coefs) for p in parsed) + 64
  b = len(jobs)
  coef = np.zeros(blocks * 64, np.int16)
  images, wins = np.zeros(b * jpeg.IMAGE_BYTES, np.uint8), np.zeros(b * jpeg.WINDOW_BYTES, np.uint8)
  qt, status = np.zeros((b, 4, 64), np.uint16), np.zeros(b, np.int32)
  jpeg.entropy_decode_window([streams[n][0] for n, _, _ in jobs], canvas[0], canvas[1], 8, [r for _, r, _ in jobs],
                             [win for _, _, win in jobs], coef, images, wins, qt, status)
  assert not status.any()
  desc = jpeg.descriptors(images, b)
  planes = [jw.planes(p) for p in parsed]
  rgb = [jw.color(p, pl) for p, pl in zip(parsed, planes)]
  for (n, r, (y, x, h, w)), img in zip(jobs, rgb):      # the restatement's windows are the fixture's pixels, cropped
    assert np.array_equal(img, streams[n][1][r][y:y + h, x:x + w]), (n, r, (y, x, h, w))
  arena = np.zeros(blocks * 64, np.uint8)
  for d, pl in zip(desc, planes):
    for c in range(d.components):
      arena[d.first_block[c] * 64:d.first_block[c] * 64 + pl[c].size] = pl[c].reshape(-1)
  return dict(jobs=jobs, images=images, wins=wins, desc=desc, rgb=rgb, blocks=blocks, arena=arena)


def _dev(a):
  return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gu.DEV)


def _color_window(s, pick, canvas):
  """edet_jpeg_color_window on the jobs `pick` of the batch -> uint8 [len(pick)][canvas][3]; a canary behind the canvases
  must stay."""
  n = len(pick)
  images = np.ascontiguousarray(s['images'].reshape(-1, jpeg.IMAGE_BYTES)[pick]).reshape(-1)
  wins = np.ascontiguousarray(s['wins'].reshape(-1, jpeg.WINDOW_BYTES)[pick]).reshape(-1)
  raw = torch.full((n * canvas[0] * canvas[1] * 3 + 4096,), 0xA5, dtype=torch.uint8, device=gu.DEV)
  arena, images_dev, wins_dev = _dev(s['arena']), _dev(images), _dev(wins)      # (held until the result has been read back)
  call('edet_jpeg_color_window', ptr(arena), ptr(images_dev), ptr(wins_dev), n, canvas[0], canvas[1], s['blocks'] * 64,
       ptr(raw), gu.stream())
  got = raw.cpu().numpy()
  assert (got[-4096:] == 0xA5).all()
  return got[:-4096].reshape(n, canvas[0], canvas[1], 3)


@pytest.mark.gpu
@pytest.mark.parametrize('canvas', [(40, 288), (41, 283)])      # three words per four pixels / bytes (width % 4 != 0)
def test_color_window_equals_the_restatement(small, canvas):
  s = small
  assert len(s['jobs']) > 150
  got = _color_window(s, list(range(len(s['jobs']))), canvas)
  for i, (job, rgb) in enumerate(zip(s['jobs'], s['rgb'])):
    want = np.zeros(canvas + (3,), np.uint8)
    want[:rgb.shape[0], :rgb.shape[1]] = rgb
    assert np.array_equal(got[i], want), job


@pytest.mark.gpu
def test_color_window_on_canvases_of_exactly_the_windows_size(small):
  s = small
  shapes = {}
  for i, rgb in enumerate(s['rgb']):
    shapes.setdefault(rgb.shape[:2], []).append(i)
  for shape in ((5, 7), (1, 1), (37, 53), (33, 49), (37, 2), (1, 53)):      # byte stores but for none; odd and even widths
    pick = shapes[shape]
    got = _color_window(s, pick, shape)
    for k, i in enumerate(pick):
      assert np.array_equal(got[k], s['rgb'][i]), (s['jobs'][i], shape)
  both = shapes[(32, 48)]      # (3, 3, 32, 48) of the 37 x 53 streams: an odd start, a width of whole words
  assert all(s['jobs'][i][2][:2] == (3, 3) for i in both)
  got = _color_window(s, both, (32, 48))
  for k, i in enumerate(both):
    assert np.array_equal(got[k], s['rgb'][i]), s['jobs'][i]


# name, ratio, window (in the output at that ratio)
MIXED = [('s37x53_420_q75', 1, (3, 5, 31, 45)), ('s37x53_422_q75', 2, (1, 1, 17, 25)), ('restart_24x280_420', 1, (2, 101, 21, 63)),
         ('refused', 1, (0, 0, 4, 4)), ('s37x53_444_q75', 4, (0, 0, 10, 14)), ('grey_19x13_q90', 1, (7, 7, 9, 6)),
         ('s17x33_420_q75', 8, (2, 4, 1, 1)), ('s8x9_422_q75', 1, (0, 0, 8, 9)), ('segments_17x33_422', 2, (8, 15, 1, 2)),
         ('s1x1_444_q75', 8, (0, 0, 1, 1)), ('restart_24x280_420', 4, (1, 3, 5, 64))]
MIXED_CANVAS = (32, 64)


def _want(streams, jobs, canvas, whole=None):
  want = np.zeros((len(jobs),) + tuple(canvas) + (3,), np.uint8)
  sizes = np.zeros((len(jobs), 2), np.int32)
  for i, (n, r, (y, x, h, w)) in enumerate(jobs):
    if n == 'refused':
      want[i, :whole.shape[0], :whole.shape[1]] = whole
      sizes[i] = whole.shape[:2]
    else:
      want[i, :h, :w] = streams[n][1][r][y:y + h, x:x + w]
      sizes[i] = (h, w)
  return want, sizes


@pytest.mark.gpu
def test_decoder_equals_the_cropped_fixture_pixels(streams):
  """One batch that mixes samplings, ratios and windows, with a restart-interval stream whose image is far wider than the
  canvas and a refused stream, which `fallback` returns whole."""
  refused = np.load(GOLDEN)['truncated_17x33/bytes'].tobytes()
  whole = streams['s17x33_444_q75'][1][1]
  datas = [refused if n == 'refused' else streams[n][0] for n, _, _ in MIXED]
  dec = jpeg.JpegDecoder(len(MIXED), MIXED_CANVAS[0], MIXED_CANVAS[1], max_ratio=8, windowed=True)
  ratios, windows = [r for _, r, _ in MIXED], np.array([w for _, _, w in MIXED], np.int32)
  out = torch.full((len(MIXED),) + MIXED_CANVAS + (3,), 0xFF, dtype=torch.uint8, device=gu.DEV)
  got_ratios = np.zeros(len(MIXED), np.int32)
  raw, sizes = dec.decode(datas, out=out, ratios=ratios, windows=windows, fallback=lambda data: whole, ratios_out=got_ratios)
  want, want_sizes = _want(streams, MIXED, MIXED_CANVAS, whole)
  assert raw is out and np.array_equal(sizes, want_sizes) and got_ratios.tolist() == [1 if n == 'refused' else r for n, r, _ in MIXED]
  got = raw.cpu().numpy()
  for i, job in enumerate(MIXED):
    assert np.array_equal(got[i], want[i]), job
  with pytest.raises(ValueError, match=r'contents\[3\] is not decoded: a malformed'):
    dec.decode(datas, ratios=ratios, windows=windows)
  # a window outside its image, and one larger than the canvas, are refused like a stream
  bad = windows.copy()
  bad[0] = (3, 5, 31, 49)
  with pytest.raises(ValueError, match=r'contents\[0\] is not decoded: a crop window outside.*status 9'):
    dec.decode(datas, ratios=ratios, windows=bad)
  bad[0] = (3, 5, 33, 45)
  with pytest.raises(ValueError, match=r'contents\[0\] is not decoded: a crop window larger than the 32 x 64 canvas'):
    dec.decode(datas, ratios=ratios, windows=bad)
  with pytest.raises(ValueError, match='needs ratios'):
    dec.decode(datas, windows=windows)
  with pytest.raises(ValueError, match=r'windows must be int \[11, 4\]'):
    dec.decode(datas, ratios=ratios, windows=windows[:3])
  plain = jpeg.JpegDecoder(1, 40, 56)
  with pytest.raises(ValueError, match='windowed=True'):
    plain.decode([streams['s37x53_420_q75'][0]], windows=[(0, 0, 1, 1)])


@pytest.mark.gpu
def test_arena_rotation_with_windows(streams):
  """depth=2, three different batches decoded back to back, the results kept and compared afterwards: the third batch writes
  the first one's arenas."""
  batches = [MIXED[0:2] + MIXED[4:6], MIXED[6:10], [MIXED[10], MIXED[2], MIXED[5], MIXED[1]]]
  dec = jpeg.JpegDecoder(4, MIXED_CANVAS[0], MIXED_CANVAS[1], max_ratio=8, windowed=True, depth=2)
  outs = [dec.decode([streams[n][0] for n, _, _ in jobs], ratios=[r for _, r, _ in jobs], windows=np.array([w for _, _, w in jobs]))
          for jobs in batches]
  torch.cuda.synchronize()
  for jobs, (raw, sizes) in zip(batches, outs):
    want, want_sizes = _want(streams, jobs, MIXED_CANVAS)
    assert np.array_equal(raw.cpu().numpy(), want) and np.array_equal(sizes, want_sizes), jobs


@pytest.mark.gpu
def test_windows_none_is_the_plain_decoder(streams):
  names = ['s37x53_420_q75', 's17x33_422_q75', 'grey_19x13_q90', 's8x9_444_q75']
  datas = [streams[n][0] for n in names]
  for max_ratio, canvas in ((1, (40, 56)), (8, (10, 36))):
    plain = jpeg.JpegDecoder(4, canvas[0], canvas[1], max_ratio=max_ratio)
    windowed = jpeg.JpegDecoder(4, canvas[0], canvas[1], max_ratio=max_ratio, windowed=True)
    assert windowed.blocks >= plain.blocks
    (a, sa), (b, sb) = plain.decode(datas), windowed.decode(datas)
    assert torch.equal(a, b) and np.array_equal(sa, sb)
  # ... and a whole-image window through the window path gives those bytes too
  windowed = jpeg.JpegDecoder(4, 40, 56, windowed=True)
  c, sc = windowed.decode(datas, windows=[(0, 0) + streams[n][1][1].shape[:2] for n in names])
  a, sa = jpeg.JpegDecoder(4, 40, 56).decode(datas)
  assert torch.equal(a, c) and np.array_equal(sa, sc)


@pytest.mark.gpu
def test_decode_and_crop_jpeg_on_the_vga_stream():
  g = np.load(GOLDEN)
  data, rgb = g['big_480x640_420/bytes'].tobytes(), g['big_480x640_420/rgb']
  got = jpeg.decode_and_crop_jpeg(data, (101, 203, 255, 301))      # interior, odd everywhere
  assert got.dtype == torch.uint8 and tuple(got.shape) == (255, 301, 3) and got.is_cuda
  assert np.array_equal(got.cpu().numpy(), rgb[101:356, 203:504])
  quarter = js.color(jr.parse(data), 4)      # 120 x 160
  got = jpeg.decode_and_crop_jpeg(data, np.array([31, 53, 67, 91]), channels=0, ratio=4)
  assert np.array_equal(got.cpu().numpy(), quarter[31:98, 53:144])
  assert np.array_equal(jpeg.decode_and_crop_jpeg(data, (0, 0, 120, 160), ratio=4).cpu().numpy(), quarter)
  with pytest.raises(ValueError, match='crop window'):
    jpeg.decode_and_crop_jpeg(data, (0, 0, 121, 160), ratio=4)


MODEL, OVER, SIZE, NC = 'efficientnetv2-b0', 'num_classes=24', 32, 24      # tests/test_effnetv2_crop.py's
TRAIN = ['s37x53_420_q75', 's37x53_422_q75', 's37x53_444_q75', 's17x33_420_q75', 'grey_19x13_q90', 's8x9_422_q75',
         's17x33_444_q75', 'segments_17x33_422']


@pytest.mark.gpu
def test_train_steps_on_decoded_windows_equal_steps_on_full_decodes_with_the_same_crops(streams):
  """Path A: train_step fed the windows the decoder cropped, transformations='flip' (the whole "image", flips drawn by the
  model).  Path B: train_step fed the full decodes, force_crop_rows = the same windows and flips.  After two steps every
  variable is bit-equal."""
  canvas = (40, 56)
  datas = [streams[n][0] for n in TRAIN]
  full_sizes = np.array([streams[n][1][1].shape[:2] for n in TRAIN], np.int32)
  rng = np.random.default_rng(11)
  args = dict(learning_rate=0.01, weight_decay=1e-5, label_smoothing=0.1, seed=4, use_graph=False, image_size=SIZE)
  a = effnetv2_train.TrainableModel(MODEL, OVER, transformations='flip', **args)
  b = effnetv2_train.TrainableModel(MODEL, OVER, **args)
  flips = vp.crop_rng(4)      # what model A's own generator draws
  dec = jpeg.JpegDecoder(len(TRAIN), canvas[0], canvas[1], windowed=True)
  plain = jpeg.JpegDecoder(len(TRAIN), canvas[0], canvas[1])
  outs = []
  for step in range(2):
    windows = np.array([vp.sample_distorted_bounding_box(rng, h, w) for h, w in full_sizes], np.int32)
    labels = rng.integers(0, NC, len(TRAIN))
    raw_a, sizes_a = dec.decode(datas, windows=windows)
    assert np.array_equal(sizes_a, windows[:, 2:])
    rows_a = vp.train_rows(flips, sizes_a, 'flip')
    raw_b, sizes_b = plain.decode(datas)
    rows_b = np.concatenate([full_sizes, windows, rows_a[:, 6:]], axis=1).astype(np.int32)
    b.force_crop_rows(rows_b)
    outs.append((a.train_step(((raw_a, sizes_a), labels)), b.train_step(((raw_b, sizes_b), labels))))
    assert np.array_equal(a.engine.crop_rows.cpu().numpy(), rows_a)
  torch.cuda.synchronize()
  assert (windows[:, 2:] < full_sizes).any() and rows_a[:, 6].any()
  for got, want in outs:
    assert got == want, (got, want)
  for key in ('params_flat', 'velocity', 'adam_v', 'state_flat'):
    assert torch.equal(getattr(a.engine.arena, key), getattr(b.engine.arena, key)), key
