"""JPEG decode of a crop window without a device (automl_amd/jpeg.py on csrc/jpeg_host.cpp's
edet_jpeg_entropy_decode_window): the numpy restatement tests/jpeg_window_ref.py -- kept grid, kept-grid coefficient order,
windowed colour stage -- equals the fixtures' pixels cropped, at ratio 1 (tests/golden/jpeg_cases.npz) and at 2, 4 and 8
(jpeg_scaled_cases.npz), for a fixed set of windows per stream; the host stage equals the restatement in every descriptor field
and every kept coefficient at 1 and 16 threads; window_grid's block count is the descriptor's; worst_window_blocks is never
exceeded over an enumeration of every window in small images; parsing stops behind the last kept MCU row; every new status and
refused argument is reached; a stand-alone program runs the entry point under the address and undefined-behaviour sanitizers.
Everything is array_equal: there is no tolerance anywhere."""
import collections
import os
import subprocess

import numpy as np
import pytest

from automl_amd import _lib, jpeg
from tests import jpeg_ref as jr
from tests import jpeg_window_ref as jw
from tests.test_jpeg import _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
SCALED = os.path.join(ROOT, 'tests', 'golden', 'jpeg_scaled_cases.npz')
RATIOS = (1, 2, 4, 8)
FAMILIES = ('s1x1_', 's8x9_', 's17x33_')
NAMED = ('s37x53_444_q75', 's37x53_422_q75', 's37x53_420_q75', 'grey_19x13_q90', 'restart_24x280_420', 'segments_17x33_422')


def load_streams():
  """name -> (bytes, {ratio: the fixture's pixels}) for the streams of the window tests."""
  g, s = np.load(GOLDEN), np.load(SCALED)
  names = [str(n) for n in g['names'] if str(n).startswith(FAMILIES) or str(n) in NAMED]
  out = collections.OrderedDict()
  for n in sorted(names):
    pixels = {1: g[n + '/rgb']}
    for r in (2, 4, 8):
      pixels[r] = s['%s/r%d' % (n, r)]
    out[n] = (g[n + '/bytes'].tobytes(), pixels)
  return out


@pytest.fixture(scope='module')
def streams():
  out = load_streams()
  assert set(NAMED) <= set(out) and len(out) == 9 + len(NAMED), sorted(out)
  return out


@pytest.fixture(scope='module')
def restated(streams):
  """(name, ratio, window) -> jpeg_window_ref.parse, computed once for every case of the window set."""
  out = collections.OrderedDict()
  for name, (data, pixels) in streams.items():
    for ratio in RATIOS:
      oh, ow = pixels[ratio].shape[:2]
      for win in jw.windows_for(oh, ow):
        out[(name, ratio, win)] = jw.parse(data, win, ratio)
  return out


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


def test_the_window_set():
  wins = jw.windows_for(37, 53)
  assert wins[0] == (0, 0, 37, 53) and (0, 0, 1, 1) in wins and (36, 52, 1, 1) in wins and (36, 0, 1, 53) in wins
  assert (0, 52, 37, 1) in wins and (1, 1, 5, 7) in wins and (0, 7, 37, 2) in wins and (0, 15, 37, 2) in wins
  assert (7, 0, 2, 53) in wins and (15, 0, 2, 53) in wins and (2, 2, 33, 49) in wins and (3, 3, 32, 48) in wins
  assert len(wins) == len(set(wins)) == 13
  assert jw.windows_for(1, 1) == [(0, 0, 1, 1)]
  for oh, ow in ((1, 2), (3, 35), (5, 7), (19, 13)):
    for y, x, h, w in jw.windows_for(oh, ow):
      assert 0 <= y and 0 <= x and h >= 1 and w >= 1 and y + h <= oh and x + w <= ow


def test_restatement_equals_the_cropped_fixture_pixels(streams, restated):
  seen = set()
  for (name, ratio, win), parsed in restated.items():
    y, x, h, w = win
    got = jw.color(parsed)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3), (name, ratio, win)
    assert np.array_equal(got, streams[name][1][ratio][y:y + h, x:x + w]), (name, ratio, win)
    my0, mx0, kh, kw = parsed.grid
    seen.add((my0 > 0, mx0 > 0))
  assert seen == {(False, False), (False, True), (True, False), (True, True)}      # kept grids that start inside the image


def test_kept_grid_known_answers(streams):
  fr = jr.info(streams['s37x53_420_q75'][0])      # 3 x 4 MCUs of 16 x 16
  assert jw.kept_grid(fr, (0, 0, 37, 53), 1) == (0, 0, 3, 4)
  assert jw.kept_grid(fr, (0, 0, 1, 1), 1) == (0, 0, 1, 1)
  assert jw.kept_grid(fr, (0, 14, 1, 1), 1) == (0, 0, 1, 2)      # chroma column 7 reads column 8: the guard crosses the seam
  assert jw.kept_grid(fr, (0, 13, 1, 1), 1) == (0, 0, 1, 1)      # chroma column 6 reads 5 .. 7
  assert jw.kept_grid(fr, (0, 16, 1, 1), 1) == (0, 0, 1, 2)      # chroma column 8 reads column 7
  assert jw.kept_grid(fr, (0, 18, 1, 1), 1) == (0, 1, 1, 1)
  assert jw.kept_grid(fr, (18, 18, 1, 1), 1) == (1, 1, 1, 1) and jw.kept_grid(fr, (17, 18, 1, 1), 1) == (0, 1, 2, 1)
  assert jw.kept_grid(fr, (36, 52, 1, 1), 1) == (2, 3, 1, 1)
  # at 1/2 the chroma of a 4:2:0 file needs no up-sampling: an MCU is 8 x 8 output pixels and there is no guard
  assert jw.kept_grid(fr, (0, 7, 1, 1), 2) == (0, 0, 1, 1) and jw.kept_grid(fr, (0, 8, 1, 1), 2) == (0, 1, 1, 1)
  fr = jr.info(streams['s37x53_422_q75'][0])      # 5 x 4 MCUs of 8 rows x 16 columns
  assert jw.kept_grid(fr, (0, 0, 37, 53), 1) == (0, 0, 5, 4) and jw.kept_grid(fr, (7, 14, 2, 1), 1) == (0, 0, 2, 2)
  assert jw.kept_grid(fr, (0, 6, 1, 1), 2) == (0, 0, 1, 2)       # 8 output columns per MCU, chroma column 3 reads column 4
  fr = jr.info(streams['grey_19x13_q90'][0])
  assert jw.kept_grid(fr, (8, 7, 2, 2), 1) == (1, 0, 1, 2) and jw.kept_grid(fr, (1, 0, 1, 1), 8) == (1, 0, 1, 1)


def _decode_host(datas, canvas, windows, ratios=None, max_ratio=8, threads=1, capacity=64 * 4096):
  n = len(datas)
  coef = np.full(capacity, 0x5A5A, np.int16)
  images = np.zeros(n * jpeg.IMAGE_BYTES, np.uint8)
  wins = np.full(n * jpeg.WINDOW_BYTES, 0xEE, np.uint8)
  qt = np.full((n, 4, 64), 0xFFFF, np.uint16)
  status = np.full(n, -1, np.int32)
  jpeg.entropy_decode_window(datas, canvas[0], canvas[1], max_ratio, ratios, windows, coef, images, wins, qt, status, threads)
  return coef, jpeg.descriptors(images, n), jpeg.window_descriptors(wins, n), qt, status


def test_host_stage_equals_the_restatement(streams, restated, lib):
  """Every case of the window set, in batches of one stream's windows at one ratio: every field of both descriptors, every
  kept coefficient and nothing behind them, identical at 1 and 16 threads; window_grid's count is total_blocks."""
  batches = collections.OrderedDict()
  for key in restated:
    batches.setdefault(key[:2], []).append(key[2])
  for (name, ratio), wins in batches.items():
    data = streams[name][0]
    info = jpeg.jpeg_info(data)
    canvas = streams[name][1][ratio].shape[:2]
    datas, ratios = [data] * len(wins), [ratio] * len(wins)
    coef, desc, wdesc, qt, status = _decode_host(datas, canvas, wins, ratios, threads=1)
    at = 0
    for i, win in enumerate(wins):
      want = restated[(name, ratio, win)]
      d, w = desc[i], wdesc[i]
      nc = len(want.coefs)
      where = (name, ratio, win)
      assert status[i] == 0 and d.status == 0 and d.reserved == ratio, where
      assert (w.y, w.x, w.h, w.w) == win and (w.image_h, w.image_w) == canvas and tuple(w.reserved) == (0, 0), where
      assert (w.mcu_y0, w.mcu_x0, w.mcus_h, w.mcus_w) == want.grid, where
      assert (d.height, d.width) == (want.kept_height, want.kept_width), where
      assert (d.components, d.h_max, d.v_max) == (nc, want.h_max, want.v_max), where
      assert list(d.blocks_w[:nc]) == want.blocks_w and list(d.blocks_h[:nc]) == want.blocks_h, where
      assert list(d.quant_id[:nc]) == list(want.frame.quant_id[:nc]) and np.array_equal(qt[i], want.qtables), where
      for c in range(nc):
        assert d.first_block[c] == at, where
        n = want.coefs[c].size
        assert np.array_equal(coef[64 * at:64 * at + n], want.coefs[c].reshape(-1)), where + (c,)
        at += n // 64
      assert d.total_blocks == sum(c.size // 64 for c in want.coefs), where
      assert jpeg.window_grid(info, win, ratio) == (want.grid, d.total_blocks), where
      if win == wins[0]:      # the whole image keeps the whole grid: the scaled stage's descriptor and coefficients
        full = jr.parse(data)
        assert list(d.blocks_w[:nc]) == full.blocks_w and (d.height, d.width) == canvas, where
        assert all(np.array_equal(a, b) for a, b in zip(want.coefs, full.coefs)), where
    assert (coef[64 * at:] == 0x5A5A).all(), (name, ratio)      # nothing is written behind the last kept block
    coef_t, desc_t, wdesc_t, qt_t, status_t = _decode_host(datas, canvas, wins, ratios, threads=16)
    assert np.array_equal(coef_t, coef) and np.array_equal(qt_t, qt) and np.array_equal(status_t, status), (name, ratio)
    assert [bytes(a) for a in desc_t] == [bytes(a) for a in desc] and [bytes(a) for a in wdesc_t] == [bytes(a) for a in wdesc]


Info = collections.namedtuple('Info', 'height width components h_samp v_samp')


def test_worst_window_blocks_is_never_exceeded():
  """Every window of up to ch x cw output pixels in every image of up to 40 x 40 (sizes around the MCU seams), greyscale and
  the three samplings, ratios 1 and 2, three small canvases: the kept blocks stay within worst_window_blocks(ch, cw,
  max_ratio=ratio), and at ratio 1 reach at least half of it somewhere (the bound is not idle)."""
  samplings = ((1, (1,), (1,)), (3, (1, 1, 1), (1, 1, 1)), (3, (2, 1, 1), (1, 1, 1)), (3, (2, 1, 1), (2, 1, 1)))
  sides = (1, 7, 16, 17, 33, 40)
  for ch, cw in ((1, 1), (3, 9), (8, 5)):
    for ratio in (1, 2):
      bound = jpeg.worst_window_blocks(ch, cw, max_ratio=ratio)
      assert bound >= jpeg.worst_window_blocks(ch, cw)      # (more ratios, never fewer blocks)
      most = 0
      for nc, hs, vs in samplings:
        for height in sides:
          for width in sides:
            info = Info(height, width, nc, hs, vs)
            oh, ow = jpeg.scaled_size(height, width, ratio)
            # the count depends on the window's two spans alone: enumerate them per axis, and take the products
            rows = {(y, h): None for h in range(1, min(ch, oh) + 1) for y in range(oh - h + 1)}
            cols = {(x, w): None for w in range(1, min(cw, ow) + 1) for x in range(ow - w + 1)}
            per = hs[0] * vs[0] + 2 if nc == 3 else 1
            tall = max(jpeg.window_grid(info, (y, 0, h, 1), ratio)[0][2] for y, h in rows)
            wide = max(jpeg.window_grid(info, (0, x, 1, w), ratio)[0][3] for x, w in cols)
            most = max(most, per * tall * wide)
            # ... which is what a window with both worst spans keeps
            y, h = max(rows, key=lambda s: jpeg.window_grid(info, (s[0], 0, s[1], 1), ratio)[0][2])
            x, w = max(cols, key=lambda s: jpeg.window_grid(info, (0, s[0], 1, s[1]), ratio)[0][3])
            grid, blocks = jpeg.window_grid(info, (y, x, h, w), ratio)
            assert blocks == per * tall * wide == per * grid[2] * grid[3], (info, ratio, (y, x, h, w))
      assert most <= bound and (ratio > 1 or most >= bound // 2), (ch, cw, ratio, most, bound)
  assert jpeg.worst_window_blocks(480, 640) >= jpeg.worst_blocks(480, 640)
  with pytest.raises(ValueError, match='max_ratio'):
    jpeg.worst_window_blocks(8, 8, 3)


def test_parsing_stops_behind_the_last_kept_mcu_row(streams, lib):
  """s37x53_420_q75 has three MCU rows.  Cut the file at the restatement's `end` for a window in the first two -- the first
  byte the window decode has not read a bit of -- and put an EOI marker and noise there: the whole-image stages call that
  MALFORMED, the window decode gives the intact stream's descriptors and coefficients.  The same cut one MCU row earlier is
  inside the kept rows: MALFORMED."""
  data = streams['s37x53_420_q75'][0]
  win = (3, 5, 20, 30)      # rows 3 .. 22: luma rows of MCU rows 0 and 1, chroma rows 0 .. 12 of 19
  intact = jw.parse(data, win, 1)
  assert intact.grid == (0, 0, 2, 3) and intact.end < len(data) - 2
  earlier = jw.parse(data, (3, 5, 4, 30), 1)
  assert earlier.grid == (0, 0, 1, 3) and earlier.end < intact.end
  damaged = data[:intact.end] + b'\xff\xd9' + bytes(range(7, 47))
  canvas = (37, 53)
  coef, desc, wdesc, qt, status = _decode_host([data, damaged], canvas, [win, win])
  assert list(status) == [0, 0]
  n = 64 * desc[0].total_blocks
  assert np.array_equal(coef[:n], coef[n:2 * n]) and desc[1].first_block[0] == desc[0].total_blocks
  assert np.array_equal(coef[:n], np.concatenate([c.reshape(-1) for c in intact.coefs]))
  assert bytes(wdesc[0]) == bytes(wdesc[1]) and np.array_equal(qt[0], qt[1])
  assert np.array_equal(jw.color(jw.parse(damaged, win, 1)), streams['s37x53_420_q75'][1][1][3:23, 5:35])
  # the whole-image window of the damaged stream, and the scaled entry point, read on and refuse it
  assert _decode_host([damaged], canvas, [(0, 0, 37, 53)])[4][0] == jpeg.MALFORMED
  images, st = np.zeros(jpeg.IMAGE_BYTES, np.uint8), np.zeros(1, np.int32)
  jpeg.entropy_decode_scaled([damaged], 37, 53, 8, None, np.zeros(64 * 4096, np.int16), images, np.zeros((1, 4, 64), np.uint16), st)
  assert st[0] == jpeg.MALFORMED
  inside = data[:earlier.end] + b'\xff\xd9' + bytes(range(7, 47))
  coef, desc, wdesc, qt, status = _decode_host([inside], canvas, [win])
  assert status[0] == jpeg.MALFORMED and desc[0].total_blocks == 0 and not any(bytes(wdesc[0])) and not qt[0].any()
  assert _decode_host([inside], canvas, [(3, 5, 4, 30)])[4][0] == 0      # ... and is behind the first row's end


def test_statuses_and_refused_arguments(streams, lib):
  data = streams['s17x33_420_q75'][0]
  small = streams['s8x9_444_q75'][0]
  ok = (2, 3, 9, 11)
  # a window outside the output image, or with a side below 1: WINDOW, at the ratio's own size
  for win in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, 18, 4), (0, 0, 4, 34), (16, 32, 2, 1), (17, 0, 1, 1)):
    coef, desc, wdesc, qt, status = _decode_host([data], (32, 40), [win])
    assert status[0] == jpeg.WINDOW == 9 == desc[0].status and desc[0].total_blocks == 0 and not any(bytes(wdesc[0])), win
    assert (coef == 0x5A5A).all() and not qt[0].any()
  assert _decode_host([data], (32, 40), [(0, 0, 9, 17)], ratios=[2])[4][0] == 0      # 17 x 33 at 1/2 is 9 x 17
  assert _decode_host([data], (32, 40), [(0, 0, 10, 17)], ratios=[2])[4][0] == jpeg.WINDOW
  assert _decode_host([data], (32, 40), [(0, 0, 3, 5)], ratios=[8])[4][0] == 0
  assert _decode_host([data], (32, 40), [(0, 0, 3, 6)], ratios=[8])[4][0] == jpeg.WINDOW
  # TOO_LARGE by the canvas: the window, not the image, has to fit it
  assert _decode_host([data], (9, 11), [ok])[4][0] == 0
  assert _decode_host([data], (8, 11), [ok])[4][0] == jpeg.TOO_LARGE and _decode_host([data], (9, 10), [ok])[4][0] == jpeg.TOO_LARGE
  # TOO_LARGE by the arena: the second window no longer fits, the small image behind it does and is intact
  blocks = jpeg.window_grid(jpeg.jpeg_info(data), ok, 1)[1]
  few = jpeg.window_grid(jpeg.jpeg_info(small), (0, 0, 8, 8), 1)[1]      # the first of its two MCUs
  coef, desc, wdesc, qt, status = _decode_host([data, data, small], (9, 11), [ok, ok, (0, 0, 8, 8)], capacity=64 * (2 * blocks - 1))
  assert list(status) == [0, jpeg.TOO_LARGE, 0] and desc[1].total_blocks == 0 and not any(bytes(wdesc[1]))
  assert (blocks, few) == (6, 3) and desc[2].first_block[0] == blocks and desc[2].total_blocks == few
  assert np.array_equal(coef[64 * blocks:64 * (blocks + few)], np.concatenate([c[:, :1].reshape(-1) for c in jr.parse(small).coefs]))
  assert (coef[64 * (blocks + few):] == 0x5A5A).all()
  # refused streams keep their statuses; a header that cannot be read leaves nothing to check a window against
  g = np.load(GOLDEN)
  for n in g['refused']:
    want = int(g[str(n) + '/status'])
    assert _decode_host([g[str(n) + '/bytes'].tobytes()], (64, 64), [(0, 0, 1, 1)])[4][0] == want, n
  assert _decode_host([b'junk'], (64, 64), [(0, 0, 1, 1)])[4][0] == jpeg.MALFORMED
  # the call itself fails for what the scaled call fails for, and for null windows
  for bad in (0, 3, 16):
    with pytest.raises(_lib.EdetError, match='max_denom'):
      _decode_host([data], (32, 40), [ok], max_ratio=bad)
    with pytest.raises(_lib.EdetError, match=r'denoms\[1\]'):
      _decode_host([data, data], (32, 40), [ok, ok], ratios=[1, bad])
  with pytest.raises(_lib.EdetError, match='null windows'):
    _decode_host([data], (32, 40), None)
  with pytest.raises(ValueError, match='windows must be'):
    _decode_host([data, data], (32, 40), [ok])
  with pytest.raises(ValueError, match='ratios'):
    _decode_host([data, data], (32, 40), [ok, ok], ratios=[1])
  # Python's refusals
  info = jpeg.jpeg_info(data)
  for win in ((0, 0, 18, 4), (0, 0, 0, 1), (-1, 0, 1, 1)):
    with pytest.raises(ValueError, match='crop window'):
      jpeg.window_grid(info, win)
  with pytest.raises(ValueError, match='ratio'):
    jpeg.window_grid(info, ok, 3)
  with pytest.raises(ValueError, match='crop_window'):
    jpeg.decode_and_crop_jpeg(data, (0, 0, 4))
  with pytest.raises(ValueError, match='crop window'):
    jpeg.decode_and_crop_jpeg(data, (0, 0, 18, 4))
  with pytest.raises(ValueError, match='ratio'):
    jpeg.decode_and_crop_jpeg(data, ok, ratio=3)
  with pytest.raises(ValueError, match='channels'):
    jpeg.decode_and_crop_jpeg(data, ok, channels=1)


def test_choose_window_ratio_and_jpeg_sizes(streams):
  """Hand-computed: the covering output window is y' = y // r, h' = ceil((y + h) / r) - y'."""
  f = jpeg.choose_window_ratio
  assert f((10, 20, 100, 200), 480, 640, 100, 200, 8) == (1, (10, 20, 100, 200))
  assert f((10, 20, 100, 200), 480, 640, 99, 200, 8) == (2, (5, 10, 50, 100))
  assert f((11, 21, 100, 200), 480, 640, 50, 100, 8) == (4, (2, 5, 26, 51))      # odd starts: (11 + 100 + 1) // 2 - 5 = 51 > 50
  assert f((11, 21, 100, 200), 480, 640, 51, 101, 8) == (2, (5, 10, 51, 101))
  assert f((0, 0, 480, 640), 480, 640, 60, 80, 8) == (8, (0, 0, 60, 80))
  assert f((7, 7, 473, 633), 480, 640, 60, 80, 8) == (8, (0, 0, 60, 80))
  assert f((0, 0, 480, 640), 480, 640, 59, 80, 8) is None and f((0, 0, 480, 640), 480, 640, 60, 80, 4) is None      # none fits
  assert f((479, 639, 1, 1), 480, 640, 1, 1, 1) == (1, (479, 639, 1, 1))
  assert f((3, 0, 2, 2), 8, 8, 1, 1, 8) == (8, (0, 0, 1, 1))      # rows 3 .. 4 straddle a pair at 1/2 and a group of four at 1/4
  assert f((4, 0, 2, 2), 8, 8, 1, 1, 8) == (2, (2, 0, 1, 1)) and f((4, 0, 2, 2), 8, 8, 1, 1, 1) is None
  for bad in ((0, 0, 0, 1), (-1, 0, 1, 1), (0, 0, 481, 1)):
    with pytest.raises(ValueError, match='crop window'):
      f(bad, 480, 640, 10, 10, 8)
  with pytest.raises(ValueError, match='max_ratio'):
    f((0, 0, 1, 1), 480, 640, 10, 10, 3)
  sizes = jpeg.jpeg_sizes([streams['s17x33_420_q75'][0], b'junk', streams['grey_19x13_q90'][0], b''])
  assert sizes.dtype == np.int32 and sizes.tolist() == [[17, 33], [0, 0], [19, 13], [0, 0]]


def test_host_stage_under_sanitizers(streams, tmp_path):
  """tests/c_host/jpeg_window_host_check.cpp + csrc/jpeg_host.cpp, built with -fsanitize=address,undefined and run as a child
  process: a sweep of windows that includes invalid ones at every ratio, each valid one again into an arena of exactly its kept
  blocks, every prefix of two streams and 300 single-byte corruptions of each.  Skips only where the host compiler cannot
  build a trivial sanitized program."""
  cxx = _cxx()
  flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-pthread']
  trivial = tmp_path / 'trivial.cpp'
  trivial.write_text('int main() { return 0; }\n')
  if cxx is None or subprocess.run([cxx] + flags + [str(trivial), '-o', str(tmp_path / 'trivial')],
                                   capture_output=True).returncode != 0 or \
      subprocess.run([str(tmp_path / 'trivial')], capture_output=True).returncode != 0:
    pytest.skip('the host compiler cannot build a sanitized program')
  exe = str(tmp_path / 'jpeg_window_host_check')
  r = subprocess.run([cxx] + flags + ['-Wall', '-Wextra', os.path.join(ROOT, 'tests', 'c_host', 'jpeg_window_host_check.cpp'),
                                      os.path.join(ROOT, 'automl_amd', 'csrc', 'jpeg_host.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  files = []
  for name in ('s17x33_420_q75', 's37x53_422_q75'):
    (tmp_path / (name + '.jpg')).write_bytes(streams[name][0])
    files.append(str(tmp_path / (name + '.jpg')))
  r = subprocess.run([exe] + files, capture_output=True, text=True, errors='replace', timeout=600)
  assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
  assert '17 x 33' in r.stdout and '37 x 53' in r.stdout and ' 0 failures' in r.stdout, r.stdout
