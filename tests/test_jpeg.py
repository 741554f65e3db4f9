"""The JPEG decoder without a device (automl_amd/jpeg.py on csrc/jpeg_host.cpp): the numpy restatement tests/jpeg_ref.py
equals the pixels Pillow decoded from every case of tests/golden/jpeg_cases.npz (and from two files encoded here, where
Pillow is installed); the host stage -- called through ctypes on the built library, it needs no device -- equals the
restatement's header fields, quantisation tables and coefficients, whatever the thread count, and refuses what is to be
refused; the argument errors raise; and a stand-alone program runs the host stage over the fixture streams, every prefix of
two of them and a few hundred single-byte corruptions under the address and undefined-behaviour sanitizers.  Everything is
array_equal: there is no tolerance anywhere."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from automl_amd import _lib, jpeg
from tests import jpeg_ref as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
CANVAS = (480, 640)


@pytest.fixture(scope='module')
def cases():
  g = np.load(GOLDEN)
  ok = {str(n): (g[str(n) + '/bytes'].tobytes(), g[str(n) + '/rgb']) for n in g['names']}
  refused = {str(n): (g[str(n) + '/bytes'].tobytes(), int(g[str(n) + '/status'])) for n in g['refused']}
  return ok, refused


@pytest.fixture(scope='module')
def parsed(cases):
  """The restatement's host stage of every decodable case, computed once."""
  return {name: jr.parse(data) for name, (data, _) in cases[0].items()}


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


def test_fixture_holds_the_families(cases):
  ok, refused = cases
  for size in ('1x1', '8x9', '16x16', '17x33', '31x22', '37x53', '24x280'):
    for sub in ('444', '422', '420'):
      assert 's%s_%s_q75' % (size, sub) in ok
  for q in (30, 95, 100):
    assert 's37x53_420_q%d' % q in ok
  assert {'grey_16x16_q75', 'grey_19x13_q90', 'const_20x20_420', 'optimize_31x22_420', 'restart_24x280_420',
          'segments_17x33_422', 'big_480x640_420'} <= set(ok)
  assert set(refused) == {'progressive_17x33', 'cmyk_16x16', 'truncated_17x33', 'huffman_17x33'}
  assert jr.info(ok['restart_24x280_420'][0]).restart_interval == 2
  assert ok['big_480x640_420'][1].shape == (480, 640, 3)
  assert os.path.getsize(GOLDEN) < 600 * 1024


def test_restatement_equals_pillow_on_every_case(cases, parsed):
  ok, refused = cases
  for name, (data, rgb) in ok.items():
    got = jr.color(parsed[name])
    assert got.dtype == np.uint8 and np.array_equal(got, rgb), name
  for name, (data, status) in refused.items():
    assert jr.status_of(data) == status, name


def test_restatement_equals_pillow_on_a_live_encode():
  Image = pytest.importorskip('PIL.Image')
  rng = np.random.default_rng(5)
  for (h, w), sub, q in (((23, 41), 2, 60), ((40, 17), 1, 90)):
    img = np.clip(rng.normal(128, 60, (h, w, 3)), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img, 'RGB').save(buf, 'JPEG', quality=q, subsampling=sub)
    want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB'))
    assert np.array_equal(jr.decode(buf.getvalue()), want), (h, w, sub, q)


def test_upsampling_and_colour_known_answers():
  """jdsample.c / jdcolor.c by hand: the edge rules of the two upsamplers and the three colour equations."""
  row = np.array([[10, 20, 40]], np.uint8)
  assert jr.upsample_h2v1(row, 1, 6).tolist() == [[10, (30 + 20 + 2) >> 2, (60 + 10 + 1) >> 2, (60 + 40 + 2) >> 2,
                                                   (120 + 20 + 1) >> 2, 40]]
  assert jr.upsample_h2v1(row, 1, 5).tolist() == [[10, 13, 17, 25, 35]]
  two = np.array([[16, 32], [48, 64]], np.uint8)
  up = jr.upsample_h2v2(two, 4, 4)
  # row 0: near = far = chroma row 0 (clamped): colsum = 4 v; row 1: 3 row 0 + row 1
  assert up[0].tolist() == [(4 * 64 + 8) >> 4, (3 * 64 + 128 + 7) >> 4, (3 * 128 + 64 + 8) >> 4, (4 * 128 + 7) >> 4]
  assert up[1].tolist() == [(4 * 96 + 8) >> 4, (3 * 96 + 160 + 7) >> 4, (3 * 160 + 96 + 8) >> 4, (4 * 160 + 7) >> 4]
  assert up[3].tolist() == [(4 * 192 + 8) >> 4, (3 * 192 + 256 + 7) >> 4, (3 * 256 + 192 + 8) >> 4, (4 * 256 + 7) >> 4]
  # a DC-only block: coefficient x table = 8 v gives a flat block of v + 128
  coef = np.zeros((1, 64), np.int16)
  coef[0, 0] = 5
  assert (jr.idct_blocks(coef, np.full(64, 16, np.uint16)) == 138).all()


def _decode_host(datas, canvas=CANVAS, threads=0, capacity=None):
  n = len(datas)
  capacity = n * jpeg.worst_blocks(*canvas) * 64 if capacity is None else capacity
  coef = np.full(capacity, 0x5A5A, np.int16)
  images = np.zeros(n * jpeg.IMAGE_BYTES, np.uint8)
  qt = np.full((n, 4, 64), 0xFFFF, np.uint16)
  status = np.full(n, -1, np.int32)
  jpeg.entropy_decode(datas, canvas[0], canvas[1], coef, images, qt, status, threads)
  return coef, jpeg.descriptors(images, n), qt, status


def test_info_equals_the_restatement(cases, lib):
  ok, refused = cases
  assert jpeg.IMAGE_BYTES == 80 and __import__('ctypes').sizeof(_lib.JpegInfo) == 56
  for name, data in [(n, d) for n, (d, _) in ok.items()] + [(n, d) for n, (d, _) in refused.items()]:
    want = jr.info(data)
    got = jpeg.jpeg_info(data)
    k = min(want.components, 4)
    assert got.kind == jpeg.KINDS[want.kind], name
    assert (got.height, got.width, got.components, got.precision, got.restart_interval, got.sof) == \
        (want.height, want.width, want.components, want.precision, want.restart_interval, want.sof), name
    assert (got.h_samp, got.v_samp, got.quant_id, got.comp_id) == \
        (want.h_samp[:k], want.v_samp[:k], want.quant_id[:k], want.comp_id[:k]), name
    assert (got.jfif, got.adobe_transform) == (bool(want.jfif), want.adobe_transform), name
  assert jpeg.jpeg_info(refused['progressive_17x33'][0]).kind == 'progressive'
  assert jpeg.jpeg_info(refused['cmyk_16x16'][0]).components == 4
  for bad in (b'', b'\xff\xd8', b'not a jpeg at all', ok['s8x9_444_q75'][0][:30]):
    with pytest.raises(ValueError):
      jpeg.jpeg_info(bad)


def test_host_stage_equals_the_restatement(cases, parsed, lib):
  """All cases, the refused ones in between, as ONE batch: descriptors, tables and every coefficient; 1, 3 and 16 threads
  give the same bytes."""
  ok, refused = cases
  names = sorted(ok)
  order = names[:5] + ['truncated_17x33'] + names[5:20] + ['progressive_17x33', 'huffman_17x33'] + names[20:] + ['cmyk_16x16']
  datas = [ok[n][0] if n in ok else refused[n][0] for n in order]
  coef, desc, qt, status = _decode_host(datas, threads=1)
  at = 0
  for i, name in enumerate(order):
    d = desc[i]
    assert d.status == status[i]
    if name in refused:
      assert d.status == refused[name][1], name
      assert (d.height, d.width, d.components, d.total_blocks) == (0, 0, 0, 0) and not qt[i].any()
      if name != 'progressive_17x33' and name != 'cmyk_16x16':      # refused inside the scan: its place stays, unused
        at += sum(b.size // 64 for b in jr.parse(ok['s17x33_420_q75'][0]).coefs)
      continue
    want = parsed[name]
    nc = want.frame.components
    assert d.status == 0 and (d.height, d.width, d.components) == (want.frame.height, want.frame.width, nc), name
    assert (d.h_max, d.v_max) == (want.h_max, want.v_max), name
    assert list(d.blocks_w[:nc]) == want.blocks_w and list(d.blocks_h[:nc]) == want.blocks_h, name
    assert list(d.quant_id[:nc]) == list(want.frame.quant_id[:nc]), name
    assert np.array_equal(qt[i], want.qtables), name
    for c in range(nc):
      assert d.first_block[c] == at, (name, c)
      n = want.coefs[c].size
      assert np.array_equal(coef[64 * at:64 * at + n], want.coefs[c].reshape(-1)), (name, c)
      at += n // 64
    assert d.total_blocks == sum(b.size // 64 for b in want.coefs)
  assert (coef[64 * at:] == 0x5A5A).all()      # nothing is written behind the last block
  for threads in (3, 16):
    coef_t, desc_t, qt_t, status_t = _decode_host(datas, threads=threads)
    assert np.array_equal(coef_t, coef) and np.array_equal(qt_t, qt) and np.array_equal(status_t, status), threads
    assert [bytes(a) for a in desc_t] == [bytes(a) for a in desc], threads


def test_host_stage_refuses(cases, lib):
  ok, refused = cases
  data = ok['s37x53_420_q75'][0]
  # larger than the canvas, in either direction; no room left in the arena
  assert _decode_host([data], canvas=(36, 64))[3][0] == jpeg.TOO_LARGE
  assert _decode_host([data], canvas=(64, 52))[3][0] == jpeg.TOO_LARGE
  assert _decode_host([data], canvas=(37, 53))[3][0] == jpeg.OK
  blocks = sum(b.size // 64 for b in jr.parse(data).coefs)
  assert list(_decode_host([data, data], canvas=(64, 64), capacity=64 * (2 * blocks - 1))[3]) == [jpeg.OK, jpeg.TOO_LARGE]
  # hand-made headers: 12-bit, 4:1:1, 4:4:0, an arithmetic-coded frame, a lossless one, RGB by Adobe's marker, two scans
  sof = data.index(b'\xff\xc0')

  def patched(at, value):
    b = bytearray(data)
    b[at] = value
    return bytes(b)
  assert _decode_host([patched(sof + 4, 12)])[3][0] == jpeg.PRECISION
  assert _decode_host([patched(sof + 11, 0x41)])[3][0] == jpeg.SAMPLING
  assert _decode_host([patched(sof + 11, 0x12)])[3][0] == jpeg.SAMPLING
  assert _decode_host([patched(sof + 14, 0x22)])[3][0] == jpeg.SAMPLING
  assert _decode_host([patched(sof + 1, 0xC9)])[3][0] == jpeg.ARITHMETIC
  assert _decode_host([patched(sof + 1, 0xC3)])[3][0] == jpeg.UNSUPPORTED
  adobe = b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00'
  assert _decode_host([data[:2] + adobe + data[2:]])[3][0] == jpeg.UNSUPPORTED
  sos = data.index(b'\xff\xda')
  one_component = data[:sos] + b'\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00' + data[sos + 14:]
  assert _decode_host([one_component])[3][0] == jpeg.UNSUPPORTED
  unknown = bytearray(data)
  unknown[sos + 5] = 9      # a scan component the frame does not have
  assert _decode_host([bytes(unknown)])[3][0] == jpeg.MALFORMED
  for name, (stream, status) in refused.items():
    assert _decode_host([stream])[3][0] == status == jr.status_of(stream), name
  for stream in (patched(sof + 4, 12), patched(sof + 11, 0x41), patched(sof + 1, 0xC9), one_component, bytes(unknown)):
    assert _decode_host([stream])[3][0] == jr.status_of(stream)
  assert _decode_host([b''])[3][0] == jpeg.MALFORMED


def test_argument_errors(cases):
  ok, _ = cases
  data = ok['s16x16_420_q75'][0]
  with pytest.raises(ValueError):
    jpeg.decode_jpeg(data, channels=1)
  with pytest.raises(ValueError):
    jpeg.decode_jpeg(data, channels=4)
  with pytest.raises(ValueError):
    jpeg.decode_jpeg('a string')
  with pytest.raises(ValueError):
    jpeg.decode_jpeg(b'\xff\xd8\xff')
  for args in ((0, 16, 16), (2, 0, 16), (2, 16, 0), (70000, 16, 16), (2, 70000, 16), (1, 30000, 30000)):
    with pytest.raises(ValueError):
      jpeg.JpegDecoder(*args)
  for kw in ({'threads': 0}, {'threads': 17}, {'depth': 0}):
    with pytest.raises(ValueError):
      jpeg.JpegDecoder(2, 16, 16, **kw)
  import torch
  if not torch.cuda.is_available():      # the arguments are fine: what is missing is the device, and there is no fall-back
    with pytest.raises(_lib.EdetError):
      jpeg.JpegDecoder(2, 16, 16)
  assert jpeg.worst_blocks(8, 8) == 6 and jpeg.worst_blocks(16, 16) == 12 and jpeg.worst_blocks(16, 8) == 8 and \
      jpeg.worst_blocks(24, 24) == 27      # 4:2:0, 4:4:4 (one MCU), 4:2:2, 4:4:4


def _cxx():
  return shutil.which('g++') or next((p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/bin/amdclang++') if os.path.exists(p)), None)


def test_host_stage_under_sanitizers(cases, tmp_path):
  """tests/c_host/jpeg_host_check.cpp + csrc/jpeg_host.cpp, built with -fsanitize=address,undefined and run as a child
  process: every fixture stream alone and as a batch on 4 threads, every prefix of two small streams and 300 single-byte
  corruptions of each.  Skips only where the host compiler cannot build a trivial sanitized program."""
  ok, refused = cases
  cxx = _cxx()
  flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-pthread']
  trivial = tmp_path / 'trivial.cpp'
  trivial.write_text('int main() { return 0; }\n')
  if cxx is None or subprocess.run([cxx] + flags + [str(trivial), '-o', str(tmp_path / 'trivial')],
                                   capture_output=True).returncode != 0 or \
      subprocess.run([str(tmp_path / 'trivial')], capture_output=True).returncode != 0:
    pytest.skip('the host compiler cannot build a sanitized program')
  exe = str(tmp_path / 'jpeg_host_check')
  r = subprocess.run([cxx] + flags + ['-Wall', '-Wextra', os.path.join(ROOT, 'tests', 'c_host', 'jpeg_host_check.cpp'),
                                      os.path.join(ROOT, 'automl_amd', 'csrc', 'jpeg_host.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  mutated = ('s8x9_420_q75', 'restart_24x280_420')
  lines = []
  for k, (name, (data, _)) in enumerate(sorted(ok.items())):
    (tmp_path / ('ok%d.jpg' % k)).write_bytes(data)
    lines.append('ok%d.jpg 0 %d' % (k, name in mutated))
  for k, (name, (data, status)) in enumerate(sorted(refused.items())):
    (tmp_path / ('refused%d.jpg' % k)).write_bytes(data)
    lines.append('refused%d.jpg %d 0' % (k, status))
  (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
  r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, errors='replace', timeout=600)
  assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
  assert '0 failures' in r.stdout, r.stdout
