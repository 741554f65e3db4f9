"""The device entropy decoder without a device (automl_amd/jpeg.py: JpegDecoder(entropy='device'); csrc/jpeg_host.cpp:
edet_jpeg_scan_prepare; csrc/jpeg_entropy_impl.h).  The restatement tests/jpeg_entropy_ref.py -- segments, units, rounds,
prefix sums, DC sums -- equals the SERIAL parse tests/jpeg_ref.py on every decodable fixture at three subsequence sizes; the
host entry point equals the restatement's segments, unit counts, descriptors and statuses, and the host stage's image
descriptors and quantisation tables, whatever the thread count; what is to be refused is refused on the host; the argument
errors raise; and a stand-alone program runs the host entry point and a sequential emulation of the kernel's workgroup over
the fixtures, every prefix of two of them and a few hundred single-byte corruptions under the address and
undefined-behaviour sanitizers, against the host stage.  Everything is array_equal: there is no tolerance anywhere."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from automl_amd import _lib, jpeg
from tests import jpeg_entropy_ref as er
from tests import jpeg_ref as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
CANVAS = (480, 640)
SIZES = (64, 128, 1024)


@pytest.fixture(scope='module')
def cases():
  g = np.load(GOLDEN)
  ok = {str(n): g[str(n) + '/bytes'].tobytes() for n in g['names']}
  refused = {str(n): (g[str(n) + '/bytes'].tobytes(), int(g[str(n) + '/status'])) for n in g['refused']}
  return ok, refused


@pytest.fixture(scope='module')
def parsed(cases):
  """The serial parse of every decodable case, computed once."""
  return {name: jr.parse(data) for name, data in cases[0].items()}


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


def test_restatement_equals_the_serial_parse(cases, parsed):
  """It has to beat jpeg_ref.parse, not itself: every coefficient of all 39 streams at 64, 128 and 1024 bits; the rounds
  never exceed the units; the noisy quality-100 pictures need hundreds of rounds at 64 bits and still come out right."""
  ok, refused = cases
  assert len(ok) == 39
  most = {}
  for name, data in ok.items():
    want = parsed[name]
    for bits in SIZES:
      prep = er.prepare(data, subseq_bits=bits)
      status, coefs, rounds = er.decode(prep, bits)
      assert status == jr.OK and 1 <= rounds <= max(prep.units, 1), (name, bits)
      assert len(coefs) == len(want.coefs), (name, bits)
      for c, coef in enumerate(coefs):
        assert coef.dtype == np.int16 and np.array_equal(coef, want.coefs[c]), (name, bits, c)
      most[bits] = max(most.get(bits, 0), rounds)
      if name == 'restart_24x280_420':
        assert len(prep.segments) == 18 and prep.ri == 2
      if name == 's37x53_444_q100' and bits == 64:
        assert prep.units > 256 and rounds > 100, (prep.units, rounds)      # more units than a workgroup has threads
  assert most[64] >= most[128] >= most[1024] >= 2, most
  for name, (data, status) in refused.items():
    for bits in (64, 1024):
      assert er.status_of(data, subseq_bits=bits) == status == jr.status_of(data), (name, bits)


def _arrays(n, capacity, scan_bytes, segments):
  return dict(scan=np.full(scan_bytes, 0xA5, np.uint8), segments=np.full(segments * jpeg.SEGMENT_BYTES, 0xA5, np.uint8),
              tables=np.full(n * jpeg.TABLES * jpeg.TABLE_BYTES, 0xA5, np.uint8), scans=np.full(n * jpeg.SCAN_BYTES, 0xA5, np.uint8),
              images=np.full(n * jpeg.IMAGE_BYTES, 0xA5, np.uint8), qt=np.full((n, 4, 64), 0xFFFF, np.uint16),
              status=np.full(n, -1, np.int32), capacity=capacity)


def _prepare(datas, bits=1024, canvas=CANVAS, threads=0, capacity=None, scan_bytes=1 << 20, segments=4096, units=1 << 20):
  n = len(datas)
  a = _arrays(n, n * jpeg.worst_blocks(*canvas) * 64 if capacity is None else capacity, scan_bytes, segments)
  a['used'] = jpeg.scan_prepare(datas, canvas[0], canvas[1], 1, None, a['capacity'], bits, a['scan'], a['segments'], units,
                                a['tables'], a['scans'], a['images'], a['qt'], a['status'], threads)
  return a


def _decode_host(datas, canvas=CANVAS, capacity=None):
  n = len(datas)
  capacity = n * jpeg.worst_blocks(*canvas) * 64 if capacity is None else capacity
  coef = np.zeros(capacity, np.int16)
  images = np.zeros(n * jpeg.IMAGE_BYTES, np.uint8)
  qt = np.full((n, 4, 64), 0xFFFF, np.uint16)
  status = np.full(n, -1, np.int32)
  jpeg.entropy_decode(datas, canvas[0], canvas[1], coef, images, qt, status, 1)
  return images, qt, status


def test_scan_prepare_equals_the_restatement(cases, lib):
  """All 43 streams, the refused ones in between, as ONE batch: every segment's bytes, place and first unit, the unit counts,
  the scan descriptors and the statuses are the restatement's; the image descriptors and quantisation tables are
  edet_jpeg_entropy_decode's byte for byte -- but for the one stream that is damaged inside its scan, which the host stage
  refuses and this entry point cannot; 1, 3 and 16 threads give the same bytes."""
  ok, refused = cases
  names = sorted(ok)
  order = names[:5] + ['truncated_17x33'] + names[5:20] + ['progressive_17x33', 'huffman_17x33'] + names[20:] + ['cmyk_16x16']
  datas = [ok[n] if n in ok else refused[n][0] for n in order]
  assert len(datas) == 43
  images_h, qt_h, status_h = _decode_host(datas)
  desc_h = jpeg.descriptors(images_h, len(datas))
  for bits in SIZES:
    a = _prepare(datas, bits, threads=1)
    scans, desc = jpeg.scan_descriptors(a['scans'], len(datas)), jpeg.descriptors(a['images'], len(datas))
    rows = jpeg.segment_rows(a['segments'], a['used'][1])
    next_seg = next_unit = next_byte = 0
    for i, name in enumerate(order):
      sc, d = scans[i], desc[i]
      if name in refused and name != 'truncated_17x33':
        assert a['status'][i] == d.status == refused[name][1] == status_h[i], name
        assert bytes(sc) == bytes(jpeg.SCAN_BYTES) and bytes(d) == bytes(desc_h[i]) and not a['qt'][i].any(), name
        assert not a['tables'].reshape(len(datas), -1)[i].any(), name
        continue
      want = er.prepare(datas[i], subseq_bits=bits)
      assert a['status'][i] == d.status == 0, name
      if name == 'truncated_17x33':      # found on the device only: here it has the descriptor of a sound file
        assert status_h[i] == jpeg.MALFORMED and er.decode(want, bits)[0] == jpeg.MALFORMED
        assert (d.height, d.width, d.total_blocks) == (17, 33, desc[order.index('s17x33_420_q75')].total_blocks)
      else:
        assert status_h[i] == 0 and bytes(d) == bytes(desc_h[i]) and np.array_equal(a['qt'][i], qt_h[i]), name
      assert (sc.status, sc.rounds, sc.first_segment, sc.segments) == (0, 0, next_seg, len(want.segments)), name
      assert (sc.first_unit, sc.units, sc.restart_interval) == (next_unit, want.units, want.ri), name
      assert (sc.mcus_w, sc.mcus_h, sc.blocks_per_mcu) == (want.mcus_w, want.mcus_h, want.blocks_per_mcu), name
      nc = want.frame.components
      assert list(sc.dc_table[:nc]) == want.dc_slot and list(sc.ac_table[:nc]) == want.ac_slot, name
      assert rows[next_seg].offset == next_byte, name      # an image's room starts where the room in front of it ends
      for j, seg in enumerate(want.segments):
        row = rows[next_seg + j]
        assert (row.length, row.first_unit, row.offset % 4) == (len(seg), want.first_unit[j], 0), (name, j)
        assert a['scan'][row.offset:row.offset + row.length].tobytes() == seg, (name, j)
        pad = -row.length % 4
        assert not a['scan'][row.offset + row.length:row.offset + row.length + pad].any(), (name, j)
        assert j == 0 or row.offset >= rows[next_seg + j - 1].offset + rows[next_seg + j - 1].length
      p = jr.walk(datas[i])[4]
      next_byte += (len(datas[i]) - p + 4 * len(want.segments) + 15) // 16 * 16
      assert rows[next_seg + len(want.segments) - 1].offset + len(want.segments[-1]) <= next_byte
      next_seg += len(want.segments)
      next_unit += want.units
    assert a['used'] == (next_byte, next_seg, next_unit), bits
    for threads in (3, 16):
      t = _prepare(datas, bits, threads=threads)
      assert t['used'] == a['used'], threads
      for key in ('segments', 'tables', 'scans', 'images', 'qt', 'status'):
        assert np.array_equal(t[key], a[key]), (threads, key)
      for row in rows:
        assert np.array_equal(t['scan'][row.offset:row.offset + row.length], a['scan'][row.offset:row.offset + row.length])
  # the same descriptors as the scaled host stage where a ratio is in play
  n = len(datas)
  b = _arrays(n, n * jpeg.worst_blocks(*CANVAS) * 64, 1 << 20, 4096)
  jpeg.scan_prepare(datas, 60, 80, 8, None, b['capacity'], 1024, b['scan'], b['segments'], 1 << 20, b['tables'], b['scans'],
                    b['images'], b['qt'], b['status'], 0)
  coef = np.zeros(b['capacity'], np.int16)
  images = np.zeros(n * jpeg.IMAGE_BYTES, np.uint8)
  qt = np.zeros((n, 4, 64), np.uint16)
  status = np.zeros(n, np.int32)
  jpeg.entropy_decode_scaled(datas, 60, 80, 8, None, coef, images, qt, status, 0)
  keep = [i for i, name in enumerate(order) if name != 'truncated_17x33']
  assert np.array_equal(b['images'].reshape(n, -1)[keep], images.reshape(n, -1)[keep])
  assert np.array_equal(b['status'][keep], status[keep]) and np.array_equal(b['qt'][keep], qt[keep])
  assert jpeg.descriptors(b['images'], n)[order.index('big_480x640_420')].reserved == 8


def test_scan_prepare_refuses(cases, lib):
  ok, refused = cases
  for name, (stream, status) in refused.items():
    got = _prepare([stream])['status'][0]
    assert got == (0 if name == 'truncated_17x33' else status), name
  data = ok['s37x53_420_q75']
  assert _prepare([data], canvas=(36, 64))['status'][0] == jpeg.TOO_LARGE
  blocks = sum(b.size // 64 for b in jr.parse(data).coefs)
  assert list(_prepare([data, data], canvas=(64, 64), capacity=64 * (2 * blocks - 1))['status']) == [jpeg.OK, jpeg.TOO_LARGE]
  # the arenas of the scan: bytes, segments, units -- each decided on the host, for the image that no longer fits
  one = _prepare([data], 64)
  room, units = one['used'][0], one['used'][2]
  assert list(_prepare([data, data], 64, scan_bytes=2 * room)['status']) == [0, 0]
  assert list(_prepare([data, data], 64, scan_bytes=2 * room - 16)['status']) == [0, jpeg.TOO_LARGE]
  assert list(_prepare([data, data], 64, units=2 * units)['status']) == [0, 0]
  short = _prepare([data, data], 64, units=2 * units - 1)
  assert list(short['status']) == [0, jpeg.TOO_LARGE] and short['used'][2] == units
  assert bytes(jpeg.scan_descriptors(short['scans'], 2)[1]) == bytes(jpeg.SCAN_BYTES)
  restart = ok['restart_24x280_420']
  assert list(_prepare([restart, restart], segments=36)['status']) == [0, 0]
  assert list(_prepare([restart, restart], segments=35)['status']) == [0, jpeg.TOO_LARGE]
  # restart markers: one out of sequence, one missing, one replaced by another marker -- MALFORMED on the host, as in the host stage
  marks = [i for i in range(jr.walk(restart)[4], len(restart) - 1) if restart[i] == 0xFF and 0xD0 <= restart[i + 1] <= 0xD7]
  assert len(marks) == 17 and [restart[i + 1] & 7 for i in marks] == [j & 7 for j in range(17)]
  for at, value in ((marks[3] + 1, 0xD5), (marks[9] + 1, 0xD0), (marks[0] + 1, 0xD9), (marks[16], 0x00)):
    bad = bytearray(restart)
    bad[at] = value
    got = _prepare([bytes(bad)])
    assert got['status'][0] == jpeg.MALFORMED == jr.status_of(bytes(bad)) == er.status_of(bytes(bad)), (at, value)
    assert not got['images'].reshape(1, -1)[0, 4:].any() and bytes(jpeg.scan_descriptors(got['scans'], 1)[0]) == bytes(jpeg.SCAN_BYTES)
  assert _prepare([restart[:marks[16]] + b'\xff\xff' + restart[marks[16]:]])['status'][0] == 0      # fill bytes are skipped
  assert _prepare([b''])['status'][0] == jpeg.MALFORMED
  for bits in (0, 32, 48, 100, 8224):
    with pytest.raises(_lib.EdetError):
      _prepare([data], bits)


def test_argument_errors(cases):
  ok, _ = cases
  data = ok['s16x16_420_q75']
  for kw in ({'entropy': 'gpu'}, {'entropy': None}, {'entropy': 'device', 'windowed': True}, {'subseq_bits': 32},
             {'subseq_bits': 100}, {'subseq_bits': 8224}, {'scan_bytes': 4096}, {'entropy': 'device', 'scan_bytes': 8},
             {'entropy': 'device', 'scan_bytes': 2 ** 31}):
    with pytest.raises(ValueError):
      jpeg.JpegDecoder(2, 16, 16, **kw)
  with pytest.raises(ValueError):
    jpeg.decode_jpeg(data, entropy='both')
  from automl_amd import dataloader
  with pytest.raises(ValueError):
    dataloader.InputReader('nothing-*.tfrecord', True, jpeg_entropy='gpu')
  import torch
  if not torch.cuda.is_available():      # the arguments are fine: what is missing is the device, and there is no fall-back
    with pytest.raises(_lib.EdetError):
      jpeg.JpegDecoder(2, 16, 16, entropy='device', subseq_bits=64)
  import ctypes
  assert (ctypes.sizeof(_lib.JpegScan), ctypes.sizeof(_lib.JpegSegment)) == (64, 16)
  header = open(os.path.join(ROOT, 'include', 'edet_hip.h')).read()
  assert '#define EDET_JPEG_TABLES %d ' % jpeg.TABLES in header and '#define EDET_JPEG_TABLE_BYTES %d ' % jpeg.TABLE_BYTES in header
  assert '#define EDET_JPEG_UNIT_WORDS %d ' % jpeg.UNIT_WORDS in header


def _cxx():
  return shutil.which('g++') or next((p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/bin/amdclang++') if os.path.exists(p)), None)


def test_workgroup_emulation_under_sanitizers(cases, tmp_path):
  """tests/c_host/jpeg_entropy_host_check.cpp + csrc/jpeg_host.cpp + csrc/jpeg_entropy_impl.h, built with
  -fsanitize=address,undefined and run as a child process: edet_jpeg_scan_prepare and a sequential emulation of the kernel's
  workgroup on every fixture stream at 64, 128 and 1024 bits, on every prefix of two small streams and on 300 single-byte
  corruptions of each at 64 and 1024 bits, against edet_jpeg_entropy_decode on the same bytes.  Skips only where the host
  compiler cannot build a trivial sanitized program."""
  ok, refused = cases
  cxx = _cxx()
  flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-pthread']
  trivial = tmp_path / 'trivial.cpp'
  trivial.write_text('int main() { return 0; }\n')
  if cxx is None or subprocess.run([cxx] + flags + [str(trivial), '-o', str(tmp_path / 'trivial')],
                                   capture_output=True).returncode != 0 or \
      subprocess.run([str(tmp_path / 'trivial')], capture_output=True).returncode != 0:
    pytest.skip('the host compiler cannot build a sanitized program')
  exe = str(tmp_path / 'jpeg_entropy_host_check')
  r = subprocess.run([cxx] + flags + ['-Wall', '-Wextra', os.path.join(ROOT, 'tests', 'c_host', 'jpeg_entropy_host_check.cpp'),
                                      os.path.join(ROOT, 'automl_amd', 'csrc', 'jpeg_host.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  mutated = ('s8x9_420_q75', 'restart_24x280_420')
  lines = []
  for k, (name, data) in enumerate(sorted(ok.items())):
    (tmp_path / ('ok%d.jpg' % k)).write_bytes(data)
    lines.append('ok%d.jpg 0 %d' % (k, name in mutated))
  for k, (name, (data, status)) in enumerate(sorted(refused.items())):
    (tmp_path / ('refused%d.jpg' % k)).write_bytes(data)
    lines.append('refused%d.jpg %d 0' % (k, status))
  (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
  r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, errors='replace', timeout=600)
  assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
  assert '43 streams' in r.stdout and ' 0 failures' in r.stdout, r.stdout
