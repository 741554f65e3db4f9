"""JPEG decode at reduced size without a device (automl_amd/jpeg.py on csrc/jpeg_host.cpp's
edet_jpeg_entropy_decode_scaled): the numpy restatement tests/jpeg_scaled_ref.py equals every case of
tests/golden/jpeg_scaled_cases.npz (Pillow's draft-mode pixels); scaled_size / choose_ratio on exact fits and one pixel over;
the host entry point against the restatement -- chosen and forced denominators, output sizes, descriptors, statuses, and
coefficients equal to the full-size stage's -- identical at 1, 3 and 16 threads; an arena that runs out; the arguments the call
refuses; a stand-alone program under the address and undefined-behaviour sanitizers; and max_ratio / --jpeg_max_ratio reaching
the decoder through the ImageNet reader and the classifier's CLI.  Everything is array_equal: there is no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

from automl_amd import _lib, effnetv2_datasets as ds, effnetv2_main as main_lib, jpeg, tfrecord
from tests import jpeg_ref as jr
from tests import jpeg_scaled_ref as js
from tests import v2_datasets_ref as ref
from tests.test_jpeg import _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
SCALED = os.path.join(ROOT, 'tests', 'golden', 'jpeg_scaled_cases.npz')
RATIOS = (2, 4, 8)


@pytest.fixture(scope='module')
def cases():
  """name -> (bytes, {ratio: pixels}), the names Pillow has no answer for, and the refused streams."""
  g, s = np.load(GOLDEN), np.load(SCALED)
  streams = {str(n): g[str(n) + '/bytes'].tobytes() for n in s['names']}
  streams.update({str(n): s[str(n) + '/bytes'].tobytes() for n in s['new']})
  assert [int(r) for r in s['ratios']] == list(RATIOS)
  ok = {n: (d, {r: s['%s/r%d' % (n, r)] for r in RATIOS}) for n, d in streams.items()}
  refused = {str(n): (g[str(n) + '/bytes'].tobytes(), int(g[str(n) + '/status'])) for n in g['refused']}
  return ok, set(str(n) for n in s['restated']), refused


@pytest.fixture(scope='module')
def parsed(cases):
  return {name: jr.parse(data) for name, (data, _) in cases[0].items()}


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


def test_fixture_holds_the_families(cases):
  ok, restated, _ = cases
  for size in ('1x1', '8x9', '16x16', '17x33', '31x22', '37x53', '24x280'):
    for sub in ('444', '422', '420'):
      assert 's%s_%s_q75' % (size, sub) in ok
  assert {'grey_16x16_q75', 'grey_19x13_q90', 's16x16_422_q100', 's64x64_420_q75', 's37x53_420_q100'} <= set(ok)
  assert not any(n.startswith('big') for n in ok)
  # Pillow's draft mode has no answer only where the ratio exceeds the image's smaller side
  assert all(n.startswith('s1x1') or n.startswith('s8x9') for n in restated) and 's1x1_420_q75/r2' in restated
  assert os.path.getsize(SCALED) < os.path.getsize(GOLDEN) // 2


def test_restatement_equals_every_fixture_case(cases, parsed):
  ok, _, _ = cases
  for name, (data, pixels) in ok.items():
    fr = parsed[name].frame
    for ratio in RATIOS:
      got = js.color(parsed[name], ratio)
      assert got.dtype == np.uint8 and got.shape == js.scaled_size(fr.height, fr.width, ratio) + (3,), (name, ratio)
      assert np.array_equal(got, pixels[ratio]), (name, ratio)
    assert np.array_equal(js.color(parsed[name], 1), jr.color(parsed[name])), name      # (no fixture file is 2 .. 4 wide)


def test_sample_sizes_and_known_answers():
  """The table of the sample sizes, and the reduced transforms on a DC-only block: coefficient x table = 8 v gives a flat
  block of v + 128 at every size."""
  assert [js.sample_sizes(3, 1, 1, d) for d in (1, 2, 4, 8)] == [[8] * 3, [4] * 3, [2] * 3, [1] * 3]
  assert [js.sample_sizes(3, 2, 1, d) for d in (1, 2, 4, 8)] == [[8] * 3, [4] * 3, [2] * 3, [1] * 3]
  assert [js.sample_sizes(3, 2, 2, d) for d in (1, 2, 4, 8)] == [[8, 8, 8], [4, 8, 8], [2, 4, 4], [1, 2, 2]]
  assert [js.sample_sizes(1, 1, 1, d) for d in (1, 2, 4, 8)] == [[8], [4], [2], [1]]
  coef = np.zeros((1, 64), np.int16)
  coef[0, 0] = 5
  for s in (8, 4, 2, 1):
    out = js.idct_blocks(coef, np.full(64, 16, np.uint16), s)
    assert out.shape == (1, s, s) and (out == 138).all(), s
  # replication: every sample twice in a row, every row twice
  two = np.array([[16, 32], [48, 64]], np.uint8)
  assert js.replicate(two, 2, 3, 2, 1).tolist() == [[16, 16, 32], [48, 48, 64]]
  assert js.replicate(two, 3, 4, 2, 2).tolist() == [[16, 16, 32, 32], [16, 16, 32, 32], [48, 48, 64, 64]]


def test_scaled_size_and_choose_ratio():
  assert jpeg.scaled_size(480, 640, 1) == (480, 640) and jpeg.scaled_size(480, 640, 2) == (240, 320)
  assert jpeg.scaled_size(481, 641, 2) == (241, 321) and jpeg.scaled_size(481, 641, 8) == (61, 81)
  assert jpeg.scaled_size(1, 1, 8) == (1, 1) and jpeg.scaled_size(8, 9, 8) == (1, 2)
  assert jpeg.choose_ratio(480, 640, 480, 640, 8) == 1
  assert jpeg.choose_ratio(480, 640, 240, 320, 8) == 2      # an exact fit
  assert jpeg.choose_ratio(481, 641, 240, 320, 8) == 4      # one pixel over, in both directions and in each
  assert jpeg.choose_ratio(481, 640, 240, 320, 8) == 4 and jpeg.choose_ratio(480, 641, 240, 320, 8) == 4
  assert jpeg.choose_ratio(480, 640, 60, 80, 8) == 8 and jpeg.choose_ratio(481, 640, 60, 80, 8) is None
  assert jpeg.choose_ratio(480, 640, 59, 80) is None
  assert jpeg.choose_ratio(480, 640, 60, 80, 4) is None and jpeg.choose_ratio(480, 640, 240, 320, 1) is None      # max_ratio caps
  assert jpeg.choose_ratio(480, 640, 120, 160, 4) == 4 and jpeg.choose_ratio(480, 640, 120, 160, 2) is None
  for h, w, canvas in ((480, 640, (240, 320)), (481, 641, (240, 320)), (37, 53, (5, 7)), (37, 53, (4, 7))):
    for cap in (1, 2, 4, 8):
      assert jpeg.choose_ratio(h, w, canvas[0], canvas[1], cap) == js.choose_denom(h, w, canvas, cap)
  for bad in (0, 3, 16, None):
    with pytest.raises(ValueError):
      jpeg.scaled_size(8, 8, bad)
    with pytest.raises(ValueError):
      jpeg.choose_ratio(8, 8, 8, 8, bad)


def _decode_host(datas, canvas, max_ratio=8, ratios=None, threads=0, capacity=None):
  n = len(datas)
  capacity = 64 * 4096 if capacity is None else capacity
  coef = np.full(capacity, 0x5A5A, np.int16)
  images = np.zeros(n * jpeg.IMAGE_BYTES, np.uint8)
  qt = np.full((n, 4, 64), 0xFFFF, np.uint16)
  status = np.full(n, -1, np.int32)
  jpeg.entropy_decode_scaled(datas, canvas[0], canvas[1], max_ratio, ratios, coef, images, qt, status, threads)
  return coef, jpeg.descriptors(images, n), qt, status


def test_host_stage_equals_the_restatement(cases, parsed, lib):
  """ONE batch of every stream, refused ones in between, into an 8 x 34 canvas: the chosen denominators are the
  restatement's (1, 2, 4, 8 and TOO_LARGE all occur); then the same batch with every denominator forced."""
  ok, _, refused = cases
  canvas = (8, 34)
  names = sorted(ok)
  order = names[:5] + ['truncated_17x33'] + names[5:20] + ['progressive_17x33', 'huffman_17x33'] + names[20:] + ['cmyk_16x16']
  datas = [ok[n][0] if n in ok else refused[n][0] for n in order]

  def check(forced):
    def denom_of(h, w):
      """The denominator of an h x w file, or None: chosen, or the forced one if its output fits."""
      if forced is None:
        return js.choose_denom(h, w, canvas)
      size = js.scaled_size(h, w, forced)
      return forced if size[0] <= canvas[0] and size[1] <= canvas[1] else None

    denoms = None if forced is None else [forced] * len(order)
    coef, desc, qt, status = _decode_host(datas, canvas, ratios=denoms, threads=1)
    at = 0
    seen = set()
    for i, name in enumerate(order):
      d = desc[i]
      assert d.status == status[i]
      if name in refused:
        # truncated and huffman are refused inside the scan, so only if their header passed: TOO_LARGE comes first, and
        # where it does not, their place in the arena stays, unused
        fr = jr.info(refused[name][0])
        in_scan = name in ('truncated_17x33', 'huffman_17x33')
        if in_scan and denom_of(fr.height, fr.width) is None:
          assert d.status == jpeg.TOO_LARGE, name
        else:
          assert d.status == refused[name][1], name
          if in_scan:
            at += sum(b.size // 64 for b in jr.parse(ok['s17x33_420_q75'][0]).coefs)
        assert (d.height, d.width, d.components, d.total_blocks, d.reserved) == (0, 0, 0, 0, 0) and not qt[i].any()
        continue
      want = parsed[name]
      fr, nc = want.frame, want.frame.components
      denom = denom_of(fr.height, fr.width)
      size = js.scaled_size(fr.height, fr.width, denom) if denom else None
      if denom is None:
        assert d.status == jpeg.TOO_LARGE and (d.height, d.width, d.total_blocks, d.reserved) == (0, 0, 0, 0), name
        assert not qt[i].any()
        seen.add(None)
        continue
      seen.add(denom)
      assert d.status == 0 and d.reserved == denom and (d.height, d.width) == size, (name, denom)
      assert (d.components, d.h_max, d.v_max) == (nc, want.h_max, want.v_max), name
      assert list(d.blocks_w[:nc]) == want.blocks_w and list(d.blocks_h[:nc]) == want.blocks_h, name
      assert list(d.quant_id[:nc]) == list(fr.quant_id[:nc]) and np.array_equal(qt[i], want.qtables), name
      for c in range(nc):
        assert d.first_block[c] == at, (name, c)
        n = want.coefs[c].size
        assert np.array_equal(coef[64 * at:64 * at + n], want.coefs[c].reshape(-1)), (name, c)
        at += n // 64
      assert d.total_blocks == sum(b.size // 64 for b in want.coefs)
    assert (coef[64 * at:] == 0x5A5A).all()      # nothing is written behind the last block
    for threads in (3, 16):
      coef_t, desc_t, qt_t, status_t = _decode_host(datas, canvas, ratios=denoms, threads=threads)
      assert np.array_equal(coef_t, coef) and np.array_equal(qt_t, qt) and np.array_equal(status_t, status), threads
      assert [bytes(a) for a in desc_t] == [bytes(a) for a in desc], threads
    return seen

  assert check(None) == {1, 2, 4, 8, None}
  assert check(1) == {1, None} and check(2) == {2, None} and check(8) == {8, None}


def test_coefficients_are_the_full_size_stages(cases, lib):
  """One stream, every denominator: the arena and the tables of edet_jpeg_entropy_decode, byte for byte; the descriptor
  differs in height, width and `reserved` alone."""
  data = cases[0]['s37x53_420_q75'][0]
  n = 64 * 80
  coef = np.full(n, 0x5A5A, np.int16)
  images, qt, status = np.zeros(jpeg.IMAGE_BYTES, np.uint8), np.zeros((1, 4, 64), np.uint16), np.zeros(1, np.int32)
  jpeg.entropy_decode([data], 37, 53, coef, images, qt, status)
  full = jpeg.descriptors(images, 1)[0]
  assert full.status == 0 and full.reserved == 0
  for denom in (1, 2, 4, 8):
    got_coef, (d,), got_qt, _ = _decode_host([data], js.scaled_size(37, 53, denom), capacity=n)
    assert np.array_equal(got_coef, coef) and np.array_equal(got_qt, qt)
    assert (d.height, d.width, d.reserved) == js.scaled_size(37, 53, denom) + (denom,)
    d.height, d.width, d.reserved = full.height, full.width, 0
    assert bytes(d) == bytes(full)


def test_an_arena_that_runs_out(cases, lib):
  ok, _, _ = cases
  big, small = ok['s37x53_420_q75'][0], ok['s8x9_444_q75'][0]
  blocks = sum(b.size // 64 for b in jr.parse(big).coefs)
  few = sum(b.size // 64 for b in jr.parse(small).coefs)
  # the second large image no longer fits; the small one behind it does, and is intact
  coef, desc, qt, status = _decode_host([big, big, small], (5, 7), capacity=64 * (2 * blocks - 1))
  assert list(status) == [jpeg.OK, jpeg.TOO_LARGE, jpeg.OK]
  assert desc[0].reserved == 8 and desc[1].total_blocks == 0 and desc[2].reserved == 2 and desc[2].first_block[0] == blocks
  want = jr.parse(small)
  got = coef[64 * blocks:64 * (blocks + few)]
  assert np.array_equal(got, np.concatenate([c.reshape(-1) for c in want.coefs])) and np.array_equal(qt[2], want.qtables)
  assert (coef[64 * (blocks + few):] == 0x5A5A).all()


def test_arguments_the_call_refuses(cases, lib):
  data = cases[0]['s16x16_420_q75'][0]
  for bad in (0, 3, 5, 16, -1):
    with pytest.raises(_lib.EdetError, match='max_denom'):
      _decode_host([data], (16, 16), max_ratio=bad)
    with pytest.raises(_lib.EdetError, match=r'denoms\[1\]'):
      _decode_host([data, data], (16, 16), ratios=[1, bad])
  with pytest.raises(ValueError, match='ratios'):
    _decode_host([data, data], (16, 16), ratios=[1])
  # a forced denominator whose output does not fit is a status, not an error; max_denom does not bound a forced one
  assert _decode_host([data], (8, 8), ratios=[1])[3][0] == jpeg.TOO_LARGE
  assert _decode_host([data], (8, 8), max_ratio=1, ratios=[2])[3][0] == jpeg.OK
  with pytest.raises(ValueError, match='ratio'):
    jpeg.decode_jpeg(data, ratio=3)
  with pytest.raises(ValueError, match='ratio'):
    jpeg.decode_jpeg(data, channels=3, ratio=0)
  for kw in ({'max_ratio': 3}, {'max_ratio': 0}, {'max_ratio': 8, 'coef_blocks': 0},
             {'max_ratio': 2, 'coef_blocks': 4 * 2 * jpeg.worst_blocks(16, 16) + 1}, {'coef_blocks': 2 * jpeg.worst_blocks(16, 16) + 1}):
    with pytest.raises(ValueError, match='max_ratio'):
      jpeg.JpegDecoder(2, 16, 16, **kw)


def test_host_stage_under_sanitizers(cases, tmp_path):
  """tests/c_host/jpeg_scaled_host_check.cpp + csrc/jpeg_host.cpp, built with -fsanitize=address,undefined and run as a child
  process: every denominator chosen and forced, every prefix of one small stream and 300 single-byte corruptions through
  edet_jpeg_entropy_decode_scaled at max_denom 8.  Skips only where the host compiler cannot build a trivial sanitized
  program."""
  cxx = _cxx()
  flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-pthread']
  trivial = tmp_path / 'trivial.cpp'
  trivial.write_text('int main() { return 0; }\n')
  if cxx is None or subprocess.run([cxx] + flags + [str(trivial), '-o', str(tmp_path / 'trivial')],
                                   capture_output=True).returncode != 0 or \
      subprocess.run([str(tmp_path / 'trivial')], capture_output=True).returncode != 0:
    pytest.skip('the host compiler cannot build a sanitized program')
  exe = str(tmp_path / 'jpeg_scaled_host_check')
  r = subprocess.run([cxx] + flags + ['-Wall', '-Wextra', os.path.join(ROOT, 'tests', 'c_host', 'jpeg_scaled_host_check.cpp'),
                                      os.path.join(ROOT, 'automl_amd', 'csrc', 'jpeg_host.cpp'), '-o', exe],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  (tmp_path / 'stream.jpg').write_bytes(cases[0]['s17x33_420_q75'][0])
  r = subprocess.run([exe, str(tmp_path / 'stream.jpg')], capture_output=True, text=True, errors='replace', timeout=600)
  assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
  assert '17 x 33' in r.stdout and ' 0 failures' in r.stdout, r.stdout


class HostDecoder(object):
  """jpeg.JpegDecoder with the device stage left out, as in tests/test_effnetv2_datasets.py, through the reduced-size host
  stage; it records how it was built."""
  built = []

  def __init__(self, batch, canvas_h, canvas_w, depth=2, threads=None, max_ratio=1):
    self.batch, self.hc, self.wc, self.threads, self.max_ratio = batch, canvas_h, canvas_w, threads or min(16, batch), max_ratio
    HostDecoder.built.append(max_ratio)

  def decode(self, contents, fallback=None):
    b = self.batch
    coef = np.zeros(64 * 8192, np.int16)
    images, qtables, status = np.zeros(b * jpeg.IMAGE_BYTES, np.uint8), np.zeros((b, 4, 64), np.uint16), np.zeros(b, np.int32)
    jpeg.entropy_decode_scaled(contents, self.hc, self.wc, self.max_ratio, None, coef, images, qtables, status, self.threads)
    sizes = np.zeros((b, 2), np.int32)
    for i, d in enumerate(jpeg.descriptors(images, b)):
      if d.status:
        raise ValueError('contents[%d] is not decoded: %s (status %d)' % (i, jpeg.REASONS.get(int(d.status), '?'), d.status))
      sizes[i] = (d.height, d.width)
    return None, sizes


def test_max_ratio_reaches_the_decoder_through_the_reader(lib, tmp_path, monkeypatch):
  """The ImageNet reader with an image larger than its canvas: refused with max_ratio=1 (the default, which builds the
  decoder without the argument), delivered at the chosen ratio's size with max_ratio=8; the order and the resume state of the
  reader are the same with and without it."""
  jpegs = ref.load_jpegs()
  wide = ref.load_jpegs(('s24x280_420_q75',))[0]
  for f in range(2):
    with tfrecord.TFRecordWriter(tmp_path / ('val-%05d-of-00002' % f)) as w:
      for r in range(4):
        w.write(tfrecord.encode_example({'image/encoded': wide if (f, r) == (1, 2) else jpegs[r + 1], 'image/class/label': [r + 1]}))
  monkeypatch.setattr(jpeg, 'JpegDecoder', HostDecoder)
  HostDecoder.built = []
  cfg = {'num_classes': 24}
  reader = ds.ImageNetInput(False, str(tmp_path), seed=3, cfg=cfg).reader(4, canvas=(56, 56), max_ratio=8)
  (_, first), _ = next(reader)
  state = reader.get_state()
  (_, sizes), labels = next(reader)      # (0, 2), (1, 2), (0, 3), (1, 3)
  assert HostDecoder.built == [8] and labels.tolist() == [2, 2, 3, 3]
  assert sizes[1].tolist() == [3, 35] == list(jpeg.scaled_size(24, 280, jpeg.choose_ratio(24, 280, 56, 56, 8)))
  assert sizes[0].tolist() == [17, 33]      # an image that fits stays at full size
  reader.close()
  plain = ds.ImageNetInput(False, str(tmp_path), seed=3, cfg=cfg).reader(4, canvas=(56, 56))
  (_, first_plain), _ = next(plain)
  assert np.array_equal(first_plain, first) and plain.get_state() == state
  with pytest.raises(ValueError, match='record 2: contents.1.*larger than the canvas'):
    next(plain)
  plain.close()
  capped = ds.ImageNetInput(False, str(tmp_path), seed=3, cfg=cfg).reader(4, canvas=(56, 56), max_ratio=4)      # 70 columns at 1/4
  next(capped)
  with pytest.raises(ValueError, match='larger than the canvas'):
    next(capped)
  capped.close()
  with pytest.raises(ValueError, match='max_ratio'):
    ds.ImageNetInput(False, str(tmp_path), seed=3, cfg=cfg).reader(4, canvas=(56, 56), max_ratio=3)


def test_the_cli_flag_reaches_the_reader(monkeypatch):
  assert main_lib.parse_flags([]).jpeg_max_ratio == 1 and main_lib.parse_flags(['--jpeg_max_ratio=8']).jpeg_max_ratio == 8
  for bad in ('3', '16', 'x'):
    with pytest.raises(SystemExit):
      main_lib.parse_flags(['--jpeg_max_ratio=' + bad])
  calls = []

  class Input(object):
    def __call__(self, batch, **kw):
      calls.append((batch, kw))
      return 'reader'

  monkeypatch.setattr(ds, 'build_dataset_input', lambda *a, **kw: Input())
  flags = main_lib.parse_flags(['--jpeg_max_ratio=4', '--canvas=56x64', '--data_dir=/nowhere'])
  config = main_lib.build_config(main_lib.parse_flags(['--hparam_str=data.augname=randaug']))
  plan = {'train_split': 'train', 'eval_split': 'eval'}
  assert main_lib.get_dataset(flags, config, plan, True) == 'reader'
  assert calls == [(config.train.batch_size, {'canvas': (56, 64), 'max_ratio': 4})]
