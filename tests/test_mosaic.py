"""automl_amd/mosaic.py, edet_mosaic and edet_mosaic_boxes (csrc/mosaic.hip): the reference's efficientdet/aug/mosaic.py.

Without a GPU: the numpy restatement tests/mosaic_ref.py against what the reference's own module computed on the torch stand-in
(tests/golden/reference_mosaic.npz, written by tests/golden/make_golden_mosaic.py) -- boxes exactly, pixels within a measured
bound, quadrant rectangles and seams exactly -- the divide-point bounds, the draws of the batch form, the clamp, the ABI.
On the GPU: both kernels against the restatement, bit for bit, and mosaic_batch through one train_step_raw."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from automl_amd import _lib, mosaic as mz, v2_preprocessing as vp
from tests import mosaic_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('ragged_seam_in_run', 'ragged_seam_on_run', 'ragged_scalar_rows', 'tiny_equal', 'tiny_equal_odd')


@pytest.fixture(scope='module')
def golden():
  return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_mosaic.npz')))


def case_of(golden, name):
  images = [golden['%s/image_%d' % (name, k)] for k in range(4)]
  x, y = (int(v) for v in golden[name + '/draws'])
  return images, golden[name + '/boxes_in'], (x, y), tuple(int(v) for v in golden[name + '/out_size'])


# ---- the restatement against the reference's own output ----------------------------------------------------------------------
def test_fixture_holds_the_cases_the_kernel_can_go_wrong_on(golden):
  seen = {(tuple(golden[n + '/out_size']), tuple(golden[n + '/draws'])) for n in CASES}
  assert ((8, 12), (3, 5)) in seen and ((8, 12), (1, 4)) in seen            # the column seam inside a run of four / on a boundary
  assert {(o, d[0]) for o, d in seen} >= {((8, 12), 1), ((8, 12), 7), ((7, 10), 1), ((7, 10), 6)}      # row seam at 1, out0 - 1
  assert [golden['ragged_seam_in_run/image_%d' % k].shape[:2] for k in range(4)] == [(5, 7), (4, 4), (9, 3), (1, 1)]
  for n in CASES:
    b = golden[n + '/boxes_in']
    assert b.dtype == np.int32 and b.shape == (4, 2, 4)
    for k in range(4):      # one box touches the image's far corner
      h, w = golden['%s/image_%d' % (n, k)].shape[:2]
      assert (b[k, :, 2] == w).any() and (b[k, :, 3] == h).any()


@pytest.mark.parametrize('name', CASES)
def test_restated_boxes_equal_the_reference_exactly(golden, name):
  images, boxes, (x, y), out_size = case_of(golden, name)
  got = mr.mosaic_boxes(boxes, [im.shape[:2] for im in images], x, y, out_size)
  want = golden[name + '/boxes']
  assert want.dtype == np.float64 and want.shape == (4, 2, 4)
  for k in range(4):
    assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
  # ... and the package's own host arithmetic (Mosaic.__call__ uses it) is the same
  subs = mr.quadrants(x, y, *out_size)
  for k, (oy, ox, qh, qw) in enumerate(subs):
    assert np.array_equal(mz.scale_boxes(boxes[k], images[k].shape[:2], (qh, qw), (ox, oy)), want[k])


# The stand-in's resize (torch's interpolate) forms the same bilinear value in another operation order.  Measured on this
# fixture on the CPU: the largest difference over the five cases is 3.0517578e-05 on the 0..255 scale (two ulps of a value in
# [128, 256)); the bound is four times that, 1.2207031e-04, below the cap of 1e-3 -- far below one grey level, so it cannot
# hide a wrong tap or a misplaced seam.
IMAGE_BOUND = 4 * 3.0517578125e-05


def test_restated_image_is_the_reference_image_within_the_measured_bound(golden):
  assert IMAGE_BOUND <= 1e-3
  worst = 0.0
  for name in CASES:
    images, _, (x, y), out_size = case_of(golden, name)
    got = mr.mosaic_image(images, x, y, out_size)
    want = golden[name + '/mosaic']
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == out_size + (3,)
    d = float(np.abs(got.astype(np.float64) - want).max())
    print('%s: largest difference %.8g' % (name, d))
    worst = max(worst, d)
    assert d <= IMAGE_BOUND, (name, d)
  print('largest difference over the fixture %.8g, bound %.8g' % (worst, IMAGE_BOUND))


@pytest.mark.parametrize('out_size, x, y', [((8, 12), 3, 5), ((8, 12), 1, 4), ((7, 10), 6, 9), ((7, 10), 1, 1), ((6, 300), 5, 257)])
def test_every_colour_fills_exactly_its_rectangle(out_size, x, y):
  """Constant sources, one colour per image: shapes of the quadrants and the position of both seams, exactly -- and the same
  from the reference's own placement, by way of its stand-in run, in the next test."""
  sizes = ((5, 7), (4, 4), (9, 3), (1, 1))
  images = [np.full((h, w, 3), 40 * (k + 1), np.uint8) for k, (h, w) in enumerate(sizes)]
  got = mr.mosaic_image(images, x, y, out_size)
  want = np.zeros(out_size + (3,), np.float32)
  want[:x, :y], want[x:, :y], want[:x, y:], want[x:, y:] = 40, 80, 120, 160
  assert np.array_equal(got, want)
  assert np.array_equal(mr.convert(got, 'u8'), want.astype(np.uint8))


@pytest.mark.parametrize('name', CASES)
def test_reference_placement_is_the_restated_one(golden, name):
  """Where the reference put each image: every rectangle of the fixture's mosaic is the restated resize of ITS source (the
  sources are random, so another image's resize, or the same one a pixel off, is tens of grey levels away)."""
  images, _, (x, y), out_size = case_of(golden, name)
  want = golden[name + '/mosaic']
  for k, (oy, ox, qh, qw) in enumerate(mr.quadrants(x, y, *out_size)):
    own = mr.mosaic_image(images, x, y, out_size)[oy:oy + qh, ox:ox + qw]
    assert own.shape == (qh, qw, 3) and np.abs(own - want[oy:oy + qh, ox:ox + qw]).max() <= IMAGE_BOUND, (name, k)
  assert sum(qh * qw for _, _, qh, qw in mr.quadrants(x, y, *out_size)) == out_size[0] * out_size[1]


def test_output_conversions():
  v = np.asarray([-3.5, -0.0, 0.99, 1.0, 127.5, 254.999, 255.0, 300.0], np.float32)
  assert mr.convert(v, 'u8').tolist() == [0, 0, 0, 1, 127, 254, 255, 255]
  assert mr.convert(v, 'f32') is not None and np.array_equal(mr.convert(v, 'f32'), v)


# ---- divide points ------------------------------------------------------------------------------------------------------------
def test_divide_point_bounds(golden):
  assert mz.divide_point_bounds() == ((170, 510), (170, 510))
  assert golden['default/bounds'].tolist() == [[170, 510], [170, 510]] and golden['default/draws'].tolist() == [170, 509]
  for name in CASES:
    out_size = tuple(int(v) for v in golden[name + '/out_size'])
    assert [list(b) for b in mz.divide_point_bounds(out_size)] == golden[name + '/bounds'].tolist(), name
  # truncation of Python doubles: 7 * 0.25 = 1.75 -> 1, 7 * 0.75 = 5.25 -> 5; 10 * 0.3 = 3.0, 10 * 0.7 = 7.000000000000001 -> 7
  assert mz.divide_point_bounds((7, 10)) == ((1, 5), (2, 7))
  assert mz.divide_point_bounds((10, 101), 30) == ((3, 7), (30, 70))
  assert mz.divide_point_bounds((680, 512), 25) == ((170, 510), (128, 384))


def test_divide_points_stay_inside_their_bounds_and_reach_both_ends():
  rng = np.random.default_rng(3)
  pts = np.array([mz.mosaic_divide_points(rng, (8, 12)) for _ in range(400)])
  assert set(pts[:, 0]) == {2, 3, 4, 5} and set(pts[:, 1]) == {3, 4, 5, 6, 7, 8}
  # x is drawn first, then y
  a, b = np.random.default_rng(9), np.random.default_rng(9)
  assert mz.mosaic_divide_points(a, (680, 680)) == (int(b.integers(170, 510)), int(b.integers(170, 510)))
  m = mz.Mosaic((8, 12))
  assert m.mosaic_divide_points(np.random.default_rng(1)) == mz.mosaic_divide_points(np.random.default_rng(1), (8, 12))


def test_the_class_and_what_it_refuses():
  m = mz.Mosaic()
  assert m.n_images == 4 and m.out_size == (680, 680)
  assert mz.Mosaic((8, 12), 4, 30).out_size == (8, 12)
  with pytest.raises(AssertionError, match='above 0'):
    mz.Mosaic(_minimum_mosaic_image_dim=0)
  boxes = np.zeros((4, 2, 4), np.int32)
  images = np.zeros((4, 5, 6, 3), np.uint8)
  with pytest.raises(ValueError, match='Currently Exact 4 Images are supported by Mosaic Aug.'):
    mz.Mosaic((8, 12))(images[:3], boxes[:3], divide_points=(3, 5))
  with pytest.raises(ValueError, match='Currently Exact 4 Images'):
    mz.Mosaic((8, 12))((np.zeros((5, 5, 6, 3), np.uint8), np.full((5, 2), 5)), [boxes[0]] * 5, divide_points=(3, 5))
  with pytest.raises(ValueError, match='uint8'):
    mz.Mosaic((8, 12))(images.astype(np.float32), boxes, divide_points=(3, 5))
  with pytest.raises(ValueError, match='integers'):
    mz.Mosaic((8, 12))(images, boxes.astype(np.float32), divide_points=(3, 5))
  with pytest.raises(ValueError, match='integers'):
    mz.scale_boxes(np.zeros((2, 4), np.float32), (4, 4), (2, 2), (0, 0))
  # bounds that leave no value to draw, where tf.random.uniform raises: int(8 * 0.5) = 4 on both sides; int(3 * 0.4) = 1 = int(3 * 0.6)
  with pytest.raises(ValueError, match='leaves no divide point'):
    mz.divide_point_bounds((8, 12), 50)
  with pytest.raises(ValueError, match='leaves no divide point'):
    mz.mosaic_divide_points(np.random.default_rng(0), (8, 12), 60)
  with pytest.raises(ValueError, match='leaves no divide point'):
    mz.Mosaic((1000, 3), 4, 40)(images, boxes, rng=np.random.default_rng(0))


# ---- the batch form's draws -----------------------------------------------------------------------------------------------------
def test_mosaic_draws():
  index, points = mz.mosaic_draws(np.random.default_rng(5), 7, 3, (8, 12))
  assert index.dtype == points.dtype == np.int32 and index.shape == (7, 4) and points.shape == (7, 2)
  assert index[:, 0].tolist() == [0, 1, 2, 0, 1, 2, 0]
  # the documented order: one [G, 3] draw over the batch, then x for every mosaic, then y for every mosaic
  rng = np.random.default_rng(5)
  assert np.array_equal(index[:, 1:], rng.integers(0, 3, (7, 3)))
  assert np.array_equal(points[:, 0], rng.integers(2, 6, 7)) and np.array_equal(points[:, 1], rng.integers(3, 9, 7))
  index, points = mz.mosaic_draws(np.random.default_rng(6), 500, 6, (680, 680))
  assert set(index[:, 1:].reshape(-1)) == set(range(6)) and points.min() >= 170 and points.max() <= 509
  # the bounds are checked before the generator moves
  rng, same = np.random.default_rng(2), np.random.default_rng(2)
  with pytest.raises(ValueError, match='leaves no divide point'):
    mz.mosaic_draws(rng, 4, 4, (8, 12), 50)
  assert rng.random() == same.random()
  rows = mz.mosaic_rows([[2, 0, 1, 1]], [[3, 5]], [[5, 7], [4, 4], [9, 3]])
  assert rows.tolist() == [[2, 0, 1, 1, 3, 5, 9, 5, 4, 4, 3, 7, 4, 4, 0, 0]]
  with pytest.raises(ValueError, match='the batch has 3 images'):
    mz.mosaic_rows([[3, 0, 1, 1]], [[3, 5]], [[5, 7], [4, 4], [9, 3]])


def test_clamp_rows():
  rows = [[-1, 6, 2, 7, 0, 12, 0, 99, 5, -4, 54, 3, 0, 7, 9, 9],
          [0, 1, 2, 3, 8, 0, 1, 37, 38, 2, 1, 53, 54, 2, 0, 0],
          [5, 5, 5, 5, 7, 11, 3, 3, 3, 3, 4, 4, 4, 4, 0, 0]]
  assert mz.clamp_rows(rows, 6, 37, 53, 8, 12).tolist() == [[0, 5, 2, 5, 1, 11, 1, 37, 5, 1, 53, 3, 1, 7, 0, 0],
                                                           [0, 1, 2, 3, 7, 1, 1, 37, 37, 2, 1, 53, 53, 2, 0, 0],
                                                           [5, 5, 5, 5, 7, 11, 3, 3, 3, 3, 4, 4, 4, 4, 0, 0]]


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_declarations_match_the_signatures():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'edet_hip.h')).read(), flags=re.S)
  for name, count in (('edet_mosaic', 11), ('edet_mosaic_boxes', 13)):
    m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
    assert m, 'include/edet_hip.h does not declare %s' % name
    args = [a.strip() for a in m.group(1).split(',')]
    bound = _lib.SIGNATURES[name]
    assert len(args) == len(bound) == count
    assert [('*' in a) for a in args] == [t is ctypes.c_void_p for t in bound], args
  fields = re.search(r'typedef struct edet_mosaic \{(.*?)\} edet_mosaic_t;', src, flags=re.S).group(1)
  names = [n.strip() for part in fields.split(';') if part.strip() for n in part.replace('int32_t', '').split(',')]
  assert names == ['index[4]', 'x', 'y', 'height[4]', 'width[4]', 'reserved[2]']
  assert [n for n, _ in _lib.MosaicRow._fields_] == ['index', 'x', 'y', 'height', 'width', 'reserved']
  assert ctypes.sizeof(_lib.MosaicRow) == 64 == 4 * mz.ROW_WORDS
  assert (_lib.MosaicRow.x.offset, _lib.MosaicRow.height.offset, _lib.MosaicRow.width.offset) == (4 * mz.X, 24, 40)
  committed = open(os.path.join(ROOT, 'automl_amd', 'csrc', 'plan_stubs.inc')).read()
  assert '"edet_mosaic",' in committed and '"edet_mosaic_boxes",' in committed


# ---- the batch form's box rule against the reference's ------------------------------------------------------------------------
def normalised(boxes_xyxy, h, w):
  """Integer pixel boxes [x1, y1, x2, y2] -> float32 (ymin, xmin, ymax, xmax) normalised by the source size."""
  b = np.asarray(boxes_xyxy, np.float32)
  return np.stack([b[:, 1] / np.float32(h), b[:, 0] / np.float32(w), b[:, 3] / np.float32(h), b[:, 2] / np.float32(w)], 1)


@pytest.mark.parametrize('name', CASES)
def test_batch_box_rule_agrees_with_the_reference(golden, name):
  """Four float32 roundings on values in [0, 1] (the normalisation, the product, the sum, the division): at most 4 * 2^-24
  from the reference's float64 pixels divided by the output size."""
  images, boxes, (x, y), (out0, out1) = case_of(golden, name)
  norm = np.stack([normalised(boxes[k], *images[k].shape[:2]) for k in range(4)])
  rows = mz.mosaic_rows([[0, 1, 2, 3]], [[x, y]], [im.shape[:2] for im in images])
  ob, oc, on = mr.batch_boxes(norm, np.ones((4, 2), np.float32), [2, 2, 2, 2], rows, (out0, out1))
  assert on.tolist() == [8] and ob.dtype == np.float32
  want = golden[name + '/boxes'].reshape(8, 4) / np.asarray([out1, out0, out1, out0], np.float64)
  got = ob[0][:, [1, 0, 3, 2]].astype(np.float64)
  d = float(np.abs(got - want).max())
  print('%s: largest difference %.3g (bound %.3g)' % (name, d, 4 * 2.0 ** -24))
  assert d <= 4 * 2.0 ** -24, (name, d)


def test_batch_boxes_row_order_and_padding():
  boxes = np.arange(3 * 2 * 4, dtype=np.float32).reshape(3, 2, 4) / 32
  classes = np.asarray([[1, 2], [3, 4], [5, 6]], np.float32)
  rows = mz.mosaic_rows([[2, 0, 1, 2]], [[3, 5]], [[4, 4]] * 3)
  ob, oc, on = mr.batch_boxes(boxes, classes, [1, 0, 2], rows, (8, 12))
  # source 2 (two rows), source 0 (one), source 1 (none), source 2 again
  assert on.tolist() == [5] and oc[0].tolist() == [5, 6, 1, 5, 6, -1, -1, -1] and (ob[0, 5:] == -1).all()
  f = np.float32
  assert ob[0, 0].tolist() == [(f(0) + boxes[2, 0, 0] * f(3)) / f(8), (f(0) + boxes[2, 0, 1] * f(5)) / f(12),
                               (f(0) + boxes[2, 0, 2] * f(3)) / f(8), (f(0) + boxes[2, 0, 3] * f(5)) / f(12)]
  assert ob[0, 2].tolist() == [(f(3) + boxes[0, 0, 0] * f(5)) / f(8), (f(0) + boxes[0, 0, 1] * f(5)) / f(12),      # below: oy = x
                               (f(3) + boxes[0, 0, 2] * f(5)) / f(8), (f(0) + boxes[0, 0, 3] * f(5)) / f(12)]
  assert ob[0, 4].tolist() == [(f(3) + boxes[2, 1, 0] * f(5)) / f(8), (f(5) + boxes[2, 1, 1] * f(7)) / f(12),
                               (f(3) + boxes[2, 1, 2] * f(5)) / f(8), (f(5) + boxes[2, 1, 3] * f(7)) / f(12)]


# ---- the kernels against the restatement ----------------------------------------------------------------------------------------
KINDS = {'f32': torch.float32, 'u8': torch.uint8}


def run_rows(raw_dev, rows, out_size, kind, out=None):
  """edet_mosaic on rows handed over as they are (no host check: out-of-range fields reach the kernel)."""
  rows_dev = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
  if out is None:
    out = torch.empty((len(rows),) + tuple(out_size) + (3,), dtype=KINDS[kind], device='cuda')
  mz.launch(raw_dev, rows_dev, out, torch.cuda.current_stream().cuda_stream)
  torch.cuda.synchronize()
  return out


def assert_equal(got, want, what):
  got = got.cpu().numpy()
  assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
  if not np.array_equal(got, want):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    raise AssertionError('%s: %d of %d values differ, worst %g at %s' % (what, int((d != 0).sum()), d.size, float(d.max()),
                                                                         np.unravel_index(int(d.argmax()), d.shape)))


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_kernel_equals_the_restatement_on_the_fixture(golden, name):
  images, boxes, (x, y), out_size = case_of(golden, name)
  raw, sizes = vp.pad_batch(images)
  rows = mz.mosaic_rows([[0, 1, 2, 3]], [[x, y]], sizes)
  for kind in KINDS:
    want = mr.mosaic_from_rows(raw.numpy(), rows, out_size, kind)
    assert_equal(mz.mosaic_images((raw, sizes), [[0, 1, 2, 3]], [[x, y]], out_size, kind), want, (name, kind))
  # the class: the float32 mosaic and the reference's boxes
  mosaic, out_boxes = mz.Mosaic(out_size)((raw, sizes), boxes, divide_points=(x, y))
  assert_equal(mosaic, mr.mosaic_image(images, x, y, out_size), (name, 'Mosaic'))
  assert float((mosaic.cpu() - torch.from_numpy(golden[name + '/mosaic'])).abs().max()) <= IMAGE_BOUND
  assert all(b.dtype == np.float64 and np.array_equal(b, golden[name + '/boxes'][k]) for k, b in enumerate(out_boxes))
  if name.startswith('tiny'):      # a dense [4, h, w, 3] array and a drawn divide point
    dense, _ = mz.Mosaic(out_size)(np.stack(images), boxes, rng=np.random.default_rng(0))
    px, py = mz.mosaic_divide_points(np.random.default_rng(0), out_size)
    assert_equal(dense, mr.mosaic_image(images, px, py, out_size), (name, 'dense'))


CANVAS = (37, 53)
SIZES = [(37, 53), (1, 1), (2, 50), (30, 3), (16, 16), (9, 20)]
INDEX = [[5, 0, 3, 1], [2, 2, 2, 2], [0, 5, 1, 4], [4, 3, 3, 0], [1, 1, 0, 5]]      # repeated, out of order, one image four times


def canvas_batch(seed=7):
  """Random images in the top-left corners of a canvas filled with another random pattern (which nothing may read)."""
  return np.random.default_rng(seed).integers(0, 256, (len(SIZES),) + CANVAS + (3,)).astype(np.uint8)


def points_for(out0, out1):
  """Seams at 1 and at out - 1 in both directions, inside a run of four, and (for rows longer than 256 pixels) past the
  first wave's stretch."""
  return [[1, 1], [out0 - 1, out1 - 1], [out0 // 2, 5], [1, out1 - 1], [out0 - 1, min(257, out1 - 2)]]


# (8, 12): three 4-pixel vector stores per thread; (7, 10): no multiple of 4, one value per store; (6, 300): a row longer than
# the 256 pixels one wave covers
@pytest.mark.gpu
@pytest.mark.parametrize('out_size', [(8, 12), (7, 10), (6, 300)], ids=lambda s: '%dx%d' % s)
def test_kernel_equals_the_restatement_on_a_canvas_batch(out_size):
  raw = canvas_batch()
  dev = torch.from_numpy(raw).cuda()
  rows = mz.mosaic_rows(INDEX, points_for(*out_size), SIZES)
  for kind in KINDS:
    want = mr.mosaic_from_rows(raw, rows, out_size, kind)
    assert_equal(run_rows(dev, rows, out_size, kind), want, (out_size, kind))
    assert_equal(mz.mosaic_images((dev, np.asarray(SIZES, np.int32)), INDEX, points_for(*out_size), out_size, kind), want,
                 (out_size, kind, 'mosaic_images'))


@pytest.mark.gpu
def test_unaligned_output_takes_the_scalar_path_to_the_same_result():
  raw = canvas_batch(8)
  dev = torch.from_numpy(raw).cuda()
  out_size = (8, 12)
  rows = mz.mosaic_rows(INDEX, points_for(*out_size), SIZES)
  n = len(rows) * 8 * 12 * 3
  for kind, dtype in KINDS.items():
    shift = 4 // torch.empty((), dtype=dtype).element_size()      # elements in 4 bytes
    buf = torch.zeros(n + shift + 8, dtype=dtype, device='cuda')
    view = buf[shift:shift + n].view(len(rows), 8, 12, 3)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    aligned = run_rows(dev, rows, out_size, kind)
    run_rows(dev, rows, out_size, kind, out=view)
    assert torch.equal(aligned, view), kind
    assert_equal(view, mr.mosaic_from_rows(raw, rows, out_size, kind), ('unaligned', kind))
    assert int(buf[:shift].abs().sum()) == 0 and int(buf[shift + n:].abs().sum()) == 0      # nothing written around it


@pytest.mark.gpu
def test_out_of_range_rows_are_clamped():
  """Index -1 and B, a size of 0 and one beyond the canvas, a divide point of 0 and of out: each gives what the Python clamp
  says.  The batch sits in the middle of a larger allocation filled with a sentinel, so a read outside shows in the result."""
  raw = np.minimum(canvas_batch(9), 200)
  b = len(SIZES)
  pad = raw[0].size
  big = torch.full((raw.size + 2 * pad,), 255, dtype=torch.uint8, device='cuda')
  big[pad:pad + raw.size] = torch.from_numpy(raw).reshape(-1).cuda()
  dev = big[pad:pad + raw.size].view(raw.shape)
  for out_size in ((8, 12), (7, 10)):
    o0, o1 = out_size
    rows = np.asarray([[-1, b, 2, 3, 0, o1, 37, 53, 0, 30, 53, 53, 50, 99, 0, 0],
                       [b + 7, -9, 5, 0, o0, 0, 0, 400, 9, 37, 1, 53, -5, 53, 0, 0],
                       [5, 4, 3, 2, 3, 5, 9, 16, 30, 2, 20, 16, 3, 50, 0, 0]], np.int32)
    clamped = mz.clamp_rows(rows, b, CANVAS[0], CANVAS[1], o0, o1)
    assert clamped[0].tolist() == [0, 5, 2, 3, 1, o1 - 1, 37, 37, 1, 30, 53, 53, 50, 53, 0, 0]
    assert clamped[1].tolist() == [5, 0, 5, 0, o0 - 1, 1, 1, 37, 9, 37, 1, 53, 1, 53, 0, 0]
    assert clamped[2].tolist() == rows[2].tolist()
    for kind in KINDS:
      got = run_rows(dev, rows, out_size, kind)
      assert torch.equal(got, run_rows(dev, clamped, out_size, kind)), (out_size, kind)
      assert_equal(got, mr.mosaic_from_rows(raw, rows, out_size, kind), ('out of range', out_size, kind))
      assert float(got.max()) <= 200, 'a sentinel byte was read'


@pytest.mark.gpu
def test_host_checks():
  dev = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device='cuda')
  rows = torch.zeros((1, 16), dtype=torch.int32, device='cuda')
  out = torch.empty((1, 4, 4, 3), dtype=torch.uint8, device='cuda')
  f = torch.zeros(64, dtype=torch.float32, device='cuda')
  i = torch.zeros(8, dtype=torch.int32, device='cuda')
  s = torch.cuda.current_stream().cuda_stream
  d, r, o = dev.data_ptr(), rows.data_ptr(), out.data_ptr()
  for args, what in (((None, 2, 4, 4, r, 1, o, 4, 4, _lib.EDET_U8, s), 'null'),
                     ((d, 2, 4, 4, r, 1, None, 4, 4, _lib.EDET_U8, s), 'null'),
                     ((d, 0, 4, 4, r, 1, o, 4, 4, _lib.EDET_U8, s), 'batch 0'),
                     ((d, 2, 4, 4, r, 0, o, 4, 4, _lib.EDET_U8, s), 'groups 0'),
                     ((d, 2, 4, 4, r, 65536, o, 4, 4, _lib.EDET_U8, s), 'groups 65536'),
                     ((d, 2, 4, 4, r, 1, o, 1, 4, _lib.EDET_U8, s), 'output 1 x 4'),
                     ((d, 2, 4, 4, r, 1, o, 4, 1, _lib.EDET_U8, s), 'output 4 x 1'),
                     ((d, 2, 30000, 30000, r, 1, o, 4, 4, _lib.EDET_U8, s), 'too large'),
                     ((d, 2, 4, 4, r, 1, o, 4, 4, _lib.EDET_BF16, s), 'bad out_dtype')):
    with pytest.raises(_lib.EdetError, match=what):
      _lib.call('edet_mosaic', *args)
  fp, ip = f.data_ptr(), i.data_ptr()
  for args, what in (((None, fp, ip, 2, 1, r, 1, 4, 4, fp, fp, ip, s), 'null'),
                     ((fp, fp, ip, 2, 0, r, 1, 4, 4, fp, fp, ip, s), 'max_boxes 0'),
                     ((fp, fp, ip, 2, 1, r, 1, 4, 1, fp, fp, ip, s), 'output 4 x 1'),
                     ((fp + 4, fp, ip, 2, 1, r, 1, 4, 4, fp, fp, ip, s), '16-byte aligned')):
    with pytest.raises(_lib.EdetError, match=what):
      _lib.call('edet_mosaic_boxes', *args)
  with pytest.raises(ValueError, match='empty sub-image'):
    mz.mosaic_images(dev, [[0, 1, 0, 1]], [[0, 2]], (4, 4))


def raw_boxes(rng, b, m):
  y0, x0 = rng.uniform(0.0, 0.6, (b, m)), rng.uniform(0.0, 0.6, (b, m))
  boxes = np.stack([y0, x0, y0 + rng.uniform(0.15, 0.4, (b, m)), x0 + rng.uniform(0.15, 0.4, (b, m))], -1).astype(np.float32)
  return boxes, rng.integers(1, 91, (b, m)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('counts', [[0] * 6, [3] * 6, [3, 0, 1, 2, 0, 3]], ids=['none', 'full', 'mixed'])
def test_box_kernel_equals_the_restatement(counts):
  """M = 3: the rows past a source's count hold a value that must never appear; padding is -1."""
  rng = np.random.default_rng(11)
  boxes, classes = raw_boxes(rng, 6, 3)
  for k, n in enumerate(counts):
    boxes[k, n:], classes[k, n:] = 777.0, 777.0
  out_size = (7, 10)
  rows = mz.mosaic_rows(INDEX, points_for(*out_size), SIZES)
  want = mr.batch_boxes(boxes, classes, counts, rows, out_size)
  ob = torch.full((5, 12, 4), 5.0, device='cuda')
  oc = torch.full((5, 12), 5.0, device='cuda')
  on = torch.full((5,), 5, dtype=torch.int32, device='cuda')
  mz.launch_boxes(torch.from_numpy(boxes).cuda(), torch.from_numpy(classes).cuda(),
                  torch.tensor(counts, dtype=torch.int32, device='cuda'), torch.from_numpy(rows).cuda(), out_size, ob, oc, on,
                  torch.cuda.current_stream().cuda_stream)
  torch.cuda.synchronize()
  assert_equal(ob, want[0], 'boxes')
  assert_equal(oc, want[1], 'classes')
  assert_equal(on, want[2], 'counts')
  assert not (ob == 777).any() and not (oc == 777).any()
  assert want[2].tolist() == [sum(counts[i] for i in r) for r in INDEX]


@pytest.mark.gpu
def test_mosaic_batch_equals_its_pieces_and_draws_from_the_generator():
  raw = canvas_batch(12)
  sizes = np.asarray(SIZES, np.int32)
  rng = np.random.default_rng(13)
  boxes, classes = raw_boxes(rng, 6, 3)
  counts = np.asarray([3, 0, 1, 2, 0, 3], np.int32)
  out_size = (16, 20)
  images, ob, oc, on = mz.mosaic_batch((raw, sizes), boxes, classes, counts, out_size, rng=np.random.default_rng(4))
  index, points = mz.mosaic_draws(np.random.default_rng(4), 6, 6, out_size)
  rows = mz.mosaic_rows(index, points, sizes)
  assert images.dtype == torch.uint8 and tuple(images.shape) == (6, 16, 20, 3) and tuple(ob.shape) == (6, 12, 4)
  assert_equal(images, mr.mosaic_from_rows(raw, rows, out_size, 'u8'), 'mosaic_batch images')
  want = mr.batch_boxes(boxes, classes, counts, rows, out_size)
  assert_equal(ob, want[0], 'boxes')
  assert_equal(oc, want[1], 'classes')
  assert_equal(on, want[2], 'counts')
  f32 = mz.mosaic_batch((raw, sizes), boxes, classes, counts, out_size, draws=(index, points), out_dtype='f32')[0]
  assert_equal(f32, mr.mosaic_from_rows(raw, rows, out_size, 'f32'), 'mosaic_batch f32')
  g, same = np.random.default_rng(1), np.random.default_rng(1)
  with pytest.raises(ValueError, match='outside'):      # sizes are checked before the generator moves
    mz.mosaic_batch((raw, sizes + 40), boxes, classes, counts, out_size, rng=g)
  assert g.random() == same.random()


@pytest.mark.gpu
def test_mosaic_batch_feeds_train_step_raw():
  """The smallest detector case of tests/test_det_input.py (efficientdet-d0 at 128 x 128, three raw images of 40 x 56, 8 box
  rows): mosaic_batch's output goes into train_step_raw as it is and gives the step that the same tensors, built from the
  restatement on the host, give."""
  from automl_amd import det_input
  from tests import test_det_input as tdi
  (raw, boxes, classes, counts), draws = tdi.batches(False, steps=1)[0]
  out_size = (48, 64)
  index, points = mz.mosaic_draws(np.random.default_rng(21), tdi.BATCH, tdi.BATCH, out_size)
  config = tdi.make_config(False, ',max_instances_per_image=%d' % (4 * tdi.MAX_BOXES))
  got_data = mz.mosaic_batch(raw, boxes, classes, counts, out_size, draws=(index, points))
  rows = mz.mosaic_rows(index, points, [[tdi.RAW_H, tdi.RAW_W]] * tdi.BATCH)
  hand = (mr.mosaic_from_rows(raw, rows, out_size, 'u8'),) + mr.batch_boxes(boxes, classes, counts, rows, out_size)
  assert int(hand[3].sum()) > 0 and (hand[3] <= 4 * tdi.MAX_BOXES).all()
  results = []
  for data in (got_data, hand):
    net = tdi.new_net(config, 'f32', False)
    results.append(tdi.snapshot(net, [net.train_step_raw(data, draws=det_input.Draws(draws.flip, draws.scale, None))]))
  assert all(np.isfinite(v[k]) for v in results[0][0] for k in tdi.KEYS) and results[0][0][0]['cls_loss'] > 0
  tdi.assert_same(results[0], results[1], 'mosaic_batch -> train_step_raw')
