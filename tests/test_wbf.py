"""Weighted box fusion (automl_amd/wbf.py on edet_wbf_cluster / edet_wbf_order, csrc/wbf.hip) and the flip test-time
augmentation of EfficientDetModel.detect_flip_tta.

CPU: the numpy restatement tests/wbf_ref.py equals tests/golden/reference_wbf.npz -- the reference's tf2/wbf.py executed on the
torch stand-in, clusters of at most two members -- bit for bit, and it and the four torch helpers give the known answers of the
reference's own wbf_test.py (:24-142).  GPU: the kernels equal the restatement bit for bit (uint32 views: the sign of a zero
counts, the padding cluster's coordinates are -0.0)."""
import os

import numpy as np
import pytest
import torch

from automl_amd import _lib, build, wbf
from tests import gpu_util as gu
from tests import wbf_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'reference_wbf.npz')
F = np.float32
CANARY = 64


def bits(a):
  return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def same_bits(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.dtype == b.dtype == F and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def close(a, b):      # tf.test.TestCase.assertAllClose's defaults
  return np.allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------ CPU
def test_restatement_equals_the_executed_reference():
  g = np.load(GOLDEN)
  names = [str(n) for n in g['names']]
  assert len(names) >= 12 and str(g['nan_cases']) == 'included'
  assert {int(g[n + '/num_models']) for n in names} == {1, 2, 3}
  for n in names:
    got = wr.ensemble_detections({'num_classes': int(g[n + '/num_classes'])}, g[n + '/detections'], int(g[n + '/num_models']))
    assert same_bits(got, g[n + '/out']), n
  # what the fixture holds: the padded shape with its -0.0 coordinates and the cluster of dummies last
  pad = g['padded/out']
  assert pad[-1, 6] == 0 and pad[-1, 5] == F(-1e5) and np.array_equal(bits(pad[-1, 1:5]), bits(np.full(4, -0.0, F)))
  one = g['padded_one/out']
  assert one[-1, 5] == F(-5e4) and np.array_equal(bits(one[-1, 1:5]), bits(np.full(4, -0.0, F)))
  assert len(g['threshold/out']) == 3      # IoU 0.55f joins, 0.545 founds
  assert sum(len(g[n + '/out']) < len(g[n + '/detections']) for n in names) >= 10


IOU_CASES = [      # wbf_test.py:24-69
    ([[1, 1, 1, 3, 3, 1, 1]], [1, 1, 1, 3, 3, 1, 1], [1.0]),
    ([[1, 1, 1, 3, 3, 1, 1]], [1, 2, 2, 4, 4, 1, 1], [1.0 / 7.0]),
    ([[1, 1, 1, 3, 2, 1, 1]], [1, 2, 1, 4, 2, 1, 1], [1.0 / 3.0]),
    ([[1, 1, 1, 3, 3, 1, 1]], [1, 3, 3, 5, 5, 1, 1], [0.0]),
    ([[1, 1, 1, 3, 3, 1, 1], [1, 2, 2, 4, 4, 1, 1], [1, 3, 3, 5, 5, 1, 1]], [1, 1, 1, 3, 3, 1, 1], [1, 1.0 / 7.0, 0]),
]
ENSEMBLE_IN = [[1, 2, 1, 10, 1, 0.75, 1], [1, 3, 1, 10, 1, 0.75, 1], [1, 3, 1, 10, 1, 1, 2]]
ENSEMBLE_OUT = [[1, 2.5, 1, 10, 1, 0.75, 1], [1, 3, 1, 10, 1, 0.5, 2]]


def t32(x):
  return torch.tensor(x, dtype=torch.float32)


def known_answers(mod, conv, back):
  """The assertions of wbf_test.py on module `mod`; conv makes its tensors, back returns numpy."""
  for clusters, det, want in IOU_CASES:
    iou = back(mod.vectorized_iou(conv(clusters), conv(det)))
    assert iou.shape == (len(clusters), 1) and close(iou.reshape(-1), want)
  match, other, box = conv([1, 1, 1, 2, 2, 1, 1]), conv([1, 3, 3, 2, 2, 1, 1]), conv([1, 1, 1, 2, 2, 1, 1])
  assert mod.find_matching_cluster((match, other), box) == 0 and mod.find_matching_cluster((other, match), box) == 1
  over, better, box = conv([1, 1, 1, 11, 2, 1, 1]), conv([1, 2, 1, 12, 2, 1, 1]), conv([1, 3, 1, 13, 2, 1, 1])
  assert mod.find_matching_cluster((over,), box) == 0 and mod.find_matching_cluster((over, better), box) == 1
  assert mod.find_matching_cluster([], box) == -1 and mod.find_matching_cluster((other,), box) == -1
  samples = conv([1, 3])
  assert close(back(mod.weighted_average(samples, conv([0.5, 0.5]))), 2)
  assert close(back(mod.weighted_average(samples, conv([1, 0]))), 1)
  assert close(back(mod.weighted_average(samples, conv([1, 2]))), 7.0 / 3.0)
  d1, d2 = conv([1, 1, 1, 2, 2, 0.3, 1]), conv([1, 3, 3, 4, 4, 0.7, 1])
  assert close(back(mod.average_detections((d1, d2), 1)), [1, 2.4, 2.4, 3.4, 3.4, 0.5, 1])
  assert close(back(mod.average_detections((d1, d2), 3)), [1, 2.4, 2.4, 3.4, 3.4, 0.333333, 1])
  assert close(back(mod.average_detections((d2,), 2)), [1, 3, 3, 4, 4, 0.35, 1])
  assert back(mod.average_detections((d1, d2), 1)).shape == (7,)


def test_reference_known_answers_hold_for_the_restatement():
  known_answers(wr, lambda x: np.asarray(x, F), lambda x: np.asarray(x))
  got = wr.ensemble_detections({'num_classes': 3}, np.asarray(ENSEMBLE_IN, F), 2)
  assert close(got, ENSEMBLE_OUT) and got.dtype == F


def test_reference_known_answers_hold_for_the_torch_helpers():
  known_answers(wbf, t32, lambda x: x.numpy())
  # and the helpers are the restatement's arithmetic: a cluster of three, sums left to right
  rows = np.asarray([[4, 1.1, 2.3, 10.7, 11.9, 0.3, 2], [4, 1.4, 2.1, 10.2, 12.3, 0.7, 2], [4, 0.9, 2.6, 10.4, 11.1, 0.45, 2]], F)
  for nm in (1, 2, 3, 5):
    assert same_bits(wbf.average_detections(torch.from_numpy(rows), nm).numpy(), wr.average_detections(list(rows), nm))
  assert same_bits(wbf.vectorized_iou(torch.from_numpy(rows), torch.from_numpy(rows[1])).numpy(), wr.vectorized_iou(rows, rows[1]))
  flat = np.asarray([[0, 0, 0, 0, 0, -1e5, 0], [0, 5, 5, 9, 9, 0.5, 0]], F)      # a NaN IoU is the maximum, wherever it stands
  for order in ([0, 1], [1, 0]):
    assert wbf.find_matching_cluster(torch.from_numpy(flat[order]), torch.from_numpy(flat[0])) == order.index(0)
    assert wr.find_matching_cluster(list(flat[order]), flat[0]) == order.index(0)


def test_entry_points_and_stubs_are_in_step():
  header = open(os.path.join(ROOT, 'include', 'edet_hip.h')).read()
  stubs = open(os.path.join(ROOT, 'automl_amd', 'csrc', 'plan_stubs.inc')).read()
  for name in ('edet_wbf_cluster', 'edet_wbf_order'):
    assert name in _lib.SIGNATURES and 'int %s(' % name in header and '"%s"' % name in stubs
  assert len(_lib.SIGNATURES['edet_wbf_cluster']) == 9 and len(_lib.SIGNATURES['edet_wbf_order']) == 7
  assert 'wbf.hip' in build.SOURCES and build.EXTRA_FLAGS['wbf.hip'] == ['-ffp-contract=off']
  assert wbf.MAX_ROWS == 1024 and '#define EDET_WBF_MAX_ROWS 1024' in header
  assert wbf.IOU_THRESHOLD == wr.IOU_THRESHOLD == 0.55
  # the kernel's float32 constant decides exactly as the double does: no float32 lies between them
  assert float(F(0.55)) > 0.55 > float(np.nextafter(F(0.55), F(0)))


def test_refusals():
  p = {'num_classes': 3}
  with pytest.raises(ValueError, match='1025 rows'):
    wbf.ensemble_detections_batch(p, np.zeros((1, 1025, 7), F), 2)
  with pytest.raises(ValueError, match='1025 rows'):
    wbf.ensemble_detections(p, np.zeros((1025, 7), F), 2)
  with pytest.raises(ValueError, match='num_models'):
    wbf.ensemble_detections_batch(p, np.zeros((1, 4, 7), F), 0)
  with pytest.raises(ValueError, match='num_models'):
    wbf.ensemble_detections(p, np.zeros((4, 7), F), 0)
  with pytest.raises(ValueError, match='float32'):
    wbf.ensemble_detections_batch(p, np.zeros((1, 4, 7), np.float64), 2)
  with pytest.raises(ValueError, match='float32'):
    wbf.ensemble_detections_batch(p, np.zeros((1, 4, 6), F), 2)


def test_ensemble_refuses_to_run_without_gpu():
  if torch.cuda.is_available():
    return
  with pytest.raises(_lib.EdetError, match='no CPU'):
    wbf.ensemble_detections({'num_classes': 3}, np.asarray(ENSEMBLE_IN, F), 2)
  with pytest.raises(_lib.EdetError, match='no CPU'):
    wbf.ensemble_detections_batch({'num_classes': 3}, torch.tensor([ENSEMBLE_IN], dtype=torch.float32), 2)


# ------------------------------------------------------------------------------------ the cases
def row(x1, y1, x2, y2, score, cls, image_id=0):
  return [image_id, x1, y1, x2, y2, score, cls]


def case_random():
  """B = 3, N = 48, 4 classes, counts 48, 31, 0: jittered copies of six base boxes, scores multiples of 1/8 (ties in the final
  order), classes from -1 .. 4 and one 1.5 (dropped rows)."""
  rng = np.random.default_rng(4801)
  base = np.array([[10, 10, 60, 50], [100, 20, 180, 90], [30, 120, 70, 200], [200, 200, 260, 230], [300, 10, 340, 100],
                   [150, 150, 190, 190]], F)
  det = np.zeros((3, 48, 7), F)
  for i in range(3):
    src = rng.integers(0, 6, 48)
    det[i, :, 0] = 11 + i
    det[i, :, 1:5] = base[src] + rng.uniform(-5, 5, (48, 4)).astype(F)
    det[i, :, 5] = rng.integers(1, 9, 48) / 8.0
    det[i, :, 6] = rng.choice([-1, 0, 1, 2, 3, 4], 48, p=[.05, .2, .25, .25, .2, .05])
  det[0, 17, 6] = 1.5
  return det, [48, 31, 0], 4


def case_lanes():
  """One image, one class, N = 80: 70 pairwise disjoint boxes (70 clusters: a second slot in lanes 0..5), then ten copies of
  rows 3, 63, 64 and 69, shifted by at most 1.5 of 10 pixels, so that each matches exactly that cluster."""
  rng = np.random.default_rng(80)
  rows = [row(20.0 * i, 0, 20.0 * i + 10, 10, rng.integers(1, 9) / 8.0, 0) for i in range(70)]
  for k, src in enumerate([3, 63, 64, 69, 64, 3, 69, 63, 64, 69]):
    dx, dy = 0.5 + 0.5 * (k % 3), 1.0 * (k % 2)
    rows.append(row(20.0 * src + dx, dy, 20.0 * src + 10 + dx, 10 + dy, rng.uniform(0.1, 0.9), 0))
  return np.asarray([rows], F), None, 1


def case_tie(a_first):
  """Cluster A = [0, 0, 10, 10] and cluster B = [4, 0, 14, 10] (IoU 60 / 140: apart), 66 disjoint clusters between them, then
  D = [2, 0, 12, 10] with IoU 80 / 120 with both: the two maxima sit in slot 0 of lane 0 and slot 1 of lane 3, and D joins
  the one with the lower index."""
  a, b = row(0, 0, 10, 10, .5, 1), row(4, 0, 14, 10, .75, 1)
  fill = [row(100 + 20.0 * i, 0, 110 + 20.0 * i, 10, .25, 1) for i in range(66)]
  first, second = (a, b) if a_first else (b, a)
  return np.asarray([[first] + fill + [second, row(2, 0, 12, 10, .625, 1)]], F), None, 2


def case_padded():
  """The reference's padded shape, B = 2: the plain pass's real rows (classes 1 and 2) and its -1e5 dummies, then the mirrored
  pass's.  Image 0 has six dummies, image 1 one."""
  dummy = lambda i: [i, 0, 0, 0, 0, -1e5, 0]
  im0 = [row(10, 10, 50, 60, .8, 1, 3), row(100, 100, 150, 160, .5, 2, 3), row(200, 10, 240, 40, .4, 1, 3)] + [dummy(3)] * 3 + \
        [row(12, 9, 51, 62, .6, 1, 3), row(98, 101, 149, 161, .7, 2, 3), row(300, 300, 340, 340, .4, 2, 3)] + [dummy(3)] * 3
  im1 = [row(10, 10, 50, 60, .8, 1, 4), row(100, 100, 150, 160, .5, 2, 4), row(200, 10, 240, 40, .4, 1, 4),
         row(5, 200, 45, 260, .3, 2, 4), row(60, 200, 90, 260, .3, 1, 4), row(120, 200, 150, 260, .2, 1, 4)] + \
        [row(12, 9, 51, 62, .6, 1, 4), row(98, 101, 149, 161, .7, 2, 4), row(300, 300, 340, 340, .4, 2, 4),
         row(6, 201, 44, 262, .9, 2, 4), row(61, 199, 91, 261, .1, 1, 4), dummy(4)]
  return np.asarray([im0, im1], F), None, 3


def case_full():
  """N = 1024 rows of one class on a 32 x 32 grid, pairwise disjoint: 1024 clusters, every slot of every lane."""
  rng = np.random.default_rng(1024)
  i = np.arange(1024)
  x, y = 20.0 * (i % 32), 20.0 * (i // 32)
  det = np.stack([np.full(1024, 2.0), x, y, x + 10, y + 10, rng.integers(1, 33, 1024) / 32.0, np.ones(1024)], 1)
  return det.astype(F)[None], None, 2


CASES = {'random': case_random, 'lanes': case_lanes, 'tie_a': lambda: case_tie(True), 'tie_b': lambda: case_tie(False),
         'padded': case_padded, 'full': case_full}
_CACHE = {}


def case(name, num_models=2):
  """(detections, counts, num_classes, the restatement's (fused, fused_counts)), made once and left unchanged."""
  key = (name, num_models)
  if key not in _CACHE:
    det, counts, nc = CASES[name]()
    _CACHE[key] = (det, counts, nc, wr.ensemble_detections_batch({'num_classes': nc}, det, num_models, counts))
  return _CACHE[key]


def test_cases_hold_what_they_must():
  det, counts, nc, (fused, n) = case('random')
  assert det.shape == (3, 48, 7) and n[2] == 0 and 6 <= n[1] < n[0] < 40 and not fused[2].any()
  assert set(fused[0, :n[0], 6].tolist()) == {0.0, 1.0, 2.0, 3.0}      # -1, 1.5 and 4 are dropped
  assert {-1.0, 4.0, 1.5} <= set(det[0, :, 6].tolist())
  sc = fused[0, :n[0], 5]
  assert np.all(np.diff(sc) <= 0) and np.count_nonzero(np.diff(sc) == 0) >= 3      # ties in the final order
  assert not np.array_equal(case('random', 3)[3][0], fused)
  det, _, _, (fused, n) = case('lanes')
  assert det.shape == (1, 80, 7) and n[0] == 70      # the ten copies found nothing
  assert np.count_nonzero(fused[0, :70, 1] % 20 != 0) == 4      # and move the averages of exactly four clusters
  for name, x1 in (('tie_a', 0), ('tie_b', 4)):
    det, _, _, (fused, n) = case(name)
    assert det.shape == (1, 69, 7) and n[0] == 68
    iou = wr.vectorized_iou(det[0, [0, 67]], det[0, 68]).reshape(-1)
    assert iou[0] == iou[1] == F(80) / F(120) and wr.vectorized_iou(det[0, [0]], det[0, 67])[0, 0] == F(60) / F(140)
    merged = fused[0, :68][fused[0, :68, 1] != np.round(fused[0, :68, 1])]
    assert len(merged) == 1 and min(x1, 2) < merged[0, 1] < max(x1, 2)      # D joined the cluster that came first
    assert (fused[0, :68, 1] == 4 - x1).any()                                # and the other one stands as it was
  det, _, _, (fused, n) = case('padded')
  assert n.tolist() == [5, 8]
  for i, (members, score) in enumerate([(6, -1e5), (1, -5e4)]):
    last = fused[i, n[i] - 1]
    assert last[6] == 0 and last[5] == F(score) and np.array_equal(bits(last[1:5]), bits(np.full(4, -0.0, F))) and last[0] == 3 + i
    assert (fused[i, :n[i] - 1, 6] > 0).all()
  assert case('full')[3][1][0] == 1024


# ------------------------------------------------------------------------------------ GPU
def run(det, counts, nc, num_models):
  fused, n = wbf.ensemble_detections_batch({'num_classes': nc}, det, num_models, counts)
  assert fused.is_cuda and n.is_cuda and fused.dtype == torch.float32 and n.dtype == torch.int32
  return fused.cpu().numpy(), n.cpu().numpy()


def assert_equals_ref(got, want, what):
  assert np.array_equal(got[1], want[1]), (what, got[1].tolist(), want[1].tolist())
  assert same_bits(got[0], want[0]), (what, int((bits(got[0]) != bits(want[0])).sum()))


@pytest.mark.gpu
def test_ensemble_boxes_on_the_device():
  """wbf_test.py test_ensemble_boxes through the kernels: d1 and d2 have no area, their IoU is 0 / 0."""
  rows = np.asarray(ENSEMBLE_IN, F)
  got = wbf.ensemble_detections({'num_classes': 3}, rows, 2)
  assert got.is_cuda and tuple(got.shape) == (2, 7)
  got = got.cpu().numpy()
  assert close(got, ENSEMBLE_OUT)
  assert same_bits(got, wr.ensemble_detections({'num_classes': 3}, rows, 2))
  empty = wbf.ensemble_detections({'num_classes': 1}, rows, 2)      # no row of class 0: where tf.stack([]) raises
  assert tuple(empty.shape) == (0, 7)


@pytest.mark.gpu
@pytest.mark.parametrize('num_models', [2, 3])
def test_random_batch(num_models):
  det, counts, nc, want = case('random', num_models)
  assert_equals_ref(run(det, counts, nc, num_models), want, 'random')
  got = run(det, torch.tensor(counts, dtype=torch.int64), nc, num_models)      # counts as a tensor of another integer type
  assert_equals_ref(got, want, 'random, tensor counts')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['lanes', 'tie_a', 'tie_b', 'padded', 'full'])
def test_kernels_equal_restatement(name):
  det, counts, nc, want = case(name)
  assert_equals_ref(run(det, counts, nc, 2), want, name)


def canaried(shape, dtype, fill, canary):
  """A flat device buffer with CANARY elements in front of and behind the body -> (the whole buffer, the body's view)."""
  n = int(np.prod(shape))
  buf = torch.full((n + 2 * CANARY,), canary, dtype=dtype, device=gu.DEV)
  buf[CANARY:CANARY + n] = fill
  return buf, buf[CANARY:CANARY + n].view(shape)


class _Calls(object):
  def __init__(self):
    self.calls = []

  def on_call(self, name, args):
    self.calls.append((name, args))


@pytest.mark.gpu
def test_device_resident_input_canaries_and_run_to_run_bits(monkeypatch):
  det, counts, nc, want = case('random')
  dd = torch.from_numpy(det).to(gu.DEV)
  dc = torch.tensor(counts, dtype=torch.int32, device=gu.DEV)
  rec = _Calls()
  monkeypatch.setattr(_lib, 'recorder', rec)
  fused, n = wbf.ensemble_detections_batch({'num_classes': nc}, dd, 2, dc)
  monkeypatch.setattr(_lib, 'recorder', None)
  assert [c[0] for c in rec.calls] == ['edet_wbf_cluster', 'edet_wbf_order']      # two launches of the library
  assert rec.calls[0][1][0] == dd.data_ptr() and rec.calls[0][1][1] == dc.data_ptr()      # read in place
  assert rec.calls[1][1][4] == fused.data_ptr() and rec.calls[1][1][5] == n.data_ptr()
  assert_equals_ref((fused.cpu().numpy(), n.cpu().numpy()), want, 'device tensors')
  b, rows = det.shape[:2]
  runs = []
  for _ in range(2):
    sc_b, scratch = canaried((b, rows, 7), torch.float32, 123.0, 777.25)
    fl_b, flags = canaried((b, rows), torch.int32, 0, 0x1234567)
    fu_b, out = canaried((b, rows, 7), torch.float32, 123.0, 777.25)
    cn_b, cnt = canaried((b,), torch.int32, 0x55, 0x1234567)
    wbf.launch_cluster(dd, dc, nc, 2, scratch, flags, gu.stream())
    wbf.launch_order(scratch, flags, out, cnt, gu.stream())
    torch.cuda.synchronize()
    for buf, body, canary in ((sc_b, scratch, 777.25), (fl_b, flags, 0x1234567), (fu_b, out, 777.25), (cn_b, cnt, 0x1234567)):
      assert bool((buf[:CANARY] == canary).all()) and bool((buf[CANARY + body.numel():] == canary).all())
    runs.append((out.cpu().numpy(), cnt.cpu().numpy(), flags.cpu().numpy()))
  assert all(x.tobytes() == y.tobytes() for x, y in zip(runs[0], runs[1]))
  assert_equals_ref(runs[0][:2], want, 'canaried')
  assert np.array_equal(dd.cpu().numpy(), det) and dc.cpu().tolist() == counts      # the inputs are not written


@pytest.mark.gpu
@pytest.mark.parametrize('pyfunc', [False, True])
def test_detect_flip_tta_equals_the_chain_by_hand(monkeypatch, pyfunc):
  """efficientdet-d0 at 128 x 128, random weights, two raw 96 x 128 uint8 images (padded below), image ids 7 and 9.  The level
  outputs of the model's own two forward passes are cloned as they are returned (two passes over one input need not agree in
  every bit), and the chain is assembled from them by hand: generate_detections for the plain and for the flipped input,
  concatenated, fused by tests/wbf_ref.py on the host.  pyfunc: the configuration's per-class NMS, whose padding rows are
  zeros, and the numpy NMS with its -1e5 dummies.  A cluster of zero-score padding rows has 0 / 0 coordinates, whose NaN
  carries another sign on the host than on the device: NaNs must stand in the same places, every other value is compared bit
  for bit, and with pyfunc=True there is no NaN."""
  from automl_amd import efficientdet_net, hparams_config, postprocess as pp, preprocess
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  config.override('image_size=128')
  config.nms_configs.pyfunc = pyfunc
  params = config.as_dict()
  raw = torch.from_numpy(np.random.default_rng(77).integers(0, 256, (2, 96, 128, 3)).astype(np.uint8))
  model = efficientdet_net.EfficientDetModel(config=config, dtype='f32', seed=5)
  passes = []
  inner = efficientdet_net.EfficientDetNet.__call__

  def recording(self, inputs, training=False):
    cls, box = inner(self, inputs, training)
    passes.append((inputs.clone(), [c.clone() for c in cls], [b.clone() for b in box]))
    return cls, box
  monkeypatch.setattr(efficientdet_net.EfficientDetNet, '__call__', recording)
  fused, counts = model.detect_flip_tta(raw, image_ids=[7, 9])
  monkeypatch.setattr(efficientdet_net.EfficientDetNet, '__call__', inner)
  m = config.nms_configs.max_output_size
  assert tuple(fused.shape) == (2, 2 * m, 7) and tuple(counts.shape) == (2,) and counts.dtype == torch.int32
  assert len(passes) == 2
  images, scales = preprocess.preprocess_infer(raw, config.image_size, config.mean_rgb, config.stddev_rgb)
  assert torch.equal(passes[0][0], images) and torch.equal(passes[1][0], images.flip(2))      # the padded input is flipped
  assert bool((images[:, 96:] == 0).all()) and bool((images[:, :96] != 0).any())
  ids = torch.tensor([7, 9])
  plain = pp.generate_detections(params, passes[0][1], passes[0][2], scales, ids)
  mirrored = pp.generate_detections(params, passes[1][1], passes[1][2], scales, ids, flip=True)
  both = torch.cat([plain, mirrored], 1).cpu().numpy()
  want, want_n = wr.ensemble_detections_batch(params, both, 2)
  got, got_n = fused.cpu().numpy(), counts.cpu().numpy()
  assert np.array_equal(got_n, want_n) and want_n.min() > 0
  nan = np.isnan(want)
  assert not (pyfunc and nan.any())
  assert np.array_equal(np.isnan(got), nan)
  assert np.array_equal(np.where(nan, 0, bits(got)), np.where(nan, 0, bits(want)))
  for i in range(2):
    assert set(got[i, :got_n[i], 0].tolist()) == {[7.0, 9.0][i]} and not got[i, got_n[i]:].any()
