"""COCO AP on the device (automl_amd/coco_metric.py on edet_coco_match / edet_coco_accumulate, csrc/coco_eval.hip): the
update_state bookkeeping and the numpy restatement tests/coco_ref.py on the CPU; the kernels against the restatement, bit for
bit, on the GPU.

Oracle status: pycocotools is not installed, and nothing here was ever compared with a run of it.  The restatement is pinned by
the known answers of the reference's own test (efficientdet/coco_metric_test.py:39-48) and by one case derived by hand below;
the kernels are pinned by the restatement.  The 12 statistics of the two pinned cases are compared as the float32 values
result() returns: in float64 COCOeval's own precision 1 / ((0 + 1) + np.spacing(1)) is 0.9999999999999998, not 1, so the
float64 means sit a few units in the last place off 2/3 and 1 (the restatement gives 0.6666666666666665 and
0.9999999999999998); every figure that is exact in float64 is compared in float64 as well."""
import json
import os

import numpy as np
import pytest
import torch

from automl_amd import _lib, build, coco_metric as cm
from tests import coco_ref as cr
from tests import gpu_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 64


def G(y1, x1, y2, x2, crowd, cls):
  """A ground-truth row; column 5 (area) is wrong on purpose: update_state recomputes it."""
  return [y1, x1, y2, x2, crowd, -5.0, cls]


def Dt(x, y, w, h, score, cls, image_id=-1):
  return [image_id, x, y, w, h, score, cls]


PAD_G = [0, 0, 0, 0, 0, 0, -1]
PAD_D = [-1, 0, 0, 0, 0, 0, -1]


def padded(images, rows, pad):
  return np.array([list(im) + [pad] * (rows - len(im)) for im in images], np.float32)


def ref_of(metric, n_labels=0):
  """The restatement on the metric's packed state (packed on the host)."""
  ids, dt, gt, cats = metric.packed_state('cpu')
  out = cr.evaluate(dt.numpy(), gt.numpy(), cats.numpy(), n_labels)
  out.update(ids=ids, dt=dt.numpy(), gt=gt.numpy(), cats=cats.numpy())
  return out


# ------------------------------------------------------------------------------------ CPU
def test_entry_points_and_stubs_are_in_step():
  header = open(os.path.join(ROOT, 'include', 'edet_hip.h')).read()
  stubs = open(os.path.join(ROOT, 'automl_amd', 'csrc', 'plan_stubs.inc')).read()
  for name in ('edet_coco_match', 'edet_coco_accumulate'):
    assert name in _lib.SIGNATURES and 'int %s(' % name in header and '"%s"' % name in stubs
  assert 'coco_eval.hip' in build.SOURCES and build.EXTRA_FLAGS['coco_eval.hip'] == ['-ffp-contract=off']
  assert cm.MAX_DETS_PER_IMAGE == 100 and cm.MAX_GTS_PER_IMAGE == 128
  assert '#define EDET_COCO_MAX_DETS 100' in header and '#define EDET_COCO_MAX_GTS 128' in header
  # both sides compare against identical doubles
  assert np.array_equal(cm.IOU_THRS, cr.IOU_THRS) and np.array_equal(cm.REC_THRS, cr.REC_THRS)
  assert cm.AREA_RNG == cr.AREA_RNG and cm.MAX_DETS == cr.MAX_DETS
  assert cm.IOU_THRS.dtype == np.float64 and cm.IOU_THRS[0] == 0.5 and cm.IOU_THRS[5] == 0.75


def test_metric_names():
  m = cm.EvaluationMetric()
  assert m.metric_names == ['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'ARmax1', 'ARmax10', 'ARmax100', 'ARs', 'ARm', 'ARl']
  assert m.metric_values is None and m.image_id == 1


def test_reference_known_answers():
  """coco_metric_test.py:26-48: AP 2/3, car 1, truck 1, bicycle 0; 12 + 3 values with the 3-entry label map."""
  gt = np.array([[[10.0, 10.0, 20.0, 20.0, 0.0, 100.0, 1], [10.0, 10.0, 30.0, 15.0, 0.0, 100.0, 2],
                  [30.0, 30.0, 40.0, 50.0, 0.0, 100.0, 3]]], np.float32)
  det = np.array([[[1.0, 10.0, 10.0, 10.0, 10.0, 0.6, 1], [1.0, 10.0, 10.0, 5.0, 20.0, 0.5, 2]]], np.float32)
  m = cm.EvaluationMetric(label_map={1: 'car', 2: 'truck', 3: 'bicycle'})
  m.update_state(gt, det)
  r = ref_of(m, n_labels=3)
  assert r['ids'] == [1] and r['cats'].tolist() == [1.0, 2.0, 3.0]
  want = [2 / 3, 2 / 3, 2 / 3, 2 / 3, -1, -1, 2 / 3, 2 / 3, 2 / 3, 2 / 3, -1, -1]
  assert r['result'].dtype == np.float32 and r['result'].shape == (15,)
  assert np.array_equal(r['result'], np.array(want + [1, 1, 0], np.float32)), r['result'].tolist()
  assert np.array_equal(r['stats'][6:], np.array(want[6:], np.float64))      # the recalls are exact in float64
  assert np.abs(r['stats'] - np.array(want)).max() <= 2 ** -52


def test_hand_derived_case():
  """One image, class 1.  Ground truths g0 = [0, 0, 10, 10] (area 100: small) and g1 = [20, 20, 60, 60] (area 1600: medium).
  By descending score: d0 = (50, 50, 5, 5) lies inside g1, IoU 25 / 1600: unmatched at every threshold; d1 = (0, 0, 10, 6)
  has IoU 60 / ((60 + 100) - 60) = 0.6 with g0 exactly: matched at 0.5, 0.55 and 0.6 only; d2 = g1, IoU 1: always matched.
    area all (npig 2), t <= 0.6: FP TP TP -> rc 0, 1/2, 1; pr 0, 1/2, 2/3 -> from the right 2/3 everywhere: AP_t = 2/3.
    the other seven t: FP FP TP -> rc 0, 0, 1/2; pr 0, 0, 1/3 -> 1/3 at the 51 recall thresholds <= 0.5, 0 at the other 50:
      AP_t = 51 / 303 = 17 / 101 = 0.16831683168316833.
    AP = (3 (2/3) + 7 (17/101)) / 10 = 0.31782178217821777; AP50 = 2/3; AP75 = 17/101.
    small (npig 1: g1 is ignored): d2 matches the ignored g1 and is ignored; t <= 0.6: FP TP -> pr 0, 1/2 -> 1/2; else FP FP
      -> 0: APs = 3 (1/2) / 10 = 0.15.  ARs = 3 / 10.
    medium (npig 1: g0 is ignored): d0 is unmatched with area 25 outside [1024, 9216]: ignored; d1 matches the ignored g0
      (t <= 0.6) or is unmatched with area 60: ignored; d2 TP -> APm = 1 (1 / (1 + 2^-52) in float64), ARm = 1.
    large: no ground truth: -1, -1.
    cap 1: d0 alone, recall 0.  caps 10 and 100: recall 1 at three t, 1/2 at seven: 0.65."""
  gt = np.array([[G(0, 0, 10, 10, 0, 1), G(20, 20, 60, 60, 0, 1), PAD_G]], np.float32)
  det = np.array([[Dt(50, 50, 5, 5, .9, 1), Dt(0, 0, 10, 6, .8, 1), Dt(20, 20, 40, 40, .7, 1), PAD_D]], np.float32)
  m = cm.EvaluationMetric()
  m.update_state(gt, det)
  r = ref_of(m)
  want = [0.31782178217821777, 2 / 3, 0.16831683168316833, 0.15, 1, -1, 0, 0.65, 0.65, 0.3, 1, -1]
  assert np.array_equal(r['result'], np.array(want, np.float32)), r['stats'].tolist()
  exact = [0, 2, 3, 5, 6, 7, 8, 9, 10, 11]      # every figure but the two that hold 1 / (1 + 2^-52)
  assert np.array_equal(r['stats'][exact], np.array(want, np.float64)[exact]), r['stats'].tolist()
  assert np.abs(r['stats'] - np.array(want)).max() <= 2 ** -51
  assert r['rank'].tolist() == [[0, 1, 2, -1]]
  assert r['matched'][0, 0].tolist() == [0, 0b111, 0x3ff, 0]      # d1: thresholds 0.5, 0.55, 0.6 only
  assert box_iou_is_exactly(0.6)


def box_iou_is_exactly(v):
  return cr.box_iou(np.array([0, 0, 10, 6], np.float32), np.array([0, 0, 10, 10], np.float32), False) == v and cr.IOU_THRS[2] <= v


def test_update_state_bookkeeping():
  gt = padded([[G(1, 2, 11, 22, 0, 4)], [G(0, 0, 5, 5, 0, 9)], [G(3, 1, 7, 9.5, 1, 2), G(0, 0, 1, 1, 0, -1), G(0, 0, 2, 2, 2.0, 6)]],
              3, PAD_G)
  det = padded([[Dt(0, 0, 1, 1, .5, 1)], [Dt(0, 0, 1, 1, .5, -1), Dt(0, 0, 1, 1, .5, -2)],
                [PAD_D, Dt(1, 2, 3, 4, .5, 0, image_id=-1), Dt(5, 6, 7, 8, .25, 3, image_id=77)]], 3, PAD_D)
  m = cm.EvaluationMetric()
  m.update_state(gt, det)
  # the second image has no kept row: no id is spent on it and its ground truth (class 9) is not added
  assert m.image_ids == [1, 2] and m.image_id == 3
  ids, dt, g, cats = m.packed_state()
  assert ids == [1, 2] and cats.tolist() == [2.0, 4.0, 6.0] and dt.shape == (2, 3, 6) and g.shape == (2, 3, 7)
  # x, y, w, h from y1, x1, y2, x2; the area recomputed in float32 (column 5 held -5); is_crowd as int() != 0
  assert g[0, 0].tolist() == [2, 1, 20, 10, 0, 200, 4]
  assert g[1, 0].tolist() == [1, 3, 8.5, 4, 1, 34, 2] and g[1, 1, 6] == -1 and g[1, 2].tolist() == [0, 0, 2, 2, 1, 4, 6]
  assert dt[1, 1].tolist() == [1, 2, 3, 4, .5, 0] and dt[1, 0, 5] == -1
  f = np.float32
  g32 = np.array([[G(f(0.1), f(0.2), f(7.3), f(9.7), 0, 1)]], f)
  m2 = cm.EvaluationMetric()
  m2.update_state(g32, np.array([[Dt(0, 0, 1, 1, .5, 1, image_id=5)]], f))
  m2.update_state(g32, np.array([[Dt(0, 0, 1, 1, .5, 1)]], f))      # image_id -1 takes the running id, now 2
  assert m2.image_ids == [5, 2] and m2.image_id == 3
  ids, dt, g, _ = m2.packed_state()
  assert ids == [2, 5]
  w, h = f(9.7) - f(0.2), f(7.3) - f(0.1)
  assert g[0, 0, 2] == w and g[0, 0, 3] == h and g[0, 0, 5] == w * h and (w * h).dtype == np.float32
  # result() is cached in metric_values until reset_states
  m2.metric_values = np.zeros(12, np.float32)
  assert m2.result() is m2.metric_values
  m2.reset_states()
  assert m2.metric_values is None and m2.image_ids == [] and m2.image_id == 1


def test_filename(tmp_path):
  data = {'images': [{'id': 7}, {'id': 3}, {'id': 9}],
          'categories': [{'id': 18, 'name': 'dog'}, {'id': 2, 'name': 'bicycle'}, {'id': 44, 'name': 'bottle'}],
          'annotations': [
              {'id': 1, 'image_id': 7, 'category_id': 18, 'bbox': [10.5, 20.0, 30.0, 40.25], 'area': 700.5, 'iscrowd': 0},
              {'id': 2, 'image_id': 7, 'category_id': 2, 'bbox': [0, 0, 50, 50], 'area': 1234.0, 'iscrowd': 1},
              {'id': 3, 'image_id': 3, 'category_id': 2, 'bbox': [1, 2, 3, 4], 'area': 11.0, 'iscrowd': 0},
              {'id': 4, 'image_id': 9, 'category_id': 44, 'bbox': [5, 5, 5, 5], 'area': 25.0, 'iscrowd': 0}]}
  path = tmp_path / 'instances.json'
  path.write_text(json.dumps(data))
  m = cm.EvaluationMetric(filename=str(path))
  junk = np.full((2, 2, 7), 3.0, np.float32)      # groundtruth_data is not read with a file
  m.update_state(junk, np.array([[Dt(0, 0, 1, 1, .5, 2, image_id=7)], [Dt(0, 0, 1, 1, .5, 18, image_id=3)]], np.float32))
  ids, dt, g, cats = m.packed_state()
  assert ids == [3, 7] and cats.tolist() == [2.0, 18.0, 44.0]      # the file's categories; image 9 has no detections
  assert g.shape == (2, 2, 7)
  assert g[0, 0].tolist() == [1, 2, 3, 4, 0, 11, 2] and g[0, 1, 6] == -1
  assert g[1, 0].tolist() == [10.5, 20, 30, 40.25, 0, 700.5, 18] and g[1, 1].tolist() == [0, 0, 50, 50, 1, 1234, 2]
  with pytest.raises(ValueError, match='image id 8'):
    m.update_state(junk[:1], np.array([[Dt(0, 0, 1, 1, .5, 2, image_id=8)]], np.float32))


def test_refusals():
  with pytest.raises(ValueError, match='not built'):
    cm.EvaluationMetric(testdev_dir='/tmp/testdev')
  m = cm.EvaluationMetric()
  with pytest.raises(ValueError, match='101 detection rows'):
    m.update_state(np.zeros((1, 3, 7), np.float32), np.zeros((1, 101, 7), np.float32))
  with pytest.raises(ValueError, match='129 ground-truth rows'):
    m.update_state(np.zeros((1, 129, 7), np.float32), np.zeros((1, 3, 7), np.float32))
  m.update_state(np.zeros((1, 128, 7), np.float32), np.ones((1, 100, 7), np.float32))      # at the limits: taken
  with pytest.raises(ValueError, match='float32'):
    m.update_state(np.zeros((1, 3, 7), np.float64), np.zeros((1, 3, 7), np.float32))
  d = cm.EvaluationMetric()
  for _ in range(2):
    d.update_state(np.array([[G(0, 0, 1, 1, 0, 1)]], np.float32), np.array([[Dt(0, 0, 1, 1, .5, 1, image_id=4)]], np.float32))
  with pytest.raises(ValueError, match=r'not distinct.*4'):
    d.packed_state()
  with pytest.raises(ValueError, match='not distinct'):
    d.result()


def test_evaluate_refuses_to_run_without_gpu():
  if torch.cuda.is_available():
    return
  m = cm.EvaluationMetric()
  m.update_state(np.array([[G(0, 0, 1, 1, 0, 1)]], np.float32), np.array([[Dt(0, 0, 1, 1, .5, 1)]], np.float32))
  with pytest.raises(_lib.EdetError):
    m.result()


# ------------------------------------------------------------------------------------ the batches
def batch_a():
  """7 images, D = 12, M = 9, integer-grid boxes; categories 1, 2, 3, 5 (class 7 is detected but never annotated)."""
  rng = np.random.default_rng(20260)
  gts, dets = [], []
  # image 0: eleven detections of class 1 (the caps 1, 10 and 100 differ) and one of class 7
  gts.append([G(0, 0, 10, 10, 0, 1),            # IoU exactly 0.6 with (0, 0, 10, 6)
              G(0, 20, 20, 30, 0, 1),           # 10 x 20: IoU exactly 0.75 with the 10 x 15 box inside it
              G(100, 100, 140, 140, 1, 1),      # a crowd, matched by two detections
              G(200, 200, 210, 210, 0, 1),      # these two have IoU 80 / 120 with the detection (202, 200, 10, 10):
              G(200, 204, 210, 214, 0, 1),      #   the equal IoU replaces the earlier match
              G(300, 0, 332, 32, 0, 1),         # area exactly 32^2
              G(300, 100, 396, 196, 0, 1),      # area exactly 96^2
              G(0, 300, 31, 332, 0, 2),         # 32 x 31 < 32^2; class 2 has no detection in this image
              G(400, 400, 497, 496, 0, 3)])     # 96 x 97 > 96^2
  dets.append([Dt(0, 0, 10, 6, .9, 1), Dt(20, 0, 10, 15, .9, 1),      # equal scores within the image
               Dt(100, 100, 20, 20, .8, 1), Dt(110, 110, 20, 20, .7, 1), Dt(202, 200, 10, 10, .6, 1),
               Dt(0, 300, 32, 32, .25, 1), Dt(100, 300, 96, 96, .5, 1),      # the first: rank 10, a match beyond cap 10
               Dt(500, 500, 32, 32, .45, 1), Dt(600, 500, 96, 96, .4, 1),      # unmatched, their own areas on the bounds
               Dt(600, 0, 33, 32, .35, 1), Dt(700, 0, 97, 96, .3, 1), Dt(0, 0, 10, 10, .95, 7)])
  # image 1: IoU exactly 0.5; one box annotated as two classes; a second detection of a taken ground truth; class 5
  gts.append([G(0, 0, 10, 10, 0, 2), G(0, 0, 10, 10, 0, 1), G(50, 50, 82, 83, 0, 2), G(200, 200, 296, 295, 0, 3),
              G(400, 0, 420, 20, 0, 5), G(400, 100, 500, 200, 1, 5)])
  dets.append([Dt(0, 0, 10, 5, .5, 2), Dt(0, 0, 10, 10, .9, 1), Dt(50, 50, 33, 32, .5, 2), Dt(200, 200, 95, 96, .5, 3),
               Dt(0, 0, 9, 10, .5, 1), PAD_D, Dt(0, 0, 10, 10, .5, 7)])
  # images 2, 3, 6: drawn on the integer grid; scores from a small set, so they tie within and across images
  for img in (2, 3, 6):
    g, d = [], []
    for _ in range(9 if img != 3 else 6):
      y, x = (int(v) for v in rng.integers(0, 300, 2))
      h, w = (int(v) for v in rng.choice([8, 16, 31, 32, 33, 64, 96, 97], 2))
      g.append(G(y, x, y + h, x + w, int(rng.random() < 0.2), int(rng.choice([1, 2, 3]))))
    for j in range(12):
      y1, x1, y2, x2, _, _, c = g[j % len(g)]
      dy, dx, dh, dw = (int(v) for v in rng.integers(-4, 5, 4))
      c = c if rng.random() < 0.8 else int(rng.choice([1, 2, 3, 7]))
      d.append(Dt(x1 + dx, y1 + dy, max(1, x2 - x1 + dw), max(1, y2 - y1 + dh), float(rng.choice([.3, .5, .7, .9])), c,
                  image_id=40 if img == 2 else -1))
    gts.append(g)
    dets.append(d)
  gts.insert(4, [])                                                          # image 4: no ground truth
  dets.insert(4, [Dt(0, 0, 32, 32, .5, 1), Dt(10, 10, 50, 50, .9, 2), PAD_D, Dt(5, 5, 96, 96, .7, 3)])
  gts.insert(5, [G(0, 0, 10, 10, 0, 1), G(0, 0, 20, 20, 0, 5)])              # image 5: no detections
  dets.insert(5, [])
  return padded(gts, 9, PAD_G), padded(dets, 12, PAD_D)


def batch_b():
  """2 images at the limits D = 100, M = 128, random boxes, 3 categories."""
  rng = np.random.default_rng(20261)
  gt = np.zeros((2, 128, 7), np.float32)
  det = np.zeros((2, 100, 7), np.float32)
  for i in range(2):
    y, x = rng.uniform(0, 300, (2, 128))
    h, w = rng.uniform(4, 130, (2, 128))
    gt[i] = np.stack([y, x, y + h, x + w, rng.random(128) < 0.1, np.zeros(128), rng.integers(1, 4, 128)], 1)
    src = rng.permutation(128)[:100]
    j = rng.uniform(-0.15, 0.15, (4, 100)) * np.stack([w[src], h[src], w[src], h[src]])
    cls = np.where(rng.random(100) < 0.9, gt[i, src, 6], rng.integers(1, 4, 100))
    score = np.round(rng.random(100), 2)      # two decimals: ties
    det[i] = np.stack([np.full(100, -1.0), x[src] + j[0], y[src] + j[1], w[src] + j[2], h[src] + j[3], score, cls], 1)
  return gt, det


def batch_d():
  """30 images, D = 100, M = 16, 2 categories: about 1,500 rows per category, so every thread of an accumulate workgroup
  walks a run of several rows and the run that holds a recall threshold's row is searched for."""
  rng = np.random.default_rng(20262)
  n, m, d = 30, 16, 100
  y, x = rng.integers(0, 400, (2, n, m)).astype(np.float64)
  h, w = rng.integers(6, 120, (2, n, m)).astype(np.float64)
  cls = rng.integers(1, 3, (n, m)).astype(np.float64)
  cls[:, 10:] = np.where(rng.random((n, 6)) < 0.5, -1, cls[:, 10:])
  gt = np.stack([y, x, y + h, x + w, rng.random((n, m)) < 0.1, np.zeros((n, m)), cls], -1).astype(np.float32)
  src = rng.integers(0, 10, (n, d))
  take = lambda a: np.take_along_axis(a, src, 1)
  hit = rng.random((n, d)) < 0.6
  jit = rng.integers(-6, 7, (4, n, d))
  det = np.stack([np.full((n, d), -1.0), np.where(hit, take(x) + jit[0], rng.integers(0, 400, (n, d))),
                  np.where(hit, take(y) + jit[1], rng.integers(0, 400, (n, d))),
                  np.maximum(1, np.where(hit, take(w) + jit[2], rng.integers(6, 120, (n, d)))),
                  np.maximum(1, np.where(hit, take(h) + jit[3], rng.integers(6, 120, (n, d)))),
                  np.round(rng.random((n, d)), 2), np.where(hit, take(cls), rng.integers(1, 3, (n, d)))], -1).astype(np.float32)
  return gt, det


_CACHE = {}


def case(name):
  """(groundtruth_data, detections, the restatement's arrays), made once and left unchanged."""
  if name not in _CACHE:
    gt, det = {'a': batch_a, 'b': batch_b, 'd': batch_d}[name]()
    m = cm.EvaluationMetric(label_map={1: 'one', 2: 'two'})
    m.update_state(gt, det)
    _CACHE[name] = (gt, det, ref_of(m, n_labels=2))
  return _CACHE[name]


def test_batch_a_holds_what_it_must():
  gt, det, r = case('a')
  assert gt.shape == (7, 9, 7) and det.shape == (7, 12, 7)
  assert r['ids'] == [1, 2, 4, 5, 6, 40] and r['cats'].tolist() == [1.0, 2.0, 3.0, 5.0]      # image 5 of 7 is skipped
  dt, g = r['dt'], r['gt']
  assert (r['matched'][0, 0, [2, 3]] == 0x3ff).all() and g[0, 2, 4] == 1                     # the crowd, matched twice
  assert cr.box_iou(dt[0, 4], g[0, 3], False) == cr.box_iou(dt[0, 4], g[0, 4], False) >= 0.65  # two equal IoUs
  assert cr.box_iou(dt[0, 1], g[0, 1], False) == 0.75 and cr.box_iou(dt[1, 0], g[1, 0], False) == 0.5
  assert r['matched'][0, 0, 1] == 0b111111 and r['matched'][1, 0, 0] == 0b1                  # IoUs on the thresholds
  assert not (dt[..., 5] == 5).any() and (g[..., 6] == 5).any() and (dt[..., 5] == 7).any()  # class 5: no detections
  assert (g[3, :, 6] == -1).all() and (dt[3, :, 5] > -1).any()                               # an image without ground truth
  assert r['rank'][0].max() == 10                                                            # eleven of class 1
  areas = set(g[..., 5][g[..., 6] > -1].tolist())
  assert {992.0, 1024.0, 1056.0, 9120.0, 9216.0, 9312.0} <= areas
  scores = dt[..., 4][dt[..., 5] > -1]
  assert np.count_nonzero(scores == np.float32(.5)) > 6
  p = r['precision']
  assert (p[:, :, 3, 0] == 0).all() and (p[:, :, 3, 2] == -1).all() and (r['recall'][:, 3, 0] == 0).all()      # class 5: ground truth, no detections
  assert not np.array_equal(r['recall'][:, 0, 0, 0], r['recall'][:, 0, 0, 1])
  assert not np.array_equal(r['recall'][:, 0, 0, 1], r['recall'][:, 0, 0, 2])
  assert len(set(np.round(r['stats'], 6).tolist())) >= 10


# ------------------------------------------------------------------------------------ GPU
def assert_equals_ref(m, got, r, what):
  ev = m.eval
  for key in ('rank', 'matched', 'ignored', 'precision', 'recall'):
    have = ev[key].cpu().numpy()
    if key in ('matched', 'ignored'):
      have = have.view(np.uint16)
    assert have.dtype == r[key].dtype and np.array_equal(have, r[key]), (what, key, int((have != r[key]).sum()))
  assert got.dtype == np.float32 and np.array_equal(got, r['result']), (what, got.tolist(), r['result'].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['a', 'b', 'd'])
def test_kernels_equal_restatement(name):
  gt, det, r = case(name)
  m = cm.EvaluationMetric(label_map={1: 'one', 2: 'two'})
  m.update_state(gt, det)
  got = m.result()
  assert got.shape == (12 + len(r['cats']),)
  assert_equals_ref(m, got, r, name)
  assert m.result() is got      # cached


@pytest.mark.gpu
def test_two_calls_equal_one_and_reset_reproduces():
  gt, det, r = case('a')
  m = cm.EvaluationMetric(label_map={1: 'one', 2: 'two'})
  m.update_state(gt[:3], det[:3])
  m.update_state(gt[3:], det[3:])
  assert_equals_ref(m, m.result(), r, 'two calls')
  first = m.result().copy()
  m.reset_states()
  assert m.metric_values is None
  m.update_state(gt, det)
  assert_equals_ref(m, m.result(), r, 'after reset')
  assert np.array_equal(m.result(), first)


@pytest.mark.gpu
def test_calls_of_different_row_counts_are_padded():
  """The second call brings two more detection rows and two more ground-truth rows per image, all padding: the packed state
  is [N, 14, 6] and [N, 11, 7], the kernels equal the restatement on it, and the statistics are those of batch (a)."""
  gt, det, r = case('a')
  m = cm.EvaluationMetric(label_map={1: 'one', 2: 'two'})
  m.update_state(gt[:3], det[:3])
  m.update_state(np.concatenate([gt[3:], padded([[]] * 4, 2, PAD_G)], 1), np.concatenate([padded([[]] * 4, 2, PAD_D), det[3:]], 1))
  wide = ref_of(m, n_labels=2)
  assert wide['dt'].shape == (6, 14, 6) and wide['gt'].shape == (6, 11, 7)
  assert_equals_ref(m, m.result(), wide, 'padded')
  assert np.array_equal(m.result(), r['result'])
  assert np.array_equal(wide['precision'], r['precision']) and np.array_equal(wide['recall'], r['recall'])


@pytest.mark.gpu
def test_filename_on_the_device(tmp_path):
  """Ground truth from a COCO annotation file: the file's categories (one of them never annotated: its cells stay -1), its
  areas and crowd flags, only the images that have detections."""
  gt, det, _ = case('a')
  data = {'images': [{'id': i} for i in range(1, 60)], 'categories': [{'id': c} for c in (5, 3, 2, 1, 9)], 'annotations': []}
  for i, rows in zip([1, 2, 40, 4, 5], gt[:5]):      # the ids update_state will give these images
    for y1, x1, y2, x2, crowd, _, c in rows.tolist():
      if c > -1:
        data['annotations'].append({'id': len(data['annotations']) + 1, 'image_id': i, 'category_id': int(c),
                                    'bbox': [x1, y1, x2 - x1, y2 - y1], 'area': (x2 - x1) * (y2 - y1) + 0.5 * (i == 2),
                                    'iscrowd': int(crowd)})
  data['annotations'].append({'id': 999, 'image_id': 50, 'category_id': 9, 'bbox': [0, 0, 5, 5], 'area': 25, 'iscrowd': 0})
  path = tmp_path / 'instances.json'
  path.write_text(json.dumps(data))
  m = cm.EvaluationMetric(filename=str(path), label_map={1: 'one'})
  m.update_state(gt[:5], det[:5])      # running ids 1, 2, 40 (given), 4, 5; image 50 has no detections
  r = ref_of(m, n_labels=1)
  assert r['ids'] == [1, 2, 4, 5, 40] and r['cats'].tolist() == [1.0, 2.0, 3.0, 5.0, 9.0]
  got = m.result()
  assert got.shape == (12 + 5,) and got[12 + 4] == -1      # category 9: nothing evaluated
  assert_equals_ref(m, got, r, 'filename')


@pytest.mark.gpu
def test_device_resident_input():
  gt, det, r = case('a')
  m = cm.EvaluationMetric(label_map={1: 'one', 2: 'two'})
  dg, dd = torch.from_numpy(gt).to(gu.DEV), torch.from_numpy(det).to(gu.DEV)
  m.update_state(dg, dd)
  assert all(t.device.type == 'cuda' for t in m._dets + m._gts)      # the state stays where it was given
  assert_equals_ref(m, m.result(), r, 'device tensors')
  assert np.array_equal(dd.cpu().numpy(), det) and np.array_equal(dg.cpu().numpy(), gt)      # the inputs are not written


def canaried(shape, dtype, fill, canary):
  """A flat device buffer with CANARY elements behind the body -> (the whole buffer, the body's view)."""
  n = int(np.prod(shape))
  buf = torch.full((n + CANARY,), canary, dtype=dtype, device=gu.DEV)
  buf[:n] = fill
  return buf, buf[:n].view(shape)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['a', 'b', 'd'])
def test_canaries_and_run_to_run_bits(name):
  """Both launches on buffers with canaries behind every output, twice: the canaries stay and the runs agree in every byte."""
  gt, det, r = case(name)
  m = cm.EvaluationMetric()
  m.update_state(gt, det)
  ids, dt, g, cats = m.packed_state(gu.DEV)
  n, d, k = dt.shape[0], dt.shape[1], cats.shape[0]
  iou_thrs, area_rng, rec_thrs, caps = cm.constants(gu.DEV)
  runs = []
  for _ in range(2):
    rank_b, rank = canaried((n, d), torch.int32, 0x55, 0x1234567)
    mt_b, mt = canaried((n, cm.A, d), torch.int16, 0x55, 0x7abc)
    ig_b, ig = canaried((n, cm.A, d), torch.int16, 0x55, 0x7abc)
    cm.launch_match(dt, g, iou_thrs, area_rng, rank, mt, ig, gu.stream())
    perm, seg, npig = cm.order_and_counts(dt, g, cats, rank)
    pr_b, pr = canaried((cm.T, cm.R, k, cm.A, cm.M), torch.float64, -1.0, 777.25)
    rc_b, rc = canaried((cm.T, k, cm.A, cm.M), torch.float64, -1.0, 777.25)
    cm.launch_accumulate(perm, seg, rank, mt, ig, npig, n, d, k, rec_thrs, caps, pr, rc, gu.stream())
    torch.cuda.synchronize()
    assert bool((rank_b[n * d:] == 0x1234567).all()) and bool((mt_b[mt.numel():] == 0x7abc).all())
    assert bool((ig_b[ig.numel():] == 0x7abc).all())
    assert bool((pr_b[pr.numel():] == 777.25).all()) and bool((rc_b[rc.numel():] == 777.25).all())
    runs.append([t.cpu().numpy() for t in (rank, mt, ig, pr, rc)])
  for x, y, key in zip(runs[0], runs[1], ('rank', 'matched', 'ignored', 'precision', 'recall')):
    assert x.tobytes() == y.tobytes(), key
    want = r[key]
    assert np.array_equal(x.view(np.uint16) if key in ('matched', 'ignored') else x, want), key
  assert np.array_equal(dt.cpu().numpy(), r['dt']) and np.array_equal(g.cpu().numpy(), r['gt'])
