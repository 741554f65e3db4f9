"""COCO-style evaluation metrics on the device: the reference's ``efficientdet/coco_metric.py`` without pycocotools.

Mirror of the reference class: ``EvaluationMetric(filename, testdev_dir, label_map)`` with ``metric_names``,
``reset_states()``, ``update_state(groundtruth_data, detections)``, ``result()`` (cached in ``metric_values``) and
``evaluate()`` (:50-237).  The reference hands its state to pycocotools' ``COCO`` / ``COCOeval``; here the state stays in padded
device arrays and two kernels of csrc/coco_eval.hip do COCOeval's work for boxes: ``edet_coco_match`` (evaluateImg: one wave per
image) and ``edet_coco_accumulate`` (accumulate: one workgroup per category, area range, cap and threshold).  Between them the
detections are ordered by (category, descending score, image, rank) with stable torch sorts on the device; the 12 statistics
are means of the two result arrays, taken on the host in numpy.  No box is ever matched on the host, and there is no CPU
fall-back: ``result()`` without the library or a GPU raises.

NEVER COMPARED WITH PYCOCOTOOLS: it is not installed here.  The definition is the algorithm of its public sources, restated in
numpy as tests/coco_ref.py, which the kernels equal bit for bit; that restatement is pinned only by the known answers of the
reference's own test (coco_metric_test.py:39-48) and by a hand-derived case (tests/test_coco_metric.py).

``update_state`` as the reference is written, and kept (:191-237):
  * detection rows with class <= -1 are dropped; an image left with none is skipped ENTIRELY: its ground truth is not added
    and the running ``image_id`` is not advanced (the ``continue`` stands in front of ``self.image_id += 1``);
  * an image whose first kept row has image_id == -1 gets the running id, and every row of an image carries the first row's;
  * ground-truth rows are kept where class > -1; their area is RECOMPUTED as float32 ``(x2 - x1) * (y2 - y1)`` (column 5 is
    ignored) and their box is ``[x1, y1, x2 - x1, y2 - y1]`` in float32;
  * the categories are the distinct ground-truth classes, ascending; a detection's area is the float32 ``width * height``.
Only the per-image flags (has a kept row, the first kept row's image id) travel to the host; tensors given on the device stay
there.  Classes are compared as the float32 values they are (the reference converts with int()): give whole numbers.

``filename``: a COCO annotation JSON read on the host with ``json``: the categories are the file's, each annotation's area,
iscrowd and bbox are taken as given (then stored as float32, like everything else here), and only images with detections are
evaluated (``params.imgIds``, :142-145).  A detection whose image id is not in the file raises ValueError.

Limits (ValueError beyond them): 100 detection rows per image (maxDets[-1], the reference's max_output_size), 128 ground
truths per image, distinct image ids at ``result()``.  Not built, and raising: ``testdev_dir`` (it only writes a JSON file).
"""
import json

import numpy as np
import torch

from automl_amd import _lib
from automl_amd._lib import call, ptr

MAX_DETS_PER_IMAGE = 100      # EDET_COCO_MAX_DETS
MAX_GTS_PER_IMAGE = 128       # EDET_COCO_MAX_GTS
# COCOeval.Params for iouType 'bbox': float64 on the host, passed to the kernels as arrays
IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)


def _as_tensor(x, what, cols):
  t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
  if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3 or t.shape[-1] != cols:
    raise ValueError('%s must be float32 [batch, rows, %d], got %s %s'
                     % (what, cols, getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
  return t


def _pad_rows(t, rows):
  """[n, r, c] -> [n, rows, c]; the new rows are padding (class -1, the last column)."""
  if t.shape[1] == rows:
    return t
  pad = torch.zeros((t.shape[0], rows - t.shape[1], t.shape[2]), dtype=t.dtype, device=t.device)
  pad[..., -1] = -1
  return torch.cat([t, pad], 1)


def launch_match(dt, gt, iou_thrs, area_rng, rank, matched, ignored, stream):
  """edet_coco_match on device tensors: dt [N, D, 6], gt [N, M, 7] float32; rank int32 [N, D]; matched, ignored int16
  (the kernel's uint16 bits) [N, 4, D]."""
  n, d, m = int(dt.shape[0]), int(dt.shape[1]), int(gt.shape[1])
  call('edet_coco_match', ptr(dt), ptr(gt), n, d, m, ptr(iou_thrs), ptr(area_rng), ptr(rank), ptr(matched), ptr(ignored), stream)


def launch_accumulate(perm, seg, rank, matched, ignored, npig, n, d, k, rec_thrs, caps, precision, recall, stream):
  """edet_coco_accumulate: precision float64 [T, R, K, A, M] and recall float64 [T, K, A, M] must hold -1 on entry."""
  call('edet_coco_accumulate', ptr(perm), ptr(seg), ptr(rank), ptr(matched), ptr(ignored), ptr(npig), n, d, k, ptr(rec_thrs),
       ptr(caps), ptr(precision), ptr(recall), stream)


def constants(device):
  """The kernels' parameter arrays on `device`: iou_thrs, area_rng, rec_thrs (float64), caps (int32)."""
  return (torch.from_numpy(IOU_THRS).to(device), torch.tensor(AREA_RNG, dtype=torch.float64, device=device),
          torch.from_numpy(REC_THRS).to(device), torch.tensor(MAX_DETS, dtype=torch.int32, device=device))


def order_and_counts(dt, gt, cats, rank):
  """What edet_coco_accumulate reads besides the match: perm int32 [N D] (the rows ordered by category, descending score,
  image, rank; rows that are padding or of no evaluated category last), seg int32 [K + 1], npig int32 [K, 4].  Stable torch
  sorts and one integer index_add on the tensors' device."""
  n, d = int(dt.shape[0]), int(dt.shape[1])
  k = int(cats.shape[0])
  dev = dt.device
  cls, score, rk = dt[..., 5].reshape(-1), dt[..., 4].reshape(-1), rank.reshape(-1).long()
  pos = torch.searchsorted(cats, cls.contiguous()).clamp(max=k - 1)
  cat = torch.where((cats[pos] == cls) & (rk >= 0), pos, torch.full_like(pos, k))
  image = torch.arange(n * d, device=dev) // d
  p = torch.argsort(image * 128 + torch.where(rk >= 0, rk, torch.full_like(rk, 127)), stable=True)
  p = p[torch.argsort(-score[p], stable=True)]
  p = p[torch.argsort(cat[p], stable=True)]
  seg = torch.searchsorted(cat[p].contiguous(), torch.arange(k + 1, device=dev)).to(torch.int32)
  gcls = gt[..., 6].reshape(-1)
  gpos = torch.searchsorted(cats, gcls.contiguous()).clamp(max=k - 1)
  gcat = torch.where((cats[gpos] == gcls) & (gcls > -1), gpos, torch.full_like(gpos, k))
  area = gt[..., 5].reshape(-1).double()
  crowd = gt[..., 4].reshape(-1) != 0
  rng = torch.tensor(AREA_RNG, dtype=torch.float64, device=dev)
  counted = ~(crowd[:, None] | (area[:, None] < rng[None, :, 0]) | (area[:, None] > rng[None, :, 1]))
  npig = torch.zeros((k + 1, A), dtype=torch.int32, device=dev).index_add_(0, gcat, counted.to(torch.int32))[:k]
  return p.to(torch.int32).contiguous(), seg.contiguous(), npig.contiguous()


def evaluate_arrays(dt, gt, cats):
  """dt [N, D, 6], gt [N, M, 7], cats [K] float32 on the GPU -> dict of device tensors: rank, matched, ignored, precision,
  recall (include/edet_hip.h).  Three launches of this library whatever N and K are."""
  if dt.device.type != 'cuda':
    raise _lib.EdetError('COCO evaluation runs on the GPU only (edet_coco_match / edet_coco_accumulate): there is no CPU '
                         'fall-back')
  _lib.load()
  n, d, k = int(dt.shape[0]), int(dt.shape[1]), int(cats.shape[0])
  dev = dt.device
  stream = torch.cuda.current_stream().cuda_stream
  iou_thrs, area_rng, rec_thrs, caps = constants(dev)
  rank = torch.empty((n, d), dtype=torch.int32, device=dev)
  matched = torch.empty((n, A, d), dtype=torch.int16, device=dev)
  ignored = torch.empty((n, A, d), dtype=torch.int16, device=dev)
  launch_match(dt, gt, iou_thrs, area_rng, rank, matched, ignored, stream)
  perm, seg, npig = order_and_counts(dt, gt, cats, rank)
  precision = torch.full((T, R, k, A, M), -1.0, dtype=torch.float64, device=dev)
  recall = torch.full((T, k, A, M), -1.0, dtype=torch.float64, device=dev)
  launch_accumulate(perm, seg, rank, matched, ignored, npig, n, d, k, rec_thrs, caps, precision, recall, stream)
  return {'rank': rank, 'matched': matched, 'ignored': ignored, 'precision': precision, 'recall': recall, 'perm': perm,
          'seg': seg, 'npig': npig}


def _mean(s):
  s = s[s > -1]
  return -1.0 if s.size == 0 else float(np.mean(s))


def summarize(precision, recall):
  """COCOeval.summarize on the host: numpy float64 [T, R, K, A, M] and [T, K, A, M] -> the 12 statistics."""
  ap = lambda t, a, m: _mean(precision[:, :, :, a, m] if t is None else precision[t, :, :, a, m])
  ar = lambda a, m: _mean(recall[:, :, a, m])
  return np.array([ap(None, 0, 2), ap(0, 0, 2), ap(5, 0, 2), ap(None, 1, 2), ap(None, 2, 2), ap(None, 3, 2),
                   ar(0, 0), ar(0, 1), ar(0, 2), ar(1, 2), ar(2, 2), ar(3, 2)], np.float64)


def load_annotation_file(filename):
  """A COCO annotation JSON -> (sorted category ids, {image id: float32 [rows, 7] {x, y, w, h, iscrowd, area, class}})."""
  with open(filename) as f:
    data = json.load(f)
  cats = sorted(set(int(c['id']) for c in data.get('categories', [])))
  images = {int(im['id']): [] for im in data.get('images', [])}
  for ann in data.get('annotations', []):
    x, y, w, h = ann['bbox']
    images.setdefault(int(ann['image_id']), []).append(
        [x, y, w, h, 1.0 if ann.get('iscrowd', 0) else 0.0, ann['area'], int(ann['category_id'])])
  return cats, {i: np.asarray(rows, np.float32).reshape(-1, 7) for i, rows in images.items()}


class EvaluationMetric():
  """COCO evaluation metric class (coco_metric.py:50-237), the evaluation on the device."""

  def __init__(self, filename=None, testdev_dir=None, label_map=None):
    """filename: ground-truth JSON in COCO annotation format; None: the ground truth passed to update_state.
    testdev_dir: not built.  label_map: a dict from id to class name; adds the per-class APs to result()."""
    if testdev_dir:
      raise ValueError('EvaluationMetric(testdev_dir=%r) is not built: the reference only writes the detections into '
                       'detections_test-dev2017_test_results.json there (coco_metric.py:119-137)' % (testdev_dir,))
    self.label_map = label_map
    self.filename = filename
    self.testdev_dir = testdev_dir
    self.metric_names = ['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'ARmax1',
                         'ARmax10', 'ARmax100', 'ARs', 'ARm', 'ARl']
    self._file = load_annotation_file(filename) if filename else None
    self.reset_states()

  def reset_states(self):
    """Reset the evaluator's state."""
    self.image_ids = []          # one id per evaluated image, in the order they came
    self._dets = []              # per update_state call: float32 [n, D, 6] {x, y, w, h, score, class}
    self._gts = []               # per call: float32 [n, M, 7] {x, y, w, h, is_crowd, area, class} (not with a file)
    self.image_id = 1
    self.metric_values = None
    self.eval = None             # evaluate_arrays' tensors of the last evaluation

  def update_state(self, groundtruth_data, detections):
    """groundtruth_data float32 [B, M, 7] rows [y1, x1, y2, x2, is_crowd, area, class]; detections float32 [B, D, 7] rows
    [image_id, x, y, width, height, score, class]; numpy arrays or torch tensors on any device."""
    det = _as_tensor(detections, 'detections', 7)
    gtd = _as_tensor(groundtruth_data, 'groundtruth_data', 7)
    if gtd.shape[0] != det.shape[0]:
      raise ValueError('groundtruth_data has %d images, detections %d' % (gtd.shape[0], det.shape[0]))
    if det.shape[1] > MAX_DETS_PER_IMAGE:
      raise ValueError('%d detection rows per image: at most %d (maxDets[-1]) are built' % (det.shape[1], MAX_DETS_PER_IMAGE))
    if gtd.shape[1] > MAX_GTS_PER_IMAGE:
      raise ValueError('%d ground-truth rows per image: at most %d are built' % (gtd.shape[1], MAX_GTS_PER_IMAGE))
    if det.shape[0] == 0 or det.shape[1] == 0:
      return
    gtd = gtd.to(det.device)
    keep = det[..., 6] > -1
    first = keep.to(torch.int8).argmax(1)
    first_id = det[torch.arange(det.shape[0], device=det.device), first, 0]
    flags = torch.stack([keep.any(1).to(torch.float32), first_id], 1).cpu().numpy()      # the only copy to the host
    rows = []
    for i in range(flags.shape[0]):
      if not flags[i, 0]:
        continue      # no ground truth either, and the running id stays
      image_id = flags[i, 1]
      if image_id == -1:
        image_id = self.image_id
      image_id = int(image_id)
      if self._file is not None and image_id not in self._file[1]:
        raise ValueError('detections of image id %d, which %s does not list' % (image_id, self.filename))
      self.image_ids.append(image_id)
      rows.append(i)
      self.image_id += 1
    if not rows:
      return
    sel = torch.as_tensor(rows, dtype=torch.long, device=det.device)
    self._dets.append(det[sel][..., 1:7].contiguous())
    if self._file is None and gtd.shape[1] > 0:
      g = gtd[sel]
      w, h = g[..., 3] - g[..., 1], g[..., 2] - g[..., 0]
      cls = torch.where(g[..., 6] > -1, g[..., 6], torch.full_like(g[..., 6], -1))
      crowd = (g[..., 4].to(torch.int32) != 0).to(torch.float32)      # int(is_crowd)
      self._gts.append(torch.stack([g[..., 1], g[..., 0], w, h, crowd, w * h, cls], -1))
    elif self._file is None:
      self._gts.append(torch.full((len(rows), 1, 7), -1.0, device=det.device))

  def _check_ids(self):
    if not self.image_ids:
      raise ValueError('no detections: update_state has kept no image')
    ids = np.asarray(self.image_ids, np.int64)
    if np.unique(ids).size != ids.size:
      dup = sorted(set(int(i) for i in ids if np.count_nonzero(ids == i) > 1))
      raise ValueError('image ids are not distinct: %s' % dup[:8])
    return ids

  def packed_state(self, device=None):
    """The state as the kernels read it, on `device` (default: where the first detections live): (image ids ascending, a
    list; dt float32 [N, D, 6]; gt float32 [N, M, 7]; categories float32 [K], ascending)."""
    ids = self._check_ids()
    dev = torch.device(device) if device is not None else self._dets[0].device
    order = np.argsort(ids, kind='stable')
    sel = torch.from_numpy(order).to(dev)
    d = max(t.shape[1] for t in self._dets)
    dt = torch.cat([_pad_rows(t.to(dev), d) for t in self._dets], 0)[sel].contiguous()
    ids = [int(i) for i in ids[order]]
    if self._file is None:
      m = max(t.shape[1] for t in self._gts)
      gt = torch.cat([_pad_rows(t.to(dev), m) for t in self._gts], 0)[sel].contiguous()
      cls = gt[..., 6]
      cats = torch.unique(cls[cls > -1])      # ascending
    else:
      file_cats, per_image = self._file
      m = max(1, max(per_image[i].shape[0] for i in ids))
      if m > MAX_GTS_PER_IMAGE:
        raise ValueError('%s lists %d annotations for one image: at most %d are built' % (self.filename, m, MAX_GTS_PER_IMAGE))
      host = np.zeros((len(ids), m, 7), np.float32)
      host[..., 6] = -1
      for n, i in enumerate(ids):
        host[n, :per_image[i].shape[0]] = per_image[i]
      gt = torch.from_numpy(host).to(dev)
      cats = torch.tensor(file_cats, dtype=torch.float32, device=dev)
    return ids, dt, gt, cats

  def evaluate(self):
    """Evaluates the detections of all images on the device.  Returns the float32 numpy array of the 12 COCO statistics,
    followed by the per-class APs when label_map is given (coco_metric.py:152-169)."""
    self._check_ids()
    if not torch.cuda.is_available():
      raise _lib.EdetError('EvaluationMetric.evaluate needs a GPU: COCO evaluation has no CPU fall-back')
    ids, dt, gt, cats = self.packed_state('cuda')
    k = int(cats.shape[0])
    if k == 0:      # no ground truth at all: nothing is evaluated
      precision, recall = -np.ones((T, R, 0, A, M)), -np.ones((T, 0, A, M))
      self.eval = None
    else:
      self.eval = evaluate_arrays(dt, gt, cats)
      precision, recall = self.eval['precision'].cpu().numpy(), self.eval['recall'].cpu().numpy()
    coco_metrics = summarize(precision, recall)
    if self.label_map:
      # TxRxKxAxM; areaRng 'all' and the last maxDets
      ap_perclass = [0] * max(k, len(self.label_map))
      for c in range(k):      # by position among the evaluated categories
        ap_perclass[c] = _mean(precision[:, :, c, 0, -1])
      coco_metrics = np.concatenate((coco_metrics, ap_perclass))
    return np.array(coco_metrics, dtype=np.float32)

  def result(self):
    """Return the metric values (and compute it if needed)."""
    if self.metric_values is None:
      self.metric_values = self.evaluate()
    return self.metric_values
