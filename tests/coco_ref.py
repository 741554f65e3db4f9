"""COCOeval for boxes, restated in numpy: the definition edet_coco_match / edet_coco_accumulate (automl_amd/csrc/coco_eval.hip)
are compared with bit for bit, and what automl_amd/coco_metric.py summarises.  Test infrastructure, like tests/gridmask_ref.py.

NOT PINNED against pycocotools: it is not installed here, and nothing in this file was ever compared with a run of it.  The
algorithm is pycocotools' `COCOeval` (evaluateImg, accumulate, summarize) and `maskApi.c`'s bbIou as read from their public
sources, restated statement by statement on the padded arrays the device works on.  What pins it: the known answers of the
reference's own test (efficientdet/coco_metric_test.py:39-48) and a case derived by hand (tests/test_coco_metric.py).

Arrays (the layout of include/edet_hip.h): images in ascending id; dt float32 [N, D, 6] rows {x, y, w, h, score, class};
gt float32 [N, M, 7] rows {x, y, w, h, is_crowd, area, class}; a row whose class is not > -1 is padding; cats: the evaluated
category ids, ascending."""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)


def box_iou(d, g, crowd):
  """maskApi.c bbIou in float64 from the float32 coordinates; one rounded operation per line."""
  dx, dy, dw, dh = (np.float64(v) for v in d[:4])
  gx, gy, gw, gh = (np.float64(v) for v in g[:4])
  w = min(dx + dw, gx + gw) - max(dx, gx)
  if w <= 0:
    return np.float64(0)
  h = min(dy + dh, gy + gh) - max(dy, gy)
  if h <= 0:
    return np.float64(0)
  i = w * h
  da = dw * dh
  u = da if crowd else (da + gw * gh) - i
  with np.errstate(all='ignore'):
    return i / u


def match_image(dt, gt):
  """COCOeval.evaluateImg for every class of one image -> rank int32 [D], matched, ignored uint16 [4, D] (bit t)."""
  D = dt.shape[0]
  rank = np.full(D, -1, np.int32)
  matched = np.zeros((A, D), np.uint16)
  ignored = np.zeros((A, D), np.uint16)
  keep = dt[:, 5] > -1
  gkeep = gt[:, 6] > -1
  for c in np.unique(dt[keep, 5]):
    di = np.where(keep & (dt[:, 5] == c))[0]
    di = di[np.argsort(-dt[di, 4], kind='mergesort')][:MAX_DETS[-1]]
    rank[di] = np.arange(len(di))
    gi = np.where(gkeep & (gt[:, 6] == c))[0]
    crowd = gt[gi, 4] != 0
    ious = np.array([[box_iou(dt[d], gt[g], gt[g, 4] != 0) for g in gi] for d in di], np.float64).reshape(len(di), len(gi))
    for a, (lo, hi) in enumerate(AREA_RNG):
      g_ig = crowd | (gt[gi, 5].astype(np.float64) < lo) | (gt[gi, 5].astype(np.float64) > hi)
      gorder = np.argsort(g_ig.astype(np.uint8), kind='mergesort')      # not ignored first, stable
      for t, thr in enumerate(IOU_THRS):
        gtm = np.zeros(len(gi), bool)
        for p, d in enumerate(di):
          best = min(thr, 1 - 1e-10)
          m = -1
          for g in gorder:
            if gtm[g] and not crowd[g]:
              continue
            if m > -1 and not g_ig[m] and g_ig[g]:
              break
            if ious[p, g] < best:
              continue
            best = ious[p, g]
            m = g
          if m >= 0:
            gtm[m] = True
            matched[a, d] |= np.uint16(1 << t)
            if g_ig[m]:
              ignored[a, d] |= np.uint16(1 << t)
          else:
            area = np.float64(np.float32(dt[d, 2] * dt[d, 3]))      # COCO.loadRes: the float32 product
            if area < lo or area > hi:
              ignored[a, d] |= np.uint16(1 << t)
  return rank, matched, ignored


def match(dt, gt):
  n, d = dt.shape[0], dt.shape[1]
  rank = np.zeros((n, d), np.int32)
  matched = np.zeros((n, A, d), np.uint16)
  ignored = np.zeros((n, A, d), np.uint16)
  for i in range(n):
    rank[i], matched[i], ignored[i] = match_image(dt[i], gt[i])
  return rank, matched, ignored


def accumulate(dt, gt, cats, rank, matched, ignored):
  """COCOeval.accumulate -> precision float64 [T, R, K, A, M], recall float64 [T, K, A, M], -1 where nothing is evaluated."""
  K, N = len(cats), dt.shape[0]
  precision = -np.ones((T, R, K, A, M))
  recall = -np.ones((T, K, A, M))
  for k, c in enumerate(cats):
    per_image = []
    for n in range(N):
      di = np.where((dt[n, :, 5] > -1) & (dt[n, :, 5] == c))[0]
      per_image.append(di[np.argsort(rank[n, di], kind='mergesort')])
    gsel = (gt[:, :, 6] > -1) & (gt[:, :, 6] == c)
    for a, (lo, hi) in enumerate(AREA_RNG):
      area = gt[:, :, 5].astype(np.float64)
      npig = int(np.count_nonzero(gsel & ~((gt[:, :, 4] != 0) | (area < lo) | (area > hi))))
      if npig == 0:
        continue
      for m, cap in enumerate(MAX_DETS):
        rows = [(n, d) for n in range(N) for d in per_image[n][:cap]]
        scores = np.array([dt[n, d, 4] for n, d in rows], np.float32)
        order = np.argsort(-scores, kind='mergesort')
        rows = [rows[i] for i in order]
        nd = len(rows)
        for t in range(T):
          dtm = np.array([(matched[n, a, d] >> t) & 1 for n, d in rows], bool)
          dig = np.array([(ignored[n, a, d] >> t) & 1 for n, d in rows], bool)
          tp = np.cumsum(dtm & ~dig).astype(np.float64)
          fp = np.cumsum(~dtm & ~dig).astype(np.float64)
          rc = tp / npig
          pr = tp / ((fp + tp) + np.spacing(1))
          recall[t, k, a, m] = rc[-1] if nd else 0
          pr = np.maximum.accumulate(pr[::-1])[::-1]      # for i in range(nd - 1, 0, -1): pr[i - 1] = max(pr[i - 1], pr[i])
          inds = np.searchsorted(rc, REC_THRS, side='left')
          q = np.zeros(R)
          for ri, pi in enumerate(inds):
            if pi < nd:
              q[ri] = pr[pi]
          precision[t, :, k, a, m] = q
  return precision, recall


def _mean(s):
  s = s[s > -1]
  return -1.0 if s.size == 0 else float(np.mean(s))


def summarize(precision, recall):
  """COCOeval.summarize: the 12 statistics, float64."""
  ap = lambda t, a, m: _mean(precision[:, :, :, a, m] if t is None else precision[t, :, :, a, m])
  ar = lambda a, m: _mean(recall[:, :, a, m])
  return np.array([ap(None, 0, 2), ap(0, 0, 2), ap(5, 0, 2), ap(None, 1, 2), ap(None, 2, 2), ap(None, 3, 2),
                   ar(0, 0), ar(0, 1), ar(0, 2), ar(1, 2), ar(2, 2), ar(3, 2)], np.float64)


def per_class_ap(precision, n_labels):
  """coco_metric.py:152-166: entry c is the c-th evaluated category by position; entries past K stay 0."""
  k = precision.shape[2]
  out = [0.0] * max(k, n_labels)
  for c in range(k):
    out[c] = _mean(precision[:, :, c, 0, -1])
  return np.array(out, np.float64)


def evaluate(dt, gt, cats, n_labels=0):
  """dt, gt, cats -> dict of every array the device makes, the 12 statistics and result() as float32."""
  dt, gt = np.asarray(dt, np.float32), np.asarray(gt, np.float32)
  rank, matched, ignored = match(dt, gt)
  precision, recall = accumulate(dt, gt, list(cats), rank, matched, ignored)
  stats = summarize(precision, recall)
  full = np.concatenate((stats, per_class_ap(precision, n_labels))) if n_labels else stats
  return {'rank': rank, 'matched': matched, 'ignored': ignored, 'precision': precision, 'recall': recall, 'stats': stats,
          'result': np.array(full, np.float32)}
