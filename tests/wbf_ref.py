"""Numpy restatement of the reference's efficientdet/tf2/wbf.py (:19-95), float32 operation by operation, with the rules the
kernels of csrc/wbf.hip follow (automl_amd/wbf.py states them):
  * sums start at float32 +0 and take their terms left to right, each product rounded before it is added;
  * the maximum IoU and its index are numpy's max / argmax: a NaN (0 / 0 between two boxes without area) is the maximum, the
    first NaN -- else the first largest value -- is its index, and a NaN is not below 0.55;
  * the final order is Python's stable list.sort(reverse=True) on the score.
tests/golden/reference_wbf.npz (the reference module executed on the torch stand-in) pins these functions bit for bit on
clusters of at most two members; the kernels are compared with ensemble_detections_batch bit for bit."""
import numpy as np

F = np.float32
IOU_THRESHOLD = 0.55      # the double; for a float32 x, x < 0.55 and x < float32(0.55) are the same statement


def vectorized_iou(clusters, detection):
  """clusters [K, 7], detection [7] -> [K, 1] (:19-36)."""
  clusters, detection = np.asarray(clusters, F).reshape(-1, 7), np.asarray(detection, F)
  x11, y11, x12, y12 = (clusters[:, i:i + 1] for i in range(1, 5))
  x21, y21, x22, y22 = (detection[i:i + 1] for i in range(1, 5))
  xa = np.maximum(x11, x21)
  ya = np.maximum(y11, y21)
  xb = np.minimum(x12, x22)
  yb = np.minimum(y12, y22)
  inter_area = np.maximum(xb - xa, F(0)) * np.maximum(yb - ya, F(0))
  boxa_area = (x12 - x11) * (y12 - y11)
  boxb_area = (x22 - x21) * (y22 - y21)
  with np.errstate(invalid='ignore', divide='ignore'):
    iou = inter_area / (boxa_area + boxb_area - inter_area)
  assert iou.dtype == F
  return iou


def find_matching_cluster(clusters, detection):
  """The index of the highest-IoU cluster, -1 if there is none or the highest is below 0.55 (:39-48)."""
  if len(clusters) == 0:
    return -1
  ious = vectorized_iou(np.stack([np.asarray(c, F) for c in clusters]), detection).reshape(len(clusters))
  if np.max(ious) < IOU_THRESHOLD:
    return -1
  return int(np.argmax(ious))


def _sum(values):
  s = F(0)
  for v in values:
    s = F(s + F(v))
  return s


def weighted_average(samples, weights):
  samples, weights = np.asarray(samples, F), np.asarray(weights, F)
  with np.errstate(invalid='ignore', divide='ignore'):
    return F(_sum(samples * weights) / _sum(weights))


def average_detections(detections, num_models):
  """A list of rows -> the cluster's row (:55-67)."""
  n = len(detections)
  d = np.stack([np.asarray(x, F) for x in detections])
  factor = F(min(1, n / num_models))
  return np.array([d[0][0], weighted_average(d[:, 1], d[:, 5]), weighted_average(d[:, 2], d[:, 5]),
                   weighted_average(d[:, 3], d[:, 5]), weighted_average(d[:, 4], d[:, 5]),
                   F(F(_sum(d[:, 5]) / F(n)) * factor), d[0][6]], F)


def ensemble_detections(params, detections, num_models):
  """detections [N, 7] -> [K, 7] (:70-95); K = 0 gives an empty [0, 7] array where the reference's tf.stack([]) raises."""
  detections = np.asarray(detections, F).reshape(-1, 7)
  all_clusters = []
  for cid in range(params['num_classes']):
    class_detections = detections[detections[:, 6] == cid]
    clusters, cluster_averages = [], []
    for d in class_detections:
      cluster_index = find_matching_cluster(cluster_averages, d)
      if cluster_index == -1:
        clusters.append([d])
        cluster_averages.append(average_detections([d], num_models))
      else:
        clusters[cluster_index].append(d)
        cluster_averages[cluster_index] = average_detections(clusters[cluster_index], num_models)
    all_clusters.extend(cluster_averages)
  all_clusters.sort(reverse=True, key=lambda d: d[5])
  return np.stack(all_clusters) if all_clusters else np.zeros((0, 7), F)


def ensemble_detections_batch(params, detections, num_models, counts=None):
  """detections [B, N, 7] -> (fused [B, N, 7] with zero rows behind the clusters, fused_counts int32 [B])."""
  detections = np.asarray(detections, F)
  b, n = detections.shape[:2]
  fused, fused_counts = np.zeros((b, n, 7), F), np.zeros((b,), np.int32)
  for i in range(b):
    c = n if counts is None else min(max(int(counts[i]), 0), n)
    out = ensemble_detections(params, detections[i, :c], num_models)
    fused[i, :len(out)] = out
    fused_counts[i] = len(out)
  return fused, fused_counts
