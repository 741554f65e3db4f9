"""numpy restatement of automl_amd/mosaic.py and csrc/mosaic.hip (the reference's efficientdet/aug/mosaic.py), one mosaic at a
time -- TEST INFRASTRUCTURE.

The quadrants are tf.image.resize of the WHOLE source images as oracle.preprocess_oracle.resize_bilinear restates it (float32,
half-pixel centres, taps clamped at the image's edges), placed as the reference's concatenations place them (mosaic.py:246-250:
image 1 BELOW image 0, image 2 to its right); the two output conversions (float32 as it is, uint8 clipped and truncated); the
reference's box arithmetic (an int32 product, a true division, an integer offset); and the batch form's box arithmetic and
row order (automl_amd.mosaic.mosaic_batch).
"""
import numpy as np

from automl_amd import mosaic as mz
from oracle import preprocess_oracle

F = np.float32


def quadrants(x, y, out0, out1):
  """-> for image 0..3: (row offset, column offset, rows, columns) of its sub-image."""
  return ((0, 0, x, y), (x, 0, out0 - x, y), (0, y, x, out1 - y), (x, y, out0 - x, out1 - y))


def mosaic_image(images, x, y, out_size):
  """Four uint8 [h, w, 3] images (each of its own size) -> float32 [out0, out1, 3]."""
  out0, out1 = out_size
  assert len(images) == 4 and 1 <= x <= out0 - 1 and 1 <= y <= out1 - 1, (len(images), x, y, out_size)
  out = np.zeros((out0, out1, 3), np.float32)
  for im, (oy, ox, qh, qw) in zip(images, quadrants(x, y, out0, out1)):
    im = np.asarray(im)
    assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3, (im.dtype, im.shape)
    out[oy:oy + qh, ox:ox + qw] = preprocess_oracle.resize_bilinear(im.astype(np.float32), qh, qw)
  return out


def convert(v, kind):
  """What edet_mosaic stores: 'f32' the values as they are, 'u8' clip to [0, 255] and truncate."""
  if kind == 'f32':
    return np.asarray(v, np.float32)
  assert kind == 'u8', kind
  return np.clip(v, F(0), F(255)).astype(np.uint8)


def mosaic_from_rows(raw, rows, out_size, kind):
  """A canvas batch uint8 [B, Hc, Wc, 3] and edet_mosaic_t rows [G, 16], clamped as the kernel clamps them -> [G, out0,
  out1, 3] of `kind`."""
  raw = np.asarray(raw)
  rows = mz.clamp_rows(rows, raw.shape[0], raw.shape[1], raw.shape[2], out_size[0], out_size[1])
  out = []
  for r in rows:
    ims = [raw[r[mz.INDEX][k], :r[mz.HEIGHT][k], :r[mz.WIDTH][k]] for k in range(4)]
    out.append(convert(mosaic_image(ims, int(r[mz.X]), int(r[mz.Y]), out_size), kind))
  return np.stack(out)


def mosaic_boxes(boxes, sizes, x, y, out_size):
  """The reference's boxes: four integer arrays [N, 4] = [x1, y1, x2, y2] in pixels, sizes [4, 2] = (height, width) ->
  four float64 [N, 4].  box * sub / src as an int32 product and a true division, + x on columns 1 and 3 for images 1 and 3,
  + y on columns 0 and 2 for images 2 and 3 (mosaic.py:98-103, :171-217)."""
  out = []
  for k, (oy, ox, qh, qw) in enumerate(quadrants(x, y, *out_size)):
    b = np.asarray(boxes[k]).astype(np.int32)
    h, w = int(sizes[k][0]), int(sizes[k][1])
    v = np.stack([b[:, 0] * np.int32(qw) / np.int32(w), b[:, 1] * np.int32(qh) / np.int32(h),
                  b[:, 2] * np.int32(qw) / np.int32(w), b[:, 3] * np.int32(qh) / np.int32(h)], 1)
    assert v.dtype == np.float64
    out.append(v + np.asarray([ox, oy, ox, oy], np.float64))
  return out


def batch_boxes(boxes, classes, counts, rows, out_size):
  """mosaic_batch's box half: boxes float32 [B, M, 4] normalised (ymin, xmin, ymax, xmax), classes [B, M], counts [B], rows
  [G, 16] (clamped as the kernel clamps them) -> (boxes [G, 4 M, 4], classes [G, 4 M], counts int32 [G]): the valid rows
  of source 0, then 1, 2, 3, the rest -1; one rounded float32 operation each."""
  boxes, classes = np.asarray(boxes, np.float32), np.asarray(classes, np.float32)
  b, m = boxes.shape[:2]
  out0, out1 = out_size
  rows = mz.clamp_rows(rows, b, 1, 1, out0, out1)
  counts = np.clip(np.asarray(counts).astype(np.int64), 0, m)
  ob = np.full((rows.shape[0], 4 * m, 4), -1, np.float32)
  oc = np.full((rows.shape[0], 4 * m), -1, np.float32)
  on = np.zeros(rows.shape[0], np.int32)
  for g, r in enumerate(rows):
    at = 0
    for k, (oy, ox, qh, qw) in enumerate(quadrants(int(r[mz.X]), int(r[mz.Y]), out0, out1)):
      src = int(r[mz.INDEX][k])
      n = int(counts[src])
      v = boxes[src, :n]
      ob[g, at:at + n, 0] = (F(oy) + v[:, 0] * F(qh)) / F(out0)
      ob[g, at:at + n, 1] = (F(ox) + v[:, 1] * F(qw)) / F(out1)
      ob[g, at:at + n, 2] = (F(oy) + v[:, 2] * F(qh)) / F(out0)
      ob[g, at:at + n, 3] = (F(ox) + v[:, 3] * F(qw)) / F(out1)
      oc[g, at:at + n] = classes[src, :n]
      at += n
    on[g] = at
  return ob, oc, on
