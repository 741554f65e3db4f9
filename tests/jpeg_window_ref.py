"""A numpy restatement of the JPEG decode of a crop window (automl_amd/jpeg.py, decode_and_crop_jpeg; include/edet_hip.h, "JPEG
decode of a crop window"), laid over tests/jpeg_ref.py and tests/jpeg_scaled_ref.py:

  * kept_grid: the smallest rectangle of whole MCUs that holds the samples a window (y, x, h, w), in output pixels at `denom`,
    needs of every component -- [x, x + w - 1] where the component is not up-sampled, [max(0, (x >> 1) - 1), min(C - 1,
    ((x + w - 1) >> 1) + 1)] where it is up-sampled by two, C its real samples; y alike;
  * parse: the host stage -- jpeg_ref.parse's scan loop, which stores a block only inside the kept grid, in raster order over
    it, and stops behind the last kept MCU row; `end` is the offset of the first byte of the file it has not read a bit of;
  * color: edet_jpeg_color_window -- jpeg_scaled_ref.color's formulas evaluated at image pixel (y + r, x + q) on the kept
    planes, every sample read at its place minus the kept grid's first sample, every edge rule the whole image's.

The definition of the result is the full decode's [y:y + h, x:x + w]; tests/test_jpeg_window.py compares color() with the
fixtures' pixels cropped."""
import collections

import numpy as np

from tests import jpeg_ref as jr
from tests import jpeg_scaled_ref as js

Windowed = collections.namedtuple('Windowed', 'frame h_max v_max denom window grid blocks_w blocks_h kept_height kept_width '
                                              'qtables coefs end')


def frame_geometry(fr):
  """-> components counted, h_max, v_max (one component: its sampling factors do not count)."""
  if fr.components == 1:
    return 1, 1, 1
  return 3, fr.h_samp[0], fr.v_samp[0]


def kept_grid(fr, window, denom):
  """-> (mcu_y0, mcu_x0, mcus_h, mcus_w) for a window inside the output image."""
  nc, hm, vm = frame_geometry(fr)
  y, x, h, w = window
  out_h, out_w = js.scaled_size(fr.height, fr.width, denom)
  assert 0 <= y and 0 <= x and h >= 1 and w >= 1 and y + h <= out_h and x + w <= out_w, window
  s = js.sample_sizes(nc, hm, vm, denom)
  rows, cols = [], []
  for c in range(nc):
    uy, ux = (1, 1) if c == 0 else (vm * s[0] // s[c], hm * s[0] // s[c])
    for u, first, size, whole, per_mcu, out in ((uy, y, h, out_h, vm if c == 0 else 1, rows),
                                                (ux, x, w, out_w, hm if c == 0 else 1, cols)):
      a, b = first, first + size - 1
      if u == 2:
        real = (whole + 1) // 2
        a, b = max(0, (a >> 1) - 1), min(real - 1, (b >> 1) + 1)
      out += [a // s[c] // per_mcu, b // s[c] // per_mcu]
  return min(rows), min(cols), max(rows) - min(rows) + 1, max(cols) - min(cols) + 1


def _offset(data, start, consumed):
  """The offset in the file of the byte behind `consumed` unstuffed bytes of the interval that starts at `start`."""
  p = start
  for _ in range(consumed):
    p += 2 if data[p] == 0xFF else 1
  return p


def parse(data, window, denom=1):
  """The host stage for one window -> Windowed (coefs: per component int16 [kept blocks_h][kept blocks_w][64]); raises
  jpeg_ref.Refused for what jpeg_ref.parse refuses IN FRONT OF `end`."""
  data = bytes(data)
  fr, qt, huff, sos, p = jr.walk(data)
  jr.check_frame(fr)
  nc = fr.components
  if len(sos) < 1 or len(sos) != 4 + 2 * sos[0]:
    raise jr.Refused(jr.MALFORMED, 'SOS length')
  ns = sos[0]
  ids = [sos[1 + 2 * i] for i in range(ns)]
  if any(i not in fr.comp_id[:nc] for i in ids):
    raise jr.Refused(jr.MALFORMED, 'scan component not in the frame')
  if ids != list(fr.comp_id[:nc]):
    raise jr.Refused(jr.UNSUPPORTED, 'not one interleaved scan')
  if (sos[1 + 2 * ns], sos[2 + 2 * ns], sos[3 + 2 * ns]) != (0, 63, 0):
    raise jr.Refused(jr.MALFORMED, 'spectral selection of a sequential scan')
  dc, ac = [], []
  for i in range(nc):
    td, ta = sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15
    if td > 3 or ta > 3 or (0, td) not in huff or (1, ta) not in huff:
      raise jr.Refused(jr.MALFORMED, 'missing Huffman table')
    if fr.quant_id[i] > 3 or fr.quant_id[i] not in qt:
      raise jr.Refused(jr.MALFORMED, 'missing quantisation table')
    dc.append(jr._Huff(huff[(0, td)][0], huff[(0, td)][1], True))
    ac.append(jr._Huff(huff[(1, ta)][0], huff[(1, ta)][1], False))
  qtables = np.zeros((4, 64), np.uint16)
  for k, t in qt.items():
    qtables[k] = t
  hm, vm, bw, bh = jr.geometry(fr)
  hs = [hm, 1, 1] if nc == 3 else [1]
  vs = [vm, 1, 1] if nc == 3 else [1]
  my0, mx0, kh, kw = kept_grid(fr, window, denom)
  kbw, kbh = [kw * hs[c] for c in range(nc)], [kh * vs[c] for c in range(nc)]
  coefs = [np.zeros((kbh[c], kbw[c], 64), np.int16) for c in range(nc)]
  mcus_w = bw[0] // hs[0]
  pred = [0] * nc
  start = p
  bits = jr._Bits(data, p)
  ri = fr.restart_interval
  todo = ri
  next_rst = 0
  natural = [int(v) for v in jr.NATURAL]
  skipped = np.zeros(64, np.int16)
  for my in range(my0 + kh):      # nothing behind the last kept MCU row is read
    for mx in range(mcus_w):
      if ri and todo == 0:
        m, q = jr._next_marker(data, bits.end)
        if m != 0xD0 + next_rst:
          raise jr.Refused(jr.MALFORMED, 'restart marker out of sequence')
        next_rst = (next_rst + 1) & 7
        start = q
        bits = jr._Bits(data, q)
        pred = [0] * nc
        todo = ri
      todo -= 1
      kept = my >= my0 and mx0 <= mx < mx0 + kw
      for c in range(nc):
        for yy in range(vs[c]):
          for xx in range(hs[c]):
            blk = coefs[c][(my - my0) * vs[c] + yy, (mx - mx0) * hs[c] + xx] if kept else skipped
            s = bits.symbol(dc[c])
            pred[c] += bits.receive_extend(s)
            blk[0] = ((pred[c] + 0x8000) & 0xFFFF) - 0x8000
            k = 1
            while k < 64:
              rs = bits.symbol(ac[c])
              r, s = rs >> 4, rs & 15
              if s == 0:
                if r != 15:
                  break
                k += 16
                continue
              k += r
              if k > 63:
                raise jr.Refused(jr.MALFORMED, 'coefficient index past 63')
              blk[natural[k]] = bits.receive_extend(s)
              k += 1
  end = _offset(data, start, bits.pos - bits.have // 8)
  out_h, out_w = js.scaled_size(fr.height, fr.width, denom)
  s0 = js.sample_sizes(nc, hm, vm, denom)[0]
  kept_h = min(out_h, (my0 + kh) * vm * s0) - my0 * vm * s0
  kept_w = min(out_w, (mx0 + kw) * hm * s0) - mx0 * hm * s0
  return Windowed(fr, hm, vm, denom, tuple(int(v) for v in window), (my0, mx0, kh, kw), kbw, kbh, kept_h, kept_w, qtables,
                  coefs, end)


def planes(win):
  """edet_jpeg_idct_scaled on the kept grid: per component uint8 [kept blocks_h * s][kept blocks_w * s]."""
  sizes = js.sample_sizes(len(win.coefs), win.h_max, win.v_max, win.denom)
  out = []
  for c, coef in enumerate(win.coefs):
    s = sizes[c]
    px = js.idct_blocks(coef, win.qtables[win.frame.quant_id[c]], s)
    bh, bw = px.shape[:2]
    out.append(np.ascontiguousarray(px.transpose(0, 2, 1, 3).reshape(bh * s, bw * s)))
  return out


def _chroma(plane, oy, ox, ys, xs, image_h, image_w, fh, fv, m):
  """One chroma plane at image pixels ys x xs -> int [len(ys)][len(xs)]; (oy, ox): the first kept sample."""
  if fh == 1:
    return plane[np.ix_(ys - oy, xs - ox)].astype(np.int32)
  n, rows = (image_w + 1) // 2, (image_h + fv - 1) // fv
  i = xs >> 1
  if not (m > 1 and n > 2):      # replication
    return plane[np.ix_((ys >> 1 if fv == 2 else ys) - oy, np.minimum(i, n - 1) - ox)].astype(np.int32)
  odd = (xs & 1) == 1
  other = np.clip(np.where(odd, i + 1, i - 1), 0, n - 1)
  edge = np.where(odd, i == n - 1, i == 0)

  def at(r, cidx):
    return plane[np.ix_(r - oy, cidx - ox)].astype(np.int32)
  if fv == 1:
    cur, oth = at(ys, i), at(ys, other)
    return np.where(edge[None, :], cur, (3 * cur + oth + np.where(odd, 2, 1)[None, :]) >> 2)
  near = ys >> 1
  far = np.clip(np.where(ys % 2 == 0, near - 1, near + 1), 0, rows - 1)
  cur = 3 * at(near, i) + at(far, i)
  oth = 3 * at(near, other) + at(far, other)
  bias = np.where(odd, 7, 8)[None, :]
  return np.where(edge[None, :], (4 * cur + bias) >> 4, (3 * cur + oth + bias) >> 4)


def color(win, pl=None):
  """edet_jpeg_color_window for one image: uint8 [h][w][3]."""
  pl = planes(win) if pl is None else pl
  fr = win.frame
  y, x, h, w = win.window
  my0, mx0 = win.grid[:2]
  image_h, image_w = js.scaled_size(fr.height, fr.width, win.denom)
  s = js.sample_sizes(len(pl), win.h_max, win.v_max, win.denom)
  ys, xs = np.arange(y, y + h), np.arange(x, x + w)
  lum = pl[0][np.ix_(ys - my0 * win.v_max * s[0], xs - mx0 * win.h_max * s[0])].astype(np.int32)
  if len(pl) == 1:
    return np.repeat(lum[:, :, None], 3, axis=2).astype(np.uint8)
  fh, fv = win.h_max * s[0] // s[1], win.v_max * s[0] // s[1]
  m = 8 // win.denom
  cb = _chroma(pl[1], my0 * s[1], mx0 * s[1], ys, xs, image_h, image_w, fh, fv, m) - 128
  cr = _chroma(pl[2], my0 * s[2], mx0 * s[2], ys, xs, image_h, image_w, fh, fv, m) - 128
  r = lum + ((91881 * cr + 32768) >> 16)
  g = lum + ((-22554 * cb - 46802 * cr + 32768) >> 16)
  b = lum + ((116130 * cb + 32768) >> 16)
  return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def windows_for(out_h, out_w):
  """The windows every test uses for an out_h x out_w output, clipped to it and deduplicated, in a fixed order: the whole
  image, the first pixel, the last pixel, the last row, the last column, (1, 1, odd, odd), width and height 2 across the
  block seam (7) and the MCU seam (15), and two windows whose chroma guard touches every edge of the image (an even and an
  odd start, ending three pixels from the far edges)."""
  raw = [(0, 0, out_h, out_w), (0, 0, 1, 1), (out_h - 1, out_w - 1, 1, 1), (out_h - 1, 0, 1, out_w), (0, out_w - 1, out_h, 1),
         (1, 1, 5, 7), (0, 7, out_h, 2), (0, 15, out_h, 2), (7, 0, 2, out_w), (15, 0, 2, out_w),
         (2, 2, out_h - 4, out_w - 4), (3, 3, out_h - 5, out_w - 5), (1, 1, out_h - 3, out_w - 3)]
  out = []
  for y, x, h, w in raw:
    y, x = min(max(y, 0), out_h - 1), min(max(x, 0), out_w - 1)
    win = (y, x, min(max(h, 1), out_h - y), min(max(w, 1), out_w - x))
    if win not in out:
      out.append(win)
  return out
