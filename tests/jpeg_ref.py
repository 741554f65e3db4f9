"""A numpy restatement of the baseline JPEG decoder of automl_amd/jpeg.py, one image at a time: the marker walk and the
Huffman stage of csrc/jpeg_host.cpp, then the two kernels of csrc/jpeg.hip -- libjpeg's integer-accurate inverse DCT
(jidctint.c), fancy chroma upsampling (jdsample.c) and YCbCr -> RGB (jdcolor.c).  tests/test_jpeg.py compares it with the
pixels Pillow decoded (tests/golden/jpeg_cases.npz) byte for byte; the host stage and each kernel are compared with its
intermediate results, so everything here is part of the definition:

  * the statuses and the order in which a file is refused (check_frame, parse);
  * coefficients int16 per component [blocks_h][blocks_w][64], not dequantised, in natural order, the block grid padded to
    whole MCUs; the DC predictor wraps (only its low 16 bits are stored);
  * every sum, product and left shift of the inverse DCT wraps at 32 bits and every right shift is arithmetic, so a corrupt
    stream gives the same bytes here and on the device;
  * planes uint8 per component [blocks_h * 8][blocks_w * 8], padding blocks included.
"""
import collections

import numpy as np

OK, PROGRESSIVE, ARITHMETIC, PRECISION, COMPONENTS, SAMPLING, TOO_LARGE, MALFORMED, UNSUPPORTED = range(9)
KIND_BASELINE, KIND_EXTENDED, KIND_PROGRESSIVE, KIND_OTHER = range(4)

# zigzag position -> natural (row-major) position
NATURAL = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
    62, 63], np.int32)


class Refused(Exception):
  def __init__(self, status, why=''):
    super().__init__('status %d %s' % (status, why))
    self.status = status


Frame = collections.namedtuple('Frame', 'height width components precision kind restart_interval sof h_samp v_samp quant_id '
                                        'comp_id jfif adobe_transform')
Decoded = collections.namedtuple('Decoded', 'frame h_max v_max blocks_w blocks_h qtables coefs')


def _u16(data, p):
  if p + 2 > len(data):
    raise Refused(MALFORMED, 'truncated')
  return (data[p] << 8) | data[p + 1]


def _next_marker(data, p):
  """-> (marker byte, position behind it); fill bytes 0xFF in front of a marker are skipped."""
  if p >= len(data) or data[p] != 0xFF:
    raise Refused(MALFORMED, 'marker expected at %d' % p)
  while p < len(data) and data[p] == 0xFF:
    p += 1
  if p >= len(data):
    raise Refused(MALFORMED, 'truncated')
  return data[p], p + 1


def walk(data, want_scan=True):
  """Walks the markers up to SOS.  -> (Frame, tables) with want_scan False as soon as the frame AND the SOS marker (or the
  end of the data) are seen; else -> (Frame, qtables, dc, ac, scan components, position of the entropy data)."""
  data = bytes(data)
  if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
    raise Refused(MALFORMED, 'no SOI')
  p = 2
  qt = {}
  huff = {}
  frame = None
  ri = 0
  jfif = 0
  adobe = -1
  while True:
    m, p = _next_marker(data, p)
    if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
      continue
    if m == 0xD9:
      raise Refused(MALFORMED, 'EOI before SOS')
    n = _u16(data, p)
    if n < 2 or p + n > len(data):
      raise Refused(MALFORMED, 'segment length')
    seg = data[p + 2:p + n]
    if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
      if frame is not None:
        raise Refused(MALFORMED, 'two frames')
      if len(seg) < 6:
        raise Refused(MALFORMED, 'SOF length')
      nc = seg[5]
      if len(seg) != 6 + 3 * nc:
        raise Refused(MALFORMED, 'SOF length')
      kind = {0xC0: KIND_BASELINE, 0xC1: KIND_EXTENDED, 0xC2: KIND_PROGRESSIVE}.get(m, KIND_OTHER)
      k = min(nc, 4)
      frame = dict(height=(seg[1] << 8) | seg[2], width=(seg[3] << 8) | seg[4], components=nc, precision=seg[0], kind=kind,
                   sof=m, comp_id=tuple(seg[6 + 3 * i] for i in range(k)) + (0,) * (4 - k),
                   h_samp=tuple(seg[7 + 3 * i] >> 4 for i in range(k)) + (0,) * (4 - k),
                   v_samp=tuple(seg[7 + 3 * i] & 15 for i in range(k)) + (0,) * (4 - k),
                   quant_id=tuple(seg[8 + 3 * i] for i in range(k)) + (0,) * (4 - k))
    elif m == 0xDB:
      q = 0
      while q < len(seg):
        pq, tq = seg[q] >> 4, seg[q] & 15
        size = 128 if pq else 64
        if pq > 1 or tq > 3 or q + 1 + size > len(seg):
          raise Refused(MALFORMED, 'DQT')
        vals = seg[q + 1:q + 1 + size]
        t = np.zeros(64, np.uint16)
        for i in range(64):
          t[NATURAL[i]] = ((vals[2 * i] << 8) | vals[2 * i + 1]) if pq else vals[i]
        qt[tq] = t
        q += 1 + size
    elif m == 0xC4:
      q = 0
      while q < len(seg):
        if q + 17 > len(seg):
          raise Refused(MALFORMED, 'DHT')
        tc, th = seg[q] >> 4, seg[q] & 15
        counts = list(seg[q + 1:q + 17])
        total = sum(counts)
        if tc > 1 or th > 3 or total > 256 or q + 17 + total > len(seg):
          raise Refused(MALFORMED, 'DHT')
        huff[(tc, th)] = (counts, list(seg[q + 17:q + 17 + total]))
        q += 17 + total
    elif m == 0xDD:
      if len(seg) != 2:
        raise Refused(MALFORMED, 'DRI')
      ri = (seg[0] << 8) | seg[1]
    elif m == 0xE0:
      if len(seg) >= 5 and seg[:5] == b'JFIF\0':
        jfif = 1
    elif m == 0xEE:
      if len(seg) >= 12 and seg[:5] == b'Adobe':
        adobe = seg[11]
    elif m == 0xDA:
      if frame is None:
        raise Refused(MALFORMED, 'SOS before SOF')
      fr = Frame(restart_interval=ri, jfif=jfif, adobe_transform=adobe, **frame)
      if not want_scan:
        return fr
      return fr, qt, huff, seg, p + n
    p += n


def info(data):
  """edet_jpeg_info: the Frame of the first frame header (its restart interval: the last DRI in front of SOS)."""
  return walk(data, want_scan=False)


def check_frame(fr, canvas=None):
  """The refusals that need only the frame, in the order of the host stage."""
  if fr.kind == KIND_PROGRESSIVE:
    raise Refused(PROGRESSIVE)
  if fr.kind == KIND_OTHER:
    raise Refused(ARITHMETIC if fr.sof in (0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF) else UNSUPPORTED)
  if fr.precision != 8:
    raise Refused(PRECISION)
  if fr.components not in (1, 3):
    raise Refused(COMPONENTS)
  if fr.components == 3:
    hs, vs = fr.h_samp, fr.v_samp
    if not (hs[1] == vs[1] == hs[2] == vs[2] == 1 and (hs[0], vs[0]) in ((1, 1), (2, 1), (2, 2))):
      raise Refused(SAMPLING)
    rgb_ids = fr.comp_id[:3] == (ord('R'), ord('G'), ord('B'))
    if fr.adobe_transform == 0 or (fr.adobe_transform < 0 and not fr.jfif and rgb_ids):
      raise Refused(UNSUPPORTED, 'RGB colour space')
  elif not (1 <= fr.h_samp[0] <= 4 and 1 <= fr.v_samp[0] <= 4):
    raise Refused(MALFORMED, 'sampling factor')
  if fr.height < 1 or fr.width < 1:
    raise Refused(MALFORMED, 'empty frame')
  if canvas is not None and (fr.height > canvas[0] or fr.width > canvas[1]):
    raise Refused(TOO_LARGE)


def geometry(fr):
  """-> (h_max, v_max, blocks_w, blocks_h) per component.  One component is a non-interleaved scan: its sampling factors
  do not count (libjpeg, jdinput.c per_scan_setup)."""
  if fr.components == 1:
    return 1, 1, [(fr.width + 7) // 8], [(fr.height + 7) // 8]
  hm, vm = fr.h_samp[0], fr.v_samp[0]
  mw, mh = (fr.width + 8 * hm - 1) // (8 * hm), (fr.height + 8 * vm - 1) // (8 * vm)
  return hm, vm, [mw * hm, mw, mw], [mh * vm, mh, mh]


class _Huff(object):
  """jdhuff.c's derived table as a 16-bit look-up: look[next 16 bits] = (length << 8) | symbol, 0 = no such code."""

  def __init__(self, counts, vals, is_dc):
    self.look = [0] * 65536
    code = 0
    k = 0
    for length in range(1, 17):
      for _ in range(counts[length - 1]):
        if code >= (1 << length):
          raise Refused(MALFORMED, 'Huffman table overflow')
        sym = vals[k]
        if is_dc and sym > 15:
          raise Refused(MALFORMED, 'DC symbol')
        lo = code << (16 - length)
        entry = (length << 8) | sym
        self.look[lo:lo + (1 << (16 - length))] = [entry] * (1 << (16 - length))
        code += 1
        k += 1
      code <<= 1


class _Bits(object):
  """The entropy-coded bytes of one restart interval, unstuffed; bits are taken from the top."""

  def __init__(self, data, p):
    out = bytearray()
    n = len(data)
    while p < n:
      b = data[p]
      if b == 0xFF:
        if p + 1 < n and data[p + 1] == 0:
          out.append(0xFF)
          p += 2
          continue
        break      # a marker (or the end of the data): no more bits
      out.append(b)
      p += 1
    self.end = p
    self.data = bytes(out)
    self.pos = 0      # next byte
    self.acc = 0
    self.have = 0

  def fill(self, need):
    while self.have < need and self.pos < len(self.data):
      self.acc = (self.acc << 8) | self.data[self.pos]
      self.pos += 1
      self.have += 8

  def symbol(self, table):
    self.fill(16)
    peek = (self.acc << (16 - self.have)) & 0xFFFF if self.have < 16 else (self.acc >> (self.have - 16)) & 0xFFFF
    e = table.look[peek]
    length = e >> 8
    if length == 0 or length > self.have:
      raise Refused(MALFORMED, 'bad Huffman code or out of data')
    self.have -= length
    self.acc &= (1 << self.have) - 1
    return e & 0xFF

  def receive_extend(self, s):
    if s == 0:
      return 0
    self.fill(s)
    if s > self.have:
      raise Refused(MALFORMED, 'out of data')
    v = self.acc >> (self.have - s)
    self.have -= s
    self.acc &= (1 << self.have) - 1
    return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def parse(data, canvas=None):
  """The host stage: -> Decoded (coefs: per component int16 [blocks_h][blocks_w][64]); raises Refused."""
  data = bytes(data)
  fr, qt, huff, sos, p = walk(data)
  check_frame(fr, canvas)
  nc = fr.components
  if len(sos) < 1 or len(sos) != 4 + 2 * sos[0]:
    raise Refused(MALFORMED, 'SOS length')
  ns = sos[0]
  ids = [sos[1 + 2 * i] for i in range(ns)]
  if any(i not in fr.comp_id[:nc] for i in ids):
    raise Refused(MALFORMED, 'scan component not in the frame')
  if ids != list(fr.comp_id[:nc]):
    raise Refused(UNSUPPORTED, 'not one interleaved scan')
  if (sos[1 + 2 * ns], sos[2 + 2 * ns], sos[3 + 2 * ns]) != (0, 63, 0):
    raise Refused(MALFORMED, 'spectral selection of a sequential scan')
  dc, ac = [], []
  for i in range(nc):
    td, ta = sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15
    if td > 3 or ta > 3 or (0, td) not in huff or (1, ta) not in huff:
      raise Refused(MALFORMED, 'missing Huffman table')
    if fr.quant_id[i] > 3 or fr.quant_id[i] not in qt:
      raise Refused(MALFORMED, 'missing quantisation table')
    dc.append(_Huff(huff[(0, td)][0], huff[(0, td)][1], True))
    ac.append(_Huff(huff[(1, ta)][0], huff[(1, ta)][1], False))
  qtables = np.zeros((4, 64), np.uint16)
  for k, t in qt.items():
    qtables[k] = t
  hm, vm, bw, bh = geometry(fr)
  coefs = [np.zeros((bh[c], bw[c], 64), np.int16) for c in range(nc)]
  hs = [hm, 1, 1] if nc == 3 else [1]
  vs = [vm, 1, 1] if nc == 3 else [1]
  mcus_w, mcus_h = bw[0] // hs[0], bh[0] // vs[0]
  pred = [0] * nc
  bits = _Bits(data, p)
  ri = fr.restart_interval
  todo = ri
  next_rst = 0
  natural = [int(v) for v in NATURAL]
  for my in range(mcus_h):
    for mx in range(mcus_w):
      if ri and todo == 0:
        q = bits.end
        m, q = _next_marker(data, q)
        if m != 0xD0 + next_rst:
          raise Refused(MALFORMED, 'restart marker out of sequence')
        next_rst = (next_rst + 1) & 7
        bits = _Bits(data, q)
        pred = [0] * nc
        todo = ri
      todo -= 1
      for c in range(nc):
        for yy in range(vs[c]):
          for xx in range(hs[c]):
            blk = coefs[c][my * vs[c] + yy, mx * hs[c] + xx]
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
                raise Refused(MALFORMED, 'coefficient index past 63')
              blk[natural[k]] = bits.receive_extend(s)
              k += 1
  return Decoded(fr, hm, vm, bw, bh, qtables, coefs)


# ------------------------------------------------------------------------------------ the device stage
def _fix(v):
  return np.uint32(v & 0xFFFFFFFF)


def _sar(x, s):
  return (x.view(np.int32) >> s).view(np.uint32)


def _idct_1d(x, first):
  """jidctint.c's one-dimensional pass on the last axis of uint32 [..., 8]: first = the column pass (descale by 11)."""
  x0, x1, x2, x3, x4, x5, x6, x7 = [np.ascontiguousarray(x[..., i]) for i in range(8)]
  z2, z3 = x2, x6
  z1 = (z2 + z3) * _fix(4433)
  tmp2 = z1 + z3 * _fix(-15137)
  tmp3 = z1 + z2 * _fix(6270)
  tmp0 = (x0 + x4) << np.uint32(13)
  tmp1 = (x0 - x4) << np.uint32(13)
  tmp10, tmp13 = tmp0 + tmp3, tmp0 - tmp3
  tmp11, tmp12 = tmp1 + tmp2, tmp1 - tmp2
  tmp0, tmp1, tmp2, tmp3 = x7, x5, x3, x1
  z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
  z5 = (z3 + z4) * _fix(9633)
  tmp0 = tmp0 * _fix(2446)
  tmp1 = tmp1 * _fix(16819)
  tmp2 = tmp2 * _fix(25172)
  tmp3 = tmp3 * _fix(12299)
  z1 = z1 * _fix(-7373)
  z2 = z2 * _fix(-20995)
  z3 = z3 * _fix(-16069)
  z4 = z4 * _fix(-3196)
  z3 = z3 + z5
  z4 = z4 + z5
  tmp0 = tmp0 + (z1 + z3)
  tmp1 = tmp1 + (z2 + z4)
  tmp2 = tmp2 + (z2 + z3)
  tmp3 = tmp3 + (z1 + z4)
  s = 11 if first else 18
  half = np.uint32(1 << (s - 1))
  outs = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
  return np.stack([_sar(o + half, s) for o in outs], axis=-1)


def idct_blocks(coef, table):
  """int16 [..., 64] coefficients, uint16 [64] table -> uint8 [..., 8, 8] samples."""
  with np.errstate(over='ignore'):
    c = np.asarray(coef, np.int16).astype(np.int32).view(np.uint32).reshape(coef.shape[:-1] + (8, 8))
    x = c * np.asarray(table, np.uint16).astype(np.uint32).reshape(8, 8)
    ws = _idct_1d(np.swapaxes(x, -1, -2), True)      # [..., column, row]
    out = _idct_1d(np.swapaxes(ws, -1, -2), False)   # [..., row, column]
  return np.clip(out.view(np.int32).astype(np.int64) + 128, 0, 255).astype(np.uint8)


def planes(dec):
  """edet_jpeg_idct: per component uint8 [blocks_h * 8][blocks_w * 8]."""
  out = []
  for c, coef in enumerate(dec.coefs):
    px = idct_blocks(coef, dec.qtables[dec.frame.quant_id[c]])      # [bh, bw, 8, 8]
    bh, bw = px.shape[:2]
    out.append(np.ascontiguousarray(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)))
  return out


def upsample_h2v1(plane, height, width):
  """jdsample.c h2v1_fancy_upsample on the ceil(width / 2) real columns -> int [height][width]."""
  n = (width + 1) // 2
  src = plane[:height, :n].astype(np.int32)
  prev = np.concatenate([src[:, :1], src[:, :-1]], axis=1)
  nxt = np.concatenate([src[:, 1:], src[:, -1:]], axis=1)
  even = (3 * src + prev + 1) >> 2
  odd = (3 * src + nxt + 2) >> 2
  even[:, 0] = src[:, 0]
  odd[:, n - 1] = src[:, n - 1]
  out = np.empty((height, 2 * n), np.int32)
  out[:, 0::2] = even
  out[:, 1::2] = odd
  return out[:, :width]


def upsample_h2v2(plane, height, width):
  """jdsample.c h2v2_fancy_upsample on the ceil(height / 2) x ceil(width / 2) real samples -> int [height][width]."""
  n, rows = (width + 1) // 2, (height + 1) // 2
  src = plane[:rows, :n].astype(np.int32)
  y = np.arange(height)
  near = y >> 1
  far = np.clip(np.where(y % 2 == 0, near - 1, near + 1), 0, rows - 1)
  colsum = 3 * src[near] + src[far]      # [height][n]
  last = np.concatenate([colsum[:, :1], colsum[:, :-1]], axis=1)
  nxt = np.concatenate([colsum[:, 1:], colsum[:, -1:]], axis=1)
  even = (3 * colsum + last + 8) >> 4
  odd = (3 * colsum + nxt + 7) >> 4
  even[:, 0] = (4 * colsum[:, 0] + 8) >> 4
  odd[:, n - 1] = (4 * colsum[:, n - 1] + 7) >> 4
  out = np.empty((height, 2 * n), np.int32)
  out[:, 0::2] = even
  out[:, 1::2] = odd
  return out[:, :width]


def color(dec, pl=None):
  """edet_jpeg_color for one image: uint8 [height][width][3]."""
  pl = planes(dec) if pl is None else pl
  h, w = dec.frame.height, dec.frame.width
  y = pl[0][:h, :w].astype(np.int32)
  if len(pl) == 1:
    return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
  if dec.h_max == 1:
    cb, cr = pl[1][:h, :w].astype(np.int32), pl[2][:h, :w].astype(np.int32)
  elif dec.v_max == 1:
    cb, cr = upsample_h2v1(pl[1], h, w), upsample_h2v1(pl[2], h, w)
  else:
    cb, cr = upsample_h2v2(pl[1], h, w), upsample_h2v2(pl[2], h, w)
  cb, cr = cb - 128, cr - 128
  r = y + ((91881 * cr + 32768) >> 16)
  g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
  b = y + ((116130 * cb + 32768) >> 16)
  return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data, canvas=None):
  """bytes -> uint8 [height][width][3]; raises Refused."""
  return color(parse(data, canvas))


def status_of(data, canvas=None):
  try:
    parse(data, canvas)
    return OK
  except Refused as e:
    return e.status
