"""A numpy / Python restatement of the device entropy decoder (include/edet_hip.h, "JPEG Huffman decode on the device"):
edet_jpeg_scan_prepare's segments, units and descriptors, and the workgroup of csrc/jpeg_entropy.hip with its rounds run in
order.  It is the definition the way tests/jpeg_ref.py is for the rest, on whose walk, check_frame, geometry and tables it
stands; tests/test_jpeg_entropy.py compares it with jpeg_ref.parse -- the SERIAL decode -- on every fixture, and the library
with it.

  * a segment: the entropy-coded bytes of one restart interval, FF 00 stuffing removed; it ends at an FF that 00 does not
    follow; the marker behind segment j (fill FFs skipped) must be RST(j mod 8); ceil(MCUs / restart interval) segments, one
    without DRI, and nothing behind the last is looked at;
  * a unit: subseq_bits bits of one segment, the last may be shorter; a segment of no bytes has no unit;
  * state (p, b, k): bit position, block inside the MCU, zigzag position (0: DC next); decode_unit decodes whole symbols until
    p >= unit end; bits behind the segment read as zeros and a symbol that needs them is an error, which leaves the state
    (segment end, 0, 0);
  * round 0 from (unit start, 0, 0); round r: a unit whose predecessor's end state differs from the start it last used adopts
    it and decodes again; the first unit of a segment never moves; the loop ends when nothing changed;
  * a segment's share is min(restart interval, MCUs left) x blocks per MCU blocks; one that completes fewer makes the image
    MALFORMED; blocks behind the share are dropped;
  * DC: the differences summed per component in scan order, reset at every segment start, 32-bit wrapping, low 16 bits kept.
"""
import collections

import numpy as np

from tests import jpeg_ref as jr

TABLES = 6

Prepared = collections.namedtuple('Prepared', 'frame h_max v_max blocks_w blocks_h qtables tables dc_slot ac_slot ri mcus_w '
                                              'mcus_h blocks_per_mcu segments first_unit units')


def cut_segments(data, p, count):
  """The scan from position p as `count` unstuffed segments; raises Refused(MALFORMED) on a restart marker that is missing
  or out of sequence."""
  data = bytes(data)
  n = len(data)
  out = []
  for j in range(count):
    seg = bytearray()
    while p < n:
      b = data[p]
      if b == 0xFF:
        if p + 1 < n and data[p + 1] == 0:
          seg.append(0xFF)
          p += 2
          continue
        break
      seg.append(b)
      p += 1
    out.append(bytes(seg))
    if j + 1 < count:
      m, p = jr._next_marker(data, p)
      if m != 0xD0 + (j & 7):
        raise jr.Refused(jr.MALFORMED, 'restart marker out of sequence')
  return out


def units_of(bits, subseq_bits):
  return (bits + subseq_bits - 1) // subseq_bits


def prepare(data, canvas=None, subseq_bits=1024):
  """edet_jpeg_scan_prepare for one image -> Prepared; raises Refused with the host stage's status."""
  data = bytes(data)
  fr, qt, huff, sos, p = jr.walk(data)
  jr.check_frame(fr, canvas)
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
  named = []
  for i in range(nc):
    td, ta = sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15
    if td > 3 or ta > 3 or (0, td) not in huff or (1, ta) not in huff:
      raise jr.Refused(jr.MALFORMED, 'missing Huffman table')
    if fr.quant_id[i] > 3 or fr.quant_id[i] not in qt:
      raise jr.Refused(jr.MALFORMED, 'missing quantisation table')
    named.append(((0, td), (1, ta)))
  slots, tables, dc_slot, ac_slot = [], [], [], []
  for c in range(nc):      # components that name one table share its slot
    for key in named[c]:
      if key not in slots:
        slots.append(key)
        tables.append(jr._Huff(huff[key][0], huff[key][1], key[0] == 0))
      (ac_slot if key[0] else dc_slot).append(slots.index(key))
  qtables = np.zeros((4, 64), np.uint16)
  for k, t in qt.items():
    qtables[k] = t
  hm, vm, bw, bh = jr.geometry(fr)
  mcus_w, mcus_h = bw[0] // hm, bh[0] // vm
  ri = fr.restart_interval
  count = (mcus_w * mcus_h + ri - 1) // ri if ri else 1
  segs = cut_segments(data, p, count)
  first_unit, units = [], 0
  for s in segs:
    first_unit.append(units)
    units += units_of(8 * len(s), subseq_bits)
  return Prepared(fr, hm, vm, bw, bh, qtables, tables, dc_slot, ac_slot, ri, mcus_w, mcus_h, hm * vm + 2 if nc == 3 else 1, segs,
                  first_unit, units)


class _Segment(object):
  """The bits of a segment: window(p) is bits p .. p + 31, zeros behind the last."""

  def __init__(self, data):
    self.bits = 8 * len(data)
    self.value = int.from_bytes(data + b'\0' * 8, 'big')
    self.width = self.bits + 64

  def window(self, p):
    return (self.value >> (self.width - p - 32)) & 0xFFFFFFFF


def _extend(v, s):
  return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def decode_unit(seg, end, prep, state, sink=None):
  """-> (end state, blocks completed, error).  state = (p, b, k).  sink(kind, n, k, value) with kind 'dc' / 'ac' receives what
  is decoded, n counting the blocks this call completed before."""
  p, b, k = state
  n = 0
  end = min(end, seg.bits)
  luma = prep.h_max * prep.v_max
  while p < end:
    c = 0 if b < luma else b - luma + 1
    w = seg.window(p)
    left = seg.bits - p
    e = prep.tables[prep.dc_slot[c] if k == 0 else prep.ac_slot[c]].look[w >> 16]
    length, sym = e >> 8, e & 0xFF
    s = sym & 15
    if length == 0 or length + s > left:
      return (seg.bits, 0, 0), n, True
    v = _extend(((w << length) & 0xFFFFFFFF) >> (32 - s), s) if s else 0
    done = False
    if k == 0:
      if sym > 15:
        return (seg.bits, 0, 0), n, True
      if sink is not None:
        sink('dc', n, 0, v)
      k = 1
    elif s == 0:
      if (sym >> 4) != 15:
        done = True
      else:
        k += 16
    else:
      k += sym >> 4
      if k > 63:
        return (seg.bits, 0, 0), n, True
      if sink is not None:
        sink('ac', n, k, v)
      k += 1
    p += length + s
    if done or k > 63:
      n += 1
      k = 0
      b = 0 if b + 1 == prep.blocks_per_mcu else b + 1
  return (p, b, k), n, False


def block_place(prep, scan_block):
  """Block `scan_block` of the image in scan order -> (component, block row, block column)."""
  luma = prep.h_max * prep.v_max
  mcu, bi = divmod(scan_block, prep.blocks_per_mcu)
  my, mx = divmod(mcu, prep.mcus_w)
  if bi < luma:
    yy, xx = divmod(bi, prep.h_max)
    return 0, my * prep.v_max + yy, mx * prep.h_max + xx
  return bi - luma + 1, my, mx


def decode(prep, subseq_bits):
  """The workgroup of one image -> (status, coefficients per component int16 [blocks_h][blocks_w][64] or None, rounds)."""
  segs = [_Segment(s) for s in prep.segments]
  seg_of, starts = [], []
  for j, s in enumerate(segs):
    for i in range(units_of(s.bits, subseq_bits)):
      seg_of.append(j)
      starts.append((i * subseq_bits, 0, 0))
  units = len(seg_of)
  assert units == prep.units
  first = [u == prep.first_unit[seg_of[u]] for u in range(units)]
  unit_end = [starts[u][0] + subseq_bits for u in range(units)]
  ends, counts = [None] * units, [0] * units
  for u in range(units):      # round 0
    ends[u], counts[u], _ = decode_unit(segs[seg_of[u]], unit_end[u], prep, starts[u])
  rounds = 1
  pending = set(range(units))      # the units whose predecessor decoded in the round before: only they can differ
  for r in range(1, units + 1):
    moved = [u for u in sorted(pending) if u > 0 and not first[u] and ends[u - 1] != starts[u]]
    if not moved:
      break
    rounds = r + 1
    for u in moved:      # all the reads first, as the vote's barrier makes them
      starts[u] = ends[u - 1]
    pending = set()
    for u in moved:
      ends[u], counts[u], _ = decode_unit(segs[seg_of[u]], unit_end[u], prep, starts[u])
      if u + 1 < units:
        pending.add(u + 1)
  base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  total = prep.mcus_w * prep.mcus_h * prep.blocks_per_mcu
  seg_blocks = min(prep.ri * prep.blocks_per_mcu, total) if prep.ri else total
  for j in range(len(segs)):
    fu = prep.first_unit[j]
    nxt = prep.first_unit[j + 1] if j + 1 < len(segs) else units
    if base[nxt] - base[fu] < min(seg_blocks, total - j * seg_blocks):
      return jr.MALFORMED, None, rounds
  nc = prep.frame.components
  coefs = [np.zeros((prep.blocks_h[c], prep.blocks_w[c], 64), np.int16) for c in range(nc)]
  diffs = np.zeros(total, np.int64)
  natural = [int(v) for v in jr.NATURAL]
  for u in range(units):      # the write pass, from the settled starts
    j = seg_of[u]
    first_block, share = j * seg_blocks, min(seg_blocks, total - j * seg_blocks)
    before = int(base[u] - base[prep.first_unit[j]])

    def sink(kind, n, k, v):
      i = before + n
      if i < share:
        if kind == 'dc':
          diffs[first_block + i] = v
        else:
          c, row, col = block_place(prep, first_block + i)
          coefs[c][row, col, natural[k]] = v
    decode_unit(segs[j], unit_end[u], prep, starts[u], sink)
  pred = [0] * nc
  luma = prep.h_max * prep.v_max
  for at in range(total):
    mcu, bi = divmod(at, prep.blocks_per_mcu)
    if prep.ri and bi == 0 and mcu % prep.ri == 0:
      pred = [0] * nc
    c, row, col = block_place(prep, at)
    pred[c] = (pred[c] + int(diffs[at])) & 0xFFFFFFFF
    coefs[c][row, col, 0] = ((pred[c] + 0x8000) & 0xFFFF) - 0x8000
  return jr.OK, coefs, rounds


def status_of(data, canvas=None, subseq_bits=1024):
  """The status of the device mode for one stream: the host's, or what the device finds in the scan."""
  try:
    prep = prepare(data, canvas, subseq_bits)
  except jr.Refused as e:
    return e.status
  return decode(prep, subseq_bits)[0]
