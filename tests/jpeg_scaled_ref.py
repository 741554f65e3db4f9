"""A numpy restatement of the reduced-size JPEG decode of automl_amd/jpeg.py (tf.io.decode_jpeg's `ratio`, libjpeg's
scale_denom 2, 4 and 8), laid over tests/jpeg_ref.py: the host stage is jpeg_ref.parse as it is -- the coefficients do not
depend on the ratio -- and what follows it is csrc/jpeg_scaled.hip's two kernels.  With denom in {1, 2, 4, 8} and m = 8 / denom:

  * the output is ceil(height / denom) x ceil(width / denom);
  * a component's blocks are inverse-transformed to s x s samples (sample_sizes: m, except 4:2:0 chroma at 2 m when m < 8, which
    then needs no upsampling); s = 8 is jidctint.c (jpeg_ref.idct_blocks), s = 4 and 2 jidctred.c's jpeg_idct_4x4 / 2x2, s = 1
    the DC term alone.  All sums, products and left shifts wrap at 32 bits, the right shifts are arithmetic;
  * planes uint8 per component [blocks_h * s][blocks_w * s], padding blocks included;
  * chroma that is still subsampled is upsampled by jdsample.c's fancy h2v1 / h2v2 only when m > 1 and the component has more
    than two real columns; otherwise its samples are replicated;
  * colour conversion is jpeg_ref.color's.

tests/golden/make_golden_jpeg_scaled.py compares decode() with Pillow's draft mode (libjpeg-turbo) byte for byte.
"""
import numpy as np

from tests import jpeg_ref as jr

DENOMS = (1, 2, 4, 8)


def scaled_size(height, width, denom):
  return (height + denom - 1) // denom, (width + denom - 1) // denom


def choose_denom(height, width, canvas, max_denom=8):
  """The smallest denominator not above max_denom whose output fits the canvas, or None."""
  for denom in DENOMS:
    if denom <= max_denom:
      h, w = scaled_size(height, width, denom)
      if h <= canvas[0] and w <= canvas[1]:
        return denom
  return None


def sample_sizes(components, h_max, v_max, denom):
  """Per component the side of a block after the inverse transform (jdmaster.c, jpeg_calc_output_dimensions)."""
  m = 8 // denom
  hs = [h_max, 1, 1][:components] if components == 3 else [1]
  vs = [v_max, 1, 1][:components] if components == 3 else [1]
  out = []
  for h_c, v_c in zip(hs, vs):
    s = m
    while s < 8 and (h_max * m) % (h_c * s * 2) == 0 and (v_max * m) % (v_c * s * 2) == 0:
      s *= 2
    out.append(s)
  return out


def _descale(x, n):
  return jr._sar(x + np.uint32(1 << (n - 1)), n)


def _idct4_1d(v, n):
  """jidctred.c jpeg_idct_4x4, one pass on the last axis of uint32 [..., 8] (entry 4 is never read) -> [..., 4]."""
  v0, v1, v2, v3, _, v5, v6, v7 = [np.ascontiguousarray(v[..., i]) for i in range(8)]
  t0 = v0 << np.uint32(14)
  t2 = v2 * jr._fix(15137) + v6 * jr._fix(-6270)
  t10, t12 = t0 + t2, t0 - t2
  a = v7 * jr._fix(-1730) + v5 * jr._fix(11893) + v3 * jr._fix(-17799) + v1 * jr._fix(8697)
  b = v7 * jr._fix(-4176) + v5 * jr._fix(-4926) + v3 * jr._fix(7373) + v1 * jr._fix(20995)
  return np.stack([_descale(o, n) for o in (t10 + b, t12 + a, t12 - a, t10 - b)], axis=-1)


def _idct2_1d(v, n):
  """jidctred.c jpeg_idct_2x2, one pass on the last axis of uint32 [..., 8] (entries 0, 1, 3, 5, 7 are read) -> [..., 2]."""
  v0, v1, v3, v5, v7 = [np.ascontiguousarray(v[..., i]) for i in (0, 1, 3, 5, 7)]
  t10 = v0 << np.uint32(15)
  t0 = v7 * jr._fix(-5906) + v5 * jr._fix(6967) + v3 * jr._fix(-10426) + v1 * jr._fix(29692)
  return np.stack([_descale(o, n) for o in (t10 + t0, t10 - t0)], axis=-1)


def idct_blocks(coef, table, s):
  """int16 [..., 64] coefficients, uint16 [64] table -> uint8 [..., s, s] samples."""
  if s == 8:
    return jr.idct_blocks(coef, table)
  with np.errstate(over='ignore'):
    c = np.asarray(coef, np.int16).astype(np.int32).view(np.uint32).reshape(coef.shape[:-1] + (8, 8))
    x = c * np.asarray(table, np.uint16).astype(np.uint32).reshape(8, 8)
    if s == 1:
      out = jr._sar(x[..., :1, :1] + np.uint32(4), 3)
    elif s == 4:
      ws = _idct4_1d(np.swapaxes(x, -1, -2), 12)      # [..., column, 4 rows]; column 4 is computed and never read
      out = _idct4_1d(np.swapaxes(ws, -1, -2), 19)    # [..., 4 rows, 4 columns]
    elif s == 2:
      ws = _idct2_1d(np.swapaxes(x, -1, -2), 13)
      out = _idct2_1d(np.swapaxes(ws, -1, -2), 20)
    else:
      raise ValueError('sample size %r' % (s,))
  return np.clip(out.view(np.int32).astype(np.int64) + 128, 0, 255).astype(np.uint8)


def planes(dec, denom):
  """edet_jpeg_idct_scaled: per component uint8 [blocks_h * s][blocks_w * s]."""
  sizes = sample_sizes(dec.frame.components, dec.h_max, dec.v_max, denom)
  out = []
  for c, coef in enumerate(dec.coefs):
    s = sizes[c]
    px = idct_blocks(coef, dec.qtables[dec.frame.quant_id[c]], s)      # [bh, bw, s, s]
    bh, bw = px.shape[:2]
    out.append(np.ascontiguousarray(px.transpose(0, 2, 1, 3).reshape(bh * s, bw * s)))
  return out


def replicate(plane, height, width, fh, fv):
  """jdsample.c h2v1_upsample / h2v2_upsample: every sample fh times in a row, every row fv times -> int [height][width]."""
  src = plane[:(height + fv - 1) // fv, :(width + fh - 1) // fh].astype(np.int32)
  return np.repeat(np.repeat(src, fv, axis=0), fh, axis=1)[:height, :width]


def color(dec, denom, pl=None):
  """edet_jpeg_color_scaled for one image: uint8 [ceil(height / denom)][ceil(width / denom)][3]."""
  pl = planes(dec, denom) if pl is None else pl
  fr = dec.frame
  h, w = scaled_size(fr.height, fr.width, denom)
  m = 8 // denom
  y = pl[0][:h, :w].astype(np.int32)
  if len(pl) == 1:
    return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
  s = sample_sizes(fr.components, dec.h_max, dec.v_max, denom)
  fh, fv = dec.h_max * s[0] // s[1], dec.v_max * s[0] // s[1]
  assert (fh, fv) in ((1, 1), (2, 1), (2, 2)), (fh, fv)
  columns = -(-fr.width * s[1] // (8 * dec.h_max))      # the component's real columns (downsampled_width)
  assert columns == (w + fh - 1) // fh
  if fh == 1:
    cb, cr = pl[1][:h, :w].astype(np.int32), pl[2][:h, :w].astype(np.int32)
  elif m > 1 and columns > 2:
    up = jr.upsample_h2v1 if fv == 1 else jr.upsample_h2v2
    cb, cr = up(pl[1], h, w), up(pl[2], h, w)
  else:
    cb, cr = replicate(pl[1], h, w, fh, fv), replicate(pl[2], h, w, fh, fv)
  cb, cr = cb - 128, cr - 128
  r = y + ((91881 * cr + 32768) >> 16)
  g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
  b = y + ((116130 * cb + 32768) >> 16)
  return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data, denom, canvas=None):
  """bytes -> uint8 [ceil(height / denom)][ceil(width / denom)][3]; raises jpeg_ref.Refused (TOO_LARGE: the OUTPUT does not
  fit the canvas)."""
  fr = jr.info(data)
  jr.check_frame(fr)
  if canvas is not None:
    h, w = scaled_size(fr.height, fr.width, denom)
    if h > canvas[0] or w > canvas[1]:
      raise jr.Refused(jr.TOO_LARGE)
  return color(jr.parse(data), denom)
