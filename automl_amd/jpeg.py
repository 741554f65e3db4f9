"""Baseline JPEG decode in front of every input path: encoded bytes -> the zero-padded uint8 canvas batch and sizes that
``v2_preprocessing.pad_batch`` returns, which TrainableModel.train_step / test_step, train_step_raw / test_step_raw,
eval_lib.evaluate and EfficientDetModel take.  The reference decodes wherever it touches data (tf.io.decode_image /
tf.image.decode_jpeg: object_detection/tf_example_decoder.py:57, inference.py:63, tf2/train_lib.py:258,
efficientnetv2/preprocessing.py:142, efficientnetv2/datasets.py:328,502).

The decoder is split where hybrid decoders are: the serial Huffman stage runs on the host (csrc/jpeg_host.cpp, up to 16
worker threads, one image each), everything behind it on the device in two launches per batch (csrc/jpeg.hip):
edet_jpeg_idct -- dequantisation and libjpeg's integer-accurate inverse DCT -- and edet_jpeg_color -- fancy chroma
upsampling, YCbCr -> RGB and the write into the canvas, zeros included.  The definition is libjpeg's default decoder, which
is what tf.io.decode_jpeg's defaults and Pillow use; tests/jpeg_ref.py restates it and is compared with Pillow byte for byte.

Decoded: 8-bit Huffman streams of SOF0 / SOF1 in one interleaved scan, greyscale (replicated to three channels) or YCbCr
at 4:4:4, 4:2:2 or 4:2:0.  Refused with a reason, never approximated: progressive, arithmetic-coded, 12-bit, lossless and
hierarchical files, CMYK / YCCK, 4:4:0, 4:1:1 and any other sampling, RGB-coded components, several scans, malformed or
truncated streams.  Not built: EXIF orientation (TensorFlow ignores it too), PNG / GIF / BMP, dct_method,
fancy_upscaling=False.  (TFRecord / tf.Example input is automl_amd/dataloader.py.)

Reduced size: tf.io.decode_jpeg's `ratio` 2, 4 and 8 is libjpeg's scale_denom -- a block is inverse-transformed straight to
4x4, 2x2 or 1x1 samples (jidctred.c), so the image comes out ceil(height / ratio) x ceil(width / ratio) at a fraction of the
device work (csrc/jpeg_scaled.hip: edet_jpeg_idct_scaled, edet_jpeg_color_scaled; restated in tests/jpeg_scaled_ref.py and
compared with Pillow's draft mode).  JpegDecoder(max_ratio=8) picks per image the smallest ratio whose output fits the canvas
(choose_ratio), so a file of several thousand pixels a side lands in a 512 x 512 canvas instead of being TOO_LARGE; the Huffman
stage and the coefficient copy still see the whole file.  max_ratio=1, the default, is the full-size decoder unchanged.

Crop window: tf.image.decode_and_crop_jpeg's crop_window = (y, x, h, w), in the coordinates of the output image at the ratio it
is decoded at.  The host stage stores only the blocks the window needs -- the kept grid, a rectangle of whole MCUs
(window_grid) -- and stops reading behind its last MCU row, so the coefficient copy, the inverse DCT and the colour stage
(csrc/jpeg_window.hip: edet_jpeg_color_window) all work on the kept area alone.  The result is the full decode's
[y:y + h, x:x + w] byte for byte (tests/jpeg_window_ref.py).  JpegDecoder(windowed=True).decode(windows=...) takes one window
per image; decode_and_crop_jpeg is the one-file form.

Huffman decode on the device: JpegDecoder(entropy='device') moves the entropy stage behind the bus as well.  The host keeps the
marker walk and one byte-copy pass over each scan (edet_jpeg_scan_prepare: stuffing removed, cut into segments at the restart
markers), the device decodes the Huffman stream with a self-synchronising parallel decoder (csrc/jpeg_entropy.hip, one
workgroup per image, units of subseq_bits bits that re-decode until each starts where its predecessor ended) and writes the
very coefficient arena the host stage writes; the compressed scan crosses the bus instead of its coefficients.  Header-level
refusals are known on the host as before; a stream damaged INSIDE its scan is only found on the device (scan_status,
decode(check_scan=True)).  Restated in tests/jpeg_entropy_ref.py.  entropy='host' stays the default.
"""
import collections
import ctypes

import numpy as np
import torch

from automl_amd import _lib
from automl_amd._lib import call, ptr

OK, PROGRESSIVE, ARITHMETIC, PRECISION, COMPONENTS, SAMPLING, TOO_LARGE, MALFORMED, UNSUPPORTED = range(9)
REASONS = {
    PROGRESSIVE: 'a progressive file (SOF2)',
    ARITHMETIC: 'arithmetic coding',
    PRECISION: 'a sample precision other than 8 bits',
    COMPONENTS: 'neither one nor three components (CMYK / YCCK)',
    SAMPLING: 'a chroma sampling other than 4:4:4, 4:2:2 and 4:2:0',
    TOO_LARGE: 'an image larger than the canvas',
    MALFORMED: 'a malformed or truncated stream',
    UNSUPPORTED: 'a lossless or hierarchical frame, several or non-interleaved scans, or RGB-coded components',
}
WINDOW = 9
REASONS[WINDOW] = 'a crop window outside the image, or with a side below 1'
KINDS = ('baseline', 'extended', 'progressive', 'other')
MAX_THREADS = 16
IMAGE_BYTES = ctypes.sizeof(_lib.JpegImage)      # 80
WINDOW_BYTES = ctypes.sizeof(_lib.JpegWindow)    # 48
SCAN_BYTES = ctypes.sizeof(_lib.JpegScan)        # 64
SEGMENT_BYTES = ctypes.sizeof(_lib.JpegSegment)  # 16
TABLES, TABLE_BYTES, UNIT_WORDS = 6, 2512, 8     # EDET_JPEG_TABLES, EDET_JPEG_TABLE_BYTES, EDET_JPEG_UNIT_WORDS
ENTROPIES = ('host', 'device')

JpegInfo = collections.namedtuple('JpegInfo', 'height width components precision kind restart_interval sof h_samp v_samp '
                                              'quant_id comp_id jfif adobe_transform')


def _buffer(contents, what='contents'):
  """-> (what to keep alive, address or bytes for a void* argument, length) of the bytes of a JPEG file WITHOUT copying them:
  bytes go as they are, a contiguous bytearray, memoryview (such as a span inside a mapped TFRecord file) or uint8 vector by
  its address.  Only a memoryview that is not contiguous is copied."""
  if isinstance(contents, bytes):
    return contents, contents, len(contents)
  if isinstance(contents, np.ndarray) and contents.dtype == np.uint8 and contents.ndim == 1:
    a = np.ascontiguousarray(contents)
  elif isinstance(contents, (bytearray, memoryview)):
    view = memoryview(contents)
    if not view.c_contiguous:
      data = view.tobytes()
      return data, data, len(data)
    a = np.frombuffer(view.cast('B') if view.format != 'B' or view.ndim != 1 else view, np.uint8)
  else:
    raise ValueError('%s must be the bytes of a JPEG file (bytes, bytearray, memoryview or a uint8 vector), got %s'
                     % (what, type(contents).__name__))
  if a.size == 0:
    return b'', b'', 0
  return a, a.ctypes.data, int(a.size)


def jpeg_info(contents):
  """What the file says in front of its first scan (edet_jpeg_info; host only, no device needed): a JpegInfo whose kind is
  'baseline', 'extended', 'progressive' or 'other'.  h_samp, v_samp, quant_id and comp_id are per component (at most four).
  A stream without a frame header and a scan raises ValueError."""
  _keep, data, size = _buffer(contents)
  out = _lib.JpegInfo()
  try:
    call('edet_jpeg_info', data, size, ctypes.byref(out))
  except _lib.EdetError as e:
    raise ValueError(str(e))
  k = min(int(out.components), 4)
  return JpegInfo(int(out.height), int(out.width), int(out.components), int(out.precision), KINDS[out.kind],
                  int(out.restart_interval), int(out.sof), tuple(out.h_samp[:k]), tuple(out.v_samp[:k]),
                  tuple(out.quant_id[:k]), tuple(out.comp_id[:k]), bool(out.jfif), int(out.adobe_transform))


RATIOS = (1, 2, 4, 8)


def scaled_size(height, width, ratio):
  """The size tf.io.decode_jpeg(ratio=ratio) gives a height x width file: (ceil(height / ratio), ceil(width / ratio))."""
  if ratio not in RATIOS:
    raise ValueError('ratio=%r: 1, 2, 4 or 8' % (ratio,))
  return (int(height) + ratio - 1) // ratio, (int(width) + ratio - 1) // ratio


def choose_ratio(height, width, canvas_h, canvas_w, max_ratio=8):
  """The ratio the host stage picks for a height x width file: the smallest of 1, 2, 4, 8 not above max_ratio whose output
  fits the canvas, or None when none does (the decoder's TOO_LARGE)."""
  if max_ratio not in RATIOS:
    raise ValueError('max_ratio=%r: 1, 2, 4 or 8' % (max_ratio,))
  for ratio in RATIOS:
    if ratio <= max_ratio:
      h, w = scaled_size(height, width, ratio)
      if h <= canvas_h and w <= canvas_w:
        return ratio
  return None


def worst_blocks(canvas_h, canvas_w):
  """The most 8x8 blocks one supported image on the canvas can have: the larger of 4:4:4, 4:2:2 and 4:2:0, whose padding
  to whole MCUs differs."""
  bh, bw = (canvas_h + 7) // 8, (canvas_w + 7) // 8
  mh, mw = (canvas_h + 15) // 16, (canvas_w + 15) // 16
  return max(3 * bh * bw, 4 * bh * mw, 6 * mh * mw)


def _sample_sizes(components, h_max, v_max, ratio):
  """Per component the side of a block after the inverse transform at `ratio`: 8 / ratio, twice that for the chroma of a
  4:2:0 file below full size."""
  m = 8 // ratio
  return [2 * m if c > 0 and (h_max, v_max) == (2, 2) and m < 8 else m for c in range(components)]


def window_grid(info, window, ratio=1):
  """The kept grid of `window` = (y, x, h, w), in output pixels of jpeg_info's `info` decoded at `ratio`: ((mcu_y0, mcu_x0,
  mcus_h, mcus_w), blocks) -- the smallest rectangle of whole MCUs that holds the samples every component needs (include/
  edet_hip.h, "JPEG decode of a crop window"), and the 8x8 blocks it has, which is the descriptor's total_blocks.  A window
  outside the output image or with a side below 1 raises ValueError."""
  if ratio not in RATIOS:
    raise ValueError('ratio=%r: 1, 2, 4 or 8' % (ratio,))
  y, x, h, w = [int(v) for v in window]
  out_h, out_w = scaled_size(info.height, info.width, ratio)
  if y < 0 or x < 0 or h < 1 or w < 1 or y + h > out_h or x + w > out_w:
    raise ValueError('crop window (y=%d, x=%d, h=%d, w=%d) is not inside the %d x %d image with sides of at least 1'
                     % (y, x, h, w, out_h, out_w))
  nc = 3 if info.components == 3 else 1
  h_max, v_max = (info.h_samp[0], info.v_samp[0]) if nc == 3 else (1, 1)
  sizes = _sample_sizes(nc, h_max, v_max, ratio)
  lo, hi = [None, None], [None, None]      # MCU rows, MCU columns
  for c in range(nc):
    for axis, (first, size, whole, samp) in enumerate(((y, h, out_h, v_max), (x, w, out_w, h_max))):
      u = 1 if c == 0 else samp * sizes[0] // sizes[c]
      per_mcu = samp if c == 0 else 1
      a, b = first, first + size - 1
      if u == 2:
        a, b = max(0, (a >> 1) - 1), min((whole + 1) // 2 - 1, (b >> 1) + 1)
      a, b = a // sizes[c] // per_mcu, b // sizes[c] // per_mcu
      lo[axis] = a if lo[axis] is None else min(lo[axis], a)
      hi[axis] = b if hi[axis] is None else max(hi[axis], b)
  mh, mw = hi[0] - lo[0] + 1, hi[1] - lo[1] + 1
  per = h_max * v_max + 2 if nc == 3 else 1
  return (lo[0], lo[1], mh, mw), per * mh * mw


def worst_window_blocks(canvas_h, canvas_w, max_ratio=1):
  """The most 8x8 blocks the kept grid of one window that fits the canvas can have, whatever the image around it, for any
  supported sampling and any ratio up to max_ratio.  Along an axis a span of L output pixels touches at most (L + P - 2) // P + 1
  MCUs of P output pixels; chroma that is still up-sampled by two needs up to three pixels more on either side (the guard of
  the fancy formulas).  (The blocks kept grow with the square of the ratio, as the files' do: the default, max_ratio=1, is what
  JpegDecoder multiplies by coef_blocks' rule.)"""
  if max_ratio not in RATIOS:
    raise ValueError('max_ratio=%r: 1, 2, 4 or 8' % (max_ratio,))

  def mcus(length, p, guard):
    return (length + (6 if guard else 0) + p - 2) // p + 1
  most = 0
  for ratio in RATIOS:
    if ratio > max_ratio:
      break
    s = 8 // ratio
    c444 = 3 * mcus(canvas_h, s, False) * mcus(canvas_w, s, False)
    c422 = 4 * mcus(canvas_h, s, False) * mcus(canvas_w, 2 * s, True)
    c420 = 6 * mcus(canvas_h, 2 * s, ratio == 1) * mcus(canvas_w, 2 * s, ratio == 1)
    most = max(most, c444, c422, c420)
  return most


def covering_window(window_full, ratio):
  """The window of the output at `ratio` that covers the full-size window (y, x, h, w): y' = y // ratio, h' = ceil((y + h) /
  ratio) - y', x alike."""
  y, x, h, w = [int(v) for v in window_full]
  y2, x2 = y // ratio, x // ratio
  return y2, x2, (y + h + ratio - 1) // ratio - y2, (x + w + ratio - 1) // ratio - x2


def choose_window_ratio(window_full, height, width, canvas_h, canvas_w, max_ratio=8):
  """For a window (y, x, h, w) in FULL-SIZE pixels of a height x width file: (ratio, window) with the smallest ratio of 1, 2, 4,
  8 not above max_ratio at which the covering output window -- y' = y // r, h' = ceil((y + h) / r) - y', x alike -- fits the
  canvas, or None if none does."""
  if max_ratio not in RATIOS:
    raise ValueError('max_ratio=%r: 1, 2, 4 or 8' % (max_ratio,))
  y, x, h, w = [int(v) for v in window_full]
  if y < 0 or x < 0 or h < 1 or w < 1 or y + h > height or x + w > width:
    raise ValueError('crop window (y=%d, x=%d, h=%d, w=%d) is not inside the %d x %d image with sides of at least 1'
                     % (y, x, h, w, height, width))
  for r in RATIOS:
    if r <= max_ratio:
      out = covering_window((y, x, h, w), r)
      if out[2] <= canvas_h and out[3] <= canvas_w:
        return r, out
  return None


def jpeg_sizes(contents):
  """(height, width) of every file from its headers (edet_jpeg_info; host only): int32 [B, 2], 0, 0 where the header cannot
  be read."""
  out = np.zeros((len(contents), 2), np.int32)
  for i, c in enumerate(contents):
    try:
      info = jpeg_info(c)
      out[i] = (info.height, info.width)
    except ValueError:
      pass
  return out


def _streams(datas):
  """-> (count, what to keep alive, the void* array, the size_t array) of a batch of streams, read where they lie."""
  n = len(datas)
  keep = [_buffer(d, 'contents[%d]' % i) for i, d in enumerate(datas)]
  ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(d), ctypes.c_void_p) if isinstance(d, bytes) else d
                                 for _, d, _ in keep])
  return n, keep, ptrs, (ctypes.c_size_t * n)(*[size for _, _, size in keep])


def _host(a):
  return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def _forced(ratios, n):
  """One ratio per image as an int32 array, or None."""
  if ratios is None:
    return None
  if len(ratios) != n:
    raise ValueError('%d ratios for %d files' % (len(ratios), n))
  return (ctypes.c_int32 * n)(*[int(r) for r in ratios])


def entropy_decode(datas, canvas_h, canvas_w, coef, images, qtables, status, threads=0):
  """edet_jpeg_entropy_decode on host arrays (numpy or CPU tensors): coef int16 [capacity], images uint8 [B * 80], qtables
  uint16 [B, 4, 64], status int32 [B].  Blocks until the batch is decoded; needs no device.  The streams are read where they
  lie (_buffer): nothing is copied, so a memoryview into a mapped file goes to the workers as it is."""
  n, _keep, ptrs, sizes = _streams(datas)      # (_keep: alive until the call returns)
  capacity = int(coef.size if isinstance(coef, np.ndarray) else coef.numel())
  call('edet_jpeg_entropy_decode', ptrs, sizes, n, int(canvas_h), int(canvas_w), _host(coef), capacity, _host(images),
       _host(qtables), _host(status), int(threads))


def entropy_decode_scaled(datas, canvas_h, canvas_w, max_ratio, ratios, coef, images, qtables, status, threads=0):
  """edet_jpeg_entropy_decode_scaled on host arrays, as entropy_decode: ratios None (each image gets choose_ratio's answer)
  or one forced ratio per image.  The descriptors' height / width are the output sizes, `reserved` the ratio."""
  n, _keep, ptrs, sizes = _streams(datas)      # (_keep: alive until the call returns)
  forced = _forced(ratios, n)
  capacity = int(coef.size if isinstance(coef, np.ndarray) else coef.numel())
  call('edet_jpeg_entropy_decode_scaled', ptrs, sizes, n, int(canvas_h), int(canvas_w), int(max_ratio),
       None if forced is None else ctypes.addressof(forced), _host(coef), capacity, _host(images), _host(qtables), _host(status),
       int(threads))


def entropy_decode_window(datas, canvas_h, canvas_w, max_ratio, ratios, windows, coef, images, wins, qtables, status,
                          threads=0):
  """edet_jpeg_entropy_decode_window on host arrays, as entropy_decode_scaled: windows int [B, 4] = (y, x, h, w) in output
  pixels, ratios None (every image at ratio 1) or one per image; wins uint8 [B * 48] receives the window descriptors.  The
  image descriptors describe the kept grids."""
  n, _keep, ptrs, sizes = _streams(datas)      # (_keep: alive until the call returns)
  forced = _forced(ratios, n)
  win = None
  if windows is not None:
    win = np.ascontiguousarray(np.asarray(windows, np.int64).astype(np.int32))
    if win.shape != (n, 4):
      raise ValueError('windows must be [%d, 4] = (y, x, h, w) per file, got %s' % (n, list(win.shape)))
  capacity = int(coef.size if isinstance(coef, np.ndarray) else coef.numel())
  call('edet_jpeg_entropy_decode_window', ptrs, sizes, n, int(canvas_h), int(canvas_w), int(max_ratio),
       None if forced is None else ctypes.addressof(forced), None if win is None else win.ctypes.data, _host(coef), capacity,
       _host(images), _host(wins), _host(qtables), _host(status), int(threads))


def check_subseq_bits(subseq_bits):
  subseq_bits = int(subseq_bits)
  if subseq_bits < 64 or subseq_bits > 8192 or subseq_bits % 32:
    raise ValueError('subseq_bits=%r: a multiple of 32 from 64 to 8192' % (subseq_bits,))
  return subseq_bits


def scan_prepare(datas, canvas_h, canvas_w, max_ratio, ratios, coef_capacity, subseq_bits, scan, segments, unit_capacity, tables,
                 scans, images, qtables, status, threads=0):
  """edet_jpeg_scan_prepare on host arrays (numpy or CPU tensors), as entropy_decode_scaled: scan uint8 [scan capacity],
  segments uint8 [segment capacity * 16], tables uint8 [B * 6 * 2512], scans uint8 [B * 64]; coef_capacity counts the int16
  elements of the coefficient arena the device will write.  -> (scan bytes, segments, units) in use.  Needs no device."""
  n, _keep, ptrs, sizes = _streams(datas)      # (_keep: alive until the call returns)
  forced = _forced(ratios, n)

  def count(a):
    return int(a.size if isinstance(a, np.ndarray) else a.numel())
  used = (ctypes.c_size_t * 3)()
  call('edet_jpeg_scan_prepare', ptrs, sizes, n, int(canvas_h), int(canvas_w), int(max_ratio),
       None if forced is None else ctypes.addressof(forced), int(coef_capacity), int(subseq_bits), _host(scan), count(scan),
       _host(segments), count(segments) // SEGMENT_BYTES, int(unit_capacity), _host(tables), _host(scans), _host(images),
       _host(qtables), _host(status), used, int(threads))
  return int(used[0]), int(used[1]), int(used[2])


def scan_descriptors(scans, batch):
  """The per-image scan array as a list of _lib.JpegScan (copies)."""
  raw = scans.tobytes() if isinstance(scans, np.ndarray) else scans.numpy().tobytes()
  return [_lib.JpegScan.from_buffer_copy(raw, i * SCAN_BYTES) for i in range(batch)]


def segment_rows(segments, count):
  """The first `count` rows of the segment table as a list of _lib.JpegSegment (copies)."""
  raw = segments.tobytes() if isinstance(segments, np.ndarray) else segments.numpy().tobytes()
  return [_lib.JpegSegment.from_buffer_copy(raw, i * SEGMENT_BYTES) for i in range(count)]


def window_descriptors(wins, batch):
  """The per-image window array as a list of _lib.JpegWindow (copies)."""
  raw = wins.tobytes() if isinstance(wins, np.ndarray) else wins.numpy().tobytes()
  return [_lib.JpegWindow.from_buffer_copy(raw, i * WINDOW_BYTES) for i in range(batch)]


def descriptors(images, batch):
  """The per-image array as a list of _lib.JpegImage (copies)."""
  raw = images.tobytes() if isinstance(images, np.ndarray) else images.numpy().tobytes()
  return [_lib.JpegImage.from_buffer_copy(raw, i * IMAGE_BYTES) for i in range(batch)]


class _Slot(object):
  """One set of arenas: pinned host memory the host stage writes, its device copy, the plane scratch, and the event behind
  the copies."""

  def __init__(self, batch, blocks, device, windowed=False):
    if windowed:
      self.windows_host = torch.zeros(batch * WINDOW_BYTES, dtype=torch.uint8).pin_memory()
      self.windows = torch.zeros(batch * WINDOW_BYTES, dtype=torch.uint8, device=device)
    self.coef_host = torch.empty(blocks * 64, dtype=torch.int16).pin_memory()
    self.images_host = torch.zeros(batch * IMAGE_BYTES, dtype=torch.uint8).pin_memory()
    self.qtables_host = torch.zeros((batch, 4, 64), dtype=torch.int16).pin_memory()      # uint16 bits
    self.status = np.zeros(batch, np.int32)
    self.coef = torch.empty(blocks * 64, dtype=torch.int16, device=device)
    self.images = torch.zeros(batch * IMAGE_BYTES, dtype=torch.uint8, device=device)
    self.qtables = torch.zeros((batch, 4, 64), dtype=torch.int16, device=device)
    self.planes = torch.empty(blocks * 64, dtype=torch.uint8, device=device)
    self.copied = None      # behind the copies out of the pinned arenas
    self.done = None        # behind the kernels that read the device arenas


class _DeviceSlot(object):
  """One set of arenas of the device entropy mode: the pinned scan arena with its segment, table and scan-descriptor arrays in
  the place of the pinned coefficients, their device copies, the unit and DC scratch, and the statuses the device reports."""

  def __init__(self, batch, blocks, scan_bytes, segments, units, device):
    def pair(count, dtype=torch.uint8):
      return torch.zeros(count, dtype=dtype).pin_memory(), torch.zeros(count, dtype=dtype, device=device)
    self.scan_host, self.scan = pair(scan_bytes)
    self.segments_host, self.segments = pair(segments * SEGMENT_BYTES)
    self.tables_host, self.tables = pair(batch * TABLES * TABLE_BYTES)
    self.scans_host, self.scans = pair(batch * SCAN_BYTES)
    self.images_host, self.images = pair(batch * IMAGE_BYTES)
    self.qtables_host = torch.zeros((batch, 4, 64), dtype=torch.int16).pin_memory()      # uint16 bits
    self.qtables = torch.zeros((batch, 4, 64), dtype=torch.int16, device=device)
    self.status = np.zeros(batch, np.int32)      # the host's: header-level refusals
    self.scan_status_host, self.scan_status = pair(batch, torch.int32)      # the device's: those, and damaged scans
    self.units = torch.empty(units * UNIT_WORDS, dtype=torch.int32, device=device)
    self.dc = torch.empty(blocks, dtype=torch.int16, device=device)
    self.coef = torch.empty(blocks * 64, dtype=torch.int16, device=device)
    self.planes = torch.empty(blocks * 64, dtype=torch.uint8, device=device)
    self.unit_capacity = units
    self.copied = None
    self.done = None


class JpegDecoder(object):
  """Decodes batches of `batch` JPEG files into a canvas_h x canvas_w canvas each.  Allocates once: `depth` sets of pinned
  host arenas (coefficients, descriptors, quantisation tables), their device copies and the plane scratch, each sized for
  the worst supported case of the canvas.  threads: worker threads of the host stage, 1 .. 16, default min(16, batch);
  never taken from the machine's core count.

  max_ratio 2, 4 or 8: an image too large for the canvas is decoded at the smallest ratio <= max_ratio whose output fits it
  (the three *_scaled entry points; max_ratio=1 calls the full-size ones and allocates what it always did).  The coefficients
  of a file do not shrink with the ratio, so the arenas then hold coef_blocks 8x8 blocks per batch: by default four times the
  full-size worst case, batch * worst_blocks(canvas), at most max_ratio ** 2 times it (every image at the largest size that
  still fits).  A batch whose files together have more blocks runs out of arena: the image that no longer fits is TOO_LARGE.

  windowed=True: decode(windows=...) is allowed, and the arenas are sized for windows -- worst_window_blocks(canvas) in the
  place of worst_blocks(canvas), under the same rule for max_ratio and coef_blocks: a window that fits the canvas can lie in
  an image of any size, and keeps at most that many blocks at full size.

  entropy='device': the Huffman stage runs on the device (edet_jpeg_scan_prepare, edet_jpeg_entropy_device).  Per set the
  pinned coefficient arena and its copy give way to a pinned scan arena of scan_bytes bytes (default 64 per block of
  coef_blocks, half the pinned memory it replaces), a segment table of 64 rows per image plus one per eight blocks, the tables
  and scan descriptors, and on the device the unit scratch (32 bytes per unit: 8 scan_bytes / subseq_bits units and one more per
  segment) and two bytes of DC scratch per block.  A batch whose scans, segments or units do not fit gives TOO_LARGE for the
  image that no longer fits, on the host.  subseq_bits: the bits of a unit, a multiple of 32 from 64 to 8192; smaller units
  are more parallel and need more rounds to synchronise (LABNOTES has the measurements behind the default).  Every max_ratio
  works, since the coefficients do not depend on it; windowed=True does not (ValueError): a window needs the DC predictors of
  blocks it does not keep.  entropy='host', the default, allocates and calls exactly what it always did."""

  def __init__(self, batch, canvas_h, canvas_w, device='cuda:0', threads=None, depth=2, max_ratio=1, coef_blocks=None,
               windowed=False, entropy='host', subseq_bits=4096, scan_bytes=None):
    batch, canvas_h, canvas_w, depth = int(batch), int(canvas_h), int(canvas_w), int(depth)
    if entropy not in ENTROPIES:
      raise ValueError("entropy=%r: 'host' or 'device'" % (entropy,))
    if entropy == 'device' and windowed:
      raise ValueError("windowed=True needs entropy='host': the device entropy decoder does not skip blocks outside a window")
    subseq_bits = check_subseq_bits(subseq_bits)
    if scan_bytes is not None and entropy != 'device':
      raise ValueError("scan_bytes= needs entropy='device'")
    if scan_bytes is not None and not 16 <= int(scan_bytes) < 2 ** 31:
      raise ValueError('scan_bytes %d outside 16 .. 2^31 - 1' % scan_bytes)
    if max_ratio not in RATIOS:
      raise ValueError('max_ratio=%r: 1, 2, 4 or 8' % (max_ratio,))
    if batch < 1 or batch > 65535:
      raise ValueError('batch %d outside 1 .. 65535' % batch)
    if canvas_h < 1 or canvas_w < 1 or canvas_h > 65535 or canvas_w > 65535 or canvas_h * canvas_w * 3 >= 2 ** 31:
      raise ValueError('canvas %d x %d: sides of 1 .. 65535 and fewer than 2^31 bytes per image' % (canvas_h, canvas_w))
    if depth < 1:
      raise ValueError('depth %d < 1' % depth)
    if threads is None:
      threads = min(MAX_THREADS, batch)
    threads = int(threads)
    if threads < 1 or threads > MAX_THREADS:
      raise ValueError('threads %d outside 1 .. %d' % (threads, MAX_THREADS))
    self.windowed = bool(windowed)
    full = batch * (worst_window_blocks if self.windowed else worst_blocks)(canvas_h, canvas_w)
    most = max_ratio ** 2 * full
    if coef_blocks is None:
      coef_blocks = min(4, max_ratio ** 2) * full
    coef_blocks = int(coef_blocks)
    if coef_blocks < 1 or coef_blocks > most:
      raise ValueError('coef_blocks %d outside 1 .. %d: max_ratio ** 2 = %d times the %d blocks of %d full-size images that '
                       'fill the %d x %d canvas is all a batch can need' % (coef_blocks, most, max_ratio ** 2, full, batch,
                                                                           canvas_h, canvas_w))
    self.blocks, self.max_ratio = coef_blocks, int(max_ratio)
    if self.blocks >= 2 ** 31:
      raise ValueError('batch %d of %d x %d canvases: more than 2^31 blocks' % (batch, canvas_h, canvas_w))
    self.device = torch.device(device)
    if self.device.type != 'cuda' or not torch.cuda.is_available():
      raise _lib.EdetError('the JPEG decoder runs its inverse DCT and colour stage on the GPU (edet_jpeg_idct / '
                           'edet_jpeg_color): there is no CPU fall-back')
    _lib.load()
    self.batch, self.canvas_h, self.canvas_w, self.threads, self.depth = batch, canvas_h, canvas_w, threads, depth
    self.entropy, self.subseq_bits = entropy, subseq_bits
    if entropy == 'device':
      scan_bytes = 64 * self.blocks if scan_bytes is None else int(scan_bytes)
      if scan_bytes >= 2 ** 31:
        raise ValueError('batch %d of %d x %d canvases: a scan arena of 2^31 bytes or more; pass scan_bytes=' % (batch, canvas_h, canvas_w))
      self.scan_bytes = (scan_bytes + 15) // 16 * 16
      self.segments = 64 * batch + self.blocks // 8
      units = 8 * self.scan_bytes // subseq_bits + self.segments
      self._slots = [_DeviceSlot(batch, self.blocks, self.scan_bytes, self.segments, units, self.device) for _ in range(depth)]
    else:
      self._slots = [_Slot(batch, self.blocks, self.device, self.windowed) for _ in range(depth)]
    self._next = 0
    self._last = None      # the set of the most recent decode

  def decode(self, contents, out=None, sizes_out=None, fallback=None, stream=None, ratios=None, ratios_out=None,
             windows=None, check_scan=False):
    """contents: `batch` JPEG files as bytes -> (raw uint8 [B, Hc, Wc, 3] on the device, sizes int32 [B, 2] = (height,
    width) on the host): exactly pad_batch(decoded images, (Hc, Wc)).  out / sizes_out: where to write them (out a
    contiguous device tensor; every byte of it is written, so it needs no clearing).  A refused stream raises ValueError
    with its index and the reason, unless `fallback` is given: a callable from the bytes to a uint8 [h, w, 3] array, whose
    result is copied into that image's canvas behind the kernels.  stream: a torch.cuda.Stream, default the current one.
    The call does not wait for the device: one asynchronous copy per arena and the two launches go on `stream`.  A pinned
    arena is written again only when the event behind its last copy has completed, and the decoder rotates through its
    `depth` sets, so the host stage of one batch overlaps the device stage of the batch before.
    With max_ratio > 1 the sizes are the OUTPUT sizes.  ratios: one ratio per image (1, 2, 4 or 8, none above max_ratio) to use
    instead of the chosen one; an output that does not fit the canvas is TOO_LARGE.  ratios_out: a numpy int32 [B] array that
    receives the ratio each image was decoded at (1 for an image that went to `fallback`).
    windows (a decoder built with windowed=True): int [B, 4] = (y, x, h, w) per image, in the coordinates of the image's
    OUTPUT at its ratio -- ratios[i], or 1 throughout when max_ratio is 1; with max_ratio > 1 ratios must be given, since a
    window belongs to one ratio.  Each canvas holds its window at the top-left, zero elsewhere, and sizes its (h, w).  A window
    outside its image is refused like a stream (status WINDOW); so is one larger than the canvas (TOO_LARGE), while the image
    around it may be of any size.  A stream that goes to `fallback` comes back WHOLE, uncropped, with the fallback image's
    size.  windows=None calls the entry points it always did.
    check_scan (entropy='device' only; it changes nothing in host mode, where the scan is decoded before the call returns):
    False, the default -- the call does not wait for the device, so a stream damaged inside its scan (a truncated file, a bad
    code, too few blocks) is NOT reported here: its canvas comes out all zero, sizes_out keeps its header size, and
    scan_status() tells afterwards.  True -- the call waits for the batch and then behaves as the host mode does: ValueError
    with the index and the reason, or the `fallback` image copied in."""
    if len(contents) != self.batch:
      raise ValueError('%d files for a decoder of batch %d' % (len(contents), self.batch))
    b, hc, wc = self.batch, self.canvas_h, self.canvas_w
    if out is None:
      out = torch.empty((b, hc, wc, 3), dtype=torch.uint8, device=self.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and tuple(out.shape) == (b, hc, wc, 3) and
              out.device == self.device and out.is_contiguous()):
      raise ValueError('out must be a contiguous uint8 [%d, %d, %d, 3] tensor on %s' % (b, hc, wc, self.device))
    if sizes_out is None:
      sizes_out = np.zeros((b, 2), np.int32)
    elif not (isinstance(sizes_out, np.ndarray) and sizes_out.dtype == np.int32 and sizes_out.shape == (b, 2)):
      raise ValueError('sizes_out must be a numpy int32 [%d, 2] array' % b)
    if ratios is not None:
      ratios = [int(r) for r in ratios]
      if len(ratios) != b or any(r not in RATIOS or r > self.max_ratio for r in ratios):
        raise ValueError('ratios must be %d values of 1, 2, 4 or 8, none above max_ratio=%d' % (b, self.max_ratio))
    if ratios_out is not None and not (isinstance(ratios_out, np.ndarray) and ratios_out.dtype == np.int32 and
                                       ratios_out.shape == (b,)):
      raise ValueError('ratios_out must be a numpy int32 [%d] array' % b)
    if windows is not None:
      if not self.windowed:
        raise ValueError('windows= needs a decoder built with windowed=True')
      if ratios is None and self.max_ratio > 1:
        raise ValueError('windows= with max_ratio=%d needs ratios=: a window is in the coordinates of one ratio' % self.max_ratio)
      windows = np.asarray(windows)
      if windows.shape != (b, 4) or windows.dtype.kind not in 'iu':
        raise ValueError('windows must be int [%d, 4] = (y, x, h, w) per file' % b)
    scaled = self.max_ratio > 1 or windows is not None
    slot = self._slots[self._next]
    self._next = (self._next + 1) % self.depth
    self._last = slot
    if slot.copied is not None:
      slot.copied.synchronize()      # the device has read this set's pinned arenas
    used_scan = None
    if self.entropy == 'device':
      used_scan = scan_prepare(contents, hc, wc, self.max_ratio, ratios, self.blocks * 64, self.subseq_bits, slot.scan_host,
                               slot.segments_host, slot.unit_capacity, slot.tables_host, slot.scans_host, slot.images_host,
                               slot.qtables_host, slot.status, self.threads)
    elif windows is not None:
      entropy_decode_window(contents, hc, wc, self.max_ratio, ratios, windows, slot.coef_host, slot.images_host,
                            slot.windows_host, slot.qtables_host, slot.status, self.threads)
      wdesc = window_descriptors(slot.windows_host, b)
    elif scaled:
      entropy_decode_scaled(contents, hc, wc, self.max_ratio, ratios, slot.coef_host, slot.images_host, slot.qtables_host,
                            slot.status, self.threads)
    else:
      entropy_decode(contents, hc, wc, slot.coef_host, slot.images_host, slot.qtables_host, slot.status, self.threads)
    desc = descriptors(slot.images_host, b)
    if ratios_out is not None:
      ratios_out[:] = [max(int(d.reserved), 1) for d in desc]
    filled = {}
    for i, d in enumerate(desc):
      if d.status:
        if fallback is None:
          why = self._reason(contents[i], d.status, None if ratios is None else ratios[i], windows is not None)
          raise ValueError('contents[%d] is not decoded: %s (status %d)' % (i, why, d.status))
        img = self._fallback_image(fallback, contents[i], i)
        filled[i] = img
        sizes_out[i] = (img.shape[0], img.shape[1])
      else:
        sizes_out[i] = (wdesc[i].h, wdesc[i].w) if windows is not None else (d.height, d.width)
    used = max([d.first_block[0] + d.total_blocks for d in desc if not d.status] or [0])
    most = max([d.total_blocks for d in desc] or [0])
    st = torch.cuda.current_stream(self.device) if stream is None else stream
    with torch.cuda.device(self.device), torch.cuda.stream(st):
      if slot.done is not None:
        st.wait_event(slot.done)      # (a device-side wait: the set's last kernels may have run on another stream)
      if used_scan is not None:
        nbytes, nseg = used_scan[0], used_scan[1] * SEGMENT_BYTES
        if nbytes:
          slot.scan[:nbytes].copy_(slot.scan_host[:nbytes], non_blocking=True)
        if nseg:
          slot.segments[:nseg].copy_(slot.segments_host[:nseg], non_blocking=True)
        slot.tables.copy_(slot.tables_host, non_blocking=True)
        slot.scans.copy_(slot.scans_host, non_blocking=True)
      elif used:
        slot.coef[:used * 64].copy_(slot.coef_host[:used * 64], non_blocking=True)
      slot.images.copy_(slot.images_host, non_blocking=True)
      slot.qtables.copy_(slot.qtables_host, non_blocking=True)
      if windows is not None:
        slot.windows.copy_(slot.windows_host, non_blocking=True)
      slot.copied = torch.cuda.Event()
      slot.copied.record(st)
      raw = st.cuda_stream
      if used_scan is not None:
        # the descriptor of an image the device refuses gets its status THERE, in front of the two kernels below
        call('edet_jpeg_entropy_device', ptr(slot.scan), self.scan_bytes, ptr(slot.segments), self.segments, ptr(slot.tables),
             ptr(slot.scans), ptr(slot.images), b, self.subseq_bits, ptr(slot.units), slot.unit_capacity, ptr(slot.dc),
             ptr(slot.coef), self.blocks * 64, ptr(slot.scan_status), raw)
      call('edet_jpeg_idct_scaled' if scaled else 'edet_jpeg_idct', ptr(slot.coef), ptr(slot.images), ptr(slot.qtables), b,
           most, ptr(slot.planes), self.blocks * 64, raw)
      if windows is not None:
        call('edet_jpeg_color_window', ptr(slot.planes), ptr(slot.images), ptr(slot.windows), b, hc, wc, self.blocks * 64,
             ptr(out), raw)
      else:
        call('edet_jpeg_color_scaled' if scaled else 'edet_jpeg_color', ptr(slot.planes), ptr(slot.images), b, hc, wc,
             self.blocks * 64, ptr(out), raw)
      if used_scan is not None:
        slot.scan_status_host.copy_(slot.scan_status, non_blocking=True)
      slot.done = torch.cuda.Event()
      slot.done.record(st)
      for i, img in filled.items():
        out[i, :img.shape[0], :img.shape[1]].copy_(img, non_blocking=True)
      if used_scan is not None and check_scan:
        slot.done.synchronize()
        found = slot.scan_status_host.numpy()
        for i in range(b):
          if found[i] and not desc[i].status:      # damaged inside the scan: its canvas is zero
            if fallback is None:
              raise ValueError('contents[%d] is not decoded: %s (status %d)' % (i, REASONS.get(int(found[i]), '?'), found[i]))
            img = self._fallback_image(fallback, contents[i], i)
            sizes_out[i] = (img.shape[0], img.shape[1])
            if ratios_out is not None:
              ratios_out[i] = 1
            out[i, :img.shape[0], :img.shape[1]].copy_(img, non_blocking=True)
    return out, sizes_out

  def _fallback_image(self, fallback, content, i):
    img = fallback(content)
    img = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
    if not torch.is_tensor(img) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or \
        not (1 <= img.shape[0] <= self.canvas_h and 1 <= img.shape[1] <= self.canvas_w):
      raise ValueError('fallback(contents[%d]) must be uint8 [h, w, 3] inside the %d x %d canvas' % (i, self.canvas_h, self.canvas_w))
    return img

  def scan_status(self, wait=True):
    """The int32 [batch] statuses of the most recent decode(): 0, or the reason an image's canvas holds no decoded pixels.  In
    the device entropy mode these come from the device and include the streams damaged inside their scans, which decode()
    without check_scan does not report; wait=True waits for that batch, wait=False returns None while it is still running.
    In host mode they are the host stage's.  None before the first decode()."""
    slot = self._last
    if slot is None:
      return None
    if self.entropy != 'device':
      return slot.status.copy()
    if slot.done is None:      # (a decode() that raised in front of its launches)
      return None
    if wait:
      slot.done.synchronize()
    elif not slot.done.query():
      return None
    return slot.scan_status_host.numpy().copy()

  def scan_failures(self, ahead=0):
    """entropy='device': the indices of the images the DEVICE refused (streams damaged inside their scans) in the batch that
    last used the set of arenas the next decode() will use -- `ahead` further decodes on -- as a list; [] for a set not used
    yet, and in host mode.  Waits for that batch, which the next decode() on that set does anyway before it writes the set's
    pinned arenas; a reader calls this in front of decode() to learn, `depth` batches late, what decode() could not tell."""
    slot = self._slots[(self._next + int(ahead)) % self.depth]
    if self.entropy != 'device' or slot.done is None:
      return []
    slot.done.synchronize()
    found = slot.scan_status_host.numpy()
    return [i for i in range(self.batch) if found[i] and not slot.status[i]]

  def scan_rounds(self):
    """entropy='device': the int32 [batch] rounds the device ran per image of the most recent decode() (round 0 included; 0
    for an image it did not decode).  Waits for that batch and copies the descriptors back: a measurement aid."""
    if self.entropy != 'device' or self._last is None:
      return None
    self._last.done.synchronize()
    return np.array([d.rounds for d in scan_descriptors(self._last.scans.cpu(), self.batch)], np.int32)

  def _reason(self, content, status, forced=None, windowed=False):
    """REASONS[status]; for TOO_LARGE with max_ratio > 1 it says which of the two limits the image met."""
    if windowed and status == TOO_LARGE:
      return ('a crop window larger than the %d x %d canvas, or no room left in the coefficient arena of coef_blocks=%d blocks'
              % (self.canvas_h, self.canvas_w, self.blocks))
    if status == TOO_LARGE and self.entropy == 'device':
      try:
        info = jpeg_info(content)
        ratio = forced if forced is not None else choose_ratio(info.height, info.width, self.canvas_h, self.canvas_w, self.max_ratio)
        h, w = scaled_size(info.height, info.width, ratio) if ratio else (self.canvas_h + 1, 0)
        if h <= self.canvas_h and w <= self.canvas_w:
          return ('no room left for this %d x %d image in the scan arena of scan_bytes=%d bytes, its %d segments or its units, or '
                  'in the coefficient arena of coef_blocks=%d blocks; raise them or pass fallback='
                  % (info.height, info.width, self.scan_bytes, self.segments, self.blocks))
      except ValueError:
        pass
    if status != TOO_LARGE or self.max_ratio == 1:
      return REASONS.get(int(status), '?')
    try:
      info = jpeg_info(content)
    except ValueError:
      return REASONS[TOO_LARGE]
    if forced is not None:
      h, w = scaled_size(info.height, info.width, forced)
      if h > self.canvas_h or w > self.canvas_w:
        return '%s at the ratio %d asked for (%d x %d of %d x %d)' % (REASONS[TOO_LARGE], forced, h, w, info.height, info.width)
    elif choose_ratio(info.height, info.width, self.canvas_h, self.canvas_w, self.max_ratio) is None:
      return '%s even at ratio %d (%d x %d)' % (REASONS[TOO_LARGE], self.max_ratio, info.height, info.width)
    return ('no room left in the coefficient arena of coef_blocks=%d blocks for this %d x %d image: the files of a batch '
            'keep all their blocks whatever the ratio; raise coef_blocks or pass fallback=' % (self.blocks, info.height,
                                                                                              info.width))


def decode_jpeg(contents, channels=3, ratio=1, entropy='host'):
  """tf.io.decode_jpeg(contents, channels, ratio) with its defaults otherwise -> uint8 [ceil(height / ratio), ceil(width /
  ratio), 3] on the device.  channels: 0 (the file's own; a greyscale file still comes out replicated, as
  decode_image(channels=3) gives it) or 3.  ratio: 1, 2, 4 or 8, libjpeg's reduced-size decode.  entropy: 'host' or 'device', where the
  Huffman stage runs (JpegDecoder); the result is the same.  A stream that is not decoded raises ValueError naming the reason
  (the device mode waits for the device to say so: check_scan=True)."""
  if entropy not in ENTROPIES:
    raise ValueError("entropy=%r: 'host' or 'device'" % (entropy,))
  if channels not in (0, 3):
    raise ValueError('channels=%r: 0 or 3 (a greyscale file is replicated to three channels)' % (channels,))
  if ratio not in RATIOS:
    raise ValueError('ratio=%r: 1, 2, 4 or 8' % (ratio,))
  info = jpeg_info(contents)
  if info.height < 1 or info.width < 1:
    raise ValueError('contents is not decoded: %s (status %d)' % (REASONS[MALFORMED], MALFORMED))
  mode = {} if entropy == 'host' else {'entropy': entropy}
  # (a scan of noise at quality 100 can outgrow 64 bytes a block: the file itself bounds it)
  room = {} if entropy == 'host' else {'scan_bytes': _buffer(contents)[2] + 64}
  if ratio == 1:
    raw, _ = JpegDecoder(1, info.height, info.width, depth=1, **mode, **room).decode([contents], **({'check_scan': True} if mode else {}))
  else:
    h, w = scaled_size(info.height, info.width, ratio)
    raw, _ = JpegDecoder(1, h, w, depth=1, max_ratio=ratio, coef_blocks=worst_blocks(info.height, info.width), **mode,
                         **room).decode([contents], ratios=[ratio], **({'check_scan': True} if mode else {}))
  return raw[0]


def decode_and_crop_jpeg(contents, crop_window, channels=3, ratio=1):
  """tf.image.decode_and_crop_jpeg(contents, crop_window, channels, ratio) with its defaults otherwise -> uint8 [h, w, 3] on
  the device: decode_jpeg(contents, channels, ratio)[y:y + h, x:x + w] byte for byte, of which only the blocks the window needs
  are copied to the device and transformed.  crop_window = (y, x, h, w) in pixels of the output at `ratio`; one that does not
  lie inside it, or has a side below 1, raises ValueError, as does a stream that is not decoded."""
  if channels not in (0, 3):
    raise ValueError('channels=%r: 0 or 3 (a greyscale file is replicated to three channels)' % (channels,))
  if ratio not in RATIOS:
    raise ValueError('ratio=%r: 1, 2, 4 or 8' % (ratio,))
  window = np.asarray(crop_window)
  if window.shape != (4,) or window.dtype.kind not in 'iu':
    raise ValueError('crop_window must be four integers (y, x, h, w), got %r' % (crop_window,))
  info = jpeg_info(contents)
  if info.height < 1 or info.width < 1:
    raise ValueError('contents is not decoded: %s (status %d)' % (REASONS[MALFORMED], MALFORMED))
  blocks = window_grid(info, window, ratio)[1]      # (raises for a window outside the image)
  h, w = int(window[2]), int(window[3])
  raw, _ = JpegDecoder(1, h, w, depth=1, max_ratio=ratio, coef_blocks=blocks, windowed=True).decode(
      [contents], windows=window[None], ratios=[ratio])
  return raw[0]
