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
truncated streams.  Not built: EXIF orientation (TensorFlow ignores it too), PNG / GIF / BMP, decode_and_crop_jpeg,
dct_method, fancy_upscaling=False.  (TFRecord / tf.Example input is automl_amd/dataloader.py.)

Reduced size: tf.io.decode_jpeg's `ratio` 2, 4 and 8 is libjpeg's scale_denom -- a block is inverse-transformed straight to
4x4, 2x2 or 1x1 samples (jidctred.c), so the image comes out ceil(height / ratio) x ceil(width / ratio) at a fraction of the
device work (csrc/jpeg_scaled.hip: edet_jpeg_idct_scaled, edet_jpeg_color_scaled; restated in tests/jpeg_scaled_ref.py and
compared with Pillow's draft mode).  JpegDecoder(max_ratio=8) picks per image the smallest ratio whose output fits the canvas
(choose_ratio), so a file of several thousand pixels a side lands in a 512 x 512 canvas instead of being TOO_LARGE; the Huffman
stage and the coefficient copy still see the whole file.  max_ratio=1, the default, is the full-size decoder unchanged.
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
KINDS = ('baseline', 'extended', 'progressive', 'other')
MAX_THREADS = 16
IMAGE_BYTES = ctypes.sizeof(_lib.JpegImage)      # 80

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


def entropy_decode(datas, canvas_h, canvas_w, coef, images, qtables, status, threads=0):
  """edet_jpeg_entropy_decode on host arrays (numpy or CPU tensors): coef int16 [capacity], images uint8 [B * 80], qtables
  uint16 [B, 4, 64], status int32 [B].  Blocks until the batch is decoded; needs no device.  The streams are read where they
  lie (_buffer): nothing is copied, so a memoryview into a mapped file goes to the workers as it is."""
  n = len(datas)
  keep = [_buffer(d, 'contents[%d]' % i) for i, d in enumerate(datas)]      # alive until the call returns
  ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(d), ctypes.c_void_p) if isinstance(d, bytes) else d
                                 for _, d, _ in keep])
  sizes = (ctypes.c_size_t * n)(*[size for _, _, size in keep])

  def host(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
  capacity = int(coef.size if isinstance(coef, np.ndarray) else coef.numel())
  call('edet_jpeg_entropy_decode', ptrs, sizes, n, int(canvas_h), int(canvas_w), host(coef), capacity, host(images),
       host(qtables), host(status), int(threads))


def entropy_decode_scaled(datas, canvas_h, canvas_w, max_ratio, ratios, coef, images, qtables, status, threads=0):
  """edet_jpeg_entropy_decode_scaled on host arrays, as entropy_decode: ratios None (each image gets choose_ratio's answer)
  or one forced ratio per image.  The descriptors' height / width are the output sizes, `reserved` the ratio."""
  n = len(datas)
  keep = [_buffer(d, 'contents[%d]' % i) for i, d in enumerate(datas)]      # alive until the call returns
  ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(d), ctypes.c_void_p) if isinstance(d, bytes) else d
                                 for _, d, _ in keep])
  sizes = (ctypes.c_size_t * n)(*[size for _, _, size in keep])
  forced = None
  if ratios is not None:
    if len(ratios) != n:
      raise ValueError('%d ratios for %d files' % (len(ratios), n))
    forced = (ctypes.c_int32 * n)(*[int(r) for r in ratios])

  def host(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
  capacity = int(coef.size if isinstance(coef, np.ndarray) else coef.numel())
  call('edet_jpeg_entropy_decode_scaled', ptrs, sizes, n, int(canvas_h), int(canvas_w), int(max_ratio),
       None if forced is None else ctypes.addressof(forced), host(coef), capacity, host(images), host(qtables), host(status),
       int(threads))


def descriptors(images, batch):
  """The per-image array as a list of _lib.JpegImage (copies)."""
  raw = images.tobytes() if isinstance(images, np.ndarray) else images.numpy().tobytes()
  return [_lib.JpegImage.from_buffer_copy(raw, i * IMAGE_BYTES) for i in range(batch)]


class _Slot(object):
  """One set of arenas: pinned host memory the host stage writes, its device copy, the plane scratch, and the event behind
  the copies."""

  def __init__(self, batch, blocks, device):
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


class JpegDecoder(object):
  """Decodes batches of `batch` JPEG files into a canvas_h x canvas_w canvas each.  Allocates once: `depth` sets of pinned
  host arenas (coefficients, descriptors, quantisation tables), their device copies and the plane scratch, each sized for
  the worst supported case of the canvas.  threads: worker threads of the host stage, 1 .. 16, default min(16, batch);
  never taken from the machine's core count.

  max_ratio 2, 4 or 8: an image too large for the canvas is decoded at the smallest ratio <= max_ratio whose output fits it
  (the three *_scaled entry points; max_ratio=1 calls the full-size ones and allocates what it always did).  The coefficients
  of a file do not shrink with the ratio, so the arenas then hold coef_blocks 8x8 blocks per batch: by default four times the
  full-size worst case, batch * worst_blocks(canvas), at most max_ratio ** 2 times it (every image at the largest size that
  still fits).  A batch whose files together have more blocks runs out of arena: the image that no longer fits is TOO_LARGE."""

  def __init__(self, batch, canvas_h, canvas_w, device='cuda:0', threads=None, depth=2, max_ratio=1, coef_blocks=None):
    batch, canvas_h, canvas_w, depth = int(batch), int(canvas_h), int(canvas_w), int(depth)
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
    full = batch * worst_blocks(canvas_h, canvas_w)
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
    self._slots = [_Slot(batch, self.blocks, self.device) for _ in range(depth)]
    self._next = 0

  def decode(self, contents, out=None, sizes_out=None, fallback=None, stream=None, ratios=None, ratios_out=None):
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
    receives the ratio each image was decoded at (1 for an image that went to `fallback`)."""
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
    scaled = self.max_ratio > 1
    slot = self._slots[self._next]
    self._next = (self._next + 1) % self.depth
    if slot.copied is not None:
      slot.copied.synchronize()      # the device has read this set's pinned arenas
    if scaled:
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
          why = self._reason(contents[i], d.status, None if ratios is None else ratios[i])
          raise ValueError('contents[%d] is not decoded: %s (status %d)' % (i, why, d.status))
        img = fallback(contents[i])
        img = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
        if not torch.is_tensor(img) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or \
            not (1 <= img.shape[0] <= hc and 1 <= img.shape[1] <= wc):
          raise ValueError('fallback(contents[%d]) must be uint8 [h, w, 3] inside the %d x %d canvas' % (i, hc, wc))
        filled[i] = img
        sizes_out[i] = (img.shape[0], img.shape[1])
      else:
        sizes_out[i] = (d.height, d.width)
    used = max([d.first_block[0] + d.total_blocks for d in desc if not d.status] or [0])
    most = max([d.total_blocks for d in desc] or [0])
    st = torch.cuda.current_stream(self.device) if stream is None else stream
    with torch.cuda.device(self.device), torch.cuda.stream(st):
      if slot.done is not None:
        st.wait_event(slot.done)      # (a device-side wait: the set's last kernels may have run on another stream)
      if used:
        slot.coef[:used * 64].copy_(slot.coef_host[:used * 64], non_blocking=True)
      slot.images.copy_(slot.images_host, non_blocking=True)
      slot.qtables.copy_(slot.qtables_host, non_blocking=True)
      slot.copied = torch.cuda.Event()
      slot.copied.record(st)
      raw = st.cuda_stream
      call('edet_jpeg_idct_scaled' if scaled else 'edet_jpeg_idct', ptr(slot.coef), ptr(slot.images), ptr(slot.qtables), b,
           most, ptr(slot.planes), self.blocks * 64, raw)
      call('edet_jpeg_color_scaled' if scaled else 'edet_jpeg_color', ptr(slot.planes), ptr(slot.images), b, hc, wc,
           self.blocks * 64, ptr(out), raw)
      slot.done = torch.cuda.Event()
      slot.done.record(st)
      for i, img in filled.items():
        out[i, :img.shape[0], :img.shape[1]].copy_(img, non_blocking=True)
    return out, sizes_out

  def _reason(self, content, status, forced=None):
    """REASONS[status]; for TOO_LARGE with max_ratio > 1 it says which of the two limits the image met."""
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


def decode_jpeg(contents, channels=3, ratio=1):
  """tf.io.decode_jpeg(contents, channels, ratio) with its defaults otherwise -> uint8 [ceil(height / ratio), ceil(width /
  ratio), 3] on the device.  channels: 0 (the file's own; a greyscale file still comes out replicated, as
  decode_image(channels=3) gives it) or 3.  ratio: 1, 2, 4 or 8, libjpeg's reduced-size decode.  A stream that is not decoded
  raises ValueError naming the reason."""
  if channels not in (0, 3):
    raise ValueError('channels=%r: 0 or 3 (a greyscale file is replicated to three channels)' % (channels,))
  if ratio not in RATIOS:
    raise ValueError('ratio=%r: 1, 2, 4 or 8' % (ratio,))
  info = jpeg_info(contents)
  if info.height < 1 or info.width < 1:
    raise ValueError('contents is not decoded: %s (status %d)' % (REASONS[MALFORMED], MALFORMED))
  if ratio == 1:
    raw, _ = JpegDecoder(1, info.height, info.width, depth=1).decode([contents])
  else:
    h, w = scaled_size(info.height, info.width, ratio)
    raw, _ = JpegDecoder(1, h, w, depth=1, max_ratio=ratio, coef_blocks=worst_blocks(info.height, info.width)).decode(
        [contents], ratios=[ratio])
  return raw[0]
