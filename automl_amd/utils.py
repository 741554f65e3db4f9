"""Shape helpers of the detection path (reference efficientdet/utils.py:484-526) and the packing of a host generator's state
that both trainers put into their optimizer state."""
import numpy as np


def parse_image_size(image_size):
  """int | 'WxH' string | (H, W) tuple -> (height, width)."""
  if isinstance(image_size, int):
    return (image_size, image_size)
  if isinstance(image_size, str):
    width, height = image_size.lower().split('x')
    return (int(height), int(width))
  if isinstance(image_size, (tuple, list)):
    return tuple(image_size)
  raise ValueError('image_size must be an int, WxH string, or (height, width)'
                   'tuple. Was %r' % (image_size,))


def get_feat_sizes(image_size, max_level):
  """Feature (height, width) per level 0..max_level: s_{l+1} = (s_l - 1)//2 + 1."""
  h, w = parse_image_size(image_size)
  sizes = [{'height': h, 'width': w}]
  for _ in range(max_level):
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    sizes.append({'height': h, 'width': w})
  return sizes


def same_padding(in_size, kernel, stride):
  """TensorFlow 'SAME' geometry: (out_size, pad_before, pad_after).

  out = ceil(in/stride); total = max((out-1)*stride + kernel - in, 0);
  before = total//2 (the extra pixel goes after: asymmetric for stride 2 on
  even inputs).  Used by every stencil kernel and by the oracle.
  """
  out = -(-in_size // stride)
  total = max((out - 1) * stride + kernel - in_size, 0)
  return out, total // 2, total - total // 2


def pack_rng_state(rng):
  """PCG64 state -> uint64 [6] (state and increment as two words each, the buffered 32-bit half)."""
  st = rng.bit_generator.state
  m = (1 << 64) - 1
  s, inc = int(st['state']['state']), int(st['state']['inc'])
  return np.array([s & m, s >> 64, inc & m, inc >> 64, int(st['has_uint32']), int(st['uinteger'])], dtype=np.uint64)


def unpack_rng_state(rng, words):
  v = [int(x) for x in np.asarray(words, dtype=np.uint64)]
  rng.bit_generator.state = {'bit_generator': 'PCG64', 'state': {'state': v[0] | (v[1] << 64), 'inc': v[2] | (v[3] << 64)},
                             'has_uint32': v[4], 'uinteger': v[5]}


def canvas_sizes(sizes, batch, canvas_h, canvas_w):
  """The (height, width) of every image of a canvas batch [batch, canvas_h, canvas_w, 3] -- image i is the top-left
  sizes[i] of its slot, as jpeg.JpegDecoder.decode returns them -- checked -> int32 numpy [batch, 2].  Sizes are HOST data: a
  numpy array, a list or a CPU tensor; a device tensor is copied to the host once, and that copy waits for the device.  A
  wrong shape or a size outside [1, canvas] raises a ValueError that names the image."""
  if hasattr(sizes, 'detach'):      # a torch tensor
    sizes = sizes.detach().cpu().numpy()
  s = np.asarray(sizes)
  if s.shape != (int(batch), 2) or s.dtype.kind not in 'iu':
    raise ValueError('sizes must be integers [batch, 2] = (height, width) per image, batch %d, got %s %s'
                     % (batch, s.dtype, s.shape))
  bad = np.flatnonzero((s[:, 0] < 1) | (s[:, 0] > int(canvas_h)) | (s[:, 1] < 1) | (s[:, 1] > int(canvas_w)))
  if bad.size:
    i = int(bad[0])
    raise ValueError('image %d: size %d x %d is outside [1, canvas] of the %d x %d canvas'
                     % (i, int(s[i, 0]), int(s[i, 1]), canvas_h, canvas_w))
  return np.ascontiguousarray(s, dtype=np.int32)
