"""Generates tests/golden/jpeg_cases.npz with Pillow (libjpeg-turbo): per case the encoded bytes and the RGB pixels Pillow
decodes from them, or for a refused file the status automl_amd/jpeg.py has to give.  The GPU tests read only the .npz.

The images are a structure (gradients, a sinusoid, a rectangle) plus noise, so that every AC position and the ZRL code
occur (asserted below through the restatement's coefficients); one image is constant (EOB only).  The sizes are the smallest
at which each part of the decoder can go wrong: 1x1; 8x9 (one column into a second block); 16x16 (exactly one 4:2:0 MCU);
17x33, 31x22 and 37x53 (partial MCUs, chroma edge replication right and bottom); 24x280 (more than 32 blocks per block row);
each with 4:4:4, 4:2:2 and 4:2:0.  Besides: greyscale, quality 30 / 95 / 100, optimize=True (file-specific Huffman tables), a
restart interval, APPn / COM segments in front of the frame, the refused kinds, and one 640x480 4:2:0 image for the
whole-size run and scripts/bench_jpeg.py (flat tiles outside a strip of gradients and a noisy patch, to keep this file small).

Run where Pillow is installed:  python tests/golden/make_golden_jpeg.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import jpeg_ref as jr   # noqa: E402

OUT = os.path.join(HERE, 'jpeg_cases.npz')
SIZES = [(1, 1), (8, 9), (16, 16), (17, 33), (31, 22), (37, 53), (24, 280)]
SUBSAMPLING = {'444': 0, '422': 1, '420': 2}


def picture(h, w, seed, noise=48.0):
  rng = np.random.default_rng(seed)
  y, x = np.mgrid[0:h, 0:w].astype(np.float64)
  img = np.stack([255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1),
                  127.5 + 127.5 * np.sin(0.9 * x + 0.37 * y)], axis=2)
  img[h // 4:h // 2 + 1, w // 3:w // 3 * 2 + 1] = (250.0, 10.0, 128.0)
  img += rng.normal(0.0, noise, img.shape)
  return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def big_picture():
  """480 x 640: flat 32 x 32 tiles (they decode to flat blocks, which compress), one strip of gradients, one noisy patch."""
  h, w = 480, 640
  rng = np.random.default_rng(7)
  tiles = rng.integers(0, 256, (h // 32, w // 32, 3)).astype(np.uint8)
  img = np.repeat(np.repeat(tiles, 32, axis=0), 32, axis=1)
  y, x = np.mgrid[0:64, 0:w].astype(np.float64)
  strip = np.stack([255.0 * x / (w - 1), 255.0 * y / 63.0, 127.5 + 127.5 * np.sin(x / 37.0) * np.cos(y / 23.0)], axis=2)
  img[128:192] = np.clip(np.rint(strip), 0, 255).astype(np.uint8)
  img[300:396, 64:192] = picture(96, 128, 99)
  return img


def encode(img, mode='RGB', **kw):
  buf = io.BytesIO()
  Image.fromarray(img, mode).save(buf, 'JPEG', **kw)
  return buf.getvalue()


def pillow_rgb(data):
  return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def main():
  ok, refused = {}, {}
  for k, (h, w) in enumerate(SIZES):
    img = picture(h, w, 10 + k)
    for name, sub in SUBSAMPLING.items():
      ok['s%dx%d_%s_q75' % (h, w, name)] = encode(img, quality=75, subsampling=sub)
  img = picture(37, 53, 15)
  for q in (30, 95, 100):
    for name, sub in SUBSAMPLING.items():
      ok['s37x53_%s_q%d' % (name, q)] = encode(img, quality=q, subsampling=sub)
  for (h, w), q in (((16, 16), 75), ((19, 13), 90)):
    ok['grey_%dx%d_q%d' % (h, w, q)] = encode(picture(h, w, 30 + h)[:, :, 1], 'L', quality=q)
  ok['const_20x20_420'] = encode(np.full((20, 20, 3), (200, 50, 90), np.uint8), quality=75, subsampling=2)
  for name, sub in SUBSAMPLING.items():
    ok['optimize_31x22_%s' % name] = encode(picture(31, 22, 14), quality=85, subsampling=sub, optimize=True)
  rst = encode(picture(24, 280, 16), quality=75, subsampling=2, restart_marker_blocks=2)      # 36 MCUs: RST0 .. RST7 and round again
  assert b'\xff\xdd\x00\x04\x00\x02' in rst and b'\xff\xd0' in rst and b'\xff\xd7' in rst, 'no restart interval in the file'
  ok['restart_24x280_420'] = rst
  plain = ok['s17x33_422_q75']
  segs = b'\xff\xfe\x00\x07hello' + b'\xff\xe5\x00\x06\xff\xd9\x00\x01' + b'\xff\xe1\x00\x08Exif\x00\x00'
  ok['segments_17x33_422'] = plain[:2] + segs + plain[2:]
  ok['big_480x640_420'] = encode(big_picture(), quality=75, subsampling=2)

  refused['progressive_17x33'] = (encode(picture(17, 33, 13), quality=75, progressive=True), jr.PROGRESSIVE)
  cmyk = np.concatenate([picture(16, 16, 5), picture(16, 16, 6)[:, :, :1]], axis=2)
  refused['cmyk_16x16'] = (encode(cmyk, 'CMYK', quality=75), jr.COMPONENTS)
  whole = ok['s17x33_420_q75']
  scan = whole.index(b'\xff\xda')
  refused['truncated_17x33'] = (whole[:scan + (len(whole) - scan) // 2], jr.MALFORMED)
  dht = whole.index(b'\xff\xc4')
  counts = bytearray(whole[dht + 5:dht + 21])
  big = max(range(16), key=lambda i: counts[i])
  assert counts[0] == 0 and counts[big] >= 3
  counts[0] += 3      # three codes of one bit
  counts[big] -= 3
  refused['huffman_17x33'] = (whole[:dht + 5] + bytes(counts) + whole[dht + 21:], jr.MALFORMED)

  out = {'names': np.array(sorted(ok)), 'refused': np.array(sorted(refused))}
  positions = np.zeros(64, bool)
  zrl = False
  for name, data in ok.items():
    rgb = pillow_rgb(data)
    assert np.array_equal(jr.decode(data), rgb), name      # the restatement equals Pillow, byte for byte
    out[name + '/bytes'] = np.frombuffer(data, np.uint8)
    out[name + '/rgb'] = rgb
    if not name.startswith('big'):
      dec = jr.parse(data)
      for c in dec.coefs:
        positions |= (c != 0).reshape(-1, 64).any(axis=0)
        zz = c.reshape(-1, 64)[:, jr.NATURAL]      # the coefficients in zigzag order
        for row in zz:
          nz = np.flatnonzero(row[1:]) + 1
          zrl |= bool(len(nz)) and bool((np.diff(np.concatenate([[0], nz])) > 16).any())
  assert positions.all(), 'AC positions never coded: %s' % np.flatnonzero(~positions)
  assert zrl, 'no ZRL code in any case'
  const = jr.parse(ok['const_20x20_420'])
  assert all(not c.reshape(-1, 64)[:, 1:].any() for c in const.coefs)
  for name, (data, status) in refused.items():
    assert jr.status_of(data) == status, (name, jr.status_of(data), status)
    out[name + '/bytes'] = np.frombuffer(data, np.uint8)
    out[name + '/status'] = np.int32(status)
  np.savez_compressed(OUT, **out)
  print('%s: %d cases, %d refused, %d bytes' % (OUT, len(ok), len(refused), os.path.getsize(OUT)))


if __name__ == '__main__':
  main()
