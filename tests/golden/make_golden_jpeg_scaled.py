"""Generates tests/golden/jpeg_scaled_cases.npz with Pillow (libjpeg-turbo): the pixels Pillow decodes at reduced size --
``im.draft('RGB', (w // denom, h // denom))``, then ``convert('RGB')``: libjpeg's scale_denom 2, 4 and 8 -- from the streams of
tests/golden/jpeg_cases.npz and from two streams encoded here (a 16x16 4:2:2 file at quality 100 and a 64x64 4:2:0 file).  The
existing streams are named, not stored again; the 640x480 one is left out (the GPU test compares it with the restatement).

Per case `<name>/r<denom>` holds the pixels.  Pillow's draft mode never picks a scale larger than the image's smaller side
allows (1x1 at every ratio, 8x9 at ratio 8): for those cases the restatement tests/jpeg_scaled_ref.py is the definition, its
pixels are stored, and the case is listed in `restated`.  Everywhere else the script asserts that the restatement equals
Pillow byte for byte.

Run where Pillow is installed:  python tests/golden/make_golden_jpeg_scaled.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import jpeg_ref as jr   # noqa: E402
from tests import jpeg_scaled_ref as js   # noqa: E402
from tests.golden.make_golden_jpeg import encode, picture   # noqa: E402

SOURCE = os.path.join(HERE, 'jpeg_cases.npz')
OUT = os.path.join(HERE, 'jpeg_scaled_cases.npz')
RATIOS = (2, 4, 8)


def pillow_scaled(data, denom):
  """-> Pillow's pixels at scale 1 / denom, or None where draft() does not reach that scale."""
  im = Image.open(io.BytesIO(data))
  w, h = im.size
  if w // denom < 1 or h // denom < 1:
    return None
  im.draft('RGB', (w // denom, h // denom))
  if im.size != js.scaled_size(h, w, denom)[::-1]:
    return None
  return np.asarray(im.convert('RGB'))


def main():
  g = np.load(SOURCE)
  streams = {str(n): g[str(n) + '/bytes'].tobytes() for n in g['names'] if not str(n).startswith('big')}
  new = {'s16x16_422_q100': encode(picture(16, 16, 41), quality=100, subsampling=1),
         's64x64_420_q75': encode(picture(64, 64, 42), quality=75, subsampling=2)}
  out = {'names': np.array(sorted(streams)), 'new': np.array(sorted(new)), 'ratios': np.array(RATIOS, np.int32)}
  restated = []
  for name, data in new.items():
    assert np.array_equal(jr.decode(data), np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))), name
    out[name + '/bytes'] = np.frombuffer(data, np.uint8)
  streams.update(new)
  for name, data in sorted(streams.items()):
    fr = jr.info(data)
    for denom in RATIOS:
      mine = js.decode(data, denom)
      assert mine.shape == js.scaled_size(fr.height, fr.width, denom) + (3,), (name, denom)
      theirs = pillow_scaled(data, denom)
      if theirs is None:
        restated.append('%s/r%d' % (name, denom))
      else:
        assert np.array_equal(mine, theirs), (name, denom)      # the restatement equals Pillow, byte for byte
      out['%s/r%d' % (name, denom)] = mine
  assert all(n.startswith('s1x1') or (n.startswith('s8x9') and n.endswith('r8')) for n in restated), restated
  out['restated'] = np.array(sorted(restated))
  np.savez_compressed(OUT, **out)
  print('%s: %d streams x %d ratios, %d of them restated, %d bytes' % (OUT, len(streams), len(RATIOS), len(restated),
                                                                      os.path.getsize(OUT)))


if __name__ == '__main__':
  main()
