"""GridMask on the device (efficientdet/aug/gridmask.py on edet_gridmask, automl_amd/gridmask.py): the host side and the numpy
restatement tests/gridmask_ref.py against the executed reference (tests/golden/reference_gridmask.npz, written by
tests/golden/make_golden_gridmask.py) on the CPU; the kernel, which evaluates the mask per pixel, against the restatement,
which materialises it, bit for bit on the GPU.

Oracle status: the fixture pins the reference's wiring -- mask(), the length formula, the stripe loop and the order of the
two scatter-and-transpose passes, crop, the occurrence branch, the final multiply.  The `rotate` the reference was executed
with is the restatement's own function, so the fixture says nothing about TensorFlow Addons: the coefficient formulas, the
rounding of the int32 bilinear blend and its truncation, float32 sin / cos and the random streams are pinned by nothing here."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from automl_amd import _lib, build, gridmask as gm
from tests import gpu_util as gu
from tests import gridmask_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(13, 11), (32, 40), (64, 48)]      # images of 143 pixels: byte by byte; two sizes on the 4-pixel path
BATCH = 5
CANARY = 64
_FIXTURE = []


def fixture():
  if not _FIXTURE:
    _FIXTURE.append(np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_gridmask.npz')))
  return _FIXTURE[0]


def draws_of(d, s1, s2, z1, z2):
  return (np.asarray(d, np.int32), np.asarray(s1, np.int32), np.asarray(s2, np.int32), np.asarray(z1, np.float32),
          np.asarray(z2, np.float32))


# ------------------------------------------------------------------------------------ CPU
def test_entry_point_struct_and_stubs_are_in_step():
  header = open(os.path.join(ROOT, 'include', 'edet_hip.h')).read()
  stubs = open(os.path.join(ROOT, 'automl_amd', 'csrc', 'plan_stubs.inc')).read()
  assert 'edet_gridmask' in _lib.SIGNATURES and 'int edet_gridmask(' in header and '"edet_gridmask"' in stubs
  assert 'gridmask.hip' in build.SOURCES and build.EXTRA_FLAGS['gridmask.hip'] == ['-ffp-contract=off']
  sys.path.insert(0, os.path.join(ROOT, 'scripts'))
  try:
    import gen_plan_stubs
  finally:
    sys.path.pop(0)
  assert gen_plan_stubs.generate() == stubs, 'plan_stubs.inc is stale: run scripts/gen_plan_stubs.py'
  # the header's struct, the ctypes mirror and the numpy rows: the same 48 bytes
  assert 'edet_gridmask_image_t' in header and 'float coef[6];' in header
  assert ctypes.sizeof(_lib.GridMaskImage) == gm.ARGS_BYTES == 48
  for name, _ in _lib.GridMaskImage._fields_:
    assert getattr(_lib.GridMaskImage, name).offset == gm.ARGS_DTYPE.fields[name][1], name
  assert [n for n, _ in _lib.GridMaskImage._fields_] == list(gm.ARGS_DTYPE.names)


@pytest.mark.parametrize('h,w,side,lo,hi,l_lo,l_hi', [
    (13, 11, 19, 3, 6, 2, 4),            # 1.5 * 13 = 19.5; min(6.5, 3.3), max; int(1.8 + .5), int(3.6 + .5)
    (32, 40, 60, 12, 16, 7, 10),         # 1.5 * 40; min(16, 12), max; int(7.2 + .5), int(9.6 + .5)
    (64, 48, 96, 14, 32, 8, 19),         # 1.5 * 64; min(32, 14.4), max; int(8.4 + .5), int(19.2 + .5)
    (640, 512, 960, 153, 320, 92, 192),  # 1.5 * 640; min(320, 153.6), max; int(91.8 + .5), int(192 + .5)
])
def test_args_against_hand_computed_values(h, w, side, lo, hi, l_lo, l_hi):
  assert gm.mask_side(h, w) == side and gm.block_range(h, w) == (lo, hi)
  assert gm.stripe_length(lo) == l_lo and gm.stripe_length(hi) == l_hi
  rows = gm.gridmask_args(draws_of([lo, hi], [0, hi], [lo, 0], [0.0, -1.0], [0.49, 0.5]), h, w)
  assert rows.dtype == gm.ARGS_DTYPE and rows.shape == (2,)
  assert rows['size'].tolist() == [side, side] and rows['d'].tolist() == [lo, hi] and rows['l'].tolist() == [l_lo, l_hi]
  assert rows['s1'].tolist() == [0, hi] and rows['s2'].tolist() == [lo, 0]
  assert rows['apply'].tolist() == [1, 0]                       # z2 < 0.5, strictly
  assert rows['coef'][0].tolist() == [1.0, -0.0, 0.0, 0.0, 1.0, 0.0]      # angle 0: the identity
  # -10 degrees: pi * (10 * -1) / 180 in float32, then the projective coefficients of an S x S image
  a = np.float32(np.float32(np.float32(np.pi) * np.float32(-10.0)) / np.float32(180))
  c, s, m = np.cos(a), np.sin(a), np.float32(side - 1)
  want = [c, -s, (m - (c * m - s * m)) / np.float32(2), s, c, (m - (s * m + c * m)) / np.float32(2)]
  assert rows['coef'][1].tolist() == [float(v) for v in want]
  draws = gm.gridmask_draws(gm.gridmask_rng(3), 64, h, w)
  assert all(v.shape == (64,) for v in draws)
  d, s1, s2, z1, z2 = draws
  assert d.min() >= lo and d.max() <= hi and s1.min() >= 0 and (s1 <= d).all() and s2.min() >= 0 and (s2 <= d).all()
  assert z1.dtype == z2.dtype == np.float32 and abs(float(z1.mean()) + 1.0) < 0.5 and abs(float(z2.mean())) < 0.5
  again = gm.gridmask_draws(gm.gridmask_rng(3), 64, h, w)
  assert all(np.array_equal(a_, b_) for a_, b_ in zip(draws, again))


def stripe(t, s, side, d, l):
  """The kernel's formula (include/edet_hip.h), in integers."""
  q = t - s
  return int(0 <= t < side and q >= 0 and q // d < side // d and q - (q // d) * d < l)


@pytest.mark.parametrize('side,d,l', [(12, 4, 2), (13, 4, 3), (10, 5, 4), (7, 3, 0)])
def test_stripe_formula_equals_the_literal_construction(side, d, l):
  """mask[r][c] = stripe(r; s1) | stripe(c; s2) for every s1, s2 in [0, d] -- the first start lands on rows -- including
  s = d with S % d == 0, where the last stripe is empty."""
  for s1 in range(d + 1):
    for s2 in range(d + 1):
      want = gr.build_mask(side, d, l, s1, s2)
      got = np.array([[stripe(r, s1, side, d, l) | stripe(c, s2, side, d, l) for c in range(side)] for r in range(side)],
                     np.int32)
      assert np.array_equal(got, want), (side, d, l, s1, s2)
  if side % d == 0:      # s1 = d: the last of the S // d row stripes starts at S and is empty (column 0 lies in no column stripe)
    assert int(gr.build_mask(side, d, l, d, d)[:, 0].sum()) == (side // d - 1) * l


def test_restatement_equals_executed_reference():
  """Every array of the fixture, bit for bit: three sizes, four draws each -- mask() from gridmask_args' S and l and the
  literal construction; the whole call (rotation by the restatement's own function, see the module docstring)."""
  z = fixture()
  applied = []
  for h, w in SIZES:
    key = '%dx%d' % (h, w)
    image, draws = z['image/' + key], z['draws/' + key]
    assert image.shape == (h, w, 3) and draws.shape == (4, 5)
    for k, (d, s1, s2, z1, z2) in enumerate(draws):
      rows = gm.gridmask_args(draws_of([d], [s1], [s2], [z1], [z2]), h, w)
      r = rows[0]
      mask = gr.build_mask(int(r['size']), int(r['d']), int(r['l']), int(r['s1']), int(r['s2']))
      assert np.array_equal(mask, z['mask/' + key][k].astype(np.int32)), (key, k)
      got = gr.gridmask_batch(image[None], rows)[0]
      assert got.dtype == np.uint8 and np.array_equal(got, z['out/' + key][k]), (key, k, int((got != z['out/' + key][k]).sum()))
      assert int(r['apply']) == int(z2 < 0.5)
      if not int(r['apply']):
        assert np.array_equal(got, image)
      applied.append(int(r['apply']))
  assert 0 < sum(applied) < len(applied)


def test_refusals():
  with pytest.raises(ValueError, match=r'fill=0 is not built.*gridmask\.py:99-101'):
    gm.GridMask(fill=0)
  with pytest.raises(ValueError, match=r'ratio=1 is not built.*gridmask\.py:82-84'):
    gm.gridmask(np.zeros((1, 32, 32, 3), np.uint8), None, ratio=1)
  with pytest.raises(ValueError, match=r'interpolation.*gridmask\.py:55'):
    gm.GridMask(interpolation='NEAREST')
  for h, w in ((1, 40), (40, 3), (2, 3)):      # int(min(H / 2, 0.3 W)) = 0: a zero gridblock
    with pytest.raises(ValueError, match=r'zero gridblock.*gridmask\.py:76-80'):
      gm.gridmask(np.zeros((2, h, w, 3), np.uint8), None)
    with pytest.raises(ValueError, match='zero gridblock'):
      gm.gridmask_draws(gm.gridmask_rng(0), 2, h, w)
  for bad in (np.zeros((2, 32, 32, 3), np.float32), np.zeros((32, 32, 3), np.uint8), np.zeros((2, 32, 32, 1), np.uint8),
              torch.zeros((2, 32, 32, 3), dtype=torch.int32)):
    with pytest.raises(ValueError, match='uint8'):
      gm.gridmask(bad, None)
  with pytest.raises(ValueError, match='five arrays'):
    gm.gridmask_args(draws_of([4, 4], [0], [0], [0.0], [0.0]), 13, 11)
  with pytest.raises(ValueError, match=r'draws are'):      # (checked before anything touches the device)
    gm.gridmask(np.zeros((2, 13, 11, 3), np.uint8), None, draws=draws_of([4], [0], [0], [0.0], [0.0]))


# ------------------------------------------------------------------------------------ GPU: the kernel
def _images(b, h, w, seed):
  return np.random.default_rng(seed).integers(1, 256, (b, h, w, 3)).astype(np.uint8)


def run_device(images, rows):
  """edet_gridmask on buffers with a canary behind each of them, twice: the two runs must agree in every byte."""
  n = images.size
  outs = []
  for _ in range(2):
    src = torch.full((n + CANARY,), 9, dtype=torch.uint8, device=gu.DEV)
    dst = torch.full((n + CANARY,), 7, dtype=torch.uint8, device=gu.DEV)
    args = torch.full((rows.shape[0] * gm.ARGS_BYTES + CANARY,), 5, dtype=torch.uint8, device=gu.DEV)
    src[:n] = torch.from_numpy(images.reshape(-1)).to(gu.DEV)
    args[:rows.shape[0] * gm.ARGS_BYTES] = gm.args_tensor(rows).reshape(-1).to(gu.DEV)
    gm.apply_mask(src[:n].view(images.shape), dst[:n].view(images.shape), args, gu.stream())
    torch.cuda.synchronize()
    assert bool((dst[n:] == 7).all()) and bool((src[n:] == 9).all()) and bool((args[rows.shape[0] * gm.ARGS_BYTES:] == 5).all())
    assert np.array_equal(src[:n].cpu().numpy().reshape(images.shape), images)      # never in place
    outs.append(dst[:n].cpu().numpy().reshape(images.shape))
  assert np.array_equal(outs[0], outs[1])
  return outs[0]


def check(images, rows, what):
  got = run_device(images, rows)
  want = gr.gridmask_batch(images, rows)
  assert np.array_equal(got, want), (what, images.shape, [int((got[i] != want[i]).sum()) for i in range(len(got))])
  return got


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', SIZES)
def test_kernel_equals_restatement(h, w):
  """Angle exactly 0 (the bare stripes), about +-10 and +-25 degrees; starts at 0 and at d; d at both ends of its range."""
  lo, hi = gm.block_range(h, w)
  mid = (lo + hi) // 2
  images = _images(BATCH, h, w, gu.seed_of('gridmask', h, w))
  on = [0.0] * BATCH
  # angle 0: the cropped mask is the stripes themselves
  rows = gm.gridmask_args(draws_of([lo, hi, mid, lo, hi], [0, hi, 1, lo, 0], [lo, 0, mid, 0, hi], [0.0] * 5, on), h, w)
  got = check(images, rows, 'angle 0')
  side = gm.mask_side(h, w)
  for i in range(BATCH):
    r = rows[i]
    bare = gr.crop(gr.build_mask(side, int(r['d']), int(r['l']), int(r['s1']), int(r['s2'])), h, w)
    assert np.array_equal(got[i], images[i] * bare[..., None].astype(np.uint8)), i
  assert 0 < int((got == 0).sum()) < got.size      # (the images hold no zero byte)
  # z1 = -+1, -+2.5: 10 and 25 degrees either way; then the same with d and the starts at their ends
  rows = gm.gridmask_args(draws_of([mid, mid, lo, hi, mid], [2, 0, lo, 0, mid], [0, 1, 0, hi, mid], [-1.0, 1.0, -2.5, 2.5, -0.37], on),
                          h, w)
  check(images, rows, 'rotated')
  rows = gm.gridmask_args(draws_of([lo, lo, hi, hi, lo], [0, lo, 0, hi, lo], [lo, 0, hi, 0, lo], [-1.0, 2.5, 1.0, -2.5, -1.7], on), h, w)
  check(images, rows, 'rotated, ends')
  # drawn as the trainer draws them
  rows = gm.gridmask_args(gm.gridmask_draws(gm.gridmask_rng(h * 100 + w), BATCH, h, w), h, w, prob=10.0)
  check(images, rows, 'drawn')


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', SIZES)
def test_every_apply_pattern_in_one_batch(h, w):
  """2^5 patterns of the occurrence bit, all-off = the copy and all-on included (the bit is uniform over a workgroup)."""
  lo, hi = gm.block_range(h, w)
  images = _images(BATCH, h, w, gu.seed_of('gridmask-apply', h, w))
  base = gm.gridmask_args(draws_of([lo, hi, lo, hi, lo], [1, 0, lo, 2, 0], [0, hi, 1, 0, lo], [-1.0, 0.0, 1.0, -2.5, 2.5], [0.0] * 5), h, w)
  masked = gr.gridmask_batch(images, base)
  assert all((masked[i] != images[i]).any() for i in range(BATCH))
  for pattern in range(1 << BATCH):
    rows = base.copy()
    bits = [(pattern >> i) & 1 for i in range(BATCH)]
    rows['apply'] = bits
    got = run_device(images, rows)
    for i in range(BATCH):
      assert np.array_equal(got[i], masked[i] if bits[i] else images[i]), (pattern, i)


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', SIZES)
def test_arguments_out_of_range_are_clamped(h, w):
  """Rows no host code would write, straight into device memory: d <= 0 (-> 1), l < 0 and l > d (-> [0, d]), starts outside
  [0, d], coefficients that are not finite or send every position far outside the mask (-> mask 0).  No fault, the canaries
  stay, and the result is the restatement's on the clamped values."""
  lo, hi = gm.block_range(h, w)
  images = _images(BATCH, h, w, gu.seed_of('gridmask-clamp', h, w))
  rows = gm.gridmask_args(draws_of([lo, hi, lo, hi, lo], [1, 0, lo, 2, 0], [0, hi, 1, 0, lo], [-1.0, 0.0, 1.0, -2.5, 2.5], [0.0] * 5), h, w)
  rows['d'] = [0, -5, lo, hi, 2 ** 31 - 1]
  rows['l'] = [1, 3, -3, 2 ** 31 - 1, 7]
  rows['s1'] = [-7, 0, 2 ** 31 - 1, -2 ** 31, 3]
  rows['s2'] = [5, -1, lo + 1, hi, -2]
  rows['apply'] = [1, -1, 2 ** 31 - 1, 1, 1]      # any non-zero value applies
  check(images, rows, 'integers')
  bad = rows.copy()
  bad['d'] = [lo, hi, lo, hi, lo]
  bad['l'] = [gm.stripe_length(int(v)) for v in bad['d']]
  bad['s1'] = 0
  bad['s2'] = 0
  bad['coef'][0] = [np.nan] * 6
  bad['coef'][1] = [np.inf, 0, 0, 0, 1, 0]
  bad['coef'][2] = [1, 0, 3e38, 0, 1, -3e38]
  bad['coef'][3] = [1e30, 1e30, 0, -1e30, 1e30, 0]
  bad['coef'][4] = [1, 0, 0, 0, 1, -np.inf]
  got = check(images, bad, 'coefficients')
  assert not got[0].any() and not got[2].any() and not got[4].any()
