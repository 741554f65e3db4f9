"""edet_crop_resize_bicubic (csrc/crop_bicubic.hip): the known answers of its numpy restatement tests/bicubic_ref.py without a
device, and the kernel against that restatement bit for bit on one."""
import numpy as np
import pytest
import torch

from automl_amd import preprocess_legacy as pl, v2_preprocessing as vp
from tests import bicubic_ref as br

f32 = np.float32


# ------------------------------------------------------------------------------------ the restatement's known answers
def test_known_weights():
  assert br.weights_of(0).tolist() == [0.0, 1.0, 0.0, 0.0]
  assert br.weights_of(512).tolist() == [-0.09375, 0.59375, 0.59375, -0.09375]
  assert br.weights_of(256).tolist() == [-0.10546875, 0.87890625, 0.26171875, -0.03515625]


def test_table_symmetry_and_weight_sums():
  t = br.TABLE
  assert t.dtype == np.float32 and t.shape == (2050,)
  assert t[0] == 1.0 and t[1] == 0.0 and t[2048] == 0.0 and t[2049] == 0.0
  worst = 0.0
  for off in range(1025):
    w = br.weights_of(off)
    assert np.array_equal(w, br.weights_of(1024 - off)[::-1]), off      # the mirrored offset has the mirrored weights
    worst = max(worst, abs(float(w.astype(np.float64).sum()) - 1.0))
  print('largest |sum of the four weights - 1| over the 1025 offsets: %.3g' % worst)
  assert worst <= 3.4e-8
  # inside the table the inner weights fall and the outer ones are never positive
  assert (np.diff(t[0::2]) <= 0).all() and (t[1::2] <= 0).all()


def test_known_row():
  row = np.array([0, 100, 200, 250], np.float32).reshape(1, 4, 1)
  got = br.resize_bicubic(row, 1, 8)[0, :, 0]
  assert got.tolist() == [0, 40.625, 100, 154.6875, 200, 234.375, 250, 254.6875]


def test_identity_resize_and_overshoot():
  rng = np.random.default_rng(11)
  img = rng.integers(0, 256, (7, 5, 3)).astype(np.uint8)
  assert np.array_equal(br.resize_bicubic(img, 7, 5), img.astype(np.float32))
  up = br.resize_bicubic(img, 14, 10)
  assert np.array_equal(up[::2, ::2], img.astype(np.float32))      # offset 0 at every even position
  assert up.min() < 0 and up.max() > 255, (up.min(), up.max())
  u8 = br.convert(up, 'u8').numpy()
  assert u8.min() == 0 and u8.max() == 255
  f = br.convert(up, 'f32', pl.NORM).numpy()
  # the signed normalisation sees the overshoot: below what a 0 byte gives, above what a 255 byte gives
  assert f.min() < float(((f32(0) - pl.MEAN_RGB) / pl.STDDEV_RGB).min())
  assert f.max() > float(((f32(255) - pl.MEAN_RGB) / pl.STDDEV_RGB).max())


def test_python_keywords_are_checked_before_the_device():
  x = np.zeros((1, 4, 4, 3), np.uint8)
  rows = vp.whole_rows(1, 4, 4)
  with pytest.raises(ValueError, match='method'):
    vp.crop_resize(x, rows, 4, method='nearest')
  with pytest.raises(ValueError, match="norm needs method='bicubic'"):
    vp.crop_resize(x, rows, 4, torch.float32, norm=pl.NORM)
  with pytest.raises(ValueError, match='no std 0'):
    vp.crop_resize(x, rows, 4, torch.float32, method='bicubic', norm=([0, 0, 0], [1, 0, 1]))
  with pytest.raises(ValueError, match='no std 0'):
    vp.crop_resize(x, rows, 4, torch.float32, method='bicubic', norm=([0, 0], [1, 1]))
  assert pl.MEAN_RGB.dtype == np.float32 and pl.MEAN_RGB.tolist() == [f32(0.485 * 255), f32(0.456 * 255), f32(0.406 * 255)]
  assert pl.STDDEV_RGB.tolist() == [f32(0.229 * 255), f32(0.224 * 255), f32(0.225 * 255)]


# ------------------------------------------------------------------------------------ GPU: the kernel
CANVAS = (37, 53)
# (height, width, crop_y, crop_x, crop_h, crop_w, flip, reserved)
CASES = {
    # the four image sizes taken whole; the last one flipped
    'whole': [(1, 1, 0, 0, 1, 1, 0, 0), (2, 3, 0, 0, 2, 3, 1, 0), (5, 4, 0, 0, 5, 4, 0, 0), (37, 53, 0, 0, 37, 53, 1, 0)],
    # crops touching each edge: top-left, bottom-right = the canvas' (and, for image 3, the batch's) last pixel
    'edges': [(1, 1, 0, 0, 1, 1, 1, 0), (2, 3, 1, 1, 1, 2, 0, 0), (5, 4, 0, 1, 3, 3, 1, 0), (37, 53, 20, 30, 17, 23, 0, 0)],
    'edges2': [(1, 1, 0, 0, 1, 1, 0, 0), (2, 3, 0, 0, 2, 1, 1, 0), (5, 4, 2, 0, 3, 2, 0, 0), (37, 53, 0, 0, 9, 53, 1, 0)],
    # the batch's very last pixel alone, and a one-column / one-row crop
    'last': [(1, 1, 0, 0, 1, 1, 0, 0), (2, 3, 1, 2, 1, 1, 0, 0), (5, 4, 4, 0, 1, 4, 1, 0), (37, 53, 36, 52, 1, 1, 0, 0)],
    # hostile rows: negative, huge
    'hostile': [(-5, 99999, -3, 7, 1 << 30, -1, 7, 0), (2, 3, 5, 5, 5, 5, -1, 0), (0, 0, 0, 0, 0, 0, 0, 0),
                (1 << 30, 1 << 30, 1 << 30, -(1 << 30), 1 << 30, 1 << 30, 1, 0)],
}
SIZES = [(1, 1), (2, 3), (5, 4), (37, 53)]
OUTS = [(1, 1), (3, 5), (8, 8), (13, 7), (5, 260)]      # 8 x 8: the vector path; 13 x 7: the scalar one; 5 x 260: 2 blocks in x and y


def _canvas():
  """A batch of 4 on the 37 x 53 canvas; every byte outside an image is 255 and every byte inside is below 200: the
  restatement slices the crop out before it resizes, so a tap outside an image would show as a difference."""
  rng = np.random.default_rng(5)
  raw = np.full((4,) + CANVAS + (3,), 255, np.uint8)
  for k, (h, w) in enumerate(SIZES):
    raw[k, :h, :w] = rng.integers(0, 200, (h, w, 3))
  return raw


@pytest.fixture(scope='module')
def device_canvas():
  raw = _canvas()
  return raw, torch.from_numpy(raw).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_kernel_equals_the_restatement(device_canvas, case):
  raw, dev = device_canvas
  rows = np.array(CASES[case], np.int64).astype(np.int32)
  clamped = vp.clamp_rows(rows, *CANVAS)
  if case != 'hostile':
    assert np.array_equal(clamped[:, :6], rows[:, :6])
    assert np.array_equal(rows[:, :2], np.array(SIZES))      # the rows name the images' own sizes: nothing outside is read
  for oh, ow in OUTS:
    values = br.resized_crops(raw, rows, oh, ow)
    for kind in br.KINDS:
      for norm in (None, pl.NORM):
        want = br.convert(values, kind, None if norm is None else np.concatenate(norm))
        got = vp.crop_resize(dev, rows, (oh, ow), br.TORCH_DTYPE[kind], method='bicubic', norm=norm).cpu()
        assert got.dtype == want.dtype and tuple(got.shape) == (4, oh, ow, 3)
        assert torch.equal(got, want), (case, oh, ow, kind, norm is not None,
                                        (got.float() - want.float()).abs().max().item())


@pytest.mark.gpu
def test_identity_size_returns_the_input_and_the_bilinear_kernel_is_untouched(device_canvas):
  raw, dev = device_canvas
  rows = np.array([(h, w, 0, 0, h, w, 0, 0) for h, w in SIZES], np.int32)
  got = vp.crop_resize(dev[3:], rows[3:], CANVAS, torch.float32, method='bicubic').cpu().numpy()
  assert np.array_equal(got[0], raw[3].astype(np.float32))
  from tests import crop_ref as cr
  for kind in cr.KINDS:
    assert torch.equal(vp.crop_resize(dev, rows, (13, 8), cr.TORCH_DTYPE[kind]).cpu(), cr.crop_resize_ref(raw, rows, 13, 8, kind))


@pytest.mark.gpu
def test_randaug_apply_norm_is_the_normalising_copy(device_canvas):
  from automl_amd import autoaugment as aa
  raw, dev = device_canvas
  for x in (dev, dev[:, :13, :7].contiguous()):      # the four-pixel path and the byte path
    for kind in br.KINDS:
      out = torch.empty(x.shape, dtype=br.TORCH_DTYPE[kind], device='cuda')
      aa.apply_layers(x, out, None, None, None, None, None, torch.cuda.current_stream().cuda_stream, norm=pl.NORM)
      assert torch.equal(out.cpu(), br.normalize_u8(x.cpu().numpy(), kind, np.concatenate(pl.NORM))), kind
