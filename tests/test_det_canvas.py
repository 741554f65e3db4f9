"""The detector's input kernels on a CANVAS batch (the six edet_*_canvas entry points of include/edet_hip.h and the `sizes=`
argument of gridmask.py, det_autoaugment.py, preprocess.py): image i, the top-left sizes[i] of its canvas slot, comes out bit
for bit as the dense entry point treats that image alone, and as the numpy restatements (tests/gridmask_ref.py,
tests/det_autoaug_ref.py, tests/randaug_ref.py) compute it at that image's size.

Two canvases of four images each: 24 x 28 (a full canvas, a narrower and shorter image, a width that is a multiple of 4 in
a canvas width that is one: the four-pixel path) and 23 x 27 (a row pitch of 81 bytes: no row starts on a dword).  The
padding around the images is random NON-ZERO bytes, and every case runs a second time with other padding bytes and must give
the same result: nothing reads outside the image.  Destinations are filled with a sentinel first: nothing outside the
rectangle is written.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

from automl_amd import _lib, autoaugment as v2aa, det_autoaugment as daa, det_input, gridmask as gm, preprocess, utils
from automl_amd._lib import call, ptr
from tests import det_autoaug_ref as dr, det_eval_ref, gridmask_ref, randaug_ref as rr

CANVASES = {
    '24x28': ((24, 28), [(24, 28), (13, 17), (12, 20), (7, 9)]),
    '23x27': ((23, 27), [(23, 27), (9, 16), (5, 26), (23, 4)]),
}
B, M = 4, 8
COUNTS = np.asarray([5, 0, M, 3], np.int32)      # one image without a box, one with every row
SENTINEL = 0xA5
PADDINGS = (1, 2)
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
OUT = (32, 40)      # the output image of the resize: more than one 4 x 64 tile in y, less than one in x


def canvas_batch(name, padding):
  """uint8 [B, ch, cw, 3]: the images' own pixels depend on the canvas only, the padding on `padding` and is never 0."""
  (ch, cw), sizes = CANVASES[name]
  raw = np.random.default_rng(1000 + padding).integers(1, 256, (B, ch, cw, 3)).astype(np.uint8)
  rng = np.random.default_rng(ch * 100 + cw)
  for i, (h, w) in enumerate(sizes):
    raw[i, :h, :w] = rng.integers(0, 256, (h, w, 3))
  raw[3, :sizes[3][0], :sizes[3][1], 0] //= 4      # a narrow histogram in one channel: AutoContrast has work to do
  return raw, np.asarray(sizes, np.int32)


def box_rows(name):
  rng = np.random.default_rng(7 + CANVASES[name][0][0])
  y0, x0 = rng.uniform(0.0, 0.6, (B, M)), rng.uniform(0.0, 0.6, (B, M))
  boxes = np.stack([y0, x0, y0 + rng.uniform(0.1, 0.4, (B, M)), x0 + rng.uniform(0.1, 0.4, (B, M))], -1).astype(np.float32)
  for i in range(B):
    boxes[i, COUNTS[i]:] = -7.5 - i      # padded rows: no operation may touch them
  classes = rng.integers(1, 91, (B, M)).astype(np.float32)
  return boxes, classes


_KEEP = []


def dev(a):
  """A host array on the device, kept alive until the test ends: the launches that read it are asynchronous, and a temporary
  handed to a call as ptr(dev(...)) would give its memory to the next one before the kernel has run."""
  _KEEP.append(torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0'))
  return _KEEP[-1]


@pytest.fixture(autouse=True)
def release_device_arrays():
  yield
  if _KEEP:
    torch.cuda.synchronize()
    _KEEP.clear()


def stream():
  return torch.cuda.current_stream().cuda_stream


def bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def sentinel_like(shape, dtype):
  """A device tensor every byte of which is the sentinel."""
  n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
  return torch.full((n,), SENTINEL, dtype=torch.uint8, device='cuda:0').view(dtype).view(*shape)


def as_bytes(t):
  return t.contiguous().view(torch.uint8)


def check_rectangles(got, want_per_image, sizes, what):
  """got [B, ch, cw, 3] (any dtype, a sentinel where nothing was written) against the dense results [1, h, w, 3] per image."""
  got = got.cpu()
  for i, (h, w) in enumerate(sizes):
    assert torch.equal(as_bytes(got[i, :h, :w]), as_bytes(want_per_image[i].cpu()[0])), (what, 'image', i)
    outside = torch.ones(got.shape[1:3], dtype=torch.bool)
    outside[:h, :w] = False
    assert bool((as_bytes(got[i][outside]) == SENTINEL).all()), (what, 'written outside image', i)


def crop(raw, sizes, i):
  return np.ascontiguousarray(raw[i:i + 1, :sizes[i][0], :sizes[i][1]])


# ------------------------------------------------------------------------------------ the six launches, canvas and dense
def gridmask_rows(sizes):
  d = gm.gridmask_draws(np.random.default_rng(3), B, sizes[:, 0], sizes[:, 1])
  d[4][:] = [-1.0, 0.2, 2.0, -0.5]      # the occurrence draw: applied, applied, copied, applied (prob 0.5)
  return gm.gridmask_args(d, sizes[:, 0], sizes[:, 1])


def run_gridmask(raw, sizes, rows):
  src, out = dev(raw), sentinel_like(raw.shape, torch.uint8)
  gm.apply_mask(src, out, dev(gm.args_tensor(rows).numpy()), stream(), dev(sizes))
  return out


def dense_gridmask(raw, sizes, rows):
  res = []
  for i in range(B):
    src = dev(crop(raw, sizes, i))
    res.append(gm.apply_mask(src, torch.empty_like(src), dev(gm.args_tensor(rows[i:i + 1]).numpy()), stream()))
  return res


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CANVASES))
def test_gridmask_canvas_equals_dense_and_restatement(name):
  results = []
  for padding in PADDINGS:
    raw, sizes = canvas_batch(name, padding)
    rows = gridmask_rows(sizes)
    got = run_gridmask(raw, sizes, rows)
    check_rectangles(got, dense_gridmask(raw, sizes, rows), sizes, ('gridmask', name, padding))
    results.append(got.cpu())
  assert torch.equal(results[0], results[1]), 'the padding bytes changed the result'
  got = results[0].numpy()
  changed = 0
  for i, (h, w) in enumerate(sizes):
    want = gridmask_ref.gridmask_batch(crop(raw, sizes, i), rows[i:i + 1])
    assert np.array_equal(got[i, :h, :w], want[0]), ('restatement', name, i)
    changed += int((want[0] != raw[i, :h, :w]).sum())
  assert changed > 0 and np.array_equal(got[2, :sizes[2][0], :sizes[2][1]], raw[2, :sizes[2][0], :sizes[2][1]])


# ---- edet_randaug_apply_canvas: every operation id, every output dtype
def apply_args(op, sizes):
  """ops / iargs / fargs of one layer where every image gets operation `op`; arguments that depend on the image's own size
  (Rotate's centre, Cutout's clamps) are made per image or left to the kernel's clamp."""
  ops = np.full(B, op, np.int32)
  iargs, fargs = np.zeros((B, 4), np.int32), np.zeros((B, 8), np.float32)
  fargs[:, 6] = 1.0
  for i, (h, w) in enumerate(sizes):
    if op == 3:
      fargs[i, :6] = v2aa.rotate_coefficients(20.0 - 10.0 * i, int(h), int(w))
    elif op == 4:
      iargs[i, 0] = 3 + i
    elif op == 5:
      iargs[i, 0] = 100 + 20 * i
    elif op == 15:
      iargs[i, :2] = [40 + 10 * i, 128]
    elif op in (6, 7, 8, 9):
      fargs[i, 6] = 0.4 + 0.5 * i
    elif op == 10:
      fargs[i, :6] = [1, 0.3 - 0.2 * i, 0, 0, 1, 0]
    elif op == 11:
      fargs[i, :6] = [1, 0, 0, -0.3 + 0.2 * i, 1, 0]
    elif op == 12:
      fargs[i, :6] = [1, 0, 3 - 2 * i, 0, 1, 0]
    elif op == 13:
      fargs[i, :6] = [1, 0, 0, 0, 1, -2 + 2 * i]
    elif op == 14:
      iargs[i] = [2, 1, 1000, 1000] if i % 2 else [1, 2, max(int(h) - 2, 2), max(int(w) - 1, 3)]      # odd: the kernel's clamp
  return ops, iargs, fargs


TORCH_DTYPE = {'u8': (torch.uint8, _lib.EDET_U8), 'f32': (torch.float32, _lib.EDET_F32), 'bf16': (torch.bfloat16, _lib.EDET_BF16)}


def run_stats(src, sizes_dev, ops_dev):
  b, ch, cw = src.shape[:3]
  luts = torch.full((b, 3, 256), SENTINEL, dtype=torch.uint8, device='cuda:0')
  call('edet_randaug_stats_canvas', ptr(src), b, ch, cw, ptr(sizes_dev), ptr(ops_dev), ptr(luts), stream())
  return luts


def dense_stats(src1, op):
  luts = torch.full((1, 3, 256), SENTINEL, dtype=torch.uint8, device='cuda:0')
  call('edet_randaug_stats', ptr(src1), 1, int(src1.shape[1]), int(src1.shape[2]), ptr(dev(np.asarray([op], np.int32))), ptr(luts),
       stream())
  return luts


def run_apply(raw, sizes, op, dtype):
  tdt, code = TORCH_DTYPE[dtype]
  ops, iargs, fargs = apply_args(op, sizes)
  src, sizes_dev, ops_dev, ia, fa = dev(raw), dev(sizes), dev(ops), dev(iargs), dev(fargs)
  luts = run_stats(src, sizes_dev, ops_dev)
  out = sentinel_like(raw.shape, tdt)
  b, ch, cw = raw.shape[:3]
  call('edet_randaug_apply_canvas', ptr(src), ptr(out), b, ch, cw, ptr(sizes_dev), ptr(ops_dev), ptr(ia), ptr(fa), ptr(luts), code,
       stream())
  want = []
  for i in range(B):
    s1 = dev(crop(raw, sizes, i))
    l1 = dense_stats(s1, op)
    if op in (0, 1):
      assert torch.equal(l1[0], luts[i]), ('table', op, i)
    o1 = torch.empty(s1.shape, dtype=tdt, device='cuda:0')
    call('edet_randaug_apply', ptr(s1), ptr(o1), 1, int(s1.shape[1]), int(s1.shape[2]), ptr(dev(ops[i:i + 1])),
         ptr(dev(iargs[i:i + 1])), ptr(dev(fargs[i:i + 1])), ptr(l1), code, stream())
    want.append(o1)
  return out, want


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['u8', 'f32', 'bf16'])
@pytest.mark.parametrize('op', list(range(17)))
def test_randaug_apply_canvas_equals_dense(op, dtype):
  for name in sorted(CANVASES):
    results = []
    for padding in PADDINGS:
      raw, sizes = canvas_batch(name, padding)
      out, want = run_apply(raw, sizes, op, dtype)
      torch.cuda.synchronize()
      check_rectangles(out, want, sizes, ('apply', name, op, dtype, padding))
      results.append(out.cpu())
    assert torch.equal(results[0].view(torch.uint8), results[1].view(torch.uint8)), 'the padding bytes changed the result'
    if op != 16 and dtype == 'u8':      # (the operation did something)
      assert any(not np.array_equal(results[0][i, :h, :w].numpy(), raw[i, :h, :w]) for i, (h, w) in enumerate(sizes)), (name, op)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CANVASES))
def test_statistics_equal_the_restatement_on_the_cropped_image(name):
  """Equalize / AutoContrast through edet_randaug_stats_canvas and the detector's Contrast through
  edet_autoaug_contrast_lut_canvas (the true mean grey level of the image's own pixels), each then applied."""
  raw, sizes = canvas_batch(name, PADDINGS[0])
  for op, ref in ((0, rr.autocontrast), (1, rr.equalize)):
    out, _ = run_apply(raw, sizes, op, 'u8')
    got = out.cpu().numpy()
    for i, (h, w) in enumerate(sizes):
      assert np.array_equal(got[i, :h, :w], ref(raw[i, :h, :w])), (name, op, i)
  factor = 1.45
  for padding in PADDINGS:
    raw, sizes = canvas_batch(name, padding)
    src, sizes_dev = dev(raw), dev(sizes)
    policy = dev(np.asarray([6, 6, 9, 6], np.int32))      # image 2: not Contrast, its table and id stay
    ops = dev(np.full(B, v2aa.IDENTITY, np.int32))
    fargs = np.zeros((B, 8), np.float32)
    fargs[:, 6] = factor
    luts = torch.full((B, 3, 256), SENTINEL, dtype=torch.uint8, device='cuda:0')
    b, ch, cw = raw.shape[:3]
    call('edet_autoaug_contrast_lut_canvas', ptr(src), b, ch, cw, ptr(sizes_dev), ptr(policy), ptr(ops), ptr(dev(fargs)),
         ptr(luts), stream())
    assert ops.cpu().tolist() == [1, 1, v2aa.IDENTITY, 1] and bool((luts[2] == SENTINEL).all())
    out = sentinel_like(raw.shape, torch.uint8)
    call('edet_randaug_apply_canvas', ptr(src), ptr(out), b, ch, cw, ptr(sizes_dev), ptr(ops), ptr(dev(np.zeros((B, 4), np.int32))),
         ptr(dev(fargs)), ptr(luts), _lib.EDET_U8, stream())
    got = out.cpu().numpy()
    for i, (h, w) in enumerate(sizes):
      want = raw[i, :h, :w] if i == 2 else dr.contrast(raw[i, :h, :w], factor)
      assert np.array_equal(got[i, :h, :w], want), (name, 'contrast', i, padding)
      # against the dense entry point too: the table and the id
      s1 = dev(crop(raw, sizes, i))
      o1, l1 = dev(np.full(1, v2aa.IDENTITY, np.int32)), torch.full((1, 3, 256), SENTINEL, dtype=torch.uint8, device='cuda:0')
      call('edet_autoaug_contrast_lut', ptr(s1), 1, int(h), int(w), ptr(dev(policy[i:i + 1].cpu().numpy())), ptr(o1), ptr(dev(fargs[i:i + 1])),
           ptr(l1), stream())
      assert torch.equal(l1[0], luts[i]) and int(o1[0]) == int(ops[i]), (name, 'contrast table', i)


# ---- edet_autoaug_boxes_canvas
BOX_POLICIES = {10: 'BBox_Cutout', 11: 'Rotate_BBox', 12: 'TranslateX_BBox', 13: 'TranslateY_BBox', 14: 'ShearX_BBox',
                15: 'ShearY_BBox', 16: None}


def box_args(policy, sizes):
  rng = np.random.default_rng(policy)
  iargs, fargs, dargs = np.full((B, 4), -3, np.int32), np.zeros((B, 8), np.float32), np.zeros((B, 4), np.float64)
  for i, (h, w) in enumerate(sizes):
    sign = 1.0 if i % 2 else -1.0
    if policy == 11:
      fargs[i, :6] = v2aa.rotate_coefficients(sign * 24.0, int(h), int(w))
    elif policy == 12:
      fargs[i, :6] = [1, 0, sign * 4.0, 0, 1, 0]
    elif policy == 13:
      fargs[i, :6] = [1, 0, 0, 0, 1, sign * 3.0]
    elif policy == 14:
      fargs[i, :6] = [1, sign * 0.24, 0, 0, 1, 0]
    elif policy == 15:
      fargs[i, :6] = [1, 0, 0, sign * 0.24, 1, 0]
    dargs[i] = [0.6, rng.random(), rng.random(), rng.random()]
  return iargs, fargs, dargs


@pytest.mark.gpu
@pytest.mark.parametrize('policy', sorted(BOX_POLICIES))
def test_autoaug_boxes_canvas_equals_dense_and_restatement(policy):
  for name in sorted(CANVASES):
    sizes = np.asarray(CANVASES[name][1], np.int32)
    boxes, _ = box_rows(name)
    iargs, fargs, dargs = box_args(policy, sizes)
    pol = np.full(B, policy, np.int32)
    got_b, got_i = torch.full((B, M, 4), -99.0, device='cuda:0'), dev(iargs)
    call('edet_autoaug_boxes_canvas', ptr(dev(boxes)), ptr(got_b), ptr(dev(COUNTS)), B, M, ptr(dev(sizes)), ptr(dev(pol)),
         ptr(got_i), ptr(dev(fargs)), ptr(dev(dargs)), stream())
    for i, (h, w) in enumerate(sizes):
      want_b, want_i = torch.full((1, M, 4), -99.0, device='cuda:0'), dev(iargs[i:i + 1])
      call('edet_autoaug_boxes', ptr(dev(boxes[i:i + 1])), ptr(want_b), ptr(dev(COUNTS[i:i + 1])), 1, M, int(h), int(w),
           ptr(dev(pol[i:i + 1])), ptr(want_i), ptr(dev(fargs[i:i + 1])), ptr(dev(dargs[i:i + 1])), stream())
      assert np.array_equal(bits(got_b[i].cpu().numpy()), bits(want_b[0].cpu().numpy())), (name, policy, 'boxes', i)
      assert torch.equal(got_i[i], want_i[0]), (name, policy, 'iargs', i)
      # the restatement at the image's own size
      n = int(COUNTS[i])
      sign = 1.0 if i % 2 else -1.0
      valid = boxes[i, :n]
      if policy == 10:
        rect = dr.bbox_cutout_rect(valid, int(h), int(w), *dargs[i])
        assert got_i[i].cpu().tolist() == list(rect), (name, 'BBox_Cutout rectangle', i, rect)
        want = valid
      elif policy == 11:
        want = np.asarray([dr.rotate_bbox(bx, int(h), int(w), sign * 24.0) for bx in valid], np.float32).reshape(-1, 4)
      elif policy in (12, 13):
        want = np.asarray([dr.shift_bbox(bx, int(h), int(w), sign * (4.0 if policy == 12 else 3.0), policy == 12) for bx in valid],
                          np.float32).reshape(-1, 4)
      elif policy in (14, 15):
        want = np.asarray([dr.shear_bbox(bx, int(h), int(w), sign * 0.24, policy == 14) for bx in valid],
                          np.float32).reshape(-1, 4)
      else:
        want = valid
      assert np.array_equal(bits(got_b[i, :n].cpu().numpy()), bits(want)), (name, policy, 'restatement', i)
      assert np.array_equal(got_b[i, n:].cpu().numpy(), boxes[i, n:]), (name, policy, 'padded rows', i)


# ---- edet_preprocess_train_canvas
def prep_rows(sizes):
  u = np.random.default_rng(11).random((B, 3)).astype(np.float32)
  u[1] = [0.99, 0.9, 0.9]      # scaled up and cropped away from the corner
  per = np.zeros((B, 5), np.int32)
  per[:, 0] = [0, 1, 1, 0]
  for i, (h, w) in enumerate(sizes):
    _, per[i, 1:3], per[i, 3:5] = preprocess.training_scale_factors(u[i], 0.1, 2.0, OUT, OUT, int(h), int(w))
  return per


def preprocess_call(fn, src, extra, per, boxes, classes, counts, tdt):
  b = int(src.shape[0])
  out = torch.full((b,) + OUT + (3,), float('nan'), dtype=tdt, device='cuda:0')
  bo, co, cn = torch.full((b, M, 4), -99.0, device='cuda:0'), torch.full((b, M), -99.0, device='cuda:0'), dev(np.full(b, -9, np.int32))
  mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
  call(fn, ptr(src), 0, b, int(src.shape[1]), int(src.shape[2]), *extra, OUT[0], OUT[1], mean, std, ptr(dev(per)), ptr(out),
       ptr(dev(boxes)), ptr(dev(classes)), ptr(dev(counts)), M, ptr(bo), ptr(co), ptr(cn),
       _lib.EDET_BF16 if tdt == torch.bfloat16 else _lib.EDET_F32, stream())
  torch.cuda.synchronize()
  return out.cpu(), bo.cpu(), co.cpu(), cn.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('tdt', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', sorted(CANVASES))
def test_preprocess_train_canvas_equals_dense(name, tdt):
  boxes, classes = box_rows(name)
  boxes = np.where(boxes < 0, np.float32(0), boxes)      # (valid coordinates in the padded rows too: they are not read)
  results = []
  for padding in PADDINGS:
    raw, sizes = canvas_batch(name, padding)
    per = prep_rows(sizes)
    sizes_dev = dev(sizes)
    got = preprocess_call('edet_preprocess_train_canvas', dev(raw), (ptr(sizes_dev),), per, boxes, classes, COUNTS, tdt)
    for i in range(B):
      want = preprocess_call('edet_preprocess_train', dev(crop(raw, sizes, i)), (), per[i:i + 1], boxes[i:i + 1], classes[i:i + 1],
                             COUNTS[i:i + 1], tdt)
      for k, what in enumerate(('image', 'boxes', 'classes', 'counts')):
        assert torch.equal(as_bytes(got[k][i:i + 1]), as_bytes(want[k][0:1])), (name, padding, what, i)
    results.append(got)
  for a, b in zip(*results):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), 'the padding bytes changed the result'
  assert not bool(torch.isnan(results[0][0].float()).any()) and int(results[0][3].sum()) > 0


# ------------------------------------------------------------------------------------ the public pieces with sizes=
@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CANVASES))
def test_distort_with_sizes_equals_the_restatement_per_image(name):
  """distort_image_with_autoaugment('v2' / 'v3') and ..._randaugment with sizes= against det_autoaug_ref.walk on the cropped
  image, boxes included: every box-aware operation at the image's own height and width."""
  boxes, _ = box_rows(name)
  rng = np.random.default_rng(5)
  for policy in ('v2', 'v3', 'randaug'):
    for rep in range(4):
      d = daa.autoaug_draws(rng, B, policy, num_layers=2)
      results = []
      for padding in PADDINGS:
        raw, sizes = canvas_batch(name, padding)
        if policy == 'randaug':
          got = daa.distort_image_with_randaugment(raw, boxes, COUNTS, 2, 15, draws=d, sizes=sizes)
        else:
          d = d._replace(index=((np.arange(B) + rep * B) % len(dr.POLICIES[policy])).astype(np.int32))
          got = daa.distort_image_with_autoaugment(raw, boxes, COUNTS, policy, draws=d, sizes=torch.from_numpy(sizes))
        results.append((got[0].cpu().numpy(), got[1].cpu().numpy()))
      assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(bits(results[0][1]), bits(results[1][1]))
      gi, gb = results[0]
      for i, (h, w) in enumerate(sizes):
        n = int(COUNTS[i])
        col = lambda a: None if a is None else np.asarray(a)[:, i]      # noqa: E731
        idx = np.asarray(d.index)[:, i] if policy == 'randaug' else np.asarray(d.index)[i]
        wi, wb = dr.walk(raw[i, :h, :w], boxes[i, :n], policy, idx, col(d.apply), col(d.sign), col(d.cy_u), col(d.cx_u),
                         col(d.box_u), 15 if policy == 'randaug' else None)
        assert np.array_equal(gi[i, :h, :w], wi), (name, policy, rep, 'image', i)
        assert np.array_equal(bits(gb[i, :n]), bits(np.asarray(wb, np.float32))), (name, policy, rep, 'boxes', i)
        assert np.array_equal(gb[i, n:], boxes[i, n:]), (name, policy, rep, 'padded rows', i)


# ------------------------------------------------------------------------------------ garbage sizes in device memory
@pytest.mark.gpu
def test_garbage_sizes_are_clamped_into_the_slot():
  """sizes rows (0, 0), (-5, 10^6), (canvas_h + 1, canvas_w + 1) in DEVICE memory (the host checks are bypassed by calling the
  entry points directly): every kernel that indexes a slot clamps them into [1, canvas] -- (1, 1), (1, canvas_w), the whole
  canvas -- as reading the kernels shows (clampi(sizes[2 img], 1, ch) / (..., 1, cw) in front of every use), so each launch
  returns 0, gives what the clamped sizes give, and the guard bands around source and destination, all one allocation, are
  untouched.  edet_autoaug_boxes_canvas has no canvas and indexes nothing by a size: it clamps into [1, 2^24 - 1], what the
  dense entry point accepts."""
  (ch, cw), _ = CANVASES['23x27']
  b, guard = 3, 4096
  garbage = np.asarray([[0, 0], [-5, 10 ** 6], [ch + 1, cw + 1]], np.int32)
  clamped = np.asarray([[1, 1], [1, cw], [ch, cw]], np.int32)
  clamped_for_boxes = np.asarray([[1, 1], [1, 10 ** 6], [ch + 1, cw + 1]], np.int32)
  raw = canvas_batch('23x27', 1)[0][:b]
  n = raw.size
  boxes, classes = box_rows('23x27')
  boxes, classes, counts = np.where(boxes[:b] < 0, np.float32(0), boxes[:b]), classes[:b], COUNTS[:b]

  def launches(sizes, box_sizes):
    """One allocation [guard | src | guard | dst | guard]; -> everything the six launches wrote, and the allocation."""
    arena = torch.full((3 * guard + 2 * n,), SENTINEL, dtype=torch.uint8, device='cuda:0')
    src, dst = arena[guard:guard + n].view(b, ch, cw, 3), arena[2 * guard + n:2 * guard + 2 * n].view(b, ch, cw, 3)
    src.copy_(dev(raw))
    sizes_dev, st = dev(sizes), stream()
    res = []
    rows = gm.gridmask_args(gm.gridmask_draws(np.random.default_rng(3), b, ch, cw), ch, cw, prob=1e9)
    call('edet_gridmask_canvas', ptr(src), ptr(dst), b, ch, cw, ptr(sizes_dev), ptr(dev(gm.args_tensor(rows).numpy())), st)
    res.append(dst.cpu().clone())
    for op in (1, 3, 9, 14):
      ops, iargs, fargs = apply_args(op, clamped)
      ops_dev = dev(ops[:b])
      luts = torch.zeros((b, 3, 256), dtype=torch.uint8, device='cuda:0')
      call('edet_randaug_stats_canvas', ptr(src), b, ch, cw, ptr(sizes_dev), ptr(ops_dev), ptr(luts), st)
      call('edet_randaug_apply_canvas', ptr(src), ptr(dst), b, ch, cw, ptr(sizes_dev), ptr(ops_dev), ptr(dev(iargs[:b])),
           ptr(dev(fargs[:b])), ptr(luts), _lib.EDET_U8, st)
      res += [luts.cpu(), dst.cpu().clone()]
    policy, ops_dev = dev(np.full(b, 6, np.int32)), dev(np.full(b, 16, np.int32))
    fargs = np.zeros((b, 8), np.float32)
    fargs[:, 6] = 0.5
    luts = torch.zeros((b, 3, 256), dtype=torch.uint8, device='cuda:0')
    call('edet_autoaug_contrast_lut_canvas', ptr(src), b, ch, cw, ptr(sizes_dev), ptr(policy), ptr(ops_dev), ptr(dev(fargs)),
         ptr(luts), st)
    res += [luts.cpu(), ops_dev.cpu()]
    for pol in (10, 11, 12):
      iargs, fa, dargs = box_args(pol, clamped)
      bo, ia = torch.zeros((b, M, 4), device='cuda:0'), dev(iargs[:b])
      call('edet_autoaug_boxes_canvas', ptr(dev(boxes)), ptr(bo), ptr(dev(counts)), b, M, ptr(dev(box_sizes)), ptr(dev(np.full(b, pol, np.int32))),
           ptr(ia), ptr(dev(fa[:b])), ptr(dev(dargs[:b])), st)
      res += [bo.cpu(), ia.cpu()]
    per = prep_rows(np.concatenate([clamped, clamped[:1]]))[:b]
    res += list(preprocess_call('edet_preprocess_train_canvas', src, (ptr(sizes_dev),), per, boxes, classes, counts, torch.float32))
    torch.cuda.synchronize()
    return res, arena.cpu()

  got, arena = launches(garbage, garbage)      # (_lib.call raises if an entry point does not return 0)
  want, _ = launches(clamped, clamped_for_boxes)
  for k, (a, c) in enumerate(zip(got, want)):
    assert torch.equal(a.view(torch.uint8), c.view(torch.uint8)), ('result', k)
  for lo in (0, guard + n, 2 * guard + 2 * n):
    assert bool((arena[lo:lo + guard] == SENTINEL).all()), ('guard band at', lo)
  assert np.array_equal(arena[guard:guard + n].numpy().reshape(raw.shape), raw)      # the source was only read
  # image 1 is clamped to one row of the full width: the rows below it in its dst slot hold the sentinel
  last = got[8]      # the destination after the last edet_randaug_apply_canvas
  assert last.shape == raw.shape
  assert bool((last[1, 1:] == SENTINEL).all()) and bool((last[0].reshape(-1)[3:] == SENTINEL).all())


# ------------------------------------------------------------------------------------ CPU: the host side
def test_args_with_per_image_sizes_equal_the_batch_of_one_calls():
  for name in sorted(CANVASES):
    sizes = np.asarray(CANVASES[name][1], np.int32)
    hs, ws = sizes[:, 0], sizes[:, 1]
    rng = np.random.default_rng(9)
    g = gm.gridmask_draws(rng, B, hs, ws)
    rows = gm.gridmask_args(g, hs, ws)
    for i in range(B):
      lo, hi = gm.block_range(int(hs[i]), int(ws[i]))
      assert lo <= int(g[0][i]) <= hi
      one = gm.gridmask_args([v[i:i + 1] for v in g], int(hs[i]), int(ws[i]))
      assert one.tobytes() == rows[i:i + 1].tobytes(), (name, 'gridmask row', i)
    for policy in ('v2', 'v3', 'randaug'):
      for _ in range(6):
        d = daa.autoaug_draws(rng, B, policy, num_layers=2)
        args = daa.autoaug_args(d, policy, hs, ws, magnitude=15)
        for i in range(B):
          di = daa.AutoAugDraws(*[None if a is None else (np.asarray(a)[i:i + 1] if np.asarray(a).ndim == 1 else np.asarray(a)[:, i:i + 1])
                                  for a in d])
          one = daa.autoaug_args(di, policy, int(hs[i]), int(ws[i]), magnitude=15)
          for field, a, o in zip(daa.AutoAugArgs._fields, args, one):
            assert np.array_equal(bits(a[:, i:i + 1]), bits(o)), (name, policy, field, i)


def test_eval_rows_and_scales_equal_the_restatement_per_image():
  for name in sorted(CANVASES):
    sizes = np.asarray(CANVASES[name][1], np.int32)
    for output_size in ((128, 128), (64, 96)):
      per, scales = det_input.eval_rows(output_size, sizes)
      assert per.dtype == np.int32 and per.shape == (B, 5) and scales.dtype == np.float32
      for i, (h, w) in enumerate(sizes):
        scale, sh, sw = det_eval_ref.scale_factors_to_output_size(int(h), int(w), output_size)
        assert per[i].tolist() == [0, sh, sw, 0, 0], (name, i)
        assert bits(scales[i:i + 1])[0] == bits(np.asarray([np.float32(1.0) / scale], np.float32))[0], (name, i)
    assert len(set(scales.tolist())) > 1      # (the scales do differ per image)


def state_of(rng):
  return repr(rng.bit_generator.state)


def test_size_checks_name_the_image_and_leave_the_generator_alone():
  (ch, cw), sizes = CANVASES['24x28']
  good = np.asarray(sizes, np.int32)
  raw = np.zeros((B, ch, cw, 3), np.uint8)
  boxes, _ = box_rows('24x28')
  for bad_row, pattern in (((0, 5), r'image 2: size 0 x 5'), ((ch + 1, 5), r'image 2: size 25 x 5'), ((5, cw + 1), r'image 2')):
    bad = good.copy()
    bad[2] = bad_row
    with pytest.raises(ValueError, match=pattern):
      utils.canvas_sizes(bad, B, ch, cw)
    rng = np.random.default_rng(4)
    before = state_of(rng)
    with pytest.raises(ValueError, match=pattern):
      gm.gridmask(raw, boxes, rng=rng, sizes=bad)
    with pytest.raises(ValueError, match=pattern):
      daa.distort_image_with_autoaugment(raw, boxes, COUNTS, 'v2', rng=rng, sizes=bad)
    with pytest.raises(ValueError, match=pattern):
      daa.distort_image_with_randaugment(raw, boxes, COUNTS, 1, 15, rng=rng, sizes=bad)
    with pytest.raises(ValueError, match=pattern):
      preprocess.DetectionInputProcessor(torch.from_numpy(raw), 64, sizes=bad)
    assert state_of(rng) == before
  for wrong in (good[:3], good.reshape(-1), good.astype(np.float32), [[1, 2, 3]] * B):
    with pytest.raises(ValueError, match='sizes must be integers'):
      utils.canvas_sizes(wrong, B, ch, cw)
  # GridMask's block range per image: a 24 x 3 image inside the canvas has int(min(H / 2, 0.3 W)) = 0
  thin = good.copy()
  thin[1] = (24, 3)
  rng = np.random.default_rng(4)
  before = state_of(rng)
  with pytest.raises(ValueError, match=r'image 1, a 24 x 3 image'):
    gm.gridmask_draws(rng, B, thin[:, 0], thin[:, 1])
  with pytest.raises(ValueError, match=r'image 1, a 24 x 3 image'):
    gm.gridmask(raw, boxes, rng=rng, sizes=thin)
  with pytest.raises(ValueError, match=r'image 1, a 24 x 3 image'):
    gm.gridmask_args(gm.gridmask_draws(np.random.default_rng(0), B, ch, cw), thin[:, 0], thin[:, 1])
  assert state_of(rng) == before
  # a device tensor or a list is as good as an array; what comes back is int32 [B, 2]
  out = utils.canvas_sizes(torch.tensor(good.tolist()), B, ch, cw)
  assert out.dtype == np.int32 and np.array_equal(out, good) and np.array_equal(utils.canvas_sizes(good.tolist(), B, ch, cw), good)


def test_a_dense_call_builds_the_rows_it_always_did():
  """Without sizes: gridmask_draws takes the stream of the documented recipe, and rows from two numbers equal rows from arrays
  that repeat them -- so the per-image code path and the dense one are the same arithmetic."""
  h, w, b = 40, 56, 5
  d = gm.gridmask_draws(np.random.default_rng(21), b, h, w)
  rng = np.random.default_rng(21)
  lo, hi = gm.block_range(h, w)
  want_d = rng.integers(lo, hi + 1, size=b).astype(np.int32)
  want_s1, want_s2 = rng.integers(0, want_d + 1).astype(np.int32), rng.integers(0, want_d + 1).astype(np.int32)
  want_z1, want_z2 = (rng.standard_normal(b) - 1.0).astype(np.float32), rng.standard_normal(b).astype(np.float32)
  for got, want in zip(d, (want_d, want_s1, want_s2, want_z1, want_z2)):
    assert got.dtype == want.dtype and np.array_equal(got, want)
  rows = gm.gridmask_args(d, h, w)
  assert rows.tobytes() == gm.gridmask_args(d, np.full(b, h), np.full(b, w)).tobytes()
  assert int(rows['size'][0]) == gm.mask_side(h, w) and rows['coef'].dtype == np.float32
  for policy in ('v2', 'randaug'):
    dd = daa.autoaug_draws(np.random.default_rng(2), b, policy, num_layers=2)
    dense = daa.autoaug_args(dd, policy, h, w, magnitude=15)
    for a, c in zip(dense, daa.autoaug_args(dd, policy, np.full(b, h), np.full(b, w), magnitude=15)):
      assert np.array_equal(bits(a), bits(c))
  per, scales = det_input.eval_rows((128, 128), np.tile([h, w], (b, 1)))
  scale, scaled = preprocess.output_size_scale_factors((128, 128), h, w)
  assert per.tolist() == [[0, scaled[0], scaled[1], 0, 0]] * b and scales.tolist() == [float(np.float32(1.0) / scale)] * b
