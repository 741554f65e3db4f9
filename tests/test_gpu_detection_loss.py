"""The detection loss kernels (csrc/det_loss.hip: edet_focal_loss, edet_focal_loss_smooth, edet_box_loss and their _eval twins)
against the float64 closed form of tests/loss_ref.py, ELEMENT BY ELEMENT: every gradient within the bound loss_ref derives from
the kernel's arithmetic for that element (no max-norm: the focal gradient spans many decades), the bias gradients and the loss
sums against exactly rounded sums of the reference, the loss of single elements through one-element launches.  General gamma
(the pow instantiations k_focal<T, false>, k_focal_ls<T, false>, k_focal_eval<T, false, *>, asserted through the launch
log), saturated logits (|x| up to 200 and 3e38, where exp2 flushes and the sigmoid is 0 or 1 exactly), NaN wherever the
kernels promise not to read, row strides beyond pad8(channels), the grid cap, and the argument space of the entry points.

Largest err / bound seen on the MI355X, per dtype and gamma (every test of this file; printed by each test as it runs):

  dtype gamma   gradient of an element   loss of an element   bias gradient   loss sum
  f32   0       0.312                    0.347                0.150           0.002
  f32   0.5     1.000                    1.000                0.269           0.005
  f32   1       0.438                    0.347                0.298           0.001
  f32   1.5     0.435                    0.347                0.302           0.120
  f32   2       0.435                    0.347                0.287           0.018
  f32   2.5     0.433                    0.347                0.285           0.077
  bf16  0       0.960                    0.347                < 0.001         0.188
  bf16  0.5     0.992                    1.000                < 0.001         0.153
  bf16  1       0.993                    0.347                < 0.001         0.096
  bf16  1.5     0.991                    0.347                < 0.001         < 0.001
  bf16  2       0.982                    0.347                < 0.001         0.066
  bf16  2.5     0.983                    0.347                < 0.001         0.001
  box   f32     0.776                    -                    0.024           0.006
  box   bf16    0.993                    -                    < 0.001         0.014

What the figures are.  bf16 gradients near 1: the storage rounding, half a bf16 ulp, is the bound and is reached (the float32
error in front of it is ~0.4 of its own bound).  0.347: 1 + ex rounds to 1 once ex < 2^-24 (|u| > 16.6), so the kernel's
log(1 + ex) is 0 where it should be ex: the loss of a well-classified element (x = +-17, +-40: 6e-14, 6e-29 / normalizer) comes
out as 0 and its gradient loses the gamma (1 - sg) sp part of the bracket (33 - 60 % of a gradient of 1e-13) -- the absolute
log term of the bound, 2^-23 af sg^gamma / normalizer, a third used.  1.000 at gamma 0.5: the flush of v_exp_f32 below 2^-126;
at u = -89 (and beyond) the kernel's sg is 0 and its loss and gradient are 0 where the reference has 1.4e-21 and 7e-22 (at
u = -87 both are right to 1e-6): the bound's flush term is the value itself, so the ratio is 1 by construction; with gamma >= 1
the same elements lie below 2^-126 and with gamma 0 the modulating factor is 1.  No ratio above 1, no kernel arithmetic changed.
"""
import itertools
import math

import numpy as np
import pytest
import torch

from automl_amd import _lib
from automl_amd._lib import call, ptr
from tests import gpu_util as gu
from tests import loss_ref as lr

gpu = pytest.mark.gpu
DT = {'f32': (_lib.EDET_F32, torch.float32, 'float'), 'bf16': (_lib.EDET_BF16, torch.bfloat16, 'unsigned short')}
NORM = 37.0
# (n, h, w, anchors, classes): the COCO width (ld 816, 128 threads per row); a chunk is exactly one anchor; the body for fewer
# than 8 classes; one class and one anchor (seven of the eight lanes are padding); ld 2048, the largest accepted (256 threads
# per row, one row per pass)
GEOMS = [(2, 5, 4, 9, 90), (1, 4, 4, 3, 8), (2, 6, 3, 9, 3), (1, 3, 3, 1, 1), (1, 2, 2, 16, 128)]
GAMMAS = (0.0, 0.5, 1.0, 2.0, 2.5, 1.5)      # 1.5 is the control: the sqrt instantiations
ALPHAS = (0.25, 0.6)
SMOOTHINGS = (0.0, 0.1)
PLANTED = [0.0] + [s * v for v in (1e-3, 1.0, 8.0, 17.0, 40.0, 87.0, 89.0, 104.0, 200.0) for s in (1.0, -1.0)]
HUGE = [3e38, -3e38]
_CACHE = {}
SEEN = {}      # (dtype, gamma) -> {check: largest err / bound}


def f32(v):
  return float(np.float32(v))


def seen(name, gamma, what, ratio):
  d = SEEN.setdefault((name, gamma), {})
  d[what] = max(d.get(what, 0.0), ratio)
  print('err / bound [%s gamma %s] %s: %.3f (largest so far %.3f)' % (name, gamma, what, ratio, d[what]))


def stored(values, tdt):
  """float64 numpy of the values as the storage dtype holds them (bf16: the representable neighbours)."""
  return torch.as_tensor(np.asarray(values, np.float32)).to(tdt).double().numpy()


def focal_cases():
  """Every (gamma, smoothing, dtype) on two geometries; alpha, the workspace / one-workgroup path and the 3e38 plants
  alternate.  48 cases."""
  out = []
  for c, (gamma, smoothing, name) in enumerate(itertools.product(GAMMAS, SMOOTHINGS, DT)):
    for j in range(2):
      out.append((GEOMS[(c + 2 * j + c // 5) % 5], name, gamma, ALPHAS[(c // 2 + j) % 2], smoothing, bool((c + j) % 2), j == 1 and (c + c // 4) % 2 == 0))
  return out


FOCAL_CASES = focal_cases()


def case_id(c):
  return '%s-%s-g%g-a%g-ls%g-%s%s' % ('x'.join(map(str, c[0])), c[1], c[2], c[3], c[4], 'ws' if c[5] else 'one', '-huge' if c[6] else '')


def test_case_list_reaches_every_general_gamma_instantiation():
  """(CPU) train, smooth and eval kernels x both dtypes x both bodies (fewer than 8 classes, 8 or more) with gamma != 1.5;
  every gamma with both smoothing settings and both dtypes; both paths; with and without the 3e38 plants."""
  assert 45 <= len(FOCAL_CASES) <= 64 and len(set(FOCAL_CASES)) == len(FOCAL_CASES)
  general = {(c[1], c[4] != 0, c[0][4] < 8) for c in FOCAL_CASES if c[2] != 1.5}
  assert general == set(itertools.product(DT, (False, True), (False, True)))
  assert {(c[2], c[4], c[1]) for c in FOCAL_CASES} == set(itertools.product(GAMMAS, SMOOTHINGS, DT))
  assert {c[0] for c in FOCAL_CASES} == set(GEOMS)
  for name in DT:
    for gamma in GAMMAS:
      mine = [c for c in FOCAL_CASES if c[1] == name and c[2] == gamma]
      assert {c[5] for c in mine} == {False, True} and {c[3] for c in mine} == set(ALPHAS), (name, gamma)
    assert {c[6] for c in FOCAL_CASES if c[1] == name} == {False, True}


# ------------------------------------------------------------------------------------------------------------ inputs
def focal_problem(geom, name, huge):
  """(x [positions, nch] float64 as stored, targets [positions, na] int32): N(0, 2^2) logits, 55 % background, 15 % ignored
  anchors; the planted logits (in an order of the case's own) on a positive anchor -- on its positive class and on a negative
  one --, the next anchor ignored, and on the anchor after that, a background one (with fewer than three anchors: positive and
  background and ignored anchors in turn)."""
  key = ('focal', geom, name, huge)
  if key not in _CACHE:
    n, h, w, na, nc = geom
    p, tdt = n * h * w, DT[name][1]
    rng = np.random.default_rng(gu.seed_of(*key))
    x = gu.rnd(rng, (p, na * nc), tdt, 2.0).double().numpy()
    t = rng.integers(0, nc, (p, na)).astype(np.int32)
    r = rng.random((p, na))
    t[r < 0.7] = -1
    t[r < 0.15] = -2
    values = stored(rng.permutation(PLANTED + (HUGE if huge else [])), tdt)
    slots = [(q, a) for q in range(p) for a in range(0, na - 2, 3)] if na >= 3 else [(q, 0) for q in range(p)]
    for i, (v, (q, a)) in enumerate(zip(values, slots)):
      k = i % nc
      if na >= 3:
        t[q, a:a + 3] = [k, -2, -1]
        x[q, a * nc + k] = x[q, a * nc + (k + 1) % nc] = x[q, (a + 2) * nc + k] = v
      else:
        t[q, a] = (k, -1, -2)[i % 3]
        x[q, a * nc + k] = v
    assert np.isfinite(x).all() and (t == -2).any()
    _CACHE[key] = (x, t)
  return _CACHE[key]


def device_logits(x, t, na, nc, tdt, ld, garbage):
  """[positions, ld] on the device; garbage: NaN in the padding columns and in the logits of the ignored anchors."""
  p, nch = x.shape
  out = torch.full((p, ld), float('nan') if garbage else 0.0, dtype=torch.float32)
  xs = torch.from_numpy(x).float()
  if garbage:
    xs = torch.where(torch.from_numpy(np.repeat(t == -2, nc, axis=1)), torch.full_like(xs, float('nan')), xs)
  out[:, :nch] = xs
  return out.to(gu.DEV).to(tdt).contiguous()


def focal_reference(geom, name, huge, alpha, gamma, smoothing, inv):
  key = ('focal_ref', geom, name, huge, alpha, gamma, smoothing, inv)
  if _CACHE.get('focal_ref_key') != key:
    x, t = focal_problem(geom, name, huge)
    args = (x, t, geom[3], geom[4], alpha, gamma, smoothing, inv)
    _CACHE['focal_ref_key'], _CACHE['focal_ref'] = key, lr.focal_ref(*args) + lr.focal_bound(*args, name)
  return _CACHE['focal_ref']


def workspace():
  if 'ws' not in _CACHE:
    _CACHE['ws'] = torch.empty(4096 * 811, dtype=torch.float32, device=gu.DEV)      # the rows of the largest grid here
  return _CACHE['ws']


def bits(t):
  return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def run_focal(logits, td, na, nc, name, alpha, gamma, smoothing, inv, use_ws, norm_dev=None):
  """The training entry point (edet_focal_loss when smoothing == 0) and the evaluation one on the same inputs ->
  (dlogits, dbias, training sums, evaluation sums, launch log)."""
  edt = DT[name][0]
  p, ld = logits.shape
  dl = torch.full_like(logits, float('nan'))
  dbias = torch.zeros(na * nc, dtype=torch.float32, device=gu.DEV)
  sums, esums = torch.zeros(4, dtype=torch.float32, device=gu.DEV), torch.zeros(4, dtype=torch.float32, device=gu.DEV)
  ws = workspace() if use_ws else None
  wsb = ws.numel() * 4 if use_ws else 0
  _lib.launch_log_start()
  try:
    if smoothing:
      call('edet_focal_loss_smooth', ptr(logits), ld, ptr(td), p, na, nc, alpha, gamma, smoothing, inv, ptr(norm_dev), ptr(dl),
           ptr(dbias), ptr(sums), ptr(ws), wsb, edt, gu.stream())
    else:
      call('edet_focal_loss', ptr(logits), ld, ptr(td), p, na, nc, alpha, gamma, inv, ptr(norm_dev), ptr(dl), ptr(dbias), ptr(sums),
           ptr(ws), wsb, edt, gu.stream())
    call('edet_focal_loss_eval', ptr(logits), ld, ptr(td), p, na, nc, alpha, gamma, smoothing, inv, ptr(norm_dev), ptr(esums),
         ptr(ws), wsb, edt, gu.stream())
    torch.cuda.synchronize()
  finally:
    log = _lib.launch_log_stop()
  return dl, dbias, sums, esums, log


def assert_instantiations(log, name, gamma, smoothing):
  """The launch log names the instantiation of this gamma -- k_focal<T, G15> or k_focal_ls<T, G15>, and
  k_focal_eval<T, G15, LS> -- and no focal kernel of the other one."""
  t, g = DT[name][2], 'true' if gamma == 1.5 else 'false'
  other = 'false' if gamma == 1.5 else 'true'
  focal = [k for k in log if 'k_focal' in k]
  train = ('k_focal_ls<%s, %s>(' if smoothing else 'k_focal<%s, %s>(') % (t, g)
  evl = 'k_focal_eval<%s, %s, %s>(' % (t, g, 'true' if smoothing else 'false')
  assert len(focal) == 2 and any(train in k for k in focal) and any(evl in k for k in focal), (train, evl, sorted(log))
  assert not any(('%s, %s>(' % (t, other)) in k or ('%s, %s, ' % (t, other)) in k for k in focal), sorted(log)


def check_sums(got_dbias, got_sum, grad, gb, loss, lb, rows, n_valid, name, gamma):
  """Bias gradients against exactly rounded column sums: the column's element bounds plus rows 2^-24 sum |g| for a float32
  sum in any order.  Loss sum: the element bounds plus n_valid 2^-24 S (the terms are non-negative)."""
  want = lr.column_sums(grad)
  bound = lr.column_sums(gb) + rows * lr.U24 * lr.column_sums(np.abs(grad))
  seen(name, gamma, 'bias gradient', lr.assert_within(got_dbias.cpu().numpy(), want, bound, 'bias gradient'))
  s = math.fsum(loss.ravel().tolist())
  seen(name, gamma, 'loss sum', lr.assert_within(np.asarray([float(got_sum)]), np.asarray([s]),
                                                 np.asarray([lr.sum_bound(loss, lb, n_valid)]), 'loss sum'))


# ------------------------------------------------------------------------------------------------------ focal: tensors
@gpu
@pytest.mark.parametrize('case', FOCAL_CASES, ids=case_id)
def test_focal_loss_element_by_element(case):
  geom, name, gamma, alpha, smoothing, use_ws, huge = case
  n, h, w, na, nc = geom
  nch, tdt = na * nc, DT[name][1]
  alpha, smoothing, inv = f32(alpha), f32(smoothing), f32(1.0 / NORM)
  x, t = focal_problem(geom, name, huge)
  loss, grad, lb, gb = focal_reference(geom, name, huge, alpha, gamma, smoothing, inv)
  logits = device_logits(x, t, na, nc, tdt, gu.pad8(nch), False)
  td = torch.from_numpy(t).to(gu.DEV)
  dl, dbias, sums, esums, log = run_focal(logits, td, na, nc, name, alpha, gamma, smoothing, inv, use_ws)
  assert_instantiations(log, name, gamma, smoothing)
  assert bool(torch.isfinite(dl.float()).all()) and bool(torch.isfinite(dbias).all()) and bool(torch.isfinite(sums).all())
  got = dl[:, :nch].double().cpu().numpy()
  seen(name, gamma, 'gradient', lr.assert_within(got, grad, gb, 'dlogits'))
  assert nch == logits.shape[1] or float(dl[:, nch:].float().abs().max()) == 0.0      # padding columns are written as zeros
  valid = np.repeat(t != -2, nc, axis=1)
  check_sums(dbias, sums[0], grad, gb, loss, lb, x.shape[0], int(valid.sum()), name, gamma)
  # the evaluation kernel: the training kernel's sum bit for bit, nothing else touched; and the same bits on a second run
  assert np.array_equal(bits(sums), bits(esums)) and float(sums[1]) == 0 and float(sums[2]) == 0
  again = run_focal(logits, td, na, nc, name, alpha, gamma, smoothing, inv, use_ws)
  for a, b, what in zip((dl, dbias, sums, esums), again, ('dlogits', 'bias gradient', 'loss sum', 'evaluation loss sum')):
    assert np.array_equal(bits(a), bits(b)), 'run-to-run difference in the %s' % what


@gpu
@pytest.mark.parametrize('name', list(DT))
@pytest.mark.parametrize('gamma,smoothing', [(2.0, 0.1), (0.0, 0.0), (1.5, 0.1)])
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'x'.join(map(str, g)))
def test_focal_loss_reads_nothing_it_may_not(geom, gamma, smoothing, name):
  """NaN in the padding columns and in the logits of the ignored anchors, row strides of pad8(channels), + 8 and + 16 (up to
  the largest accepted): gradient, bias gradient and both sums bit-identical to the clean run of that stride (zeros in the
  padding columns; the stride chooses the rows per workgroup, and with them the order of the sums), padding columns zeros."""
  n, h, w, na, nc = geom
  nch, tdt = na * nc, DT[name][1]
  alpha, smoothing, inv = 0.25, f32(smoothing), f32(1.0 / NORM)
  x, t = focal_problem(geom, name, True)
  td = torch.from_numpy(t).to(gu.DEV)
  assert (t == -2).any()
  for use_ws in (True, False):
    narrow = None
    for ld in (gu.pad8(nch), gu.pad8(nch) + 8, gu.pad8(nch) + 16):
      if ld > 2048:
        continue
      clean = run_focal(device_logits(x, t, na, nc, tdt, ld, False), td, na, nc, name, alpha, gamma, smoothing, inv, use_ws)
      narrow = narrow or clean
      assert bool(torch.isfinite(clean[0].float()).all())
      assert np.array_equal(bits(clean[0][:, :nch]), bits(narrow[0][:, :nch])), ld      # elementwise: whatever the stride
      dirty = run_focal(device_logits(x, t, na, nc, tdt, ld, True), td, na, nc, name, alpha, gamma, smoothing, inv, use_ws)
      assert np.array_equal(bits(dirty[0][:, :nch]), bits(clean[0][:, :nch])), ld
      assert ld == nch or float(dirty[0][:, nch:].float().abs().max()) == 0.0
      for a, b in zip(clean[1:4], dirty[1:4]):
        assert np.array_equal(bits(a), bits(b)), ld


# ------------------------------------------------------------------------------------------- focal: one element at a time
@gpu
@pytest.mark.parametrize('name', list(DT))
@pytest.mark.parametrize('smoothing', SMOOTHINGS)
@pytest.mark.parametrize('gamma', GAMMAS)
def test_focal_loss_of_single_elements(gamma, smoothing, name):
  """positions = 1, one anchor, one class, ld = 8 (the seven padding lanes hold NaN): sums[0] is the loss of that element, the
  planted logits and +-3e38 on the positive and on the background target.  Loss, gradient and the evaluation kernel's loss."""
  edt, tdt, _ = DT[name]
  alpha, smoothing, inv = 0.25, f32(smoothing), f32(1.0 / NORM)
  values = stored(PLANTED + HUGE, tdt)
  xs = np.repeat(values, 2).reshape(-1, 1)
  ts = np.tile(np.asarray([0, -1], np.int32), len(values)).reshape(-1, 1)
  m = xs.shape[0]
  logits = device_logits(xs, ts, 1, 1, tdt, 8, True)
  td = torch.from_numpy(ts).to(gu.DEV)
  dl = torch.full_like(logits, float('nan'))
  dbias = torch.zeros(m, 1, dtype=torch.float32, device=gu.DEV)
  sums, esums = torch.zeros(m, 4, dtype=torch.float32, device=gu.DEV), torch.zeros(m, 4, dtype=torch.float32, device=gu.DEV)
  ws = workspace()
  for i in range(m):
    wsb = ws.numel() * 4 if i % 3 else 0      # with the partial row and as one workgroup
    if smoothing:
      call('edet_focal_loss_smooth', ptr(logits[i]), 8, ptr(td[i]), 1, 1, 1, alpha, gamma, smoothing, inv, None, ptr(dl[i]),
           ptr(dbias[i]), ptr(sums[i]), ptr(ws), wsb, edt, gu.stream())
    else:
      call('edet_focal_loss', ptr(logits[i]), 8, ptr(td[i]), 1, 1, 1, alpha, gamma, inv, None, ptr(dl[i]), ptr(dbias[i]),
           ptr(sums[i]), ptr(ws), wsb, edt, gu.stream())
    call('edet_focal_loss_eval', ptr(logits[i]), 8, ptr(td[i]), 1, 1, 1, alpha, gamma, smoothing, inv, None, ptr(esums[i]), ptr(ws),
         wsb, edt, gu.stream())
  torch.cuda.synchronize()
  loss, grad = lr.focal_ref(xs, ts, 1, 1, alpha, gamma, smoothing, inv)
  lb, gb = lr.focal_bound(xs, ts, 1, 1, alpha, gamma, smoothing, inv, name)
  print('x, target, loss, want, gradient, want:')
  for i in range(m):
    print('  %-12g %2d  %-14.8g %-14.8g %-14.8g %-14.8g' % (xs[i, 0], ts[i, 0], float(sums[i, 0]), loss[i, 0], float(dl[i, 0]), grad[i, 0]))
  assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(dl[:, 0].float()).all())
  seen(name, gamma, 'loss of an element', lr.assert_within(sums[:, :1].cpu().numpy(), loss, lb, 'loss of a single element'))
  seen(name, gamma, 'gradient', lr.assert_within(dl[:, :1].double().cpu().numpy(), grad, gb, 'gradient of a single element'))
  # the bias gradient of a one-element launch is the float32 gradient before it is stored: the float32 bound in both dtypes
  lr.assert_within(dbias.cpu().numpy(), grad, lr.focal_bound(xs, ts, 1, 1, alpha, gamma, smoothing, inv, 'f32')[1], 'bias gradient')
  assert float(dl[:, 1:].float().abs().max()) == 0.0 and float(sums[:, 1:].abs().max()) == 0.0
  assert np.array_equal(bits(sums), bits(esums))


# ------------------------------------------------------------------------------------------------ focal: the grid cap
@gpu
@pytest.mark.parametrize('gamma,smoothing', [(2.0, 0.1), (1.5, 0.0)])
def test_focal_loss_past_the_grid_cap(gamma, smoothing):
  """810 channels in bf16 rows of 816 (two rows per pass) and 3 x 2048 x 4 x 2 = 49152 positions: the grid rule asks for
  ceil(ceil(positions / 2) / 4) = 6144 workgroups, three times the 2048 a chip of 256 CUs holds of this kernel and above the
  4096 of the rule's fallback, so the cap is taken and every workgroup strides over its rows three times.  The rows repeat
  with a period of 1021 (a prime: the stride of 2 x cap rows is no multiple of it), so the reference is 1021 rows."""
  name, na, nc, period, p = 'bf16', 9, 90, 1021, 3 * 2048 * 4 * 2
  edt, tdt, _ = DT[name]
  nch, ld = na * nc, gu.pad8(na * nc)
  alpha, smoothing, inv = 0.25, f32(smoothing), f32(1.0 / 4001.0)
  rng = np.random.default_rng(77)
  x = gu.rnd(rng, (period, nch), tdt, 2.0).double().numpy()
  t = rng.integers(0, nc, (period, na)).astype(np.int32)
  r = rng.random((period, na))
  t[r < 0.7] = -1
  t[r < 0.15] = -2
  idx = torch.arange(p) % period
  logits = device_logits(x, t, na, nc, tdt, ld, True)[idx.to(gu.DEV)].contiguous()
  td = torch.from_numpy(t)[idx].to(gu.DEV).contiguous()
  assert logits.shape == (p, ld) and logits.numel() * 2 < 100e6
  dl, dbias, sums, esums, log = run_focal(logits, td, na, nc, name, alpha, gamma, smoothing, inv, True)
  assert_instantiations(log, name, gamma, smoothing)
  args = (x, t, na, nc, alpha, gamma, smoothing, inv)
  (loss, grad), (lb, gb) = lr.focal_ref(*args), lr.focal_bound(*args, name)
  got = dl.float().cpu()
  assert bool(torch.isfinite(got).all()) and float(got[:, nch:].abs().max()) == 0.0
  worst = 0.0
  for b in range(0, p, period):
    g = got[b:b + period, :nch].double().numpy()
    worst = max(worst, lr.assert_within(g, grad[:len(g)], gb[:len(g)], 'dlogits of rows %d ..' % b))
  seen(name, gamma, 'gradient', worst)
  # the sums of the whole tensor from the period's: full periods and the remainder, in float64 (2^-53 relative: nothing
  # against the float32 bounds)
  full, rem = divmod(p, period)
  colsum = lambda a: full * lr.column_sums(a) + lr.column_sums(a[:rem])      # noqa: E731
  want, bound = colsum(grad), colsum(gb) + p * lr.U24 * colsum(np.abs(grad))
  seen(name, gamma, 'bias gradient', lr.assert_within(dbias.cpu().numpy(), want, bound, 'bias gradient'))
  total = lambda a: full * math.fsum(a.ravel().tolist()) + math.fsum(a[:rem].ravel().tolist())      # noqa: E731
  n_valid = full * int((t != -2).sum()) * nc + int((t[:rem] != -2).sum()) * nc
  seen(name, gamma, 'loss sum', lr.assert_within(np.asarray([float(sums[0])]), np.asarray([total(loss)]),
                                                 np.asarray([total(lb) + n_valid * lr.U24 * total(loss)]), 'loss sum'))
  assert np.array_equal(bits(sums), bits(esums))


# ------------------------------------------------------------------------------------------------------------- the box loss
def neighbour(v, tdt, up):
  """The next value of the storage dtype above (up) or below a positive v."""
  if tdt == torch.float32:
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else 0.0)))
  b = torch.tensor([v], dtype=torch.float32).to(torch.bfloat16).view(torch.int16)
  return float((b + (1 if up else -1)).view(torch.bfloat16).float())


def box_problem(positions, nch, name, delta):
  """Outputs N(0, 0.3^2) and targets N(0, 0.2^2), 55 % of them masked (0.0, and -0.0 in row 0); errors planted at +-delta (for
  delta 0.125 and these targets x - t is exact in bf16 and in float32), one value of the storage dtype inside and outside, and
  at +-1e4."""
  key = ('box', positions, nch, name, delta)
  if key not in _CACHE:
    tdt = DT[name][1]
    rng = np.random.default_rng(gu.seed_of(*key))
    x = gu.rnd(rng, (positions, nch), tdt, 0.3).double().numpy()
    t = (rng.standard_normal((positions, nch)) * 0.2).astype(np.float32)
    t[rng.random((positions, nch)) < 0.55] = 0.0
    t[0, ::2] = -0.0
    d = f32(delta)
    plants = []
    for base in (1.5, 2.0, 4.0):
      for e in (d, -d):
        v = float(stored([base + e], tdt)[0])
        plants += [(base, v), (base, neighbour(v, tdt, True)), (base, neighbour(v, tdt, False))]
      plants += [(base, float(stored([base + 1e4], tdt)[0])), (base, float(stored([base - 1e4], tdt)[0]))]
    for i, (base, v) in enumerate(plants):
      q, j = 1 + i // nch, i % nch
      t[q, j], x[q, j] = base, v
    assert np.isfinite(x).all() and (delta != 0.125 or (np.abs(x - t.astype(np.float64)) == 0.125).sum() >= 6)
    _CACHE[key] = (x, t)
  return _CACHE[key]


def run_box(x, t, name, delta, inv, grad_scale, norm_dev, use_ws, ld, garbage):
  edt, tdt, _ = DT[name]
  p, nch = x.shape
  out = torch.full((p, ld), float('nan') if garbage else 0.0, dtype=torch.float32)
  xs = torch.from_numpy(x).float()
  if garbage:      # NaN where the target masks the slot
    xs = torch.where(torch.from_numpy(t == 0), torch.full_like(xs, float('nan')), xs)
  out[:, :nch] = xs
  box = out.to(gu.DEV).to(tdt).contiguous()
  td = torch.from_numpy(t).to(gu.DEV)
  db = torch.full_like(box, float('nan'))
  dbias = torch.zeros(nch, dtype=torch.float32, device=gu.DEV)
  sums, esums = torch.zeros(4, dtype=torch.float32, device=gu.DEV), torch.zeros(4, dtype=torch.float32, device=gu.DEV)
  ws = workspace() if use_ws else None
  wsb = ws.numel() * 4 if use_ws else 0
  _lib.launch_log_start()
  try:
    call('edet_box_loss', ptr(box), ld, ptr(td), p, nch, delta, inv, grad_scale, ptr(norm_dev), ptr(db), ptr(dbias), ptr(sums),
         ptr(ws), wsb, edt, gu.stream())
    call('edet_box_loss_eval', ptr(box), ld, ptr(td), p, nch, delta, inv, ptr(norm_dev), ptr(esums), ptr(ws), wsb, edt, gu.stream())
    torch.cuda.synchronize()
  finally:
    log = _lib.launch_log_stop()
  t_ = DT[name][2]
  assert any('k_box<%s>(' % t_ in k for k in log) and any('k_box_eval<%s>(' % t_ in k for k in log), sorted(log)
  return db, dbias, sums, esums


@gpu
@pytest.mark.parametrize('name', list(DT))
@pytest.mark.parametrize('device_norm', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('grad_scale', [50.0, 1.0])
@pytest.mark.parametrize('delta', [0.05, 0.125, 1.0])
@pytest.mark.parametrize('positions,nch', [(301, 36), (70, 4)])
def test_box_loss_element_by_element(positions, nch, delta, grad_scale, device_norm, name):
  """36 channels in rows of 40 (32 rows per pass, three workgroups) and 4 in rows of 8.  The normalizer as a host float, and
  as a device scalar with inv_normalizer = 1.  Then NaN in the masked slots and the padding columns, rows of pad8 + 8 and
  + 16: bit-identical to the clean run of that stride."""
  delta, inv = f32(delta), f32(1.0 / (4.0 * NORM))
  x, t = box_problem(positions, nch, name, delta)
  norm_dev = torch.tensor([inv], dtype=torch.float32, device=gu.DEV) if device_norm else None
  inv_arg = 1.0 if device_norm else inv
  use_ws = (nch == 36) != device_norm
  loss, grad = lr.box_ref(x, t, delta, inv, grad_scale)
  lb, gb = lr.box_bound(x, t, delta, inv, grad_scale, name)
  ld = gu.pad8(nch)
  db, dbias, sums, esums = run_box(x, t, name, delta, inv_arg, grad_scale, norm_dev, use_ws, ld, False)
  assert bool(torch.isfinite(db.float()).all()) and bool(torch.isfinite(sums).all())
  seen(name, 'box', 'gradient', lr.assert_within(db[:, :nch].double().cpu().numpy(), grad, gb, 'dbox'))
  assert ld == nch or float(db[:, nch:].float().abs().max()) == 0.0
  assert not grad[0, ::2].any() and not bits(db[0, :nch:2]).any()      # targets of -0.0 are masked
  want = lr.column_sums(grad)
  bound = lr.column_sums(gb) + positions * lr.U24 * lr.column_sums(np.abs(grad))
  seen(name, 'box', 'bias gradient', lr.assert_within(dbias.cpu().numpy(), want, bound, 'box bias gradient'))
  s = math.fsum(loss.ravel().tolist())
  seen(name, 'box', 'loss sum', lr.assert_within(np.asarray([float(sums[1])]), np.asarray([s]),
                                                 np.asarray([lr.sum_bound(loss, lb, int((t != 0).sum()))]), 'box loss sum'))
  assert float(sums[0]) == 0 and np.array_equal(bits(sums), bits(esums))
  for ld2 in (ld, ld + 8, ld + 16):      # (the stride chooses the rows per workgroup, and with them the order of the sums)
    clean = run_box(x, t, name, delta, inv_arg, grad_scale, norm_dev, use_ws, ld2, False)
    dirty = run_box(x, t, name, delta, inv_arg, grad_scale, norm_dev, use_ws, ld2, True)
    assert np.array_equal(bits(clean[0][:, :nch]), bits(db[:, :nch])), ld2
    assert ld2 != ld or all(np.array_equal(bits(a), bits(b)) for a, b in zip((dbias, sums, esums), clean[1:])), 'run to run'
    for a, b in zip(clean, dirty):
      assert np.array_equal(bits(a), bits(b)), ld2
    assert ld2 == nch or float(dirty[0][:, nch:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------ the argument space
def loss_calls(name='f32'):
  """name -> f(**overrides): the four entry points on a small valid problem (2 positions, 3 anchors, 5 classes, rows of 16)."""
  edt, tdt, _ = DT[name]
  logits = torch.zeros(4, 24, dtype=tdt, device=gu.DEV)
  td = torch.zeros(4, 3, dtype=torch.int32, device=gu.DEV)
  bt = torch.ones(4, 12, dtype=torch.float32, device=gu.DEV)
  state = dict(dl=torch.full_like(logits, float('nan')), dbias=torch.full((16,), 3.5, device=gu.DEV),
               sums=torch.tensor([-0.0, 7.25, 1.0, 2.0], device=gu.DEV))
  base = dict(ld=16, positions=2, na=3, nc=5, nch=12, alpha=0.25, gamma=2.0, ls=0.1, delta=0.1, inv=0.5)

  def focal(smooth, **kw):
    a = dict(base, **kw)
    if smooth:
      call('edet_focal_loss_smooth', ptr(logits), a['ld'], ptr(td), a['positions'], a['na'], a['nc'], a['alpha'], a['gamma'], a['ls'],
           a['inv'], None, ptr(state['dl']), ptr(state['dbias']), ptr(state['sums']), None, 0, edt, gu.stream())
    else:
      call('edet_focal_loss', ptr(logits), a['ld'], ptr(td), a['positions'], a['na'], a['nc'], a['alpha'], a['gamma'], a['inv'], None,
           ptr(state['dl']), ptr(state['dbias']), ptr(state['sums']), None, 0, edt, gu.stream())

  def focal_eval(**kw):
    a = dict(base, **kw)
    call('edet_focal_loss_eval', ptr(logits), a['ld'], ptr(td), a['positions'], a['na'], a['nc'], a['alpha'], a['gamma'], a['ls'],
         a['inv'], None, ptr(state['sums']), None, 0, edt, gu.stream())

  def box(**kw):
    a = dict(base, **kw)
    call('edet_box_loss', ptr(logits), a['ld'], ptr(bt), a['positions'], a['nch'], a['delta'], a['inv'], 50.0, None, ptr(state['dl']),
         ptr(state['dbias']), ptr(state['sums']), None, 0, edt, gu.stream())

  def box_eval(**kw):
    a = dict(base, **kw)
    call('edet_box_loss_eval', ptr(logits), a['ld'], ptr(bt), a['positions'], a['nch'], a['delta'], a['inv'], None, ptr(state['sums']),
         None, 0, edt, gu.stream())

  calls = {'edet_focal_loss': lambda **kw: focal(False, **kw), 'edet_focal_loss_smooth': lambda **kw: focal(True, **kw),
           'edet_focal_loss_eval': focal_eval, 'edet_box_loss': box, 'edet_box_loss_eval': box_eval}
  return calls, state


@gpu
def test_loss_entry_points_refuse_bad_arguments():
  """Refused with EdetError, before anything is launched or written: a negative or non-finite gamma, alpha outside [0, 1], a
  non-positive or non-finite delta, rows wider than 2048, rows that are no multiple of 8 or narrower than the channels, no
  classes.  The valid call goes through."""
  calls, state = loss_calls()
  before = {k: bits(v).copy() for k, v in state.items()}
  nan, inf = float('nan'), float('inf')
  focal_bad = [dict(gamma=-0.5), dict(gamma=nan), dict(gamma=inf), dict(gamma=-inf), dict(alpha=-0.01), dict(alpha=1.01),
               dict(alpha=nan), dict(alpha=inf), dict(ld=2056), dict(ld=20), dict(ld=8), dict(nc=0, ld=16), dict(nc=-1),
               dict(na=0), dict(positions=-1)]
  box_bad = [dict(delta=0.0), dict(delta=-0.1), dict(delta=nan), dict(delta=inf), dict(ld=2056), dict(ld=20), dict(ld=8),
             dict(nch=0), dict(positions=-1)]
  for fn, bad in (('edet_focal_loss', focal_bad), ('edet_focal_loss_smooth', focal_bad + [dict(ls=-0.1), dict(ls=1.5), dict(ls=nan)]),
                  ('edet_focal_loss_eval', focal_bad + [dict(ls=-0.1), dict(ls=1.5)]), ('edet_box_loss', box_bad),
                  ('edet_box_loss_eval', box_bad)):
    for kw in bad:
      with pytest.raises(_lib.EdetError):
        calls[fn](**kw)
      torch.cuda.synchronize()
      for k, v in state.items():
        assert np.array_equal(bits(v), before[k]), (fn, kw, k)
  # the edges that are accepted: gamma 0, alpha 0 and 1, the widest row
  for kw in (dict(gamma=0.0), dict(alpha=0.0), dict(alpha=1.0)):
    for fn in ('edet_focal_loss', 'edet_focal_loss_smooth', 'edet_focal_loss_eval'):
      calls[fn](**kw)
  calls['edet_box_loss']()
  calls['edet_box_loss_eval']()
  torch.cuda.synchronize()
  assert bool(torch.isfinite(state['sums']).all()) and bool(torch.isfinite(state['dl'].reshape(-1)[:32].float()).all())
  assert float(state['sums'][0]) > 0 and float(state['sums'][1]) > 7.25


@gpu
@pytest.mark.parametrize('name', list(DT))
def test_no_positions_write_nothing(name):
  """positions == 0 is accepted by all five entry points: the sums (a -0.0 among them), the bias gradient and the gradient
  tensor keep their bits."""
  calls, state = loss_calls(name)
  before = {k: bits(v).copy() for k, v in state.items()}
  for fn in calls:
    calls[fn](positions=0)
  torch.cuda.synchronize()
  for k, v in state.items():
    assert np.array_equal(bits(v), before[k]), k
