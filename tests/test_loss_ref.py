"""CPU tests of tests/loss_ref.py: the closed form against the oracle's autograd where both are accurate, the error bounds
against their non-vacuity rule, and a mutation check of the comparator that tests/test_gpu_detection_loss.py applies to the
kernels (loss_ref.assert_within on the gradient of every element and on the loss of every element)."""
import numpy as np
import pytest
import torch

from oracle import efficientdet_oracle as orc
from tests import loss_ref as lr

GAMMAS = (0.0, 0.5, 1.0, 1.5, 2.0, 2.5)
ALPHAS = (0.25, 0.6)
SMOOTHINGS = (0.0, 0.1)
NA, NC, POSITIONS, NORM = 3, 8, 96, 37.0


def f32(v):
  return float(np.float32(v))


def problem(limit, seed=3, dt=np.float32):
  """N(0, 2^2) logits clipped to |x| <= limit with the limits themselves planted, float32 values; targets with positives,
  background and ignored anchors, every pair of neighbouring anchors different somewhere."""
  rng = np.random.default_rng(seed)
  x = np.clip(rng.standard_normal((POSITIONS, NA * NC)) * 2.0, -limit, limit).astype(dt)
  x[0, :8] = [limit, -limit, 0.0, 1e-3, -1e-3, limit / 2, -limit / 2, 1.0]
  x[1, :8] = x[0, :8]
  t = rng.integers(0, NC, (POSITIONS, NA)).astype(np.int32)
  r = rng.random((POSITIONS, NA))
  t[r < 0.5] = -1
  t[r < 0.15] = -2
  t[0], t[1] = [0, -1, 1], [-1, 1, -2]      # the planted values on a positive (class 0 and 1), on negatives, next to an ignored one
  return x.astype(np.float64), t


def oracle_focal(x, t, alpha, gamma, smoothing):
  xq = torch.from_numpy(x).double().requires_grad_(True)
  tt = torch.from_numpy(t)
  onehot = torch.nn.functional.one_hot(torch.clamp(tt, min=0).long(), NC).double() * (tt >= 0).unsqueeze(-1)
  fl = orc.focal_loss(xq, onehot.reshape(POSITIONS, -1), alpha, gamma, NORM, smoothing).reshape(POSITIONS, NA, NC)
  fl = fl * (tt != -2).unsqueeze(-1)
  fl.sum().backward()
  return fl.detach().reshape(POSITIONS, -1).numpy(), xq.grad.numpy()


@pytest.mark.parametrize('smoothing', SMOOTHINGS)
@pytest.mark.parametrize('alpha', ALPHAS)
@pytest.mark.parametrize('gamma', GAMMAS)
def test_focal_ref_equals_the_oracle_where_both_are_accurate(gamma, alpha, smoothing):
  """|x| <= 8, float64 on both sides.  The difference is taken relative to af sg^gamma (gamma (1 - sg) sp + sg + h) / norm,
  which is |gradient| without smoothing (with it the gradient has a zero crossing in u, where no relative figure exists).
  Measured worst over the 24 cases: gradient 8.82e-13, loss 7.93e-13 (both at gamma 2.5; they grow with gamma: the oracle
  raises a 1 - p_t that has lost 3 to 4 digits at x = -8 to that power), orders below its 2e-5 at |x| ~ 25.  The tolerance is
  ten times that."""
  x, t = problem(8.0)
  loss, grad = lr.focal_ref(x, t, NA, NC, alpha, gamma, smoothing, 1.0 / NORM)
  want_loss, want_grad = oracle_focal(x, t, alpha, gamma, smoothing)
  _, gmag, _, _ = lr.focal_scale(x, t, NA, NC, alpha, gamma, smoothing, 1.0 / NORM)
  valid = gmag > 0
  assert valid.sum() > 0.8 * valid.size and np.array_equal(loss == 0, ~valid) and not grad[~valid].any()
  dg = float((np.abs(grad - want_grad)[valid] / gmag[valid]).max())
  dl = float((np.abs(loss - want_loss)[valid] / loss[valid]).max())
  print('focal_ref against the oracle: gamma %g alpha %g smoothing %g: gradient %.3g, loss %.3g' % (gamma, alpha, smoothing, dg, dl))
  assert dg <= 8.82e-12 and dl <= 7.93e-12
  assert not want_grad[~valid].any()


@pytest.mark.parametrize('delta', [0.05, 0.125, 1.0])
def test_box_ref_equals_the_oracle(delta):
  """orc.huber with autograd, float64; masked targets 0.0 and -0.0; errors at +-delta exactly (delta 0.125), where the
  branches meet.  Both sides are a handful of float64 operations: 1e-15 relative."""
  rng = np.random.default_rng(4)
  t = (rng.standard_normal((40, 12)) * 0.2).astype(np.float32).astype(np.float64)
  t[rng.random(t.shape) < 0.4] = 0.0
  t[0, :2] = [-0.0, 0.0]
  x = rng.standard_normal(t.shape) * 0.3
  t[1, :4], x[1, :4] = [1.0, 1.0, -1.0, 0.5], [1.0 + delta, 1.0 - delta, -1.0 + delta, 1e4]
  loss, grad = lr.box_ref(x, t, delta, 1.0 / (4 * NORM), 50.0)
  xq = torch.from_numpy(x).requires_grad_(True)
  tt = torch.from_numpy(t)
  ol = orc.huber(xq - tt, delta) * (tt != 0).double() / (4 * NORM)
  (50.0 * ol.sum()).backward()
  assert not loss[0, :2].any() and not grad[0, :2].any() and (np.signbit(t[0, 0]) and t[0, 0] == 0)
  np.testing.assert_allclose(loss, ol.detach().numpy(), rtol=1e-15, atol=0)
  np.testing.assert_allclose(grad, xq.grad.numpy(), rtol=1e-15, atol=0)
  assert abs(grad[1, 0]) == pytest.approx(delta * 50.0 / (4 * NORM), rel=1e-15) and loss[1, 3] > 0


@pytest.mark.parametrize('smoothing', SMOOTHINGS)
@pytest.mark.parametrize('gamma', GAMMAS)
def test_fp32_focal_bound_is_not_vacuous(gamma, smoothing):
  """float32 storage, |u| <= 20: the bounds stay below 1e-4 of the value plus the log(1 + ex) term (and the 2^-126 floor).
  For the gradient under smoothing the value is replaced by the magnitude of its terms (loss_ref.focal_scale): the bracket
  gamma (1 - sg) sp + sg - h crosses zero there, and no float32 evaluation keeps a bound relative to a difference that
  cancels."""
  for alpha in ALPHAS:
    x, t = problem(20.0)
    args = (x, t, NA, NC, f32(alpha), gamma, f32(smoothing), f32(1.0 / NORM))
    lb, gb = lr.focal_bound(*args, 'f32')
    loss, gmag, llog, glog = lr.focal_scale(*args)
    _, grad = lr.focal_ref(*args)
    if not smoothing:
      np.testing.assert_allclose(gmag, np.abs(grad), rtol=1e-12, atol=0)
    floor = 1e-36
    assert (lb <= 1e-4 * loss + llog + floor).all() and (gb <= 1e-4 * gmag + glog + floor).all()
    valid = gmag > 0
    print('bound / value at |u| <= 20: gamma %g smoothing %g alpha %g: loss %.3g, gradient %.3g' % (
        gamma, smoothing, alpha, float(((lb - llog)[valid] / loss[valid]).max()), float(((gb - glog)[valid] / gmag[valid]).max())))
    assert (lb[valid] >= 3 * lr.U23 * loss[valid]).all() and (gb[valid] >= 3 * lr.U23 * np.abs(grad)[valid]).all()      # K0


def neighbour_target(t):
  """One anchor's target taken from the anchor next to it, at the first place where that changes a class or a background."""
  t = t.copy()
  for p in range(t.shape[0]):
    for a in range(NA - 1):
      if t[p, a] != t[p, a + 1] and t[p, a] >= -1 and t[p, a + 1] >= -1:
        t[p, a] = t[p, a + 1]
        return t
  raise AssertionError('no such pair')


def mutants(x, t, na, nc, alpha, gamma, smoothing, inv):
  """name -> (loss, gradient) of a subtly wrong focal loss; a mutant that IS the loss at these hyper-parameters is left out:
  the (1 - sg) factor multiplies gamma (nothing at gamma 0), gamma -> 1.5 is the identity at 1.5, h is 0 without smoothing."""
  def terms():
    return lr.focal_terms(x, t, NA, NC, alpha, gamma, smoothing)
  out = {'alpha swapped': lr.focal_ref(x, t, NA, NC, 1.0 - alpha, gamma, smoothing, inv),
         "a neighbour's target": lr.focal_ref(x, neighbour_target(t), NA, NC, alpha, gamma, smoothing, inv)}
  if gamma != 0:
    m = terms()
    m.omsg = np.ones_like(m.omsg)
    out['(1 - sg) dropped'] = lr.focal_from_terms(m, inv)
  if gamma != 1.5:
    out['gamma 1.5'] = lr.focal_ref(x, t, NA, NC, alpha, 1.5, smoothing, inv)
  if smoothing:
    m = terms()
    loss, _ = lr.focal_from_terms(m, inv)
    m.h = 0.0 * m.h
    out['sg instead of sg - h'] = (loss, lr.focal_from_terms(m, inv)[1])
    m = terms()
    m.sp = m.sp + m.h * m.u
    out['sp without -h u'] = lr.focal_from_terms(m, inv)
  return out


@pytest.mark.parametrize('storage', ['f32', 'bf16'])
@pytest.mark.parametrize('smoothing', SMOOTHINGS)
@pytest.mark.parametrize('gamma', GAMMAS)
def test_comparator_rejects_the_mutants_and_accepts_float32(gamma, smoothing, storage):
  """The elementwise checks of the device tests -- assert_within on every gradient and on every loss -- accept focal_ref
  evaluated in float32 numpy and reject every mutant cast to float32 (for bf16 storage: the gradient rounded to bf16)."""
  x, t = problem(20.0)
  if storage == 'bf16':
    x = torch.from_numpy(x).to(torch.bfloat16).double().numpy()
  store = (lambda g: torch.from_numpy(g.astype(np.float32)).to(torch.bfloat16).double().numpy()) if storage == 'bf16' else (
      lambda g: g.astype(np.float32))
  for alpha in ALPHAS:
    args = (x, t, NA, NC, f32(alpha), gamma, f32(smoothing), f32(1.0 / NORM))
    want_loss, want_grad = lr.focal_ref(*args)
    lb, gb = lr.focal_bound(*args, storage)
    loss32, grad32 = lr.focal_ref(*args, dt=np.float32)
    assert loss32.dtype == grad32.dtype == np.float32
    rl, rg = lr.assert_within(loss32, want_loss, lb, 'float32 loss'), lr.assert_within(store(grad32), want_grad, gb, 'float32 gradient')
    print('float32 numpy, %s gamma %g smoothing %g alpha %g: err / bound loss %.3f gradient %.3f' % (storage, gamma, smoothing, alpha, rl, rg))
    found = mutants(*args)
    assert len(found) == 2 + (gamma != 0) + (gamma != 1.5) + 2 * bool(smoothing)
    for name, (ml, mg) in found.items():
      rejected = 0
      for got, want, bound in ((store(mg), want_grad, gb), (ml.astype(np.float32), want_loss, lb)):
        try:
          lr.assert_within(got, want, bound, name)
        except AssertionError:
          rejected += 1
      assert rejected, 'the comparator accepts the mutant %r (gamma %g, smoothing %g, alpha %g, %s)' % (name, gamma, smoothing, alpha, storage)
      if name != 'sp without -h u' or gamma != 0:      # (at gamma 0 the cross entropy is not in the gradient: the loss check finds it)
        with pytest.raises(AssertionError):
          lr.assert_within(store(mg), want_grad, gb, name)


def test_comparator_refuses_non_finite_values_and_zero_bounds():
  want, bound = np.asarray([1.0, 0.0]), np.asarray([0.5, 0.0])
  assert lr.worst_ratio([1.25, 0.0], want, bound) == 0.5
  assert lr.worst_ratio([1.0, 1e-300], want, bound) == np.inf and lr.worst_ratio([np.nan, 0.0], want, bound) == np.inf
  for bad in ([1.0, 1e-300], [np.nan, 0.0], [np.inf, 0.0], [1.6, 0.0]):
    with pytest.raises(AssertionError):
      lr.assert_within(bad, want, bound, 'x')


def test_box_bound_is_a_few_roundings():
  rng = np.random.default_rng(6)
  t = (rng.standard_normal((30, 8)) * 0.2).astype(np.float32).astype(np.float64)
  x = (rng.standard_normal((30, 8)) * 0.3).astype(np.float32).astype(np.float64)
  t[0, 0] = -0.0
  loss, grad = lr.box_ref(x, t, f32(0.1), f32(1 / 148.0), 50.0)
  lb, gb = lr.box_bound(x, t, f32(0.1), f32(1 / 148.0), 50.0, 'f32')
  assert lb[0, 0] == 0 and gb[0, 0] == 0
  m = t != 0
  assert (gb[m] <= 4 * lr.U24 * np.abs(grad[m])).all() and (lb[m] <= 8 * lr.U24 * loss[m] + 1e-37).all()
  x32, t32 = x.astype(np.float32), t.astype(np.float32)
  e = x32 - t32
  g32 = np.where(np.abs(e) <= np.float32(0.1), e, np.sign(e) * np.float32(0.1)) * np.float32(1 / 148.0) * np.float32(50.0)
  lr.assert_within(np.where(m, g32, 0), grad, gb, 'float32 Huber gradient')
  with pytest.raises(AssertionError):
    lr.assert_within(np.where(m, g32 * np.float32(1.000001), 0), grad, gb, 'scaled by 1 + 1e-6')
