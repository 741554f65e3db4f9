"""Float64 numpy reference of the detection losses (csrc/det_loss.hip: focal_body, box_body), with an elementwise error bound
derived from the kernels' arithmetic, and the comparator the device tests use (tests/test_gpu_detection_loss.py; the CPU
tests of this file are in tests/test_loss_ref.py).

The focal loss is written in the cancellation-free form of the kernel's own comments -- u = -x for the positive class and x
otherwise, everything a function of exp(-|u|) -- and not as the oracle writes it (oracle.efficientdet_oracle.focal_loss forms
1 - p_t, which cancels for confident logits: its float64 autograd gradient is only good to ~2e-5 relative at |x| ~ 25).  The
oracle validates this form where both are accurate (|x| <= 8); at the edges this form is the reference.

All hyper-parameters are taken as the float32 values the kernels receive (the callers pass float(np.float32(v))); the logits
and box outputs are the stored values (already rounded to bf16 for a bf16 run), so the input side is exact."""
import math
from types import SimpleNamespace

import numpy as np

U23 = 2.0 ** -23          # one ulp of a float32 in [1, 2): what the hardware transcendentals are stated to keep, relative
U24 = 2.0 ** -24          # half an ulp: one IEEE-rounded float32 operation, relative
FLT_MIN = 2.0 ** -126     # the smallest normal float32 -- and the smallest normal bfloat16
BF16_HALF_ULP = 2.0 ** -8  # round-to-nearest-even to 8 significant bits, relative
A_LOG = 2.0 ** -23        # absolute error of log(1 + ex), see focal_bound


def focal_terms(x, targets, na, nc, alpha, gamma, label_smoothing, dt=np.float64):
  """The pieces of the focal loss per element, [positions, na, nc] arrays of dtype `dt`: x [positions, na * nc] logits,
  targets [positions, na] (class index, -1 background, -2 ignored)."""
  x = np.asarray(x, dt).reshape(-1, na, nc)
  t = np.asarray(targets).reshape(-1, na, 1)
  pos = t == np.arange(nc).reshape(1, 1, nc)
  valid = np.broadcast_to(t != -2, x.shape)
  one = dt(1)
  u = np.where(pos, -x, x)
  with np.errstate(under='ignore', over='ignore'):
    ex = np.exp(-np.abs(u))                                  # in (0, 1]; 0 once it underflows
    sg = np.where(u >= 0, one / (one + ex), ex / (one + ex))      # sigmoid(u) = 1 - p_t
    omsg = np.where(u >= 0, ex / (one + ex), one / (one + ex))    # 1 - sigmoid(u), not by subtraction
    h = dt(0.5) * dt(label_smoothing)
    sp = np.logaddexp(dt(0), u) - h * u                      # cross entropy against the smoothed label; >= 0
    mod = np.power(sg, dt(gamma))                            # 0 ** 0 = 1
  af = np.where(pos, dt(alpha), one - dt(alpha))
  return SimpleNamespace(pos=pos, valid=valid, u=u, ex=ex, sg=sg, omsg=omsg, sp=sp, mod=mod, af=af, h=h, gamma=dt(gamma))


def focal_from_terms(t, inv_norm):
  """(loss, d loss / d logit) per element, [positions, na * nc]; zero at the anchors with target -2."""
  dt = t.sp.dtype.type
  with np.errstate(under='ignore'):
    w = t.af * t.mod * dt(inv_norm)
    loss = w * t.sp
    dldu = w * (t.gamma * t.omsg * t.sp + t.sg - t.h)
  grad = np.where(t.pos, -dldu, dldu)
  p = t.sp.shape[0]
  return np.where(t.valid, loss, 0).reshape(p, -1), np.where(t.valid, grad, 0).reshape(p, -1)


def focal_ref(x, targets, na, nc, alpha, gamma, label_smoothing, inv_norm, dt=np.float64):
  """loss = af sg^gamma sp inv_norm, d loss / du = af sg^gamma (gamma (1 - sg) sp + sg - h) inv_norm, the sign flipped for
  the positive class; af = alpha for the positive class, else 1 - alpha; h = label_smoothing / 2."""
  return focal_from_terms(focal_terms(x, targets, na, nc, alpha, gamma, label_smoothing, dt), inv_norm)


def focal_bound(x, targets, na, nc, alpha, gamma, label_smoothing, inv_norm, storage):
  """(loss bound, gradient bound) per element, [positions, na * nc] float64: how far the kernel's float32 value of an element
  may be from focal_ref, term by term from focal_body.  storage: 'f32' or 'bf16' (the gradient's; the loss is always float32).

  The kernel, per element (float32; a hardware transcendental is taken at its stated 1 ulp = 2^-23 relative, an IEEE
  operation at half an ulp = 2^-24):
    a   = -1.44269504f |u|             constant 2^-24 + multiply 2^-24: exp2 turns a relative error d of its argument into
                                        |a| ln 2 d = |u| d, so                            e_arg = |u| 2^-23
    ex  = v_exp(a)                                                                        e_ex  = e_arg + 2^-23
          where exp(-|u|) < 2^-126 (|u| > 87.3) the instruction returns 0, not a denormal: the flush terms below
    inv = v_rcp(1 + ex)                 add 2^-24, rcp 2^-23, ex's error scaled by q = ex / (1 + ex):
                                                                                          e_inv = 1.5 2^-23 + q e_ex
    sg  = u >= 0 ? inv : ex inv                                                           e_sg  = e_inv  or  e_ex + e_inv + 2^-24
    mod = sg^gamma  (pow, 2^-23)  or  sg v_sqrt(sg)  (sqrt 2^-23, multiply 2^-24; gamma == 1.5):
                                                                                          e_mod = gamma e_sg + 2^-23 (+ 2^-24)
          -- the argument error of exp2 grows with |u| and reaches the gradient (1 + gamma)-fold, through sg^gamma and sg
    L   = 0.69314718f v_log(1 + ex)     1 + ex is rounded to float32 in [1, 2]: absolute 2^-24 on the argument, the same on
          its logarithm (d ln y = dy / y); v_log's 1 ulp is of a result whose spacing near 1 is far finer than its
          argument's, so as much again is allowed for it: A_LOG = 2^-23 ABSOLUTE.  Relative: log 2^-23, constant 2^-24,
          multiply 2^-24, and ex's own error:                                             d_L = A_LOG + 2 2^-23 L + q e_ex
    sp  = fmax(u, 0) + L, then fma(-h, u, .) with smoothing: one rounding each            d_sp = d_L + 2^-24 sp (+ 2^-24 sp)
    w   = af mod inv_norm               1 - alpha 2^-24, two multiplies
    loss: fma(w, sp, acc) 2^-24.  K0 = pow 1 + (af 1/2 + two multiplies 1 + fma 1/2) = 3 units of 2^-23
          loss bound = loss (e_mod + 2 2^-23) + w d_sp
          The log term enters the loss as af sg^gamma A_LOG inv_norm.
    1 - sg by subtraction: absolute sg e_sg + 2^-24 (1 - sg)
    B   = fma(gamma (1 - sg), sp, sg - h):  the multiply gamma (1 - sg) 2^-24, the subtraction sg - h 2^-24 (smoothing only),
          the fma 2^-24:
          d_B = gamma sp (sg e_sg + 2^-24 (1 - sg)) + 2^-24 T1 + gamma (1 - sg) d_sp + sg e_sg + 2^-24 |sg - h| + 2^-24 |B|
          The log term enters the gradient as af sg^gamma gamma (1 - sg) A_LOG inv_norm.
    g   = w B                           one more multiply.  K0 = pow 1 + (af 1/2 + three multiplies 3/2) = 3 units of 2^-23
          gradient bound = |g| (e_mod + 2 2^-23) + w d_B
  With smoothing B has a zero crossing (sg - h < 0 < gamma (1 - sg) sp), so d_B is absolute in the magnitudes of B's terms;
  without smoothing every term of B is positive and the bound is relative to |g| (plus the log term).
  Underflow: sg^gamma, w and the result itself may fall below 2^-126 and be flushed: 2^-126 (1 + 2 af inv_norm |B|mag).
  Flush of ex, u < 0: the kernel's sg is anywhere in [0, sg]: |mod B - mod' B'| <= [gamma > 0] mod |B| + mod (gamma sg (2 + sp)
  + sg); the loss moves by at most [gamma > 0] loss + 2 w sg.  u >= 0: e_ex = 1 in the terms above (everything depends on ex
  through q <= ex).
  bf16 storage: the gradient is rounded once more, 2^-8 of the computed value; the floor 2^-126 is bf16's smallest normal too."""
  assert storage in ('f32', 'bf16')
  t = focal_terms(x, targets, na, nc, alpha, gamma, label_smoothing)
  g15 = np.float32(gamma) == np.float32(1.5)
  with np.errstate(under='ignore', over='ignore', invalid='ignore'):
    au = np.abs(t.u)
    e_ex = au * U23 + U23
    flush = t.ex * (1.0 - 2.0 * e_ex) < FLT_MIN
    e_ex = np.where(flush & (t.u >= 0), 1.0, e_ex)
    q = t.ex / (1.0 + t.ex)
    e_inv = 1.5 * U23 + q * e_ex
    e_sg = np.where(t.u >= 0, e_inv, e_ex + e_inv + U24)
    e_mod = gamma * e_sg + U23 + (U24 if g15 else 0.0)
    lg = np.log1p(t.ex)
    d_l = A_LOG + 2.0 * U23 * lg + q * e_ex
    d_sp = d_l + U24 * t.sp * (2.0 if label_smoothing else 1.0)
    w = t.af * t.mod * inv_norm
    loss = w * t.sp
    t1 = gamma * t.omsg * t.sp
    b = t1 + t.sg - t.h
    bmag = t1 + t.sg + t.h
    d_b = (gamma * t.sp * (t.sg * e_sg + U24 * t.omsg) + U24 * t1 + gamma * t.omsg * d_sp + t.sg * e_sg +
           (U24 * np.abs(t.sg - t.h) if label_smoothing else 0.0) + U24 * np.abs(b))
    lb = loss * (e_mod + 2.0 * U23) + w * d_sp + FLT_MIN * (1.0 + 2.0 * t.af * inv_norm * t.sp)
    gb = w * np.abs(b) * (e_mod + 2.0 * U23) + w * d_b + FLT_MIN * (1.0 + 2.0 * t.af * inv_norm * bmag)
    neg = flush & (t.u < 0)
    some = 1.0 if gamma > 0 else 0.0
    lb = lb + np.where(neg, some * loss + 2.0 * w * t.sg, 0.0)
    gb = gb + np.where(neg, some * w * np.abs(b) + w * (gamma * t.sg * (2.0 + t.sp) + t.sg), 0.0)
    if storage == 'bf16':
      gb = gb + BF16_HALF_ULP * (w * np.abs(b) + gb)
  p = t.sp.shape[0]
  return np.where(t.valid, lb, 0.0).reshape(p, -1), np.where(t.valid, gb, 0.0).reshape(p, -1)


def focal_scale(x, targets, na, nc, alpha, gamma, label_smoothing, inv_norm):
  """What the non-vacuity rule measures the bounds against: (loss, af sg^gamma (gamma (1 - sg) sp + sg + h) inv_norm -- |g|
  without smoothing, the magnitude of its terms with --, the log term of the loss bound, the log term of the gradient bound)."""
  t = focal_terms(x, targets, na, nc, alpha, gamma, label_smoothing)
  w = t.af * t.mod * inv_norm
  p = t.sp.shape[0]
  out = (w * t.sp, w * (gamma * t.omsg * t.sp + t.sg + t.h), w * A_LOG, w * gamma * t.omsg * A_LOG)
  return tuple(np.where(t.valid, a, 0.0).reshape(p, -1) for a in out)


def box_ref(x, t, delta, inv_norm, grad_scale):
  """Huber loss on x - t where t != 0 (a target of -0.0 is masked too, as tf.not_equal(t, 0.0) masks it): (loss, gradient) per
  element, float64.  The loss carries inv_norm alone, the gradient inv_norm * grad_scale: the kernel's convention."""
  x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
  mask = t != 0
  err = x - t
  ae = np.abs(err)
  quad = ae <= delta
  loss = np.where(quad, 0.5 * err * err, delta * ae - 0.5 * delta * delta) * inv_norm
  grad = np.where(quad, err, np.sign(err) * delta) * inv_norm * grad_scale
  return np.where(mask, loss, 0.0), np.where(mask, grad, 0.0)


def box_bound(x, t, delta, inv_norm, grad_scale, storage):
  """(loss bound, gradient bound) per element from box_body's float32 arithmetic, every operation IEEE (2^-24 relative):
    err = x - t                          one rounding; |err| <= delta is then decided on the rounded value, and the Huber
                                         loss and its gradient are continuous there, so a branch taken the other way costs
                                         no more than that rounding
    quadratic: 0.5 err err inv_norm      err twice + two multiplies (0.5 x is exact): 4 2^-24 of the loss
    linear:    (delta ae - 0.5 delta delta) inv_norm: delta ae 2 2^-24 (err + multiply), 0.5 delta delta 2^-24, absolute
               in those terms (they cancel down to >= half of delta ae), then the subtraction and the multiply: 2 2^-24
    gradient:  (err or +-delta) inv_norm grad_scale: err + two multiplies, K0 = 3 units of 2^-24
  2^-126 for a flushed result; bf16 storage: 2^-8 of the computed gradient."""
  assert storage in ('f32', 'bf16')
  loss, grad = box_ref(x, t, delta, inv_norm, grad_scale)
  ae = np.abs(np.asarray(x, np.float64) - np.asarray(t, np.float64))
  lin = inv_norm * (delta * ae * 2.0 * U24 + 0.5 * delta * delta * U24) + 2.0 * U24 * loss
  lb = np.where(ae <= delta, 4.0 * U24 * loss, lin) + FLT_MIN
  gb = 3.0 * U24 * np.abs(grad) + FLT_MIN
  if storage == 'bf16':
    gb = gb + BF16_HALF_ULP * (np.abs(grad) + gb)
  mask = np.asarray(t) != 0
  return np.where(mask, lb, 0.0), np.where(mask, gb, 0.0)


# ------------------------------------------------------------------------------------------------------- the comparator
def worst_ratio(got, want, bound):
  """max over the elements of |got - want| / bound (0 / 0 = 0); inf when a value of `got` is not finite or an element with a
  zero bound differs."""
  got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
  assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
  if got.size == 0:
    return 0.0
  if not np.isfinite(got).all():
    return math.inf
  err = np.abs(got - want)
  with np.errstate(divide='ignore', invalid='ignore'):
    r = np.where(err == 0, 0.0, err / bound)
  return float(r.max())


def assert_within(got, want, bound, what):
  """Every element of `got` within its own bound of `want`, none excluded -> the largest err / bound."""
  r = worst_ratio(got, want, bound)
  if not r <= 1.0:
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    with np.errstate(divide='ignore', invalid='ignore'):
      i = np.unravel_index(int(np.nanargmax(np.where(np.isfinite(got), np.abs(got - want) / bound, np.inf))), got.shape)
    raise AssertionError('%s: err / bound = %.3g at %s: got %r, want %r, bound %.3g' % (what, r, i, got[i], want[i], bound[i]))
  return r


def column_sums(a):
  """Exactly rounded column sums (math.fsum) of a [rows, columns] float64 array."""
  a = np.asarray(a, np.float64)
  return np.asarray([math.fsum(a[:, j].tolist()) for j in range(a.shape[1])], np.float64)


def sum_bound(terms, bounds, count):
  """Bound of a float32 sum, in any order, of `count` computed terms whose elementwise bounds are `bounds`: the sum of the
  bounds plus count 2^-24 sum |term| (first order; for non-negative terms sum |term| is the sum itself)."""
  return math.fsum(np.asarray(bounds, np.float64).ravel().tolist()) + count * U24 * math.fsum(np.abs(np.asarray(terms, np.float64)).ravel().tolist())
