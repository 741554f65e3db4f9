"""Lion in numpy float32, one rounded operation per line in the order lion/lion_tf2.py:60-74 (_resource_apply_dense) writes
them -- what edet_opt_lion_ema is held to bit for bit:

  g  = grad * f
  c  = m * b1 + g * (1 - b1)
  s  = sign(c)                        -1, 0, +1; sign(NaN) = NaN
  w' = w - lr * (s + w * wd)          from the OLD m
  m' = m * b2 + g * (1 - b2)
  ema' = ema - (1 - decay) * (ema - w')

`one_minus`: how 1 - beta is formed.  'tf2': a float32 subtraction (`1 - beta_1_t` of a float32 tensor, and the kernel's
__fsub_rn(1.f, b1)); 'torch': the Python double subtraction rounded to float32 when it meets the float32 tensor
(lion/lion_pytorch.py:79,84: `grad * (1 - beta1)`).
"""
import numpy as np

F = np.float32


def one_minus(beta, how='tf2'):
  if how == 'tf2':
    return F(1.0) - F(beta)
  if how == 'torch':
    return F(1.0 - float(beta))
  raise ValueError(how)


def interpolation(m, g, beta, how='tf2'):
  """m * beta + g * (1 - beta), three rounded operations."""
  m, g = np.asarray(m, F), np.asarray(g, F)
  return (m * F(beta) + g * one_minus(beta, how)).astype(F)


def sign(c):
  with np.errstate(invalid='ignore'):
    return np.sign(np.asarray(c, F)).astype(F)      # numpy: sign(+-0) = 0, sign(NaN) = NaN


def lion_step(w, m, grad, lr, b1=0.9, b2=0.99, wd=0.0, f=1.0, ema=None, decay=0.0, how='tf2'):
  """One step on arrays of any (equal) shape -> (w', m', ema' or None).  The inputs are not changed."""
  w, m, grad = np.asarray(w, F), np.asarray(m, F), np.asarray(grad, F)
  with np.errstate(invalid='ignore', over='ignore'):
    g = (grad * F(f)).astype(F)
    s = sign(interpolation(m, g, b1, how))
    w2 = (w - F(lr) * (s + w * F(wd))).astype(F)
    m2 = interpolation(m, g, b2, how)
    ema2 = None
    if ema is not None:
      ema = np.asarray(ema, F)
      ema2 = (ema - (F(1.0) - F(decay)) * (ema - w2)).astype(F)
  return w2, m2, ema2


def lion_arena(w, m, grad, seg_offsets, seg_flags, hyper, b1, b2, wd, seg_factor=None, ema=None, frozen_flag=2, how='tf2'):
  """lion_step over a flat arena in the kernel's segment layout: segment s = [seg_offsets[s], seg_offsets[s + 1]), its clip
  factor seg_factor[s] (None: 1), skipped when its flag has `frozen_flag`; hyper = (learning rate, EMA decay).
  -> new (w, m, ema or None)."""
  w2, m2 = np.array(w, F), np.array(m, F)
  ema2 = None if ema is None else np.array(ema, F)
  for s in range(len(seg_offsets) - 1):
    if seg_flags is not None and int(seg_flags[s]) & frozen_flag:
      continue
    a, b = int(seg_offsets[s]), int(seg_offsets[s + 1])
    f = 1.0 if seg_factor is None else seg_factor[s]
    r = lion_step(w[a:b], m[a:b], grad[a:b], hyper[0], b1, b2, wd, f, None if ema is None else ema[a:b], hyper[1], how)
    w2[a:b], m2[a:b] = r[0], r[1]
    if ema is not None:
      ema2[a:b] = r[2]
  return w2, m2, ema2
