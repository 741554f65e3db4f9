"""Generates tests/golden/reference_lion.npz by EXECUTING the reference's two dense Lion implementations, unmodified:

  * lion/lion_tf2.py on the torch-backed `tf` stand-in (mini_keras.build_tf) plus the small
    keras.optimizers.legacy.Optimizer base below -- _set_hyper / _get_hyper, add_slot / get_slot, _prepare_local giving a
    float32 `lr_t`, apply_gradients calling _resource_apply_dense per variable -- with tf.function a pass-through,
    tf.math.sign torch.sign and tf.control_dependencies an empty context;
  * lion/lion_pytorch.py on the installed torch, on the CPU.

Cases: three variables of shapes (7,), (5, 3), (1,), four steps with a different learning rate each, for the hyper-parameter
sets (beta_1 .9, beta_2 .99, wd 0) and (.95, .98, 0.1).  Some gradient elements are exactly zero on step one (m = 0 there, so
c = 0 and sign(0) = 0 is exercised).  The gradients are chosen -- and checked here, on both runs -- so that every
c = m beta_1 + g (1 - beta_1) is exactly 0 or at least 1e-3 of the largest |g| of its tensor: no rounding difference between
two implementations can flip a sign, on about half of the later elements with the momentum deciding the sign against the
gradient; and so that no new slot value is a cancellation of its two terms (inputs, check_step).  Only inputs and results are
recorded.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_lion.py
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mini_keras   # noqa
from mini_keras import T, ns   # noqa

REF = '/root/reference/lion'
F = np.float32
SHAPES = [(7,), (5, 3), (1,)]
STEPS = 4
LRS = [1e-3, 3e-4, 2e-3, 1e-4]
HYPERS = [(0.9, 0.99, 0.0), (0.95, 0.98, 0.1)]      # beta_1, beta_2, wd
MARGIN = 1e-3


class _DType(object):
  def __init__(self, base):
    self.base_dtype = base


class Variable(object):
  """A resource variable as _resource_apply_dense uses one: device, dtype.base_dtype, value arithmetic, assign, assign_sub."""
  device = 'cpu'

  def __init__(self, value):
    self.value = T(torch.from_numpy(np.array(value, F)))
    self.dtype = _DType(torch.float32)

  def __mul__(self, other):
    return self.value * other
  __rmul__ = __mul__

  def assign(self, value):
    self.value = T(value.clone())
    return self

  def assign_sub(self, delta):
    self.value = T(self.value - delta)
    return self

  def numpy(self):
    return self.value.numpy().copy()


class Optimizer(object):
  """What lion_tf2.Lion needs of tf.keras.optimizers.legacy.Optimizer (optimizer_v2.py): hyper-parameters by name, zero
  slots per variable, and apply_gradients = _create_slots once, _prepare_local once per (device, dtype), then
  _resource_apply_dense per variable."""

  def __init__(self, name, **kwargs):
    self._name, self._hyper, self._slots, self._slots_made = name, {}, {}, False

  def _set_hyper(self, name, value):
    self._hyper[name] = value

  def _get_hyper(self, name, dtype=None):
    value = self._hyper[name]
    return T(torch.tensor(value() if callable(value) else value, dtype=dtype or torch.float32))

  def add_slot(self, var, slot_name, initializer='zeros'):
    assert initializer == 'zeros'
    self._slots.setdefault(id(var), {}).setdefault(slot_name, Variable(np.zeros(tuple(var.value.shape), F)))
    return self._slots[id(var)][slot_name]

  def get_slot(self, var, slot_name):
    return self._slots[id(var)][slot_name]

  def _prepare_local(self, var_device, var_dtype, apply_state):
    apply_state[(var_device, var_dtype)]['lr_t'] = self._get_hyper('learning_rate', var_dtype)      # no decay schedule here

  def _fallback_apply_state(self, var_device, var_dtype):
    apply_state = {(var_device, var_dtype): {}}
    self._prepare_local(var_device, var_dtype, apply_state)
    return apply_state[(var_device, var_dtype)]

  def apply_gradients(self, grads_and_vars):
    grads_and_vars = list(grads_and_vars)
    if not self._slots_made:
      self._create_slots([v for _, v in grads_and_vars])
      self._slots_made = True
    apply_state = {}
    for _, v in grads_and_vars:
      key = (v.device, v.dtype.base_dtype)
      if key not in apply_state:
        apply_state[key] = {}
        self._prepare_local(key[0], key[1], apply_state)
    for g, v in grads_and_vars:
      self._resource_apply_dense(g, v, apply_state=apply_state)


def build_tf():
  tf = mini_keras.build_tf()

  def function(fn=None, **kwargs):
    return fn if fn is not None else (lambda f: f)
  tf.function = function
  tf.math = ns('math', sign=torch.sign)
  tf.control_dependencies = lambda deps: contextlib.nullcontext()
  tf.keras.optimizers = ns('optimizers', legacy=ns('legacy', Optimizer=Optimizer))
  return tf


def inputs(seed, b2):
  """-> (w0 [3 arrays], grads [STEPS][3 arrays]).  Step one: magnitudes in [0.5, 1], random signs, two exact zeros in each of
  the two larger tensors.  Later steps, per element, one of two kinds at random:
    large  magnitude in [0.5, 1] with the sign of the element's momentum (a random sign where that is still 0);
    small  magnitude in [0.005, 0.02] AGAINST the momentum -- so that the momentum, not the gradient, decides sign(c): m b1
           outweighs g (1 - b1) about twice or more for both hyper-parameter sets (|m| stays above 0.4 (1 - b2)).
  Either way the two terms of m' = m b2 + g (1 - b2) do not cancel (same sign, or one at most a tenth of the other): a
  slot value that is the small difference of two terms would show one implementation's rounding of a term as many ulp of
  the result and say nothing about either implementation.  The momentum's sign is followed in double here; check_step holds
  both executed runs to what this construction promises."""
  rng = np.random.default_rng(seed)
  w0 = [rng.standard_normal(s).astype(F) for s in SHAPES]
  grads, m = [], [np.zeros(s) for s in SHAPES]
  for t in range(STEPS):
    row = []
    for v, s in enumerate(SHAPES):
      large = rng.uniform(0.5, 1.0, s)
      small = rng.uniform(0.005, 0.02, s)
      coin, sign = rng.random(s) < 0.5, rng.choice([-1.0, 1.0], s)
      toward = np.where(m[v] != 0, np.sign(m[v]), sign)
      g = np.where((m[v] == 0) | coin, large * toward, -small * toward).astype(F)
      if t == 0 and g.size > 1:
        g.reshape(-1)[[1, g.size - 2]] = 0.0
      m[v] = m[v] * b2 + g.astype(np.float64) * (1.0 - b2)
      row.append(g)
    grads.append(row)
  assert all((grads[0][v] == 0).sum() == 2 for v in (0, 1))
  return w0, grads


def check_step(m, g, b1, b2, what):
  """What inputs() promises of a step, asserted on an executed run's own slot values (in double: the conditions are about
  the values, not about a rounding): every c = m b1 + g (1 - b1) is exactly 0 or at least MARGIN * max|g|, so that no
  rounding difference flips a sign; every m' = m b2 + g (1 - b2) is at least half its larger term.
  -> (exact zeros among the c, elements whose sign(c) is against their gradient's)."""
  m, g = np.asarray(m, np.float64), np.asarray(g, np.float64)
  c = m * b1 + g * (1.0 - b1)
  bound = MARGIN * np.abs(g).max()
  small = (c != 0) & (np.abs(c) < bound)
  assert not small.any(), (what, 'c', c[small], bound)
  m2 = m * b2 + g * (1.0 - b2)
  cancelled = np.abs(m2) < 0.5 * np.maximum(np.abs(m * b2), np.abs(g * (1.0 - b2)))
  assert not cancelled.any(), (what, 'm', m2[cancelled])
  return int((c == 0).sum()), int((np.sign(c) * np.sign(g) < 0).sum())


def run_tf2(lion_tf2, w0, grads, b1, b2, wd):
  opt = lion_tf2.Lion(learning_rate=LRS[0], beta_1=b1, beta_2=b2, wd=wd)
  variables = [Variable(w) for w in w0]
  out, zeros, against = [], 0, 0
  for t in range(STEPS):
    opt._set_hyper('learning_rate', LRS[t])
    for v, g in zip(variables, grads[t]):
      z, a = check_step(opt.get_slot(v, 'm').numpy() if t else np.zeros_like(g), g, b1, b2, ('tf2', t))
      zeros, against = zeros + z, against + a
    opt.apply_gradients([(T(torch.from_numpy(g.copy())), v) for g, v in zip(grads[t], variables)])
    out.append(([v.numpy() for v in variables], [opt.get_slot(v, 'm').numpy() for v in variables]))
  assert zeros == 4, zeros          # sign(0) = 0 was exercised
  assert against >= 10, against     # and so was the momentum deciding the sign against the gradient
  return out


def run_torch(lion_pytorch, w0, grads, b1, b2, wd):
  params = [torch.nn.Parameter(torch.from_numpy(w.copy())) for w in w0]
  opt = lion_pytorch.Lion(params, lr=LRS[0], betas=(b1, b2), weight_decay=wd)
  out = []
  for t in range(STEPS):
    for group in opt.param_groups:
      group['lr'] = LRS[t]
    for p, g in zip(params, grads[t]):
      check_step(opt.state[p]['exp_avg'].numpy() if t else np.zeros_like(g), g, b1, b2, ('torch', t))
      p.grad = torch.from_numpy(g.copy())
    opt.step()
    out.append(([p.detach().numpy().copy() for p in params], [opt.state[p]['exp_avg'].numpy().copy() for p in params]))
  return out


def main():
  sys.path.insert(0, REF)
  import lion_pytorch     # noqa: the reference modules
  # torch.optim imports half of torch on its first use, which must not meet the stand-in modules: one throw-away step first
  warm = torch.nn.Parameter(torch.zeros(1))
  warm.grad = torch.ones(1)
  lion_pytorch.Lion([warm]).step()
  mini_keras.install(build_tf())
  import lion_tf2         # noqa
  for mod in (lion_tf2, lion_pytorch):
    assert mod.__file__.startswith(REF), mod.__file__
  out = {'shapes': np.asarray([str(s) for s in SHAPES]), 'steps': np.int32(STEPS), 'margin': np.float64(MARGIN)}
  for h, (b1, b2, wd) in enumerate(HYPERS):
    w0, grads = inputs(100 + h, b2)
    runs = (('tf2', run_tf2(lion_tf2, w0, grads, b1, b2, wd)), ('torch', run_torch(lion_pytorch, w0, grads, b1, b2, wd)))
    out['h%d/hyper' % h] = np.asarray([b1, b2, wd], np.float64)
    out['h%d/lr' % h] = np.asarray(LRS, np.float64)
    for v, w in enumerate(w0):
      out['h%d/w0_%d' % (h, v)] = w
    for t in range(STEPS):
      for v, g in enumerate(grads[t]):
        out['h%d/g_%d_%d' % (h, t, v)] = g
    for who, res in runs:
      for t, (ws, ms) in enumerate(res):
        for v in range(len(SHAPES)):
          assert ws[v].dtype == F and ms[v].dtype == F and ws[v].shape == SHAPES[v] == ms[v].shape
          out['h%d/%s/w_%d_%d' % (h, who, t, v)] = ws[v]
          out['h%d/%s/m_%d_%d' % (h, who, t, v)] = ms[v]
  path = os.path.join(HERE, 'reference_lion.npz')
  np.savez_compressed(path, **out)
  print(path, len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
