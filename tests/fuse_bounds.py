"""What tests/test_gpu_fuse_exact.py (device) and tests/test_fuse_bounds.py (CPU) share for the BiFPN fusion kernels
(automl_amd/csrc/fuse.hip): a float64 / numpy reference of one fusion node written with plain indexing (so that the tie
rule of the pool is stated here and not inherited from a library), exact-integer problems on which nothing is rounded,
real-valued swish problems with componentwise bounds, a float32 restatement of edet_fuse_bwd_input, the normalisers of
the fusion variables, and the measured ulp budgets.  Nothing here touches the device.

Conventions of the reference (those the kernels document):
  view         v = float32(x * scale + shift): evaluated in float64 and rounded once -- the kernel's fmaf
  up-sample    nearest, source index min((o * in) // out, in - 1)
  max-pool     3x3, stride 2, TF 'SAME'; padding is excluded, never a candidate
  pool winner  the FIRST maximum of the row-major scan over the taps inside the image, reported as ky * 3 + kx
               (efficientdet_keras.py:254-263 delegates to TF's MaxPoolGrad, whose CPU kernel does the same)
  weights      the normalised weights are an INPUT of the node ([nin][wc], wc = 1 or c)
  gradients    with respect to the BatchNorm OUTPUT (the view), as edet_fuse_bwd_input returns them
  ReluGrad     x > 0;  Relu6Grad  0 < x < 6  (TensorFlow's gradient kernels)
"""
import functools

import numpy as np
import torch

from automl_amd._lib import (ACT_HSWISH, ACT_MISH, ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SRELU, ACT_SWISH, RS_IDENTITY,
                             RS_POOL, RS_UP2)
from tests import gpu_util as gu
from tests.inference_bounds import U32, f64, ulp32, ulp_distance      # noqa: F401  (one home for the ulp helpers)

ID, UP2, POOL = RS_IDENTITY, RS_UP2, RS_POOL
SRELU_BETA = 160000.0
TINY = 2.0 ** -126        # the smallest normal float32: what a flushed denormal may be off by


def f32r(a):
  """float64 -> nearest float32, returned as float64."""
  return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def bf16r(a):
  """nearest-even rounding to bf16, returned as float32 (numpy)."""
  t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
  return t.to(torch.bfloat16).float().numpy()


def bf16_trunc(a):
  """bf16 by dropping the low 16 bits (what a kernel that forgets to round would store), as float32."""
  a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
  return (a.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def store_round(a, name):
  """Rounds float32 values to the storage type 'f32' / 'bf16' (returned as float32)."""
  a = np.asarray(a, dtype=np.float32)
  return bf16r(a) if name == 'bf16' else a


def same_bits(a, b):
  a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
  b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
  return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def same_pad(size):
  """(output size, padding before) of a 3x3 / stride 2 'SAME' pool."""
  out = (size + 1) // 2
  return out, max((out - 1) * 2 + 3 - size, 0) // 2


# ---------------------------------------------------------------------------------------- activations, float64
def sigmoid(s):
  return 1.0 / (1.0 + np.exp(-s))


def act_ref(act, s, variant=()):
  s = np.asarray(s, dtype=np.float64)
  if act == ACT_NONE:
    return s.copy()
  if act == ACT_SWISH:
    return s * sigmoid(s)
  if act == ACT_RELU:
    return np.maximum(s, 0.0)
  if act == ACT_RELU6:
    return np.minimum(np.maximum(s, 0.0), 6.0)
  if act == ACT_HSWISH:
    return s * np.minimum(np.maximum(s + 3.0, 0.0), 6.0) / 6.0
  if act == ACT_MISH:
    return s * np.tanh(np.logaddexp(0.0, s))
  assert act == ACT_SRELU, act
  # s - log1p(u) / beta, u = beta s: below u = 1e-3 the difference cancels even in float64 (u = 1e-13 leaves three digits),
  # so there the series of u - log1p(u) = u^2/2 - u^3/3 + .. (seven terms: truncated at 1e-18 of the result)
  u = SRELU_BETA * np.maximum(s, 0.0)
  us = np.minimum(u, 1e-3)
  series = us * us * (1 / 2.0 - us * (1 / 3.0 - us * (1 / 4.0 - us * (1 / 5.0 - us * (1 / 6.0 - us * (1 / 7.0 - us / 8.0))))))
  return np.where(s > 0, np.where(u < 1e-3, series, u - np.log1p(u)) / SRELU_BETA, 0.0)


def act_grad_ref(act, s, variant=()):
  """d act / d s; variant may hold 'relu_ge' (ReluGrad as x >= 0) or 'relu6_le' (Relu6Grad as x <= 6): the mutants."""
  s = np.asarray(s, dtype=np.float64)
  if act == ACT_NONE:
    return np.ones_like(s)
  if act == ACT_SWISH:
    g = sigmoid(s)
    return g * (1.0 + s * (1.0 - g))
  if act in (ACT_RELU, ACT_RELU6):
    lo = (s >= 0) if 'relu_ge' in variant else (s > 0)
    if act == ACT_RELU:
      return lo.astype(np.float64)
    hi = (s <= 6) if 'relu6_le' in variant else (s < 6)
    return (lo & hi).astype(np.float64)
  if act == ACT_HSWISH:
    return np.where(s <= -3, 0.0, np.where(s >= 3, 1.0, (2.0 * s + 3.0) / 6.0))
  if act == ACT_MISH:
    t = np.tanh(np.logaddexp(0.0, s))
    return t + s * (1.0 - t * t) * sigmoid(s)
  assert act == ACT_SRELU, act
  u = SRELU_BETA * np.maximum(s, 0.0)
  return np.where(s > 0, u / (1.0 + u), 0.0)


def act_mag(act, s):
  """The magnitude the activation's VALUE error is measured against, in float32 ulps: |act(s)|, except where the value
  is a difference of two terms (srelu: s - log1p(beta s) / beta), where it is the sum of their magnitudes -- the error of
  a rounded difference scales with its operands, not with what is left of them."""
  s = np.asarray(s, dtype=np.float64)
  if act == ACT_SRELU:
    return np.where(s > 0, s + np.log1p(SRELU_BETA * np.maximum(s, 0.0)) / SRELU_BETA, 0.0)
  return np.abs(act_ref(act, s))


def act_grad_mag(act, s):
  """The same for the DERIVATIVE: swish' = g (1 + s (1 - g)) and mish' = t + s (1 - t^2) g are sums whose terms cancel for
  s < 0 (swish' has a root at s = -1.2785), hswish' = (2 s + 3) / 6 has one at -1.5, srelu' = 1 - 1 / (1 + beta s)."""
  s = np.asarray(s, dtype=np.float64)
  if act == ACT_SWISH:
    g = sigmoid(s)
    return g * (1.0 + np.abs(s) * (1.0 - g))
  if act == ACT_HSWISH:
    return np.where(s <= -3, 0.0, np.where(s >= 3, 1.0, (2.0 * np.abs(s) + 3.0) / 6.0))
  if act == ACT_MISH:
    t = np.tanh(np.logaddexp(0.0, s))
    return t + np.abs(s) * (1.0 - t * t) * sigmoid(s)
  if act == ACT_SRELU:
    return np.where(s > 0, 1.0 + 1.0 / (1.0 + SRELU_BETA * np.maximum(s, 0.0)), 0.0)
  return np.abs(act_grad_ref(act, s))


# ---------------------------------------------------------------------------------------- one fusion node, float64
class Ref(object):
  """vals [nin] resampled views, s, out, ds [n,oh,ow,c]; gin [nin] input gradients (w.r.t. the view, without the old
  value); dwn [nin, wc]; win {input index: uint8 [n,oh,ow,c]}; mag = sum_i |wn_i v_i| (for the bounds)."""


def views(p, variant=()):
  """v_i = float32(x * scale + shift) per input as float64 [n,h,w,c]."""
  return [f32r(x * sc + sh) for x, sc, sh in zip(p.xs, p.scs, p.shs)]


def up_index(o, i, ceil=False):
  idx = np.arange(o) * i
  idx = -((-idx) // o) if ceil else idx // o
  return np.minimum(idx, i - 1)


def pool_ref(v, oh, ow, variant=()):
  """Max-pool 3x3 / s2 'SAME' of v [n,h,w,c] by a row-major scan of the nine taps: (max, winner ky*3+kx).
  variant: 'last_max' (a later equal tap replaces the winner), 'zero_pad' (padding is a candidate of value 0)."""
  n, h, w, c = v.shape
  assert same_pad(h)[0] == oh and same_pad(w)[0] == ow
  pt, pl = same_pad(h)[1], same_pad(w)[1]
  best = np.full((n, oh, ow, c), -np.inf)
  win = np.zeros((n, oh, ow, c), dtype=np.uint8)
  for ky in range(3):
    sy = np.arange(oh) * 2 - pt + ky
    for kx in range(3):
      sx = np.arange(ow) * 2 - pl + kx
      ok = ((sy >= 0) & (sy < h))[:, None] & ((sx >= 0) & (sx < w))[None, :]
      t = v[:, np.clip(sy, 0, h - 1)][:, :, np.clip(sx, 0, w - 1)]
      ok4 = np.broadcast_to(ok[None, :, :, None], t.shape)
      if 'zero_pad' in variant:
        t = np.where(ok4, t, 0.0)
        ok4 = np.ones_like(ok4)
      better = ok4 & ((t >= best) if 'last_max' in variant else (t > best))
      best = np.where(better, t, best)
      win = np.where(better, np.uint8(ky * 3 + kx), win)
  return best, win


def pool_taps(h, w):
  """[oh, ow] number of taps of each window that lie inside the image."""
  oh, pt = same_pad(h)
  ow, pl = same_pad(w)
  cy = sum(((np.arange(oh) * 2 - pt + k >= 0) & (np.arange(oh) * 2 - pt + k < h)).astype(int) for k in range(3))
  cx = sum(((np.arange(ow) * 2 - pl + k >= 0) & (np.arange(ow) * 2 - pl + k < w)).astype(int) for k in range(3))
  return cy[:, None] * cx[None, :]


def pool_ties(v, oh, ow):
  """Boolean [n,oh,ow,c]: the window's maximum is attained by more than one tap inside the image."""
  n, h, w, c = v.shape
  pt, pl = same_pad(h)[1], same_pad(w)[1]
  best, _ = pool_ref(v, oh, ow)
  count = np.zeros(best.shape, dtype=int)
  for ky in range(3):
    sy = np.arange(oh) * 2 - pt + ky
    for kx in range(3):
      sx = np.arange(ow) * 2 - pl + kx
      ok = ((sy >= 0) & (sy < h))[:, None] & ((sx >= 0) & (sx < w))[None, :]
      t = v[:, np.clip(sy, 0, h - 1)][:, :, np.clip(sx, 0, w - 1)]
      count += (ok[None, :, :, None] & (t == best)).astype(int)
  return count > 1


def node_ref(p, wn=None, variant=(), vs=None):
  """The float64 reference of problem p with normalised weights wn [nin, wc] (default: p.wn).  variant: a set of mutant
  names -- 'max_before_affine', 'last_max', 'zero_pad', 'ceil_nearest', 'relu_ge', 'relu6_le'; vs: the views, if the
  caller damaged them itself."""
  n, oh, ow, c = p.shape
  wn = np.asarray(p.wn if wn is None else wn, dtype=np.float64).reshape(p.nin, -1)
  r = Ref()
  vs = views(p) if vs is None else vs
  r.vals, r.win = [], {}
  for i, (mode, h, w) in enumerate(p.ins):
    v = vs[i]
    if mode == ID:
      val = v
    elif mode == UP2:
      ceil = 'ceil_nearest' in variant
      val = v[:, up_index(oh, h, ceil)][:, :, up_index(ow, w, ceil)]
    else:
      if 'max_before_affine' in variant:
        raw, win = pool_ref(p.xs[i], oh, ow, variant)
        val = f32r(raw * p.scs[i] + p.shs[i])
      else:
        val, win = pool_ref(v, oh, ow, variant)
      r.win[i] = win
    r.vals.append(val)
  r.s = sum(wn[i] * r.vals[i] for i in range(p.nin))
  r.mag = sum(np.abs(wn[i] * r.vals[i]) for i in range(p.nin))
  r.out = act_ref(p.act, r.s)
  r.ds = p.dout * act_grad_ref(p.act, r.s, variant)
  r.dwn = np.stack([(r.ds * val).sum((0, 1, 2)) if wn.shape[1] > 1 else (r.ds * val).sum(keepdims=True).reshape(1)
                    for val in r.vals])
  r.dwn_mag = np.stack([np.abs(r.ds * val).sum((0, 1, 2)) if wn.shape[1] > 1 else np.abs(r.ds * val).sum().reshape(1)
                        for val in r.vals])
  r.gin = [input_grad_ref(p, i, r.ds, wn[i], r.win.get(i), variant) for i in range(p.nin)]
  return r


def input_grad_ref(p, i, ds, wn_i, win=None, variant=()):
  """d loss / d view_i from ds (float64), without the old value."""
  n, oh, ow, c = p.shape
  mode, h, w = p.ins[i]
  if mode == ID:
    return wn_i * ds
  g = np.zeros((n, h, w, c))
  if mode == UP2:
    ceil = 'ceil_nearest' in variant
    iy, ix = up_index(oh, h, ceil), up_index(ow, w, ceil)
    np.add.at(g, (slice(None), iy[:, None], ix[None, :]), ds)
    return wn_i * g
  pt, pl = same_pad(h)[1], same_pad(w)[1]
  for ky in range(3):
    sy = np.arange(oh) * 2 - pt + ky
    for kx in range(3):
      sx = np.arange(ow) * 2 - pl + kx
      hit = np.where(win == ky * 3 + kx, ds, 0.0)
      oky, okx = (sy >= 0) & (sy < h), (sx >= 0) & (sx < w)
      # (a winner is always a tap inside the image; the zero_pad mutant may elect a padding tap: its ds is lost)
      np.add.at(g, (slice(None), sy[oky][:, None], sx[okx][None, :]), hit[:, oky][:, :, okx])
  return wn_i * g


# ---------------------------------------------------------------------------------------- edet_fuse_bwd_input, float32
def bwd_input_f32(mode, in_hw, ds, wn_i, old, name, win=None):
  """edet_fuse_bwd_input as an exact function of what is stored: ds float32 [n,oh,ow,c] (the stored values), wn_i a
  float32 scalar or [c], old the float32 gradient to accumulate into or None, win the winner plane of a pooled input.
  The ds that reach a source pixel are added in float32 in the kernel's loop order (output rows, then columns) starting
  from 0, then ONE rounded product with wn_i, ONE rounded add of the old value, ONE rounding to the storage type."""
  ds = np.asarray(ds, dtype=np.float32)
  n, oh, ow, c = ds.shape
  h, w = in_hw
  if mode == ID:
    g = ds.copy()
  else:
    g = np.zeros((n, h, w, c), dtype=np.float32)
    sy, sx = np.arange(h), np.arange(w)
    if mode == UP2:
      ylo, yhi = -((-sy * oh) // h), -((-(sy + 1) * oh) // h)
      xlo, xhi = -((-sx * ow) // w), -((-(sx + 1) * ow) // w)
      yhi[-1], xhi[-1] = oh, ow
    else:
      pt, pl = same_pad(h)[1], same_pad(w)[1]
      ylo, yhi = np.maximum((sy + pt - 1) // 2, 0), np.minimum((sy + pt) // 2, oh - 1) + 1
      xlo, xhi = np.maximum((sx + pl - 1) // 2, 0), np.minimum((sx + pl) // 2, ow - 1) + 1
    for a in range(int((yhi - ylo).max())):
      oy = ylo + a
      for b in range(int((xhi - xlo).max())):
        ox = xlo + b
        ok = (oy < yhi)[:, None] & (ox < xhi)[None, :]
        oyc, oxc = np.minimum(oy, oh - 1), np.minimum(ox, ow - 1)
        t = ds[:, oyc][:, :, oxc]
        ok4 = np.broadcast_to(ok[None, :, :, None], t.shape)
        if mode == POOL:
          tap = ((sy - (oyc * 2 - pt)) * 3)[:, None] + (sx - (oxc * 2 - pl))[None, :]
          ok4 = ok4 & (win[:, oyc][:, :, oxc] == tap[None, :, :, None])
        g = np.where(ok4, g + t, g).astype(np.float32)
  g = (g * np.asarray(wn_i, dtype=np.float32)).astype(np.float32)
  if old is not None:
    g = (g + np.asarray(old, dtype=np.float32)).astype(np.float32)
  return store_round(g, name)


# ---------------------------------------------------------------------------------------- the fusion variables
def normalise_ref(ws, method):
  """Normalised weights [nin, wc] in float64 from the variables ws [nin, wc] (float32 values): method 0 'fastattn'
  relu(w) / (sum relu(w) + 1e-4), 1 'sum' (ones), 2 'attn' (softmax).  eps: see normalise_ref_eps."""
  return normalise_ref_eps(ws, method, 1e-4)


def normalise_ref_eps(ws, method, eps):
  ws = np.asarray(ws, dtype=np.float64)
  if method == 1:
    return np.ones_like(ws)
  if method == 2:
    e = np.exp(ws - ws.max(0))
    return e / e.sum(0)
  r = np.maximum(ws, 0.0)
  return r / (r.sum(0) + eps)


def normalise_bwd_ref(ws, method, dwn, eps=1e-4):
  """(dw, mag) [nin, wc] float64: the variables' gradients given d(normalised weights), and the sum of the magnitudes of
  the terms each is made of -- |dwn_i / s| + |dot / s^2| for fastattn, p_i (|dwn_i| + sum_j |dwn_j p_j|) for softmax."""
  ws, dwn = np.asarray(ws, dtype=np.float64), np.asarray(dwn, dtype=np.float64)
  if method == 1:
    return np.zeros_like(ws), np.zeros_like(ws)
  if method == 2:
    p = normalise_ref(ws, 2)
    dot = (dwn * p).sum(0)
    return p * (dwn - dot), p * (np.abs(dwn) + np.abs(dwn * p).sum(0))
  r = np.maximum(ws, 0.0)
  s = r.sum(0) + eps
  dot = (dwn * r).sum(0)
  live = ws > 0
  return np.where(live, dwn / s - dot / (s * s), 0.0), np.where(live, np.abs(dwn / s) + np.abs(dwn * r).sum(0) / (s * s), 0.0)


def normaliser_distance(wn, ref):
  """Largest distance of float32 normalised weights from the float64 reference, in float32 ulps of the reference."""
  ref = np.asarray(ref, dtype=np.float64)
  err = np.abs(f64(wn).reshape(ref.shape) - ref)
  return float((np.maximum(err - TINY, 0.0) / ulp32(np.maximum(np.abs(ref), TINY))).max())


def normaliser_bwd_distance(dw, ref, mag):
  """The same for the variables' gradients, in float32 ulps of the term sum `mag`."""
  ref, mag = np.asarray(ref, dtype=np.float64), np.asarray(mag, dtype=np.float64)
  err = np.abs(f64(dw).reshape(ref.shape) - ref)
  return float((np.maximum(err - TINY, 0.0) / ulp32(np.maximum(mag, TINY))).max())


# ---------------------------------------------------------------------------------------- measured constants
# Every budget is twice the largest distance of the device's result from the float64 reference, measured on an MI355X on
# the inputs named; it cannot be derived, because it comes from v_exp_f32, v_log_f32, v_rcp_f32 and the fast division.
# A bound never exceeds its cap (the budget functions below clamp it there): a MEASUREMENT above the cap is a finding about
# the kernel, not a number to raise.
ACT_ULPS_CAP = 16.0
NORM_ULPS_CAP = 8.0
# The activation sweep of test_gpu_fuse_exact.py: s = k / 256 for every integer k in [-4096, 4096] (|s| <= 16), fp32
# storage, one identity input with weight 1; value through edet_fuse_fwd, derivative through the ds of edet_fuse_bwd_pre
# with dout = 1.  Distances in float32 ulps of act_mag / act_grad_mag.  Measured maxima and where they occur:
#   swish   value 14.2627 at s = -11.48828125, derivative 12.5934 at s = -12.30078125
#   hswish  value  0.3333 at s =  -2.99609375, derivative  0.3333 at s =   0.00390625
#   mish    value 13.8655 at s = -15.94140625, derivative 13.7710 at s = -13.828125
#   srelu   value  0.4999 at s =   5.5390625,  derivative  0.2500 at s =   5.66796875
# The large figures sit at large negative s and are __expf's: exp(x) is exp2(x * log2(e)) with the product rounded to
# float32, half an ulp of a number near 16..23 in the exponent, which is up to 11 ulps of the result; twice such a
# measurement is past the cap, so the bound of swish and mish IS the cap, 16 ulps.  (Before this module the derivative of
# mish measured 21.9654 ulps at s = 11.546875 -- above the cap: 1 - t^2 taken from a rounded t next to 1; common.h now
# evaluates it as 4 (w + 1) / (w + 2)^2.)
ACT_VALUE_MEASURED_ULPS = {ACT_SWISH: 14.27, ACT_HSWISH: 0.334, ACT_MISH: 13.87, ACT_SRELU: 0.5}
ACT_GRAD_MEASURED_ULPS = {ACT_SWISH: 12.60, ACT_HSWISH: 0.334, ACT_MISH: 13.78, ACT_SRELU: 0.25}
# The normalisers on NORM_EDGE below, scalar variables and the per-channel form (edet_fuse_weights /
# edet_fuse_weights_bwd): ulps of the reference weight, and of the term sum of normalise_bwd_ref for the gradients, whose
# d(normalised weights) are the exact weight sums of a 2x2x8 integer node (scalar) or (3, -2, 0.75) (per channel).
#   fastattn  weights 1.6661 at variables (0.001, 0.002, 0.0015); gradients 1.0127, same variables, per-channel form
#   softmax   weights 0.6994 at variables (0.3, -1.2, 0.8);       gradients 0.7421, same variables, per-channel form
NORM_MEASURED_ULPS = {0: 1.67, 2: 0.70}
NORM_BWD_MEASURED_ULPS = {0: 1.02, 2: 0.75}


def act_value_ulps(act):
  return min(2.0 * ACT_VALUE_MEASURED_ULPS[act], ACT_ULPS_CAP)


def act_grad_ulps(act):
  return min(2.0 * ACT_GRAD_MEASURED_ULPS[act], ACT_ULPS_CAP)


def norm_ulps(method):
  return min(2.0 * NORM_MEASURED_ULPS[method], NORM_ULPS_CAP)


def norm_bwd_ulps(method):
  return min(2.0 * NORM_BWD_MEASURED_ULPS[method], NORM_ULPS_CAP)


SWEEP_GRID = np.arange(-4096, 4097, dtype=np.float64) / 256.0
# the wide sweep: only finite / sign / exact kinks / |got - ref| <= 2^-10 |ref| + 2^-126 max(1, |s|)
SWEEP_WIDE = np.concatenate([
    np.array([0.0, -0.0, 3.0, -3.0, 6.0, 20.0, -20.0, 100.0, -100.0, 2.0 ** -126, 2.0 ** -100, 2.0 ** -60, 2.0 ** -30,
              2.0 ** -20, 2.0 ** -12, 2.0 ** -6]),
    np.linspace(-100.0, 100.0, 2001)]).astype(np.float32).astype(np.float64)


def wide_ok(got, ref, s):
  return np.abs(f64(got) - ref) <= 2.0 ** -10 * np.abs(ref) + TINY * np.maximum(1.0, np.abs(s))


# (method, variables [nin][wc = 1]) -- the scalar cases; the per-channel form of a case puts case k in channel k
NORM_EDGE = [
    (0, (-1.0, -0.5, 0.0)),            # all variables <= 0: exact zeros, value and gradient
    (0, (0.7, 0.0, 1.3)),              # one variable exactly 0: its weight and its gradient are exactly 0
    (0, (1e-6, 1e-6, 1e-6)),           # far below the 1e-4
    (0, (0.9, 0.9, 0.9)),              # equal variables
    (0, (0.001, 0.002, 0.0015)),       # the swish problems' variables: the 1e-4 is 3 % of the sum
    (0, (0.4, 1.1)),
    (2, (100.0, -100.0, 0.0)),
    (2, (0.0, 0.0, 0.0)),
    (2, (0.3, -1.2, 0.8)),
    (2, (1.5, 1.5)),
]


# ---------------------------------------------------------------------------------------- problems
class Problem(object):
  """shape (n, oh, ow, c); ins [(mode, h, w)]; xs, scs, shs, dout, olds: float64 arrays holding values the storage type
  represents; wn [nin, wc] float64; act."""

  def wide_ld(self, i):
    return self.shape[3] + 8 * (i + 1)


# name -> ((n, oh, ow, c), inputs, activation, per-channel weights)
EXACT = {
    'td10': ((2, 10, 10, 64), [(ID, 10, 10), (UP2, 5, 5)], ACT_RELU6, False),        # fast loop and quad loop
    'td10pc': ((1, 10, 10, 40), [(ID, 10, 10), (UP2, 5, 5)], ACT_RELU, True),         # k_fuse_pc, 256 % 5 != 0
    'up9': ((2, 9, 9, 8), [(ID, 9, 9), (UP2, 5, 5)], ACT_RELU, False),                # generic: not a 2x up-sample
    'up7x9': ((3, 7, 9, 88), [(ID, 7, 9), (UP2, 4, 5)], ACT_RELU6, False),
    'td2': ((3, 2, 2, 88), [(ID, 2, 2), (UP2, 1, 1)], ACT_RELU6, False),
    'td1': ((3, 1, 1, 88), [(ID, 1, 1), (UP2, 1, 1)], ACT_RELU6, False),
    'top5': ((2, 5, 5, 40), [(ID, 5, 5), (POOL, 10, 10)], ACT_RELU6, False),
    'bu5': ((2, 5, 5, 64), [(ID, 5, 5), (ID, 5, 5), (POOL, 10, 10)], ACT_RELU, False),
    'bu5pc': ((1, 5, 5, 88), [(ID, 5, 5), (ID, 5, 5), (POOL, 10, 10)], ACT_RELU6, True),
    'top5odd': ((2, 5, 5, 64), [(ID, 5, 5), (POOL, 9, 9)], ACT_NONE, False),          # padding on one side only
    'bu5odd': ((3, 5, 5, 8), [(ID, 5, 5), (ID, 5, 5), (POOL, 9, 9)], ACT_RELU6, False),
    'top1of2': ((3, 1, 1, 88), [(ID, 1, 1), (POOL, 2, 2)], ACT_RELU6, False),
    'bu1of2': ((3, 1, 1, 88), [(ID, 1, 1), (ID, 1, 1), (POOL, 2, 2)], ACT_RELU, False),
    'top1of1': ((3, 1, 1, 88), [(ID, 1, 1), (POOL, 1, 1)], ACT_RELU6, False),
    'bu1of1': ((3, 1, 1, 88), [(ID, 1, 1), (ID, 1, 1), (POOL, 1, 1)], ACT_NONE, False),
    'pool': ((2, 5, 5, 64), [(POOL, 10, 10)], ACT_RELU6, False),                      # generic: a single input
    'upidup': ((2, 7, 9, 40), [(UP2, 4, 5), (ID, 7, 9), (UP2, 4, 5)], ACT_RELU, True),
    'poolpc': ((2, 5, 5, 8), [(ID, 5, 5), (POOL, 9, 9)], ACT_RELU6, True),            # k_fuse_pc, one chunk per pixel
    'td70': ((2, 70, 70, 64), [(ID, 70, 70), (UP2, 35, 35)], ACT_RELU6, False),       # several workgroups, ragged tails
    'bu70': ((2, 35, 35, 64), [(ID, 35, 35), (ID, 35, 35), (POOL, 70, 70)], ACT_RELU, False),
}
LAYOUTS = ('tight', 'wide')
# scalar weights from {1, 2, -1, 0.5}, all different within a node and sum |wn_i| <= 4, so |s| <= 4 * 15 = 60 < 64
SCALAR_WN = {1: [(2.0,), (-1.0,), (0.5,)],
             2: [(1.0, 2.0), (2.0, -1.0), (0.5, 1.0), (-1.0, 0.5), (2.0, 0.5)],
             3: [(1.0, 2.0, -1.0), (0.5, 1.0, 2.0), (2.0, -1.0, 0.5), (-1.0, 0.5, 1.0)]}
CYCLE_WN = (1.0, 2.0, -1.0, 0.5)      # per channel: wn[i][ch] = CYCLE_WN[(ch + i) % 4]: any three in a row sum to <= 4


def kinks(act):
  return {ACT_RELU: (0.0,), ACT_RELU6: (0.0, 6.0)}.get(act, ())


def _draw_exact(name, attempt):
  shape, ins, act, per_ch = EXACT[name]
  n, oh, ow, c = shape
  rng = np.random.default_rng(gu.seed_of('fuse_exact', name, attempt))
  p = Problem()
  p.name, p.shape, p.ins, p.act, p.nin = name, shape, ins, act, len(ins)
  p.wc = c if per_ch else 1
  p.xs = [rng.integers(-4, 5, (n, h, w, c)).astype(np.float64) for (_, h, w) in ins]
  p.scs, p.shs = [], []
  for _ in ins:
    sc = rng.choice([-2.0, -1.0, 0.0, 1.0, 2.0, 3.0], c)
    where = rng.permutation(c)
    sc[where[0]], sc[where[1]], sc[where[2]] = 0.0, -1.0, -2.0      # every input has zero and negative channels
    p.scs.append(sc)
    p.shs.append(rng.integers(-3, 4, c).astype(np.float64))
  p.dout = rng.integers(-4, 5, shape).astype(np.float64)
  p.olds = [rng.integers(-8, 9, (n, h, w, c)).astype(np.float64) for (_, h, w) in ins]
  if per_ch:
    p.wn = np.array([[CYCLE_WN[(ch + i) % 4] for ch in range(c)] for i in range(p.nin)])
  else:
    choices = SCALAR_WN[p.nin]
    p.wn = np.array(choices[rng.integers(len(choices))]).reshape(p.nin, 1)
  return p


@functools.lru_cache(maxsize=None)
def exact_problem(name):
  """The first draw of the problem's seed sequence in which s lands on every kink of the activation (the CPU test
  asserts this and everything else the exact problems claim)."""
  for attempt in range(64):
    p = _draw_exact(name, attempt)
    p.ref = node_ref(p)
    if all(bool((p.ref.s == k).any()) for k in kinks(p.act)):
      return p
  raise AssertionError('no draw of %s hits the kinks' % name)


# The real-valued problems: the shapes of tests/test_gpu_fuse_fast.py::SMALL.
SWISH = {
    'td64': ((2, 10, 10, 64), [(ID, 10, 10), (UP2, 5, 5)]),
    'bu64': ((2, 5, 5, 64), [(ID, 5, 5), (ID, 5, 5), (POOL, 10, 10)]),
    'top64': ((2, 5, 5, 64), [(ID, 5, 5), (POOL, 10, 10)]),
    'td8': ((2, 10, 10, 8), [(ID, 10, 10), (UP2, 5, 5)]),
    'td40': ((2, 10, 10, 40), [(ID, 10, 10), (UP2, 5, 5)]),
    'bu8': ((2, 5, 5, 8), [(ID, 5, 5), (ID, 5, 5), (POOL, 10, 10)]),
    'bu40': ((2, 5, 5, 40), [(ID, 5, 5), (ID, 5, 5), (POOL, 10, 10)]),
    'bu64odd': ((2, 5, 5, 64), [(ID, 5, 5), (ID, 5, 5), (POOL, 9, 9)]),
    'top40odd': ((2, 5, 5, 40), [(ID, 5, 5), (POOL, 9, 9)]),
    'td64x35': ((2, 70, 70, 64), [(ID, 70, 70), (UP2, 35, 35)]),
    'bu64x35': ((2, 35, 35, 64), [(ID, 35, 35), (ID, 35, 35), (POOL, 70, 70)]),
    'up5to9': ((2, 9, 9, 64), [(ID, 9, 9), (UP2, 5, 5)]),
}
SWISH_VARS = (0.001, 0.002, 0.0015)      # 'fastattn' variables: the 1e-4 is about 3 % of their sum


def bits8(a):
  """Rounds to 8 significant bits (bf16 values): products with bf16 / fp32 data are then exact in float64."""
  return bf16r(a).astype(np.float64)


@functools.lru_cache(maxsize=None)
def swish_problem(name, storage):
  """x, dout and the old gradients random and rounded to the storage type ('f32' / 'bf16'); scale and shift with 8
  significant bits, about a tenth of the scales negative; the weights are NOT part of the problem (the device test
  hands in the device's own normalised weights; swish_wn() is their float32-rounded reference)."""
  shape, ins = SWISH[name]
  n, oh, ow, c = shape
  rng = np.random.default_rng(gu.seed_of('fuse_swish', name, storage))
  p = Problem()
  p.name, p.shape, p.ins, p.act, p.nin, p.wc = name, shape, ins, ACT_SWISH, len(ins), 1
  draw = lambda s: store_round(rng.standard_normal(s).astype(np.float32), storage).astype(np.float64)
  p.xs = [draw((n, h, w, c)) for (_, h, w) in ins]
  p.scs, p.shs = [], []
  for _ in ins:
    sc = bits8(1 + 0.3 * rng.standard_normal(c))
    neg = rng.permutation(c)[:max(1, c // 10)]
    sc[neg] = -np.abs(sc[neg])
    p.scs.append(sc)
    p.shs.append(bits8(0.3 * rng.standard_normal(c)))
  p.dout = draw(shape)
  p.olds = [draw((n, h, w, c)) for (_, h, w) in ins]
  p.vars = np.array(SWISH_VARS[:p.nin]).astype(np.float32).reshape(p.nin, 1)
  p.wn = None
  return p


def swish_wn(p, eps=1e-4):
  """The float32 rounding of the float64 fastattn weights of the problem's variables, as float64 [nin, 1]."""
  return f32r(normalise_ref_eps(p.vars, 0, eps))


# ---------------------------------------------------------------------------------------- bounds of the swish path
def half_ulp_storage(x, name):
  """Half a unit in the last place of the storage type at |x| (float64)."""
  return (2.0 ** 16 if name == 'bf16' else 1.0) * 0.5 * ulp32(x)


def pre_bound(ref, nin):
  """|s - s_ref| of the kernel's fmaf chain: nin rounded accumulations, each of at most one ulp of a partial sum that
  sum_i |wn_i v_i| bounds -- (nin + 1) u sum_i |wn_i v_i| with room for the rounding of the bound itself."""
  return (nin + 1) * U32 * ref.mag


def fwd_bound(ref, nin, act, name, ulps=None):
  """|out - act(s_ref)|: the pre-activation error through |act'| <= 1.1 (swish), the activation's ulp budget at the
  reference value, half an ulp of the storage type at the largest value inside that bound."""
  ulps = act_value_ulps(act) if ulps is None else ulps
  e32 = 1.1 * pre_bound(ref, nin) + ulps * ulp32(act_mag(act, ref.s))
  return e32 + half_ulp_storage(np.abs(ref.out) + e32, name)


def ds_bound(p, ref, name, ulps=None):
  """|ds - dout act'(s_ref)|: |dout| times (the pre-activation error through |swish''| <= 0.5, plus the derivative's
  ulp budget), one rounded product, half an ulp of the storage type."""
  ulps = act_grad_ulps(p.act) if ulps is None else ulps
  e32 = np.abs(p.dout) * (0.5 * pre_bound(ref, p.nin) + ulps * ulp32(act_grad_mag(p.act, ref.s)))
  e32 = e32 + 0.5 * ulp32(np.abs(ref.ds) + e32)
  return e32 + half_ulp_storage(np.abs(ref.ds) + e32, name)


def violations(got, want, bound):
  """Boolean array: elements outside the bound (a NaN is outside)."""
  return ~(np.abs(f64(got) - want) <= bound)


def forward_f32(p, wn, name):
  """A plain numpy float32 restatement of the forward (np.exp in float32, fmaf chain as float32 operations)."""
  n, oh, ow, c = p.shape
  wn = np.asarray(wn, dtype=np.float32).reshape(p.nin, -1)
  r = node_ref(p, wn)
  s = np.zeros(p.shape, dtype=np.float32)
  for i in range(p.nin):
    s = (wn[i].astype(np.float64) * r.vals[i] + s.astype(np.float64)).astype(np.float32)      # one fmaf
  sig = (np.float32(1) / (np.float32(1) + np.exp(-s))).astype(np.float32)
  out = (s * sig).astype(np.float32)
  ds = (p.dout.astype(np.float32) * (sig * (np.float32(1) + s * (np.float32(1) - sig)))).astype(np.float32)
  return store_round(out, name), store_round(ds, name)
