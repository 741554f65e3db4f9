"""The checks of tests/test_gpu_fuse_exact.py must have teeth, and its inputs must be what they claim: on the CPU, the
exact problems of tests/fuse_bounds.py are shown to be exact (nothing a kernel computes on them is ever rounded) and to
land on the kinks, ties and zero-scale channels they are built for; every damaged kernel of the list below is restated
as a variant of the reference and must be rejected -- by bit inequality on the exact problems, by the bounds at their CAP
values on the swish problems; and faithful results are accepted."""
import numpy as np
import pytest

from automl_amd._lib import ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SWISH
from tests import fuse_bounds as fb
from tests.fuse_bounds import ID, POOL, UP2

EXACT_NAMES = sorted(fb.EXACT)
SWISH_NAMES = sorted(fb.SWISH)
STORAGE = ('f32', 'bf16')


def f32(a):
  return np.asarray(a, dtype=np.float64).astype(np.float32)


def asserted(p, r):
  """name -> float32 array: every tensor the device test compares bit for bit on an exact problem (with beta = 1 the
  old gradient is added; the winner planes are compared as bytes and go in as floats here)."""
  out = {'out': f32(r.out), 'ds': f32(r.ds), 'dwn': f32(r.dwn)}
  for i in range(p.nin):
    out['gin%d' % i] = f32(r.gin[i])
    out['gin%d+old' % i] = f32(r.gin[i] + p.olds[i])
  for i, w in r.win.items():
    out['win%d' % i] = w.astype(np.float32)
  return out


def rejected(p, r):
  """The tensors whose bits differ from the reference's."""
  good, bad = asserted(p, p.ref), asserted(p, r)
  return [k for k in good if not fb.same_bits(good[k], bad[k])]


def has(p, mode):
  return any(m == mode for m, _, _ in p.ins)


def pooled(p):
  return [i for i, (m, _, _) in enumerate(p.ins) if m == POOL]


# ---------------------------------------------------------------------------------------- the exact problems are exact
@pytest.mark.parametrize('name', EXACT_NAMES)
def test_exact_problems_are_exact(name):
  """Operands and every reference output survive bf16 (so also fp32) storage; the weight sums are integers or
  half-integers whose terms add up to less than 2^24 in magnitude, so every partial sum in any order is exact in fp32
  (they are fp32 outputs and are asserted in fp32: a sum of thousands of terms has more than bf16's eight bits)."""
  p = fb.exact_problem(name)
  r = p.ref
  n, oh, ow, c = p.shape
  for t in p.xs + p.scs + p.shs + p.olds + [p.dout, p.wn] + fb.views(p):
    assert np.array_equal(fb.bf16r(t).astype(np.float64), t)
  assert all(float(np.abs(x).max()) <= 4 for x in p.xs) and float(np.abs(p.dout).max()) <= 4
  assert all(float(np.abs(o).max()) <= 8 for o in p.olds) and all(float(np.abs(s).max()) <= 3 for s in p.shs)
  assert set(np.unique(p.wn).tolist()) <= {1.0, 2.0, -1.0, 0.5}
  assert p.wn.shape == (p.nin, c if fb.EXACT[name][3] else 1)
  if p.wc > 1:
    assert all(len(set(p.wn[i].tolist())) == 4 for i in range(p.nin))      # the weight depends on the channel
  for sc in p.scs:
    assert set(sc.tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0, 3.0} and (sc < 0).any() and (sc == 0).any()
  for t in [r.s, r.out, r.ds] + r.gin + [g + o for g, o in zip(r.gin, p.olds)]:
    assert float(np.abs(t).max()) < 64 and np.array_equal(t * 2, np.round(t * 2))
    assert np.array_equal(fb.bf16r(t).astype(np.float64), t)
  assert float(r.dwn_mag.max()) < 2.0 ** 24
  assert np.array_equal(f32(r.dwn).astype(np.float64), r.dwn) and np.array_equal(r.dwn * 2, np.round(r.dwn * 2))
  assert float(np.abs(r.dwn).max()) > 0 and float(np.abs(r.ds).max()) > 0
  for k in fb.kinks(p.act):
    assert bool((r.s == k).any()), 'no s == %g' % k
    assert bool(((r.s == k) & (p.dout != 0)).any())      # ... at an element where the derivative's convention shows in ds


@pytest.mark.parametrize('name', [k for k in EXACT_NAMES if any(m == POOL for m, _, _ in fb.EXACT[k][1])])
def test_exact_pool_windows_are_tied(name):
  """At least a fifth of the windows with more than one tap have a tie for the maximum, and at least one window is tied
  only because its channel's scale is zero (the raw values have a single maximum).  A window of one tap -- all of them
  in a 1x1-from-1x1 node -- cannot tie."""
  p = fb.exact_problem(name)
  n, oh, ow, c = p.shape
  for i in pooled(p):
    _, h, w = p.ins[i]
    multi = np.broadcast_to((fb.pool_taps(h, w) > 1)[None, :, :, None], p.shape)
    if not multi.any():
      assert (h, w) == (1, 1)
      continue
    tied = fb.pool_ties(fb.views(p)[i], oh, ow)
    assert float(tied[multi].mean()) >= 0.2, float(tied[multi].mean())
    raw_tied = fb.pool_ties(p.xs[i], oh, ow)
    zero = np.broadcast_to(p.scs[i] == 0, p.shape)
    assert bool((tied & ~raw_tied & zero & multi).any())
    # the winner of such a window is its first tap inside the image
    first = fb.pool_ref(np.zeros_like(p.xs[i]), oh, ow)[1]
    assert np.array_equal(p.ref.win[i][zero], first[zero])


# ---------------------------------------------------------------------------------------- mutants, exact problems
REF_VARIANTS = {
    'max_before_affine': lambda p: any(p.ins[i][1:] != (1, 1) for i in pooled(p)),      # (one tap: nothing to order)
    'last_max': lambda p: any(p.ins[i][1:] != (1, 1) for i in pooled(p)),
    'zero_pad': lambda p: has(p, POOL),
    'ceil_nearest': lambda p: any(m == UP2 and h > 1 for m, h, w in p.ins),      # (one source pixel: the clamp hides it)
    'relu_ge': lambda p: p.act in (ACT_RELU, ACT_RELU6),
    'relu6_le': lambda p: p.act == ACT_RELU6,
}


@pytest.mark.parametrize('variant', sorted(REF_VARIANTS))
def test_exact_problems_reject_the_damaged_reference(variant):
  names = [k for k in EXACT_NAMES if REF_VARIANTS[variant](fb.exact_problem(k))]
  assert len(names) >= 3, names
  for name in names:
    p = fb.exact_problem(name)
    diff = rejected(p, fb.node_ref(p, variant={variant}))
    assert diff, (variant, name)
    if variant == 'last_max':      # the forward is the same; the winner bytes and the pooled input's gradient are not
      assert not {'out', 'ds', 'dwn'} & set(diff) and any(k.startswith('win') for k in diff) and any(k.startswith('gin') for k in diff)
    if variant in ('relu_ge', 'relu6_le'):
      assert 'ds' in diff and 'out' not in diff


def test_exact_problems_reject_swapped_identity_weights():
  names = [k for k in EXACT_NAMES if [m for m, _, _ in fb.EXACT[k][1]][:2] == [ID, ID]]
  assert len(names) >= 4
  for name in names:
    p = fb.exact_problem(name)
    wn = p.wn.copy()
    wn[[0, 1]] = wn[[1, 0]]
    diff = rejected(p, fb.node_ref(p, wn))
    assert {'out', 'gin0', 'gin1'} <= set(diff), (name, diff)


def test_exact_problems_reject_rotated_channel_weights():
  names = [k for k in EXACT_NAMES if fb.EXACT[k][3]]
  assert len(names) >= 4
  for name in names:
    p = fb.exact_problem(name)
    diff = rejected(p, fb.node_ref(p, np.roll(p.wn, 1, axis=1)))
    assert 'out' in diff and 'gin0' in diff, (name, diff)


def pack(t, ld, fill):
  """[n,h,w,c] -> the buffer [pixels, ld] of a layout with channel stride ld; padding columns hold `fill`."""
  c = t.shape[-1]
  buf = np.full((t.size // c, ld), fill, dtype=np.float64)
  buf[:, :c] = t.reshape(-1, c)
  return buf


def misread(buf, shape):
  """What a kernel reads that computes this operand's offsets with c where ld is meant (it stays inside the buffer)."""
  c = shape[-1]
  rows = buf.shape[0]
  return buf.reshape(-1)[:rows * c].reshape(shape)


@pytest.mark.filterwarnings('ignore::RuntimeWarning')      # (the NaN of the padding, multiplied on purpose)
@pytest.mark.parametrize('name', EXACT_NAMES)
def test_wide_layouts_reject_c_for_ld(name):
  """Wide layouts: every operand misread in turn.  Inputs and dout carry NaN in the padding, which reaches the outputs;
  an output written with the wrong stride leaves its bytes in the wrong place (read back here with the right one)."""
  p = fb.exact_problem(name)
  n, oh, ow, c = p.shape
  for i in range(p.nin):
    ld = p.wide_ld(i)
    assert ld > c and ld % 8 == 0
    q = fb.Problem()
    q.__dict__.update(p.__dict__)
    q.xs = list(p.xs)
    q.xs[i] = misread(pack(p.xs[i], ld, np.nan), p.xs[i].shape)
    assert 'out' in rejected(p, fb.node_ref(q)), (name, i)
  q = fb.Problem()
  q.__dict__.update(p.__dict__)
  q.dout = misread(pack(p.dout, c + 32, np.nan), p.shape)
  assert 'ds' in rejected(p, fb.node_ref(q))
  # outputs: written at pixel * c + ch into a buffer of stride ld, read back with stride ld
  for what, ld in (('out', c + 32), ('ds', c + 16)):
    want = getattr(p.ref, what)
    buf = np.full((want.size // c) * ld, 77.0)
    buf[:want.size] = want.reshape(-1)
    got = buf.reshape(-1, ld)[:, :c].reshape(want.shape)
    if want.size > c:      # (a single pixel has no second row to misplace: its canary columns would show it)
      assert not fb.same_bits(f32(got), f32(want)), (name, what)
    assert not np.array_equal(buf.reshape(-1, ld)[:, c:], np.full((want.size // c, ld - c), 77.0)) or want.size == c


@pytest.mark.parametrize('name', EXACT_NAMES)
def test_exact_problems_reject_a_dropped_partial_row(name):
  """The weight sums with one workgroup's share left out: 256 consecutive 8-channel chunks (scalar weights), or the
  pixels of one workgroup's slices (per-channel weights, 256 // (c / 8) pixels)."""
  p = fb.exact_problem(name)
  r = p.ref
  n, oh, ow, c = p.shape
  nvec = c // 8
  block = (256 // nvec) * c if p.wc > 1 else 256 * 8
  for i in range(p.nin):
    terms = (r.ds * r.vals[i]).reshape(-1)
    dropped = None
    for b in range(0, terms.size, block):
      part = terms[b:b + block]
      part = part.reshape(-1, c).sum(0) if p.wc > 1 else part.sum(keepdims=True)
      if np.any(part != 0):
        dropped = r.dwn[i] - part
        break
    assert dropped is not None and not fb.same_bits(f32(dropped), f32(r.dwn[i])), (name, i)


@pytest.mark.parametrize('name', EXACT_NAMES)
def test_float32_restatement_of_bwd_input_on_the_exact_problems(name):
  """bwd_input_f32 (the float32 restatement the device test compares bit for bit on the swish problems) gives the
  reference's gradients on the exact problems, where no order of additions matters -- and not with the mutant winners."""
  p = fb.exact_problem(name)
  r = p.ref
  for storage in STORAGE:
    for i, (mode, h, w) in enumerate(p.ins):
      wn_i = p.wn[i] if p.wc > 1 else p.wn[i, 0]
      for old in (None, p.olds[i]):
        got = fb.bwd_input_f32(mode, (h, w), r.ds, wn_i, old, storage, r.win.get(i))
        assert fb.same_bits(got, f32(r.gin[i] if old is None else r.gin[i] + old)), (name, i)
      if mode == POOL and (h, w) != (1, 1):
        last = fb.node_ref(p, variant={'last_max'}).win[i]
        assert not fb.same_bits(fb.bwd_input_f32(mode, (h, w), r.ds, wn_i, None, storage, last), f32(r.gin[i]))


# ---------------------------------------------------------------------------------------- the swish problems
@pytest.mark.parametrize('storage', STORAGE)
@pytest.mark.parametrize('name', SWISH_NAMES)
def test_swish_problems_are_what_they_claim(name, storage):
  p = fb.swish_problem(name, storage)
  c = p.shape[3]
  for x in p.xs + p.olds + [p.dout]:
    assert np.array_equal(fb.store_round(x, storage).astype(np.float64), x)
  for sc, sh in zip(p.scs, p.shs):
    assert np.array_equal(fb.bits8(sc), sc) and np.array_equal(fb.bits8(sh), sh)
    assert 1 <= int((sc < 0).sum()) and abs(int((sc < 0).sum()) - c / 10.0) <= max(1.0, c / 10.0)
  # v is exact in float64 before its one rounding: x (24 bits) * scale (8 bits) + shift, exponents within 2^12 of each other
  wn = fb.normalise_ref(p.vars, 0)
  assert 0.02 < 1e-4 / (float(p.vars.sum()) + 1e-4) < 0.04


SWISH_VARIANTS = ('max_before_affine', 'zero_pad', 'ceil_nearest')


@pytest.mark.parametrize('storage', STORAGE)
@pytest.mark.parametrize('name', SWISH_NAMES)
def test_swish_bounds_accept_faithful_results_and_reject_the_mutants_at_the_cap(name, storage):
  """The float32 cast of the float64 reference (rounded to the storage type) passes the bounds with NO activation
  budget, a plain float32 evaluation passes at the caps, and every applicable mutant breaks the forward bound at the cap."""
  p = fb.swish_problem(name, storage)
  wn = fb.swish_wn(p)
  r = fb.node_ref(p, wn)
  cap = fb.ACT_ULPS_CAP
  out, ds = fb.store_round(f32(r.out), storage), fb.store_round(f32(r.ds), storage)
  assert not fb.violations(out, r.out, fb.fwd_bound(r, p.nin, ACT_SWISH, storage, ulps=0.0)).any()
  assert not fb.violations(ds, r.ds, fb.ds_bound(p, r, storage, ulps=0.0)).any()
  out32, ds32 = fb.forward_f32(p, wn, storage)
  assert not fb.violations(out32, r.out, fb.fwd_bound(r, p.nin, ACT_SWISH, storage, ulps=cap)).any()
  assert not fb.violations(ds32, r.ds, fb.ds_bound(p, r, storage, ulps=cap)).any()
  fwd_cap, ds_cap = fb.fwd_bound(r, p.nin, ACT_SWISH, storage, ulps=cap), fb.ds_bound(p, r, storage, ulps=cap)

  def broken(m):
    o = fb.store_round(f32(m.out), storage)
    d = fb.store_round(f32(m.ds), storage)
    return fb.violations(o, r.out, fwd_cap).any() and fb.violations(d, r.ds, ds_cap).any()

  applicable = {'max_before_affine': has(p, POOL), 'zero_pad': has(p, POOL), 'ceil_nearest': has(p, UP2)}
  for variant in SWISH_VARIANTS:
    if applicable[variant]:
      assert broken(fb.node_ref(p, wn, variant={variant})), variant
  if p.nin == 3:
    sw = wn.copy()
    sw[[0, 1]] = sw[[1, 0]]
    assert broken(fb.node_ref(p, sw)), 'weights swapped'
  # the fusion weights of a kernel whose 1e-4 is missing or is 1e-3, through the whole node
  for eps in (0.0, 1e-3):
    assert broken(fb.node_ref(p, fb.swish_wn(p, eps))), eps
  # last maximum wins: the forward is the same, the winner bytes (compared as bytes on the device) are not
  if has(p, POOL):
    i = pooled(p)[0]
    last = fb.node_ref(p, wn, variant={'last_max'})
    assert fb.same_bits(f32(last.out), f32(r.out))
    ties = float(fb.pool_ties(fb.views(p)[i], p.shape[1], p.shape[2]).mean())
    assert (ties == 0.0) == np.array_equal(last.win[i], r.win[i])


@pytest.mark.parametrize('name', SWISH_NAMES)
def test_bf16_truncation_breaks_the_swish_bound(name):
  """An output truncated to bf16 instead of rounded is off by up to one bf16 ulp: outside the bound, even at the cap, on
  more than 30 % of the elements."""
  p = fb.swish_problem(name, 'bf16')
  wn = fb.swish_wn(p)
  r = fb.node_ref(p, wn)
  bound = fb.fwd_bound(r, p.nin, ACT_SWISH, 'bf16', ulps=fb.ACT_ULPS_CAP)
  frac = float(fb.violations(fb.bf16_trunc(f32(r.out)), r.out, bound).mean())
  assert frac > 0.3, frac
  assert not fb.violations(fb.bf16r(f32(r.out)), r.out, bound).any()
  frac = float(fb.violations(fb.bf16_trunc(f32(r.ds)), r.ds, fb.ds_bound(p, r, 'bf16', ulps=fb.ACT_ULPS_CAP)).mean())
  assert frac > 0.3, frac


# ---------------------------------------------------------------------------------------- normalisers, constants
def test_normaliser_bounds_reject_the_wrong_epsilon():
  for nin in (2, 3):
    ws = np.array(fb.SWISH_VARS[:nin]).astype(np.float32).astype(np.float64).reshape(nin, 1)
    ref = fb.normalise_ref(ws, 0)
    assert fb.normaliser_distance(f32(ref), ref) <= 0.5
    for eps in (0.0, 1e-3):
      assert fb.normaliser_distance(f32(fb.normalise_ref_eps(ws, 0, eps)), ref) > 1e3 * fb.NORM_ULPS_CAP
    dwn = np.array([[3.0], [-2.0], [0.7]])[:nin]
    dw, mag = fb.normalise_bwd_ref(ws, 0, dwn)
    assert fb.normaliser_bwd_distance(f32(dw), dw, mag) <= 0.5
    for eps in (0.0, 1e-3):
      assert fb.normaliser_bwd_distance(f32(fb.normalise_bwd_ref(ws, 0, dwn, eps)[0]), dw, mag) > 1e3 * fb.NORM_ULPS_CAP
  # with the weights of tests/test_gpu_fuse_fast.py (0.3 .. 1.5) the same damage moves the result by some 5e-5 relative
  ws = np.array([[0.9], [1.2]])
  rel = np.abs(fb.normalise_ref_eps(ws, 0, 0.0) / fb.normalise_ref(ws, 0) - 1).max()
  assert 2e-5 < rel < 2e-4


def test_normaliser_references():
  for method, ws in fb.NORM_EDGE:
    ws = np.array(ws).reshape(len(ws), 1)
    wn = fb.normalise_ref(ws, method)
    if method == 2:
      assert abs(float(wn.sum()) - 1) < 1e-12
    # the gradient against central differences of the float64 reference
    dwn = np.arange(1, len(ws) + 1, dtype=np.float64).reshape(-1, 1) * np.array([[1.0], [-1.0], [0.5]])[:len(ws)]
    dw, mag = fb.normalise_bwd_ref(ws, method, dwn)
    assert np.all(np.abs(dw) <= mag * (1 + 1e-12))
    for i in range(len(ws)):
      if method == 0 and ws[i, 0] <= 0:
        assert dw[i, 0] == 0.0
        continue
      h = 1e-7 * max(1.0, abs(ws[i, 0])) if ws[i, 0] > 1e-5 or method == 2 else 1e-9
      up, dn = ws.copy(), ws.copy()
      up[i] += h
      dn[i] -= h
      num = float(((fb.normalise_ref(up, method) - fb.normalise_ref(dn, method)) * dwn).sum() / (2 * h))
      assert abs(num - dw[i, 0]) <= 1e-5 * max(float(mag[i, 0]), 1e-30), (method, ws.ravel(), i, num, dw[i, 0])


def test_measured_constants_respect_their_caps():
  for table in (fb.ACT_VALUE_MEASURED_ULPS, fb.ACT_GRAD_MEASURED_ULPS):
    for act, v in table.items():
      assert 0 < v <= fb.ACT_ULPS_CAP, (act, v)
  for table in (fb.NORM_MEASURED_ULPS, fb.NORM_BWD_MEASURED_ULPS):
    for m, v in table.items():
      assert 0 < v <= fb.NORM_ULPS_CAP, (m, v)
  for act in fb.ACT_VALUE_MEASURED_ULPS:
    assert fb.act_value_ulps(act) <= fb.ACT_ULPS_CAP and fb.act_grad_ulps(act) <= fb.ACT_ULPS_CAP
  for m in fb.NORM_MEASURED_ULPS:
    assert fb.norm_ulps(m) <= fb.NORM_ULPS_CAP and fb.norm_bwd_ulps(m) <= fb.NORM_ULPS_CAP


def test_activation_references():
  """Kinks as TensorFlow's gradient kernels define them, derivatives against central differences, and the wide bound's
  teeth: a result off by 2^-9 relative is refused."""
  from automl_amd._lib import ACT_HSWISH, ACT_MISH, ACT_SRELU
  assert fb.act_grad_ref(ACT_RELU, np.array([-1.0, 0.0, 1.0])).tolist() == [0.0, 0.0, 1.0]
  assert fb.act_grad_ref(ACT_RELU6, np.array([0.0, 3.0, 6.0, 7.0])).tolist() == [0.0, 1.0, 0.0, 0.0]
  assert fb.act_grad_ref(ACT_RELU, np.array([0.0]), {'relu_ge'}).tolist() == [1.0]
  assert fb.act_grad_ref(ACT_RELU6, np.array([6.0]), {'relu6_le'}).tolist() == [1.0]
  assert fb.act_grad_ref(ACT_HSWISH, np.array([-3.0, 3.0, 0.0])).tolist() == [0.0, 1.0, 0.5]
  s = np.linspace(-15.9, 15.9, 2001) + 1e-3
  for act in (ACT_SWISH, ACT_HSWISH, ACT_MISH, ACT_SRELU):
    s_ = s[np.abs(np.abs(s) - 3) > 1e-2] if act == ACT_HSWISH else s
    s_ = s_[np.abs(s_) > 1e-2] if act == ACT_SRELU else s_
    h = 1e-6
    num = (fb.act_ref(act, s_ + h) - fb.act_ref(act, s_ - h)) / (2 * h)
    assert np.abs(num - fb.act_grad_ref(act, s_)).max() < 1e-6, act
    assert np.all(fb.act_mag(act, s_) >= np.abs(fb.act_ref(act, s_)) * (1 - 1e-12))
    assert np.all(fb.act_grad_mag(act, s_) >= np.abs(fb.act_grad_ref(act, s_)) * (1 - 1e-12))
    ref = fb.act_ref(act, fb.SWEEP_WIDE)
    assert fb.wide_ok(f32(ref), ref, fb.SWEEP_WIDE).all()
    big = np.abs(ref) > 1e-30
    assert not fb.wide_ok(f32(ref * (1 + 2.0 ** -9)), ref, fb.SWEEP_WIDE)[big].any()
