"""The BiFPN fusion kernels (automl_amd/csrc/fuse.hip) against the independent references of tests/fuse_bounds.py:

  * exact-integer problems, where no operation rounds: forward, ds, weight sums, recorded pool winners and every input
    gradient bit for bit against the float64 reference, through every code path (specialised loops, 2x2 quad backward,
    generic body, k_fuse_pc, edet_fuse_bwd_input's branches), in tight layouts and in wide ones (every operand its own
    channel stride, NaN in the padding of what is read, canaries in the padding of and behind what is written);
  * edet_fuse_bwd_input as an exact float32 function of the stored ds, weights, winners and old gradient;
  * the real-valued swish path elementwise inside componentwise bounds;
  * the activations swept through the entry points, and the fusion-variable normalisers at their edges, inside measured
    ulp budgets.

tests/test_fuse_bounds.py shows on the CPU that these checks refuse the damaged kernels they are meant to catch.
The launch log names kernels, not the loops inside k_fuse: it tells k_fuse_pc, k_fuse and k_fuse_dwn_finish apart; that
a node is one of those with a specialised loop is asserted from its shape (fill_args' rule, restated in fast_kind)."""
import ctypes

import numpy as np
import pytest
import torch

from automl_amd import _lib
from automl_amd._lib import ACT_HSWISH, ACT_MISH, ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SRELU, ACT_SWISH, TView, call, ptr
from tests import fuse_bounds as fb
from tests import gpu_util as gu
from tests.fuse_bounds import ID, POOL, UP2
from tests.test_gpu_fuse_fast import wtol

pytestmark = pytest.mark.gpu

CANARY = 77.0
NAN = float('nan')
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}


def bits(t):
  return t.view(INT_OF[t.dtype])


class Buf(object):
  """[rows + 1, ld] on the device: `rows` pixels of c payload channels and ld - c padding channels, and one guard row.
  An operand the kernel READS has NaN in its padding; one it WRITES has the canary there; the guard row is the canary."""

  def __init__(self, shape, ld, tdt, payload=None, reads=False):
    self.shape, self.c, self.ld = shape, shape[-1], ld
    self.rows = int(np.prod(shape[:-1]))
    t = torch.full((self.rows + 1, ld), CANARY, dtype=torch.float32)
    t[:self.rows, self.c:] = NAN if reads else CANARY
    t[:self.rows, :self.c] = NAN if payload is None else torch.from_numpy(
        np.ascontiguousarray(np.asarray(payload, dtype=np.float32))).reshape(self.rows, self.c)
    self.t = t.to(device=gu.DEV, dtype=tdt)
    self.snap = self.t.clone()
    self.reads = reads

  def ptr(self):
    return self.t.data_ptr()

  def payload(self):
    return self.t[:self.rows, :self.c].float().cpu().numpy().reshape(self.shape)

  def check(self, what):
    if self.reads:
      assert torch.equal(bits(self.t), bits(self.snap)), '%s: an input buffer changed' % what
    else:
      assert torch.equal(bits(self.t[:self.rows, self.c:]), bits(self.snap[:self.rows, self.c:])), '%s: padding written' % what
      assert torch.equal(bits(self.t[self.rows]), bits(self.snap[self.rows])), '%s: guard row written' % what


def fast_kind(p, wc):
  """fill_args' rule: scalar weights, identities and then one exact 2x up-sample (two inputs) or one pool."""
  modes = [m for m, _, _ in p.ins]
  if wc != 1 or p.nin < 2 or any(m != ID for m in modes[:-1]):
    return None
  _, h, w = p.ins[-1]
  if modes[-1] == UP2 and p.nin == 2 and p.shape[1] == 2 * h and p.shape[2] == 2 * w:
    return 'up2'
  return 'pool' if modes[-1] == POOL else None


class DevNode(object):
  """Problem p on the device in storage type dt and layout 'tight' / 'wide', with normalised weights wn [nin, wc]."""

  def __init__(self, p, dt, layout, wn):
    self.p, (self.name, self.edt, self.tdt) = p, dt
    n, oh, ow, c = p.shape
    wide = layout == 'wide'
    self.ldi = [p.wide_ld(i) if wide else c for i in range(p.nin)]
    self.ldo = c + 32 if wide else c
    self.ldds = c + 16 if wide else c      # the stride of the ds handed to edet_fuse_bwd_input
    self.xb = [Buf(x.shape, ld, self.tdt, x, reads=True) for x, ld in zip(p.xs, self.ldi)]
    self.coef = [(gu.fdev(torch.from_numpy(sc.astype(np.float32))), gu.fdev(torch.from_numpy(sh.astype(np.float32))))
                 for sc, sh in zip(p.scs, p.shs)]
    self.tvs = [TView(b.ptr(), ptr(sc), ptr(sh), None, 0, n, h, w, c, ld)
                for b, (sc, sh), (_, h, w), ld in zip(self.xb, self.coef, p.ins, self.ldi)]
    self.tvp = [ctypes.byref(t) for t in self.tvs] + [None] * (3 - p.nin)
    self.modes = (ctypes.c_int * 3)(*([m for m, _, _ in p.ins] + [0] * (3 - p.nin)))
    wn = np.asarray(wn, dtype=np.float32).reshape(p.nin, -1)
    self.wc = wn.shape[1]
    self.wn_np = wn
    self.wn = torch.zeros(max(4, 3 * self.wc), dtype=torch.float32, device=gu.DEV)
    self.wn[:wn.size] = torch.from_numpy(wn.reshape(-1)).to(gu.DEV)
    self.dout = Buf(p.shape, self.ldo, self.tdt, p.dout, reads=True)
    self.pools = [i for i, (m, _, _) in enumerate(p.ins) if m == POOL]
    self.wsp = torch.empty(1 << 20, dtype=torch.float32, device=gu.DEV)
    self.log = {}

  def inputs_intact(self, what):
    for b in self.xb + [self.dout]:
      b.check(what)

  def fwd(self, wraw=None, method=0):
    p = self.p
    n, oh, ow, c = p.shape
    out = Buf(p.shape, self.ldo, self.tdt)
    wn = torch.full_like(self.wn, NAN) if wraw is not None else self.wn
    call('edet_fuse_fwd', self.tvp[0], self.tvp[1], self.tvp[2], self.modes, p.nin, ptr(wn), self.wc, p.act, out.ptr(),
         oh, ow, self.ldo, wraw, method, self.edt, gu.stream())
    torch.cuda.synchronize()
    out.check('fwd out')
    self.inputs_intact('fwd')
    return (out.payload(), wn) if wraw is not None else out.payload()

  def bwd_pre(self, dwn=True, workspace=True, argmax=True, merged=(), beta=0, write_ds=1, wraw=None, dwraw=None, method=0):
    """-> ds payload, dwn [nin, wc], winner planes {input: uint8 [n,oh,ow,c]}, {i: gradient payload written in-pass}."""
    p = self.p
    n, oh, ow, c = p.shape
    ds = Buf(p.shape, self.ldo, self.tdt)
    dw = torch.zeros(max(4, 3 * self.wc), dtype=torch.float32, device=gu.DEV)
    plane = n * oh * ow * c
    amax = torch.full((max(len(self.pools), 1) * plane + c,), 255, dtype=torch.uint8, device=gu.DEV)
    gin, gbeta, gb = (ctypes.c_void_p * 3)(), (ctypes.c_int * 3)(), {}
    for i in merged:
      gb[i] = Buf(p.xs[i].shape, self.ldi[i], self.tdt, p.olds[i] if beta else None)
      gin[i], gbeta[i] = gb[i].ptr(), beta
    use_amax = bool(self.pools) and argmax
    _lib.launch_log_start()
    try:
      call('edet_fuse_bwd_pre', self.tvp[0], self.tvp[1], self.tvp[2], self.modes, p.nin, ptr(self.wn), self.wc, p.act,
           self.dout.ptr(), oh, ow, self.ldo, ds.ptr(), ptr(dw) if dwn else None, ptr(amax) if use_amax else None,
           gin if merged else None, gbeta if merged else None, write_ds, ptr(self.wsp) if workspace else None,
           self.wsp.numel() * 4 if workspace else 0, wraw, method, dwraw, self.edt, gu.stream())
    finally:
      self.log = _lib.launch_log_stop()
    torch.cuda.synchronize()
    what = 'bwd_pre merged=%s beta=%d write_ds=%d' % (list(merged), beta, write_ds)
    ds.check(what + ' ds')
    for i in merged:
      gb[i].check(what + ' gin %d' % i)
    self.inputs_intact(what)
    used = len(self.pools) * plane if use_amax else 0
    assert bool((amax[used:] == 255).all()), what + ': winner bytes written past the planes'
    wins = {i: amax[k * plane:(k + 1) * plane].cpu().numpy().reshape(p.shape) for k, i in enumerate(self.pools)} if use_amax else {}
    return ds.payload(), dw[:p.nin * self.wc].cpu().numpy().reshape(p.nin, self.wc), wins, {i: gb[i].payload() for i in merged}

  def bwd_input(self, i, ds, win=None, beta=0):
    p = self.p
    n, oh, ow, c = p.shape
    dsb = Buf(p.shape, self.ldds, self.tdt, ds, reads=True)
    g = Buf(p.xs[i].shape, self.ldi[i], self.tdt, p.olds[i] if beta else None)
    am = None
    if win is not None:
      am = torch.full((win.size + c,), 255, dtype=torch.uint8, device=gu.DEV)
      am[:win.size] = torch.from_numpy(np.ascontiguousarray(win).reshape(-1)).to(gu.DEV)
    call('edet_fuse_bwd_input', ctypes.byref(self.tvs[i]), p.ins[i][0], ptr(self.wn), self.wc, i, dsb.ptr(), oh, ow,
         self.ldds, ptr(am), g.ptr(), beta, self.edt, gu.stream())
    torch.cuda.synchronize()
    what = 'bwd_input %d beta=%d recorded=%s' % (i, beta, win is not None)
    g.check(what)
    dsb.check(what + ' ds')
    self.inputs_intact(what)
    return g.payload()

  def merged_inputs(self):
    m = [i for i, (mode, _, _) in enumerate(self.p.ins) if mode == ID]
    if fast_kind(self.p, self.wc) == 'up2':
      m.append(1)
    return m


def logged(log, sub):
  return any(sub in k for k in log)


def f32(a):
  return np.asarray(a, dtype=np.float64).astype(np.float32)


def assert_bits(got, want, what):
  want = f32(want)
  if not fb.same_bits(got, want):
    bad = np.asarray(got, dtype=np.float32).view(np.uint32) != want.view(np.uint32)
    k = tuple(np.argwhere(bad)[0])
    raise AssertionError('%s: %d of %d elements differ, first at %s: got %r, want %r' % (
        what, int(bad.sum()), bad.size, k, np.asarray(got)[k], want[k]))


# ---------------------------------------------------------------------------------------- exact problems
@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('layout', fb.LAYOUTS)
@pytest.mark.parametrize('name', sorted(fb.EXACT))
def test_exact_problems_bit_for_bit(name, layout, dt):
  p = fb.exact_problem(name)
  r = p.ref
  nd = DevNode(p, dt, layout, p.wn)
  kind = fast_kind(p, nd.wc)
  assert kind == {'td10': 'up2', 'td70': 'up2', 'td2': 'up2', 'top5': 'pool', 'bu5': 'pool', 'bu70': 'pool',
                  'up9': None, 'up7x9': None, 'pool': None, 'upidup': None, 'td10pc': None, 'bu5pc': None}.get(name, kind)
  assert_bits(nd.fwd(), r.out, 'out')
  # ds, weight sums (ordered partial rows, and one workgroup adding into dwn), recorded winners
  for workspace in (True, False):
    ds, dwn, wins, _ = nd.bwd_pre(workspace=workspace)
    assert_bits(ds, r.ds, 'ds (workspace %s)' % workspace)
    assert_bits(dwn, r.dwn, 'dwn (workspace %s)' % workspace)
    for i in nd.pools:
      assert np.array_equal(wins[i], r.win[i]), 'winner plane of input %d (workspace %s)' % (i, workspace)
    if nd.wc > 1:
      assert logged(nd.log, 'k_fuse_pc<') and not logged(nd.log, 'k_fuse<'), nd.log
    else:
      assert logged(nd.log, 'k_fuse<') and not logged(nd.log, 'k_fuse_pc<'), nd.log
      assert logged(nd.log, 'k_fuse_dwn_finish') == workspace, nd.log
  if nd.pools:      # winners not asked for: the generic body, the same ds and sums
    ds, dwn, _, _ = nd.bwd_pre(argmax=False)
    assert_bits(ds, r.ds, 'ds (no winner planes)')
    assert_bits(dwn, r.dwn, 'dwn (no winner planes)')
  ds, _, _, _ = nd.bwd_pre(dwn=False)
  assert_bits(ds, r.ds, 'ds (no weight sums)')
  # input gradients written in-pass (the quad loop when the up-sampled input's is among them)
  merged = nd.merged_inputs()
  for beta in (0, 1):
    for write_ds in (0, 1):
      ds, dwn, wins, g = nd.bwd_pre(merged=merged, beta=beta, write_ds=write_ds)
      if write_ds:
        assert_bits(ds, r.ds, 'ds (in-pass gradients, beta %d)' % beta)
      else:
        assert bool(np.isnan(ds).all()), 'write_ds = 0 stored something'
      assert_bits(dwn, r.dwn, 'dwn (in-pass gradients, beta %d, write_ds %d)' % (beta, write_ds))
      for i in nd.pools:
        assert np.array_equal(wins[i], r.win[i])
      for i in merged:
        assert_bits(g[i], r.gin[i] + p.olds[i] if beta else r.gin[i], 'in-pass gradient %d beta %d write_ds %d' % (i, beta, write_ds))
  # edet_fuse_bwd_input: every input, pooled ones through recorded and recomputed winners
  for i, (mode, _, _) in enumerate(p.ins):
    for win in ([r.win[i], None] if mode == POOL else [None]):
      for beta in (0, 1):
        g = nd.bwd_input(i, r.ds, win, beta)
        assert_bits(g, r.gin[i] + p.olds[i] if beta else r.gin[i], 'bwd_input %d beta %d recorded %s' % (i, beta, win is not None))


# ---------------------------------------------------------------------------------------- swish problems
def device_weights(variables, method):
  """edet_fuse_weights of scalar variables [nin, 1] -> float32 [nin, 1] (numpy) and the device tensors of the variables."""
  nin = len(variables)
  wd = [gu.fdev(torch.tensor([float(v)])) for v in np.asarray(variables).reshape(-1)] + [None] * (3 - nin)
  wn = torch.zeros(4, dtype=torch.float32, device=gu.DEV)
  call('edet_fuse_weights', ptr(wd[0]), ptr(wd[1]), ptr(wd[2]), nin, method, ptr(wn), 1, gu.stream())
  torch.cuda.synchronize()
  return wn[:nin].cpu().numpy().reshape(nin, 1), wd


@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('name', sorted(fb.SWISH))
def test_swish_problems_inside_the_bounds(name, dt):
  """Forward and ds elementwise inside fwd_bound / ds_bound of the float64 reference evaluated with the device's own
  normalised weights (themselves within the normaliser's ulp budget of THEIR reference), winner bytes equal, weight sums
  within test_fuse's tolerance; every input gradient bit for bit what the float32 restatement makes of the stored ds."""
  storage = dt[0]
  p = fb.swish_problem(name, storage)
  wn, wd = device_weights(p.vars, 0)
  d = fb.normaliser_distance(wn, fb.normalise_ref(p.vars, 0))
  print('%s %s: wn %s, %.3f ulps from the reference' % (name, storage, wn.ravel(), d))
  assert d <= fb.norm_ulps(0)
  r = fb.node_ref(p, wn)
  nd = DevNode(p, dt, 'tight', wn)
  out = nd.fwd()
  bad = fb.violations(out, r.out, fb.fwd_bound(r, p.nin, ACT_SWISH, storage))
  assert not bad.any(), 'out: %d outside the bound, worst ratio %.3f' % (
      int(bad.sum()), float((np.abs(out - r.out) / fb.fwd_bound(r, p.nin, ACT_SWISH, storage)).max()))
  # the raw variables normalised inside the kernel: the same weights, the same output
  wraw = (ctypes.c_void_p * 3)(*[ptr(w) for w in wd])
  out2, wn2 = nd.fwd(wraw=wraw)
  assert fb.same_bits(wn2[:p.nin].cpu().numpy(), wn.reshape(-1)) and fb.same_bits(out2, out)
  ds, dwn, wins, _ = nd.bwd_pre()
  bad = fb.violations(ds, r.ds, fb.ds_bound(p, r, storage))
  assert not bad.any(), 'ds: %d outside the bound, worst ratio %.3f' % (
      int(bad.sum()), float((np.abs(ds - r.ds) / fb.ds_bound(p, r, storage)).max()))
  for i in nd.pools:
    assert np.array_equal(wins[i], r.win[i]), 'winner plane of input %d' % i
  gu.check(torch.from_numpy(dwn.reshape(-1)), torch.from_numpy(f32(r.dwn).reshape(-1)), 'f32', 'dwn %s' % name,
           **wtol(storage, p.shape))
  merged = nd.merged_inputs()
  for beta in (0, 1):
    ds2, _, _, g = nd.bwd_pre(merged=merged, beta=beta)
    assert fb.same_bits(ds2, ds)
    for i, (mode, h, w) in enumerate(p.ins):
      old = f32(p.olds[i]) if beta else None
      for win in ([wins[i], None] if mode == POOL else [None]):
        want = fb.bwd_input_f32(mode, (h, w), ds, wn[i, 0], old, storage, wins.get(i))
        assert_bits(nd.bwd_input(i, ds, win, beta), want, 'bwd_input %d beta %d recorded %s' % (i, beta, win is not None))
      if i in merged:
        assert_bits(g[i], want, 'in-pass gradient %d beta %d' % (i, beta))


# ---------------------------------------------------------------------------------------- activation sweep
F32 = gu.DTYPES[0]
assert F32[0] == 'f32'


def sweep(act, s):
  """(value, derivative) of the activation at the float32 values s through edet_fuse_fwd / edet_fuse_bwd_pre: one
  identity input without an affine, weight 1, fp32 storage, dout = 1 -- the pre-activation is the input itself."""
  s = np.asarray(s, dtype=np.float32)
  m = (s.size + 7) // 8 * 8
  x = np.zeros(m, dtype=np.float32)
  x[:s.size] = s
  p = fb.Problem()
  p.shape, p.ins, p.act, p.nin = (1, 1, m // 8, 8), [(ID, 1, m // 8)], act, 1
  p.xs, p.dout, p.olds = [x.reshape(p.shape).astype(np.float64)], np.ones(p.shape), [np.zeros(p.shape)]
  p.scs, p.shs = [np.ones(8)], [np.zeros(8)]
  nd = DevNode(p, F32, 'tight', np.ones((1, 1)))
  nd.tvs[0].scale = nd.tvs[0].shift = None
  val = nd.fwd().reshape(-1)[:s.size]
  grad = nd.bwd_pre(dwn=False)[0].reshape(-1)[:s.size]
  return val, grad


SWEPT = [(ACT_SWISH, 'swish'), (ACT_HSWISH, 'hswish'), (ACT_MISH, 'mish'), (ACT_SRELU, 'srelu')]


@pytest.mark.parametrize('act', SWEPT, ids=lambda a: a[1])
def test_activation_sweep_dense(act):
  """|s| <= 16 on a grid of 1/256: value and derivative within the measured ulp budgets (this is where they are measured:
  the figures are printed before they are asserted)."""
  act, label = act
  s = fb.SWEEP_GRID
  val, grad = sweep(act, s)
  dv = fb.ulp_distance(val, fb.act_ref(act, s), at=np.maximum(fb.act_mag(act, s), fb.TINY))
  dg = fb.ulp_distance(grad, fb.act_grad_ref(act, s), at=np.maximum(fb.act_grad_mag(act, s), fb.TINY))
  print('MEASURED %s value %.4f ulps at s = %r; derivative %.4f ulps at s = %r' % (
      label, dv.max(), s[dv.argmax()], dg.max(), s[dg.argmax()]))
  assert np.isfinite(val).all() and np.isfinite(grad).all()
  assert float(dv.max()) <= fb.act_value_ulps(act), (float(dv.max()), float(s[dv.argmax()]))
  assert float(dg.max()) <= fb.act_grad_ulps(act), (float(dg.max()), float(s[dg.argmax()]))


@pytest.mark.parametrize('act', SWEPT + [(ACT_RELU, 'relu'), (ACT_RELU6, 'relu6')], ids=lambda a: a[1])
def test_activation_sweep_wide(act):
  """[-100, 100] with +-0, +-3, 6, 20 and tiny positive values: finite, the right sign, the derivative exact at the
  kinks, |got - ref| <= 2^-10 |ref| + 2^-126 max(1, |s|)."""
  act, label = act
  s = fb.SWEEP_WIDE
  val, grad = sweep(act, s)
  rv, rg = fb.act_ref(act, s), fb.act_grad_ref(act, s)
  assert np.isfinite(val).all() and np.isfinite(grad).all()
  okv, okg = fb.wide_ok(val, rv, s), fb.wide_ok(grad, rg, s)
  print('WIDE %s: value misses at s = %r (got %r, want %r); derivative misses at s = %r (got %r, want %r)' % (
      label, s[~okv][:8], val[~okv][:8], rv[~okv][:8], s[~okg][:8], grad[~okg][:8], rg[~okg][:8]))
  assert okv.all() and okg.all()
  assert not (val * rv < 0).any() and not (grad * rg < 0).any()
  at = lambda x: grad[np.flatnonzero(s == x)]
  if act == ACT_RELU:
    assert (at(0.0) == 0).all() and (at(2.0 ** -126) == 1).all()
  if act == ACT_RELU6:
    assert (at(0.0) == 0).all() and (at(6.0) == 0).all() and (at(3.0) == 1).all() and (at(2.0 ** -126) == 1).all()
  if act == ACT_HSWISH:
    assert (at(-3.0) == 0).all() and (at(3.0) == 1).all() and (at(0.0) == 0.5).all()
  if act == ACT_SRELU:
    assert (at(0.0) == 0).all() and (val[s <= 0] == 0).all()
  if act == ACT_SWISH:
    assert (at(0.0) == 0.5).all() and (val[s == 0] == 0).all()


# ---------------------------------------------------------------------------------------- normalisers
def tiny_node(nin, storage_dt, wn):
  """nin identity inputs of 2x2x8 small integers, no activation: exact weight sums to feed the normalisers' backward."""
  rng = np.random.default_rng(gu.seed_of('fuse_norm', nin))
  p = fb.Problem()
  p.shape, p.ins, p.act, p.nin = (1, 2, 2, 8), [(ID, 2, 2)] * nin, ACT_NONE, nin
  p.xs = [rng.integers(-4, 5, p.shape).astype(np.float64) for _ in range(nin)]
  p.scs, p.shs = [np.ones(8)] * nin, [np.zeros(8)] * nin
  p.dout = rng.integers(-4, 5, p.shape).astype(np.float64)
  p.olds = [np.zeros(p.shape)] * nin
  return p, DevNode(p, storage_dt, 'tight', wn)


@pytest.mark.parametrize('case', range(len(fb.NORM_EDGE)), ids=lambda k: '%s-%s' % ({0: 'fastattn', 2: 'softmax'}[fb.NORM_EDGE[k][0]], 'x'.join('%g' % v for v in fb.NORM_EDGE[k][1])))
def test_normaliser_edges_scalar(case):
  """edet_fuse_weights, the in-kernel path of edet_fuse_fwd (same bits), edet_fuse_weights_bwd and the folded path of
  edet_fuse_bwd_pre (same bits) on scalar variables, against the float64 reference within the measured ulp budgets;
  exact zeros where the reference has exact zeros."""
  method, ws = fb.NORM_EDGE[case]
  ws = np.array(ws, dtype=np.float32).astype(np.float64).reshape(-1, 1)
  nin = len(ws)
  wn, wd = device_weights(ws, method)
  ref = fb.normalise_ref(ws, method)
  d = fb.normaliser_distance(wn, ref)
  print('MEASURED normaliser method %d %s: %.4f ulps' % (method, ws.ravel(), d))
  assert np.isfinite(wn).all()
  assert (wn[ref == 0] == 0).all()
  if method == 2 and len(set(ws.ravel().tolist())) == 1:
    assert (wn == np.float32(1.0 / nin)).all()
  p, nd = tiny_node(nin, F32, wn)
  wraw = (ctypes.c_void_p * 3)(*[ptr(w) for w in wd])
  _, wn2 = nd.fwd(wraw=wraw, method=method)
  assert fb.same_bits(wn2[:nin].cpu().numpy(), wn.reshape(-1))
  dws2 = [torch.zeros(1, dtype=torch.float32, device=gu.DEV) for _ in range(3)]
  dwraw = (ctypes.c_void_p * 3)(*[ptr(t) for t in dws2])
  _, dwn, _, _ = nd.bwd_pre(wraw=wraw, dwraw=dwraw, method=method)
  assert_bits(dwn, fb.node_ref(p, wn).dwn, 'dwn of the tiny node')
  dwn_d = torch.zeros(4, dtype=torch.float32, device=gu.DEV)
  dwn_d[:nin] = torch.from_numpy(dwn.reshape(-1)).to(gu.DEV)
  dws = [torch.zeros(1, dtype=torch.float32, device=gu.DEV) for _ in range(3)]
  call('edet_fuse_weights_bwd', ptr(wd[0]), ptr(wd[1]), ptr(wd[2]), nin, method, ptr(dwn_d), ptr(dws[0]), ptr(dws[1]),
       ptr(dws[2]), 1, gu.stream())
  torch.cuda.synchronize()
  dw = torch.cat(dws[:nin]).cpu().numpy()
  assert fb.same_bits(torch.cat(dws2[:nin]).cpu().numpy(), dw), 'folded gradient of the variables'
  want, mag = fb.normalise_bwd_ref(ws, method, dwn.astype(np.float64))
  d = fb.normaliser_bwd_distance(dw, want, mag)
  print('MEASURED normaliser backward method %d %s: %.4f ulps (dw %s, want %s)' % (method, ws.ravel(), d, dw, want.ravel()))
  assert np.isfinite(dw).all() and d <= fb.norm_bwd_ulps(method)
  assert fb.normaliser_distance(wn, ref) <= fb.norm_ulps(method)
  assert (dw.reshape(-1, 1)[(ws <= 0) & (method == 0)] == 0).all()


@pytest.mark.parametrize('method', [0, 2], ids=['fastattn', 'softmax'])
@pytest.mark.parametrize('nin', [2, 3])
def test_normaliser_edges_per_channel(method, nin):
  """The per-channel form: the scalar cases side by side, one per channel -- the same bits as the scalar calls."""
  cases = [ws for m, ws in fb.NORM_EDGE if m == method and len(ws) == nin]
  wc = len(cases)
  cols = np.array(cases, dtype=np.float32).T.copy()      # [nin, wc]
  wd = [gu.fdev(torch.from_numpy(cols[i])) for i in range(nin)] + [None] * (3 - nin)
  wn = torch.full((3 * wc + 8,), NAN, dtype=torch.float32, device=gu.DEV)
  call('edet_fuse_weights', ptr(wd[0]), ptr(wd[1]), ptr(wd[2]), nin, method, ptr(wn), wc, gu.stream())
  dwn = np.array([[3.0], [-2.0], [0.75]])[:nin] * np.ones((1, wc))
  dwn_d = gu.fdev(torch.from_numpy(dwn.astype(np.float32).reshape(-1)))
  dws = [torch.zeros(wc, dtype=torch.float32, device=gu.DEV) for _ in range(3)]
  call('edet_fuse_weights_bwd', ptr(wd[0]), ptr(wd[1]), ptr(wd[2]), nin, method, ptr(dwn_d), ptr(dws[0]), ptr(dws[1]),
       ptr(dws[2]), wc, gu.stream())
  torch.cuda.synchronize()
  assert bool(torch.isnan(wn[nin * wc:]).all())
  got = wn[:nin * wc].cpu().numpy().reshape(nin, wc)
  dw = torch.stack(dws[:nin]).cpu().numpy()
  ref = fb.normalise_ref(cols.astype(np.float64), method)
  want, mag = fb.normalise_bwd_ref(cols.astype(np.float64), method, dwn)
  d, db = fb.normaliser_distance(got, ref), fb.normaliser_bwd_distance(dw, want, mag)
  print('MEASURED per-channel normaliser method %d nin %d: %.4f ulps, backward %.4f ulps' % (method, nin, d, db))
  assert d <= fb.norm_ulps(method) and db <= fb.norm_bwd_ulps(method)
  assert (got[ref == 0] == 0).all() and (dw[want == 0] == 0).all()
  for k, ws in enumerate(cases):
    one, wd1 = device_weights(np.array(ws).reshape(-1, 1), method)
    assert fb.same_bits(one.reshape(-1), got[:, k]), ws
    d1 = gu.fdev(torch.from_numpy(np.concatenate([dwn[:, k], np.zeros(4 - nin)]).astype(np.float32)))
    dws1 = [torch.zeros(1, dtype=torch.float32, device=gu.DEV) for _ in range(3)]
    call('edet_fuse_weights_bwd', ptr(wd1[0]), ptr(wd1[1]), ptr(wd1[2]), nin, method, ptr(d1), ptr(dws1[0]), ptr(dws1[1]),
         ptr(dws1[2]), 1, gu.stream())
    torch.cuda.synchronize()
    assert fb.same_bits(torch.cat(dws1[:nin]).cpu().numpy(), dw[:, k]), ws
