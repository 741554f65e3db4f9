"""The specialised loops of the BiFPN fusion kernels (automl_amd/csrc/fuse.hip): scalar fusion weights and a node shape
{identity.., 2x up-sample} or {identity.., pool}.  Every load of a trip is issued before the arithmetic, the pooled input is
read at clamped addresses, and the backward of a top-down node writes the up-sampled input's gradient itself (a thread then
owns the 2x2 output pixels of a coarse pixel).  Checked against the CPU oracle, bit for bit against the generic body (the
per-channel path fed the same weight in every channel) and for run-to-run identical bytes."""
import ctypes

import numpy as np
import pytest
import torch

from automl_amd import _lib
from automl_amd._lib import ACT_SWISH, call, ptr
from oracle import efficientdet_oracle as orc
from tests import gpu_util as gu
from tests.test_gpu_kernels import resample_oracle

pytestmark = pytest.mark.gpu

ID, UP2, POOL = _lib.RS_IDENTITY, _lib.RS_UP2, _lib.RS_POOL

# (n, oh, ow, c), inputs (mode, h, w).  The three node shapes of a D0 BiFPN; 8 and 40 channels (40: five chunks per pixel do
# not divide the grid's stride, so scale and shift are loaded per trip, not once); maps where every thread runs at most the
# loops' tail; an odd pooled map (padding on one side only); a non-2x up-sample, which takes the generic body.
SMALL = {
    'td64': ((2, 10, 10, 64), [(ID, 10, 10), (UP2, 5, 5)]),
    'bu64': ((2, 5, 5, 64), [(ID, 5, 5), (ID, 5, 5), (POOL, 10, 10)]),
    'top64': ((2, 5, 5, 64), [(ID, 5, 5), (POOL, 10, 10)]),
    'td8': ((2, 10, 10, 8), [(ID, 10, 10), (UP2, 5, 5)]),
    'td40': ((2, 10, 10, 40), [(ID, 10, 10), (UP2, 5, 5)]),
    'bu8': ((2, 5, 5, 8), [(ID, 5, 5), (ID, 5, 5), (POOL, 10, 10)]),
    'bu40': ((2, 5, 5, 40), [(ID, 5, 5), (ID, 5, 5), (POOL, 10, 10)]),
    'bu64odd': ((2, 5, 5, 64), [(ID, 5, 5), (ID, 5, 5), (POOL, 9, 9)]),
    'top40odd': ((2, 5, 5, 40), [(ID, 5, 5), (POOL, 9, 9)]),
    'td64x35': ((2, 70, 70, 64), [(ID, 70, 70), (UP2, 35, 35)]),        # 78400 chunks: more than one workgroup, odd rows
    'bu64x35': ((2, 35, 35, 64), [(ID, 35, 35), (ID, 35, 35), (POOL, 70, 70)]),
    'up5to9': ((2, 9, 9, 64), [(ID, 9, 9), (UP2, 5, 5)]),
}
# 2 x 264 x 264 x 8 = 1 115 136 chunks.  The bf16 kernels run one round of resident workgroups (at most 3 per SIMD: 196 608
# threads), so a thread owns five or six chunks -- two trips of the two-chunk loop of the top-down node and a ragged tail;
# the fp32 kernels run 4096 workgroups (1 048 576 threads): one chunk and, for 66 560 threads, a second one.
BIG = {
    'td64big': ((2, 264, 264, 64), [(ID, 264, 264), (UP2, 132, 132)]),
    'bu64big': ((2, 264, 264, 64), [(ID, 264, 264), (ID, 264, 264), (POOL, 528, 528)]),
}


def exact2x(shape, ins, i):
  return ins[i][0] == UP2 and shape[1] == 2 * ins[i][1] and shape[2] == 2 * ins[i][2]


class Node:
  """One fusion node on the device: inputs with BatchNorm scale / shift, 'fastattn' scalar variables, dout."""

  def __init__(self, dt, shape, ins, seed, on_device=False):
    self.name, self.edt, self.tdt = dt
    self.shape, self.ins, self.nin = shape, ins, len(ins)
    n, oh, ow, c = shape
    rng = np.random.default_rng(seed)
    self.scs = [torch.from_numpy((1 + 0.3 * rng.standard_normal(c)).astype(np.float32)) for _ in ins]
    self.shs = [torch.from_numpy((0.3 * rng.standard_normal(c)).astype(np.float32)) for _ in ins]
    self.ws = [torch.from_numpy(rng.uniform(0.3, 1.5, 1).astype(np.float32)) for _ in ins]
    if on_device:      # the big maps: drawn on the device, no CPU copy
      gen = torch.Generator(device=gu.DEV).manual_seed(seed)
      draw = lambda s: torch.randn(s, device=gu.DEV, generator=gen).to(self.tdt)
      self.xs, self.dout = None, None
      self.xd = [draw((n, h, w, c)) for (_, h, w) in ins]
      self.dd = draw((n, oh, ow, c))
    else:
      self.xs = [gu.rnd(rng, (n, h, w, c), self.tdt) for (_, h, w) in ins]
      self.dout = gu.rnd(rng, (n, oh, ow, c), self.tdt)
      self.xd = [gu.to_dev(x, self.tdt) for x in self.xs]
      self.dd = gu.to_dev(self.dout, self.tdt)
    self.tvs = [gu.tview(x, c, sc, sh) for x, sc, sh in zip(self.xd, self.scs, self.shs)]
    self.tvp = [ctypes.byref(t) for t in self.tvs] + [None] * (3 - self.nin)
    self.modes = (ctypes.c_int * 3)(*([m[0] for m in ins] + [0] * (3 - self.nin)))
    self.wd = [gu.fdev(w) for w in self.ws] + [None] * (3 - self.nin)
    self.wraw = (ctypes.c_void_p * 3)(*[ptr(w) for w in self.wd])
    self.npool = sum(1 for m in ins if m[0] == POOL)
    self.wsp = torch.empty(1 << 20, dtype=torch.float32, device=gu.DEV)      # partial rows of up to 4096 workgroups x [3][c]
    # normalised weights: [3] scalars, and the same value in every channel for the per-channel (generic) path
    self.wn = torch.zeros(4, dtype=torch.float32, device=gu.DEV)
    call('edet_fuse_weights', ptr(self.wd[0]), ptr(self.wd[1]), ptr(self.wd[2]), self.nin, 0, ptr(self.wn), 1, gu.stream())
    self.wn_pc = self.wn[:3].repeat_interleave(c).contiguous()
    self.grad_start = [torch.randn(x.shape, device=gu.DEV, generator=torch.Generator(device=gu.DEV).manual_seed(i)).to(self.tdt)
                       for i, x in enumerate(self.xd)]

  def weights(self, wc):
    return self.wn if wc == 1 else self.wn_pc

  def fwd(self, wc, raw=False):
    n, oh, ow, c = self.shape
    od = torch.full((n, oh, ow, c), float('nan'), dtype=self.tdt, device=gu.DEV)
    wn = torch.full_like(self.wn, float('nan')) if raw else self.weights(wc)
    call('edet_fuse_fwd', self.tvp[0], self.tvp[1], self.tvp[2], self.modes, self.nin, ptr(wn), wc, ACT_SWISH, ptr(od),
         oh, ow, c, self.wraw if raw else None, 0, self.edt, gu.stream())
    torch.cuda.synchronize()
    return (od, wn) if raw else od

  def bwd_pre(self, wc, merged=(), beta=0, write_ds=1, argmax=True, dwraw=False, null_ds=False):
    """Returns ds, dwn, the argmax planes, {i: gin written in-pass} and the raw variables' gradients."""
    n, oh, ow, c = self.shape
    ds = torch.full((n, oh, ow, c), float('nan'), dtype=self.tdt, device=gu.DEV)
    dwn = torch.zeros(max(4, 3 * wc), dtype=torch.float32, device=gu.DEV)
    amax = torch.full((max(self.npool, 1), n, oh, ow, c), 255, dtype=torch.uint8, device=gu.DEV)
    gin = (ctypes.c_void_p * 3)()
    gbeta = (ctypes.c_int * 3)()
    g = {}
    for i in merged:
      g[i] = self.grad_start[i].clone() if beta else torch.full_like(self.xd[i], float('nan'))
      gin[i] = g[i].data_ptr()
      gbeta[i] = beta
    dws = [torch.zeros(1, dtype=torch.float32, device=gu.DEV) for _ in range(3)]
    dwp = (ctypes.c_void_p * 3)(*[ptr(t) for t in dws])
    call('edet_fuse_bwd_pre', self.tvp[0], self.tvp[1], self.tvp[2], self.modes, self.nin, ptr(self.weights(wc)), wc,
         ACT_SWISH, ptr(self.dd), oh, ow, c, None if null_ds else ptr(ds), ptr(dwn), ptr(amax) if (self.npool and argmax) else None,
         gin if merged else None, gbeta if merged else None, write_ds, ptr(self.wsp), self.wsp.numel() * 4,
         self.wraw if dwraw else None, 0, dwp if dwraw else None, self.edt, gu.stream())
    torch.cuda.synchronize()
    return ds, dwn, amax, g, dws

  def bwd_input(self, wc, i, ds, amax=None, beta=0):
    n, oh, ow, c = self.shape
    g = self.grad_start[i].clone() if beta else torch.full_like(self.xd[i], float('nan'))
    call('edet_fuse_bwd_input', ctypes.byref(self.tvs[i]), self.ins[i][0], ptr(self.weights(wc)), wc, i, ptr(ds), oh, ow, c,
         amax.data_ptr() if amax is not None else None, ptr(g), beta, self.edt, gu.stream())
    torch.cuda.synchronize()
    return g

  def oracle(self):
    """out, ds, d(out)/d(normalised weights), the raw variables' gradients and the inputs' gradients (w.r.t. the BatchNorm
    OUTPUT: the engine applies the scale in the BatchNorm backward coefficients), from torch autograd on the CPU."""
    n, oh, ow, c = self.shape
    xq = [x.clone().requires_grad_(True) for x in self.xs]
    wq = [w.clone().requires_grad_(True) for w in self.ws]
    vals = [resample_oracle(x * sc + sh, m[0], oh, ow) for x, sc, sh, m in zip(xq, self.scs, self.shs, self.ins)]
    r = [torch.relu(w) for w in wq]
    tot = sum(r) + 0.0001
    s = sum(v * ri / tot for v, ri in zip(vals, r))
    s.retain_grad()
    out = orc.swish(s)
    out.backward(self.dout)
    dwn = torch.stack([(s.grad * v.detach()).sum() for v in vals])
    return {'out': out.detach(), 'ds': s.grad, 'dwn': dwn, 'dw': [w.grad for w in wq],
            'gx': [x.grad / sc for x, sc in zip(xq, self.scs)]}


def wtol(name, shape):
  """The weight-gradient tolerance of test_fuse (rtol 2e-2 bf16 / 2e-3 fp32, atol 2e-2 / 1e-3), absolute as there on maps
  of test_fuse's size (at most 100 pixels: sums of some 1e4 terms); on the larger maps the sums grow with the map (6e5 to
  7e7 terms) and the same figures are taken relative to the largest of the node's sums."""
  return dict(rtol=2e-2 if name == 'bf16' else 2e-3, atol=2e-2 if name == 'bf16' else 1e-3,
              scale_by_max=shape[1] * shape[2] > 100)


def seed_for(case):
  return gu.seed_of('fuse_fast', case)


def merged_inputs(shape, ins):
  """The inputs whose gradient edet_fuse_bwd_pre writes itself: identities, and the exact 2x up-sample of {identity, up}."""
  m = [i for i, x in enumerate(ins) if x[0] == ID]
  if len(ins) == 2 and ins[0][0] == ID and exact2x(shape, ins, 1):
    m.append(1)
  return m


@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('case', sorted(SMALL))
def test_fuse_fast_matches_the_oracle(dt, case):
  """Forward output, ds, every input gradient (written in-pass with and without accumulation, and by edet_fuse_bwd_input
  from recorded and from recomputed pool winners), d(normalised weights) and the raw variables' gradients.  Tolerances of
  tests/test_gpu_kernels.py::test_fuse: gu.check defaults elementwise, 2e-2 (bf16) / 2e-3 (fp32) on the weight gradients."""
  shape, ins = SMALL[case]
  nd = Node(dt, shape, ins, seed_for(case))
  name = nd.name
  want = nd.oracle()
  wt = wtol(name, shape)
  gu.check(nd.fwd(1), want['out'], name, 'fwd %s' % case)
  od, wn = nd.fwd(1, raw=True)
  gu.check(od, want['out'], name, 'fwd (raw variables) %s' % case)
  assert torch.equal(wn[:nd.nin], nd.wn[:nd.nin])
  ds, dwn, amax, _, dws = nd.bwd_pre(1, dwraw=True)
  gu.check(ds, want['ds'], name, 'ds %s' % case)
  gu.check(dwn[:nd.nin], want['dwn'], 'f32', 'dwn %s' % case, **wt)
  gu.check(torch.cat(dws[:nd.nin]), torch.cat(want['dw']), 'f32', 'dW %s' % case, **wt)
  merged = merged_inputs(shape, ins)
  for beta in (0, 1):
    ds2, dwn2, _, g, _ = nd.bwd_pre(1, merged=merged, beta=beta, write_ds=0)
    assert bool(torch.isnan(ds2.float()).all())                       # write_ds = 0: nothing stored
    gu.check(dwn2[:nd.nin], want['dwn'], 'f32', 'dwn (in-pass gradients) %s' % case, **wt)
    for i in merged:
      start = nd.grad_start[i].float().cpu() if beta else 0
      gu.check(g[i], want['gx'][i] + start, name, 'gin %d beta %d %s' % (i, beta, case))
  plane = 0
  for i, (mode, _, _) in enumerate(ins):
    planes = [None]
    if mode == POOL:
      planes = [amax[plane], None]
      plane += 1
    for am in planes:
      for beta in (0, 1):
        g = nd.bwd_input(1, i, ds, am, beta)
        start = nd.grad_start[i].float().cpu() if beta else 0
        gu.check(g, want['gx'][i] + start, name, 'bwd_input %d beta %d argmax %s %s' % (i, beta, am is not None, case))


@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('case', sorted(SMALL) + sorted(BIG))
def test_fuse_fast_equals_the_generic_body_bit_for_bit(dt, case):
  """The specialised loops (scalar weights) against the generic per-channel path fed the same weight in every channel: the
  arithmetic is the same fmaf chain, so out, ds, the pool winners and every input gradient agree bit for bit; so does the
  up-sampled input's gradient written in-pass with what edet_fuse_bwd_input makes of the stored ds.  The weight sums differ
  in order only (per-channel sums added over the channels: the weight-gradient tolerance of test_fuse)."""
  big = case in BIG
  shape, ins = (BIG if big else SMALL)[case]
  nd = Node(dt, shape, ins, seed_for(case), on_device=big)
  assert torch.equal(nd.fwd(1), nd.fwd(shape[3]))
  ds1, dwn1, am1, _, _ = nd.bwd_pre(1)
  dsc, dwnc, amc, _, _ = nd.bwd_pre(shape[3])
  assert torch.equal(ds1, dsc) and torch.equal(am1, amc)
  assert not bool(torch.isnan(ds1.float()).any())
  gu.check(dwn1[:nd.nin], dwnc[:nd.nin * shape[3]].view(nd.nin, shape[3]).sum(1), 'f32', 'dwn %s' % case,
           **wtol(nd.name, shape))
  merged = merged_inputs(shape, ins)
  ids = [i for i in merged if ins[i][0] == ID]
  for beta in (0, 1):
    _, _, _, g1, _ = nd.bwd_pre(1, merged=merged, beta=beta, write_ds=0)
    _, _, _, gc, _ = nd.bwd_pre(shape[3], merged=ids, beta=beta, write_ds=0)
    for i in merged:
      # (the generic body never writes a resampled input's gradient: that one comes from edet_fuse_bwd_input below)
      ref = gc[i] if i in gc else nd.bwd_input(shape[3], i, dsc, None, beta)
      assert torch.equal(g1[i], ref), 'in-pass gradient %d beta %d' % (i, beta)
      assert torch.equal(g1[i], nd.bwd_input(1, i, ds1, None, beta)), 'in-pass gradient %d beta %d against bwd_input' % (i, beta)
    plane = 0
    for i, (mode, _, _) in enumerate(ins):
      if mode == ID:
        continue
      am = None
      if mode == POOL:
        am = am1[plane]
        plane += 1
      assert torch.equal(nd.bwd_input(1, i, ds1, am, beta), nd.bwd_input(shape[3], i, dsc, am, beta)), (i, beta)
  if not exact2x(shape, ins, nd.nin - 1) and ins[-1][0] == UP2:
    with pytest.raises(_lib.EdetError):      # a non-2x up-sample: its gradient is edet_fuse_bwd_input's alone
      nd.bwd_pre(1, merged=[nd.nin - 1])
  if ins[-1][0] == POOL:
    with pytest.raises(_lib.EdetError):
      nd.bwd_pre(1, merged=[nd.nin - 1])


@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('case', ['td64', 'td40', 'bu64', 'top40odd', 'td64x35', 'bu64x35', 'up5to9', 'td64big'])
def test_fuse_fast_backward_is_bit_reproducible(dt, case):
  """Two runs of every backward call give the same bytes, the fusion-weight sums included (ordered partial rows)."""
  big = case in BIG
  shape, ins = (BIG if big else SMALL)[case]
  nd = Node(dt, shape, ins, seed_for(case), on_device=big)
  merged = merged_inputs(shape, ins)
  runs = []
  for _ in range(2):
    ds, dwn, am, _, dws = nd.bwd_pre(1, dwraw=True)
    _, dwn2, _, g, dws2 = nd.bwd_pre(1, merged=merged, beta=1, write_ds=0, dwraw=True, null_ds=True)      # (no ds, no buffer)
    outs = [ds, dwn, am, dwn2] + dws + dws2 + [g[i] for i in merged]
    plane = 0
    for i, (mode, _, _) in enumerate(ins):
      if mode == POOL:
        outs += [nd.bwd_input(1, i, ds, am[plane], 1), nd.bwd_input(1, i, ds, None, 1)]
        plane += 1
      elif mode == UP2:
        outs.append(nd.bwd_input(1, i, ds, None, 1))
    runs.append(outs)
  for a, b in zip(*runs):
    assert torch.equal(a, b)
