"""-m gpu: the kernels only the bf16 inference forward (and the plan / cast plumbing around it) runs, each called through
the C ABI against a float64 reference of the same operation: edet_pw_fwd_f32out (the class logits of every bf16 inference
pass), edet_bn_eval, edet_cast_batch, edet_compact_rows.  The comparison helpers and the seeded problems live in
tests/inference_bounds.py; tests/test_inference_kernel_bounds.py shows on the CPU that they reject damaged results."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from automl_amd import _lib
from automl_amd._lib import EDET_BF16, EDET_F32, EdetError, call, ptr
from tests import gpu_util as gu
from tests import inference_bounds as ib

pytestmark = pytest.mark.gpu

NP = ctypes.c_int
BF16, F32 = torch.bfloat16, torch.float32
# quiet NaNs with a payload: nothing a kernel computes from these inputs has these bits
CANARY = {F32: (torch.int32, 0x7fc0dead), BF16: (torch.int16, 0x7fc1)}


def canary(shape, tdt):
  idt, bits = CANARY[tdt]
  return torch.full(shape, bits, dtype=idt, device=gu.DEV).view(tdt)


def bits_of(t):
  return t.contiguous().view(CANARY[t.dtype][0])


def is_canary(t):
  return t.numel() == 0 or bool((bits_of(t) == CANARY[t.dtype][1]).all())


def same_bits(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits_of(a.cpu()), bits_of(b.cpu())))


def ids_shape(s):
  return 'x'.join(map(str, s))


# ------------------------------------------------------------------------------------ edet_pw_fwd_f32out
class PwDevice(object):
  """The device operands of an ib.PwProblem: bf16 input view, the transposed bf16 compute copy of the weight, fp32 bias."""

  def __init__(self, p):
    self.p = p
    n, h, w, cin, cout = p.shape
    self.xd = gu.to_dev(p.x, BF16)
    self.ldk = gu.pad8(cin)
    self.wt = torch.zeros(cout, self.ldk, dtype=BF16, device=gu.DEV)
    call('edet_cast_matrix', ptr(gu.fdev(p.wk)), ptr(self.wt), cin, cout, self.ldk, 1, EDET_BF16, gu.stream())
    self.bias = gu.fdev(p.bias)
    self.tv = gu.tview(self.xd, cin, gu.fdev(p.scale), gu.fdev(p.shift), gu.fdev(p.gate), p.act)

  def f32out(self, ldo=None, out=None):
    """-> out [M + 3][ldo] fp32, NaN canary before the call, and the launch log of the call."""
    p = self.p
    ldo = ldo or gu.pad8(p.N)
    out = canary((p.M + 3, ldo), F32) if out is None else out
    _lib.launch_log_start()
    try:
      call('edet_pw_fwd_f32out', ctypes.byref(self.tv), ptr(self.wt), self.ldk, ptr(self.bias), ptr(out), p.N, ldo, gu.stream())
      torch.cuda.synchronize()
    finally:
      log = _lib.launch_log_stop()
    return out, log

  def bf16out(self):
    """The same layer through edet_pw_fwd (bf16 output) -> out [M][pad8(N)] bf16 and the launch log."""
    p = self.p
    ldo = gu.pad8(p.N)
    out = canary((p.M, ldo), BF16)
    npart = NP(0)
    _lib.launch_log_start()
    try:
      call('edet_pw_fwd', ctypes.byref(self.tv), ptr(self.wt), self.ldk, ptr(self.bias), ptr(out), p.N, ldo, None,
           ctypes.byref(npart), EDET_BF16, gu.stream())
      torch.cuda.synchronize()
    finally:
      log = _lib.launch_log_stop()
    return out, log


def check_layout(out, p, ldo):
  """Rows >= M and columns >= pad8(N) keep the canary; the padding columns N .. pad8(N) - 1 of the valid rows are 0.0."""
  n8 = gu.pad8(p.N)
  assert tuple(out.shape) == (p.M + 3, ldo)
  assert is_canary(out[p.M:]), 'rows behind the last one were written'
  assert is_canary(out[:p.M, n8:]), 'columns behind pad8(N) were written'
  assert bool((out[:p.M, p.N:n8] == 0.0).all()), 'padding columns N .. pad8(N) - 1 are not zero'
  assert bool(torch.isfinite(out[:p.M, :p.N]).all())


def ran_big_gemm(log):
  return bool(log) and all('pwb::k_big_gemm<' in k for k in log)


@pytest.mark.parametrize('shape', ib.PW_EXACT_SHAPES, ids=ids_shape)
def test_pw_fwd_f32out_exact_integers(shape):
  """Small integer operands (inputs in [-8, 8], weights in [-4, 4], bias in [-64, 64]): every product and every partial sum
  is an integer below 2^24 (tests/test_inference_kernel_bounds.py), so the output equals the reference bit for bit."""
  p = ib.pw_problem(shape, 'plain', True)
  out, log = PwDevice(p).f32out()
  assert ran_big_gemm(log), sorted(log)
  check_layout(out, p, gu.pad8(p.N))
  want = torch.from_numpy(p.want.astype(np.float32))
  got = out[:p.M, :p.N].cpu()
  bad = (bits_of(got) != bits_of(want))
  assert not bool(bad.any()), '%d of %d elements differ, first at %s' % (int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())


@pytest.mark.parametrize('case', ib.PW_CASES, ids=lambda c: '%s-%s' % (ids_shape(c[0]), c[1]))
def test_pw_fwd_f32out(case, monkeypatch):
  """Random operands.  Plain views: |got - ref| <= (K + 2) 2^-23 (sum_k |a_ik| |w_kj| + |bias_j|) per element
  (ib.gemm_bound: derived, not measured).  Every mode: the output rounded to bf16 equals, bit for bit, what the bf16-output
  instantiation of the same kernel stores (both epilogues form acc + bias from the same accumulators; the bf16 one rounds
  it once); at least 90 % of the elements are not bf16-representable; the layout; the usual bf16 tolerance against the
  float64 reference as the anchor of the activated modes."""
  shape, mode = case
  p = ib.pw_problem(shape, mode)
  dev = PwDevice(p)
  out, log = dev.f32out()
  assert ran_big_gemm(log), sorted(log)
  check_layout(out, p, gu.pad8(p.N))
  got = out[:p.M, :p.N].cpu()
  want = torch.from_numpy(p.want)
  gu.check(got, want, 'bf16', 'pw_fwd_f32out %s %s' % (shape, mode))
  frac = ib.frac_not_bf16(got)
  if mode in ib.PW_PLAIN_MODES:
    ratio = np.abs(got.double().numpy() - p.want) / np.maximum(ib.gemm_bound(p.mag, p.K), 1e-300)
    print('pw_fwd_f32out %s %s: worst |err| / bound %.4f, not bf16-representable %.4f' % (shape, mode, float(ratio.max()), frac))
    v = ib.gemm_violations(got.numpy(), p.want, p.mag, p.K)
    assert not v.any(), '%d of %d elements outside the bound, worst |err| / bound %.3f, first at %s' % (
        int(v.sum()), v.size, float(ratio.max()), np.argwhere(v)[0].tolist())
  assert frac >= ib.MIN_FRAC_NOT_BF16, 'only %.3f of the outputs are not bf16-representable' % frac
  # the tested bf16-output kernel on the same inputs (the register-staged workgroup-tiled one: same tile, same order)
  monkeypatch.setenv('EDET_PW_IMPL', 'big')
  monkeypatch.setenv('EDET_PW_GLDS', '0')
  out16, log16 = dev.bf16out()
  assert ran_big_gemm(log16), sorted(log16)
  diff = bits_of(out16[:, :p.N].cpu()) != bits_of(got.to(BF16))
  assert not bool(diff.any()), '%d of %d elements of the bf16 output are not the rounded fp32 output, first at %s' % (
      int(diff.sum()), diff.numel(), diff.nonzero()[0].tolist())


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
@pytest.mark.parametrize('shape', ib.PW_LDO4_SHAPES, ids=ids_shape)
def test_pw_fwd_f32out_row_stride_of_four(shape, exact):
  """ldo = pad8(N) + 4, which the ldo % 4 rule allows: the same values, and the four floats behind pad8(N) of every row keep
  the canary."""
  p = ib.pw_problem(shape, 'plain', exact)
  dev = PwDevice(p)
  ldo = gu.pad8(p.N) + 4
  out, _ = dev.f32out(ldo)
  check_layout(out, p, ldo)
  if exact:
    assert same_bits(out[:p.M, :p.N], torch.from_numpy(p.want.astype(np.float32)))
  else:
    assert ib.gemm_accepts(out[:p.M, :p.N].cpu().numpy(), p.want, p.mag, p.K)
    dense, _ = dev.f32out()
    assert same_bits(out[:p.M, :p.N], dense[:p.M, :p.N])


@pytest.mark.parametrize('what', ['in->c % 8 != 0', 'ldo % 4 != 0', 'ldo < pad8(N)', 'null out'])
def test_pw_fwd_f32out_refusals(what):
  p = ib.pw_problem(ib.PW_SHAPES[3], 'plain')      # N = 36, pad8(N) = 40
  dev = PwDevice(p)
  out = canary((p.M + 3, 48), F32)
  tv, ldo, dst = dev.tv, 40, out
  if what == 'in->c % 8 != 0':
    tv = gu.tview(dev.xd, p.K - 4)
  elif what == 'ldo % 4 != 0':
    ldo = 42
  elif what == 'ldo < pad8(N)':
    ldo = 36
  else:
    dst = None
  with pytest.raises(EdetError, match='edet_pw_fwd_f32out'):
    call('edet_pw_fwd_f32out', ctypes.byref(tv), ptr(dev.wt), dev.ldk, ptr(dev.bias), ptr(dst), p.N, ldo, gu.stream())
  torch.cuda.synchronize()
  assert is_canary(out)


# ------------------------------------------------------------------------------------ the engine takes these paths
def test_engine_inference_takes_the_f32out_and_fp32_island_paths(monkeypatch):
  """efficientdet-d0, 64 x 64 images, batch 2, bf16 storage, inference: the class-predict pointwise of each of the five
  pyramid levels runs through edet_pw_fwd_f32out with 810 columns, the box-predict pointwise through edet_pw_fwd with
  dtype EDET_F32 (the fp32 island); both logits come back as fp32 and the class logits were not rounded to bf16.  (Accuracy
  against the oracle: tests/test_gpu_network.py.)"""
  from automl_amd import efficientdet_net, engine as engine_lib, hparams_config, layer_engine
  from oracle.problems import perturbed_params
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  calls = []

  def counting(name, *args, **kw):
    calls.append((name, args))
    return call(name, *args, **kw)
  assert layer_engine.call is call and engine_lib.call is call
  monkeypatch.setattr(layer_engine, 'call', counting)
  monkeypatch.setattr(engine_lib, 'call', counting)
  rng = np.random.default_rng(17)
  images = torch.from_numpy(rng.standard_normal((2, 64, 64, 3)).astype(np.float32)).to(BF16).float()
  net = efficientdet_net.EfficientDetNet(config=config, dtype='bf16', params=perturbed_params(config, 3))
  net(images, training=False)
  torch.cuda.synchronize()
  cls, box = net.engine.outputs()
  f32out = [a for n, a in calls if n == 'edet_pw_fwd_f32out']
  assert len(f32out) == 5 and all(a[5] == 810 for a in f32out), [a[5] for a in f32out]
  island = [a for n, a in calls if n == 'edet_pw_fwd' and a[9] == EDET_F32]
  assert len(island) == 5 and all(a[5] == 36 for a in island), [a[5] for a in island]
  assert len(cls) == 5 and len(box) == 5
  sizes = [8, 4, 2, 1, 1]
  for lvl, (c, b) in enumerate(zip(cls, box)):
    assert c.dtype == torch.float32 and b.dtype == torch.float32
    assert tuple(c.shape) == (2, sizes[lvl], sizes[lvl], 810) and tuple(b.shape) == (2, sizes[lvl], sizes[lvl], 36)
    assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(b).all())
    frac = ib.frac_not_bf16(c.contiguous())
    assert frac >= ib.MIN_FRAC_NOT_BF16, 'level %d: only %.3f of the class logits are not bf16-representable' % (lvl, frac)


# ------------------------------------------------------------------------------------ edet_bn_eval
@pytest.mark.parametrize('eps', ib.BN_EPS)
@pytest.mark.parametrize('c', ib.BN_CHANNELS)
def test_bn_eval(c, eps):
  """scale = gamma / sqrt(mv + eps), shift = beta - mm * scale against float64, in float32 ulps (shift: of |beta| +
  |mm * scale|).  Measured on an MI355X over these inputs: the scale is at most 1.727 ulps from the reference (c = 3840,
  eps = 1e-4), the shift 1.804; the bound is twice the former, 3.46 ulps (ib.BN_EVAL_ULPS), and may never exceed 8.  A
  reference with eps 1e-4 for 1e-3 rejects the device's result."""
  p = ib.bn_problem(c, eps)
  scale, shift = canary((c + 16,), F32), canary((c + 16,), F32)
  dev = [gu.fdev(torch.from_numpy(a)) for a in (p.gamma, p.beta, p.mm, p.mv)]
  call('edet_bn_eval', c, ptr(dev[0]), ptr(dev[1]), eps, ptr(dev[2]), ptr(dev[3]), ptr(scale), ptr(shift), gu.stream())
  torch.cuda.synchronize()
  assert is_canary(scale[c:]) and is_canary(shift[c:]), 'written behind channel c'
  sc, sh = scale[:c].cpu().numpy(), shift[:c].cpu().numpy()
  ds, dh = ib.bn_eval_distances(sc, sh, p)
  print('bn_eval c=%d eps=%g: scale %.3f ulps, shift %.3f ulps from the float64 reference' % (c, eps, ds, dh))
  assert ib.BN_EVAL_ULPS <= ib.BN_EVAL_ULPS_CAP
  assert ds <= ib.BN_EVAL_ULPS and dh <= ib.BN_EVAL_ULPS, (ds, dh, ib.BN_EVAL_ULPS)
  if eps == 1e-3:
    assert not ib.bn_eval_accepts(sc, sh, p, ref=ib.bn_eval_ref(p, eps=1e-4))


# ------------------------------------------------------------------------------------ edet_cast_batch
# (rows, cols, ld_out, transpose): the arguments of edet_cast_matrix
CAST_ITEMS = [(64, 810, 64, 1), (64, 810, 816, 0), (3, 5, 8, 1), (3, 5, 8, 0), (1, 1, 8, 1), (88, 36, 88, 1), (88, 36, 40, 0),
              (1152, 3840, 1152, 1)]     # the last: more elements than 64 x 256 threads, the grid-stride loop
CAST_TAIL = 64


def cast_reference(src, ld, transpose, tdt):
  m = (src.t() if transpose else src).to(tdt)        # round to nearest even
  out = torch.zeros(m.shape[0], ld, dtype=tdt, device=src.device)
  out[:, :m.shape[1]] = m
  return out


@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('max_blocks', [1, 64, 200])
def test_cast_batch(dt, max_blocks):
  """One descriptor table, built as LayerEngine._cast_all builds it (edet_cast_item_t, packed '<QQiiii'): every destination
  equals edet_cast_matrix's and the torch cast, the 64 elements behind it survive, and a second call picks up changed
  sources."""
  name, edt, tdt = dt
  gen = torch.Generator(device=gu.DEV)
  gen.manual_seed(gu.seed_of(('cast_batch', name)))
  srcs = [torch.randn(r, c, generator=gen, device=gu.DEV, dtype=F32) for (r, c, _, _) in CAST_ITEMS]
  srcs[0][0, :4] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], device=gu.DEV)     # ties: to even
  sizes = [(c if t else r) * ld for (r, c, ld, t) in CAST_ITEMS]
  dsts = [canary((sz + CAST_TAIL,), tdt) for sz in sizes]
  raw = b''.join(struct.pack('<QQiiii', s.data_ptr(), d.data_ptr(), r, c, ld, t)
                 for s, d, (r, c, ld, t) in zip(srcs, dsts, CAST_ITEMS))
  assert len(raw) == 32 * len(CAST_ITEMS)
  table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(gu.DEV)
  for attempt in range(2):
    call('edet_cast_batch', ptr(table), len(CAST_ITEMS), max_blocks, edt, gu.stream())
    torch.cuda.synchronize()
    for s, d, sz, (r, c, ld, t) in zip(srcs, dsts, sizes, CAST_ITEMS):
      what = 'item %s, call %d' % ((r, c, ld, t), attempt)
      assert is_canary(d[sz:]), 'written behind the destination: ' + what
      got = d[:sz].view(-1, ld)
      single = canary((sz,), tdt)
      call('edet_cast_matrix', ptr(s), ptr(single), r, c, ld, t, edt, gu.stream())
      torch.cuda.synchronize()
      assert same_bits(got, single.view(-1, ld)), 'differs from edet_cast_matrix: ' + what
      assert same_bits(got, cast_reference(s, ld, t, tdt)), 'differs from the torch cast: ' + what
    for s in srcs:      # the sources change (an optimizer step), the table does not
      s.mul_(-1.7).add_(0.3)


# ------------------------------------------------------------------------------------ edet_compact_rows
# (rows, c, ld, elem_bytes)
COMPACT_CASES = [(50, 810, 816, 2), (50, 810, 816, 4), (1, 36, 40, 4), (7, 2, 8, 2), (131406, 8, 16, 2),
                 (5, 24, 24, 4),      # ld == c: a straight copy
                 (0, 8, 16, 4)]       # no rows: returns 0 and writes nothing


@pytest.mark.parametrize('case', COMPACT_CASES, ids=ids_shape)
def test_compact_rows(case):
  rows, c, ld, eb = case
  idt = torch.int16 if eb == 2 else torch.int32
  info = torch.iinfo(idt)
  gen = torch.Generator(device=gu.DEV)
  gen.manual_seed(gu.seed_of(('compact_rows', case)))
  src = torch.randint(info.min, info.max, (max(rows, 1), ld), generator=gen, device=gu.DEV, dtype=idt)
  src[0, :2] = torch.tensor([0x7fc1, -1] if eb == 2 else [0x7fc0dead, -1], dtype=idt, device=gu.DEV)     # NaN payloads travel as raw bits
  tdt = BF16 if eb == 2 else F32
  dst = canary((rows * c + 64,), tdt)
  call('edet_compact_rows', ptr(src), rows, c, ld, ptr(dst), eb, gu.stream())
  torch.cuda.synchronize()
  assert is_canary(dst[rows * c:]), 'written behind the destination'
  if rows:
    assert bool(torch.equal(bits_of(dst[:rows * c]).view(rows, c), src[:, :c]))


@pytest.mark.parametrize('bad', [(4, 5, 8, 2), (4, 24, 16, 4), (4, 8, 8, 3)],
                         ids=['odd c of 2-byte elements', 'ld < c', 'elem_bytes 3'])
def test_compact_rows_refusals(bad):
  rows, c, ld, eb = bad
  src = torch.zeros(rows * 32, dtype=torch.int32, device=gu.DEV)
  dst = canary((rows * 32,), F32)
  with pytest.raises(EdetError, match='edet_compact_rows'):
    call('edet_compact_rows', ptr(src), rows, c, ld, ptr(dst), eb, gu.stream())
  torch.cuda.synchronize()
  assert is_canary(dst)
