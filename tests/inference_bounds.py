"""What tests/test_gpu_inference_kernels.py (device) and tests/test_inference_kernel_bounds.py (CPU) share: the comparison
helpers of the inference-only kernels -- a componentwise error bound for the fp32-output GEMM, an ulp distance, an
"is not bf16-representable" predicate -- and the seeded problems they are applied to, each with its float64 reference,
built once per process.  Nothing here touches the device."""
import functools

import numpy as np
import torch

from automl_amd._lib import ACT_NONE, ACT_RELU6, ACT_SWISH
from tests import gpu_util as gu
from tests.test_gpu_kernels import apply_view, off_kinks

# ---------------------------------------------------------------------------------------- comparison helpers
U32 = 2.0 ** -23        # one unit in the last place of a float32 in [1, 2): an upper bound of ANY rounding of one operation


def f64(t):
  return np.asarray(t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)


def gemm_bound(mag, k):
  """Componentwise bound of out = sum_k a_ik w_kj + bias_j computed with exact products (bf16 x bf16 fits a float32) and
  fp32 additions in any order and with any rounding (to nearest or truncating: at most one ulp each): the K - 1
  accumulations and the bias add give |err| <= ((1 + u)^K - 1) mag <= (K + 2) u mag for K u << 1, u = 2^-23,
  mag = sum_k |a_ik| |w_kj| + |bias_j|."""
  return (k + 2) * U32 * f64(mag)


def gemm_violations(got, ref, mag, k):
  """Boolean array: the elements of `got` (float32) outside gemm_bound of the float64 reference (a NaN is outside)."""
  err = np.abs(f64(got) - f64(ref))
  return ~(err <= gemm_bound(mag, k))


def gemm_accepts(got, ref, mag, k):
  return not bool(gemm_violations(got, ref, mag, k).any())


def ulp32(x):
  """The float32 spacing at |x|, as float64 (x: float64 reference values)."""
  return np.spacing(np.abs(f64(x)).astype(np.float32)).astype(np.float64)


def ulp_distance(got, ref, at=None):
  """|got - ref| in float32 ulps of `at` (default: of the reference itself); got float32, ref float64."""
  ref = f64(ref)
  return np.abs(f64(got) - ref) / ulp32(ref if at is None else at)


def not_bf16(x):
  """Boolean array: the float32 elements whose low 16 bits are not zero, i.e. that bf16 does not represent."""
  x = x.detach().cpu().contiguous() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
  assert x.dtype == torch.float32, x.dtype
  return ((x.view(torch.int32) & 0xffff) != 0).numpy()


def frac_not_bf16(x):
  return float(not_bf16(x).mean())


MIN_FRAC_NOT_BF16 = 0.9


def is_bf16_integer(t):
  t = t.detach().cpu().float()
  return bool((t == t.round()).all()) and bool((t.to(torch.bfloat16).float() == t).all())


# ---------------------------------------------------------------------------------------- edet_pw_fwd_f32out problems
# (n, h, w, cin, cout)
PW_SHAPES = [
    (2, 5, 5, 64, 810),     # d0 head: M = 50 < 128, seven column tiles, the last 42 wide, padding columns 810..815
    (1, 1, 1, 64, 810),     # M = 1: the top pyramid level of a small image
    (1, 16, 8, 88, 810),    # M = 128 exactly; K = 88 leaves a reduction tail of 24
    (1, 43, 3, 112, 36),    # M = 129; N = 36 gives ldo 40, a single ragged column tile
    (3, 7, 9, 160, 9),      # one class: N = 9, ldo 16
    (2, 10, 10, 224, 24),   # K = 224: four reduction steps with a ragged last one
    (1, 3, 3, 8, 8),        # the smallest K and N the envelope allows
    (1, 362, 363, 8, 8),    # M = 131406: more row tiles than EDET_MAX_PARTS, two row tiles per workgroup; output 4 MB
]
PW_BIG_M = PW_SHAPES[7]
PW_EXACT_SHAPES = PW_SHAPES[:7]
PW_MODE_SHAPES = [PW_SHAPES[0], PW_SHAPES[2], PW_SHAPES[3]]      # the modes besides 'plain'
PW_OTHER_MODES = ['plain_nobias', 'bn_swish', 'bn_relu6', 'bn_swish_gate']
PW_PLAIN_MODES = ('plain', 'plain_nobias')
PW_CASES = [(s, 'plain') for s in PW_SHAPES] + [(s, m) for s in PW_MODE_SHAPES for m in PW_OTHER_MODES]
PW_LDO4_SHAPES = [PW_SHAPES[0], PW_SHAPES[3]]      # ldo = pad8(N) + 4


class PwProblem(object):
  """x [n,h,w,cin], wk [cin,cout] (fp32 holding bf16 values), bias / scale / shift / gate fp32 or None, act;
  want [M,cout] float64: view in float64, activated operand rounded to bf16, matmul and bias add in float64;
  mag [M,cout] float64 = sum_k |a_ik| |w_kj| + |bias_j|."""


@functools.lru_cache(maxsize=None)
def pw_problem(shape, mode, exact=False):
  n, h, w, cin, cout = shape
  bf = torch.bfloat16
  rng = np.random.default_rng(gu.seed_of(('pw_f32out', shape, mode, exact)))
  p = PwProblem()
  p.shape, p.mode, p.exact = shape, mode, exact
  p.scale = p.shift = p.gate = None
  p.act = ACT_NONE
  if exact:
    assert mode == 'plain'
    p.x = torch.from_numpy(rng.integers(-8, 9, (n, h, w, cin)).astype(np.float32))
    p.wk = torch.from_numpy(rng.integers(-4, 5, (cin, cout)).astype(np.float32))
    p.bias = torch.from_numpy(rng.integers(-64, 65, cout).astype(np.float32))
  else:
    # the operands rounded to bf16 as test_pw_fwd does: the device and the reference see the same values
    p.x = gu.rnd(rng, (n, h, w, cin), bf)
    p.wk = gu.rnd(rng, (cin, cout), bf, 1.0 / np.sqrt(cin))
    p.bias = None if mode == 'plain_nobias' else torch.from_numpy(rng.standard_normal(cout).astype(np.float32))
  if mode.startswith('bn_'):
    p.scale = torch.from_numpy((1 + 0.3 * rng.standard_normal(cin)).astype(np.float32))
    p.shift = torch.from_numpy((0.3 * rng.standard_normal(cin)).astype(np.float32))
    p.act = ACT_RELU6 if mode == 'bn_relu6' else ACT_SWISH
    # off_kinks adds 0.25, which bf16 does not hold exactly next to a small x: round again, until nothing moves
    for _ in range(4):
      moved = off_kinks(p.x, p.scale, p.shift, p.act).to(bf).float()
      if torch.equal(moved, p.x):
        break
      p.x = moved
    assert torch.equal(off_kinks(p.x, p.scale, p.shift, p.act), p.x) and torch.equal(p.x.to(bf).float(), p.x)
  if mode == 'bn_swish_gate':
    p.gate = torch.from_numpy(rng.uniform(0.2, 1.0, (n, cin)).astype(np.float32))
  d = lambda t: None if t is None else t.double()
  a = apply_view(d(p.x), d(p.scale), d(p.shift), p.act, d(p.gate))
  a = a.to(bf).double().reshape(-1, cin)
  b = torch.zeros(cout, dtype=torch.float64) if p.bias is None else p.bias.double()
  p.want = (a @ p.wk.double() + b).numpy()
  p.mag = (a.abs() @ p.wk.double().abs() + b.abs()).numpy()
  p.M, p.K, p.N = n * h * w, cin, cout
  return p


# ---------------------------------------------------------------------------------------- edet_bn_eval problems
BN_CHANNELS = (8, 24, 127, 128, 129, 3840)
BN_EPS = (1e-3, 1e-4)
# |scale - ref| <= BN_EVAL_ULPS float32 ulps of ref, |shift - ref| <= BN_EVAL_ULPS ulps of |beta| + |mm * scale|.
# Twice the largest distance of the device's scale from the float64 reference over these inputs, measured on an MI355X
# (gamma * rsqrtf(mv + eps): a 1-ulp reciprocal square root and one rounded product): 1.727 ulps, at c = 3840 and eps = 1e-4
# (1.538 at eps = 1e-3; the shift: 1.804).  The bound: 3.46 ulps.  8 is the most it may ever be; above that is a finding.
BN_EVAL_MEASURED_ULPS = 1.73
BN_EVAL_ULPS = 2 * BN_EVAL_MEASURED_ULPS
BN_EVAL_ULPS_CAP = 8.0


class BnProblem(object):
  """gamma, beta, mm, mv: float32 arrays [c]."""


@functools.lru_cache(maxsize=None)
def bn_problem(c, eps):
  rng = np.random.default_rng(gu.seed_of(('bn_eval', c, eps)))
  p = BnProblem()
  p.c, p.eps = c, eps
  p.gamma = rng.standard_normal(c).astype(np.float32)
  p.beta = rng.standard_normal(c).astype(np.float32)
  p.mm = (3 * rng.standard_normal(c)).astype(np.float32)
  # moving variance: exact 0 / inside [0, 10 eps], where eps matters / near 1 / up to 1e4 -- every kind in every problem
  kind = np.arange(c) % 4
  rng.shuffle(kind)
  mv = np.where(kind == 0, 0.0,
                np.where(kind == 1, rng.uniform(0, 10 * eps, c),
                         np.where(kind == 2, rng.uniform(0.5, 2.0, c), 10.0 ** rng.uniform(0, 4, c))))
  p.mv = mv.astype(np.float32)
  p.kind = kind
  return p


def bn_eval_ref(p, eps=None):
  """(scale, shift) in float64: scale = gamma / sqrt(float32(mv + eps)), shift = beta - mm * scale."""
  eps = np.float32(p.eps if eps is None else eps)
  scale = p.gamma.astype(np.float64) / np.sqrt((p.mv + eps).astype(np.float32).astype(np.float64))
  return scale, p.beta.astype(np.float64) - p.mm.astype(np.float64) * scale


def bn_eval_distances(scale, shift, p, ref=None):
  """Largest ulp distances (scale, shift) of float32 results from the float64 reference of problem p."""
  rs, rh = bn_eval_ref(p) if ref is None else ref
  at = np.abs(p.beta.astype(np.float64)) + np.abs(p.mm.astype(np.float64) * rs)
  return float(ulp_distance(scale, rs).max()), float(ulp_distance(shift, rh, at=at).max())


def bn_eval_accepts(scale, shift, p, ulps=BN_EVAL_ULPS, ref=None):
  ds, dh = bn_eval_distances(scale, shift, p, ref)
  return ds <= ulps and dh <= ulps
