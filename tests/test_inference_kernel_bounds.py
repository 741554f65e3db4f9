"""The checks of tests/test_gpu_inference_kernels.py must have teeth: on the CPU, the comparison helpers of
tests/inference_bounds.py are fed results that have been damaged on purpose and must reject every one of them, and the
inputs of the exact-integer case are shown to make every fp32 partial sum exact."""
import numpy as np
import pytest
import torch

from tests import inference_bounds as ib

HEAD = ib.PW_SHAPES[0]      # (2, 5, 5, 64, 810)


def f32(a):
  return np.asarray(a, dtype=np.float64).astype(np.float32)


def damaged(p):
  """name -> float32 [M, N]: what a subtly wrong kernel would give for problem p (its float64 reference, damaged)."""
  want, n = p.want, p.N
  bias = np.zeros(n) if p.bias is None else p.bias.double().numpy()
  nobias = want - bias
  out = {}
  out['rounded to bf16'] = torch.from_numpy(f32(want)).to(torch.bfloat16).float().numpy()
  out['bias rotated by one column'] = f32(nobias + np.roll(bias, 1))
  tail = bias.copy()
  tail[768:] = 0.0
  out['bias dropped on the last column tile'] = f32(nobias + tail)
  rows = want.copy()
  rows[-1] = rows[-2]
  out['last row repeats the row before it'] = f32(rows)
  return out


@pytest.mark.parametrize('exact', [False, True], ids=['random', 'exact'])
def test_gemm_checks_reject_damaged_results(exact):
  p = ib.pw_problem(HEAD, 'plain', exact)
  good = f32(p.want)
  assert ib.gemm_accepts(good, p.want, p.mag, p.K)       # the float32 cast of the reference itself passes
  for name, bad in damaged(p).items():
    if exact and name == 'rounded to bf16':
      continue      # small integers: nothing to round, and the exact case asserts equality, not the bound
    assert not np.array_equal(bad.view(np.int32), good.view(np.int32)), name      # the bit-for-bit assertion of the exact case
    assert not ib.gemm_accepts(bad, p.want, p.mag, p.K), name                     # the bound of the random case


def test_bf16_rounded_output_breaks_the_bound_on_most_elements():
  p = ib.pw_problem(HEAD, 'plain')
  bad = damaged(p)['rounded to bf16']
  frac = float(ib.gemm_violations(bad, p.want, p.mag, p.K).mean())
  assert frac > 0.5, frac
  assert ib.frac_not_bf16(bad) == 0.0
  # ... and one bf16 ulp is a distance the ulp helper reports as 2^16 float32 ulps
  assert ib.ulp_distance(np.float32([1.0 + 2.0 ** -7]), np.float64([1.0]))[0] == 2.0 ** 16


def test_localised_damage_is_found_where_it_is():
  p = ib.pw_problem(HEAD, 'plain')
  d = damaged(p)
  v = ib.gemm_violations(d['bias dropped on the last column tile'], p.want, p.mag, p.K)
  assert not v[:, :768].any() and v[:, 768:].any()
  v = ib.gemm_violations(d['last row repeats the row before it'], p.want, p.mag, p.K)
  assert not v[:-1].any() and v[-1].any()


@pytest.mark.parametrize('case', ib.PW_CASES, ids=lambda c: '%s-%s' % ('x'.join(map(str, c[0])), c[1]))
def test_reference_is_not_bf16_representable(case):
  """Assertion 1.4 of the device test (at least 90 % of the outputs have non-zero low 16 bits) holds for the float32 cast of
  the float64 reference of every random-case input, so a kernel that does not round its output passes it."""
  p = ib.pw_problem(*case)
  assert ib.frac_not_bf16(torch.from_numpy(f32(p.want))) >= ib.MIN_FRAC_NOT_BF16


@pytest.mark.parametrize('shape', ib.PW_EXACT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_exact_case_operands_make_every_partial_sum_exact(shape):
  """Every operand is an integer that bf16 represents and sum_k |a_ik| |w_kj| + |bias_j| < 2^24 for every output: every
  product and every partial sum, in any order, is an integer below 2^24 in magnitude, which float32 holds exactly."""
  p = ib.pw_problem(shape, 'plain', True)
  for t in (p.x, p.wk, p.bias):
    assert ib.is_bf16_integer(t)
  assert float(p.x.abs().max()) <= 8 and float(p.wk.abs().max()) <= 4 and float(p.bias.abs().max()) <= 64
  assert float(p.mag.max()) < 2.0 ** 24
  assert np.array_equal(f32(p.want).astype(np.float64), p.want)
  assert float(np.abs(p.want).max()) > 0


def test_is_bf16_integer_has_teeth():
  assert ib.is_bf16_integer(torch.tensor([-8.0, 0.0, 64.0, 256.0]))
  assert not ib.is_bf16_integer(torch.tensor([0.5]))
  assert not ib.is_bf16_integer(torch.tensor([257.0]))      # an integer, but bf16 has 8 significant bits


def test_ulp_helpers():
  assert ib.ulp32(np.float64([1.0, 1.5, 2.0, -4.0])).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -21]
  one = np.float32(1.0)
  assert ib.ulp_distance(np.float32([np.nextafter(one, np.float32(2))]), np.float64([1.0]))[0] == 1.0
  assert ib.not_bf16(np.float32([1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -8, 0.0])).tolist() == [False, False, True, False]


@pytest.mark.parametrize('c', ib.BN_CHANNELS)
def test_bn_eval_bound_rejects_the_wrong_epsilon(c):
  """A scale computed with eps 1e-4 where 1e-3 was asked for is rejected, even at the widest bound the device test may ever
  take (8 ulps): the variances inside [0, 10 eps] guarantee it.  The float32 cast of the reference itself passes."""
  assert 0 < ib.BN_EVAL_ULPS <= ib.BN_EVAL_ULPS_CAP
  p = ib.bn_problem(c, 1e-3)
  assert set(p.kind.tolist()) == {0, 1, 2, 3} and float(p.mv.min()) == 0.0 and float(p.mv.max()) > 100.0
  scale, shift = bn_eval_f32(p)
  assert ib.bn_eval_accepts(scale, shift, p, ulps=1.0)
  wrong_scale, wrong_shift = bn_eval_f32(p, eps=1e-4)
  assert not ib.bn_eval_accepts(wrong_scale, shift, p, ulps=ib.BN_EVAL_ULPS_CAP)
  assert not ib.bn_eval_accepts(scale, wrong_shift, p, ulps=ib.BN_EVAL_ULPS_CAP)
  # the damage sits in the channels where eps matters, and is orders of magnitude beyond the bound there
  d = ib.ulp_distance(wrong_scale, ib.bn_eval_ref(p)[0])
  assert float(d[p.kind <= 1].min()) > 1e3 * ib.BN_EVAL_ULPS_CAP


def bn_eval_f32(p, eps=None):
  scale, shift = ib.bn_eval_ref(p, eps)
  return f32(scale), f32(shift)
