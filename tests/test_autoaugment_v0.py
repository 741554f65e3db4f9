"""AutoAugment v0 on the RandAugment kernels (automl_amd/autoaugment.py: policy_v0, autoaug_draws, autoaug_args,
distort_image_with_autoaugment): the tables and the policy walk against the reference executed on a stand-in
(tests/golden/reference_autoaug.npz, made by tests/golden/make_golden_autoaug.py), without a device; the device path against
the restatement tests/autoaug_ref.py bit for bit."""
import os

import numpy as np
import pytest
import torch

from automl_amd import autoaugment as aa, preprocess_legacy as pl
from tests import autoaug_ref as ar
from tests import bicubic_ref as br

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_autoaug.npz')


@pytest.fixture(scope='module')
def golden():
  return dict(np.load(GOLDEN))


def _runs(golden, key):
  """(image, sub, apply_u [2], sign [2], expected output) of every stored run of policy `key`."""
  for (is_b, sub, sign, pos), u in zip(golden[key + '/index'], golden[key + '/apply_u']):
    image = 'b' if is_b else 'a'
    yield golden['image/' + image], int(sub), u, np.full(2, float(sign), np.float32), golden['%s/out/%s' % (key, image)][pos]


def test_tables_equal_the_reference(golden):
  for key, table in (('v0', aa.policy_v0()), ('test', aa.policy_vtest())):
    want = ar.table_of(golden, key)
    assert [[tuple(e) for e in sub] for sub in table] == [[tuple(e) for e in sub] for sub in want], key
  assert len(aa.policy_v0()) == 25 and all(len(sub) == 2 for sub in aa.policy_v0())
  probs = [p for sub in aa.policy_v0() for _, p, _ in sub]
  assert 0.0 in probs and 1.0 in probs
  assert (aa.AUTOAUG_TRANSLATE_CONST, aa.AUTOAUG_CUTOUT_CONST) == (250, 100)
  # a caller's edits never reach the module's table
  aa.policy_v0()[0][0] = ('Invert', 1.0, 1)
  assert aa.policy_v0()[0][0] == ('Equalize', 0.8, 1)


def test_restatement_equals_the_reference_byte_for_byte(golden):
  seen = set()
  for key in ('v0', 'test'):
    table = ar.table_of(golden, key)
    for img, sub, u, sign, want in _runs(golden, key):
      got = ar.autoaugment_image(img, table, sub, u, sign)
      assert np.array_equal(got, want), (key, sub, u.tolist(), sign.tolist())
      for k, (name, prob, _) in enumerate(table[sub]):
        seen.add((key, sub, k, ar.applied(u[k], prob), float(sign[k]) if name in aa.SIGNED_OPS else 0.0))
  # every sub-policy, every position applied and -- unless its probability is 1.0 -- skipped; the signed ones with both signs
  for sub, entries in enumerate(ar.table_of(golden, 'v0')):
    for k, (name, prob, _) in enumerate(entries):
      signs = (1.0, -1.0) if name in aa.SIGNED_OPS else (0.0,)
      if prob > 0.0:
        assert all(('v0', sub, k, True, s) in seen for s in signs), (sub, k, name)
      if prob < 1.0:
        assert any(('v0', sub, k, False, s) in seen for s in signs), (sub, k, name)
  assert not any(a for (key, sub, k, a, s) in seen if key == 'v0' and (sub, k) in ((16, 0), (19, 1)))      # the 0.0 entries
  assert str(golden['invalid_name_message']) == 'Invalid augmentation_name: v1'


def test_autoaug_args_against_the_fixture_runs(golden):
  """Every stored run: the operation ids follow the apply rule, and every applied position's arguments are randaug_args' of
  that one operation at the table's level with AutoAugment's constants (randaug_args is pinned by tests/test_randaug.py)."""
  for key in ('v0', 'test'):
    table = ar.table_of(golden, key)
    for img, sub, u, sign, _ in _runs(golden, key):
      h, w = img.shape[:2]
      draws = (np.array([sub], np.int32), u.reshape(2, 1), sign.reshape(2, 1))
      ops, iargs, fargs = aa.autoaug_args(draws, h, w, table)
      assert ops.shape == (2, 1) and ops.dtype == np.int32 and iargs.shape == (2, 1, 4) and fargs.shape == (2, 1, 8)
      for k, (name, prob, level) in enumerate(table[sub]):
        if not ar.applied(u[k], prob):
          assert ops[k, 0] == aa.IDENTITY and not iargs[k, 0].any() and fargs[k, 0].tolist() == [0] * 6 + [1, 0]
          continue
        one = (np.array([[aa.OP_ID[name]]], np.int32), sign[k].reshape(1, 1), np.zeros((1, 1)), np.zeros((1, 1)))
        want = aa.randaug_args(one, level, h, w, translate_const=250, cutout_const=100)
        for got, exp in zip((ops[k], iargs[k], fargs[k]), (want[0][0], want[1][0], want[2][0])):
          assert np.array_equal(got, exp), (key, sub, k, name)
  # the boundary of the apply rule in float32: 0.6 + 0.4 and 0.4 + 0.6 round to 1.0
  assert aa.autoaug_applied(0.6, 0.4) and aa.autoaug_applied(0.4, 0.6) and not aa.autoaug_applied(0.59, 0.4)
  assert aa.autoaug_applied(0.0, 1.0) and not aa.autoaug_applied(np.float32(1) - np.float32(2) ** -24, 0.0)


def test_draws_stream_and_errors():
  a = aa.autoaug_draws(np.random.default_rng(3), 400, 'v0')
  b = aa.autoaug_draws(np.random.default_rng(3), 400, aa.policy_v0())
  assert all(np.array_equal(x, y) for x, y in zip(a, b))
  sub, u, sign = a
  assert sub.dtype == np.int32 and sub.shape == (400,) and set(sub.tolist()) == set(range(25))
  assert u.dtype == np.float32 and u.shape == (2, 400) and u.min() >= 0 and u.max() < 1
  assert sign.dtype == np.float32 and set(np.unique(sign).tolist()) == {-1.0, 1.0}
  # the stream does not depend on the table: the one-row test policy consumes the same draws
  t = aa.autoaug_draws(np.random.default_rng(3), 400, 'test')
  assert np.array_equal(t[1], u) and np.array_equal(t[2], sign) and not t[0].any()
  # a sub-policy index outside the table is the copy
  ops, _, _ = aa.autoaug_args((np.array([25, -1], np.int32), np.zeros((2, 2), np.float32) + 0.99, np.ones((2, 2), np.float32)), 8, 8)
  assert (ops == aa.IDENTITY).all()
  x = np.zeros((2, 8, 8, 3), np.uint8)
  for name in ('v1', 'autoaug', None):
    with pytest.raises(ValueError, match='Invalid augmentation_name'):      # (refused before anything touches the device)
      aa.distort_image_with_autoaugment(x, name)
  with pytest.raises(ValueError, match='out_dtype'):
    aa.distort_image_with_autoaugment(x, 'v0', out_dtype=torch.float16)
  with pytest.raises(ValueError, match='uint8'):
    aa.distort_image_with_autoaugment(x.astype(np.float32), 'v0')
  with pytest.raises(ValueError, match='apply_u'):
    aa.autoaug_args((np.zeros(2, np.int32), np.zeros((1, 2)), np.zeros((1, 2))), 8, 8)
  # the old spellings keep raising what they raised, with the hint behind it
  with pytest.raises(ValueError, match=r"aug_name 'autoaug' is not built: .*only 'randaug' is.*preprocessing='legacy'"):
    aa.check_aug_name('autoaug')
  with pytest.raises(ValueError, match=r"only 'randaug' is.*--legacy_input"):
    aa.check_aug_name('effnetv1_autoaug')
  with pytest.raises(ValueError, match=r"only 'randaug' is$"):
    aa.check_aug_name('ra_aa')
  with pytest.raises(ValueError, match='autoaugment.py:33-65'):
    aa.distort_image(x, 'autoaug', 2, 10)


def test_randaug_args_is_unchanged_by_the_shared_filler():
  """randaug_args on every operation and both signs against values written out here from level_to_arg."""
  h, w = 24, 20
  op = np.arange(17, dtype=np.int32).reshape(1, 17)
  for sg in (1.0, -1.0):
    draws = (op, np.full((1, 17), sg, np.float32), np.full((1, 17), 0.5), np.full((1, 17), 0.25))
    ops, iargs, fargs = aa.randaug_args(draws, 10, h, w)
    assert ops[0].tolist() == list(range(17))
    f = np.float32
    assert fargs[0, 3, :6].tolist() == [f(v) for v in aa.rotate_coefficients(sg * 30.0, h, w)]
    assert fargs[0, 10, :6].tolist() == [1, f(sg * 0.3), 0, 0, 1, 0] and fargs[0, 11, :6].tolist() == [1, 0, 0, f(sg * 0.3), 1, 0]
    assert fargs[0, 12, :6].tolist() == [1, 0, f(sg * 100.0), 0, 1, 0] and fargs[0, 13, :6].tolist() == [1, 0, 0, 0, 1, f(sg * 100.0)]
    assert iargs[0, 4].tolist() == [4, 0, 0, 0] and iargs[0, 5].tolist() == [256, 0, 0, 0] and iargs[0, 15].tolist() == [110, 128, 0, 0]
    assert iargs[0, 14].tolist() == [0, 0, 24, 20]      # centre (12, 5), pad 40
    for k in (6, 7, 8, 9):
      assert fargs[0, k, 6] == f(1.9)
    for k in (0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15, 16):
      assert fargs[0, k, 6] == 1.0


# ------------------------------------------------------------------------------------ GPU
def _batch50(golden):
  """50 images of 24 x 20: every sub-policy twice.  The first copy has apply draws (0.999, 0.999): every position with a
  probability above 0 is applied; the second (0.0, 0.0): every position with a probability below 1 is skipped.  The sign
  alternates every two sub-policies and is opposite in the two positions, so both signs reach the device for the signed
  operations that the table holds more than once (Rotate, ShearY; ShearX and TranslateY have one applicable entry each)."""
  rng = np.random.default_rng(77)
  images = rng.integers(0, 256, (50, 24, 20, 3)).astype(np.uint8)
  images[::7] = golden['image/a']
  sub = np.repeat(np.arange(25, dtype=np.int32), 2)
  u = np.where(np.arange(50) % 2 == 0, 0.999, 0.0).astype(np.float32)
  apply_u = np.stack([u, u]).astype(np.float32)
  first = np.where(sub % 4 < 2, 1.0, -1.0)
  sign = np.stack([first, -first]).astype(np.float32)
  return images, (sub, apply_u, sign)


@pytest.mark.gpu
def test_device_equals_the_restatement(golden):
  images, draws = _batch50(golden)
  table = ar.table_of(golden, 'v0')
  ops, _, _ = aa.autoaug_args(draws, 24, 20)
  applied = {(int(s), k): set() for s in range(25) for k in range(2)}
  for i in range(50):
    for k in range(2):
      applied[(int(draws[0][i]), k)].add(bool(ops[k, i] != aa.IDENTITY))
  # every entry of the table: both apply outcomes where 0 < p < 1, always applied at 1.0, never at 0.0
  for (s, k), seen in applied.items():
    prob = table[s][k][1]
    assert seen == ({True, False} if 0.0 < prob < 1.0 else {prob == 1.0}), (s, k, table[s][k], seen)
  # every operation of the table runs on the device, the five signed ones under both signs
  ran = {(int(ops[k, i]), float(draws[2][k, i])) for i in range(50) for k in range(2) if ops[k, i] != aa.IDENTITY}
  for name in {name for entries in table for name, prob, _ in entries if prob > 0.0}:
    signs = {sg for op, sg in ran if op == aa.OP_ID[name]}
    assert signs, name
    if name in ('Rotate', 'ShearY'):
      assert signs == {1.0, -1.0}, (name, signs)
  want = ar.autoaugment(images, draws, table)
  assert (want != images).reshape(50, -1).any(axis=1).sum() >= 25
  got = aa.distort_image_with_autoaugment(images, 'v0', draws=draws)
  assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
  ms = np.concatenate(pl.NORM)
  for kind in ('f32', 'bf16'):
    got = aa.distort_image_with_autoaugment(torch.from_numpy(images), 'v0', draws=draws, out_dtype=br.TORCH_DTYPE[kind], norm=pl.NORM)
    assert torch.equal(got.cpu(), br.normalize_u8(want, kind, ms)), kind
  # the default conversion is RandAugment's (x - 128) / 128
  got = aa.distort_image_with_autoaugment(images, 'v0', draws=draws, out_dtype=torch.float32)
  assert np.array_equal(got.cpu().numpy(), (want.astype(np.float32) - np.float32(128)) / np.float32(128))
  # the test policy, and draws made from a generator
  t = aa.distort_image_with_autoaugment(images[:4], 'test', rng=np.random.default_rng(1))
  tdraws = aa.autoaug_draws(np.random.default_rng(1), 4, 'test')
  assert np.array_equal(t.cpu().numpy(), ar.autoaugment(images[:4], tdraws, ar.table_of(golden, 'test')))
