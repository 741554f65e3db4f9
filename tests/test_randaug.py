"""RandAugment on the device (efficientnetv2/autoaugment.py on edet_randaug_stats / edet_randaug_apply,
automl_amd/autoaugment.py): the numpy restatement tests/randaug_ref.py against the executed reference
(tests/golden/reference_randaug.npz, written by tests/golden/make_golden_randaug.py) and the host side on the CPU; the kernels
against the restatement, bit for bit, on the GPU.

Oracle status: the fixture pins the reference's wiring (level_to_arg, the blend branches, the Contrast expression, the
histogram / look-up-table logic, wrap / unwrap, the operation order).  Not pinned by anything here, because TensorFlow and
TensorFlow Addons cannot run where this is tested: the rounding of the geometric operations (nearest source pixel, halves away
from zero) and their coefficient formulas, which follow the documented ImageProjectiveTransformV2 / TFA behaviour; the rounding
of tf.image.rgb_to_grayscale; Solarize thresholds >= 256 (compared as integers: identity)."""
import os

import numpy as np
import pytest
import torch

from automl_amd import _lib, autoaugment as aa, effnetv2_train
from automl_amd._lib import call, ptr
from tests import gpu_util as gu
from tests import randaug_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('edet_randaug_stats', 'edet_randaug_apply')
MAGNITUDES = (0, 5, 10, 15, 20)
_FIXTURE = []


def fixture():
  if not _FIXTURE:
    _FIXTURE.append(np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_randaug.npz')))
  return _FIXTURE[0]


# ------------------------------------------------------------------------------------ CPU
def test_new_entry_points_are_declared_and_bound():
  header = open(os.path.join(ROOT, 'include', 'edet_hip.h')).read()
  stubs = open(os.path.join(ROOT, 'automl_amd', 'csrc', 'plan_stubs.inc')).read()
  for name in NEW:
    assert name in _lib.SIGNATURES
    assert 'int %s(' % name in header
    assert '"%s"' % name in stubs
  assert aa.AVAILABLE_OPS == rr.OPS and aa.IDENTITY == 16


def test_restatement_equals_executed_reference():
  """Every array of the fixture, bit for bit: 16 operations x 5 magnitudes (x 2 signs for the five signed ones) x 3 images."""
  z = fixture()
  seen = set()
  for key in 'abc':
    img = z['image/' + key]
    names, cases = z['names/' + key], z['cases/' + key]
    assert len(names) == len(cases) == (11 + 2 * 5) * 5
    for nm, want in zip(names, cases):
      name, m, s = str(nm).split('/')
      m = int(m[1:])
      cy, cx = z['centre/%s/m%d' % (key, m)] if name == 'Cutout' else (0, 0)
      got = rr.apply_op(img, rr.OPS.index(name), m, 1.0 if s == 'p' else -1.0, cy, cx)
      assert got.dtype == np.uint8 and np.array_equal(got, want), (key, str(nm), int((got != want).sum()))
      seen.add((name, m))
  assert seen == {(n, m) for n in rr.OPS for m in MAGNITUDES}
  # the constant channel of image c: AutoContrast and Equalize leave that channel alone, and only that one
  c = z['image/c']
  out = rr.apply_op(c, 0, 10)
  assert np.array_equal(out[..., 1], c[..., 1]) and not np.array_equal(out[..., 0], c[..., 0])
  # 63 pixels: Equalize's step (63 - last bin) // 255 is 0, the whole image stays; image a has 480 and moves
  assert np.array_equal(rr.apply_op(c, 1, 10), c) and not np.array_equal(rr.apply_op(z['image/a'], 1, 10), z['image/a'])


def test_restatement_equals_executed_randaugment_runs():
  """distort_image_with_randaugment, two layers, with the queued draws of the fixture."""
  z = fixture()
  for r in ('ra0', 'ra1'):
    img = z['image/' + str(z[r + '/image'])]
    cu = z[r + '/centre_u']
    draws = (z[r + '/ops'][:, None], z[r + '/signs'][:, None], cu[:, 0:1], cu[:, 1:2])
    got = rr.randaugment(img[None], draws, int(z[r + '/magnitude']))[0]
    assert np.array_equal(got, z[r + '/out']), r
    assert not np.array_equal(got, img)


def test_level_to_arg_matches_the_reference():
  z = fixture()
  for name in aa.AVAILABLE_OPS:
    for m in MAGNITUDES:
      want = z['args/%s/m%d' % (name, m)]
      got = aa.level_to_arg(name, m)
      assert len(got) == len(want) and all(float(g) == float(w) for g, w in zip(got, want)), (name, m, got, want)
      assert rr.level_to_arg(name, float(m)) == got
  assert aa.level_to_arg('Color', 5) == (1.0,)                 # the blend early-out
  assert aa.level_to_arg('Posterize', 20) == (8,) and aa.level_to_arg('Posterize', 0) == (0,)
  assert aa.level_to_arg('TranslateX', 20) == (200.0,) and aa.level_to_arg('Cutout', 15) == (60,)
  assert aa.level_to_arg('Solarize', 10) == (256,) and aa.level_to_arg('SolarizeAdd', 7.5) == (82,)
  assert aa.level_to_arg('TranslateY', 10, translate_const=250) == (250.0,)      # AutoAugment's constants fit through


def test_randaug_args_follow_the_restatement():
  h, w = 17, 31
  ops = np.arange(17, dtype=np.int32)[None]
  sign = np.where(np.arange(17) % 2 == 0, 1.0, -1.0).astype(np.float32)[None]
  cy_u, cx_u = np.full((1, 17), 0.5), np.full((1, 17), 0.99)
  o, ia, fa = aa.randaug_args((ops, sign, cy_u, cx_u), 15, h, w)
  assert o.dtype == np.int32 and ia.dtype == np.int32 and fa.dtype == np.float32
  assert o.shape == (1, 17) and ia.shape == (1, 17, 4) and fa.shape == (1, 17, 8)
  assert np.array_equal(fa[0, 3, :6], np.asarray(rr.rotate_coef(-45.0, h, w), np.float32))       # odd ids: sign -1
  assert np.array_equal(fa[0, 10, :6], np.asarray([1, np.float32(1.5 * 0.3), 0, 0, 1, 0], np.float32))
  assert np.array_equal(fa[0, 11, :6], np.asarray([1, 0, 0, -np.float32(1.5 * 0.3), 1, 0], np.float32))
  assert np.array_equal(fa[0, 12, :6], np.asarray([1, 0, 150, 0, 1, 0], np.float32))
  assert np.array_equal(fa[0, 13, :6], np.asarray([1, 0, 0, 0, 1, -150], np.float32))
  assert ia[0, 4, 0] == 8 - 6 and ia[0, 5, 0] == 384 and tuple(ia[0, 15, :2]) == (165, 128)
  assert tuple(ia[0, 14]) == (0, 0, 17, 31)      # centre (8, 30), pad 60
  assert fa[0, 6, 6] == np.float32(2.8) and fa[0, 0, 6] == 1.0
  assert o[0, 16] == 16
  # an id outside [0, 16] becomes the identity
  o2, _, _ = aa.randaug_args((np.array([[99, -1]]), np.ones((1, 2)), np.zeros((1, 2)), np.zeros((1, 2))), 10, 8, 8)
  assert o2.tolist() == [[16, 16]]


def test_randaug_draws_are_deterministic_and_uniform():
  a = aa.randaug_draws(aa.randaug_rng(7), 8000, 2)
  b = aa.randaug_draws(aa.randaug_rng(7), 8000, 2)
  c = aa.randaug_draws(aa.randaug_rng(8), 8000, 2)
  assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[0], c[0])
  op, sign, cy_u, cx_u = a
  assert op.shape == sign.shape == cy_u.shape == cx_u.shape == (2, 8000) and op.dtype == np.int32
  counts = np.bincount(op.reshape(-1), minlength=16)
  assert len(counts) == 16 and counts.sum() == 16000
  chi2 = float(((counts - 1000.0) ** 2 / 1000.0).sum())
  print('chi-square over the 16 operations, 16000 draws: %.2f' % chi2)
  assert chi2 < 37.70      # 15 degrees of freedom, p = 0.001 (a fixed seed: it cannot flake)
  assert set(np.unique(sign).tolist()) == {-1.0, 1.0} and abs(float((sign > 0).mean()) - 0.5) < 0.02
  for u in (cy_u, cx_u):
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0 and abs(float(u.mean()) - 0.5) < 0.01


def test_value_errors():
  with pytest.raises(ValueError, match='autoaugment.py:33-65'):
    aa.check_aug_name('autoaug')
  with pytest.raises(ValueError, match='autoaugment.py:712-719'):
    aa.check_aug_name('ra_aa')
  for name in ('effnetv1_autoaug', 'effnetv1_randaug', 'ft', 'ft_autoaug'):
    with pytest.raises(ValueError, match='preprocessing.py'):
      aa.check_aug_name(name)
  with pytest.raises(ValueError, match='autoaugment.py:721'):
    aa.check_aug_name('nonsense')
  for bad in (-0.5, 20.5, 30):
    with pytest.raises(ValueError, match='magnitude'):
      aa.level_to_arg('Posterize', bad)
    with pytest.raises(ValueError, match='magnitude'):
      aa.randaug_args(aa.identity_draws(2, 1), bad, 8, 8)
  with pytest.raises(ValueError, match='unknown RandAugment operation'):
    aa.level_to_arg('Flip', 5)
  with pytest.raises(ValueError, match='num_layers, batch'):
    aa.randaug_args((np.zeros((1, 2)), np.zeros((1, 3)), np.zeros((1, 2)), np.zeros((1, 2))), 5, 8, 8)
  x = np.zeros((2, 8, 8, 3), np.uint8)
  with pytest.raises(ValueError, match='autoaugment.py:33-65'):      # (all refused before anything touches the device)
    aa.distort_image(x, 'autoaug', 2, 10)
  with pytest.raises(ValueError, match='ra_num_layers'):
    aa.distort_image(x, 'randaug', -1, 10)
  with pytest.raises(ValueError, match='magnitude'):
    aa.distort_image(x, 'randaug', 2, 21)
  with pytest.raises(ValueError, match='out_dtype'):
    aa.distort_image(x, 'randaug', 2, 10, out_dtype=torch.float16)
  with pytest.raises(ValueError, match='uint8'):
    aa.distort_image(x.astype(np.float32), 'randaug', 2, 10)
  with pytest.raises(ValueError, match='uint8'):
    aa.distort_image(x[..., :2], 'randaug', 2, 10)


def test_trainer_options():
  assert effnetv2_train.randaug_params('efficientnetv2-s') == ('randaug', 2, 10)
  assert effnetv2_train.randaug_params('efficientnetv2-m') == ('randaug', 2, 15)
  assert effnetv2_train.randaug_params('efficientnetv2-l') == ('randaug', 2, 20)
  assert effnetv2_train.randaug_params('efficientnetv2-xl') == ('randaug', 2, 20)
  assert effnetv2_train.randaug_params('efficientnetv2-b0')[0] == 'effnetv1_autoaug'
  make = lambda **kw: effnetv2_train.TrainableModel('efficientnetv2-b0', 'num_classes=24', **kw)
  net = make()
  assert net.augname is None and net.ra_num_layers == 2 and net.ra_magnitude == 15.0
  with pytest.raises(ValueError, match='without augname'):
    net.set_randaug(5)
  for name in ('autoaug', 'ra_aa', 'effnetv1_autoaug'):
    with pytest.raises(ValueError, match='not built'):
      make(augname=name)
  with pytest.raises(ValueError, match='magnitude'):
    make(augname='randaug', ra_magnitude=25)
  with pytest.raises(ValueError, match='ra_num_layers'):
    make(augname='randaug', ra_num_layers=-1)
  net = make(augname='randaug', ra_magnitude=7.5)
  net.set_randaug(12)
  assert net.ra_magnitude == 12.0
  with pytest.raises(ValueError, match='magnitude'):
    net.set_randaug(-1)


# ------------------------------------------------------------------------------------ GPU: the kernels
SIZES = [(13, 11), (32, 40), (64, 48)]      # rows of 33 bytes, images of 429: byte by byte; two sizes on the 4-pixel path
CANARY = 64


def _images(b, h, w, seed):
  return np.random.default_rng(seed).integers(0, 256, (b, h, w, 3)).astype(np.uint8)


def _one_op(op, b, sign=1.0, layers=1):
  shape = (layers, b)
  cy_u = np.broadcast_to((np.arange(b) + 0.5) / b, shape).copy()
  cx_u = np.broadcast_to(((np.arange(b) * 3 + 1) % b + 0.25) / b, shape).copy()
  return np.full(shape, op, np.int32), np.full(shape, sign, np.float32), cy_u, cx_u


def run_device(images, draws, magnitude, out_dtype=None):
  """The layers of `draws` through autoaugment.apply_layers on buffers with a canary behind each of them, twice: the two
  runs must agree in every byte.  -> numpy (uint8, or float32 holding the normalised output exactly)."""
  b, h, w = images.shape[:3]
  n = images.size
  tdt = out_dtype or torch.uint8
  layers = int(np.asarray(draws[0]).shape[0])
  src = torch.from_numpy(images).to(gu.DEV)
  args = [torch.from_numpy(a).to(gu.DEV) for a in aa.randaug_args(draws, magnitude, h, w)] if layers else [None] * 3
  fill = 7 if tdt == torch.uint8 else 5.0

  def flat(dtype, value):
    return torch.full((n + CANARY,), value, dtype=dtype, device=gu.DEV)
  outs = []
  for _ in range(2):
    out, sc = flat(tdt, fill), [flat(torch.uint8, 7) for _ in range(min(max(layers - 1, 0), 2))]
    luts = torch.zeros((b, 3, 256), dtype=torch.uint8, device=gu.DEV)
    aa.apply_layers(src, out[:n].view(b, h, w, 3), args[0], args[1], args[2], luts if layers else None,
                    [s[:n].view(b, h, w, 3) for s in sc], gu.stream())
    torch.cuda.synchronize()
    for t, v in [(out, fill)] + [(s, 7) for s in sc]:
      assert bool((t[n:] == v).all()), 'write behind the batch'
    outs.append(out[:n].clone().view(b, h, w, 3))
  a, c = (o.view(torch.uint8) if o.dtype == torch.uint8 else o.view(torch.int16 if o.dtype == torch.bfloat16 else torch.int32)
          for o in outs)
  assert torch.equal(a, c), 'run-to-run difference'
  assert torch.equal(src.cpu(), torch.from_numpy(images)), 'the source batch was written'
  return outs[0].cpu().numpy() if tdt == torch.uint8 else outs[0].float().cpu().numpy()


def _compare(got, want, what):
  assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
  if not np.array_equal(got, want):
    bad = np.argwhere(got != want)
    raise AssertionError('%s: %d values differ, first at %s: got %s, want %s' % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.gpu
@pytest.mark.parametrize('hw', SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('op', range(16), ids=lambda k: rr.OPS[k])
def test_every_op_alone(op, hw):
  """The whole batch of 5 one operation, at M = 0, 5, 10, 15, 20 and both signs, exactly.  M = 5: the enhance factor is
  exactly 1.0 (the blend early-out); M = 0: 0.1; M = 20: Posterize keeps 8 bits, Translate moves 200 px -- every pixel 128."""
  h, w = hw
  images = _images(5, h, w, gu.seed_of('one', h, w))
  images[1] = images[1] // 2 + 40      # a narrower range: AutoContrast has something to stretch at every size
  changed = 0
  for m in MAGNITUDES:
    for sign in ((1.0, -1.0) if rr.OPS[op] in rr.SIGNED else (1.0,)):
      draws = _one_op(op, 5, sign)
      want = rr.randaugment(images, draws, m)
      got = run_device(images, draws, m)
      _compare(got, want, '%s M=%d sign %+d %dx%d' % (rr.OPS[op], m, sign, h, w))
      changed += int(not np.array_equal(got, images))
      if rr.OPS[op] in ('TranslateX', 'TranslateY') and m == 20:
        assert (got == 128).all()
      if rr.OPS[op] in ('Color', 'Contrast', 'Brightness', 'Sharpness') and m == 5:
        assert np.array_equal(got, images)
      if rr.OPS[op] == 'Posterize':
        assert np.array_equal(got, images) == (m == 20) and ((got == 0).all() == (m == 0))
  if rr.OPS[op] == 'Equalize' and h * w <= 255:
    assert changed == 0      # step = (H W - last bin) // 255 = 0: the identity, as the reference has it
  else:
    assert changed > 0


@pytest.mark.gpu
def test_training_size_every_op():
  """4 x 300 x 300 (the 4-pixel path at efficientnetv2-s's training size), four layers: image i of layer k runs operation
  4 k + i, so the 16 operations all run once, chained, at the model's own magnitude."""
  b, h, w = 4, 300, 300
  images = _images(b, h, w, 300)
  images[1, :, :, 2] = 9                                    # a constant channel under AutoContrast / Equalize
  op = (np.arange(4)[:, None] * 4 + np.arange(4)[None]).astype(np.int32)
  sign = np.where((op % 2) == 0, 1.0, -1.0).astype(np.float32)
  rng = np.random.default_rng(5)
  draws = (op, sign, rng.random((4, 4)), rng.random((4, 4)))
  for k in (1, 4):
    sub = tuple(d[:k] for d in draws)
    _compare(run_device(images, sub, 10), rr.randaugment(images, sub, 10), '300x300, %d layers' % k)


@pytest.mark.gpu
@pytest.mark.parametrize('hw', SIZES[:2], ids=lambda s: '%dx%d' % s)
def test_mixed_batch_and_its_reverse(hw):
  """17 images carry the 17 operation ids (16 = identity) in one launch; the same batch in reverse order gives the same
  result per image: nothing depends on an image's place in the batch."""
  h, w = hw
  images = _images(17, h, w, gu.seed_of('mixed', h, w))
  ops = np.arange(17, dtype=np.int32)[None]
  sign = np.where(np.arange(17) % 3 == 0, -1.0, 1.0).astype(np.float32)[None]
  rng = np.random.default_rng(3)
  cy_u, cx_u = rng.random((1, 17)), rng.random((1, 17))
  draws = (ops, sign, cy_u, cx_u)
  want = rr.randaugment(images, draws, 15)
  got = run_device(images, draws, 15)
  _compare(got, want, 'mixed batch')
  assert np.array_equal(got[16], images[16])
  rev = tuple(d[:, ::-1].copy() for d in draws)
  got_rev = run_device(images[::-1].copy(), rev, 15)
  _compare(got_rev[::-1], got, 'reversed batch')
  # an operation id outside [0, 16] in device memory is the identity
  o, ia, fa = (torch.from_numpy(a).to(gu.DEV) for a in aa.randaug_args(draws, 15, h, w))
  o.fill_(99)
  o[0, 0] = -3
  src = torch.from_numpy(images).to(gu.DEV)
  out = torch.zeros_like(src)
  luts = torch.zeros((17, 3, 256), dtype=torch.uint8, device=gu.DEV)
  aa.apply_layers(src, out, o, ia, fa, luts, [], gu.stream())
  torch.cuda.synchronize()
  assert torch.equal(out, src)


def _edge_images(h, w):
  rng = np.random.default_rng(11)
  const_ch = rng.integers(20, 231, (h, w, 3)).astype(np.uint8)      # (a range AutoContrast has to stretch)
  const_ch[..., 2] = 200
  all_equal = np.full((h, w, 3), 93, np.uint8)
  two = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
  black, white = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
  return np.stack([const_ch, all_equal, two, black, white])


@pytest.mark.gpu
@pytest.mark.parametrize('hw', [(13, 11), (20, 16)], ids=lambda s: '%dx%d' % s)
def test_edge_images(hw):
  """A constant channel (AutoContrast / Equalize are the identity for that channel only), an all-equal image, an image of
  {0, 255} only, all black, all white: every operation, exactly."""
  h, w = hw
  images = _edge_images(h, w)
  for op in range(16):
    for m, sign in ((10, 1.0), (17.5, -1.0)):
      draws = _one_op(op, len(images), sign)
      got = run_device(images, draws, m)
      _compare(got, rr.randaugment(images, draws, m), '%s M=%s' % (rr.OPS[op], m))
      if op in (0, 1):
        assert np.array_equal(got[0, ..., 2], images[0, ..., 2]) and np.array_equal(got[1], images[1])
        # (up to 255 pixels Equalize's step (H W - last bin) // 255 is 0: the identity for every channel)
        assert np.array_equal(got[0, ..., 0], images[0, ..., 0]) == (op == 1 and h * w <= 255)


@pytest.mark.gpu
@pytest.mark.parametrize('hw', SIZES[:2], ids=lambda s: '%dx%d' % s)
def test_cutout_corners(hw):
  """Centres at (0, 0), (H - 1, W - 1) and the middle; at M = 20 (pad 80) the box is larger than the image from everywhere,
  at M = 1.25 (pad 5) it is clipped at the corners."""
  h, w = hw
  images = _images(3, h, w, gu.seed_of('cutout', h, w))
  cy_u = np.array([[0.0, (h - 0.5) / h, 0.5]])
  cx_u = np.array([[0.0, (w - 0.5) / w, 0.5]])
  draws = (np.full((1, 3), 14, np.int32), np.ones((1, 3), np.float32), cy_u, cx_u)
  for m in (20, 1.25):
    got = run_device(images, draws, m)
    _compare(got, rr.randaugment(images, draws, m), 'cutout M=%s' % m)
    if m == 20:
      assert (got == 128).all()
    else:
      assert (got[0, :5, :5] == 128).all() and np.array_equal(got[0, 5:], images[0, 5:])
      assert (got[1, h - 6:, w - 6:] == 128).all() and np.array_equal(got[1, :h - 6], images[1, :h - 6])


@pytest.mark.gpu
@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('hw', SIZES[:2], ids=lambda s: '%dx%d' % s)
def test_two_layers_and_fused_normalisation(dt, hw):
  """Two layers chained, the second one storing the network input: exactly (restatement - 128) / 128 in fp32 and in bf16
  (x - 128 has at most 8 significant bits); three layers use both ping-pong buffers; no layer is the normalising copy."""
  name, _, tdt = dt
  h, w = hw
  images = _images(6, h, w, gu.seed_of('two', h, w))
  draws = aa.randaug_draws(np.random.default_rng(gu.seed_of('draws', h, w)), 6, 3)
  draws[0][0, :] = [9, 3, 1, 0, 14, 6]      # a layer of neighbours and statistics in front of whatever was drawn
  for layers in (2, 3):
    sub = tuple(d[:layers] for d in draws)
    want_u8 = rr.randaugment(images, sub, 15)
    _compare(run_device(images, sub, 15), want_u8, '%d layers uint8' % layers)
    _compare(run_device(images, sub, 15, tdt), rr.normalise(want_u8), '%d layers %s' % (layers, name))
  none = tuple(d[:0] for d in draws)
  _compare(run_device(images, none, 15, tdt), rr.normalise(images), 'no layer %s' % name)
  _compare(run_device(images, none, 15), images, 'no layer uint8')
  # the public entry point: the same result from host images and from its own draws
  got = aa.distort_image(images, 'randaug', 2, 15, draws=tuple(d[:2] for d in draws), out_dtype=tdt)
  assert got.dtype == tdt and np.array_equal(got.float().cpu().numpy(), rr.normalise(rr.randaugment(images, tuple(d[:2] for d in draws), 15)))
  a = aa.distort_image(images, 'randaug', 2, 10, rng=np.random.default_rng(1))
  b = aa.distort_image(torch.from_numpy(images), 'randaug', 2, 10, rng=np.random.default_rng(1))
  assert a.dtype == torch.uint8 and torch.equal(a, b) and not torch.equal(a.cpu(), torch.from_numpy(images))


@pytest.mark.gpu
def test_randaug_refuses_bad_arguments():
  x = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=gu.DEV)
  y = torch.zeros((2, 4, 4, 3), dtype=torch.float32, device=gu.DEV)
  ops = torch.zeros(2, dtype=torch.int32, device=gu.DEV)
  ia = torch.zeros((2, 4), dtype=torch.int32, device=gu.DEV)
  fa = torch.zeros((2, 8), dtype=torch.float32, device=gu.DEV)
  luts = torch.zeros((2, 3, 256), dtype=torch.uint8, device=gu.DEV)
  u8, st = _lib.EDET_U8, gu.stream()
  with pytest.raises(_lib.EdetError):      # null source
    call('edet_randaug_apply', None, ptr(y), 2, 4, 4, ptr(ops), ptr(ia), ptr(fa), ptr(luts), _lib.EDET_F32, st)
  with pytest.raises(_lib.EdetError):      # in place
    call('edet_randaug_apply', ptr(x), ptr(x), 2, 4, 4, ptr(ops), ptr(ia), ptr(fa), ptr(luts), u8, st)
  with pytest.raises(_lib.EdetError):      # operations without their arguments
    call('edet_randaug_apply', ptr(x), ptr(y), 2, 4, 4, ptr(ops), None, ptr(fa), ptr(luts), _lib.EDET_F32, st)
  with pytest.raises(_lib.EdetError):      # bad output type
    call('edet_randaug_apply', ptr(x), ptr(y), 2, 4, 4, ptr(ops), ptr(ia), ptr(fa), ptr(luts), 3, st)
  with pytest.raises(_lib.EdetError):      # empty image
    call('edet_randaug_apply', ptr(x), ptr(y), 2, 0, 4, ptr(ops), ptr(ia), ptr(fa), ptr(luts), _lib.EDET_F32, st)
  with pytest.raises(_lib.EdetError):      # batch beyond grid.y
    call('edet_randaug_apply', ptr(x), ptr(y), 70000, 4, 4, ptr(ops), ptr(ia), ptr(fa), ptr(luts), _lib.EDET_F32, st)
  with pytest.raises(_lib.EdetError):      # no table to write
    call('edet_randaug_stats', ptr(x), 2, 4, 4, ptr(ops), None, st)
  with pytest.raises(_lib.EdetError):
    call('edet_randaug_stats', ptr(x), 0, 4, 4, ptr(ops), ptr(luts), st)
  torch.cuda.synchronize()
