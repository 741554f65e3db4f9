"""Inference preprocessing on a CANVAS batch (edet_preprocess_infer_canvas behind preprocess.preprocess_infer_canvas, csrc/
preprocess.hip) and EfficientDetModel on a (raw, sizes) pair.

Host: sizes and scaled sizes are checked before anything touches the device; what would be uploaded is
output_size_scale_factors per image and equals the scales recorded from the executed reference (tests/golden/
reference_preprocess.npz).  Kernel: image b of the canvas call is the dense call on that image alone, bit for bit over the
whole output, zero padding included; the mirrored output is torch.flip of the plain one; the canvas around the images holds
255 (inf for float raw), so a tap outside an image's rectangle shows.  Model: the pair path equals the chain assembled from
the public pieces, bit for bit in every output.  No tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

from automl_amd import _lib, preprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'reference_preprocess.npz')
F = np.float32
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
CANVAS = (53, 53)
SIZES = np.asarray([(1, 1), (37, 53), (53, 37), (53, 53), (2, 53)], np.int32)
OUTPUTS = {'64x64': (64, 64), '64x96': (64, 96)}      # the binding side differs between the images, and between the two


def same_bits(a, b):
  """Two device tensors of one dtype and shape, compared as raw bits (a NaN or the sign of a zero would count)."""
  if a.dtype != b.dtype or a.shape != b.shape:
    return False
  view = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
  return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ---------------------------------------------------------------------------------------------- host, no GPU
@pytest.fixture
def no_device(monkeypatch):
  """Any library call, or a copy to the device, fails the test: the checks under test come before both."""
  def refuse(*args, **kwargs):
    raise AssertionError('the device was touched before the sizes were checked')
  monkeypatch.setattr(_lib, 'call', refuse)
  monkeypatch.setattr(torch.Tensor, 'cuda', refuse)


def test_rejects_bad_sizes_before_the_device(no_device):
  raw = torch.zeros((3, 200, 200, 3), dtype=torch.uint8)
  with pytest.raises(ValueError, match=r'sizes must be integers \[batch, 2\].*batch 3'):
    preprocess.preprocess_infer_canvas(raw, np.ones((2, 2), np.int32), 64, MEAN, STD)
  with pytest.raises(ValueError, match=r'sizes must be integers'):
    preprocess.preprocess_infer_canvas(raw, np.ones((3, 2), np.float32), 64, MEAN, STD)
  with pytest.raises(ValueError, match=r'image 1: size 201 x 10 is outside'):
    preprocess.preprocess_infer_canvas(raw, np.asarray([(5, 5), (201, 10), (5, 5)], np.int32), 64, MEAN, STD)
  with pytest.raises(ValueError, match=r'image 2: size 5 x 0 is outside'):
    preprocess.preprocess_infer_canvas(raw, np.asarray([(5, 5), (5, 5), (5, 0)], np.int32), 64, MEAN, STD)
  with pytest.raises(ValueError, match=r'image 2: 1 x 200 scaled into 64 x 64 is empty \(0 x 64\)'):
    preprocess.preprocess_infer_canvas(raw, np.asarray([(5, 5), (7, 9), (1, 200)], np.int32), 64, MEAN, STD)
  with pytest.raises(ValueError, match=r'raw images must be'):
    preprocess.preprocess_infer_canvas(raw[0], np.ones((3, 2), np.int32), 64, MEAN, STD)
  with pytest.raises(ValueError, match=r'dtype must be'):
    preprocess.preprocess_infer_canvas(raw, np.ones((3, 2), np.int32), 64, MEAN, STD, dtype=torch.float16)


def test_uploaded_factors_are_the_evaluation_inputs(no_device):
  """Per image exactly output_size_scale_factors, for sizes where height binds, width binds, both, and a 1 x 1 image."""
  sizes = np.asarray([(1, 1), (37, 53), (53, 37), (53, 53), (2, 53), (480, 640), (427, 640), (640, 427), (333, 500)], np.int32)
  for out in ((64, 64), (64, 96), (512, 512), (640, 384)):
    got_sizes, scaled, scales = preprocess.infer_canvas_factors(torch.from_numpy(sizes), len(sizes), 640, 640, out)
    assert got_sizes.dtype == scaled.dtype == np.int32 and scales.dtype == F and np.array_equal(got_sizes, sizes)
    for i, (h, w) in enumerate(sizes):
      scale, (sh, sw) = preprocess.output_size_scale_factors(out, int(h), int(w))
      assert (int(scaled[i, 0]), int(scaled[i, 1])) == (sh, sw) and 1 <= sh <= out[0] and 1 <= sw <= out[1]
      assert scales[i].tobytes() == (F(1.0) / scale).tobytes()


def test_factors_equal_the_reference_fixture(no_device):
  """The raw sizes of the executed reference's inference cases: its recorded scale and scaled size."""
  g = np.load(GOLDEN)
  for name in ('infer_wide', 'infer_tall'):
    h, w = g[name + '/raw'].shape[:2]
    out = g[name + '/image'].shape[:2]
    _, scaled, scales = preprocess.infer_canvas_factors(np.asarray([(h, w), (1, 1)], np.int32), 2, 300, 300, out)
    assert scaled[0].tolist() == g[name + '/scaled'][:2].tolist()
    assert scales[0].tobytes() == (F(1.0) / g[name + '/image_scale']).astype(F).tobytes()
    assert scales[1] == F(1.0) / F(min(out))


# ---------------------------------------------------------------------------------------------- kernel, bit for bit
def canvas_batch(raw_dtype):
  """[5, 53, 53, 3]: 255 (uint8) or inf (float32) outside every image's rectangle, seeded pixels inside."""
  rng = np.random.default_rng(53)
  if raw_dtype == 'uint8':
    raw = np.full((len(SIZES),) + CANVAS + (3,), 255, np.uint8)
  else:
    raw = np.full((len(SIZES),) + CANVAS + (3,), np.inf, np.float32)
  for i, (h, w) in enumerate(SIZES):
    pixels = rng.integers(0, 256, (h, w, 3))
    raw[i, :h, :w] = pixels if raw_dtype == 'uint8' else pixels + rng.random((h, w, 3)).astype(F)
  return raw


@pytest.mark.gpu
@pytest.mark.parametrize('tdt', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('raw_dtype', ['uint8', 'float32'])
@pytest.mark.parametrize('out_name', sorted(OUTPUTS))
def test_canvas_image_equals_the_dense_call_on_that_image(out_name, raw_dtype, tdt):
  out_size = OUTPUTS[out_name]
  raw = canvas_batch(raw_dtype)
  dev = torch.from_numpy(raw).to('cuda:0')
  images, scales = preprocess.preprocess_infer_canvas(dev, SIZES, out_size, MEAN, STD, dtype=tdt)
  both = preprocess.preprocess_infer_canvas(dev, SIZES, out_size, MEAN, STD, dtype=tdt, mirrored=True)
  assert images.dtype == tdt and tuple(images.shape) == (len(SIZES),) + out_size + (3,)
  assert scales.dtype == torch.float32 and scales.is_cuda and tuple(scales.shape) == (len(SIZES),)
  bound = set()
  for i, (h, w) in enumerate(SIZES):
    alone = torch.from_numpy(np.ascontiguousarray(raw[i, :h, :w]))[None]
    want, want_scale = preprocess.preprocess_infer(alone, out_size, MEAN, STD, dtype=tdt)
    assert same_bits(images[i:i + 1], want), 'image %d (%d x %d)' % (i, h, w)
    assert same_bits(scales[i:i + 1], want_scale)
    assert bool(torch.isfinite(images[i].float()).all())      # nothing of the inf / 255 surroundings came in
    _, (sh, sw) = preprocess.output_size_scale_factors(out_size, int(h), int(w))
    assert not bool(images[i, sh:].any()) and not bool(images[i, :, sw:].any())      # the padding is zeros
    bound.add((sh == out_size[0], sw == out_size[1]))
  assert len(bound) >= 2      # the height binds for some images, the width for others
  assert len(both) == 3
  assert same_bits(both[0], images), 'out changes when the mirrored output is asked for'
  assert same_bits(both[1], torch.flip(images, dims=[2])), 'mirrored output'
  assert same_bits(both[2], scales)


@pytest.mark.gpu
@pytest.mark.parametrize('tdt', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('raw_dtype', ['uint8', 'float32'])
def test_full_sizes_equal_the_dense_batch(raw_dtype, tdt):
  rng = np.random.default_rng(5)
  raw = rng.integers(0, 256, (3,) + CANVAS + (3,)).astype(raw_dtype)
  full = np.tile(np.asarray(CANVAS, np.int32), (3, 1))
  for out_size in OUTPUTS.values():
    want, want_scales = preprocess.preprocess_infer(torch.from_numpy(raw), out_size, MEAN, STD, dtype=tdt)
    got, got_scales = preprocess.preprocess_infer_canvas(torch.from_numpy(raw), full, out_size, MEAN, STD, dtype=tdt)
    assert same_bits(got, want) and same_bits(got_scales, want_scales)


@pytest.mark.gpu
def test_entry_point_refuses_bad_arguments():
  """The C entry point's own checks: they return an error, nothing is launched."""
  raw = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device='cuda:0')
  per = torch.ones((2, 2), dtype=torch.int32, device='cuda:0')
  out = torch.zeros((1, 8, 8, 3), dtype=torch.float32, device='cuda:0')
  import ctypes
  mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
  st = torch.cuda.current_stream().cuda_stream

  def run(sizes, scaled, mirrored, dtype, batch=1):
    _lib.call('edet_preprocess_infer_canvas', raw.data_ptr(), 0, batch, 4, 4, sizes, scaled, 8, 8, mean, std, out.data_ptr(),
              mirrored, dtype, st)
  for bad in (lambda: run(None, per.data_ptr() + 8, None, _lib.EDET_F32),
              lambda: run(per.data_ptr(), None, None, _lib.EDET_F32),
              lambda: run(per.data_ptr(), per.data_ptr() + 8, out.data_ptr(), _lib.EDET_F32),
              lambda: run(per.data_ptr(), per.data_ptr() + 8, None, 77),
              lambda: run(per.data_ptr(), per.data_ptr() + 8, None, _lib.EDET_F32, batch=0)):
    with pytest.raises(_lib.EdetError, match='edet_preprocess_infer_canvas'):
      bad()
  torch.cuda.synchronize()
  assert not bool(out.any())


# ---------------------------------------------------------------------------------------------- the model on a pair
MODEL_CANVAS = (96, 120)
MODEL_SIZES = np.asarray([(96, 120), (60, 100), (96, 50)], np.int32)


@pytest.fixture(scope='module')
def model_case():
  """efficientdet-d0 at 128 x 128, fp32, seed 5; three images of different sizes on a 96 x 120 canvas whose surroundings are
  255; the per-image dense preprocessing, stacked: computed once and left unchanged."""
  from automl_amd import efficientdet_net, hparams_config
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  config.override('image_size=128')
  model = efficientdet_net.EfficientDetModel(config=config, dtype='f32', seed=5)
  rng = np.random.default_rng(96)
  raw = np.full((3,) + MODEL_CANVAS + (3,), 255, np.uint8)
  parts = []
  for i, (h, w) in enumerate(MODEL_SIZES):
    raw[i, :h, :w] = rng.integers(0, 256, (h, w, 3))
    parts.append(preprocess.preprocess_infer(torch.from_numpy(np.ascontiguousarray(raw[i, :h, :w]))[None], 128, config.mean_rgb,
                                             config.stddev_rgb))
  stacked = torch.cat([p[0] for p in parts], 0)
  scales = torch.cat([p[1] for p in parts], 0)
  return {'config': config, 'model': model, 'raw': torch.from_numpy(raw), 'stacked': stacked, 'scales': scales}


def tta_by_hand(model, images, scales, ids):
  """detect_flip_tta as it is written for a dense batch: two passes, torch.flip between them, fused."""
  from automl_amd import efficientdet_net, postprocess, wbf
  params = model.config.as_dict()
  cls_outputs, box_outputs = efficientdet_net.EfficientDetNet.__call__(model, images, False)
  plain = postprocess.generate_detections(params, cls_outputs, box_outputs, scales, ids)
  cls_outputs, box_outputs = efficientdet_net.EfficientDetNet.__call__(model, torch.flip(images, dims=[2]), False)
  mirrored = postprocess.generate_detections(params, cls_outputs, box_outputs, scales, ids, flip=True)
  return wbf.ensemble_detections_batch(params, torch.cat([plain, mirrored], 1), num_models=2)


@pytest.mark.gpu
def test_model_on_a_pair_equals_the_chain_by_hand(model_case):
  from automl_amd import postprocess
  c = model_case
  model, config = c['model'], c['config']
  got = model((c['raw'], MODEL_SIZES))
  got = [t.clone() for t in got]
  cls_outputs, box_outputs = model(c['stacked'], pre_mode=None, post_mode=None)
  want = postprocess.postprocess_global(config.as_dict(), cls_outputs, box_outputs, c['scales'])
  assert len(got) == len(want) == 4
  for name, g, w in zip(('boxes', 'scores', 'classes', 'valid_len'), got, want):
    assert same_bits(g, w), name
  assert int(want[3].min()) > 0, 'the problem must produce detections'
  # the scales are per image: the boxes of the narrow image reach no further than its own width
  assert len(set(c['scales'].tolist())) == 3
  boxes, valid = got[0].cpu().numpy(), got[3].cpu().numpy()
  for i, (h, w) in enumerate(MODEL_SIZES):
    assert boxes[i, :valid[i], 2].max() <= 128 * float(c['scales'][i]) + 1e-3
    assert boxes[i, :valid[i], 3].max() <= 128 * float(c['scales'][i]) + 1e-3
  # numpy inputs and sizes as a list are taken too
  again = model((c['raw'].numpy(), MODEL_SIZES.tolist()))
  assert all(same_bits(a, g) for a, g in zip(again, got))


@pytest.mark.gpu
def test_model_on_a_pair_of_full_sizes_equals_the_dense_batch(model_case):
  model = model_case['model']
  raw = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (3,) + MODEL_CANVAS + (3,)).astype(np.uint8))
  want = [t.clone() for t in model(raw)]
  got = model((raw, np.tile(np.asarray(MODEL_CANVAS, np.int32), (3, 1))))
  for name, g, w in zip(('boxes', 'scores', 'classes', 'valid_len'), got, want):
    assert same_bits(g, w), name


@pytest.mark.gpu
def test_flip_tta_on_a_pair_equals_the_chain_by_hand(model_case, monkeypatch):
  c = model_case
  ids = torch.tensor([7, 9, 11])
  want, want_n = [t.clone() for t in tta_by_hand(c['model'], c['stacked'], c['scales'], ids)]

  def no_flip(*args, **kwargs):
    raise AssertionError('torch.flip on the pair path: the mirrored output is the second input')
  monkeypatch.setattr(torch, 'flip', no_flip)
  got, got_n = c['model'].detect_flip_tta((c['raw'], MODEL_SIZES), image_ids=ids)
  monkeypatch.undo()
  assert same_bits(got_n, want_n) and int(want_n.min()) > 0
  assert same_bits(got, want)


@pytest.mark.gpu
def test_dense_flip_tta_is_unchanged(model_case):
  c = model_case
  raw = torch.from_numpy(np.random.default_rng(8).integers(0, 256, (3, 96, 128, 3)).astype(np.uint8))
  images, scales = preprocess.preprocess_infer(raw, 128, c['config'].mean_rgb, c['config'].stddev_rgb)
  ids = torch.arange(3)
  want, want_n = [t.clone() for t in tta_by_hand(c['model'], images, scales, ids)]
  got, got_n = c['model'].detect_flip_tta(raw)
  assert same_bits(got_n, want_n) and int(want_n.min()) > 0
  assert same_bits(got, want)


def test_pair_must_have_two_items():
  from automl_amd import efficientdet_net, hparams_config
  model = efficientdet_net.EfficientDetModel(config=hparams_config.get_efficientdet_config('efficientdet-d0'))
  with pytest.raises(ValueError, match='a canvas batch is a pair'):
    model((torch.zeros((1, 4, 4, 3), dtype=torch.uint8),))
