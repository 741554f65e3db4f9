"""Detector evaluation on the device: the evaluation input stage (det_input.DetectionEvalInput, edet_pack_groundtruth), the
loss-only kernels (edet_focal_loss_eval, edet_box_loss_eval, edet_l2_loss), EfficientDetNetTrain.test_step / test_step_raw,
eval_lib.evaluate and train_lib.COCOCallback.

CPU: tests/det_eval_ref.py against the executed reference (tests/golden/reference_det_eval.npz, written by
tests/golden/make_golden_det_eval.py, which runs the reference's dataset_parser(is_training=False) and process_example), and
the host-side checks.  GPU: the kernels against the training kernels and the restatement, bit for bit; the network cases use
efficientdet-d0 at 128 x 128, batch 3, raw images of 40 x 56 with at most 8 box rows, as tests/test_det_input.py does."""
import copy
import os

import numpy as np
import pytest
import torch

from automl_amd import _lib, anchors as anchors_lib, coco_metric, det_input, eval_lib, hparams_config, labeling, postprocess
from automl_amd import preprocess, train_lib
from automl_amd._lib import call, ptr
from oracle.problems import perturbed_params
from tests import det_eval_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'reference_det_eval.npz')
SIZE, BATCH, RAW_H, RAW_W, MAX_BOXES = 128, 3, 40, 56, 8
LOSS_KEYS = ('cls_loss', 'box_loss', 'det_loss', 'reg_l2_loss', 'loss')
CASES = ('rows_at_max', 'rows_below_max')
_CACHE = {}


def fixture():
  if 'golden' not in _CACHE:
    _CACHE['golden'] = dict(np.load(GOLDEN))
  return _CACHE['golden']


def case_arrays(name):
  g = fixture()
  return {k: g['%s/%s' % (name, k)] for k in ('raw', 'boxes', 'classes', 'counts', 'is_crowds', 'areas', 'source_id_strings',
                                              'groundtruth_data', 'image_scales', 'source_ids')}


def raw_tuple(c):
  return (c['raw'], c['boxes'], c['classes'], c['counts'], c['is_crowds'], c['areas'], c['source_ids'])


def ref_groundtruth(c):
  g = fixture()
  out = []
  for i in range(c['raw'].shape[0]):
    n = int(c['counts'][i])
    out.append(det_eval_ref.eval_groundtruth(c['raw'].shape[1], c['raw'].shape[2], tuple(g['output_size']), c['boxes'][i, :n],
                                             c['classes'][i, :n], c['is_crowds'][i, :n], c['areas'][i, :n],
                                             str(c['source_id_strings'][i]), int(g['max_instances'])))
  return (np.stack([o[0] for o in out]), np.asarray([o[1] for o in out], np.float32), np.asarray([o[2] for o in out], np.float32))


def bits(a):
  return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('name', CASES)
def test_restatement_equals_the_executed_reference(name):
  c = case_arrays(name)
  gt, scales, ids = ref_groundtruth(c)
  assert gt.dtype == np.float32 and np.array_equal(bits(gt), bits(c['groundtruth_data']))
  assert np.array_equal(bits(scales), bits(c['image_scales']))
  assert np.array_equal(bits(ids), bits(c['source_ids']))
  assert np.array_equal(det_input.parse_source_ids(c['source_id_strings']), c['source_ids'])


def test_fixture_holds_the_cases_it_is_for():
  g = fixture()
  n = int(g['max_instances'])
  a, b = case_arrays('rows_at_max'), case_arrays('rows_below_max')
  assert a['boxes'].shape[1] == n and b['boxes'].shape[1] < n      # box rows == max_instances_per_image, and fewer
  assert int(a['counts'][1]) == 0 and float(a['source_ids'][1]) == -1.0 and a['source_id_strings'][1] == ''
  assert np.array_equal(a['groundtruth_data'][1], np.tile(np.asarray([-1, -1, -1, -1, 0, -1, -1], np.float32), (n, 1)))
  # image 0: the box of row 2 has no area and the annotation of row 3 is a crowd.  The kept boxes move up a row, the crowd
  # flags and the areas do not: row 3 holds the crowd flag of annotation 3 next to the box and class of annotation 4, and the
  # last annotation's area stands next to a box of -1
  gt, cnt = a['groundtruth_data'][0], int(a['counts'][0])
  assert a['boxes'][0, 2, 0] == a['boxes'][0, 2, 2] and a['is_crowds'][0, 3] == 1
  assert np.array_equal(gt[:cnt, 4], a['is_crowds'][0, :cnt]) and np.array_equal(gt[:cnt, 5], a['areas'][0, :cnt])
  assert np.array_equal(gt[:cnt - 1, 6], np.delete(a['classes'][0, :cnt], 2)) and gt[3, 4] == 1 and gt[3, 6] == a['classes'][0, 4]
  assert np.array_equal(gt[cnt - 1, :4], [-1, -1, -1, -1]) and gt[cnt - 1, 6] == -1 and gt[cnt - 1, 5] == a['areas'][0, cnt - 1]


def eval_config(extra=''):
  config = hparams_config.get_efficientdet_config('efficientdet-d0')
  config.override('image_size=%d,max_instances_per_image=%d%s' % (SIZE, int(fixture()['max_instances']), extra))
  return config


def test_more_box_rows_than_max_instances_raise_on_the_host():
  config = eval_config()
  with pytest.raises(ValueError, match='max_instances_per_image'):
    det_input.DetectionEvalInput(config, None, 2, RAW_H, RAW_W, config.max_instances_per_image + 1)
  net = train_lib.EfficientDetNetTrain(config=config)
  m = config.max_instances_per_image + 1
  data = (np.zeros((2, RAW_H, RAW_W, 3), np.uint8), np.zeros((2, m, 4), np.float32), np.zeros((2, m), np.float32),
          np.zeros(2, np.int32), np.zeros((2, m), np.float32), np.zeros((2, m), np.float32), np.zeros(2, np.float32))
  with pytest.raises(ValueError, match='max_instances_per_image'):
    net.test_step_raw(data)
  assert net.engine is None      # refused before anything was built


def test_max_instances_check_is_a_function_of_its_own():
  """det_input.check_max_instances: what DetectionEvalInput and test_step_raw both call, before any device work."""
  config = eval_config()
  n = config.max_instances_per_image
  assert det_input.check_max_instances(config, n) == n and det_input.check_max_instances(config, 1) == n
  with pytest.raises(ValueError, match=r'please increase config.max_instances_per_image \(%d box rows, max_instances_per_image %d'
                     % (n + 1, n)):
    det_input.check_max_instances(config, n + 1)
  config.max_instances_per_image = None      # the reference's default
  assert det_input.check_max_instances(config, 100) == 100
  with pytest.raises(ValueError, match='max_instances_per_image'):
    det_input.check_max_instances(config, 101)


def test_one_normalizer_reads_or_stores():
  """EfficientDetNetTrain._normalizer on a net without an engine (host value, host result).  store=False is the evaluation
  step's: v * m + x * (1 - m) from the stored v -- a float, a 0-d tensor, or nothing yet (0) -- and v stays.  store=True is
  the training step's: the sequence tests/test_hparams_config.py checks through _host_normalizer."""
  m, xs = 0.9, [101.0, 57.0, 230.5, 1.0, 88.0]
  net = train_lib.EfficientDetNetTrain(config=eval_config(',positives_momentum=%r' % m))
  assert net._normalizer(7.0, None, store=False) == 0.0 * m + 7.0 * (1 - m) and net._moving_normalizer is None
  net._moving_normalizer = 5.0
  assert net._normalizer(7.0, None, store=False) == 5.0 * m + 7.0 * (1 - m)
  assert net._moving_normalizer == 5.0 and not torch.is_tensor(net._moving_normalizer)
  state = net._moving_normalizer = torch.full((), 5.0, dtype=torch.float32)
  assert net._normalizer(7.0, None, store=False) == 5.0 * m + 7.0 * (1 - m)
  assert net._moving_normalizer is state and float(state) == 5.0
  want, v = [], 0.0
  for x in xs:
    v = v - (v - x) * (1.0 - m)
    want.append(v)
  for start in (None, torch.zeros((), dtype=torch.float32)):
    net._moving_normalizer = start
    got = [net._normalizer(x, None, store=True) for x in xs]
    np.testing.assert_allclose(got, want, rtol=1e-12 if start is None else 1e-6)
    assert torch.is_tensor(net._moving_normalizer) == (start is not None) and abs(float(net._moving_normalizer) - want[-1]) < 1e-3
    assert start is None or net._moving_normalizer is start
  # ... and _host_normalizer is that call
  net._moving_normalizer = None
  np.testing.assert_allclose([net._host_normalizer(x) for x in xs], want, rtol=1e-12)
  np.testing.assert_allclose(float(net._moving_normalizer), want[-1], rtol=1e-12)
  off = train_lib.EfficientDetNetTrain(config=eval_config())
  assert off._normalizer(101.0, None, store=True) == 101.0 == off._normalizer(101.0, None, store=False)
  assert off._moving_normalizer is None


class StubEvaluator(object):
  metric_names = ['AP', 'AP50']
  label_map = None

  def __init__(self):
    self.resets = self.results = 0

  def reset_states(self):
    self.resets += 1

  def update_state(self, groundtruth_data, detections):
    raise AssertionError('the stub test set is empty')

  def result(self):
    self.results += 1
    return np.asarray([0.25, 0.5], np.float32)


class StubModel(object):
  config = hparams_config.get_efficientdet_config('efficientdet-d0')


@pytest.mark.parametrize('update_freq,ran', [(5, [4, 9]), (1, list(range(10))), (None, []), (0, []), (3, [2, 5, 8])])
def test_coco_callback_runs_at_the_epochs_of_the_reference(update_freq, ran):
  """tf2/train_lib.py:233-234: epoch += 1; if self.update_freq and epoch % self.update_freq == 0."""
  cb = train_lib.COCOCallback([], update_freq=update_freq)
  cb.set_model(StubModel())
  assert isinstance(cb.evaluator, coco_metric.EvaluationMetric)
  cb.evaluator = stub = StubEvaluator()
  seen = []
  for epoch in range(10):
    logs = {'loss': 1.0}
    out = cb.on_epoch_end(epoch, logs)
    if out is not None:
      seen.append(epoch)
      assert out == {'AP': np.float32(0.25), 'AP50': np.float32(0.5)} and logs == {'loss': 1.0, **out}
    else:
      assert logs == {'loss': 1.0}
  assert seen == ran and stub.resets == stub.results == len(ran)


# ------------------------------------------------------------------------------------------------- GPU: the kernels
def _loss_inputs(positions, na, nc, tdt, seed):
  rng = np.random.default_rng(seed)
  pad8 = lambda c: (c + 7) // 8 * 8      # noqa: E731
  logits = torch.zeros((positions, pad8(na * nc)), dtype=torch.float32)
  logits[:, :na * nc] = torch.from_numpy((rng.standard_normal((positions, na * nc)) * 2.0).astype(np.float32))
  logits[:, na * nc:] = 7.0      # padding columns may hold anything
  box = torch.zeros((positions, pad8(4 * na)), dtype=torch.float32)
  box[:, :4 * na] = torch.from_numpy((rng.standard_normal((positions, 4 * na)) * 0.3).astype(np.float32))
  ct = rng.integers(0, nc, (positions, na)).astype(np.int32)
  r = rng.random((positions, na))
  ct[r < 0.6] = -1
  ct[r < 0.15] = -2      # ignored anchors
  bt = (rng.standard_normal((positions, 4 * na)) * 0.2).astype(np.float32)
  bt[rng.random((positions, 4 * na)) < 0.6] = 0.0
  dev = 'cuda:0'
  return (logits.to(dev).to(tdt).contiguous(), box.to(dev).to(tdt).contiguous(), torch.from_numpy(ct).to(dev),
          torch.from_numpy(bt).to(dev))


# (positions, anchors, classes).  810 class channels in rows of 816 (two rows per workgroup pass) and 36 box channels in rows of
# 40: 37 positions are no multiple of the rows per workgroup and make 5 (class) / 1 (box) workgroups, 301 make 38 / 3.  3
# classes: focal_body's branch for fewer than 8 classes (rows of 32, 64 rows per pass, 2 workgroups).  8 classes: a chunk is
# exactly one anchor.
# Past each cap of the grid rule (the smallest shapes that get there): 33000 positions of 816-wide class rows ask for
# ceil(ceil(33000 / 2) / 4) = 4125 workgroups, above the 4096 fallback and above any residency of 256-thread workgroups, so the
# class cap is taken whatever its value (box: 258, uncapped); 262200 positions of 40-wide box rows (32 rows per pass) ask for
# ceil(ceil(262200 / 32) / 4) = 2049 > 2048, the box cap (class: rows of 32, 64 per pass, 1025).
LOSS_GEOMETRIES = [(37, 9, 90), (301, 9, 90), (301, 9, 3), (70, 3, 8), (33000, 9, 90), (262200, 9, 3)]
THREADS = 256      # of the loss kernels


def loss_grid(ld, positions):
  """The documented grid rule of the loss kernels before its cap: rows per pass from the row width (one thread per 8
  elements, rounded up to a power of two), then (positions + rpp - 1) / rpp, then (g + 3) / 4."""
  tpr = 1
  while tpr < ld // 8 and tpr < THREADS:
    tpr *= 2
  rpp = THREADS // tpr
  return max(((positions + rpp - 1) // rpp + 3) // 4, 1)


def loss_inputs(geom, tdt):
  """_loss_inputs of the geometry, made once per geometry (the cases of one geometry follow each other)."""
  if _CACHE.get('loss_geom') != geom:
    _CACHE['loss_geom'], _CACHE['loss_inputs'] = geom, {}
  if tdt not in _CACHE['loss_inputs']:
    _CACHE['loss_inputs'][tdt] = _loss_inputs(*geom, tdt, 11)
  return _CACHE['loss_inputs'][tdt]


def four_losses(inputs, geom, edt, smoothing, ws, bytes_cls, bytes_box, inv_c, inv_b, nd_c, nd_b):
  """The two training and the two evaluation entry points on the same inputs -> (training sums, evaluation sums) as numpy
  [4]; `ws` with bytes_cls / bytes_box as the workspace size of the class / box calls."""
  logits, box, ct, bt = inputs
  positions, na, nc = geom
  dev = logits.device
  st = torch.cuda.current_stream().cuda_stream
  train, evl = torch.zeros(4, device=dev), torch.zeros(4, device=dev)
  dl, db = torch.empty_like(logits), torch.empty_like(box)
  dbc, dbb = torch.zeros(na * nc, device=dev), torch.zeros(4 * na, device=dev)
  if smoothing:
    call('edet_focal_loss_smooth', ptr(logits), logits.shape[1], ptr(ct), positions, na, nc, 0.25, 1.5, smoothing, inv_c,
         ptr(nd_c), ptr(dl), ptr(dbc), ptr(train), ptr(ws), bytes_cls, edt, st)
  else:
    call('edet_focal_loss', ptr(logits), logits.shape[1], ptr(ct), positions, na, nc, 0.25, 1.5, inv_c, ptr(nd_c), ptr(dl),
         ptr(dbc), ptr(train), ptr(ws), bytes_cls, edt, st)
  call('edet_box_loss', ptr(box), box.shape[1], ptr(bt), positions, 4 * na, 0.1, inv_b, 50.0, ptr(nd_b), ptr(db), ptr(dbb),
       ptr(train), ptr(ws), bytes_box, edt, st)
  call('edet_focal_loss_eval', ptr(logits), logits.shape[1], ptr(ct), positions, na, nc, 0.25, 1.5, smoothing, inv_c,
       ptr(nd_c), ptr(evl), ptr(ws), bytes_cls, edt, st)
  call('edet_box_loss_eval', ptr(box), box.shape[1], ptr(bt), positions, 4 * na, 0.1, inv_b, ptr(nd_b), ptr(evl), ptr(ws),
       bytes_box, edt, st)
  torch.cuda.synchronize()
  return train.cpu().numpy(), evl.cpu().numpy()


def normalizer_conventions(dev, norm=37.0):
  """(inv class, inv box, device class, device box): a host value; 1.0 with a device scalar."""
  inv_dev = torch.tensor([1.0 / norm], dtype=torch.float32, device=dev)
  inv_box = torch.tensor([1.0 / (norm * 4.0)], dtype=torch.float32, device=dev)
  return ((1.0 / norm, 1.0 / (norm * 4.0), None, None), (1.0, 1.0, inv_dev, inv_box))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [('f32', _lib.EDET_F32, torch.float32), ('bf16', _lib.EDET_BF16, torch.bfloat16)], ids=lambda d: d[0])
@pytest.mark.parametrize('smoothing', [0.0, 0.1], ids=['hard', 'ls0.1'])
@pytest.mark.parametrize('geom', LOSS_GEOMETRIES, ids=lambda g: 'x'.join(map(str, g)))
def test_loss_only_kernels_equal_the_training_kernels_bit_for_bit(dt, smoothing, geom):
  """sums[0:2] of edet_focal_loss_eval / edet_box_loss_eval against edet_focal_loss(_smooth) / edet_box_loss as uint32, for
  the grid with a partial buffer and for ONE workgroup (no workspace), and for both normalizer conventions (a host value;
  1.0 with a device scalar); the logits are left as they were.  The partial buffer holds the rows of the uncapped grid, so
  the two large geometries run their capped grids and not one workgroup."""
  _, edt, tdt = dt
  positions, na, nc = geom
  inputs = loss_inputs(geom, tdt)
  logits, box = inputs[:2]
  dev = logits.device
  rows = max(loss_grid(logits.shape[1], positions) * (1 + na * nc), loss_grid(box.shape[1], positions) * (1 + 4 * na))
  wsp = torch.empty(max(1024 * 1024, rows), dtype=torch.float32, device=dev)
  logits0, box0 = logits.clone(), box.clone()
  for ws, wsb in ((wsp, wsp.numel() * 4), (None, 0)):
    for inv_c, inv_b, nd_c, nd_b in normalizer_conventions(dev):
      t, e = four_losses(inputs, geom, edt, smoothing, ws, wsb, wsb, inv_c, inv_b, nd_c, nd_b)
      print(geom, dt[0], smoothing, 'workspace' if ws is not None else 'one workgroup', 'device' if nd_c is not None else 'host',
            t[:2], e[:2])
      assert np.isfinite(t[:2]).all() and t[0] > 0 and t[1] > 0
      assert np.array_equal(bits(t[:2]), bits(e[:2])), (t[:2], e[:2])
      assert e[2] == 0 and e[3] == 0
      assert torch.equal(logits.view(torch.int16 if tdt == torch.bfloat16 else torch.int32),
                         logits0.view(torch.int16 if tdt == torch.bfloat16 else torch.int32))
      assert torch.equal(box.float(), box0.float())


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [('f32', _lib.EDET_F32, torch.float32), ('bf16', _lib.EDET_BF16, torch.bfloat16)], ids=lambda d: d[0])
@pytest.mark.parametrize('smoothing', [0.0, 0.1], ids=['hard', 'ls0.1'])
@pytest.mark.parametrize('geom', [(37, 9, 90), (301, 9, 90)], ids=lambda g: 'x'.join(map(str, g)))
def test_loss_workspace_boundary_is_the_training_rows_for_all_four(dt, smoothing, geom):
  """A workspace of exactly g * (1 + nch) floats -- the TRAINING rows of the (here uncapped) grid, sized per call -- just
  holds them: all four entry points give the huge-workspace sums.  One float less and the training entry points go to one
  workgroup, and so must the evaluation ones, although their own g floats would fit: the no-workspace sums, bit for bit."""
  _, edt, tdt = dt
  positions, na, nc = geom
  inputs = loss_inputs(geom, tdt)
  logits, box = inputs[:2]
  dev = logits.device
  fit_c = loss_grid(logits.shape[1], positions) * (1 + na * nc) * 4
  fit_b = loss_grid(box.shape[1], positions) * (1 + 4 * na) * 4
  assert loss_grid(logits.shape[1], positions) == {37: 5, 301: 38}[positions] and fit_c > 4 and fit_b > 4
  wsp = torch.empty(1024 * 1024, dtype=torch.float32, device=dev)
  for conv in normalizer_conventions(dev):
    huge = four_losses(inputs, geom, edt, smoothing, wsp, wsp.numel() * 4, wsp.numel() * 4, *conv)
    none = four_losses(inputs, geom, edt, smoothing, None, 0, 0, *conv)
    fits = four_losses(inputs, geom, edt, smoothing, wsp, fit_c, fit_b, *conv)
    short = four_losses(inputs, geom, edt, smoothing, wsp, fit_c - 4, fit_b - 4, *conv)
    print(geom, dt[0], smoothing, fit_c, fit_b, huge[0][:2], fits[0][:2], none[0][:2], short[0][:2])
    for (t, e), (wt, we), what in ((fits, huge, 'rows just fit'), (short, none, 'one float short')):
      assert np.array_equal(bits(t[:2]), bits(wt[:2])), (what, 'training', t[:2], wt[:2])
      assert np.array_equal(bits(e[:2]), bits(we[:2])), (what, 'evaluation', e[:2], we[:2])
      assert np.array_equal(bits(e[:2]), bits(t[:2])), (what, 'evaluation against training', e[:2], t[:2])


@pytest.mark.gpu
def test_l2_loss_equals_the_training_sum_bit_for_bit():
  """The segment layout of tests/test_gpu_kernels.test_optimizer: unaligned, multi-slice and vectorised segments, two frozen
  ones, segments without the L2 flag.  edet_l2_loss takes no gradient pointer at all; the arena beside it stays as it is."""
  rng = np.random.default_rng(11)
  sizes = [7, 64, 1, 1000, 33, 4096, 40003, 3, 65536]
  flags = [1, 0, 0, 1, _lib.SEG_FROZEN, 0, 1, _lib.SEG_FROZEN, 1]
  offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  tot = int(offs[-1])
  dev = 'cuda:0'
  st = torch.cuda.current_stream().cuda_stream
  p = torch.from_numpy(rng.standard_normal(tot).astype(np.float32)).to(dev)
  g = torch.from_numpy((rng.standard_normal(tot) * 3).astype(np.float32)).to(dev)
  od, fd = torch.from_numpy(offs).to(dev), torch.tensor(flags, dtype=torch.int32, device=dev)
  wd = 4e-5
  seg_l2 = torch.full((len(sizes) * _lib.OPT_SPLIT,), float('nan'), dtype=torch.float32, device=dev)
  out = torch.full((1,), float('nan'), dtype=torch.float32, device=dev)
  g0, p0 = g.clone(), p.clone()
  call('edet_l2_loss', ptr(p), ptr(od), ptr(fd), len(sizes), wd, ptr(seg_l2), ptr(out), st)
  torch.cuda.synchronize()
  assert torch.equal(g, g0) and torch.equal(p, p0)
  sq = torch.zeros(2 * len(sizes) * _lib.OPT_SPLIT, dtype=torch.float32, device=dev)
  fac = torch.zeros(len(sizes), dtype=torch.float32, device=dev)
  l2d, gnd = torch.zeros(1, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
  call('edet_opt_l2_norms', ptr(g), ptr(p), ptr(od), ptr(fd), len(sizes), wd, ptr(sq), st)
  call('edet_opt_clip_factors', ptr(sq), len(sizes), 10.0, ptr(fac), ptr(gnd), ptr(l2d), st)
  torch.cuda.synchronize()
  want = 0.0
  for i, f in enumerate(flags):
    if f == 1:
      want += 0.5 * wd * float((p0[int(offs[i]):int(offs[i + 1])].double() ** 2).sum())
  print('l2', float(out), float(l2d), want)
  assert abs(float(l2d) - want) <= 1e-5 * want
  assert np.array_equal(bits(out.cpu().numpy()), bits(l2d.cpu().numpy())), (float(out), float(l2d))
  assert not torch.equal(g, g0)      # (the training kernel did add wd * w into its arena)


# --------------------------------------------------------------------------------------------- GPU: the input stage
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_eval_input_equals_the_pieces_composed_by_hand(dtype):
  config = eval_config()
  c = case_arrays('rows_at_max')
  anchors = anchors_lib.Anchors(config.min_level, config.max_level, config.num_scales, config.aspect_ratios, config.anchor_scale,
                                SIZE)
  inp = det_input.DetectionEvalInput(config, anchors, BATCH, RAW_H, RAW_W, MAX_BOXES, dtype=dtype)
  images, labels = inp.run(*raw_tuple(c), *inp.own_buffers())
  p = preprocess.DetectionInputProcessor(torch.from_numpy(c['raw']), config.image_size, c['boxes'], c['classes'], c['counts'],
                                         dtype=dtype)
  p.normalize_image(config.mean_rgb, config.stddev_rgb)
  p.set_scale_factors_to_output_size()
  want_images = p.resize_and_crop_image()
  bo, co, cnt = p.resize_and_crop_boxes()
  cls, box, npos = labeling.AnchorLabeler(anchors, config.num_classes).label_anchors_batch(bo, co, cnt)
  torch.cuda.synchronize()
  assert images.dtype == dtype and torch.equal(images.float(), want_images.float())
  assert float(npos.sum()) > 0
  for level in cls:
    assert torch.equal(labels['cls_targets_%d' % level], cls[level]), level
    assert torch.equal(labels['box_targets_%d' % level].reshape(box[level].shape), box[level]), level
  assert torch.equal(labels['mean_num_positives'], det_input.mean_num_positives(npos))
  assert np.array_equal(bits(labels['image_scales'].cpu().numpy()), bits(p.image_scale_to_original.numpy()))
  with pytest.raises(TypeError):
    inp.draw(np.random.default_rng(0))


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_groundtruth_equals_the_restatement_bit_for_bit(name):
  config = eval_config()
  c = case_arrays(name)
  b, h, w = c['raw'].shape[:3]
  m = c['boxes'].shape[1]
  anchors = anchors_lib.Anchors(config.min_level, config.max_level, config.num_scales, config.aspect_ratios, config.anchor_scale,
                                SIZE)
  inp = det_input.DetectionEvalInput(config, anchors, b, h, w, m)
  images, labels = inp.own_buffers()
  labels['groundtruth_data'].fill_(float('nan'))
  # the source ids as the strings of the annotation file, '' included
  inp.run(c['raw'], c['boxes'], c['classes'], c['counts'], c['is_crowds'] != 0, c['areas'], c['source_id_strings'], images, labels)
  torch.cuda.synchronize()
  gt, scales, ids = ref_groundtruth(c)
  got = labels['groundtruth_data'].cpu().numpy()
  assert got.shape == (b, config.max_instances_per_image, 7)
  assert np.array_equal(bits(got), bits(gt)) and np.array_equal(bits(got), bits(c['groundtruth_data']))
  assert np.array_equal(bits(labels['image_scales'].cpu().numpy()), bits(scales))
  assert np.array_equal(bits(labels['source_ids'].cpu().numpy()), bits(ids))


@pytest.mark.gpu
def test_pack_groundtruth_clamps_the_counts_it_reads():
  """Counts outside [0, M] in device memory (not what a caller should pass): clamped before they index anything."""
  dev = 'cuda:0'
  b, m, n = 3, 4, 6
  rng = np.random.default_rng(3)
  boxes = torch.from_numpy(rng.uniform(1, 50, (b, m, 4)).astype(np.float32)).to(dev)
  classes = torch.from_numpy(rng.integers(1, 9, (b, m)).astype(np.float32)).to(dev)
  crowds, areas = torch.ones((b, m), device=dev), torch.full((b, m), 9.0, device=dev)
  kept = torch.tensor([-5, 1000000, 2], dtype=torch.int32, device=dev)
  given = torch.tensor([1 << 30, -1, 3], dtype=torch.int32, device=dev)
  scales = torch.full((b,), 2.0, device=dev)
  guard = torch.full((b * n * 7 + 64,), 123.0, device=dev)
  call('edet_pack_groundtruth', ptr(boxes), ptr(classes), ptr(kept), ptr(crowds), ptr(areas), ptr(given), ptr(scales), b, m, n,
       ptr(guard), torch.cuda.current_stream().cuda_stream)
  torch.cuda.synchronize()
  assert float(guard[b * n * 7:].min()) == 123.0 and float(guard[b * n * 7:].max()) == 123.0
  gt = guard[:b * n * 7].view(b, n, 7).cpu()
  for i, (k, g) in enumerate(((0, m), (m, 0), (2, 3))):
    want = torch.tensor([-1, -1, -1, -1, 0, -1, -1], dtype=torch.float32).repeat(n, 1)
    want[:k, :4] = boxes[i, :k].cpu() * 2.0
    want[:k, 6] = classes[i, :k].cpu()
    want[:g, 4], want[:g, 5] = 1.0, 9.0
    assert torch.equal(gt[i], want), i


# ------------------------------------------------------------------------------------------------- GPU: test_step
def new_net(config, dtype, use_graph):
  return train_lib.EfficientDetNetTrain(config=config, dtype=dtype, params=perturbed_params(config, 3), seed=5,
                                        steps_per_epoch=10, global_batch_size=64, use_graph=use_graph)


def train_batches(steps=2, seed=7):
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(steps):
    raw = rng.integers(0, 256, (BATCH, RAW_H, RAW_W, 3)).astype(np.uint8)
    y0, x0 = rng.uniform(0.0, 0.6, (BATCH, MAX_BOXES)), rng.uniform(0.0, 0.6, (BATCH, MAX_BOXES))
    hh, ww = rng.uniform(0.15, 0.4, (BATCH, MAX_BOXES)), rng.uniform(0.15, 0.4, (BATCH, MAX_BOXES))
    boxes = np.stack([y0, x0, y0 + hh, x0 + ww], -1).astype(np.float32)
    classes = rng.integers(1, 91, (BATCH, MAX_BOXES)).astype(np.float32)
    out.append((raw, boxes, classes, np.asarray([5, 0, MAX_BOXES], np.int32)))
  return out


def full_state(net):
  torch.cuda.synchronize()
  eng = net.engine
  return (net.get_weights(), net.get_optimizer_state(), eng.arena.state_flat.cpu().numpy().copy(),
          eng.grads_flat.cpu().numpy().copy(), net.iterations, eng.arena.step_count)


def assert_states_equal(a, b, what):
  (wa, sa, ma, ga, ia, ca), (wb, sb, mb, gb, ib, cb) = a, b
  assert sorted(wa) == sorted(wb) and sorted(sa) == sorted(sb), what
  for k in wa:
    assert np.array_equal(wa[k], wb[k]), (what, 'variable', k)
  for k in sa:
    assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), (what, 'optimizer state', k)
  assert np.array_equal(ma, mb), (what, 'BatchNorm moving statistics')
  assert np.array_equal(ga, gb), (what, 'gradient arena')
  assert (ia, ca) == (ib, cb), (what, 'iterations')


@pytest.mark.gpu
def test_test_step_leaves_the_training_state_alone():
  """bf16, use_graph: a train step, two test_step_raw calls (the second captures the evaluation pass), then the train step
  that captures the TRAINING graph -- against a twin that never evaluated.  reg_l2_loss of the evaluation is the next train
  step's, bit for bit."""
  config = eval_config()
  ev = raw_tuple(case_arrays('rows_at_max'))
  steps = train_batches(3)
  net, twin = new_net(config, 'bf16', True), new_net(config, 'bf16', True)
  first = net.train_step_raw(steps[0])
  assert twin.train_step_raw(steps[0]) == first
  before = full_state(net)
  assert 'input_rng_state' in before[1]
  evals = [net.test_step_raw(ev)[0] for _ in range(3)]      # eager, captured + replayed, replayed
  after = full_state(net)
  assert_states_equal(before, after, 'test_step_raw')
  assert_states_equal(after, full_state(twin), 'twin before the next step')
  assert all(np.isfinite(v['loss']) and v['cls_loss'] > 0 and v['box_loss'] > 0 for v in evals), evals
  assert evals[0] == evals[1] == evals[2] and sorted(evals[0]) == sorted(LOSS_KEYS)
  for step in steps[1:]:      # the capture of the training graph, then a replay
    got, want = net.train_step_raw(step), twin.train_step_raw(step)
    assert got == want, (got, want)
    if step is steps[1]:
      assert got['reg_l2_loss'] == evals[0]['reg_l2_loss'], (got['reg_l2_loss'], evals[0]['reg_l2_loss'])
    assert_states_equal(full_state(net), full_state(twin), 'after a train step')
  # ... and the replayed evaluation sees the variables as they are now
  later = net.test_step_raw(ev)[0]
  assert later['reg_l2_loss'] != evals[0]['reg_l2_loss'] and later['cls_loss'] != evals[0]['cls_loss']
  fresh = new_net(config, 'bf16', False)
  fresh.set_weights(net.get_weights())
  assert fresh.test_step_raw(ev)[0] == later


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_replayed_test_step_equals_the_eager_one(dtype):
  config = eval_config()
  ev = raw_tuple(case_arrays('rows_at_max'))
  graph, eager = new_net(config, dtype, True), new_net(config, dtype, False)
  g = [graph.test_step_raw(ev) for _ in range(3)]
  e = [eager.test_step_raw(ev) for _ in range(3)]
  assert graph._eval_graphs[(BATCH, SIZE, SIZE)]['graph'] is not None and not eager._eval_graphs
  for k in LOSS_KEYS:
    assert g[2][0][k] == e[2][0][k], (k, g[2][0][k], e[2][0][k])
  assert np.isfinite(g[2][0]['loss']) and g[2][0]['cls_loss'] > 0
  # labels come back with the ground truth of the batch
  torch.cuda.synchronize()
  assert np.array_equal(bits(g[2][1]['groundtruth_data'].cpu().numpy()), bits(case_arrays('rows_at_max')['groundtruth_data']))
  # test_step on the same tensors is the same step
  images, labels = eager._det_eval_input[1].own_buffers()
  again = eager.test_step((images.clone(), {k: v.clone() for k, v in labels.items() if k.split('_')[0] in ('cls', 'box', 'mean')}))
  assert again == e[2][0]


@pytest.mark.gpu
def test_test_step_raw_after_a_capture_that_test_step_made():
  """use_graph, mixed order: test_step twice (eager, then the capture) on tensors of its own, then test_step_raw of the same
  shape.  The capture's static labels have no ground-truth keys; test_step_raw adds them, writes into the captured buffers and
  replays the graph test_step captured."""
  config = eval_config()
  ev = raw_tuple(case_arrays('rows_at_max'))
  graph, eager = new_net(config, 'bf16', True), new_net(config, 'bf16', False)
  want, want_labels = eager.test_step_raw(ev)
  images, labels = eager._det_eval_input[1].own_buffers()
  data = (images.clone(), {k: v.clone() for k, v in labels.items() if k.split('_')[0] in ('cls', 'box', 'mean')})
  first = [graph.test_step(data) for _ in range(2)]
  state = graph._eval_graphs[(BATCH, SIZE, SIZE)]
  captured = state['graph']
  assert captured is not None and state['steps'] == 2 and 'groundtruth_data' not in state['labels']
  assert first[0] == first[1] == want
  state['images'].zero_()      # the raw call fills the captured buffers itself
  got, got_labels = graph.test_step_raw(ev)
  assert sorted(got) == sorted(LOSS_KEYS)
  for k in LOSS_KEYS:
    assert got[k] == want[k], (k, got[k], want[k])
  assert graph._eval_graphs[(BATCH, SIZE, SIZE)]['graph'] is captured and state['steps'] == 3
  torch.cuda.synchronize()
  assert {'groundtruth_data', 'source_ids', 'image_scales'} <= set(got_labels)
  for k in ('groundtruth_data', 'source_ids', 'image_scales'):
    assert np.array_equal(bits(got_labels[k].cpu().numpy()), bits(want_labels[k].cpu().numpy())), k
  assert np.array_equal(bits(got_labels['groundtruth_data'].cpu().numpy()), bits(case_arrays('rows_at_max')['groundtruth_data']))


@pytest.mark.gpu
@pytest.mark.parametrize('smoothing', [0.0, 0.1], ids=['hard', 'ls0.1'])
def test_test_step_matches_the_oracle_fp32(smoothing):
  """forward(images, False) + detection_loss + the L2 sum of the CPU oracle; the tolerance the project applies to these keys
  against the oracle (tests/test_gpu_network.py: 2e-3 |ref| + 1e-6)."""
  from oracle import efficientdet_oracle as orc
  from tests.test_gpu_network import make_labels
  config = eval_config(',label_smoothing=%g' % smoothing)
  vals = perturbed_params(config, 5)
  images = np.random.default_rng(23).standard_normal((BATCH, SIZE, SIZE, 3)).astype(np.float32)
  labels = make_labels(config, BATCH, SIZE, 29)
  net = train_lib.EfficientDetNetTrain(config=config, dtype='f32', params=vals)
  got = net.test_step((torch.from_numpy(images), labels))
  oracle = orc.Oracle(config=config, params={k: torch.from_numpy(v.copy()) for k, v in vals.items()})
  with torch.no_grad():
    cls_out, box_out = oracle.forward(torch.from_numpy(images), False)
    det, cls_loss, box_loss = orc.detection_loss(config, cls_out, box_out, {k: torch.from_numpy(v) for k, v in labels.items()})
    params = oracle.params()
    l2 = config.weight_decay * sum((params[n].double() ** 2).sum() / 2 for n in oracle.trainable_names() if orc.is_l2_regularised(n))
  ref = {'cls_loss': float(cls_loss), 'box_loss': float(box_loss), 'det_loss': float(det), 'reg_l2_loss': float(l2),
         'loss': float(det) + float(l2)}
  print('test_step: got %s\n ref %s' % (got, ref))
  for k in LOSS_KEYS:
    assert abs(got[k] - ref[k]) <= 2e-3 * abs(ref[k]) + 1e-6, (k, got[k], ref[k])
  assert ref['cls_loss'] > 0 and ref['box_loss'] > 0 and ref['reg_l2_loss'] > 0


@pytest.mark.gpu
def test_positives_momentum_is_read_and_not_stored():
  """The reported losses use v * m + x * (1 - m) from the stored moving normalizer v; v stays.  Against the same variables
  with positives_momentum off, whose normalizer is x: the class loss scales by x / (v m + x (1 - m)), up to the rounding of the
  two reciprocals."""
  from tests.test_gpu_network import make_labels
  m, v = 0.9, 5.0
  images = torch.from_numpy(np.random.default_rng(23).standard_normal((BATCH, SIZE, SIZE, 3)).astype(np.float32))
  out = {}
  for mom in (0.0, m):
    config = eval_config(',positives_momentum=%g' % mom if mom else '')
    labels = make_labels(config, BATCH, SIZE, 29)
    net = new_net(config, 'f32', False)
    out[mom, 'new'] = net.test_step((images, labels))      # builds the engine; no stored normalizer yet: v = 0
    if mom:
      state = net.get_optimizer_state()
      assert 'moving_normalizer' not in state
      state['moving_normalizer'] = v
      net.set_optimizer_state(state)
      out[mom, 'stored'] = net.test_step((images, labels))
      out[mom, 'host'] = net.test_step((images, dict(labels, normalizer=float(labels['mean_num_positives'].sum()) + 1.0)))
      assert net.get_optimizer_state()['moving_normalizer'] == v
  x = float(labels['mean_num_positives'].sum()) + 1.0
  plain = out[0.0, 'new']
  for key, norm in (('new', x * (1 - m)), ('stored', v * m + x * (1 - m)), ('host', v * m + x * (1 - m))):
    got = out[m, key]
    for k in ('cls_loss', 'box_loss'):
      want = plain[k] * x / norm
      assert abs(got[k] - want) <= 1e-5 * want, (key, k, got[k], want)
    assert got['reg_l2_loss'] == plain['reg_l2_loss']


# -------------------------------------------------------------------------------------------------- GPU: evaluate
def _own_detections_as_groundtruth(model, config, raws):
  """Per raw batch: the model's top detections of those images as ground truth, mapped back to normalised raw coordinates."""
  params = eval_lib.eval_config(config).as_dict()
  out, next_id = [], 1
  for raw in raws:
    b = raw.shape[0]
    zeros = np.zeros((b, MAX_BOXES), np.float32)
    ids = np.arange(next_id, next_id + b).astype(np.float32)
    next_id += b
    inp = det_input.DetectionEvalInput(config, model.anchors((SIZE, SIZE)), b, RAW_H, RAW_W, MAX_BOXES, dtype=torch.float32)
    images, labels = inp.run(raw, np.zeros((b, MAX_BOXES, 4), np.float32), zeros, np.zeros(b, np.int32), zeros, zeros, ids,
                             *inp.own_buffers())
    cls_out, box_out = model(images, training=False)
    det = postprocess.generate_detections(params, cls_out, box_out, labels['image_scales'], labels['source_ids']).cpu().numpy()
    boxes, classes, areas, counts = np.zeros((b, MAX_BOXES, 4), np.float32), zeros.copy(), zeros.copy(), np.zeros(b, np.int32)
    for i in range(b):
      d = det[i]
      wide = d[(d[:, 3] - d[:, 1] > 4) & (d[:, 4] - d[:, 2] > 4) & (d[:, 5] > 0) & (d[:, 1] >= 0) & (d[:, 2] >= 0) &
               (d[:, 3] <= RAW_W - 2) & (d[:, 4] <= RAW_H - 2)]      # inside the image: the ground truth is clipped to it
      top = wide[np.argsort(-wide[:, 5], kind='stable')[:3]]
      counts[i] = len(top)
      boxes[i, :len(top)] = np.stack([top[:, 2] / RAW_H, top[:, 1] / RAW_W, top[:, 4] / RAW_H, top[:, 3] / RAW_W], -1)
      classes[i, :len(top)] = top[:, 6]
      areas[i, :len(top)] = (top[:, 3] - top[:, 1]) * (top[:, 4] - top[:, 2])
    out.append((raw, np.clip(boxes, 0, 1), classes, counts, zeros.copy(), areas, ids))
  return out


@pytest.mark.gpu
def test_evaluate_equals_the_chain_composed_by_hand():
  """Two batches of 3 and 2 images (a partial last batch: a second input stage and a second engine shape)."""
  config = eval_config()
  model = new_net(config, 'f32', False)
  rng = np.random.default_rng(41)
  raws = [rng.integers(0, 256, (n, RAW_H, RAW_W, 3)).astype(np.uint8) for n in (3, 2)]
  batches = _own_detections_as_groundtruth(model, config, raws)
  assert sum(int(b[3].sum()) for b in batches) >= 5, [b[3] for b in batches]
  label_map = {1: 'one', 2: 'two', 3: 'three'}
  got = eval_lib.evaluate(model, batches, evaluator=coco_metric.EvaluationMetric(label_map=label_map))
  # by hand
  hand = coco_metric.EvaluationMetric(label_map=label_map)
  cfg = copy.deepcopy(config)
  cfg.nms_configs.max_nms_inputs = anchors_lib.MAX_DETECTION_POINTS
  for batch in batches:
    b = batch[0].shape[0]
    inp = det_input.DetectionEvalInput(cfg, model.anchors((SIZE, SIZE)), b, RAW_H, RAW_W, MAX_BOXES, dtype=torch.float32)
    images, labels = inp.run(*batch, *inp.own_buffers())
    cls_out, box_out = model(images, training=False)
    det = postprocess.generate_detections(cfg.as_dict(), cls_out, box_out, labels['image_scales'], labels['source_ids'])
    hand.update_state(labels['groundtruth_data'], postprocess.transform_detections(det))
  metrics = hand.result()
  want = {name: metrics[i] for i, name in enumerate(hand.metric_names)}
  for i, cid in enumerate(sorted(label_map)):
    want['AP_/%s' % label_map[cid]] = metrics[i + len(hand.metric_names)]
  print('evaluate', got)
  assert sorted(got) == sorted(want) and {'AP', 'AP50', 'ARmax100', 'AP_/one', 'AP_/two', 'AP_/three'} <= set(got)
  for k in want:
    assert np.array_equal(bits(got[k]), bits(want[k])), (k, got[k], want[k])
  assert got['AP'] > 0      # a condition on the inputs: the ground truth is the model's own detections
  assert hand.image_ids == [1, 2, 3, 4, 5]
  # eval_samples = 3 with batches of 3: exactly one batch
  one = coco_metric.EvaluationMetric()
  eval_lib.evaluate(model, batches, evaluator=one, eval_samples=3)
  assert one.image_ids == [1, 2, 3]
  four = coco_metric.EvaluationMetric()
  eval_lib.evaluate(model, batches, evaluator=four, eval_samples=4)
  assert four.image_ids == [1, 2, 3, 4, 5]
  # the callback puts the same numbers into the logs
  cb = train_lib.COCOCallback(batches, update_freq=2)
  cb.set_model(model)
  logs = {}
  assert cb.on_epoch_end(0, logs) is None and logs == {}
  cb.on_epoch_end(1, logs)
  assert sorted(logs) == sorted(hand.metric_names)
  for k in logs:
    assert np.array_equal(bits(logs[k]), bits(want[k])), k
