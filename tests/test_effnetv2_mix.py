"""Mixup, cutmix and soft labels in the EfficientNetV2 classifier trainer (efficientnetv2/datasets.py:191-301 on
edet_mix_images, edet_mix_labels and edet_softmax_xent_soft): the host side of the draws on the CPU, the three kernels and
the mixed train step against fp32 / float64 restatements on the GPU.

The restatements live here: `xent_soft` (CategoricalCrossentropy(label_smoothing, from_logits=True) on dense labels: Keras
smooths whatever y_true it gets, and nothing assumes a row sums to 1), `mix_images_ref` / `mix_labels_ref` (the reference's
`mixing` with "reverse" taken within each part, numpy float32, out of place) and `oracle_mixed_step` (test_effnetv2_train's
oracle_train_step with the soft-label loss)."""
import os

import numpy as np
import pytest
import torch

from automl_amd import _lib, effnetv2_configs, effnetv2_model, effnetv2_train, netspec
from automl_amd._lib import call, ptr
from oracle import effnetv2_oracle as v2orc
from tests import gpu_util as gu
from tests.test_effnetv2_train import EPSILON, _perturbed, _xent_problem, rmsprop_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('edet_softmax_xent_soft', 'edet_mix_images', 'edet_mix_labels')


# ------------------------------------------------------------------------------------ restatements
def xent_soft(logits, y, smoothing):
  """-> mean loss: y' = (1 - s) y + s / C, loss_row = logsumexp(x) * sum_c y'_c - sum_c y'_c x_c."""
  c = logits.shape[1]
  ys = y.to(logits.dtype) * (1.0 - smoothing) + smoothing / c
  rows = torch.logsumexp(logits, dim=1) * ys.sum(1) - (ys * logits).sum(1)
  return rows.mean()


def topk_rows_soft(logits, y, k):
  """TopKCategoricalAccuracy: the row's class is argmax_c y_c (numpy: the first index on ties); the row counts when fewer
  than k logits are strictly greater than that class's."""
  cls = torch.from_numpy(np.argmax(np.asarray(y), axis=1))
  xl = logits.gather(1, cls.view(-1, 1))
  return int(((logits > xl).sum(1) < k).sum())


def partner(i, batch, n_mixup):
  return n_mixup - 1 - i if i < n_mixup else n_mixup + batch - 1 - i


def mix_images_ref(x, n_mixup, weights, boxes):
  """numpy float32, out of place: mixup rows x_i w_i + x_partner (1 - w_i); cutmix rows x_partner inside row i's own box."""
  b = x.shape[0]
  out = x.copy()
  for i in range(b):
    p = partner(i, b, n_mixup)
    if i < n_mixup:
      w = np.float32(weights[i])
      out[i] = x[i] * w + x[p] * (np.float32(1) - w)
    else:
      y1, x1, y2, x2 = (int(v) for v in boxes[i])
      out[i, y1:y2, x1:x2] = x[p, y1:y2, x1:x2]
  return out


def cutmix_area(boxes, batch, n_mixup, h, w):
  """The one scalar of the cutmix part: sum of the box areas / ((batch - n_mixup) h w), the mean of datasets.py:236."""
  area = sum(max(int(b[2]) - int(b[0]), 0) * max(int(b[3]) - int(b[1]), 0) for b in boxes[n_mixup:])
  return np.float32(area) / np.float32((batch - n_mixup) * h * w)


def mix_labels_ref(labels, nc, n_mixup, weights, boxes, h, w):
  b = len(labels)
  onehot = np.eye(nc, dtype=np.float32)[np.asarray(labels)]
  out = np.zeros((b, nc), np.float32)
  a = cutmix_area(boxes, b, n_mixup, h, w) if n_mixup < b else np.float32(0)
  for i in range(b):
    p = partner(i, b, n_mixup)
    if i < n_mixup:
      wi = np.float32(weights[i])
      out[i] = wi * onehot[i] + (np.float32(1) - wi) * onehot[p]
    else:
      out[i] = (np.float32(1) - a) * onehot[i] + a * onehot[p]
  return out


# ------------------------------------------------------------------------------------ CPU
def test_new_entry_points_are_declared_and_bound():
  header = open(os.path.join(ROOT, 'include', 'edet_hip.h')).read()
  stubs = open(os.path.join(ROOT, 'automl_amd', 'csrc', 'plan_stubs.inc')).read()
  for name in NEW:
    assert name in _lib.SIGNATURES
    assert 'int %s(' % name in header
    assert '"%s"' % name in stubs
  # the soft-label twin: edet_softmax_xent's list with (soft_labels, label_ld) in place of labels
  assert len(_lib.SIGNATURES['edet_softmax_xent_soft']) == len(_lib.SIGNATURES['edet_softmax_xent']) + 1


def test_cutmix_box_known_answers():
  """datasets.py:191-203 by hand, h = w = 8.
  (r_y 7, r_x 0, area 0.75): ratio = sqrt(0.25) = 0.5, r_w = r_h = int(4.0) = 4, half = 2: x 0 -+ 2 -> clip(-2), 2 = 0, 2;
  y 7 -+ 2 -> 5, clip(9) = 8.  (4, 4, 0): ratio 1, r = 8, half 4: 0, 8 both ways.  (3, 5, 1): ratio 0, r = 0: empty at the
  centre."""
  box = effnetv2_train.cutmix_box
  assert box(7, 0, 0.75, 8, 8) == (5, 0, 8, 2)
  assert box(4, 4, 0.0, 8, 8) == (0, 0, 8, 8)
  assert box(3, 5, 1.0, 8, 8) == (3, 5, 3, 5)
  # non-square, h = 10, w = 7, centre (r_y 2, r_x 6), area 0.36: ratio = sqrt(0.64) = 0.8 (float32 0.800000012),
  # r_w = int(0.8 * 7 = 5.6) = 5, r_h = int(0.8 * 10 = 8.0000001) = 8; r_w // 2 = 2, r_h // 2 = 4:
  # x: 6 - 2 = 4, 6 + 2 = 8 -> clip to w = 7; y: 2 - 4 = -2 -> 0, 2 + 4 = 6
  assert box(2, 6, 0.36, 10, 7) == (0, 4, 6, 7)
  # truncation, not rounding: area 0.19 -> ratio 0.9, r_w = int(0.9 * 7 = 6.3) = 6, r_h = int(9.0 -+ an ulp)
  y1, x1, y2, x2 = box(5, 3, 0.19, 10, 7)
  assert (x1, x2) == (0, 6) and y2 - y1 in (8, 9)


def test_split_rule():
  split = effnetv2_train.mix_split
  for b in (1, 2, 5, 8, 256):
    assert split(b, 0.4, 0.4) == b // 2      # both: half and half (datasets.py:287-294)
    assert split(b, 0.4, 0.0) == b           # mixup only
    assert split(b, 0.0, 0.4) == 0           # cutmix only
    assert split(b, 0.0, 0.0) is None        # off
  assert split(5, 0.2, 0.5) == 2
  # what the named models ask for (effnetv2_configs: 0 for S and the B models, 0.2 for M, 0.5 for L / XL)
  assert effnetv2_train.mix_alphas('efficientnetv2-s') == (0.0, 0.0)
  assert effnetv2_train.mix_alphas('efficientnetv2-m') == (0.2, 0.2)
  assert effnetv2_train.mix_alphas('efficientnetv2-l') == (0.5, 0.5)
  assert effnetv2_train.mix_alphas('efficientnetv2-xl') == (0.5, 0.5)
  assert effnetv2_train.mix_alphas('efficientnetv2-b0') == (0.0, 0.0)


def test_draws():
  """Beta(a, a) has mean 1/2 and variance 1 / (4 (2a + 1)); the mixup weight is the draw folded into [1/2, 1]."""
  alpha, n = 0.4, 20000
  beta = effnetv2_train.draw_beta(effnetv2_train.mix_rng(11), alpha, n)
  var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
  assert abs(beta.mean() - 0.5) <= 4.0 * np.sqrt(var / n), beta.mean()
  assert abs(beta.var() - var) <= 0.1 * var, (beta.var(), var)
  rng = effnetv2_train.mix_rng(11)
  for b, h, w, ma, ca in ((8, 8, 8, 0.4, 0.4), (5, 33, 17, 0.4, 0.4), (6, 8, 8, 0.4, 0.0), (6, 10, 7, 0.0, 0.4)):
    n_mixup = effnetv2_train.mix_split(b, ma, ca)
    for _ in range(50):
      wts, boxes = effnetv2_train.draw_mix(rng, b, h, w, ma, ca)
      assert wts.dtype == np.float32 and boxes.dtype == np.int32 and wts.shape == (b,) and boxes.shape == (b, 4)
      assert (wts >= 0.5).all() and (wts <= 1.0).all()
      assert (wts[n_mixup:] == 1.0).all() and (boxes[:n_mixup] == 0).all()
      y1, x1, y2, x2 = boxes.T
      assert (0 <= y1).all() and (y1 <= y2).all() and (y2 <= h).all() and (0 <= x1).all() and (x1 <= x2).all() and (x2 <= w).all()
  # seeded by the model's seed; the state survives the round trip through the optimizer state's words
  a, b = effnetv2_train.mix_rng(3), effnetv2_train.mix_rng(3)
  assert np.array_equal(effnetv2_train.draw_mix(a, 5, 8, 8, 0.4, 0.4)[0], effnetv2_train.draw_mix(b, 5, 8, 8, 0.4, 0.4)[0])
  assert not np.array_equal(effnetv2_train.draw_beta(effnetv2_train.mix_rng(4), 0.4, 4), effnetv2_train.draw_beta(effnetv2_train.mix_rng(3), 0.4, 4))
  a.integers(0, 7)      # leaves a buffered 32-bit half behind
  words = effnetv2_train._pack_rng_state(a)
  assert words.dtype == np.uint64 and words.shape == (6,)
  want = effnetv2_train.draw_mix(a, 5, 8, 8, 0.4, 0.4)
  effnetv2_train._unpack_rng_state(b, words)
  got = effnetv2_train.draw_mix(b, 5, 8, 8, 0.4, 0.4)
  assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])


def test_trainer_mix_options():
  """No GPU needed: the constructor, set_mix_alphas and the refusal of float labels with mixing on (before any launch)."""
  t = effnetv2_train.TrainableModel('efficientnetv2-b0', 'num_classes=24')
  assert not t.mixing and t.mixup_alpha == 0.0 and t.cutmix_alpha == 0.0
  t = effnetv2_train.TrainableModel('efficientnetv2-b0', 'num_classes=24', mixup_alpha=0.2, cutmix_alpha=0.5)
  assert t.mixing and (t.mixup_alpha, t.cutmix_alpha) == (0.2, 0.5)
  images = np.zeros((4, 64, 64, 3), np.float32)
  onehot = np.eye(24, dtype=np.float32)[[0, 1, 2, 3]]
  with pytest.raises(ValueError, match='float labels'):
    t.train_step((images, onehot))
  t.set_mix_alphas(0, 0)
  assert not t.mixing
  with pytest.raises(ValueError):
    t.set_mix_alphas(-0.1, 0)
  with pytest.raises(ValueError):      # float labels of another width
    t.train_step((images, np.zeros((4, 23), np.float32)))


# ------------------------------------------------------------------------------------ GPU: edet_softmax_xent_soft
def _soft_problem(name, tdt, b, nc, seed):
  """The logits of _xent_problem (rows with max x ~ 80, a row with tied logits) and soft labels: two-hot rows (w, 1 - w) on
  the sparse problem's label and another class; rows 1, 5, .. an exact 0.5 / 0.5 tie (the class is the lower index);
  rows 2, 6, .. scaled to sum to 0.7."""
  logits, labels = _xent_problem(name, tdt, b, nc, seed)
  rng = np.random.default_rng(seed + 1)
  y = np.zeros((b, nc), np.float32)
  for r in range(b):
    l = int(labels[r])
    o = (l + 3) % nc
    w = np.float32(rng.uniform(0.55, 1.0))
    if r % 4 == 1:
      w = np.float32(0.5)
    y[r, l] = w
    y[r, o] = np.float32(1) - w
    if r % 4 == 2:
      y[r] *= np.float32(0.7)
  return logits, labels, torch.from_numpy(y)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('nc', [5, 24, 1000, 1001])
@pytest.mark.parametrize('b', [1, 8, 256])
@pytest.mark.parametrize('smoothing', [0.0, 0.1], ids=['hard', 'ls0.1'])
def test_softmax_xent_soft(dt, nc, b, smoothing):
  """Against the float64 restatement with autograd, at test_softmax_xent's tolerances: loss 1e-3 |loss| + 1e-5, dlogits
  rtol 1e-2 (bf16) / 1e-4 (fp32) of the largest gradient, padding columns exactly zero, both counts exact; label rows of
  exactly num_classes floats (no alignment, column by column) and padded to a multiple of 8 (16-byte loads)."""
  name, edt, tdt = dt
  logits, labels, y = _soft_problem(name, tdt, b, nc, gu.seed_of(nc, b, smoothing))
  assert float(logits.max()) > 75
  if b >= 8:
    assert int(np.argmax(y[1].numpy())) == min(int(labels[1]), (int(labels[1]) + 3) % nc) and float(y[1].max()) == 0.5
    assert abs(float(y[2].sum()) - 0.7) < 1e-6
  xq = logits.double().requires_grad_(True)
  want = xent_soft(xq, y.double(), smoothing)
  gscale = 1.0 if nc != 24 else 0.37
  (want * gscale).backward()
  loss = float(want.detach())
  top1, top5 = topk_rows_soft(logits, y, 1), topk_rows_soft(logits, y, 5)
  ld = gu.to_dev(logits.view(b, 1, 1, nc), tdt)
  ld[..., nc:] = 7.0                       # padding columns may hold anything
  dl = torch.full_like(ld, float('nan'))
  sums = torch.zeros(4, dtype=torch.float32, device=gu.DEV)
  y_tight = y.to(gu.DEV).contiguous()
  y_wide = torch.full((b, gu.pad8(nc) + 8), 3.0, dtype=torch.float32, device=gu.DEV)
  y_wide[:, :nc] = y_tight
  wsp = torch.empty(4096, dtype=torch.float32, device=gu.DEV)

  def run(ws, yd):
    sums.zero_()
    dl.fill_(float('nan'))
    call('edet_softmax_xent_soft', ptr(ld), ld.shape[-1], ptr(yd), yd.shape[1], b, nc, smoothing, gscale, ptr(dl), ptr(sums),
         ptr(ws), ws.numel() * 4 if ws is not None else 0, edt, gu.stream())
    torch.cuda.synchronize()
    return sums.cpu().clone(), dl.clone()
  s, d = run(wsp, y_tight)
  s2, d2 = run(wsp, y_tight)
  assert torch.equal(s, s2) and torch.equal(d.view(torch.uint8), d2.view(torch.uint8)), 'run-to-run difference'
  s3, d3 = run(None, y_wide)               # no workspace: one workgroup walks the rows
  s4, d4 = run(wsp, y_wide)
  s5, d5 = run(None, y_tight)
  print('softmax_xent_soft %s nc=%d b=%d ls=%g: loss %.6f vs %.6f, top1 %d top5 %d' % (name, nc, b, smoothing, float(s[0]), loss,
                                                                                      top1, top5))
  for got in (s, s3, s4, s5):
    assert abs(float(got[0]) - loss) <= 1e-3 * abs(loss) + 1e-5, (float(got[0]), loss)
    assert int(got[1]) == top1 and int(got[2]) == top5, (got, top1, top5)
    assert float(got[3]) == 0.0
  for got in (d, d3, d4, d5):
    gu.check(got.view(b, -1)[:, :nc], xq.grad.float(), name, 'dlogits', rtol=1e-2 if name == 'bf16' else 1e-4)
    assert ld.shape[-1] == nc or float(got[..., nc:].abs().max()) == 0.0
  # one-hot rows: the counts of the sparse kernel exactly, its loss within the tolerance
  onehot = torch.nn.functional.one_hot(labels.long(), nc).float().to(gu.DEV).contiguous()
  so, _ = run(wsp, onehot)
  sums.zero_()
  lab = labels.to(gu.DEV)
  call('edet_softmax_xent', ptr(ld), ld.shape[-1], ptr(lab), b, nc, smoothing, gscale, ptr(dl), ptr(sums), ptr(wsp),
       wsp.numel() * 4, edt, gu.stream())
  torch.cuda.synchronize()
  sp = sums.cpu()
  assert int(so[1]) == int(sp[1]) and int(so[2]) == int(sp[2]), (so, sp)
  assert abs(float(so[0]) - float(sp[0])) <= 1e-3 * abs(float(sp[0])) + 1e-5, (so, sp)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('entry', ['edet_softmax_xent', 'edet_softmax_xent_soft'])
def test_softmax_xent_without_workspace(entry, dt):
  """workspace = NULL against a workspace, sums starting at [0.5, 2, 3, 7].  Batch 1..4 is one workgroup either way: the
  same bits everywhere.  Batch 9 is three workgroups with partial rows against ONE workgroup whose waves walk rows w, w + 4,
  w + 8 and add into sums themselves: a row's arithmetic does not know the grid, so dlogits has the same bits and the counts
  are equal; the loss is the same 9 non-negative terms and the 0.5 added in another order -- at most 10 additions each way,
  each rounding by at most 2^-24 of a partial sum that is at most the total, so the two differ by at most 2 * 10 * 2^-24 *
  total (24 taken for the second-order terms).  sums[3] is nobody's."""
  name, edt, tdt = dt
  nc, smoothing = 24, 0.1
  for b in (1, 2, 3, 4, 9):
    logits, labels, y = _soft_problem(name, tdt, b, nc, gu.seed_of('no_workspace', b))
    ld = gu.to_dev(logits.view(b, 1, 1, nc), tdt)
    lab, yd = labels.to(gu.DEV), y.to(gu.DEV).contiguous()
    wsp = torch.empty(4096, dtype=torch.float32, device=gu.DEV)

    def run(ws):
      sums = torch.tensor([0.5, 2.0, 3.0, 7.0], dtype=torch.float32, device=gu.DEV)
      dl = torch.full_like(ld, float('nan'))
      tgt = (ptr(lab),) if entry == 'edet_softmax_xent' else (ptr(yd), yd.shape[1])
      call(entry, ptr(ld), ld.shape[-1], *tgt, b, nc, smoothing, 1.0, ptr(dl), ptr(sums), ptr(ws),
           ws.numel() * 4 if ws is not None else 0, edt, gu.stream())
      torch.cuda.synchronize()
      return sums.cpu(), dl
    s_ws, d_ws = run(wsp)
    s_no, d_no = run(None)
    print('%s %s b=%d: sums %s (workspace) %s (none)' % (entry, name, b, s_ws.tolist(), s_no.tolist()))
    assert torch.equal(d_ws.view(torch.uint8), d_no.view(torch.uint8)), b
    assert torch.equal(s_ws[1:], s_no[1:]) and float(s_no[3]) == 7.0, (b, s_ws, s_no)
    assert float(s_no[1]) >= 2.0 and float(s_no[2]) >= float(s_no[1]) + 1.0, (b, s_no)      # added into, top5 >= top1
    assert float(s_no[0]) > 0.5, (b, s_no)
    if b <= 4:
      assert float(s_ws[0]) == float(s_no[0]), (b, s_ws, s_no)
    else:
      assert abs(float(s_ws[0]) - float(s_no[0])) <= 24 * 2.0 ** -24 * float(s_ws[0]), (b, s_ws, s_no)


@pytest.mark.gpu
def test_softmax_xent_soft_refuses_bad_arguments():
  x = torch.zeros(2, 8, device=gu.DEV)
  y = torch.zeros(2, 16, device=gu.DEV)
  s = torch.zeros(4, device=gu.DEV)
  f32 = _lib.EDET_F32
  with pytest.raises(_lib.EdetError):      # ld < C
    call('edet_softmax_xent_soft', ptr(x), 8, ptr(y), 16, 2, 9, 0.0, 1.0, ptr(x), ptr(s), None, 0, f32, gu.stream())
  with pytest.raises(_lib.EdetError):      # label_ld < C
    call('edet_softmax_xent_soft', ptr(x), 8, ptr(y), 7, 2, 8, 0.0, 1.0, ptr(x), ptr(s), None, 0, f32, gu.stream())
  with pytest.raises(_lib.EdetError):      # smoothing
    call('edet_softmax_xent_soft', ptr(x), 8, ptr(y), 16, 2, 8, 1.5, 1.0, ptr(x), ptr(s), None, 0, f32, gu.stream())
  with pytest.raises(_lib.EdetError):      # null labels
    call('edet_softmax_xent_soft', ptr(x), 8, None, 16, 2, 8, 0.0, 1.0, ptr(x), ptr(s), None, 0, f32, gu.stream())
  with pytest.raises(_lib.EdetError):
    call('edet_mix_images', ptr(x), 2, 1, 1, 4, 3, ptr(s), None, f32, gu.stream())
  w = torch.zeros(2, device=gu.DEV)
  bx = torch.zeros(2, 4, dtype=torch.int32, device=gu.DEV)
  with pytest.raises(_lib.EdetError):      # n_mixup > batch
    call('edet_mix_images', ptr(x), 2, 1, 1, 4, 3, ptr(w), ptr(bx), f32, gu.stream())
  lab = torch.zeros(2, dtype=torch.int32, device=gu.DEV)
  with pytest.raises(_lib.EdetError):      # label_ld < C
    call('edet_mix_labels', ptr(lab), 2, 17, 4, 4, 1, ptr(w), ptr(bx), ptr(y), 16, gu.stream())


# ------------------------------------------------------------------------------------ GPU: the mix kernels
def _mix_draws(b, n_mixup, h, w, seed):
  """Weights in [0.5, 1] for the mixup rows; for the cutmix part a fixed catalogue: the first and the last row (partners)
  hold two boxes that overlap, then in turn an empty box, a box that touches two edges, the whole image and an inner box, so
  that pairs of every kind occur; an odd part has a self-partnered middle row."""
  rng = np.random.default_rng(seed)
  weights = np.ones(b, np.float32)
  weights[:n_mixup] = rng.uniform(0.5, 1.0, n_mixup).astype(np.float32)
  if n_mixup >= 2:
    weights[1] = 1.0                      # w = 1: the row keeps itself
  inner = (1, 1, h - 1, w - 1)
  catalogue = [inner, (h // 2, w // 2, h // 2, w // 2), (0, 0, h // 2 + 1, w // 2 + 1), (0, 0, h, w), (h // 2, 1, h, w - 2)]
  boxes = np.zeros((b, 4), np.int32)
  m = b - n_mixup
  for k in range(m):
    boxes[n_mixup + k] = catalogue[k % len(catalogue)]
  if m >= 2:
    boxes[b - 1] = (0, 2, h // 2 + 1, w)      # overlaps `inner` of the part's first row
  return weights, boxes


def _mix_cases():
  out = []
  for b in (1, 2, 5, 8):
    for n in sorted({0, b // 2, b}):
      out.append((b, n))
  return out


@pytest.mark.gpu
@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('hw', [(8, 8), (5, 7), (33, 17)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('bn', _mix_cases(), ids=lambda c: 'b%d_n%d' % c)
def test_mix_images(dt, hw, bn):
  """In place on the device against the out-of-place numpy float32 restatement.  Cutmix rows bit for bit (selection only;
  pixels outside the boxes and a self-partnered row are the input's bits).  Mixup rows, with t1 = x_i w and
  t2 = x_partner (1 - w): fp32 within 4 * 2^-24 (|t1| + |t2|) -- two products and a sum rounded once each on either side,
  1 - w exact or rounded once, a fused multiply-add on either side only removes a rounding -- and bf16 within that plus
  half a bf16 ulp of the result.  bf16 keeps 8 significant bits, so for a result r in [2^e, 2^(e+1)) half an ulp is
  2^(e-8): between 2^-9 |r| (top of the binade) and 2^-8 |r| (bottom).  The figure 2^-9 |result| that the feature request
  puts beside "half a bf16 ulp" is the lower end of that range and no correctly rounded bf16 store can keep it over a whole
  binade (measured on the MI355X with it: b2_n2-8x8-bf16 row 0, error 0.0037 above the bound at |result| ~ 2, i.e. the
  rounding error of 2^-8 * 2 = 0.0078 that the format gives); the bound here is the exact half ulp of each result."""
  name, edt, tdt = dt
  (h, w), (b, n_mixup) = hw, bn
  c = 3
  rng = np.random.default_rng(gu.seed_of(h, w, b, n_mixup))
  x = gu.rnd(rng, (b, h, w, c), tdt, 2.0).numpy()
  weights, boxes = _mix_draws(b, n_mixup, h, w, gu.seed_of('draws', h, w, b, n_mixup))
  want = mix_images_ref(x, n_mixup, weights, boxes)
  n = b * h * w * c
  flat = torch.full((n + 64,), 5.0, dtype=tdt, device=gu.DEV)      # a canary behind the batch
  wd = torch.from_numpy(weights).to(gu.DEV)
  bd = torch.from_numpy(boxes).to(gu.DEV)

  def run():
    flat[:n] = torch.from_numpy(x).reshape(-1).to(device=gu.DEV, dtype=tdt)
    call('edet_mix_images', ptr(flat), b, h, w, c, n_mixup, ptr(wd), ptr(bd), edt, gu.stream())
    torch.cuda.synchronize()
    assert float((flat[n:].float() - 5.0).abs().max()) == 0.0, 'write behind the batch'
    return flat[:n].clone().view(b, h, w, c)
  got_dev = run()
  assert torch.equal(run().view(torch.uint8), got_dev.view(torch.uint8)), 'run-to-run difference'
  got = got_dev.float().cpu().numpy()
  if n_mixup < b:
    assert np.array_equal(got[n_mixup:].view(np.uint32), want[n_mixup:].view(np.uint32)), 'cutmix rows are pure selection'
    m = b - n_mixup
    if m % 2:
      mid = n_mixup + m // 2
      assert np.array_equal(got[mid].view(np.uint32), x[mid].view(np.uint32)), 'self-partnered cutmix row'
    if m >= 2:      # the overlapping pair really swapped something, and left something alone
      assert not np.array_equal(got[n_mixup], x[n_mixup]) and np.array_equal(got[n_mixup, 0, 0], x[n_mixup, 0, 0])
  for i in range(n_mixup):
    p = partner(i, b, n_mixup)
    wi = np.float64(weights[i])
    t1, t2 = np.abs(x[i].astype(np.float64) * wi), np.abs(x[p].astype(np.float64) * (1.0 - wi))
    bound = 4.0 * 2.0 ** -24 * (t1 + t2)
    if name == 'bf16':
      bound = bound + np.ldexp(1.0, np.frexp(want[i].astype(np.float64))[1] - 9)      # frexp: |r| = m 2^ex, m in [1/2, 1)
    err = np.abs(got[i].astype(np.float64) - want[i].astype(np.float64))
    print('mix_images %s %dx%d b=%d n=%d row %d: max err / bound %.3f' % (name, h, w, b, n_mixup, i, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), ('mixup row', i, float((err - bound).max()))
  if n_mixup >= 2:
    assert np.array_equal(got[1], x[1]) and not np.array_equal(got[0], x[0])      # w = 1 keeps the row; its partner mixes


@pytest.mark.gpu
@pytest.mark.parametrize('nc', [5, 1001])
@pytest.mark.parametrize('bn', _mix_cases(), ids=lambda c: 'b%d_n%d' % c)
def test_mix_labels(nc, bn):
  b, n_mixup = bn
  h, w = 5, 7
  rng = np.random.default_rng(gu.seed_of(nc, b, n_mixup))
  labels = rng.integers(0, nc, b).astype(np.int32)
  if n_mixup >= 2:
    labels[n_mixup - 1] = labels[0]        # a mixup pair of one class
  if b - n_mixup >= 4:
    labels[b - 2] = labels[n_mixup + 1]    # and a cutmix pair of one class
  if b - n_mixup >= 2 and labels[n_mixup] == labels[b - 1]:
    labels[b - 1] = (labels[b - 1] + 1) % nc      # the cutmix part's outer pair: two classes
  weights, boxes = _mix_draws(b, n_mixup, h, w, gu.seed_of('draws', nc, b, n_mixup))
  want = mix_labels_ref(labels, nc, n_mixup, weights, boxes, h, w)
  ld = gu.pad8(nc)
  out = torch.full((b, ld), float('nan'), dtype=torch.float32, device=gu.DEV)
  ldv, wd, bd = (torch.from_numpy(t).to(gu.DEV) for t in (labels, weights, boxes))
  call('edet_mix_labels', ptr(ldv), b, nc, h, w, n_mixup, ptr(wd), ptr(bd), ptr(out), ld, gu.stream())
  torch.cuda.synchronize()
  got = out.cpu().numpy()
  assert ld > nc and float(np.abs(got[:, nc:]).max()) == 0.0
  assert np.isfinite(got).all()
  assert float(np.abs(got[:, :nc] - want).max()) <= 2.0 ** -23
  if n_mixup >= 2:      # partner of the same class: one entry, 1 within 2^-23
    assert abs(float(got[0, labels[0]]) - 1.0) <= 2.0 ** -23 and int((got[0] != 0).sum()) == 1
  if b - n_mixup >= 4:
    assert abs(float(got[n_mixup + 1, labels[b - 2]]) - 1.0) <= 2.0 ** -23 and int((got[b - 2] != 0).sum()) == 1
  if b - n_mixup >= 2:  # the part's one scalar, read from a row whose partner has another class
    a = float(cutmix_area(boxes, b, n_mixup, h, w))
    assert 0.0 < a < 1.0
    i, p = n_mixup, b - 1
    assert labels[i] != labels[p]
    assert abs(float(got[i, labels[p]]) - a) <= 2.0 ** -23 and abs(float(got[p, labels[i]]) - a) <= 2.0 ** -23
    assert abs(float(got[i, labels[i]]) - (1.0 - a)) <= 2.0 ** -23


# ------------------------------------------------------------------------------------ GPU: the train step
MODEL, OVER, SIZE, NC = 'efficientnetv2-b0', 'num_classes=24', 64, 24


def oracle_mixed_step(vals, images, soft_labels, smoothing, weight_decay, drop_scale, dropout_mask):
  """tests.test_effnetv2_train.oracle_train_step with the soft-label loss; everything downstream of the loss is the same."""
  params = {k: torch.from_numpy(np.array(v, dtype=np.float32)).requires_grad_(not k.endswith(('moving_mean', 'moving_variance')))
            for k, v in vals.items()}
  oracle = v2orc.V2Oracle(MODEL, OVER, params=params)
  oracle.drop_scale = drop_scale or {}
  ends = oracle.forward(torch.as_tensor(images, dtype=torch.float32), True)
  n = oracle.mconfig.model_name
  pooled = ends['pooled_features']
  if dropout_mask is not None:
    pooled = pooled * dropout_mask
  logits = pooled @ params[n + '/head/dense/kernel'] + params[n + '/head/dense/bias']
  loss = xent_soft(logits, torch.as_tensor(soft_labels), smoothing)
  l2 = sum((0.5 * weight_decay * (p * p).sum() for k, p in params.items()
            if p.requires_grad and netspec.is_l2_regularised(k)), torch.zeros(()))
  (loss + l2).backward()
  grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).numpy() for k, p in params.items() if p.requires_grad}
  return float(loss.detach()), float(l2.detach()), grads, logits.detach()


@pytest.mark.gpu
def test_mixed_train_step_matches_oracle_fp32():
  """One eager RMSprop step with mixup on rows [0, 2) and cutmix on rows [2, 5), fp32 storage, against the oracle that is
  handed the device's draws (mix weights and boxes, stochastic depth, dropout) and mixes in numpy.  Bounds: those of
  test_train_step_matches_oracle_fp32 (loss and L2 1e-3; gradients 1e-2 max(|g|_max, 1e-4 g_max) per tensor; the update
  within lr / sqrt(epsilon) times that), and the metric counts of the mixed labels exactly."""
  batch, lr, wd, smoothing = 5, 0.01, 1e-4, 0.1
  spec = effnetv2_model.V2Spec(effnetv2_configs.model_config(MODEL, OVER))
  vals = _perturbed(spec, 9)
  rng = np.random.default_rng(13)
  images = rng.standard_normal((batch, SIZE, SIZE, 3)).astype(np.float32)
  labels = np.array([3, 17, 5, 11, 20])
  net = effnetv2_train.TrainableModel(MODEL, OVER, dtype='f32', params=vals, use_graph=False, learning_rate=lr, weight_decay=wd,
                                      label_smoothing=smoothing, mixup_alpha=0.4, cutmix_alpha=0.4, seed=1)
  dev_images = torch.from_numpy(images).to(gu.DEV)
  out = net.train_step((dev_images, labels))
  torch.cuda.synchronize()
  assert torch.equal(dev_images.cpu(), torch.from_numpy(images)), 'the eager step mixed the caller\'s tensor'
  eng = net.engine
  assert eng.n_mixup == 2
  weights, boxes = eng.mix_weights.cpu().numpy(), eng.mix_boxes.cpu().numpy()
  area = float(cutmix_area(boxes, batch, 2, SIZE, SIZE))
  print('mix weights %s, boxes %s, cutmix area %.4f' % (weights, boxes.tolist(), area))
  assert (weights[:2] >= 0.5).all() and (weights[:2] < 1.0).all() and 0.0 < area < 1.0
  mixed = mix_images_ref(images, 2, weights, boxes)
  soft = mix_labels_ref(labels, NC, 2, weights, boxes, SIZE, SIZE)
  assert float(np.abs(eng.soft_labels.cpu().numpy()[:, :NC] - soft).max()) <= 2.0 ** -23
  drop_scale = {k[:-len(':out')]: m[:, 0].detach().cpu().clone() for k, (m, p) in eng.drop_masks.items()}
  loss, l2, grads, logits = oracle_mixed_step(vals, mixed, soft, smoothing, wd, drop_scale, eng.dropout_mask.cpu().clone())
  print('mixed step: loss %.6f (oracle %.6f), L2 %.6f (%.6f)' % (out['loss'] - out['reg_l2_loss'], loss, out['reg_l2_loss'], l2))
  assert abs(out['loss'] - out['reg_l2_loss'] - loss) <= 1e-3 * abs(loss), (out, loss)
  assert abs(out['reg_l2_loss'] - l2) <= 1e-3 * l2, (out, l2)
  assert out['acc_top1'] == topk_rows_soft(logits, soft, 1) / batch
  assert out['acc_top5'] == topk_rows_soft(logits, soft, 5) / batch
  got_g = eng.get_grads()
  new = net.get_weights()
  gmax = max(float(np.abs(g).max()) for g in grads.values())
  bad_g, bad_w = [], []
  for name, g in grads.items():
    bound = 1e-2 * max(float(np.abs(g).max()), 1e-4 * gmax)
    e = float(np.abs(np.asarray(got_g[name]).reshape(g.shape) - g).max())
    if not e <= bound:
      bad_g.append((name, e / bound))
    w, ms, mom = vals[name].copy(), np.zeros_like(g), np.zeros_like(g)
    rmsprop_step(w, g, ms, mom, lr)
    e = float(np.abs(new[name].reshape(w.shape) - w).max())
    if not e <= lr / np.sqrt(EPSILON) * bound:
      bad_w.append((name, e / (lr / np.sqrt(EPSILON) * bound)))
  assert not bad_g, 'gradient mismatch in %d/%d tensors, worst %s' % (len(bad_g), len(grads), sorted(bad_g, key=lambda t: -t[1])[:8])
  assert not bad_w, 'update mismatch in %d/%d tensors, worst %s' % (len(bad_w), len(grads), sorted(bad_w, key=lambda t: -t[1])[:8])


def _data(seed, steps, batch=4):
  rng = np.random.default_rng(seed)
  return [(rng.standard_normal((batch, SIZE, SIZE, 3)).astype(np.float32), rng.integers(0, NC, batch)) for _ in range(steps)]


def _net(**kw):
  args = dict(learning_rate=0.01, weight_decay=1e-5, label_smoothing=0.1, seed=4, mixup_alpha=0.4, cutmix_alpha=0.4)
  args.update(kw)
  return effnetv2_train.TrainableModel(MODEL, OVER, **args)


def _same_state(a, b, keys=('params_flat', 'velocity', 'adam_v', 'state_flat')):
  for key in keys:
    assert torch.equal(getattr(a.engine.arena, key), getattr(b.engine.arena, key)), key


@pytest.mark.gpu
def test_mixed_graph_replay_equals_eager():
  """bf16 storage, four mixed steps: one eager and three replays of the captured step (the mix kernels are its first
  launches, reading the static draw buffers) leave exactly the state and the losses of four eager steps; the draws differ
  from step to step."""
  data = _data(29, 4)
  runs = []
  for use_graph in (True, False):
    net = _net(use_graph=use_graph)
    outs, draws = [], []
    for d in data:
      outs.append(net.train_step(d))
      draws.append((net.engine.mix_weights.cpu().clone(), net.engine.mix_boxes.cpu().clone()))
    torch.cuda.synchronize()
    runs.append((net, outs, draws))
  (g, og, dg), (e, oe, de) = runs
  assert g._graph['graph'] is not None and g._graph['steps'] == 4 and e._graph is None
  assert og == oe, (og, oe)
  _same_state(g, e)
  for (wg, bg), (we, be) in zip(dg, de):
    assert torch.equal(wg, we) and torch.equal(bg, be)
  assert all(not torch.equal(dg[i][0], dg[i + 1][0]) for i in range(3)), 'the mixup weights did not change between steps'
  assert torch.equal(g.engine.soft_labels, e.engine.soft_labels) and float(g.engine.soft_labels.sum()) > 0
  # the replayed step read the static image buffer after it was refilled: it holds this step's MIXED images
  images, _ = g.input_buffers()
  assert not torch.equal(images.float().cpu(), torch.from_numpy(data[-1][0]).to(images.dtype).float())


@pytest.mark.gpu
def test_mixed_state_round_trip():
  """State and weights after step 2 -> a fresh model: its steps 3 and 4 are the uninterrupted ones bit for bit, the
  mixup / cutmix draws included."""
  data = _data(31, 4)
  net = _net(use_graph=False)
  net.train_step(data[0])
  net.train_step(data[1])
  state, weights = net.get_optimizer_state(), net.get_weights()
  assert 'mix_rng_state' in state and 'rng_state' in state
  other = _net(use_graph=False)
  other.set_weights(weights)
  other.set_optimizer_state(state)
  for d in data[2:]:
    want = net.train_step(d)
    got = other.train_step(d)
    assert got == want
    assert torch.equal(net.engine.mix_weights, other.engine.mix_weights)
    assert torch.equal(net.engine.mix_boxes, other.engine.mix_boxes)
  torch.cuda.synchronize()
  _same_state(net, other)


@pytest.mark.gpu
def test_float_onehot_labels_equal_integer_labels():
  """Mixing off, fp32 storage: float one-hot labels [B, C] give the loss of the integer labels within the kernel test's
  tolerance (1e-3 |loss| + 1e-5), the same counts, and gradients and updated variables within the kernel tests' fp32
  tolerance carried through the backward pass and the update (derived where it is applied below); test_step takes them too
  and updates nothing."""
  (images, labels), = _data(37, 1)
  onehot = np.eye(NC, dtype=np.float32)[labels]
  lr = 0.01
  nets = [_net(use_graph=False, mixup_alpha=0, cutmix_alpha=0, dtype='f32', learning_rate=lr) for _ in range(2)]
  start = effnetv2_model.init_params(nets[0].spec, 4)      # _net's seed: the variables before the step
  a = nets[0].train_step((images, labels))
  b = nets[1].train_step((images, onehot))
  torch.cuda.synchronize()
  assert abs(a['loss'] - b['loss']) <= 1e-3 * abs(a['loss']) + 1e-5, (a, b)
  assert a['acc_top1'] == b['acc_top1'] and a['acc_top5'] == b['acc_top5']
  # The two kernels' d(logits) agree within the kernel tests' fp32 tolerance, 1e-4 of the largest value, and the backward
  # pass is the same linear map in both runs.  Per tensor: 1e-4 of its largest gradient, with the absolute floor that
  # test_train_step_matches_oracle_fp32 grants a tensor whose true gradient is (nearly) zero -- a beta in front of another
  # BatchNorm holds fp32 summation noise only -- 1e-2 * 1e-4 = 1e-6 of the largest gradient of the model.  An updated
  # variable lies within lr / sqrt(epsilon) times that, the largest slope of the RMSprop step from zero slots (as there).
  ga, gb = nets[0].engine.get_grads(), nets[1].engine.get_grads()
  gmax = max(float(np.abs(g).max()) for g in ga.values())
  wa, wb = nets[0].get_weights(), nets[1].get_weights()
  moved, worst = 0, 0.0
  for name, w in wa.items():
    if name not in ga:      # moving statistics: the same forward pass
      assert np.array_equal(w, wb[name]), name
      continue
    g = np.asarray(ga[name])
    bound = max(1e-4 * float(np.abs(g).max()), 1e-6 * gmax)
    eg = float(np.abs(np.asarray(gb[name]) - g).max())
    ew = float(np.abs(np.asarray(wb[name]) - np.asarray(w)).max())
    worst = max(worst, eg / bound, ew / (lr / np.sqrt(EPSILON) * bound))
    assert eg <= bound, (name, eg, bound)
    assert ew <= lr / np.sqrt(EPSILON) * bound, (name, ew, lr / np.sqrt(EPSILON) * bound)
    moved += int(not np.array_equal(np.asarray(w).reshape(start[name].shape), start[name]))
  print('float one-hot against integer labels: worst error / bound %.3g over %d tensors' % (worst, len(ga)))
  assert moved > 100, 'the step moved %d tensors' % moved
  before = nets[1].get_weights()
  t_int = nets[1].test_step((images, labels))
  t_soft = nets[1].test_step((images, onehot))
  assert set(t_soft) == {'loss', 'reg_l2_loss', 'acc_top1', 'acc_top5'} and np.isfinite(t_soft['loss'])
  assert abs(t_int['loss'] - t_soft['loss']) <= 1e-3 * abs(t_int['loss']) + 1e-5
  assert t_int['acc_top1'] == t_soft['acc_top1'] and t_int['acc_top5'] == t_soft['acc_top5']
  after = nets[1].get_weights()
  assert all(np.array_equal(v, after[k]) for k, v in before.items()), 'test_step changed a variable'
  # a mixing model: test_step never mixes (and so takes float labels), train_step refuses them
  mixing = _net(use_graph=False, dtype='f32')
  mixing.set_weights(before)
  t_mix = mixing.test_step((images, onehot))
  assert abs(t_mix['loss'] - t_soft['loss']) <= 1e-3 * abs(t_soft['loss']) + 1e-5
  with pytest.raises(ValueError, match='float labels'):
    mixing.train_step((images, onehot))


@pytest.mark.gpu
def test_alphas_off_again_is_the_unmixed_step():
  """Two mixed steps (the second one a graph replay), then set_mix_alphas(0, 0): the captured step is dropped and the next
  step is bit for bit the step of a model that never mixed, started from the same state."""
  data = _data(43, 3)
  net = _net(use_graph=True)
  net.train_step(data[0])
  net.train_step(data[1])
  assert net._graph['graph'] is not None
  state, weights = net.get_optimizer_state(), net.get_weights()
  net.set_mix_alphas(0, 0)
  assert net._graph is None and not net.mixing
  plain = _net(use_graph=False, mixup_alpha=0.0, cutmix_alpha=0.0)
  plain.set_weights(weights)
  plain.set_optimizer_state(state)
  want = plain.train_step(data[2])
  got = net.train_step(data[2])
  torch.cuda.synchronize()
  assert got == want, (got, want)
  _same_state(net, plain)
  assert plain.engine.mix_weights is None
  # and on again, mixup only: another split, another captured step
  net.set_mix_alphas(0.2, 0)
  out = net.train_step(data[0])
  assert net.engine.n_mixup == 4 and np.isfinite(out['loss'])
