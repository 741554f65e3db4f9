"""EffNetV2Model: the reference's EfficientNetV2 interface on MI355X kernels (forward path).

Mirror of ``efficientnetv2/effnetv2_model.py``: ``EffNetV2Model(model_name, model_config, include_top)
(inputs[B,H,W,3], training=False, with_endpoints=False)`` (:532-658) built from Stem (:409-432),
MBConvBlock (:187-310), FusedMBConvBlock (:313-406), SE (:105-147) and Head (:435-497).
Variable names follow the Keras model (model name as prefix, ``blocks_%d``, per-block ``conv2d[_1]`` /
``tpu_batch_normalization[_1,_2]`` counters, ``se/conv2d[_1]``, ``head/...``).

Scope: the forward pass in both BatchNorm modes and the backward
pass of the whole graph (``backward(d_outputs)``: Fused-MBConv dense convolutions, MBConv, SE, stochastic depth,
head, dense layer).  The classifier's training step -- softmax cross-entropy with label smoothing, head dropout, the
RMSprop / momentum / Adam update (``efficientnetv2/main_tf2.py``) -- is ``effnetv2_train.TrainableModel`` on the
V2Engine methods at the end of this file (``softmax_loss`` for sparse or soft labels, ``head_dropout``, ``mix_batch`` for
mixup / cutmix, ``randaug_batch`` for RandAugment on uint8 images) and the layer engine's update step
(``LayerEngine.optimizer_local`` / ``optimizer_apply`` with the trainer's ``Update`` description).
``EffNetV2Model.__call__(training=True)`` itself still refuses dropout (pass ``model_config='dropout_rate=0'``): it has
no labels to train with, and only the trainer owns the draws.  ``conv_dropout`` is not built anywhere.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from automl_amd import _lib
from automl_amd import effnetv2_configs
from automl_amd import layer_engine
from automl_amd import netspec as netspec_lib
from automl_amd._lib import ACT_NONE, ACT_SWISH, call, ptr
from automl_amd.netspec import ParamSpec


class V2Spec(object):
  """Structure + variable list of one EffNetV2Model (creation order == the Keras layer order)."""

  def __init__(self, mconfig, include_top=True):
    self.mconfig = mconfig
    self.include_top = include_top
    if mconfig.act_fn not in ('silu', 'swish', None):
      raise ValueError('act_fn %r is out of scope (silu/swish only)' % (mconfig.act_fn,))
    if mconfig.bn_type not in (None, 'tpu_bn'):
      raise ValueError('bn_type %r is out of scope (batch norm only)' % (mconfig.bn_type,))
    if mconfig.data_format != 'channels_last':
      raise ValueError('only channels_last (NHWC) is built')
    self.bn_momentum = float(mconfig.bn_momentum)
    self.bn_epsilon = float(mconfig.bn_epsilon)
    self.act_code = ACT_SWISH      # (act_fn silu / swish, checked above)
    self.name = mconfig.model_name
    self.stem_filters, self.blocks = effnetv2_configs.expand_blocks(mconfig)
    # stochastic depth (effnetv2_model.py:624-629): survival_prob 0.8 -> per block 1 - 0.2 * idx / n
    sp = mconfig.survival_prob
    self.survival_probs = [(1.0 - (1.0 - sp) * float(b.index) / len(self.blocks)) if sp else None
                           for b in self.blocks]
    self.head_filters = effnetv2_configs.round_filters(mconfig.feature_size or 1280, mconfig)
    self.num_classes = mconfig.num_classes if include_top else 0
    self.params = []
    self._build()

  def _add(self, name, shape, init, trainable=True):
    self.params.append(ParamSpec(name, tuple(shape), init, trainable))

  def _bn(self, scope, c):
    self._add(scope + '/gamma', (c,), 'ones')
    self._add(scope + '/beta', (c,), 'zeros')
    self._add(scope + '/moving_mean', (c,), 'zeros', False)
    self._add(scope + '/moving_variance', (c,), 'ones', False)

  def _build(self):
    n = self.name
    self._add(n + '/stem/conv2d/kernel', (3, 3, 3, self.stem_filters), 'conv')
    self._bn(n + '/stem/tpu_batch_normalization', self.stem_filters)
    bn_names = ['tpu_batch_normalization', 'tpu_batch_normalization_1', 'tpu_batch_normalization_2']
    for b in self.blocks:
      s = '%s/blocks_%d' % (n, b.index)
      cexp = b.input_filters * b.expand_ratio
      k = b.kernel_size
      if b.conv_type == 0:       # MBConv
        ci = bi = 0
        if b.expand_ratio != 1:
          self._add(s + '/conv2d/kernel', (1, 1, b.input_filters, cexp), 'conv')
          self._bn('%s/%s' % (s, bn_names[bi]), cexp)
          ci, bi = 1, 1
        self._add(s + '/depthwise_conv2d/depthwise_kernel', (k, k, cexp, 1), 'conv')
        self._bn('%s/%s' % (s, bn_names[bi]), cexp)
        bi += 1
        if b.se_filters:
          self._se(s, cexp, b.se_filters)
        self._add('%s/%s/kernel' % (s, 'conv2d_1' if ci else 'conv2d'), (1, 1, cexp, b.output_filters), 'conv')
        self._bn('%s/%s' % (s, bn_names[bi]), b.output_filters)
      elif b.conv_type == 1:     # Fused-MBConv
        if b.expand_ratio != 1:
          self._add(s + '/conv2d/kernel', (k, k, b.input_filters, cexp), 'conv')
          self._bn(s + '/tpu_batch_normalization', cexp)
          if b.se_filters:
            self._se(s, cexp, b.se_filters)
          self._add(s + '/conv2d_1/kernel', (1, 1, cexp, b.output_filters), 'conv')
          self._bn(s + '/tpu_batch_normalization_1', b.output_filters)
        else:
          if b.se_filters:
            self._se(s, cexp, b.se_filters)
          self._add(s + '/conv2d/kernel', (k, k, cexp, b.output_filters), 'conv')
          self._bn(s + '/tpu_batch_normalization', b.output_filters)
      else:
        raise ValueError('conv_type %r is out of scope' % (b.conv_type,))
    self._add(n + '/head/conv2d/kernel', (1, 1, self.blocks[-1].output_filters, self.head_filters), 'conv')
    self._bn(n + '/head/tpu_batch_normalization', self.head_filters)
    if self.num_classes:
      self._add(n + '/head/dense/kernel', (self.head_filters, self.num_classes), 'dense')
      self._add(n + '/head/dense/bias', (self.num_classes,), 'zeros')

  def _se(self, s, c, se):
    self._add(s + '/se/conv2d/kernel', (1, 1, c, se), 'conv')
    self._add(s + '/se/conv2d/bias', (se,), 'zeros')
    self._add(s + '/se/conv2d_1/kernel', (1, 1, se, c), 'conv')
    self._add(s + '/se/conv2d_1/bias', (c,), 'zeros')

  def count_params(self):
    """All weights incl. BatchNorm moving statistics (Keras model.count_params(),
    effnetv2_model_test.py:24-52)."""
    return sum(int(np.prod(p.shape)) if p.shape else 1 for p in self.params)

  def reduction_indices(self):
    """Blocks whose outputs are reduction_1..5 (effnetv2_model.py:618-622)."""
    b = self.blocks
    return [i for i in range(len(b)) if i == len(b) - 1 or b[i + 1].stride > 1]


def init_value(spec, rng):
  """conv: N(0, sqrt(2/(kh*kw*cout))) (effnetv2_model.py:40-61); dense: U(+-1/sqrt(cout)) (:64-81)."""
  if spec.init == 'dense':
    lim = 1.0 / math.sqrt(spec.shape[1])
    return rng.uniform(-lim, lim, spec.shape).astype(np.float32)
  return netspec_lib.init_value(spec, rng)


def init_params(spec, seed=0):
  rng = np.random.default_rng(seed)
  return collections.OrderedDict((p.name, init_value(p, rng)) for p in spec.params)


class V2Engine(layer_engine.LayerEngine):
  """Launch plan of one EffNetV2Model on one MI355X (buffers, BatchNorm plumbing, the layer primitives and the update
  step come from LayerEngine): the graph, the classifier head with its dropout, and the softmax loss."""

  def __init__(self, spec, batch_size, image_size, update, dtype='bf16', device='cuda:0', seed=0, params=None, arena=None):
    if arena is None and (params is None or any(p.name not in params for p in spec.params)):
      params = {**init_params(spec, seed), **(params or {})}      # a partial set keeps the other initial values
    super().__init__(spec, batch_size, image_size, dtype=dtype, device=device, seed=seed, params=params, arena=arena,
                     update=update)
    # head dropout (effnetv2_model.py:464-467,483-484): set by effnetv2_train.TrainableModel only -- 0 = the plain cast
    self.head_dropout = 0.0
    self.dropout_mask = None      # fp32 [B, feature_size] in {0, 1 / (1 - rate)}, redrawn by refresh_drop_masks
    self.cls_sums = self.zbuf('cls_sums', (4,))      # mean loss, top-1 rows, top-5 rows, L2 loss (zeroed every pass)

  def forward(self, images, training=False, update_moving=True):
    """images: device tensor [B,H,W,3] in the engine dtype.  Fills self.endpoints / self.outputs.  A training pass reads
    the stochastic-depth and dropout masks as they are: they are drawn where they are created and redrawn by
    refresh_drop_masks, which the trainer calls in front of every step (eager or replayed) and nothing here does."""
    spec = self.spec
    self._begin(training, update_moving)
    n = self.batch
    name = spec.name
    x = self.stem(name, images, self.act)
    if training or spec.blocks[0].has_residual or spec.blocks[0].conv_type == 1:
      # the dense convolutions (and a first block that adds its input back) read a STORED tensor: the stem
      # output is materialised in activated form (one extra pass over a stride-2, 24..32-channel map)
      x = self.bn_res('stem:out', x, None)
    reds = set(spec.reduction_indices())
    self.endpoints = {'stem': x}
    ridx = 0
    for b in spec.blocks:
      scope = '%s/blocks_%d' % (name, b.index)
      x = self._mbconv(x, b, scope) if b.conv_type == 0 else self._fused_mbconv(x, b, scope)
      self.endpoints['block_%d' % b.index] = x
      if b.index in reds:
        ridx += 1
        self.endpoints['reduction_%d' % ridx] = x
    self.endpoints['features'] = x
    hv = self.pw('head:conv', x, name + '/head/conv2d/kernel', spec.head_filters,
                 bn=name + '/head/tpu_batch_normalization', act=ACT_SWISH)
    self.endpoints['head_1x1'] = hv
    r = hv.raw
    pooled = self.buf('head:pool', (n, r.c), torch.float32)
    call('edet_se_pool', ctypes.byref(hv.tview()), ptr(pooled), ptr(self.partials), self.partials.numel() * 4,
         self.dtype, self.stream, nbytes=r.rows * r.c * self.esize)
    self.pooled_sum, self.pooled_inv_hw = pooled, 1.0 / (r.h * r.w)
    self.head_view = hv
    self.logits = None
    self._dlogits_ready = False
    self._dropout_on = False
    if spec.num_classes:
      pv = layer_engine.Raw(self, 'head:pooled', n, 1, 1, r.c, needs_grad=False)
      self._dropout_on = bool(training and self.head_dropout)
      if self._dropout_on:
        if self.dropout_mask is None:
          self.dropout_mask = self.buf('head:dropmask', (n, r.c), torch.float32)
          if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('the head-dropout mask must exist before the step is captured (run one eager step)')
          self._draw_dropout_mask()
        call('edet_dropout_cast', ptr(pooled), ptr(self.dropout_mask), ptr(pv.data), n * r.c, self.dtype, self.stream)
      else:
        call('edet_cast', ptr(pooled), ptr(pv.data), n * r.c, self.dtype, self.stream)
      inv = self.buf('head:inv_hw', (2, r.c), torch.float32)
      inv[0].fill_(self.pooled_inv_hw)
      inv[1].zero_()
      view = layer_engine.View(pv)
      wt, ldk, _, _ = self._pw_copies(name + '/head/dense/kernel', r.c, spec.num_classes)
      out = layer_engine.Raw(self, 'head:logits', n, 1, 1, spec.num_classes, needs_grad=False)
      tv = view.tview()
      tv.scale, tv.shift = inv[0].data_ptr(), inv[1].data_ptr()      # mean = sum / (H*W) folded into the load
      call('edet_pw_fwd', ctypes.byref(tv), ptr(wt), ldk, ptr(self.param(name + '/head/dense/bias')),
           ptr(out.data), spec.num_classes, out.ld, None, ctypes.byref(self._nparts), self.dtype, self.stream)
      self.logits = out
      self._fc = (pv, tv, inv)
    return self.logits

  def backward(self, d_out=None):
    """Gradients of every variable for a given gradient of the model output (after forward(training=True)):
    d_out = d(logits) [B, num_classes] with include_top, else d(pooled features) [B, feature_size].  Fills
    grads_flat (get_grads()).  d_out = None: d(logits) is what softmax_loss() left in the 'head:dlogits' buffer (the
    classifier's training step, effnetv2_train.TrainableModel)."""
    spec = self.spec
    assert self.training, 'run forward(training=True) first'
    name = spec.name
    hv = self.head_view
    r = hv.raw
    n, c = r.n, r.c
    if d_out is None:
      assert spec.num_classes and self._dlogits_ready, 'backward() without d_out needs softmax_loss() after this forward pass'
    else:
      d_out = torch.as_tensor(d_out).to(device=self.device, dtype=torch.float32).reshape(n, -1)
    if spec.num_classes:
      pv, tv, inv = self._fc
      ncls = spec.num_classes
      dl = layer_engine.Raw(self, 'head:dlogits', n, 1, 1, ncls, needs_grad=False)
      if d_out is not None:
        dl.data.zero_()
        dl.data.reshape(n, -1)[:, :ncls] = d_out.to(self.tdtype)
      self._dlogits_ready = False
      g = _lib.GView(ptr(dl.data), None, None, None, None, n, 1, 1, ncls, dl.ld)
      wname = name + '/head/dense/kernel'
      _, _, wcopy, ldn = self._pw_copies(wname, c, ncls)
      call('edet_pw_bwd_weight', ctypes.byref(tv), ctypes.byref(g), ptr(self.grad(wname)), *self._ws(), self.dtype, self.stream)
      self._ws_mark()
      self.grad(name + '/head/dense/bias').add_(dl.data.reshape(n, -1)[:, :ncls].float().sum(0))
      dpv = self.buf('head:dpooled', (n, 1, 1, pv.ld), self.tdtype)
      epi = _lib.BwdEpi(ptr(dpv), 0, None, None, None, None)
      plain = _lib.TView(ptr(pv.data), None, None, None, ACT_NONE, n, 1, 1, c, pv.ld)
      call('edet_pw_bwd_data', ctypes.byref(g), ptr(wcopy), ldn, ctypes.byref(plain), ctypes.byref(epi),
           ctypes.byref(self._nparts), self.dtype, self.stream)
      d_mean = dpv.reshape(n, -1)[:, :c].float()          # d(mean-pooled features)
    else:
      d_mean = d_out
    # global average pooling backward: every pixel receives d_mean / (H*W); through swish' and the head BatchNorm
    dpool = self.buf('head:dpool', (n, c), torch.float32)
    dpool.copy_(d_mean * self.pooled_inv_hw)
    if spec.num_classes and self._dropout_on:      # the forward pass's mask on d(pooled), in place
      call('edet_dropout_cast', ptr(dpool), ptr(self.dropout_mask), ptr(dpool), n * c, _lib.EDET_F32, self.stream)
    gbuf = r.ensure_grad()
    gbuf.zero_()
    ones = self.buf('ones:%d:%d' % (n, c), (n, c), torch.float32)
    ones.fill_(1.0)
    gv = _lib.TView(ptr(r.data), ptr(hv.bn.scale), ptr(hv.bn.shift), ptr(ones), hv.act, r.n, r.h, r.w, c, r.ld)
    call('edet_se_gate_bwd', ctypes.byref(gv), ptr(gbuf), ptr(dpool), ptr(hv.bn.mean), ptr(hv.bn.rstd),
         ptr(self.partials), ctypes.byref(self._nparts), self.dtype, self.stream)
    self._bn_bwd_finalize(hv.bn, self._nparts.value)
    r.grad_written = True
    super().backward()

  # ---- classifier training (efficientnetv2/main_tf2.py:62-117): loss, dropout draws; the update is LayerEngine's -------
  def _draw_dropout_mask(self):
    """tf.keras.layers.Dropout(rate): keep with probability 1 - rate, kept values scaled by 1 / (1 - rate); one draw per
    (image, feature).  From the engine's generator, like the stochastic-depth masks."""
    keep = 1.0 - float(self.head_dropout)
    u = torch.rand(self.dropout_mask.shape, device=self.device, generator=self._rng)
    self.dropout_mask.copy_((u + keep).floor() / keep)

  def refresh_drop_masks(self):
    """New stochastic-depth draws and a new head-dropout mask (device-side, OUTSIDE any captured graph: the masks live in
    static buffers that a replayed step reads)."""
    super().refresh_drop_masks()
    if self.dropout_mask is not None:
      self._draw_dropout_mask()

  def softmax_loss(self, labels, label_smoothing=0.0, grad_scale=1.0):
    """CategoricalCrossentropy(label_smoothing, from_logits=True) of the logits of the last forward pass (main_tf2.py:199-207)
    against device labels: sparse int32 [B] (edet_softmax_xent; the caller has checked the range) or dense fp32 [B, >= C]
    with C valid columns (edet_softmax_xent_soft: one-hot or mixed rows, what the reference's input pipeline hands its
    loss).  Adds the mean loss and the top-1 / top-5 row counts to cls_sums[0:3] and, after a training forward pass, leaves
    d(logits) for backward()."""
    out = self.logits
    assert out is not None, 'softmax_loss needs a model with a classifier head (include_top)'
    ncls = self.spec.num_classes
    dl = layer_engine.Raw(self, 'head:dlogits', out.n, 1, 1, ncls, needs_grad=False)
    if labels.dtype == torch.int32:
      assert labels.is_contiguous() and labels.numel() == self.batch
      call('edet_softmax_xent', ptr(out.data), out.ld, ptr(labels), out.n, ncls, float(label_smoothing), float(grad_scale),
           ptr(dl.data), ptr(self.cls_sums), *self._ws(), self.dtype, self.stream)
    else:
      assert labels.dtype == torch.float32 and labels.is_contiguous() and labels.dim() == 2, 'labels: int32 [B] or fp32 [B, C]'
      assert labels.shape[0] == self.batch and labels.shape[1] >= ncls, (tuple(labels.shape), ncls)
      call('edet_softmax_xent_soft', ptr(out.data), out.ld, ptr(labels), int(labels.shape[1]), out.n, ncls,
           float(label_smoothing), float(grad_scale), ptr(dl.data), ptr(self.cls_sums), *self._ws(), self.dtype, self.stream)
    self._dlogits_ready = self.training

  # ---- mixup / cutmix (efficientnetv2/datasets.py:191-301) on the device -------------------------------------------------
  mix_weights = mix_boxes = soft_labels = None      # static buffers of mix_batch, created by set_mix_draws
  n_mixup = 0

  def set_mix_draws(self, weights, boxes, n_mixup):
    """This step's draws, made on the host by the trainer (effnetv2_train.draw_mix), into the static buffers that
    mix_batch's kernels read: weights fp32 [B] (mixup rows), boxes int32 [B, 4] = y1, x1, y2, x2 (cutmix rows); rows
    [0, n_mixup) are the mixup part.  Like refresh_drop_masks this runs OUTSIDE any captured graph, in front of every step;
    the copies are asynchronous from pinned memory and the step that follows them on the stream sees them."""
    b = self.batch
    if self.mix_weights is None:
      self.mix_weights = self.buf('mix:weights', (b,), torch.float32)
      self.mix_boxes = self.buf('mix:boxes', (b, 4), torch.int32)
      ld = (self.spec.num_classes + 7) // 8 * 8
      self.soft_labels = self.buf('mix:soft_labels', (b, ld), torch.float32)
    assert 0 <= int(n_mixup) <= b
    self.n_mixup = int(n_mixup)
    w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32).reshape(b)).pin_memory()
    x = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.int32).reshape(b, 4)).pin_memory()
    self.mix_weights.copy_(w, non_blocking=True)
    self.mix_boxes.copy_(x, non_blocking=True)

  def mix_batch(self, images, labels):
    """Mixes images [B, H, W, 3] (engine dtype, dense) IN PLACE and the sparse int32 labels [B] into the static soft-label
    buffer with the draws of set_mix_draws: edet_mix_images + edet_mix_labels, the first launches of a mixed step.
    -> soft labels fp32 [B, ld] for softmax_loss."""
    assert self.mix_weights is not None, 'mix_batch needs set_mix_draws first'
    b, (h, w) = self.batch, self.image_size
    assert images.is_contiguous() and images.dtype == self.tdtype and tuple(images.shape) == (b, h, w, 3), tuple(images.shape)
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == b
    call('edet_mix_images', ptr(images), b, h, w, 3, self.n_mixup, ptr(self.mix_weights), ptr(self.mix_boxes), self.dtype,
         self.stream, nbytes=2 * images.numel() * self.esize)
    call('edet_mix_labels', ptr(labels), b, self.spec.num_classes, h, w, self.n_mixup, ptr(self.mix_weights),
         ptr(self.mix_boxes), ptr(self.soft_labels), int(self.soft_labels.shape[1]), self.stream)
    return self.soft_labels

  # ---- RandAugment (efficientnetv2/autoaugment.py:663-702) on the device -----------------------------------------------
  ra_ops = ra_iargs = ra_fargs = ra_luts = None      # static buffers of randaug_batch, created by set_randaug_draws

  def set_randaug_draws(self, ops, iargs, fargs):
    """This step's RandAugment arguments, made on the host by the trainer (autoaugment.randaug_draws / randaug_args), into
    the static buffers that randaug_batch's kernels read: ops int32 [L, B], iargs int32 [L, B, 4], fargs fp32 [L, B, 8].
    Like set_mix_draws this runs OUTSIDE any captured graph, in front of every step, by asynchronous copies from pinned
    memory.  The number of layers is fixed at the first call (it is part of the launch sequence)."""
    b = self.batch
    ops = np.ascontiguousarray(ops, dtype=np.int32)
    layers = int(ops.shape[0])
    if self.ra_ops is None:
      self.ra_ops = self.buf('randaug:ops', (layers, b), torch.int32)
      self.ra_iargs = self.buf('randaug:iargs', (layers, b, 4), torch.int32)
      self.ra_fargs = self.buf('randaug:fargs', (layers, b, 8), torch.float32)
      self.ra_luts = self.buf('randaug:luts', (b, 3, 256), torch.uint8)
    assert tuple(ops.shape) == tuple(self.ra_ops.shape), (ops.shape, tuple(self.ra_ops.shape))
    for dst, src, dt in ((self.ra_ops, ops, np.int32), (self.ra_iargs, iargs, np.int32), (self.ra_fargs, fargs, np.float32)):
      dst.copy_(torch.from_numpy(np.ascontiguousarray(src, dtype=dt).reshape(tuple(dst.shape))).pin_memory(), non_blocking=True)

  def randaug_batch(self, images_u8, augment=True, norm=None):
    """uint8 images [B, H, W, 3] -> the static network-input buffer (engine dtype), normalised (x - 128) / 128 by the last
    layer's launch: per layer edet_randaug_stats + edet_randaug_apply with the arguments of set_randaug_draws, ping-pong
    through two uint8 buffers.  augment=False (test_step), or no layers: the normalising copy alone.  norm = (mean [3],
    std [3]): the legacy pipeline's (x - mean) / std instead, by edet_randaug_apply_norm as the last launch."""
    from automl_amd import autoaugment
    b, (h, w) = self.batch, self.image_size
    assert images_u8.dtype == torch.uint8 and images_u8.is_contiguous() and tuple(images_u8.shape) == (b, h, w, 3), (
        images_u8.dtype, tuple(images_u8.shape))
    out = self.buf('randaug:images', (b, h, w, 3), self.tdtype)
    if not augment or self.ra_ops is None or self.ra_ops.shape[0] == 0:
      return autoaugment.apply_layers(images_u8, out, None, None, None, None, None, self.stream, norm=norm)
    scratch = [self.buf('randaug:scratch%d' % k, (b, h, w, 3), torch.uint8) for k in range(min(int(self.ra_ops.shape[0]) - 1, 2))]
    return autoaugment.apply_layers(images_u8, out, self.ra_ops, self.ra_iargs, self.ra_fargs, self.ra_luts, scratch, self.stream,
                                    norm=norm)

  # ---- crop, resize and flip (efficientnetv2/preprocessing.py:22-70) on the device --------------------------------------
  crop_rows = None      # static int32 [B, 8] buffer of crop_batch (edet_crop_image_t rows), created by set_crop_rows

  def set_crop_rows(self, rows):
    """This step's crops and flip bits, made on the host by the trainer (v2_preprocessing.train_rows / eval_rows), into the
    static buffer that crop_batch's kernel reads: int32 [B, 8] in edet_crop_image_t's field order.  Like set_mix_draws this
    runs OUTSIDE any captured graph, in front of every step, by an asynchronous copy from pinned memory."""
    b = self.batch
    if self.crop_rows is None:
      self.crop_rows = self.buf('crop:rows', (b, 8), torch.int32)
    r = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32).reshape(b, 8)).pin_memory()
    self.crop_rows.copy_(r, non_blocking=True)

  def crop_batch(self, raw_u8, to_u8, method='bilinear', norm=None):
    """Decoded uint8 images on a common canvas [B, Hc, Wc, 3] -> this executor's image size with the rows of set_crop_rows:
    edet_crop_resize, the first launch of a step.  to_u8: into a static uint8 buffer (clipped and truncated,
    preprocessing.py:49-50) that randaug_batch reads next; else into the static network-input buffer in the engine's dtype,
    normalised (v - 128) / 128.  method='bicubic': edet_crop_resize_bicubic, whose float output is (v - mean) / std for
    norm = (mean [3], std [3]) (the legacy pipeline, preprocess_legacy.py)."""
    from automl_amd import v2_preprocessing
    assert self.crop_rows is not None, 'crop_batch needs set_crop_rows first'
    b, (h, w) = self.batch, self.image_size
    assert raw_u8.dtype == torch.uint8 and raw_u8.is_contiguous() and raw_u8.dim() == 4 and raw_u8.shape[0] == b and \
        raw_u8.shape[3] == 3, (raw_u8.dtype, tuple(raw_u8.shape))
    out = self.buf('crop:u8', (b, h, w, 3), torch.uint8) if to_u8 else self.buf('crop:images', (b, h, w, 3), self.tdtype)
    return v2_preprocessing.launch(raw_u8, self.crop_rows, out, self.stream, method, norm)

  def l2_loss_eval(self, weight_decay):
    """The same L2 term for an evaluation pass (test_step, main_tf2.py:105-117), added to cls_sums[3] WITHOUT touching the
    gradient arena, the clip factors or the gradient norm (optimizer_local adds weight_decay * w to the gradients): per-segment
    sums of squares by torch.segment_reduce, weighted by the arena's L2 flags.  Not on the training path."""
    a = self.arena
    if getattr(a, '_l2_weights', None) is None:
      a._seg_lengths = (a.seg_offsets[1:] - a.seg_offsets[:-1]).contiguous()
      a._l2_weights = (a.seg_flags == _lib.SEG_L2).to(torch.float32)
    sq = torch.segment_reduce(self.params_flat * self.params_flat, 'sum', lengths=a._seg_lengths, unsafe=True)
    self.cls_sums[3:4].add_((0.5 * float(weight_decay)) * (sq * a._l2_weights).sum().reshape(1))

  def _fused_mbconv(self, xin, b, scope):
    """FusedMBConvBlock.call (effnetv2_model.py:373-406)."""
    cexp = b.input_filters * b.expand_ratio
    x = xin
    if b.expand_ratio != 1:
      x = self.conv(scope + ':exp', x, scope + '/conv2d/kernel', b.kernel_size, b.stride, cexp,
                    bn=scope + '/tpu_batch_normalization', act=ACT_SWISH)
      if b.se_filters:
        x = self.se(scope + ':se', x, scope, b.se_filters)
      y = self.pw(scope + ':proj', x, scope + '/conv2d_1/kernel', b.output_filters,
                  bn=scope + '/tpu_batch_normalization_1', act=ACT_NONE)
    else:
      if b.se_filters:
        raise ValueError('SE in an expand_ratio == 1 fused block gates the block input: out of scope')
      y = self.conv(scope + ':conv', x, scope + '/conv2d/kernel', b.kernel_size, b.stride, b.output_filters,
                    bn=scope + '/tpu_batch_normalization', act=ACT_SWISH)     # act because no expansion
    return self.bn_res(scope + ':out', y, xin if b.has_residual else None,
                       survival_prob=self.spec.survival_probs[b.index])


class EffNetV2Model(object):
  """EfficientNetV2 / EfficientNet (V2 code base) forward model, same call surface as the reference."""
  update = layer_engine.Update('sgd', 0.0)      # this model applies no update; effnetv2_train.TrainableModel names its own

  def __init__(self, model_name='efficientnetv2-s', model_config=None, include_top=True, name=None,
               dtype='bf16', device='cuda:0', seed=0, params=None):
    self.name = name or model_name
    self.cfg_model = effnetv2_configs.model_config(model_name, model_config)
    self._mconfig = self.cfg_model
    self.include_top = include_top
    self.spec = V2Spec(self.cfg_model, include_top)
    self._dtype, self._device, self._seed, self._init_params = dtype, device, seed, params
    self.engine = None
    self.endpoints = None

  def count_params(self):
    return self.spec.count_params()

  def _ensure_engine(self, batch, height, width):
    e = self.engine
    if e is None or e.batch != batch or e.image_size != (height, width):
      # a new shape gets new buffers; the variables stay in the arena the previous executor used
      self.engine = V2Engine(self.spec, batch, (height, width), self.update, dtype=self._dtype, device=self._device,
                             seed=self._seed, params=self._init_params, arena=None if e is None else e.arena)
    return self.engine

  def backward(self, d_outputs):
    """Gradients of every variable w.r.t. a given d(outputs) of the last training=True call -> {name: array}."""
    self.engine.backward(d_outputs)
    return self.engine.get_grads()

  def __call__(self, inputs, training=False, with_endpoints=False):
    """-> logits [B,num_classes] (include_top) or pooled features [B,feature_size]; with_endpoints:
    [outputs, reduction_1..5] (effnetv2_model.py:595-658).  Tensors are device torch tensors."""
    if training and (self._mconfig.dropout_rate or self._mconfig.conv_dropout):
      raise ValueError('training=True with dropout is outside the built path; '
                       "override model_config='dropout_rate=0'")
    if isinstance(inputs, np.ndarray):
      inputs = torch.from_numpy(inputs)
    if inputs.dim() != 4 or inputs.shape[-1] != 3:
      raise ValueError('inputs must be [batch, height, width, 3], got %s' % (tuple(inputs.shape),))
    b, h, w = int(inputs.shape[0]), int(inputs.shape[1]), int(inputs.shape[2])
    eng = self._ensure_engine(b, h, w)
    eng.forward(inputs.to(device=eng.device, dtype=eng.tdtype).contiguous(), training=training)
    self.endpoints = {k: self._materialise(eng, v) for k, v in eng.endpoints.items()
                      if k.startswith('reduction_') or k == 'features'}
    pooled = (eng.pooled_sum * eng.pooled_inv_hw)
    self.endpoints['pooled_features'] = pooled
    if eng.logits is not None:
      outputs = eng.logits.data.reshape(b, -1)[:, :self.spec.num_classes].float()
    else:
      outputs = pooled
    self.endpoints['head'] = outputs
    if with_endpoints:
      return [outputs] + [self.endpoints['reduction_%d' % i] for i in range(1, 6)
                          if 'reduction_%d' % i in self.endpoints]
    return outputs

  call = __call__

  @staticmethod
  def _materialise(eng, view):
    """Block outputs are stored plain (edet_bn_res): a strided torch view of the buffer."""
    assert view.bn is None and view.gate is None and view.act == ACT_NONE
    return view.raw.data[..., :view.raw.c]

  def set_weights(self, values):
    if self.engine is None:
      self._init_params = dict(values) if self._init_params is None else {**self._init_params, **values}
    else:
      self.engine.set_params(values)

  def get_weights(self):
    if self.engine is None:
      raise RuntimeError('the network has not been built yet (call it once)')
    return self.engine.get_params()


def get_model(model_name, model_config=None, include_top=True, weights=None, **kwargs):
  """effnetv2_model.get_model (:661-760).  ``weights``: None (random initialisation) or the path of a checkpoint /
  checkpoint directory, as the reference's last branch (``tf.train.latest_checkpoint`` + ``load_weights``); the named
  pretrained sets ('imagenet', 'imagenet21k', ...) are downloads and cannot be fetched offline."""
  model = EffNetV2Model(model_name, model_config, include_top, **kwargs)
  if weights:
    import os
    if weights in ('imagenet', 'imagenet21k', 'imagenet21k-ft1k', 'jft') or not (
        os.path.isdir(weights) or os.path.exists(weights + '.index')):
      raise ValueError('pretrained weights %r cannot be fetched here; pass a checkpoint path or set_weights()' % (weights,))
    from automl_amd import util_keras
    util_keras.restore_ckpt(model, weights, ema_decay=0, skip_mismatch=False)
  return model
