"""Training step of the detection path on MI355X (mirror of efficientdet/tf2/train_lib.py).

``EfficientDetNetTrain.train_step((images, labels))`` follows train_lib.py:606-684: forward with
training BatchNorm, focal + Huber detection loss (:493-604), L2 on kernels (:486-491), per-tensor
clip_by_norm then clip_by_global_norm (:675-682, on the LOCAL gradient), gradient all-reduce SUM
across data-parallel replicas (implicit in optimizer.apply_gradients, :683), SGD momentum and the
TFA MovingAverage EMA (:176-199).  LR schedules restate :37-173.

``EfficientDetNetTrain.fit`` / ``.evaluate`` are the loop of ``tf.keras.Model.fit`` as tf2/train.py:283-290 calls it, over
``train_step_raw`` / ``test_step_raw`` without a wait for the device per step; ``ModelCheckpoint`` and ``get_callbacks``
mirror :293-325; ``save_train_state`` / ``restore_train_state`` write and read, next to a checkpoint, everything else a
next step reads, so that an interrupted run continues bit for bit.  The entry point is automl_amd/train.py.
"""
import collections.abc
import json
import math
import os

import numpy as np
import torch

from automl_amd import _lib
from automl_amd import det_autoaugment
from automl_amd import det_input
from automl_amd import efficientdet_net
from automl_amd import engine as engine_lib
from automl_amd import iou_utils
from automl_amd import layer_engine
from automl_amd import utils


def update_learning_rate_schedule_parameters(params):
  """train_lib.py:37-49 (params: dict-like with batch_size and steps_per_epoch)."""
  params['adjusted_learning_rate'] = params['learning_rate'] * params['batch_size'] / 64
  spe = params['steps_per_epoch']
  params['lr_warmup_step'] = int(params['lr_warmup_epoch'] * spe)
  params['first_lr_drop_step'] = int(params['first_lr_drop_epoch'] * spe)
  params['second_lr_drop_step'] = int(params['second_lr_drop_epoch'] * spe)
  params['total_steps'] = int(params['num_epochs'] * spe)


def _warmup(step, lr_warmup_init, lr_warmup_step, adjusted_lr):
  return lr_warmup_init + (float(step) / lr_warmup_step * (adjusted_lr - lr_warmup_init))


class StepwiseLrSchedule(object):
  def __init__(self, adjusted_lr, lr_warmup_init, lr_warmup_step, first_lr_drop_step, second_lr_drop_step):
    self.adjusted_lr, self.lr_warmup_init, self.lr_warmup_step = adjusted_lr, lr_warmup_init, lr_warmup_step
    self.first_lr_drop_step, self.second_lr_drop_step = first_lr_drop_step, second_lr_drop_step

  def __call__(self, step):
    lr = _warmup(step, self.lr_warmup_init, self.lr_warmup_step, self.adjusted_lr) \
        if step < self.lr_warmup_step else self.adjusted_lr
    for mult, start in ((1.0, self.lr_warmup_step), (0.1, self.first_lr_drop_step),
                        (0.01, self.second_lr_drop_step)):
      if step >= start:
        lr = self.adjusted_lr * mult
    return lr


class CosineLrSchedule(object):
  def __init__(self, adjusted_lr, lr_warmup_init, lr_warmup_step, total_steps):
    self.adjusted_lr, self.lr_warmup_init, self.lr_warmup_step = adjusted_lr, lr_warmup_init, lr_warmup_step
    self.decay_steps = float(total_steps - lr_warmup_step)

  def __call__(self, step):
    if step < self.lr_warmup_step:
      return _warmup(step, self.lr_warmup_init, self.lr_warmup_step, self.adjusted_lr)
    return 0.5 * self.adjusted_lr * (1 + math.cos(math.pi * float(step) / self.decay_steps))


class PolynomialLrSchedule(object):
  def __init__(self, adjusted_lr, lr_warmup_init, lr_warmup_step, power, total_steps):
    self.adjusted_lr, self.lr_warmup_init, self.lr_warmup_step = adjusted_lr, lr_warmup_init, lr_warmup_step
    self.power, self.total_steps = power, total_steps

  def __call__(self, step):
    if step < self.lr_warmup_step:
      return _warmup(step, self.lr_warmup_init, self.lr_warmup_step, self.adjusted_lr)
    return self.adjusted_lr * (1 - float(step) / self.total_steps)**self.power


def learning_rate_schedule(params):
  update_learning_rate_schedule_parameters(params)
  m = params['lr_decay_method']
  if m == 'stepwise':
    return StepwiseLrSchedule(params['adjusted_learning_rate'], params['lr_warmup_init'],
                              params['lr_warmup_step'], params['first_lr_drop_step'],
                              params['second_lr_drop_step'])
  if m == 'cosine':
    return CosineLrSchedule(params['adjusted_learning_rate'], params['lr_warmup_init'],
                            params['lr_warmup_step'], params['total_steps'])
  if m == 'polynomial':
    return PolynomialLrSchedule(params['adjusted_learning_rate'], params['lr_warmup_init'],
                                params['lr_warmup_step'], params['poly_lr_power'], params['total_steps'])
  raise ValueError('unknown lr_decay_method: {}'.format(m))


def split_global_batch(global_batch_size, world_size, rank):
  """Per-replica slice [begin, end) of the global batch; the reference requires divisibility
  (tf2/train.py:186-189: 'batch size must be divisible by number of replicas')."""
  if global_batch_size % world_size != 0:
    raise ValueError('batch size {} must be divisible by the number of replicas {}'.format(
        global_batch_size, world_size))
  per = global_batch_size // world_size
  return rank * per, (rank + 1) * per


def make_grad_all_reduce(process_group=None):
  """SUM all-reduce of the flat gradient arena (one RCCL call per step; 15.5 MB fp32 for D0).

  The reference clips the LOCAL gradient (per tensor, then global norm) before apply_gradients
  reduces it (train_lib.py:675-683), and the global-norm clip needs every local gradient, so the
  reduce cannot start before the backward pass has finished; see DESIGN.md section multi-GPU.
  """
  import torch.distributed as dist

  def reduce_fn(flat):
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=process_group)
    return flat
  return reduce_fn


def ema_decay_dynamic(average_decay, num_updates):
  """TFA MovingAverage(dynamic_decay=True): min(decay, (1 + n) / (10 + n))."""
  return min(average_decay, (1.0 + num_updates) / (10.0 + num_updates))


def moving_normalizer_update(state, value, momentum):
  """The loss normalizer as a moving average (train_lib.py:519-531, config.positives_momentum > 0): Keras'
  moving_average_update on a variable that starts at 0.0 -- state <- state * momentum + value * (1 - momentum), with no
  zero-debiasing, so the first steps divide the loss by a small number exactly as the reference does.  `state` is a python
  float (returned) or a 0-d torch tensor (updated in place and returned: the device path, no host synchronisation)."""
  if torch.is_tensor(state):
    return state.mul_(momentum).add_(value, alpha=1.0 - momentum)
  return state * momentum + float(value) * (1.0 - momentum)


class EfficientDetNetTrain(efficientdet_net.EfficientDetNet):
  """EfficientDetNet plus the reference train_step.

  Data parallel: one process per GPU; pass ``process_group`` (torch.distributed, backend 'nccl'
  == RCCL over xGMI) and every replica's locally-clipped gradient is SUM all-reduced before the
  update, exactly the reference's MirroredStrategy semantics.
  """

  def __init__(self, *args, steps_per_epoch=1000, global_batch_size=None, process_group=None,
               use_dist=False, use_graph=False, sync_bn=False, overlap_grad_reduce=None, lion=None, iou_loss=None,
               **kwargs):
    """use_graph: capture the whole step (forward, loss, backward, L2/clip, update: ~1600 kernel launches)
    into a hipGraph at the second call for a given batch shape and replay it afterwards; inputs are
    copied into static device buffers (input_buffers() exposes them for in-place filling), learning
    rate / EMA decay / loss normalizer travel through a small device vector.  With data parallelism the
    gradient all-reduce stays an eager RCCL call between two captured halves.
    lion: with config.optimizer = 'lion', dict(beta_2=0.99, wd=0.0) -- lion_tf2.Lion's two arguments that are no
    configuration keys (see set_lion).
    iou_loss: dict(type='ciou', weight=None) -- BoxIouLoss added to the detection loss (see set_iou_loss)."""
    super().__init__(*args, **kwargs)
    self._check_training_options(self.config)
    if lion is not None:
      self.set_lion(**lion)
    if iou_loss is not None:
      self.set_iou_loss(**iou_loss)
    # sync_bn: cross-replica BatchNorm statistics (the reference's --strategy=gpus / tpu BatchNorm classes,
    # utils.py:166-266): two small all-reduces per BatchNorm layer and step, eager launches only.
    self.sync_bn = sync_bn
    self.use_graph = use_graph and not sync_bn
    self._graph = None
    self.steps_per_epoch = steps_per_epoch
    self.global_batch_size = global_batch_size
    self.process_group = process_group
    self.use_dist = use_dist or process_group is not None
    self.one_graph_dp = os.environ.get('EDET_DP_ONE_GRAPH', '0') == '1'      # see _graph_step
    # The gradient all-reduce in buckets UNDER the backward pass (Engine.set_overlap_reduce) -- what north_star asks for.
    # Legal only with clip_gradients_norm = 0: the reference clips the local gradient by its global norm before the reduce
    # (train_lib.py:675-683), so with the default clip_gradients_norm = 10 the one flat reduce after the backward pass stays.
    if overlap_grad_reduce is None:
      overlap_grad_reduce = os.environ.get('EDET_DP_OVERLAP', '0') == '1'
    self.overlap_grad_reduce = bool(overlap_grad_reduce)
    if self.overlap_grad_reduce and self.config.clip_gradients_norm:
      raise ValueError('overlap_grad_reduce needs clip_gradients_norm=0 (the reference clips by the global norm of the '
                       'local gradient before the reduce, train_lib.py:675-683); got %r' % (self.config.clip_gradients_norm,))
    self.overlap_buckets = int(os.environ.get('EDET_DP_BUCKETS', '6'))
    self._lr_fn = None
    self.iterations = 0
    # positives_momentum > 0: the moving loss normalizer (train_lib.py:519-531).  A 0-d fp32 DEVICE tensor once the
    # engine exists (updated in place by both the graph and the eager step, no host synchronisation); a python float
    # only before that (a state restored into a net that has not stepped yet) or when the caller supplies the
    # normalizer of a step as a host float (labels['normalizer'])
    self._moving_normalizer = None
    # a list: every graph-mode data-parallel step appends (start, end) events recorded on the step's stream around the
    # gradient all-reduce (between the two captured graphs) -- its duration as the device sees it; None = off
    self.collective_timer = None
    # train_step_raw's input stage (det_input.DetectionInput) and the host generator behind its draws: both created by the
    # first train_step_raw, so a model that never calls it keeps its state keys
    self._det_input = None
    self._input_rng = None
    # test_step / test_step_raw: the evaluation input stage of the last raw shape and the captured evaluation pass per engine
    self._det_eval_input = None
    self._eval_graphs = {}
    self.autoaugment = None      # set_autoaugment: the box-aware AutoAugment / RandAugment in front of train_step_raw's crop
    # restore_train_state into a model without an engine: applied by _ensure_engine
    self._pending_state = None
    self._pending_drop_rng = {}
    # fit / evaluate: float32 [5] device sums of Engine.LOSS_KEYS over the steps, and the vector a step's values are formed in
    self._loss_acc = {}
    self.fit_input = None        # the iterator fit is reading from (ModelCheckpoint saves its state)
    self.stop_training = False

  def set_autoaugment(self, policy):
    """Switches the box-aware AutoAugment / RandAugment of aug/autoaugment.py (dataloader.py:312-319) on for train_step_raw:
    'randaug' (num_layers=1, magnitude=15), 'v2', 'v3' or 'test'; None switches it off.  'v0' and 'v1' need the
    *_Only_BBoxes operations, which are not built, and raise.  Needs no device; the input stage is rebuilt by the next
    train_step_raw.  The draws come from the generator behind 'input_rng_state', after the step's other draws."""
    if policy is not None:
      det_autoaugment.available_policy(policy)
    self.autoaugment = policy
    self._det_input = None

  def set_lion(self, beta_2=None, wd=None):
    """Lion's beta_2 and decoupled weight decay wd (lion/lion_tf2.py:23-28: 0.99 and 0; beta_1 is config.momentum, as for
    Adam); None keeps a value.  wd reaches every variable the optimizer is given, BatchNorm scales and biases included, as the
    reference's does.  The scalars are arguments of the update launch an engine records, so once an engine exists they are
    fixed: build a new model for other values."""
    if str(getattr(self.config, 'optimizer', 'sgd')).lower() != 'lion':
      raise ValueError('set_lion needs config.optimizer = lion, this model has %r' % (self.config.optimizer,))
    if self.engine is not None:
      raise ValueError('set_lion after the first engine was made: beta_2 and wd are arguments of the update it launches '
                       '(and of a step it has captured); set them before the first step, or build a new model')
    current = self._lion or {}
    beta_2, wd = layer_engine.lion_options({'beta_2': beta_2, 'wd': wd}, current.get('beta_2', layer_engine.LION_BETA2),
                                           current.get('wd', layer_engine.LION_WD))
    self._lion = {'beta_2': beta_2, 'wd': wd}

  def set_iou_loss(self, type, weight=None):      # pylint: disable=redefined-builtin
    """Switches BoxIouLoss (tf2/train_lib.py:440-464, :580-600) on: type 'iou', 'giou', 'diou' or 'ciou' (iou_utils.py), added to
    det_loss with `weight` (None: config.iou_loss_weight, 1.0) and reported as 'box_iou_loss'; type=None switches it off.
    The configuration key iou_loss_type keeps raising: this is its switch.  Every row of the box outputs is decoded with its own
    anchor; the gradient is the reference's as TensorFlow executes it (CIoU's v is a constant of the backward pass).  The
    type and the weight are arguments of launches an engine makes (and of a step it has captured), so once an engine exists
    they are fixed: build a new model for other values."""
    if self.engine is not None:
      raise ValueError('set_iou_loss after the first engine was made: the type and the weight are arguments of the loss kernels '
                       'it launches (and of a step it has captured); set them before the first step, or build a new model')
    if type is None:
      self._iou_loss = None
      return
    iou_utils.iou_type_id(type)      # an unknown type raises the reference's message
    if weight is None:
      weight = getattr(self.config, 'iou_loss_weight', 1.0)
    weight = float(weight)
    if not np.isfinite(weight):
      raise ValueError('set_iou_loss: weight %r is not finite' % (weight,))
    self._iou_loss = (str(type), weight)

  def _loss_keys(self):
    """Engine.LOSS_KEYS, and 'box_iou_loss' behind them with the IoU loss on (Engine.loss_keys, without an engine)."""
    return engine_lib.Engine.LOSS_KEYS + (('box_iou_loss',) if self._iou_loss is not None else ())

  @property
  def update(self):
    """The update description of this model's engines (layer_engine.Update), from the configuration alone: no device."""
    c = self.config
    kind, momentum = str(getattr(c, 'optimizer', 'sgd')).lower(), float(c.momentum)
    if kind == 'lion':
      beta_2, wd = layer_engine.lion_options(self._lion)
      return layer_engine.Update('lion', momentum, beta_2, wd=wd)
    if kind == 'adam':
      return layer_engine.Update('adam', momentum, layer_engine.LayerEngine.ADAM_BETA2, layer_engine.LayerEngine.ADAM_EPSILON)
    return layer_engine.Update('sgd', momentum)

  def get_optimizer_state(self):
    """Optimizer slots, iteration count and -- with positives_momentum > 0 -- the moving loss normalizer.  (The reference
    creates that variable inside the loss call, train_lib.py:521-527, untracked by its checkpoints: a resumed reference
    run restarts the average at 0 and divides the first losses by ~(1 - m) * N.  Carrying it in the state avoids that
    spike; a state without the key restores to the reference's behaviour.)"""
    state = super().get_optimizer_state()
    if self._moving_normalizer is not None:
      state['moving_normalizer'] = float(self._moving_normalizer)
    if self._input_rng is not None:      # only once train_step_raw has been used (or such a state restored)
      state['input_rng_state'] = utils.pack_rng_state(self._input_rng)
    return state

  def set_optimizer_state(self, state):
    """Optimizer slots + iteration count; the count also drives the learning-rate schedule and the dynamic EMA decay
    of the next train_step (optimizer.iterations in the reference, train_lib.py:37-173,193-197)."""
    super().set_optimizer_state(state)
    self.iterations = int(state['iterations'])
    if 'moving_normalizer' in state:
      value = float(state['moving_normalizer'])
      if torch.is_tensor(self._moving_normalizer):
        self._moving_normalizer.fill_(value)
      else:
        self._moving_normalizer = value
    elif torch.is_tensor(self._moving_normalizer):
      self._moving_normalizer.zero_()     # a state without the key: the reference's behaviour, the average restarts at 0
    else:
      self._moving_normalizer = None
    if 'input_rng_state' in state:
      if self._input_rng is None:
        self._input_rng = det_input.input_rng(self._seed)
      utils.unpack_rng_state(self._input_rng, state['input_rng_state'])

  @staticmethod
  def _check_training_options(c):
    """The train step here is the reference's default one (train_lib.py:606-684 with the d0..d7x settings); options
    that would change its arithmetic and are not built raise instead of being ignored.  BoxIouLoss itself is built, behind the
    constructor's iou_loss= and set_iou_loss: the configuration key iou_loss_type is not its switch and keeps raising."""
    unsupported = []
    if getattr(c, 'iou_loss_type', None):
      unsupported.append('iou_loss_type=%r as a configuration key (BoxIouLoss, train_lib.py:440-466, is switched on with '
                         'EfficientDetNetTrain(..., iou_loss=dict(type=%r)) or set_iou_loss; train.py: --iou_loss_type)'
                         % (c.iou_loss_type, c.iou_loss_type))
    if str(getattr(c, 'optimizer', 'sgd')).lower() not in ('sgd', 'adam', 'lion'):
      unsupported.append("optimizer=%r (the reference has 'sgd' and 'adam', train_lib.py:180-188; 'lion' is lion/lion_tf2.py's)"
                         % c.optimizer)
    if unsupported:
      raise ValueError('training options that are not built: ' + '; '.join(unsupported))

  def _lr(self, batch):
    if self._lr_fn is None:
      p = self.config.as_dict()
      gbs = self.global_batch_size
      if gbs is None:
        # the reference scales by the GLOBAL batch (train_lib.py:41); per replica batch x number of replicas
        gbs = batch
        if self.use_dist:
          import torch.distributed as dist
          gbs = batch * dist.get_world_size(self.process_group)
      p['batch_size'] = gbs
      p['steps_per_epoch'] = self.steps_per_epoch
      self._lr_fn = learning_rate_schedule(p)
    return self._lr_fn(self.iterations)

  def _labels_to_device(self, labels, eng):
    out = {}
    for k, v in labels.items():
      if k == 'normalizer':
        out[k] = float(v)
        continue
      t = torch.as_tensor(v)
      if k.startswith('cls_targets'):
        t = t.to(device=eng.device, dtype=torch.int32)
      else:
        t = t.to(device=eng.device, dtype=torch.float32)
      out[k] = t.contiguous()
    return out

  # ---- hipGraph replay of the step ---------------------------------------------------------------
  def input_buffers(self):
    """(images, labels) static device buffers of the captured step (None before the first graph step):
    fill them in place and pass them to train_step to skip the staging copy."""
    g = self._graph
    return (g['images'], g['labels']) if g else None

  @staticmethod
  def _new_graph_state(eng, images, labels):
    return {'engine': eng, 'steps': 0, 'graphs': None, 'images': images, 'labels': labels}

  @staticmethod
  def _static_like(images, labels):
    """Static buffers for device (images, labels): a host 'normalizer' has none."""
    return torch.empty_like(images), {k: torch.empty_like(v) for k, v in labels.items() if torch.is_tensor(v)}

  @staticmethod
  def _stage(g, images, labels):
    """Device (images, labels) into the static buffers of the graph state `g` -- a tensor that already IS its buffer is not
    copied, one the buffers have no place for is left out -- -> (images, labels) of static tensors; a host 'normalizer'
    passes through."""
    if images.data_ptr() != g['images'].data_ptr():
      g['images'].copy_(images, non_blocking=True)
    static = dict(g['labels'])
    for k, v in labels.items():
      if not torch.is_tensor(v):
        static[k] = v
      elif k in static and v.data_ptr() != static[k].data_ptr():
        static[k].copy_(v, non_blocking=True)
    return g['images'], static

  def _graph_step(self, eng, images, labels, lr, decay):
    g = self._graph
    if g is None or g['engine'] is not eng:
      g = self._graph = self._new_graph_state(eng, *self._static_like(images, labels))
    _, labels = self._stage(g, images, labels)
    eng.set_hyper(lr, decay)
    self._inv_normalizer(eng, labels, eng.hyper[2:3], store=True)
    glabels = dict(g['labels'])
    glabels['normalizer'] = 'device'
    reduce_fn = make_grad_all_reduce(self.process_group) if self.use_dist else None
    overlap = self.overlap_grad_reduce and reduce_fn is not None
    eng.set_overlap_reduce(reduce_fn if overlap else None, self.overlap_buckets)

    def body_a():
      eng.forward(g['images'], training=True)
      eng.loss_backward(glabels)           # (overlap: the bucketed all-reduce runs inside, on the communication stream)
      if overlap:
        eng.optimizer_apply(decay is not None, True)
        return
      eng.optimizer_local(reduce_fn is not None)
      if reduce_fn is None:
        eng.optimizer_apply(decay is not None, False)

    def body_b():
      eng.optimizer_apply(decay is not None, True)

    if g['steps'] == 0:
      # first step eager: allocates every buffer and runs the one-time kernel attribute setup
      body_a()
      if reduce_fn is not None and not overlap:
        reduce_fn(eng.grads_flat)
        body_b()
    else:
      if g['graphs'] is None:
        torch.cuda.synchronize()
        ga = gb = None
        if overlap:
          # forward, backward with the bucketed collectives on their own stream (a parallel branch of the graph), update
          ga = engine_lib.capture_graph(eng.arena, body_a)
          g['overlap'] = True
        elif reduce_fn is not None and self.one_graph_dp:
          # The collective captured INSIDE the step's graph (RCCL 2.26 supports stream capture): no host hop between the
          # two halves.  Opt-in (EDET_DP_ONE_GRAPH=1): exercised on the device at world size 1 only -- no multi-GPU node
          # was available to any round -- so the default stays the two-graph structure below; if the capture itself
          # raises, the step falls back to it.
          def one_graph():
            body_a()
            reduce_fn(eng.grads_flat)
            body_b()
          try:
            ga = engine_lib.capture_graph(eng.arena, one_graph)
          except Exception as e:      # noqa: BLE001 -- any capture failure: the robust structure
            import warnings
            warnings.warn('one-graph data-parallel capture failed (%s); using two graphs around an eager all-reduce' % (e,))
            ga = None
            torch.cuda.synchronize()
        if ga is None:
          ga = engine_lib.capture_graph(eng.arena, body_a)
          if reduce_fn is not None and not overlap:
            gb = engine_lib.capture_graph(eng.arena, body_b, pool=ga.pool())
          g['one_graph'] = False
        else:
          g['one_graph'] = True
        g['graphs'] = (ga, gb)
      ga, gb = g['graphs']
      eng.refresh_drop_masks()      # stochastic-depth draws live in static buffers the graph reads
      ga.replay()
      if gb is not None:
        timer = self.collective_timer
        if timer is not None:           # bench.py / the world-size-1 rehearsal: the collective's own duration
          e0 = torch.cuda.Event(enable_timing=True)
          e0.record()
        reduce_fn(eng.grads_flat)
        if timer is not None:
          e1 = torch.cuda.Event(enable_timing=True)
          e1.record()
          timer.append((e0, e1))
        gb.replay()
      eng.arena.count_step()        # what optimizer_apply does on the host when it is not replayed
    g['steps'] += 1

  def _ensure_engine(self, batch, height, width):
    known = (batch, height, width) in self._engines
    eng = super()._ensure_engine(batch, height, width)
    expr = getattr(self.config, 'var_freeze_expr', None) or None
    if eng.arena.frozen_expr != expr:
      eng.arena.set_frozen(expr)         # tf2/train_lib.py:478-491: out of L2, gradients and updates (None: un-freeze)
    # what restore_train_state left for a model that had no engine yet: the optimizer state goes into the arena the first
    # engine brings, a stochastic-depth generator state into the engine of its shape when that one is made
    if self._pending_state is not None:
      state, self._pending_state = self._pending_state, None
      check_arena_length(state, eng.arena)
      self.set_optimizer_state(state)
    if not known:
      rng_state = self._pending_drop_rng.pop(_shape_key(batch, height, width), None)
      if rng_state is not None:
        eng.set_drop_rng_state(rng_state)
    return eng

  def _positives_momentum(self):
    return float(getattr(self.config, 'positives_momentum', None) or 0.0)

  def _normalizer(self, value, dest, store, eng=None):
    """The loss normalizer sum(mean_num_positives) + 1 as the reference uses it (train_lib.py:517-534): the moving average
    over the steps for positives_momentum > 0, the mean over the replicas for positives_momentum < 0 (a collective, no
    state), the value itself otherwise.

    value: the sum + 1 of this step as a host float supplied by the caller, or the device tensor mean_num_positives (then
    `eng` launches edet_loss_normalizer where no average is asked for, and nothing waits for the host: no .item()).
    dest: a one-element device tensor that receives 1 / normalizer (eng.hyper[2:3], eng.eval_inv_norm), or None: the
    normalizer comes back as a host float (host values only).
    store: True, the training step: the moving average v <- v * m + x * (1 - m) is stored.  False, the evaluation step: it
    is READ, v * m + x * (1 - m), and v stays.

    The stored average is a python float only until a device value arrives; from then on the 0-d device tensor is its one
    representation, updated in place.  A state without the key restarts at 0."""
    m = self._positives_momentum()
    v = self._moving_normalizer
    if not torch.is_tensor(value):
      norm = value
      if m > 0 and store and torch.is_tensor(v):
        norm = float(moving_normalizer_update(v, float(value), m))
      elif m > 0:
        norm = moving_normalizer_update(float(v or 0.0), value, m)
        if store:
          self._moving_normalizer = norm
      elif m < 0 and self.use_dist:
        import torch.distributed as dist
        t = torch.tensor([value], dtype=torch.float32)
        if dist.get_backend(self.process_group) == 'nccl':
          t = t.cuda()
        dist.all_reduce(t, group=self.process_group)
        norm = float(t.item()) / dist.get_world_size(self.process_group)
      if dest is None:
        return norm
      dest.copy_(torch.tensor([1.0 / norm], dtype=torch.float32), non_blocking=True)
      return None
    mnp = value.reshape(-1)
    if mnp.dtype != torch.float32 or not mnp.is_contiguous():
      mnp = mnp.float().contiguous()
    if m == 0 or (m < 0 and not self.use_dist):
      _lib.call('edet_loss_normalizer', _lib.ptr(mnp), mnp.numel(), _lib.ptr(dest), eng.stream)
      return None
    s = mnp.sum() + 1.0
    if m > 0:
      if not torch.is_tensor(v):
        v = torch.full((), float(v or 0.0), dtype=torch.float32, device=s.device)
      if store:
        self._moving_normalizer = v
      s = moving_normalizer_update(v if store else v.clone(), s, m)
    else:
      import torch.distributed as dist
      s = s.clone()
      dist.all_reduce(s, group=self.process_group)
      s = s / dist.get_world_size(self.process_group)
    torch.reciprocal(s, out=dest[0])
    return None

  def _host_normalizer(self, value):
    return self._normalizer(value, None, store=True)

  def _device_normalizer(self, eng, mean_num_positives):
    return self._normalizer(mean_num_positives, eng.hyper[2:3], store=True, eng=eng)

  def _inv_normalizer(self, eng, labels, dest, store):
    """1 / normalizer of a step whose launches read it from the device, into `dest`: runs eagerly in front of the replayed
    graph."""
    if 'normalizer' in labels:                         # host value supplied by the caller
      self._normalizer(float(labels['normalizer']), dest, store)
    elif 'mean_num_positives' in labels:
      self._normalizer(labels['mean_num_positives'], dest, store, eng)
    else:
      raise KeyError("labels need 'mean_num_positives' (dataloader.py:393) or a host 'normalizer'")

  def _raw_input(self, raw, boxes, training):
    """What train_step_raw and test_step_raw open with: the raw batch checked on the host -> (engine, the input stage of this
    shape: det_input.DetectionInput / DetectionEvalInput, built when the shape, the dtype or the AutoAugment switch moved,
    raw images, sizes checked or None).  raw: the images, or the pair (images, sizes) of a canvas batch -- the stage is then
    keyed on the canvas and serves every batch on it."""
    raw, sizes = det_input.split_raw(raw)
    raw = torch.as_tensor(raw)
    if raw.dtype != torch.uint8 or raw.dim() != 4 or raw.shape[-1] != 3:
      raise ValueError('raw images must be uint8 [batch, height, width, 3], got %s %s' % (raw.dtype, tuple(raw.shape)))
    boxes = torch.as_tensor(boxes)
    if boxes.dim() != 3 or boxes.shape[0] != raw.shape[0] or boxes.shape[-1] != 4:
      raise ValueError('boxes must be [batch, max_boxes, 4], got %s' % (tuple(boxes.shape),))
    c = self.config
    b, rh, rw, m = int(raw.shape[0]), int(raw.shape[1]), int(raw.shape[2]), int(boxes.shape[1])
    h, w = utils.parse_image_size(c.image_size)
    if not training:
      det_input.check_max_instances(c, m)      # raises, before any device work
    eng = self._ensure_engine(b, h, w)
    attr = '_det_input' if training else '_det_eval_input'
    key = (b, rh, rw, m, h, w, eng.tdtype, self.autoaugment if training else None)
    cached = getattr(self, attr)
    if cached is None or cached[0] != key:
      extra = {'autoaugment': self.autoaugment} if training else {}
      stage = det_input.DetectionInput if training else det_input.DetectionEvalInput
      cached = (key, stage(c, self.anchors((h, w)), b, rh, rw, m, dtype=eng.tdtype, device=eng.device, **extra))
      setattr(self, attr, cached)
    return eng, cached[1], raw, cached[1].check_sizes(sizes)

  def train_step_raw(self, data, sync_loss=True, draws=None):
    """One training step from a raw batch: data = (raw_images uint8 [B, H, W, 3], boxes float32 [B, M, 4] normalised (ymin,
    xmin, ymax, xmax), classes [B, M] 1-based, counts [B] valid rows per image).  The training branch of the reference's
    input pipeline (dataloader.py:301-338, :369-382; det_input.py) runs on the device at config.image_size -- GridMask if
    config.grid_mask, normalisation, random flip, random scale and crop, the boxes with it, anchor labelling,
    mean_num_positives -- as eager launches on the step's stream IN FRONT of the replayed graph, straight into
    input_buffers(), the way _device_normalizer runs in front of it; after that the step is train_step's.

    The draws (per image: flip, three scale draws, the five GridMask draws) come from a host generator seeded from the
    model's seed, whose state joins get_optimizer_state() as 'input_rng_state' once this method has been used; draws =
    det_input.Draws(flip [B], scale [B, 3], gridmask five arrays [B] or None) hands the values in instead.
    skip_crowd_during_training (dataloader.py:303-306) is the caller's filtering of boxes / counts.

    The box-aware AutoAugment / RandAugment of aug/autoaugment.py (dataloader.py:312-319) runs between GridMask and the crop
    once set_autoaugment(policy) has switched it on ('randaug', 'v2', 'v3', 'test'; 'v0', 'v1' and the *_Only_BBoxes
    operations are not built); its draws then follow the others in the same generator, or come as the fourth field of
    det_input.Draws (det_autoaugment.autoaug_draws).  The config key autoaugment_policy itself is still refused.

    A canvas batch: raw_images = (raw uint8 [B, Hc, Wc, 3], sizes int32 [B, 2]) as jpeg.JpegDecoder.decode returns it -- image
    i is the top-left sizes[i] = (height, width) of its slot and goes through every launch at its own size, as the reference
    processes it (dataloader.py:301-353; det_input.py "A canvas batch").  One stage serves every batch on the same canvas.
    Sizes are host data: a numpy array or a CPU tensor; a device tensor is copied to the host once, and that copy waits for
    the device.  They are checked before the generator moves; with sizes GridMask's gridblock draw is a stream of its own."""
    c = self.config
    if getattr(c, 'autoaugment_policy', None):
      raise ValueError('autoaugment_policy=%r is not built (the box-aware AutoAugment / RandAugment of aug/autoaugment.py, '
                       'dataloader.py:312-319); train_step_raw would have to ignore it -- the part that is built is switched '
                       'on with set_autoaugment(policy)' % (c.autoaugment_policy,))
    raw, boxes, classes, counts = data
    eng, inp, raw, sizes = self._raw_input(raw, boxes, training=True)
    if draws is None:
      if self._input_rng is None:
        self._input_rng = det_input.input_rng(self._seed)
      draws = inp.draw(self._input_rng, sizes)
    g = self._graph
    if self.use_graph and g is not None and g['engine'] is eng:
      images, labels = g['images'], g['labels']
    else:
      images, labels = inp.own_buffers()
      if self.use_graph:      # they become the captured step's static buffers
        self._graph = self._new_graph_state(eng, images, labels)
    inp.run(raw, boxes, classes, counts, draws, images, labels, sizes=sizes)
    return self.train_step((images, labels), sync_loss=sync_loss)

  def train_step(self, data, sync_loss=True):
    """data = (images [B, H, W, 3] already normalised and resized, labels {'cls_targets_<l>', 'box_targets_<l>',
    'mean_num_positives' or a host 'normalizer'}).  config.grid_mask cannot be honoured here -- GridMask works on the raw
    image in front of the normalisation (dataloader.py:308-310) and this path gets preprocessed images -- so it is the
    caller's pipeline's, or train_step_raw's."""
    images, labels = data
    b, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    eng = self._ensure_engine(b, h, w)
    if self.sync_bn and self.use_dist and eng.sync_bn is None:
      import torch.distributed as dist
      eng.sync_bn = (make_grad_all_reduce(self.process_group), dist.get_world_size(self.process_group))
    lr = self._lr(b)
    decay = None
    if self.config.moving_average_decay:
      decay = ema_decay_dynamic(self.config.moving_average_decay, self.iterations)
    if self.use_graph:
      self._graph_step(eng, self._to_device_images(images, eng), self._labels_to_device(labels, eng), lr, decay)
    else:
      reduce_fn = make_grad_all_reduce(self.process_group) if self.use_dist else None
      eng.set_overlap_reduce(reduce_fn if self.overlap_grad_reduce else None, self.overlap_buckets)
      eng.forward(self._to_device_images(images, eng), training=True)
      dlabels = self._labels_to_device(labels, eng)
      if self._positives_momentum() != 0:
        if 'normalizer' in dlabels:
          # the caller supplied this step's sum(mean_num_positives) + 1 as a host float: moving average / replica mean on the host
          dlabels['normalizer'] = self._host_normalizer(dlabels['normalizer'])
        else:
          # on the device, as the captured step does it (no .item(): the eager step does not wait for the host either)
          self._device_normalizer(eng, dlabels['mean_num_positives'])
          dlabels['normalizer'] = 'device'
      eng.loss_backward(dlabels)
      eng.optimizer_step(lr, decay, reduce_fn)
    self.iterations += 1
    if not sync_loss:
      return {'learning_rate': lr}
    vals = eng.loss_values()
    vals['learning_rate'] = lr
    return vals

  # ---- test_step: the losses of a batch, nothing moved (tf2/train_lib.py:686-732) ---------------------------------------
  def _eval_pass(self, eng, images, labels):
    """forward(training=False) and the loss-only kernels; with use_graph the first call per engine is eager, the second
    captures the pass -- separately from the train step's graph -- and later calls replay it.  images / labels: device
    tensors, with use_graph the static buffers of that capture."""
    # as the training step forms it, except that the moving average of positives_momentum > 0 is read and not stored
    self._inv_normalizer(eng, labels, eng.eval_inv_norm, store=False)
    glabels = {k: v for k, v in labels.items() if k != 'normalizer'}
    glabels['normalizer'] = 'device'

    def body():
      eng.forward(images, training=False)
      eng.loss_only(glabels)

    g = self._eval_graphs.get((eng.batch,) + tuple(eng.image_size)) if self.use_graph else None
    if g is None or g['steps'] == 0:
      body()
    else:
      if g['graph'] is None:
        torch.cuda.synchronize()
        eng._cast_version = -1      # the captured pass makes its own compute copies and BatchNorm vectors: variables move
        g['graph'] = engine_lib.capture_graph(eng.arena, body)
      g['graph'].replay()
    if g is not None:
      g['steps'] += 1
    # the next pass of this engine -- a training step, perhaps the one that is captured -- makes its compute copies again
    eng._cast_version = -1

  def _eval_graph_state(self, eng, make_buffers):
    """The captured evaluation pass of `eng` (by its shape; a state whose engine has been dropped is dropped with it)."""
    self._eval_graphs = {k: v for k, v in self._eval_graphs.items() if self._engines.get(k) is v['engine']}
    key = (eng.batch,) + tuple(eng.image_size)
    g = self._eval_graphs.get(key)
    if g is None:
      images, labels = make_buffers()
      g = self._eval_graphs[key] = {'engine': eng, 'steps': 0, 'graph': None, 'images': images, 'labels': labels}
    return g

  def test_step(self, data, sync_loss=True):
    """tf2/train_lib.py:686-732: data = (images, labels) as train_step takes them -> {'cls_loss', 'box_loss', 'det_loss',
    'reg_l2_loss', 'loss'} of a forward pass with training=False (BatchNorm moving statistics, no stochastic depth) on the
    model's CURRENT variables, config.label_smoothing honoured as in training, the normalizer sum(mean_num_positives) + 1 on
    the device or a host 'normalizer'.  The loss kernels are the training kernels without their gradient half
    (edet_focal_loss_eval, edet_box_loss_eval: the same sums bit for bit) and edet_l2_loss, which reads the variables only:
    reg_l2_loss is what the next train_step reports.

    Nothing moves: no variable, optimizer slot, BatchNorm moving statistic, iteration count, input_rng_state or gradient
    buffer.  That includes the moving loss normalizer of positives_momentum > 0: the step uses v * m + x * (1 - m) from the
    stored value v and does NOT store it -- a deliberate difference from the reference, whose _detection_loss runs Keras'
    moving_average_update in test_step too, so that validation never moves the training state.

    With use_graph the first call per batch shape is eager and later calls replay a captured graph of their own (static
    buffers: evaluation copies, or the evaluation input stage's destinations for test_step_raw).  The values are not
    averaged over batches; that is the caller's."""
    images, labels = data
    b, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    eng = self._ensure_engine(b, h, w)
    images, labels = self._to_device_images(images, eng), self._labels_to_device(labels, eng)
    if self.use_graph:
      images, labels = self._stage(self._eval_graph_state(eng, lambda: self._static_like(images, labels)), images, labels)
    self._eval_pass(eng, images, labels)
    return eng.eval_loss_values() if sync_loss else {}

  def test_step_raw(self, data, sync_loss=True):
    """test_step from a raw batch: data = (raw_images uint8 [B, H, W, 3], boxes float32 [B, M, 4] normalised, classes [B, M],
    counts [B], is_crowds [B, M], areas [B, M], source_ids [B]).  The evaluation branch of the input pipeline
    (det_input.DetectionEvalInput: no draws, no GridMask, no AutoAugment) runs on the device in front of the pass, straight
    into the captured pass's static buffers.  -> (loss values, labels): labels also holds 'source_ids', 'image_scales' and
    'groundtruth_data', so a caller can go on to detections without a second input pass (the buffers are reused by the next
    call).  raw_images may be the pair (raw, sizes) of a canvas batch, as train_step_raw takes it: 'image_scales' and the
    ground truth are then each image's own."""
    raw, boxes, classes, counts, is_crowds, areas, source_ids = data
    eng, inp, raw, sizes = self._raw_input(raw, boxes, training=False)
    if self.use_graph:
      g = self._eval_graph_state(eng, inp.own_buffers)
      images, labels = g['images'], g['labels']
      for k, (shape, dt) in inp.label_shapes().items():      # a capture that test_step made: without the ground-truth keys
        if k not in labels:
          labels[k] = torch.empty(shape, dtype=dt, device=eng.device)
    else:
      images, labels = inp.own_buffers()
    inp.run(raw, boxes, classes, counts, is_crowds, areas, source_ids, images, labels, sizes=sizes)
    self._eval_pass(eng, images, labels)
    return (eng.eval_loss_values() if sync_loss else {}), labels

  # ---- fit / evaluate: the loop of tf.keras.Model.fit as tf2/train.py:283-290 calls it ----------------------------------
  def _accumulate(self, name, sums, first):
    """acc[name] (+)= Engine.LOSS_KEYS of the step whose sums lie in `sums`, on the current stream: Engine.loss_vector, then ONE
    in-place add into the accumulator, in step order.  first: the accumulator starts at zero.  Nothing is read."""
    if name not in self._loss_acc:
      dev = sums.device
      n = len(self._loss_keys())
      self._loss_acc[name] = (torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev))
    acc, vec = self._loss_acc[name]
    if first:
      acc.zero_()
    acc.add_(self.engine.loss_vector(sums, vec))
    return acc

  def _read_losses(self, acc):
    """The one place fit and evaluate read loss values from the device (it waits for the stream) -> float32 numpy [5]."""
    return acc.detach().cpu().numpy()

  def _mean_losses(self, acc, steps, prefix=''):
    """Keras' Mean: total / count, both float32, the total summed on the device in step order."""
    mean = self._read_losses(acc) / np.float32(steps)
    return {prefix + k: float(mean[i]) for i, k in enumerate(self._loss_keys())}

  def evaluate(self, x, steps=None):
    """tf.keras.Model.evaluate over test_step: x = an iterable of the raw batches test_step_raw takes; -> the means of its five
    values (six with the IoU loss on: box_iou_loss) over `steps` batches (all of them for None), accumulated on the device and read ONCE, at the end.  Like test_step
    it moves nothing of the training state."""
    acc, n = None, 0
    for batch in x:
      if steps is not None and n >= steps:
        break
      self.test_step_raw(batch, sync_loss=False)
      acc = self._accumulate('evaluate', self.engine.eval_sums, n == 0)
      n += 1
    if not n:
      raise ValueError('evaluate: the data holds no batch')
    return self._mean_losses(acc, n)

  def fit(self, x, epochs=1, steps_per_epoch=None, initial_epoch=0, callbacks=None, validation_data=None, validation_steps=None,
          verbose=1):
    """tf.keras.Model.fit for the detector.  x: an iterator of raw batches as dataloader.InputReader(...)(params, batch_size,
    canvas=...) yields them; every batch goes to train_step_raw(batch, sync_loss=False).  An epoch is steps_per_epoch batches,
    or the iterator's end for None; the iterator is NOT restarted between epochs (the reader repeats on its own), and fit
    ends early when it runs dry.  -> History: .history = {name: [value per epoch]}, .epoch = the epoch numbers.

    The loop does not wait for the device per step.  After a step its loss values are added, on the step's stream, into a
    float32 device accumulator (_accumulate); the epoch's logs are accumulator / steps in float32 -- Keras' Mean with the sum
    in step order -- for loss, cls_loss, box_loss, det_loss, reg_l2_loss (and box_iou_loss with the IoU loss on), plus learning_rate of the last step.  The waits
    are the reader's arena event, the one read at the end of an epoch, a batch-level callback that ACCESSES a device value of
    its logs (LazyLogs: the running means of the epoch), and a checkpoint.

    validation_data: an iterable of test_step_raw's batches that can be iterated once per epoch (a list, or
    RepeatableReader(reader)); every epoch ends with evaluate(validation_data, steps=validation_steps), whose values enter
    the logs under 'val_' + name.  callbacks: objects with any of set_model, on_train_begin, on_train_end(logs),
    on_epoch_begin(epoch, logs), on_epoch_end(epoch, logs), on_train_batch_end(step, logs); a callback that sets
    model.stop_training ends the run after the epoch."""
    if self.use_dist:
      raise ValueError('data-parallel fit is not built: the replicas would each average their own losses and write the same '
                       'checkpoint; drive train_step_raw per replica by hand')
    callbacks = list(callbacks or [])

    def call(name, *args):
      for cb in callbacks:
        fn = getattr(cb, name, None)
        if fn is not None:
          fn(*args)
    batch_level = [cb.on_train_batch_end for cb in callbacks if getattr(cb, 'on_train_batch_end', None) is not None]
    history = History()
    self.fit_input, self.stop_training = x, False
    it = iter(x)
    call('set_model', self)
    call('on_train_begin', None)
    logs = {}
    for epoch in range(int(initial_epoch), int(epochs)):
      call('on_epoch_begin', epoch, None)
      acc, steps, lr = None, 0, None
      while steps_per_epoch is None or steps < steps_per_epoch:
        try:
          batch = next(it)
        except StopIteration:
          break
        lr = self.train_step_raw(batch, sync_loss=False)['learning_rate']
        acc = self._accumulate('fit', self.engine.loss_sums, steps == 0)
        steps += 1
        if batch_level:
          blogs = LazyLogs({'learning_rate': lr, 'step': self.iterations}, self._loss_keys(),
                           lambda acc=acc, steps=steps: self._mean_losses(acc, steps))
          for fn in batch_level:
            fn(steps - 1, blogs)
      if not steps:
        break      # the data ran dry at an epoch's border
      logs = self._mean_losses(acc, steps)
      logs['learning_rate'] = lr
      if validation_data is not None:
        logs.update({'val_' + k: v for k, v in self.evaluate(validation_data, steps=validation_steps or None).items()})
      call('on_epoch_end', epoch, logs)
      history.append(epoch, logs)
      if verbose:
        print('Epoch %d/%d: %d steps - %s' % (epoch + 1, epochs, steps, ' - '.join(
            '%s: %.4g' % (k, v) for k, v in logs.items() if isinstance(v, (int, float)) and not k.startswith('AP_/'))), flush=True)
      if self.stop_training or (steps_per_epoch is not None and steps < steps_per_epoch):
        break
    call('on_train_end', logs)
    return history


class History(object):
  """What fit returns (tf.keras.callbacks.History): .history = {name: [one value per epoch]}, .epoch = [epoch numbers]."""

  def __init__(self):
    self.history, self.epoch = {}, []

  def append(self, epoch, logs):
    self.epoch.append(epoch)
    for k, v in logs.items():
      self.history.setdefault(k, []).append(v)


class LazyLogs(collections.abc.Mapping):
  """The logs of a batch-level callback: `host` values (learning_rate, step) are plain; the values under `device_keys` are
  read -- read() -> {key: value}, one wait for the device, at most once per batch -- only when one of them is ACCESSED.
  Asking for the keys, for membership or for a host value reads nothing."""

  def __init__(self, host, device_keys, read):
    self._host, self._device_keys, self._read, self._values = dict(host), tuple(device_keys), read, None

  def __getitem__(self, key):
    if key in self._host:
      return self._host[key]
    if key not in self._device_keys:
      raise KeyError(key)
    if self._values is None:
      self._values = self._read()
    return self._values[key]

  def __iter__(self):
    yield from self._device_keys
    yield from self._host

  def __len__(self):
    return len(self._device_keys) + len(self._host)

  def __contains__(self, key):
    return key in self._host or key in self._device_keys


class RepeatableReader(object):
  """An evaluation reader (dataloader.DeviceReader: one pass, then it has ended) as data that can be iterated again and again,
  which fit's validation_data and COCOCallback need once per epoch: every iter() puts the reader back to the state it was
  wrapped in and hands it out."""

  def __init__(self, reader):
    self.reader = reader
    self._initial = reader.get_state()

  def __iter__(self):
    self.reader.set_state(self._initial)
    return iter(self.reader)

  def close(self):
    self.reader.close()


class COCOCallback(object):
  """tf2/train_lib.py:202-250: COCO AP of the model on a test set every `update_freq` epochs.  test_batches: an iterable of
  the raw tuples eval_lib.evaluate takes.  set_model(model) builds the evaluator from the model's config (val_json_file,
  label_map); on_epoch_end(epoch, logs) follows :232-248 as written -- epoch += 1, then `update_freq and epoch % update_freq
  == 0` -- resets the evaluator, runs config.eval_samples // config.batch_size batches when both are set (:237-238; all of
  them otherwise) and puts the metrics into `logs` under evaluator.metric_names.  No summary writer.  update_freq is
  config.map_freq in the reference's get_callbacks (:343-346)."""

  def __init__(self, test_batches, update_freq=None):
    self.test_dataset = test_batches
    self.update_freq = update_freq
    self.model = self.config = self.evaluator = None

  def set_model(self, model):
    from automl_amd import coco_metric
    self.model = model
    self.config = model.config
    self.evaluator = coco_metric.EvaluationMetric(filename=getattr(self.config, 'val_json_file', None),
                                                  label_map=getattr(self.config, 'label_map', None))

  def on_epoch_end(self, epoch, logs=None):
    from automl_amd import eval_lib
    epoch += 1
    if self.update_freq and epoch % self.update_freq == 0:
      self.evaluator.reset_states()
      samples, batch = getattr(self.config, 'eval_samples', None), getattr(self.config, 'batch_size', None)
      count = samples // batch if samples and batch else None
      metrics = eval_lib.evaluate(self.model, self.test_dataset, evaluator=self.evaluator, max_batches=count)
      eval_results = {name: metrics[name] for name in self.evaluator.metric_names}
      if logs is not None:
        logs.update(eval_results)
      return eval_results
    return None


# ---- the training-state file: everything a next step reads that util_keras.save_ckpt does not hold ---------------------------
TRAIN_STATE_SUFFIX = '.train_state.npz'
TRAIN_STATE_FORMAT = 1
_SLOT_KEYS = ('velocity', 'ema', 'adam_v', 'rms')


def train_state_path(ckpt_prefix):
  return ckpt_prefix + TRAIN_STATE_SUFFIX


def _shape_key(batch, height, width):
  return '%dx%dx%d' % (batch, height, width)


def arena_length(model):
  """Elements of the model's flat variable arena (layer_engine.ParamArena: the trainable variables in creation order, each
  padded to a multiple of four), from the variable list alone -- no device."""
  from automl_amd import util_keras
  return sum(((int(np.prod(shape)) if shape else 1) + 3) // 4 * 4 for _, shape, trainable in util_keras.model_variables(model) if trainable)


def check_arena_length(state, arena):
  if int(np.asarray(state['velocity']).size) != int(arena.velocity.numel()):
    raise ValueError('the training state is another model\'s: its arena holds %d elements, this model\'s %d'
                     % (np.asarray(state['velocity']).size, arena.velocity.numel()))


def _model_identity(model):
  from automl_amd import util_keras
  return {'num_variables': len(util_keras.model_variables(model)), 'arena_length': arena_length(model),
          'optimizer': str(getattr(model.config, 'optimizer', 'sgd')).lower()}


def lion_identity(update):
  """What a training-state file carries of a Lion update besides the optimizer's name (beta_1 is the momentum both trainers
  already have): {'beta_2':, 'wd':}; None for every other kind."""
  return {'beta_2': float(update.beta2), 'wd': float(update.wd or 0.0)} if update.kind == 'lion' else None


def lion_difference(theirs, mine):
  """The differences between a file's 'lion' entry and this model's, worded for restore_train_state's refusal."""
  if mine is None:
    return []
  theirs = theirs or {}
  return ['lion %s %r, this model %r' % (k, theirs.get(k), mine[k]) for k in ('beta_2', 'wd') if theirs.get(k) != mine[k]]


def iou_loss_identity(model):
  """What a training-state file carries of the IoU loss: {'type':, 'weight':}; None with it off (and the file is as without)."""
  iou = getattr(model, '_iou_loss', None)
  return {'type': iou[0], 'weight': float(iou[1])} if iou else None


def iou_loss_difference(theirs, mine):
  """The differences between a file's 'iou_loss' entry and this model's, worded for restore_train_state's refusal."""
  if theirs == mine:
    return []
  if theirs is None or mine is None:
    return ['iou_loss %r, this model %r' % (theirs, mine)]
  return ['iou_loss %s %r, this model %r' % (k, theirs.get(k), mine[k]) for k in ('type', 'weight') if theirs.get(k) != mine[k]]


def save_train_state(model, path, reader=None):
  """Writes <ckpt prefix>.train_state.npz next to a checkpoint: get_optimizer_state() in full (velocity, ema, the second slot
  under its key, iterations, moving_normalizer, input_rng_state), the stochastic-depth generator's state of every engine the
  model holds (by batch x height x width), and reader.get_state() -- with the variables, the shadows and the BatchNorm
  statistics of the checkpoint, everything the next step reads.  Arrays are npz members; everything else is ONE JSON member,
  'meta' (uint8).  No pickle.  Reading the slots waits for the device."""
  state = model.get_optimizer_state()
  arrays, meta = {}, {'format': TRAIN_STATE_FORMAT}
  meta.update(_model_identity(model))
  if meta['optimizer'] == 'lion':
    meta['lion'] = lion_identity(model.update)
  if iou_loss_identity(model) is not None:
    meta['iou_loss'] = iou_loss_identity(model)
  for k, v in state.items():
    if k in _SLOT_KEYS or k == 'input_rng_state':
      arrays[k] = np.asarray(v)
    elif k == 'iterations':
      meta[k] = int(v)
    elif k == 'moving_normalizer':
      meta[k] = float(v)
    else:
      raise ValueError('save_train_state: the optimizer state has a key this file has no place for: %r' % (k,))
  for (b, h, w), eng in getattr(model, '_engines', {}).items():
    arrays['drop_rng.' + _shape_key(b, h, w)] = np.asarray(eng.drop_rng_state(), np.uint8)
  for key, v in getattr(model, '_pending_drop_rng', {}).items():      # restored, and its engine not made since
    arrays.setdefault('drop_rng.' + key, np.asarray(v, np.uint8))
  meta['reader'] = None if reader is None else reader.get_state()
  arrays['meta'] = np.frombuffer(json.dumps(meta).encode('utf-8'), np.uint8)
  tmp = path + '.tmp'
  with open(tmp, 'wb') as f:
    np.savez(f, **arrays)
  os.replace(tmp, path)
  return path


def load_train_state(path):
  """-> (meta dict, {member: array}) of a training-state file; allow_pickle=False."""
  with np.load(path, allow_pickle=False) as z:
    arrays = {k: z[k] for k in z.files}
  meta = json.loads(arrays.pop('meta').tobytes().decode('utf-8'))
  if meta.get('format') != TRAIN_STATE_FORMAT:
    raise ValueError('%s: training-state format %r, this code reads %d' % (path, meta.get('format'), TRAIN_STATE_FORMAT))
  return meta, arrays


def restore_train_state(model, path, reader=None):
  """Puts a save_train_state file back into `model` (and the reader's part into `reader`).  A file from another model is
  refused with the difference named: the variable count, the arena length or the optimizer.  A model without an engine keeps
  the state until its first engine is made (as set_weights / set_ema_weights do); model.iterations is set at once, so the
  caller can form initial_epoch from it.  -> the meta dict."""
  meta, arrays = load_train_state(path)
  mine = _model_identity(model)
  what = {'num_variables': 'variables', 'arena_length': 'arena elements', 'optimizer': 'as optimizer'}
  diff = ['%s %s, this model %s' % (meta.get(k), what[k], mine[k]) for k in ('num_variables', 'arena_length', 'optimizer')
          if meta.get(k) != mine[k]]
  if not diff and mine['optimizer'] == 'lion':
    diff = lion_difference(meta.get('lion'), lion_identity(model.update))
  if not diff:
    diff = iou_loss_difference(meta.get('iou_loss'), iou_loss_identity(model))
  if diff:
    raise ValueError('%s is the training state of another model: the file has %s' % (path, '; '.join(diff)))
  state = {k: arrays[k] for k in _SLOT_KEYS + ('input_rng_state',) if k in arrays}
  state['iterations'] = int(meta['iterations'])
  if 'moving_normalizer' in meta:
    state['moving_normalizer'] = float(meta['moving_normalizer'])
  drop = {k[len('drop_rng.'):]: v for k, v in arrays.items() if k.startswith('drop_rng.')}
  if reader is not None:
    if meta.get('reader') is None:
      raise ValueError('%s holds no reader state' % (path,))
    reader.set_state(meta['reader'])
  if model.engine is None:
    model._pending_state, model._pending_drop_rng = state, drop
    model.iterations = state['iterations']
  else:
    check_arena_length(state, model.engine.arena)
    model.set_optimizer_state(state)
    model._pending_drop_rng = {}
    for (b, h, w), eng in model._engines.items():
      if _shape_key(b, h, w) in drop:
        eng.set_drop_rng_state(drop.pop(_shape_key(b, h, w)))
    model._pending_drop_rng = drop
  return meta


# ---- callbacks (tf2/train_lib.py:293-325) ------------------------------------------------------------------------------------
class ModelCheckpoint(object):
  """tf.keras.callbacks.ModelCheckpoint(save_weights_only=True) / tfa AverageModelCheckpoint(update_weights=False) as
  get_callbacks uses them: save_freq='epoch' saves at every epoch's end, an integer every that many batches.  The file is
  util_keras.save_ckpt(model, filepath.format(epoch=epoch + 1), ema=bool(moving_average_decay), global_step=iterations) --
  the name-based layout, plain variables and /ExponentialMovingAverage shadows in one checkpoint -- and next to it the
  training-state file with the state of the iterator fit reads from.  Saving waits for the device."""

  def __init__(self, filepath, save_freq='epoch', verbose=0):
    if save_freq != 'epoch' and (not isinstance(save_freq, int) or save_freq < 1):
      raise ValueError("save_freq must be 'epoch' or a positive number of batches, got %r" % (save_freq,))
    self.filepath, self.save_freq, self.verbose = filepath, save_freq, verbose
    self.model = None
    self._epoch = self._batches = 0
    # a batch-level callback only where batches are counted: fit builds batch logs only for callbacks that have one
    self.on_train_batch_end = None if save_freq == 'epoch' else self._count_batch

  def set_model(self, model):
    self.model = model

  def _count_batch(self, step, logs=None):
    self._batches += 1
    if self._batches % self.save_freq == 0:
      self.save(self._epoch)

  def on_epoch_begin(self, epoch, logs=None):
    self._epoch = epoch

  def on_epoch_end(self, epoch, logs=None):
    if self.save_freq == 'epoch':
      self.save(epoch)

  def save(self, epoch):
    from automl_amd import util_keras
    model = self.model
    prefix = self.filepath.format(epoch=epoch + 1)
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    util_keras.save_ckpt(model, prefix, ema=bool(model.config.moving_average_decay), global_step=model.iterations)
    reader = model.fit_input if hasattr(model.fit_input, 'get_state') else None
    save_train_state(model, train_state_path(prefix), reader)
    if self.verbose:
      print('Epoch %d: saving model to %s' % (epoch + 1, prefix), flush=True)
    return prefix


def get_callbacks(params, val_dataset=None):
  """tf2/train_lib.py:293-325: the checkpoint callback -- <model_dir>/emackpt-{epoch:d} with moving_average_decay,
  <model_dir>/ckpt-{epoch:d} without, the reference's names -- and COCOCallback(val_dataset, map_freq) when both are given.
  TensorBoard is left out; sample_image (DisplayCallback: the visualisation is not built) raises."""
  if params.get('sample_image', None):
    raise ValueError('sample_image=%r: DisplayCallback is not built (it needs the visualisation of '
                     'visualize/vis_utils.py, tf2/train_lib.py:253-290)' % (params['sample_image'],))
  name = 'emackpt-{epoch:d}' if params['moving_average_decay'] else 'ckpt-{epoch:d}'
  ckpt = ModelCheckpoint(os.path.join(params['model_dir'], name), save_freq=params.get('save_freq', 'epoch'),
                         verbose=params.get('verbose', 0))
  callbacks = [ckpt]
  if params.get('map_freq', None) and val_dataset is not None and params.get('strategy', None) != 'tpu':
    callbacks.append(COCOCallback(val_dataset, params['map_freq']))
  return callbacks
