"""EfficientNetV2 classifier training on one MI355X: the reference's TF2 trainer on the HIP kernels.

Mirror of ``efficientnetv2/main_tf2.py``: ``TrainableModel`` (:62-117, ``train_step`` / ``test_step``) on top of
``EffNetV2Model``, ``build_tf2_optimizer`` (:36-59: RMSprop(rho 0.9, momentum 0.9, epsilon 0.001) by default,
hparams.py:249; 'momentum', 'sgd', 'adam'), the compiled loss ``CategoricalCrossentropy(label_smoothing,
from_logits=True)`` with the ``acc_top1`` / ``acc_top5`` metrics (:199-207), and ``WarmupLearningRateSchedule``
(``efficientnetv2/utils.py:78-131``).

One step = [``V2Engine.crop_batch``: crop, bilinear resize and flip of the decoded uint8 images, with ``image_size`` set] ->
[``V2Engine.randaug_batch``: RandAugment of the uint8 batch and its normalisation into the static image
buffer, with ``augname='randaug'``] -> [``V2Engine.mix_batch``: mixup / cutmix of the images in place and of the labels into soft labels, when an
alpha is non-zero] -> forward(training) with stochastic depth and head dropout -> ``edet_softmax_xent`` /
``edet_softmax_xent_soft`` (loss, d logits and the metric counts in one pass) -> ``V2Engine.backward`` -> ``LayerEngine.optimizer_local`` (the L2 term of ``_reg_l2_loss`` and the
gradient norm; the reference clips nothing, gclip = 0) -> ``LayerEngine.optimizer_apply`` with this trainer's ``Update``
(``edet_opt_rmsprop_ema``, or the SGD / Adam entry point).  The BatchNorm moving statistics move in the forward pass.  With ``use_graph`` the step is captured once
into a hipGraph and replayed; the learning rate travels through a device vector and the dropout / stochastic-depth masks
are redrawn outside the graph, and so are the mixup weights and cutmix boxes and the RandAugment arguments.

RandAugment (``augname='randaug'``, ``ra_num_layers``, ``ra_magnitude``; ``randaug_params(model_name)`` for a named model's
recipe, ``set_randaug`` between steps; ``automl_amd/autoaugment.py``) runs on the device in front of the mixing, per image as
in the reference (``preprocessing.py:107-153``): ``train_step`` then takes the **uint8** images [B, H, W, 3] that the reference
hands ``distort_image`` after crop, resize, flip and the clip / cast of ``preprocessing.py:49-50``, and normalises them
(x - 128) / 128 itself; ``test_step`` only normalises.  The draws come from a third host generator seeded by the model's
seed, whose state travels with the optimizer state under 'randaug_rng_state' (present only when ``augname`` is set).

Crop, resize and flip on the device; staged sizes (``image_size``, ``eval_image_size``, ``transformations``;
``automl_amd/v2_preprocessing.py``, the reference's ``preprocessing.py:22-70``): ``train_step`` then takes the **decoded uint8
images** on a common canvas of any size, ``((raw [B, Hc, Wc, 3], sizes [B, 2]), labels)`` or ``({'image': raw, 'size':
sizes}, {'label': ...})`` (``sizes`` may be left out when every image fills the canvas; ``v2_preprocessing.pad_batch`` makes
both), draws one crop and one flip bit per image on the host from a fourth generator seeded by the model's seed
('crop_rng_state' in the optimizer state, present only when ``image_size`` is set), and runs ``edet_crop_resize`` as the first
launch of the step, in front of RandAugment and the mixing.  ``test_step`` on the same input does ``preprocess_for_eval``.
``progressive_stages(model_name, epochs)`` restates the staged schedule of ``main_tf2.py:256-275`` and ``set_stage`` /
``set_image_size`` apply it between steps: a new size builds a new executor on the same variable arena and the step is captured
again.  The crop sampler's random stream and the float32 staircase of ``tf.image.resize`` are not pinned against TensorFlow
(``v2_preprocessing``'s docstring).

Labels are the reference's dense float labels [B, C] (``datasets.py:321-323``: one-hot, or mixed by the caller's own
pipeline; used as they are) or sparse integer class ids [B].  Mixup / cutmix (``datasets.py:191-301``; ``mixup_alpha`` /
``cutmix_alpha`` of the constructor, ``set_mix_alphas`` between steps, ``mix_alphas(model_name)`` for a named model's
recipe) run on the device and take integer labels: rows [0, n_mixup) of the batch are mixed by mixup and the rest by
cutmix, each part with itself in reverse order as ``mixing`` does (``mix_split``); the draws come from a host generator
seeded by the model's seed whose state travels with the optimizer state.  Mixing float labels on the device is not built
(a ``ValueError``).

``TrainableModel.fit`` / ``.evaluate`` are the loop of ``tf.keras.Model.fit`` as ``main_tf2.py:235-295`` calls it, over
``train_step`` / ``test_step`` without a wait for the device per step: the step's ``cls_sums`` are added on the device into a
float32 accumulator that is read once per epoch, and ``metrics_from_sums`` is the one place the four metrics are formed, for a
step and for an epoch.  ``fit(stages=...)`` applies the progressive stage of every epoch through ``set_stage``.
``save_train_state`` / ``restore_train_state`` write and read, next to a checkpoint, everything else a next step reads (both
slots, the shadows, the iteration count, the four generators, the current stage, the reader's position), so that an
interrupted run continues bit for bit; ``ModelCheckpoint`` is ``train_lib``'s callback writing this trainer's two files.  The
reader is automl_amd/effnetv2_datasets.py, the entry point automl_amd/effnetv2_main.py.

Single GPU.  Not built, and raising or absent rather than ignored: data-parallel classifier training, ``conv_dropout``,
``ra_aa``, the ``ft*`` fine-tuning preprocessing, the TF1 trainer's EMA-of-everything.  The legacy ``effnetv1_*`` input
pipeline (``preprocess_legacy.py``: bicubic crop-resize, AutoAugment v0 or RandAugment, mean / stddev normalisation) is built
under keywords of its own, ``preprocessing='legacy'`` and ``augment_name``; ``augname`` keeps refusing the reference's
spellings of it.  ``ema_decay`` is a constant-decay TFA MovingAverage shadow of the trainable variables (None, the
reference's TF2 trainer, keeps none).
"""
import json
import math
import os

import numpy as np
import torch

from automl_amd import autoaugment
from automl_amd import effnetv2_model
from automl_amd import preprocess_legacy
from automl_amd import train_lib
from automl_amd import util_keras
from automl_amd import utils
from automl_amd import v2_preprocessing
from automl_amd.layer_engine import LION_BETA2, LION_WD, LayerEngine, Update, capture_graph, lion_options

OPTIMIZERS = ('rmsprop', 'momentum', 'sgd', 'adam', 'lion')


def build_update(optimizer, momentum, lion_beta2=LION_BETA2, lion_wd=LION_WD):
  """build_tf2_optimizer (main_tf2.py:36-59) as the engine's update description: 'rmsprop' (rho 0.9, momentum, epsilon
  0.001), 'momentum' / 'sgd' (Keras SGD; the trainer passes momentum 0 for 'sgd'), 'adam' (tf.keras.optimizers.Adam(learning_rate) defaults);
  and 'lion' (lion/lion_tf2.py's Lion, what a user of the reference passes to Keras in the optimizer's place: beta_1 = momentum,
  beta_2, decoupled decay wd)."""
  if optimizer == 'lion':
    beta_2, wd = lion_options({'beta_2': lion_beta2, 'wd': lion_wd})
    if not 0.0 <= momentum < 1.0:
      raise ValueError('lion: beta_1 (momentum) %r outside [0, 1)' % (momentum,))
    return Update('lion', momentum, beta_2, wd=wd)
  if optimizer == 'rmsprop':
    return Update('rmsprop', momentum, epsilon=0.001, rho=0.9)
  if optimizer == 'adam':
    return Update('adam', 0.9, LayerEngine.ADAM_BETA2, LayerEngine.ADAM_EPSILON)
  return Update('sgd', momentum)


class WarmupLearningRateSchedule(object):
  """efficientnetv2/utils.py:78-131, evaluated on the host for an integer step."""

  def __init__(self, initial_lr, steps_per_epoch=None, lr_decay_type='exponential', decay_factor=0.97, decay_epochs=2.4,
               total_steps=None, warmup_epochs=5, minimal_lr=0):
    if lr_decay_type not in ('exponential', 'cosine', 'linear', 'constant'):
      raise ValueError('Unknown lr_decay_type : %s' % lr_decay_type)
    self.initial_lr = initial_lr
    self.steps_per_epoch = steps_per_epoch
    self.lr_decay_type = lr_decay_type
    self.decay_factor = decay_factor
    self.decay_epochs = decay_epochs
    self.total_steps = total_steps
    self.warmup_epochs = warmup_epochs
    self.minimal_lr = minimal_lr

  def __call__(self, step):
    step = int(step)
    if self.lr_decay_type == 'exponential':
      assert self.steps_per_epoch is not None
      decay_steps = self.steps_per_epoch * self.decay_epochs
      # tf.keras ExponentialDecay(staircase=True): initial * factor ^ floor(step / decay_steps).  Keras divides in float32,
      # this host in double: where decay_steps is not exactly representable the two can sit one stair apart for the one
      # step at a boundary (not pinned: TensorFlow is not available to the tests)
      lr = self.initial_lr * self.decay_factor ** math.floor(step / decay_steps)
    elif self.lr_decay_type == 'cosine':
      assert self.total_steps is not None
      lr = 0.5 * self.initial_lr * (1 + math.cos(math.pi * float(step) / self.total_steps))
    elif self.lr_decay_type == 'linear':
      assert self.total_steps is not None
      lr = (1.0 - float(step) / self.total_steps) * self.initial_lr
    else:
      lr = self.initial_lr
    if self.minimal_lr:
      lr = max(lr, self.minimal_lr)
    if self.warmup_epochs:
      warmup_steps = int(self.warmup_epochs * self.steps_per_epoch)
      if step < warmup_steps:
        lr = self.initial_lr * float(step) / float(warmup_steps)
    return float(lr)

  def get_config(self):
    return {k: getattr(self, k) for k in ('initial_lr', 'steps_per_epoch', 'lr_decay_type', 'decay_factor',
                                          'decay_epochs', 'total_steps', 'warmup_epochs', 'minimal_lr')}


# ---- mixup / cutmix draws (efficientnetv2/datasets.py:191-301): pure host functions ------------------------------------
def mix_alphas(model_name):
  """(data.mixup_alpha, data.cutmix_alpha) of a named model's training recipe (effnetv2_configs; hparams.py:282-283 = 0, 0
  where the model names none).  The reference ramps them per progressive-training stage (main_tf2.py:262-275):
  TrainableModel.set_mix_alphas."""
  from automl_amd import effnetv2_configs
  data = effnetv2_configs.get_model_config(model_name).as_dict().get('data') or {}
  return float(data.get('mixup_alpha') or 0.0), float(data.get('cutmix_alpha') or 0.0)


def randaug_params(model_name):
  """(data.augname, data.ra_num_layers, data.ram) of a named model's training recipe (effnetv2_configs; the layer count
  defaults to preprocessing.py:115's 2, the magnitude to :116's 15); augname None where the model names none."""
  from automl_amd import effnetv2_configs
  data = effnetv2_configs.get_model_config(model_name).as_dict().get('data') or {}
  ram = data.get('ram')
  return data.get('augname') or None, int(data.get('ra_num_layers') or 2), 15 if ram is None else ram


def legacy_params(model_name):
  """('autoaug' | 'randaug' | None, data.ra_num_layers, data.ram) of a named model whose recipe names the legacy input pipeline
  (data.augname starts with 'effnetv1_': efficientnetv2-b0 .. b3, efficientnet-b0 .. b7; preprocessing.py:133-139) -- what
  TrainableModel(preprocessing='legacy', augment_name=..., ra_num_layers=..., ra_magnitude=...) takes; None for every other
  model.  The remainder of the name is the augmentation; an empty one means none."""
  augname, layers, magnitude = randaug_params(model_name)
  if not (augname or '').startswith('effnetv1_'):
    return None
  return preprocess_legacy.check_augment_name(augname[len('effnetv1_'):] or None), layers, magnitude


IBASE = 128      # data.ibase of the reference's base configuration (hparams.py:284)


def progressive_stages(model_name, epochs, stages=None, ibase=None, sched=None):
  """The staged schedule of main_tf2.py:256-275 for a named model's recipe (effnetv2_configs: train.isize, train.stages,
  train.sched, data.ram, data.mixup_alpha, data.cutmix_alpha) over `epochs` epochs -> a list of dicts {start_epoch,
  end_epoch, image_size, ra_magnitude, mixup_alpha, cutmix_alpha}, one per stage, for TrainableModel.set_stage.
  Stage k of n: ratio = (k + 1) / n, epochs [int(k / n * epochs), int(ratio * epochs)), image_size = int(ibase +
  (train_size - ibase) * ratio); with `sched` the magnitude ramps np.linspace(5, ram, n) and both alphas np.linspace(0,
  alpha, n), else every stage keeps the model's own values.  ibase: None = IBASE; a falsy value = train_size / 2 (:258).
  stages == 0 (:248-255): one stage at train.isize with the model's own values."""
  from automl_amd import effnetv2_configs
  cfg = effnetv2_configs.get_model_config(model_name).as_dict()
  train, data = cfg.get('train') or {}, cfg.get('data') or {}
  train_size = int(train['isize'])
  total = int(train.get('stages') or 0) if stages is None else int(stages)
  sched = bool(train.get('sched')) if sched is None else bool(sched)
  ram = data.get('ram')
  ram = 15 if ram is None else ram
  mixup, cutmix = float(data.get('mixup_alpha') or 0.0), float(data.get('cutmix_alpha') or 0.0)
  return stage_list(train_size, epochs, total, sched, IBASE if ibase is None else ibase, ram, mixup, cutmix)


def stage_list(train_size, epochs, total, sched, ibase, ram, mixup, cutmix):
  """main_tf2.py:256-275 on plain values (progressive_stages reads them from a named model's recipe, effnetv2_main from the
  assembled configuration): `total` stages over `epochs` epochs up to train_size; a falsy ibase = train_size / 2 (:258)."""
  total = int(total or 0)
  if total < 0:
    raise ValueError('stages %r must be >= 0' % (total,))
  if not total:
    return [dict(start_epoch=0, end_epoch=int(epochs), image_size=train_size, ra_magnitude=float(ram), mixup_alpha=mixup,
                 cutmix_alpha=cutmix)]
  ibase = ibase or (train_size / 2)
  ram_list = np.linspace(5, ram, total) if sched else [ram] * total
  mixup_list = np.linspace(0, mixup, total) if sched else [mixup] * total
  cutmix_list = np.linspace(0, cutmix, total) if sched else [cutmix] * total
  out = []
  for stage in range(total):
    ratio = float(stage + 1) / float(total)
    out.append(dict(start_epoch=int(float(stage) / float(total) * epochs), end_epoch=int(ratio * epochs),
                    image_size=int(ibase + (train_size - ibase) * ratio), ra_magnitude=float(ram_list[stage]),
                    mixup_alpha=float(mixup_list[stage]), cutmix_alpha=float(cutmix_list[stage])))
  return out


def mix_split(batch, mixup_alpha, cutmix_alpha):
  """Rows [0, n_mixup) are mixed by mixup, rows [n_mixup, batch) by cutmix (datasets.py:287-300: both -> batch // 2, mixup
  only -> batch, cutmix only -> 0); None = no mixing."""
  if mixup_alpha and cutmix_alpha:
    return batch // 2
  if mixup_alpha:
    return batch
  if cutmix_alpha:
    return 0
  return None


def cutmix_box(r_y, r_x, area, h, w):
  """cutmix_mask (datasets.py:191-211) for its three draws -> (y1, x1, y2, x2), half-open: ratio = float32(sqrt(1 - area)),
  r_w = int(ratio * w), r_h = int(ratio * h) (float32 products, truncated), the box of that size centred on (r_y, r_x),
  clipped to the image."""
  ratio = np.float32(np.sqrt(1.0 - float(area)))
  r_w = int(ratio * np.float32(w))
  r_h = int(ratio * np.float32(h))
  clip = lambda v, hi: int(min(max(v, 0), hi))
  return (clip(r_y - r_h // 2, h), clip(r_x - r_w // 2, w), clip(r_y + r_h // 2, h), clip(r_x + r_w // 2, w))


def mix_rng(seed):
  """The generator behind the mixup / cutmix draws of a model built with `seed`."""
  return np.random.Generator(np.random.PCG64([int(seed), 0x6d6978]))


def draw_beta(rng, alpha, n):
  """n draws of Beta(alpha, alpha), float64."""
  return rng.beta(alpha, alpha, size=n)


def draw_mix(rng, batch, h, w, mixup_alpha, cutmix_alpha):
  """One step's draws -> (weights float32 [batch], boxes int32 [batch, 4]).  Mixup rows (datasets.py:261-262):
  w_i = max(beta, 1 - beta), beta ~ Beta(alpha, alpha); their boxes are empty.  Cutmix rows (:191-203): r_x ~ U{0..w-1},
  r_y ~ U{0..h-1}, area ~ Beta(alpha, alpha) -> cutmix_box; their weights are 1."""
  n = mix_split(batch, mixup_alpha, cutmix_alpha)
  weights = np.ones(batch, np.float32)
  boxes = np.zeros((batch, 4), np.int32)
  if n:
    beta = draw_beta(rng, mixup_alpha, n)
    weights[:n] = np.maximum(beta, 1.0 - beta).astype(np.float32)
  for i in range(n, batch):
    r_x = int(rng.integers(0, w))
    r_y = int(rng.integers(0, h))
    boxes[i] = cutmix_box(r_y, r_x, float(draw_beta(rng, cutmix_alpha, 1)[0]), h, w)
  return weights, boxes


_pack_rng_state, _unpack_rng_state = utils.pack_rng_state, utils.unpack_rng_state

METRIC_KEYS = ('loss', 'reg_l2_loss', 'acc_top1', 'acc_top5')


def metrics_from_sums(sums, steps, batch, dtype=np.float32, prefix=''):
  """The one place the four metrics are formed from sums laid out as V2Engine.cls_sums (mean loss, top-1 rows, top-5 rows,
  L2 loss), added up over `steps` steps of `batch` images: loss = (A[0] + A[3]) / n, reg_l2_loss = A[3] / n, acc_top1 = A[1] /
  (n B), acc_top5 = A[2] / (n B) -- Keras' Mean and TopKCategoricalAccuracy over equal batches.  dtype: the arithmetic's;
  float32 for the epoch logs of fit and evaluate, float64 for the single step's values of train_step / test_step."""
  a = np.asarray(sums).astype(dtype)
  n, rows = dtype(steps), dtype(steps) * dtype(batch)
  return {prefix + 'loss': float((a[0] + a[3]) / n), prefix + 'reg_l2_loss': float(a[3] / n),
          prefix + 'acc_top1': float(a[1] / rows), prefix + 'acc_top5': float(a[2] / rows)}


def stage_of_epoch(stages, epoch):
  """The entry of a progressive_stages list whose [start_epoch, end_epoch) holds `epoch`; None when none does."""
  for stage in stages:
    if stage['start_epoch'] <= epoch < stage['end_epoch']:
      return stage
  return None


class TrainableModel(effnetv2_model.EffNetV2Model):
  """EffNetV2Model plus the reference's train_step / test_step (main_tf2.py:62-117).

  learning_rate: a float or a callable of the iteration count (WarmupLearningRateSchedule).  use_graph: capture the step
  at its second call for a batch shape and replay it afterwards; False = every launch eager (the tests compare both).
  check_device_labels: also range-check labels that arrive as device tensors (one synchronisation per step).
  ``momentum`` is build_tf2_optimizer's (0.9), used by 'rmsprop' and 'momentum'; optimizer='lion' takes it as beta_1, with
  ``lion_beta2`` and ``lion_wd`` (lion_tf2.Lion's beta_2 and wd; the decay reaches every variable, as the reference's does).
  mixup_alpha / cutmix_alpha: the Beta parameters of datasets.py:244-301 (0 = off, the default: the step is then exactly
  the unmixed one); a named model's own pair is mix_alphas(model_name).
  augname: None (the default: nothing changes) or 'randaug' -- RandAugment of ra_num_layers layers at ra_magnitude on the
  device (the reference's defaults, preprocessing.py:115-116; a named model's own are randaug_params(model_name));
  train_step then takes uint8 images.  The other names of the reference raise.
  image_size: None (the default: nothing changes) or the training size -- train_step then takes decoded uint8 images on a
  canvas of any size (with their sizes) and crops, resizes and flips them on the device (`transformations`, the
  reference's 'crop|flip'; '' = the whole image, unflipped); test_step centre-crops and resizes them to eval_image_size
  (default: image_size).  The captured step is keyed on the canvas shape: a new one makes the next step eager and the one
  after it captured again, so a fixed canvas (pad_batch(images, canvas)) keeps the graph.
  preprocessing: None (the default: nothing changes) or 'legacy' -- the reference's preprocess_legacy.py in front of the
  network (automl_amd/preprocess_legacy.py; a named model's own recipe is legacy_params(model_name)): needs image_size (the
  path starts from decoded canvases) and augname=None.  train_step then draws legacy_train_rows (with transformations='flip':
  whole-image rows plus the flip draw, for a reader that already cut the windows), resizes with the bicubic kernel, augments
  with augment_name -- None, 'autoaug' (AutoAugment v0) or 'randaug' (ra_num_layers, ra_magnitude), drawn from the generator
  behind 'randaug_rng_state' -- and normalises with (x - MEAN_RGB) / STDDEV_RGB; test_step is the padded centre crop."""

  def __init__(self, model_name='efficientnetv2-s', model_config=None, name=None, weight_decay=0.0, optimizer='rmsprop',
               learning_rate=0.016, label_smoothing=0.0, ema_decay=None, momentum=0.9, use_graph=True, check_device_labels=False,
               mixup_alpha=0.0, cutmix_alpha=0.0, augname=None, ra_num_layers=2, ra_magnitude=15, image_size=None,
               eval_image_size=None, transformations='crop|flip', lion_beta2=LION_BETA2, lion_wd=LION_WD, preprocessing=None,
               augment_name=None, **kwargs):
    super().__init__(model_name=model_name, model_config=model_config, include_top=True, name=name or model_name, **kwargs)
    optimizer = str(optimizer).lower()
    if optimizer not in OPTIMIZERS:
      raise ValueError('Unknown optimizer: %s (build_tf2_optimizer has %s)' % (optimizer, ', '.join(OPTIMIZERS)))
    if self._mconfig.conv_dropout:
      raise ValueError('conv_dropout=%r is not built (None in every named model)' % (self._mconfig.conv_dropout,))
    if not self.spec.num_classes:
      raise ValueError('a classifier needs num_classes > 0')
    if not 0.0 <= float(self._mconfig.dropout_rate or 0.0) < 1.0:
      raise ValueError('dropout_rate %r outside [0, 1)' % (self._mconfig.dropout_rate,))
    self.weight_decay = float(weight_decay)
    self.optimizer = optimizer
    self.momentum = 0.0 if optimizer == 'sgd' else float(momentum)
    self.update = build_update(optimizer, self.momentum, lion_beta2, lion_wd)      # what every executor of this model is built with
    self.learning_rate = learning_rate
    self.label_smoothing = float(label_smoothing)
    self.ema_decay = None if not ema_decay else float(ema_decay)
    self.use_graph = bool(use_graph)
    self.check_device_labels = bool(check_device_labels)
    self.iterations = 0
    self._graph = None
    self._pending_state = None
    self.mixup_alpha = self.cutmix_alpha = 0.0
    self._mix_rng = mix_rng(self._seed)
    self.set_mix_alphas(mixup_alpha, cutmix_alpha)
    self.augname = None if augname is None else autoaugment.check_aug_name(augname)
    self.ra_num_layers = int(ra_num_layers)
    if self.ra_num_layers < 0:
      raise ValueError('ra_num_layers %r must be >= 0' % (ra_num_layers,))
    self.ra_magnitude = autoaugment.check_magnitude(ra_magnitude)
    self._ra_rng = autoaugment.randaug_rng(self._seed)
    self._ra_forced = None
    self.image_size = None if image_size is None else self._check_size(image_size)
    self.eval_image_size = None if eval_image_size is None else self._check_size(eval_image_size)
    self.transformations = 'crop|flip' if transformations is None else str(transformations)
    self._crop_rng = v2_preprocessing.crop_rng(self._seed)
    self._crop_forced = None
    if preprocessing not in (None, 'legacy'):
      raise ValueError("preprocessing %r: None or 'legacy'" % (preprocessing,))
    self.preprocessing = preprocessing
    self.augment_name = preprocess_legacy.check_augment_name(augment_name)
    if preprocessing is None and self.augment_name is not None:
      raise ValueError("augment_name=%r belongs to preprocessing='legacy'; the EfficientNetV2 pipeline's RandAugment is "
                       "augname='randaug'" % (augment_name,))
    if preprocessing == 'legacy':
      if self.image_size is None:
        raise ValueError("preprocessing='legacy' needs image_size: the legacy path starts from decoded canvases "
                         '(preprocess_legacy.py:88-127)')
      if self.augname is not None:
        raise ValueError("preprocessing='legacy' needs augname=None, got %r: the legacy pipeline's augmentation is the "
                         "keyword augment_name (None, 'autoaug' or 'randaug')" % (augname,))
      if self.transformations not in ('crop|flip', 'flip'):
        raise ValueError("preprocessing='legacy' takes transformations 'crop|flip' or 'flip' (windows already cut by the "
                         'reader), got %r' % (self.transformations,))
    # fit / evaluate: float32 [4] device sums of cls_sums over the steps, by name
    self._sums_acc = {}
    self.fit_input = None        # the iterator fit is reading from (ModelCheckpoint saves its state)
    self.stop_training = False

  @staticmethod
  def _check_size(size):
    if int(size) != size or int(size) < 1:
      raise ValueError('image size %r must be a positive integer' % (size,))
    return int(size)

  def set_image_size(self, size):
    """A new training size from the next step on (the reference trains each progressive stage at its own size,
    main_tf2.py:265-284).  The next step builds a new executor for it on the same variable arena and runs eager, the one
    after it is captured again; optimizer slots, EMA shadows, the iteration count and every generator carry over."""
    if self.image_size is None:
      raise ValueError('set_image_size on a model built without image_size')
    self.image_size = self._check_size(size)
    self._graph = None

  def set_stage(self, stage):
    """One entry of progressive_stages: its image size, its RandAugment magnitude (when augname is set) and its mixup /
    cutmix alphas, from the next step on."""
    self.set_image_size(stage['image_size'])
    if self._has_magnitude:
      self.set_randaug(stage['ra_magnitude'])
    self.set_mix_alphas(stage['mixup_alpha'], stage['cutmix_alpha'])

  @property
  def _augments(self):
    """The step augments uint8 images on the device: augname (the V2 pipeline) or augment_name (the legacy one)."""
    return self.augname is not None or self.augment_name is not None

  @property
  def _has_magnitude(self):
    """A RandAugment magnitude is part of the step (AutoAugment's levels are its table's own)."""
    return self.augname is not None or self.augment_name == 'randaug'

  @property
  def legacy(self):
    return self.preprocessing == 'legacy'

  def force_crop_rows(self, rows):
    """Use these rows (v2_preprocessing.train_rows' int32 [batch, 8]) for every following train_step instead of drawing;
    None = draw again.  For tests and debugging."""
    self._crop_forced = rows

  def set_randaug(self, magnitude):
    """A new RandAugment magnitude from the next step on (the reference ramps it per progressive-training stage,
    main_tf2.py:262-275); a float in [0, 20].  Only the argument buffers change: the captured step is kept."""
    if not self._has_magnitude:
      raise ValueError("set_randaug on a model built without augname (or, with preprocessing='legacy', without "
                       "augment_name='randaug')")
    self.ra_magnitude = autoaugment.check_magnitude(magnitude)

  def force_randaug_draws(self, draws):
    """Use these draws (autoaugment.randaug_draws' four arrays [ra_num_layers, batch]; with augment_name='autoaug'
    autoaugment.autoaug_draws' three) for every following step instead of drawing; None = draw again.  For tests and
    debugging."""
    self._ra_forced = draws

  def set_mix_alphas(self, mixup_alpha, cutmix_alpha):
    """New mixup / cutmix Beta parameters from the next step on (the reference ramps them per progressive-training stage,
    main_tf2.py:262-275); 0 = off.  The captured step is dropped when the split of the batch changes (mixing switched on or
    off, or one of the two parts appearing or disappearing): the next step runs eager and the one after it is captured again."""
    mixup_alpha, cutmix_alpha = float(mixup_alpha or 0.0), float(cutmix_alpha or 0.0)
    if mixup_alpha < 0 or cutmix_alpha < 0:
      raise ValueError('mixup_alpha %r / cutmix_alpha %r must be >= 0' % (mixup_alpha, cutmix_alpha))
    if mix_split(2, mixup_alpha, cutmix_alpha) != mix_split(2, self.mixup_alpha, self.cutmix_alpha):
      self._graph = None
    self.mixup_alpha, self.cutmix_alpha = mixup_alpha, cutmix_alpha

  @property
  def mixing(self):
    return bool(self.mixup_alpha or self.cutmix_alpha)

  # ---- plumbing ------------------------------------------------------------------------------------------------------
  def _ensure_engine(self, batch, height, width):
    old = self.engine
    eng = super()._ensure_engine(batch, height, width)
    if self.image_size is not None and old is not None and eng is not old:
      # a new size is a stage of one run (set_image_size; test_step at eval_image_size): the dropout / stochastic-depth
      # generator goes on where the previous executor's stopped
      eng._rng.set_state(old._rng.get_state())
    eng.head_dropout = float(self._mconfig.dropout_rate or 0.0)
    if self.optimizer in ('rmsprop', 'adam'):
      eng.arena.use_second_slot('rms' if self.optimizer == 'rmsprop' else 'adam_v')
    if self._pending_state is not None:
      state, self._pending_state = self._pending_state, None
      self._apply_state(eng, state)
    return eng

  def _lr(self):
    lr = self.learning_rate
    return float(lr(self.iterations)) if callable(lr) else float(lr)

  @staticmethod
  def _split(data):
    """(images, labels), ((raw, sizes), labels) or the reference's ({'image': ..., ['size': ...]}, {'label': ...})
    -> (images, sizes or None, labels)."""
    images, labels = data
    sizes = None
    if isinstance(images, dict):
      sizes, images, labels = images.get('size'), images['image'], labels['label']
    elif isinstance(images, (tuple, list)):
      images, sizes = images
    if isinstance(images, np.ndarray):
      images = torch.from_numpy(images)
    return images, sizes, labels

  @staticmethod
  def _raw_sizes(sizes, raw):
    """(height, width) of every image on its canvas, int [batch, 2]; None = every image fills the canvas."""
    b, hc, wc = int(raw.shape[0]), int(raw.shape[1]), int(raw.shape[2])
    if sizes is None:
      return np.tile(np.array([hc, wc], np.int32), (b, 1))
    s = np.asarray(sizes.cpu() if isinstance(sizes, torch.Tensor) else sizes)
    if s.shape != (b, 2) or (s < 1).any() or (s[:, 0] > hc).any() or (s[:, 1] > wc).any():
      raise ValueError('sizes must be [batch, 2] = (height, width) inside the %d x %d canvas, got %s' % (hc, wc, s.tolist()))
    return s.astype(np.int32)

  def _prepare(self, data, mixing=False, augment=False, crop_size=None):
    """(images, labels) -> (executor, device images, device labels).
    Labels: integer class ids [batch] -> int32, or float [batch, num_classes] (one-hot or already mixed rows, used as they
    are) -> float32.  mixing: the step will mix this batch on the device -- integer labels only.  augment: the step will
    RandAugment this batch -- uint8 images only; with augname set uint8 images stay uint8 (the engine normalises them).
    crop_size: the step will crop and resize this batch to that size on the device -- uint8 images on a canvas of any
    size, which stay as they are; the executor is the one for (crop_size, crop_size)."""
    images, labels = data
    if images.dim() != 4 or images.shape[-1] != 3:
      raise ValueError('images must be [batch, height, width, 3], got %s' % (tuple(images.shape),))
    if crop_size is not None and images.dtype != torch.uint8:
      raise ValueError('image_size=%r: the step takes the decoded uint8 images [batch, canvas_h, canvas_w, 3] that the '
                       'reference crops, resizes and flips itself (preprocessing.py:22-55), got %s' % (self.image_size, images.dtype))
    if augment and images.dtype != torch.uint8:
      raise ValueError('augname=%r: train_step takes uint8 images [batch, height, width, 3] (what the reference hands '
                       'distort_image, preprocessing.py:49-50,107-111), got %s' % (self.augname, images.dtype))
    labels = torch.as_tensor(labels)
    soft = labels.is_floating_point()
    if soft:
      if labels.dim() != 2 or tuple(labels.shape) != (images.shape[0], self.spec.num_classes):
        raise ValueError('float labels must be [batch, num_classes] = [%d, %d], got %s' % (
            images.shape[0], self.spec.num_classes, tuple(labels.shape)))
      if mixing:
        raise ValueError('mixup / cutmix on the device take sparse integer labels [batch]; float labels are used as they '
                         'are: mix them in the input pipeline and set both alphas to 0')
    else:
      if labels.dim() != 1 or labels.numel() != images.shape[0]:
        raise ValueError('labels must be integer class ids [batch] or float [batch, num_classes], got %s' % (tuple(labels.shape),))
      if labels.device.type == 'cpu' or self.check_device_labels:
        # (labels already on the device are the caller's promise unless check_device_labels: the check waits for the device)
        if int(labels.min()) < 0 or int(labels.max()) >= self.spec.num_classes:
          raise ValueError('labels outside [0, %d)' % self.spec.num_classes)
    if crop_size is not None:
      eng = self._ensure_engine(int(images.shape[0]), crop_size, crop_size)
    else:
      eng = self._ensure_engine(int(images.shape[0]), int(images.shape[1]), int(images.shape[2]))
    if crop_size is not None or (self.augname is not None and images.dtype == torch.uint8):
      dev_images = images.to(device=eng.device).contiguous()
    else:
      dev_images = images.to(device=eng.device, dtype=eng.tdtype).contiguous()
    if crop_size is None and mixing and not self.use_graph and dev_images.data_ptr() == images.data_ptr():
      dev_images = dev_images.clone()      # the eager step mixes in place: never in the caller's own tensor
    return eng, dev_images, labels.to(device=eng.device, dtype=torch.float32 if soft else torch.int32).contiguous()

  def _metrics(self, eng, lr=None):
    out = metrics_from_sums(eng.cls_sums.detach().cpu().numpy(), 1, eng.batch, np.float64)
    if lr is not None:
      out['gradient_norm'] = float(eng.gnorm.item())
      out['learning_rate'] = lr
    return out

  # ---- the step ------------------------------------------------------------------------------------------------------
  def _step_body(self, eng, images, labels):
    if self.legacy:
      # decoded uint8 canvases -> the training size by the bicubic kernel: uint8 for the augmentation, else normalised
      norm = preprocess_legacy.NORM
      images = eng.crop_batch(images, to_u8=self._augments, method='bicubic', norm=None if self._augments else norm)
      if self._augments:
        images = eng.randaug_batch(images, norm=norm)
    elif self.image_size is not None:
      # decoded uint8 canvases -> the training size: uint8 for RandAugment, else the normalised network input
      images = eng.crop_batch(images, to_u8=self.augname is not None)
    if self.augname is not None:
      images = eng.randaug_batch(images)      # uint8 -> the engine's own normalised buffer (mixed in place below)
    if self.mixing:
      labels = eng.mix_batch(images, labels)      # the first launches of the step; images in place
    eng.forward(images, training=True)
    eng.softmax_loss(labels, self.label_smoothing)
    eng.backward()
    eng.optimizer_local(False, weight_decay=self.weight_decay, clip=0.0, l2_sum=eng.cls_sums[3:])
    eng.optimizer_apply(self.ema_decay is not None, False)

  def _graph_step(self, eng, images, labels):
    g = self._graph
    if g is None or g['engine'] is not eng or g['labels'].dtype != labels.dtype or g['labels'].shape != labels.shape or \
        g['images'].shape != images.shape:      # (a new canvas shape, with image_size set: captured again)
      g = self._graph = {'engine': eng, 'steps': 0, 'graph': None, 'images': torch.empty_like(images),
                         'labels': torch.empty_like(labels)}
    # (refilled every step: the in-place mixing of a step never sees an already mixed buffer)
    if images.data_ptr() != g['images'].data_ptr():
      g['images'].copy_(images, non_blocking=True)
    if labels.data_ptr() != g['labels'].data_ptr():
      g['labels'].copy_(labels, non_blocking=True)
    if g['steps'] == 0:
      # first step eager: allocates every buffer (the masks among them) and runs the one-time kernel attribute setup
      self._step_body(eng, g['images'], g['labels'])
    else:
      if g['graph'] is None:
        torch.cuda.synchronize()
        g['graph'] = capture_graph(eng.arena, lambda: self._step_body(eng, g['images'], g['labels']))
      g['graph'].replay()
      eng.arena.count_step()
    g['steps'] += 1

  def input_buffers(self):
    """(images, labels) static device buffers of the captured step (None before the first graph step).  A caller that
    fills them directly (and passes them to train_step) skips the copy; with mixup / cutmix on, the step then mixes the
    caller's own image buffer in place, so it has to be refilled before every step."""
    g = self._graph
    return (g['images'], g['labels']) if g else None

  def train_step(self, data, sync_loss=True):
    """data = (images [B,H,W,3], labels int [B] or float [B,C]) -> {'loss', 'reg_l2_loss', 'acc_top1', 'acc_top5',
    'gradient_norm', 'learning_rate'} of this step's batch (main_tf2.py:89-103; sync_loss=False skips the read-back).
    With a non-zero mixup_alpha / cutmix_alpha the batch is mixed on the device first (integer labels only), and the loss
    and the metrics are those of the mixed batch, as in the reference, whose trainer only ever sees the mixed one.
    Labels outside [0, num_classes) raise before anything is launched when they arrive on the host.  Labels that are
    already DEVICE tensors are not looked at (that would synchronise every step) unless the model was built with
    check_device_labels=True: an out-of-range device label is then the caller's error, and the kernel -- which reads
    nothing out of bounds for it -- returns a finite loss for a row without a hot class, with no signal."""
    images, sizes, labels = self._split(data)
    eng, images, labels = self._prepare((images, labels), mixing=self.mixing,
                                        augment=self.augname is not None and self.image_size is None, crop_size=self.image_size)
    if self.image_size is not None:
      sizes = self._raw_sizes(sizes, images)      # (checked before any generator moves)
    lr = self._lr()
    eng.set_hyper(lr, self.ema_decay)
    if eng.drop_masks or eng.dropout_mask is not None:
      eng.refresh_drop_masks()      # (an engine's first step draws its masks where it creates them)
    if self.mixing:
      h, w = eng.image_size
      weights, boxes = draw_mix(self._mix_rng, eng.batch, h, w, self.mixup_alpha, self.cutmix_alpha)
      eng.set_mix_draws(weights, boxes, mix_split(eng.batch, self.mixup_alpha, self.cutmix_alpha))
    if self.augment_name == 'autoaug':
      h, w = eng.image_size
      draws = self._ra_forced
      if draws is None:
        draws = autoaugment.autoaug_draws(self._ra_rng, eng.batch, 'v0')
      eng.set_randaug_draws(*autoaugment.autoaug_args(draws, h, w, 'v0'))
    elif self._augments:
      h, w = eng.image_size
      draws = self._ra_forced
      if draws is None:
        draws = autoaugment.randaug_draws(self._ra_rng, eng.batch, self.ra_num_layers)
      eng.set_randaug_draws(*autoaugment.randaug_args(draws, self.ra_magnitude, h, w))
    if self.image_size is not None:
      rows = self._crop_forced
      if rows is None and self.legacy:
        rows = (preprocess_legacy.legacy_flip_rows(self._crop_rng, sizes) if self.transformations == 'flip' else
                preprocess_legacy.legacy_train_rows(self._crop_rng, sizes, self.image_size))
      elif rows is None:
        rows = v2_preprocessing.train_rows(self._crop_rng, sizes, self.transformations)
      eng.set_crop_rows(rows)
    if self.use_graph:
      self._graph_step(eng, images, labels)
    else:
      self._step_body(eng, images, labels)
    self.iterations += 1
    if not sync_loss:
      return {'learning_rate': lr}
    return self._metrics(eng, lr)

  def test_step(self, data, sync_loss=True):
    """forward(training=False) + loss + metrics, no update (main_tf2.py:105-117; sync_loss=False skips the read-back and
    returns {}).  Never mixes and never augments; both
    label kinds; with augname set, uint8 images are normalised (x - 128) / 128 on the way in.  With image_size set, uint8
    images are decoded images on a canvas (train_step's input): preprocess_for_eval's centre crop and resize to
    eval_image_size or image_size (v2_preprocessing.eval_rows), never flipped, then normalised."""
    images, sizes, labels = self._split(data)
    size = None
    if self.image_size is not None and images.dtype == torch.uint8:
      size = self.eval_image_size or self.image_size
    eng, images, labels = self._prepare((images, labels), crop_size=size)
    if size is not None and self.legacy:
      eng.set_crop_rows(preprocess_legacy.legacy_eval_rows(self._raw_sizes(sizes, images), size))
      images = eng.crop_batch(images, to_u8=False, method='bicubic', norm=preprocess_legacy.NORM)
    elif size is not None:
      eng.set_crop_rows(v2_preprocessing.eval_rows(self._raw_sizes(sizes, images), size))
      images = eng.crop_batch(images, to_u8=False)
    elif images.dtype == torch.uint8:
      images = eng.randaug_batch(images, augment=False)
    eng.forward(images, training=False)
    eng.softmax_loss(labels, self.label_smoothing)
    # the compiled loss's regularisation term; the gradient arena of the last train_step stays as it is
    eng.l2_loss_eval(self.weight_decay)
    return self._metrics(eng) if sync_loss else {}

  # ---- state ---------------------------------------------------------------------------------------------------------
  def get_optimizer_state(self):
    """Optimizer slots ('velocity' = the momentum slot, 'rms' = RMSprop's mean square or 'adam_v'), EMA shadows, the
    iteration count (it drives the learning-rate schedule) and the states of the two generators -- 'rng_state' behind the
    dropout and stochastic-depth draws, 'mix_rng_state' behind the mixup / cutmix draws and, only when augname is set,
    'randaug_rng_state' behind the RandAugment draws and, only when image_size is set, 'crop_rng_state' behind the crop and
    flip draws -- so that a resumed run continues the uninterrupted one bit for bit."""
    if self.engine is None:
      raise RuntimeError('the network has not been built yet (call it once)')
    state = self.engine.arena.get_optimizer_state()
    state['iterations'] = self.iterations
    state['rng_state'] = self.engine._rng.get_state().cpu().numpy().copy()
    state['mix_rng_state'] = _pack_rng_state(self._mix_rng)
    if self._augments:
      state['randaug_rng_state'] = _pack_rng_state(self._ra_rng)
    if self.image_size is not None:
      state['crop_rng_state'] = _pack_rng_state(self._crop_rng)
    return state

  def set_optimizer_state(self, state):
    if self.engine is None:
      self._pending_state = dict(state)      # applied when the first executor is built
      self.iterations = int(state['iterations'])
      return
    self._apply_state(self.engine, state)

  def _apply_state(self, eng, state):
    eng.arena.set_optimizer_state(state)
    self.iterations = int(state['iterations'])
    if 'rng_state' in state:
      eng._rng.set_state(torch.as_tensor(state['rng_state'], dtype=torch.uint8))
    if 'mix_rng_state' in state:
      _unpack_rng_state(self._mix_rng, state['mix_rng_state'])
    if self._augments and 'randaug_rng_state' in state:
      _unpack_rng_state(self._ra_rng, state['randaug_rng_state'])
    if self.image_size is not None and 'crop_rng_state' in state:
      _unpack_rng_state(self._crop_rng, state['crop_rng_state'])

  # ---- fit / evaluate: the loop of tf.keras.Model.fit as main_tf2.py:235-295 calls it -----------------------------------
  def current_stage(self):
    """What set_stage sets, as the model has it now: image_size, ra_magnitude, mixup_alpha, cutmix_alpha."""
    return {'image_size': self.image_size, 'ra_magnitude': float(self.ra_magnitude), 'mixup_alpha': self.mixup_alpha,
            'cutmix_alpha': self.cutmix_alpha}

  def _in_stage(self, stage):
    keys = ('image_size', 'mixup_alpha', 'cutmix_alpha') + (('ra_magnitude',) if self._has_magnitude else ())
    mine = self.current_stage()
    return all(float(stage[k]) == float(mine[k]) for k in keys)

  def _accumulate(self, name, first):
    """acc[name] (+)= the last step's cls_sums, on the step's stream: ONE in-place add, in step order.  first: the
    accumulator starts at zero.  Nothing is read."""
    sums = self.engine.cls_sums
    acc = self._sums_acc.get(name)
    if acc is None or acc.device != sums.device:
      acc = self._sums_acc[name] = torch.zeros(4, dtype=torch.float32, device=sums.device)
    if first:
      acc.zero_()
    acc.add_(sums)
    return acc

  def _epoch_metrics(self, acc, steps, batch, prefix=''):
    """The one place fit and evaluate read values from the device (it waits for the stream)."""
    return metrics_from_sums(acc.detach().cpu().numpy(), steps, batch, np.float32, prefix)

  def evaluate(self, x, steps=None):
    """tf.keras.Model.evaluate over test_step: x = an iterable of test_step's batches -> {'loss', 'reg_l2_loss', 'acc_top1',
    'acc_top5'} over `steps` batches (all of them for None): cls_sums added up on the device in step order, float32, and read
    ONCE, at the end (metrics_from_sums).  Like test_step it moves nothing of the training state."""
    acc, n, batch = None, 0, None
    for data in x:
      if steps is not None and n >= steps:
        break
      self.test_step(data, sync_loss=False)
      if batch is None:
        batch = self.engine.batch
      elif batch != self.engine.batch:
        raise ValueError('evaluate: a batch of %d after batches of %d (the metrics are means over equal batches)' % (self.engine.batch, batch))
      acc = self._accumulate('evaluate', n == 0)
      n += 1
    if not n:
      raise ValueError('evaluate: the data holds no batch')
    return self._epoch_metrics(acc, n, batch)

  def fit(self, x, epochs=1, steps_per_epoch=None, initial_epoch=0, callbacks=None, validation_data=None, validation_steps=None,
          verbose=1, stages=None):
    """tf.keras.Model.fit for the classifier.  x: an iterator of train_step's batches, as effnetv2_datasets.ImageNetInput(...)(
    batch_size, canvas=...) yields them; every batch goes to train_step(batch, sync_loss=False).  An epoch is steps_per_epoch
    batches, or the iterator's end for None; the iterator is NOT restarted between epochs (the reader repeats on its own), and
    fit ends early when it runs dry.  -> train_lib.History.

    stages: a list as progressive_stages returns it.  At the start of every epoch the stage whose [start_epoch, end_epoch)
    holds the epoch is applied through set_stage, when it differs from what the model has (current_stage) -- one fit and one
    reader for the whole staged run, where the reference calls fit once per stage (main_tf2.py:256-284); an initial_epoch
    inside a stage picks that stage.

    The loop does not wait for the device per step.  After a step its cls_sums are added, on the step's stream, into a
    float32 device accumulator; the epoch's logs are metrics_from_sums of it, plus learning_rate of the last step.  The waits
    are the reader's arena event, the one read at the end of an epoch, a batch-level callback that ACCESSES a device value of
    its logs (train_lib.LazyLogs: the running values of the epoch), and a checkpoint.  With mixing on, the metrics are those
    of the mixed batch, as in train_step.

    validation_data: an iterable of test_step's batches that can be iterated once per epoch (a list, or
    train_lib.RepeatableReader(reader)); every epoch ends with evaluate(validation_data, steps=validation_steps), whose
    values enter the logs under 'val_' + name.  callbacks: train_lib.fit's protocol -- objects with any of set_model,
    on_train_begin, on_train_end(logs), on_epoch_begin(epoch, logs), on_epoch_end(epoch, logs), on_train_batch_end(step,
    logs); a callback that sets model.stop_training ends the run after the epoch."""
    callbacks = list(callbacks or [])

    def call(name, *args):
      for cb in callbacks:
        fn = getattr(cb, name, None)
        if fn is not None:
          fn(*args)
    batch_level = [cb.on_train_batch_end for cb in callbacks if getattr(cb, 'on_train_batch_end', None) is not None]
    history = train_lib.History()
    self.fit_input, self.stop_training = x, False
    it = iter(x)
    call('set_model', self)
    call('on_train_begin', None)
    logs = {}
    for epoch in range(int(initial_epoch), int(epochs)):
      if stages:
        stage = stage_of_epoch(stages, epoch)
        if stage is not None and not self._in_stage(stage):
          self.set_stage(stage)
      call('on_epoch_begin', epoch, None)
      acc, steps, lr, batch = None, 0, None, None
      while steps_per_epoch is None or steps < steps_per_epoch:
        try:
          data = next(it)
        except StopIteration:
          break
        lr = self.train_step(data, sync_loss=False)['learning_rate']
        if batch is None:
          batch = self.engine.batch
        elif batch != self.engine.batch:
          raise ValueError('fit: a batch of %d after batches of %d (the metrics are means over equal batches)' % (self.engine.batch, batch))
        acc = self._accumulate('fit', steps == 0)
        steps += 1
        if batch_level:
          blogs = train_lib.LazyLogs({'learning_rate': lr, 'step': self.iterations}, METRIC_KEYS,
                                     lambda acc=acc, steps=steps, batch=batch: self._epoch_metrics(acc, steps, batch))
          for fn in batch_level:
            fn(steps - 1, blogs)
      if not steps:
        break      # the data ran dry at an epoch's border
      logs = self._epoch_metrics(acc, steps, batch)
      logs['learning_rate'] = lr
      if validation_data is not None:
        logs.update({'val_' + k: v for k, v in self.evaluate(validation_data, steps=validation_steps or None).items()})
      call('on_epoch_end', epoch, logs)
      history.append(epoch, logs)
      if verbose:
        print('Epoch %d/%d: %d steps - %s' % (epoch + 1, epochs, steps, ' - '.join(
            '%s: %.4g' % (k, v) for k, v in logs.items() if isinstance(v, (int, float)))), flush=True)
      if self.stop_training or (steps_per_epoch is not None and steps < steps_per_epoch):
        break
    call('on_train_end', logs)
    return history


# ---- the training-state file: everything a next step reads that util_keras.save_ckpt does not hold ---------------------------
_ARRAY_KEYS = ('velocity', 'ema', 'adam_v', 'rms', 'rng_state', 'mix_rng_state', 'randaug_rng_state', 'crop_rng_state')
TRAIN_STATE_KIND = 'effnetv2'


def _model_identity(model):
  return {'num_variables': len(util_keras.model_variables(model)), 'arena_length': train_lib.arena_length(model),
          'optimizer': model.optimizer}


def _lion_identity(model):
  """The two Lion scalars the state file carries besides the optimizer's name; None for the other optimizers."""
  return train_lib.lion_identity(model.update)


def save_train_state(model, path, reader=None):
  """Writes <ckpt prefix>.train_state.npz next to a checkpoint, in train_lib.save_train_state's conventions: get_optimizer_state()
  in full (both slots, the shadows, iterations, rng_state, mix_rng_state, randaug_rng_state, crop_rng_state), the model's
  current stage (image size, RandAugment magnitude, the two alphas) and reader.get_state() -- with the variables and the
  BatchNorm statistics of the checkpoint, everything the next step reads.  Arrays are npz members; everything else is ONE
  JSON member, 'meta' (uint8).  No pickle; written to a temporary name and renamed.  A model without an engine that holds a
  restored state writes that state.  Reading the slots waits for the device."""
  if model.engine is None and model._pending_state is not None:
    state = dict(model._pending_state)
  else:
    state = model.get_optimizer_state()
  arrays, meta = {}, {'format': train_lib.TRAIN_STATE_FORMAT, 'kind': TRAIN_STATE_KIND}
  meta.update(_model_identity(model))
  if _lion_identity(model) is not None:
    meta['lion'] = _lion_identity(model)
  for k, v in state.items():
    if k in _ARRAY_KEYS:
      arrays[k] = np.asarray(v)
    elif k == 'iterations':
      meta[k] = int(v)
    else:
      raise ValueError('save_train_state: the optimizer state has a key this file has no place for: %r' % (k,))
  meta['stage'] = model.current_stage()
  meta['reader'] = None if reader is None else reader.get_state()
  arrays['meta'] = np.frombuffer(json.dumps(meta).encode('utf-8'), np.uint8)
  tmp = path + '.tmp'
  with open(tmp, 'wb') as f:
    np.savez(f, **arrays)
  os.replace(tmp, path)
  return path


def restore_train_state(model, path, reader=None):
  """Puts a save_train_state file back into `model` (and the reader's part into `reader`).  A file from another model is
  refused with the difference named: the variable count, the arena length or the optimizer.  The stage goes in at once
  (set_image_size / set_randaug / set_mix_alphas, where the model has them); a model without an engine keeps the rest until
  its first engine is made, and model.iterations is set at once, so the caller can form initial_epoch from it.  -> the meta
  dict."""
  meta, arrays = train_lib.load_train_state(path)
  if meta.get('kind') != TRAIN_STATE_KIND:
    raise ValueError('%s is not a classifier training state (kind %r, this code reads %r)' % (path, meta.get('kind'), TRAIN_STATE_KIND))
  mine = _model_identity(model)
  what = {'num_variables': 'variables', 'arena_length': 'arena elements', 'optimizer': 'as optimizer'}
  diff = ['%s %s, this model %s' % (meta.get(k), what[k], mine[k]) for k in ('num_variables', 'arena_length', 'optimizer')
          if meta.get(k) != mine[k]]
  if not diff:
    diff = train_lib.lion_difference(meta.get('lion'), _lion_identity(model))
  if diff:
    raise ValueError('%s is the training state of another model: the file has %s' % (path, '; '.join(diff)))
  if reader is not None:
    if meta.get('reader') is None:
      raise ValueError('%s holds no reader state' % (path,))
    reader.set_state(meta['reader'])
  stage = meta.get('stage') or {}
  if model.image_size is not None and stage.get('image_size') is not None:
    model.set_image_size(stage['image_size'])
  if model._has_magnitude and 'ra_magnitude' in stage:
    model.set_randaug(stage['ra_magnitude'])
  if 'mixup_alpha' in stage:
    model.set_mix_alphas(stage['mixup_alpha'], stage['cutmix_alpha'])
  state = {k: arrays[k] for k in _ARRAY_KEYS if k in arrays}
  state['iterations'] = int(meta['iterations'])
  if model.engine is not None:
    train_lib.check_arena_length(state, model.engine.arena)
  model.set_optimizer_state(state)
  return meta


class ModelCheckpoint(train_lib.ModelCheckpoint):
  """train_lib.ModelCheckpoint for this trainer: the same callback (save_freq 'epoch' or a number of batches), whose file is
  util_keras.save_ckpt(model, filepath.format(epoch=epoch + 1), ema=bool(model.ema_decay), global_step=model.iterations) with
  this module's training-state file next to it.  Saving waits for the device."""

  def save(self, epoch):
    model = self.model
    prefix = self.filepath.format(epoch=epoch + 1)
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    util_keras.save_ckpt(model, prefix, ema=bool(model.ema_decay), global_step=model.iterations)
    reader = model.fit_input if hasattr(model.fit_input, 'get_state') else None
    save_train_state(model, train_lib.train_state_path(prefix), reader)
    if self.verbose:
      print('Epoch %d: saving model to %s' % (epoch + 1, prefix), flush=True)
    return prefix
