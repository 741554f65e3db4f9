"""The classifier's training entry point on MI355X (mirror of efficientnetv2/main_tf2.py:120-307):
``python -m automl_amd.effnetv2_main`` or ``main(argv)``.

  python -m automl_amd.effnetv2_main --mode=traineval --model_name=efficientnetv2-s --dataset_cfg=imagenet \
      --data_dir=/data/imagenet --model_dir=/tmp/v2s --hparam_str=train.batch_size=256 --canvas=512x512

The flags of efficientnetv2/cflags.py that mean something here keep their names: ``--model_name``, ``--dataset_cfg``,
``--hparam_str``, ``--data_dir``, ``--model_dir``, ``--mode``.  ``--canvas=HxW`` (the slot the reader's JPEG decoder writes
every image into), ``--jpeg_max_ratio`` (1, 2, 4 or 8: an image larger than the canvas is decoded at the smallest
tf.io.decode_jpeg ratio that fits it; default 1, full size only), ``--decode_crop`` (the training crop is drawn in the reader and only that window of each JPEG is
decoded; the model then only flips), ``--legacy_input`` (the reference's preprocess_legacy.py in front of the network, for the
recipes whose data.augname starts with ``effnetv1_``: efficientnetv2-b0 .. b3, efficientnet-b0 .. b7), ``--dtype`` (default: bf16 with runtime.mixed_precision, else f32) and ``--seed`` (the model's, its input
draws' and the reader's) are this project's own.

The configuration is assembled as :121-125 does: ``base_config()`` -- hparams.base_config's train / eval / data / runtime
sections restated, with its model section from effnetv2_configs -- overridden by effnetv2_configs.get_model_config, by
effnetv2_datasets.get_dataset_config and by ``--hparam_str``, in that order; model.num_classes = data.num_classes; saved as
``config.yaml`` in model_dir.  data.splits.<split>.num_images can be overridden through ``--hparam_str``, so a small data set
can be described.  From the configuration to the model as :154-207: train_size from a fraction (isize <= 16),
steps_per_epoch = num_train_images // batch_size, lr_base and lr_min scaled by batch_size / 256, WarmupLearningRateSchedule,
label_smoothing, weight_decay, optimizer, data.augname / ra_num_layers / ram / mixup_alpha / cutmix_alpha.  As in the
reference's TF2 trainer, train.ema_decay is not used (its TrainableModel keeps no shadows).

Modes.  ``train``: TrainableModel.fit, staged by train.stages (one fit over one reader, stage_list).  ``traineval``: unstaged,
with validation every epoch, validation_steps = num_eval_images // eval.batch_size.  ``eval``: one evaluate over the latest
checkpoint of model_dir, printing the four values; the reference's checkpoints_iterator polling loop is not built.  Starting
``train`` / ``traineval`` in a model_dir that holds a checkpoint continues from it -- the weights through
util_keras.restore_ckpt, the training state (optimizer slots, generators, stage, reader position) through
effnetv2_train.restore_train_state, initial_epoch = iterations // steps_per_epoch -- which is the job ReuableBackupAndRestore
has in the reference.  train.ft_init_ckpt restores a checkpoint without the classification layer's kernel and bias.

Refused with a reason, before a model or a reader exists: runtime.strategy 'tpu' / 'gpus' (absent or None means one device;
base_config() restates it as None where the reference's default is 'tpu', which would refuse every run), ``--tpu*``,
``--use_tpu=true``, ``--export_to_tpu``, ``--sweeps``, a dataset configuration that is not built, an augname that
TrainableModel refuses.  TensorBoard is left out.

``--legacy_input``: a data.augname that starts with ``effnetv1_`` is then accepted; its remainder is the legacy pipeline's
augment_name (``autoaug``, ``randaug``, or nothing for none) and the model is TrainableModel(preprocessing='legacy',
augment_name=..., augname=None); ``--decode_crop`` then asks the reader for the legacy window (decode_crop='legacy' with the
training size).  With the flag, an augname without the prefix is refused, and so is ``--decode_crop`` with a staged size
schedule (the reader's centre-crop fallback is made for one training size and cannot follow the stages).  Without the flag
everything is as before, the refusal of those names included.
"""
import argparse
import copy
import logging
import os
import sys

from automl_amd import autoaugment
from automl_amd import effnetv2_configs
from automl_amd import effnetv2_datasets
from automl_amd import hparams_config

Config = hparams_config.Config


def base_config():
  """hparams.base_config (hparams.py:221-312); runtime.strategy is None here (the module's docstring)."""
  split = dict(num_images=None, files=None, tfds_split=None, slice=None)
  return Config(dict(
      model=copy.deepcopy(effnetv2_configs.base_model_config),
      train=dict(stages=0, epochs=350, min_steps=0, optimizer='rmsprop', lr_sched='exponential', lr_base=0.016,
                 lr_decay_epoch=2.4, lr_decay_factor=0.97, lr_warmup_epoch=5, lr_min=0, ema_decay=0.9999, weight_decay=1e-5,
                 weight_decay_inc=0.0, weight_decay_exclude='.*(bias|gamma|beta).*', label_smoothing=0.1, gclip=0,
                 batch_size=4096, isize=None, split=None, loss_type=None, ft_init_ckpt=None, ft_init_ema=True, varsexp=None,
                 sched=None),
      eval=dict(batch_size=8, isize=None, split=None),
      data=dict(ds_name='imagenet', augname='randaug', ra_num_layers=2, ram=15, mixup_alpha=0., cutmix_alpha=0., ibase=128,
                cache=True, resize=None, data_dir=None, multiclass=None, num_classes=1000, tfds_name=None, try_gcs=False,
                tfds_split=None, splits=dict(train=dict(split), eval=dict(split), minival=dict(split), trainval=dict(split))),
      runtime=dict(iterations_per_loop=1000, skip_host_call=False, mixed_precision=True, use_async_checkpointing=False,
                   log_step_count_steps=64, keep_checkpoint_max=5, keep_checkpoint_every_n_hours=5, strategy=None)))


def _flag_bool(text):
  if text.lower() in ('true', 't', '1', 'yes'):
    return True
  if text.lower() in ('false', 'f', '0', 'no'):
    return False
  raise argparse.ArgumentTypeError('a boolean flag takes true or false, got %r' % (text,))


def _canvas(text):
  try:
    h, w = (int(v) for v in text.lower().split('x'))
  except ValueError:
    raise argparse.ArgumentTypeError('--canvas takes HxW, got %r' % (text,))
  if h < 1 or w < 1:
    raise argparse.ArgumentTypeError('--canvas takes HxW, got %r' % (text,))
  return (h, w)


def define_flags():
  """efficientnetv2/cflags.py as an argparse parser; a boolean flag is --name or --name=true|false."""
  ap = argparse.ArgumentParser(prog='python -m automl_amd.effnetv2_main', description='EfficientNetV2 training on MI355X')

  def boolean(name, text):
    ap.add_argument('--' + name, type=_flag_bool, nargs='?', const=True, default=False, help=text)
  ap.add_argument('--model_name', default='efficientnetv2-b0', help='model name.')
  ap.add_argument('--dataset_cfg', default='Imagenet', help='dataset config name.')
  ap.add_argument('--hparam_str', default='', help='Comma separated k=v pairs of hparams.')
  ap.add_argument('--sweeps', default='', help='refused: sweeping is not built')
  boolean('use_tpu', 'refused: there is no TPU path')
  ap.add_argument('--tpu_job_name', default=None, help='refused: there is no TPU path')
  ap.add_argument('--tpu', default=None, help='refused: there is no TPU path')
  ap.add_argument('--gcp_project', default=None, help='refused: there is no TPU path')
  ap.add_argument('--tpu_zone', default=None, help='refused: there is no TPU path')
  ap.add_argument('--data_dir', default=None, help='The directory of the TFRecord files.')
  ap.add_argument('--model_dir', default=None, help='Dir for checkpoints and config.yaml.')
  ap.add_argument('--mode', default='train', choices=['train', 'traineval', 'eval'], help='train, traineval or eval.')
  boolean('export_to_tpu', 'refused: there is no TPU path')
  ap.add_argument('--canvas', type=_canvas, default=(512, 512), help='HxW of the slot every decoded image is written into')
  ap.add_argument('--jpeg_max_ratio', type=int, default=1, choices=[1, 2, 4, 8],
                  help='the largest ratio (tf.io.decode_jpeg) the reader may decode an image at so that it fits --canvas; 1: '
                       'full size only, a larger image is refused; 8 is recommended for full-size ImageNet')
  ap.add_argument('--decode_crop', action='store_true',
                  help="draw the training crop in the reader and decode only that window of each JPEG "
                       "(tf.image.decode_and_crop_jpeg); the model is then built with transformations='flip'")
  ap.add_argument('--legacy_input', action='store_true',
                  help="the legacy EfficientNet input pipeline (preprocess_legacy.py: bicubic resize, AutoAugment v0, mean / "
                       "stddev) for a recipe whose data.augname starts with 'effnetv1_'")
  ap.add_argument('--dtype', default=None, choices=['bf16', 'f32'], help='storage dtype of the activations')
  ap.add_argument('--seed', type=int, default=0, help='seed of the model, its input draws and the reader')
  ap.add_argument('--lion_beta2', type=float, default=None, help='train.optimizer=lion: beta_2 (default 0.99)')
  ap.add_argument('--lion_wd', type=float, default=None,
                  help='train.optimizer=lion: the decoupled weight decay wd (default 0), on every variable')
  return ap


def parse_flags(argv):
  """argv (without the program name) -> the flags; what is not built is refused here, before a model or a reader exists."""
  flags = define_flags().parse_args(list(argv))
  refused = []
  for name in ('tpu', 'tpu_zone', 'gcp_project', 'tpu_job_name'):
    if getattr(flags, name):
      refused.append('--%s: there is no TPU path' % name)
  if flags.use_tpu:
    refused.append('--use_tpu=true: there is no TPU path')
  if flags.export_to_tpu:
    refused.append('--export_to_tpu: there is no TPU path and no metagraph export')
  if flags.sweeps:
    refused.append('--sweeps=%s: sweeping is not built; start one run per setting with --hparam_str' % flags.sweeps)
  if refused:
    raise ValueError('; '.join(refused))
  return flags


def build_config(flags):
  """main_tf2.py:121-126, and the refusals that depend on the configuration."""
  config = base_config()
  config.override(effnetv2_configs.get_model_config(flags.model_name))
  config.override(effnetv2_datasets.get_dataset_config(flags.dataset_cfg))      # (a configuration that is not built raises)
  config.override(flags.hparam_str)
  config.model.num_classes = config.data.num_classes
  strategy = config.runtime.get('strategy', None)
  if strategy not in (None, '', 'None'):
    raise ValueError("runtime.strategy=%r is not built: classifier training is on one device ('tpu' has no counterpart and "
                     "'gpus' is data-parallel fit, which is not built); leave it out or set runtime.strategy=None" % (strategy,))
  effnetv2_datasets.get_dataset_class(config.data.ds_name)      # raises for a data set that is not built
  if getattr(flags, 'legacy_input', False):
    legacy_augment_name(config.data.augname)      # raises for a name without the prefix or with an unknown remainder
  elif config.data.augname is not None:
    try:
      autoaugment.check_aug_name(config.data.augname)
    except ValueError as e:
      raise ValueError("%s -- the efficientnetv2-b* and efficientnet-b* recipes name 'effnetv1_autoaug' and the fine-tuning "
                       "configuration 'ft'; override it with --hparam_str=data.augname=randaug, or data.augname=None for no "
                       "augmentation; or, for an 'effnetv1_*' recipe, run its own legacy input pipeline with --legacy_input" % (e,))
  if config.train.loss_type not in (None, 'softmax'):
    raise ValueError('train.loss_type=%r is not built: train_step has the softmax loss' % (config.train.loss_type,))
  return config


def legacy_augment_name(augname):
  """data.augname of a legacy recipe -> TrainableModel's augment_name: 'effnetv1_autoaug' -> 'autoaug', 'effnetv1_randaug' ->
  'randaug', 'effnetv1_' -> None (preprocessing.py:133-139 hands the remainder to preprocess_legacy)."""
  from automl_amd import preprocess_legacy
  name = str(augname)
  if augname is None or not name.startswith('effnetv1_'):
    raise ValueError("--legacy_input needs a data.augname that starts with 'effnetv1_' (the recipes of efficientnetv2-b0 .. b3 "
                     'and efficientnet-b0 .. b7), this run has %r; without the flag the EfficientNetV2 pipeline runs' % (augname,))
  return preprocess_legacy.check_augment_name(name[len('effnetv1_'):] or None)


def _plain(value):
  if isinstance(value, Config):
    value = value.as_dict()
  if isinstance(value, dict):
    return {k: _plain(v) for k, v in value.items()}
  if isinstance(value, (list, tuple)):
    return [_plain(v) for v in value]
  return value


def save_config(config, model_dir):
  """config.save_to_yaml(model_dir/config.yaml) (main_tf2.py:132-135), as plain data."""
  import yaml
  os.makedirs(model_dir, exist_ok=True)
  path = os.path.join(model_dir, 'config.yaml')
  with open(path, 'w') as f:
    yaml.safe_dump(_plain(config), f, default_flow_style=False)
  return path


def plan_of(config):
  """main_tf2.py:154-194, :256-275 -> the numbers of the run: splits, num_train_images, num_eval_images, train_size,
  eval_size, steps_per_epoch, total_steps, scaled_lr, scaled_lr_min, validation_steps, stages."""
  from automl_amd import effnetv2_train
  train, evalc, data = config.train, config.eval, config.data
  train_split, eval_split = train.split or 'train', evalc.split or 'eval'
  num_train_images = data.splits[train_split].num_images
  num_eval_images = data.splits[eval_split].num_images
  if not num_train_images or not num_eval_images:
    raise ValueError('data.splits.%s.num_images / data.splits.%s.num_images are not set' % (train_split, eval_split))
  train_size, eval_size = train.isize, evalc.isize
  if train_size is None or eval_size is None:
    raise ValueError('train.isize / eval.isize are not set')
  if train_size <= 16.:
    train_size = int(eval_size * train_size) // 16 * 16
  steps_per_epoch = num_train_images // train.batch_size
  if steps_per_epoch < 1:
    raise ValueError('data.splits.%s.num_images=%d holds no batch of train.batch_size=%d' % (train_split, num_train_images, train.batch_size))
  stages = effnetv2_train.stage_list(int(train_size), train.epochs, train.stages, bool(train.sched), data.ibase,
                                     15 if data.ram is None else data.ram, float(data.mixup_alpha or 0.0), float(data.cutmix_alpha or 0.0))
  return dict(train_split=train_split, eval_split=eval_split, num_train_images=num_train_images, num_eval_images=num_eval_images,
              train_size=int(train_size), eval_size=int(eval_size), steps_per_epoch=steps_per_epoch,
              total_steps=steps_per_epoch * train.epochs, scaled_lr=train.lr_base * (train.batch_size / 256.0),
              scaled_lr_min=train.lr_min * (train.batch_size / 256.0), validation_steps=num_eval_images // evalc.batch_size,
              stages=stages)


def build_model(flags, config, plan):
  from automl_amd import effnetv2_train
  train, data = config.train, config.data
  learning_rate = effnetv2_train.WarmupLearningRateSchedule(
      plan['scaled_lr'], steps_per_epoch=plan['steps_per_epoch'], decay_epochs=train.lr_decay_epoch,
      warmup_epochs=train.lr_warmup_epoch, decay_factor=train.lr_decay_factor, lr_decay_type=train.lr_sched,
      total_steps=plan['total_steps'], minimal_lr=plan['scaled_lr_min'])
  dtype = flags.dtype or ('bf16' if config.runtime.mixed_precision else 'f32')
  lion = {k: v for k, v in (('lion_beta2', getattr(flags, 'lion_beta2', None)), ('lion_wd', getattr(flags, 'lion_wd', None)))
          if v is not None}
  if lion and str(train.optimizer).lower() != 'lion':
    raise ValueError('--lion_beta2 / --lion_wd need train.optimizer=lion, this run has %r' % (train.optimizer,))
  # --decode_crop: the reader has cropped already (get_dataset), the step takes the whole "image" and draws the flip
  crop = {'transformations': 'flip'} if getattr(flags, 'decode_crop', False) else {}
  augname = data.augname
  if getattr(flags, 'legacy_input', False):
    crop.update(preprocessing='legacy', augment_name=legacy_augment_name(data.augname))
    augname = None
  return effnetv2_train.TrainableModel(
      config.model.model_name, config.model.as_dict(), weight_decay=train.weight_decay, optimizer=train.optimizer,
      learning_rate=learning_rate, label_smoothing=train.label_smoothing, dtype=dtype, seed=flags.seed,
      mixup_alpha=data.mixup_alpha, cutmix_alpha=data.cutmix_alpha, augname=augname,
      ra_num_layers=data.ra_num_layers, ra_magnitude=15 if data.ram is None else data.ram, image_size=plan['train_size'],
      eval_image_size=plan['eval_size'], **lion, **crop)


def get_dataset(flags, config, plan, is_training):
  """main_tf2.py:222-233 -> the reader of train_step's / test_step's batches."""
  split = plan['train_split'] if is_training else plan['eval_split']
  batch = config.train.batch_size if is_training else config.eval.batch_size
  ds = effnetv2_datasets.build_dataset_input(is_training, None, None, flags.data_dir, split, config.data, seed=flags.seed)
  crop = {'decode_crop': True} if is_training and getattr(flags, 'decode_crop', False) else {}
  if crop and getattr(flags, 'legacy_input', False):
    crop = {'decode_crop': 'legacy', 'crop_image_size': plan['train_size']}
  return ds(batch, canvas=flags.canvas, max_ratio=flags.jpeg_max_ratio, **crop)


class _WithoutHead(object):
  """The model as util_keras.restore_ckpt sees it, without the classification layer's kernel and bias (main_tf2.py:176-179:
  exclude_layers=('_fc', 'optimizer'))."""

  def __init__(self, model):
    import types
    self._model = model
    self.spec = types.SimpleNamespace(params=[p for p in model.spec.params if '/head/dense/' not in p.name])

  def set_weights(self, values):
    self._model.set_weights(values)


def main(argv=None):
  """-> fit's History (train, traineval) or the four values (eval).  Never replaces the process."""
  flags = parse_flags(sys.argv[1:] if argv is None else argv)
  if not flags.model_dir:
    raise ValueError('--model_dir is needed')
  config = build_config(flags)
  plan = plan_of(config)
  if flags.legacy_input and flags.decode_crop and flags.mode == 'train' and config.train.stages:
    raise ValueError('--legacy_input with --decode_crop and train.stages=%r: the reader draws the legacy window, whose centre-'
                     'crop fallback is made for ONE training size, and cannot follow a staged size schedule; drop --decode_crop '
                     'or set train.stages=0' % (config.train.stages,))
  from automl_amd import effnetv2_train, tf_checkpoint, train_lib, util_keras
  if 'train' in flags.mode:
    save_config(config, flags.model_dir)
  model = build_model(flags, config, plan)
  latest = tf_checkpoint.latest_checkpoint(flags.model_dir) if os.path.isdir(flags.model_dir) else None

  if flags.mode == 'eval':
    if latest is None:
      raise FileNotFoundError('no checkpoint found in directory %s' % flags.model_dir)
    util_keras.restore_ckpt(model, latest, ema_decay=0, skip_mismatch=False)
    val = get_dataset(flags, config, plan, False)
    try:
      results = model.evaluate(val, steps=plan['validation_steps'] or None)
    finally:
      val.close()
    print('eval results for %s: %s' % (latest, ' - '.join('%s: %.6g' % (k, results[k]) for k in effnetv2_train.METRIC_KEYS)), flush=True)
    return results

  train = get_dataset(flags, config, plan, True)
  val = None
  try:
    if latest is not None:
      util_keras.restore_ckpt(model, latest, ema_decay=0, skip_mismatch=False)
      state_file = train_lib.train_state_path(latest)
      if os.path.exists(state_file):
        effnetv2_train.restore_train_state(model, state_file, reader=train)
      else:
        logging.warning('%s has no training-state file: the weights are restored, the optimizer slots, the step count and '
                        'the reader start afresh', latest)
    elif config.train.ft_init_ckpt:
      util_keras.restore_ckpt(_WithoutHead(model), config.train.ft_init_ckpt, ema_decay=0, skip_mismatch=True)
    staged = flags.mode == 'train' and bool(config.train.stages)
    if flags.mode == 'traineval':
      val = train_lib.RepeatableReader(get_dataset(flags, config, plan, False))
    ckpt = effnetv2_train.ModelCheckpoint(os.path.join(flags.model_dir, 'ckpt-{epoch:d}'), verbose=1)
    return model.fit(train, epochs=config.train.epochs, steps_per_epoch=plan['steps_per_epoch'],
                     initial_epoch=model.iterations // plan['steps_per_epoch'], callbacks=[ckpt], validation_data=val,
                     validation_steps=plan['validation_steps'], stages=plan['stages'] if staged else None)
  finally:
    train.close()
    if val is not None:
      val.close()


if __name__ == '__main__':
  logging.basicConfig(level=logging.INFO)
  main()
