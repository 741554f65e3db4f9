"""The detector's training entry point on MI355X (mirror of efficientdet/tf2/train.py): ``python -m automl_amd.train`` or
``main(argv)``.

  python -m automl_amd.train --mode=traineval --model_name=efficientdet-d0 --model_dir=/tmp/d0 --batch_size=128 \
      --train_file_pattern='train-*.tfrecord' --val_file_pattern='val-*.tfrecord' --num_examples_per_epoch=118287

The flags of tf2/train.py:32-109 keep their names and defaults.  ``--canvas=HxW`` (the slot the reader's JPEG decoder writes
every image into, jpeg.JpegDecoder) and ``--dtype`` are this project's own.  The flow is main's (:153-290): the config from
the model name, ``--hparams`` and ``--num_epochs``; steps_per_epoch = num_examples_per_epoch // batch_size; config.yaml written
into model_dir once; the latest checkpoint of model_dir restored if there is one -- the weights through
util_keras.restore_ckpt and the training-state file next to it (train_lib.restore_train_state), the reader's position
included, so the run goes on as the uninterrupted one would -- else ``--pretrained_ckpt`` without its heads; initial_epoch =
iterations // steps_per_epoch; EfficientDetNetTrain.fit with train_lib.get_callbacks and, in ``traineval``, the validation
reader.  ``--mode=eval`` is one pass of COCOCallback over the latest checkpoint (the body of the loop at :293-319 without the
polling); it prints and returns the metrics.  ``--debug`` runs the steps eagerly and reads the files in order, as the
reference's debug mode does.

Refused with a reason before anything touches the device: ``--strategy`` other than empty, ``--tpu`` / ``--tpu_zone`` /
``--gcp_project``, ``--hub_module_url``, ``--use_xla``, ``--profile``, ``--steps_per_execution`` other than 1.
"""
import argparse
import logging
import os
import sys


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
  """tf2/train.py:32-109 as an argparse parser: the same names and defaults; a boolean flag is --name or --name=true|false."""
  ap = argparse.ArgumentParser(prog='python -m automl_amd.train', description='EfficientDet training on MI355X')

  def boolean(name, text):
    ap.add_argument('--' + name, type=_flag_bool, nargs='?', const=True, default=False, help=text)
  ap.add_argument('--tpu', default=None, help='refused: there is no TPU path')
  ap.add_argument('--gcp_project', default=None, help='refused: there is no TPU path')
  ap.add_argument('--tpu_zone', default=None, help='refused: there is no TPU path')
  ap.add_argument('--strategy', default='', help="refused unless empty: data-parallel fit is not built")
  boolean('use_fake_data', 'Use fake input.')
  boolean('use_xla', 'refused: there is no XLA here')
  ap.add_argument('--model_dir', default=None, help='Location of model_dir')
  ap.add_argument('--pretrained_ckpt', default=None, help='Start training from this EfficientDet checkpoint.')
  ap.add_argument('--hparams', default='', help='Comma separated k=v pairs of hyperparameters or a yaml file.')
  ap.add_argument('--batch_size', type=int, default=64, help='training batch size')
  ap.add_argument('--eval_samples', type=int, default=5000, help='The number of samples for evaluation.')
  ap.add_argument('--steps_per_execution', type=int, default=1, help='refused unless 1')
  ap.add_argument('--train_file_pattern', default=None, help='Glob for train data files')
  ap.add_argument('--val_file_pattern', default=None, help='Glob for evaluation tfrecords')
  ap.add_argument('--val_json_file', default=None,
                  help='COCO validation JSON containing golden bounding boxes. If None, use the ground truth from the dataloader.')
  ap.add_argument('--mode', default='traineval', choices=['train', 'traineval', 'eval'], help='job mode: train, traineval, eval.')
  ap.add_argument('--hub_module_url', default=None, help='refused: TF-Hub modules are not read')
  ap.add_argument('--num_examples_per_epoch', type=int, default=120000, help='Number of examples in one epoch')
  ap.add_argument('--num_epochs', type=int, default=None, help='Number of epochs for training')
  ap.add_argument('--model_name', default='efficientdet-d0', help='Model name.')
  boolean('debug', 'Enable debug mode: eager steps, files read in order')
  ap.add_argument('--tf_random_seed', type=int, default=None, help='Fixed random seed for the model, the input draws and the reader.')
  boolean('profile', 'refused: use rocprofv3 on the process instead')
  ap.add_argument('--canvas', type=_canvas, default=(640, 640), help='HxW of the slot every decoded image is written into')
  ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f32'], help='storage dtype of the activations')
  ap.add_argument('--lion_beta2', type=float, default=None, help='--hparams=optimizer=lion: beta_2 (default 0.99)')
  ap.add_argument('--lion_wd', type=float, default=None,
                  help='--hparams=optimizer=lion: the decoupled weight decay wd (default 0), on every variable')
  ap.add_argument('--iou_loss_type', default=None, choices=['iou', 'giou', 'diou', 'ciou'],
                  help='adds BoxIouLoss of this type to the detection loss (not --hparams=iou_loss_type, which is refused)')
  ap.add_argument('--iou_loss_weight', type=float, default=None,
                  help='--iou_loss_type: its weight in det_loss (default: the configuration key iou_loss_weight, 1.0)')
  return ap


def iou_loss_of(flags):
  """--iou_loss_type / --iou_loss_weight -> EfficientDetNetTrain's `iou_loss` keyword; a weight without a type is refused."""
  if flags.iou_loss_type is None:
    if flags.iou_loss_weight is not None:
      raise ValueError('--iou_loss_weight needs --iou_loss_type')
    return None
  return {'type': flags.iou_loss_type, 'weight': flags.iou_loss_weight}


def lion_of(flags, config):
  """--lion_beta2 / --lion_wd -> EfficientDetNetTrain's `lion` keyword; refused for another optimizer."""
  lion = {k: v for k, v in (('beta_2', flags.lion_beta2), ('wd', flags.lion_wd)) if v is not None}
  if lion and str(config.optimizer).lower() != 'lion':
    raise ValueError('--lion_beta2 / --lion_wd need --hparams=optimizer=lion, this run has %r' % (config.optimizer,))
  return lion or None


def parse_flags(argv):
  """argv (without the program name) -> the flags; what is not built is refused here, before a model or a reader exists."""
  flags = define_flags().parse_args(list(argv))
  refused = []
  if flags.strategy:
    refused.append("--strategy=%s: data-parallel fit is not built (EfficientDetNetTrain takes a process_group; wiring the "
                   "driver to it is not done) -- leave it empty" % flags.strategy)
  for name in ('tpu', 'tpu_zone', 'gcp_project'):
    if getattr(flags, name):
      refused.append('--%s: there is no TPU path' % name)
  if flags.hub_module_url:
    refused.append('--hub_module_url: EfficientDetNetTrainHub (a TF-Hub SavedModel) is not read; use --pretrained_ckpt')
  if flags.use_xla:
    refused.append('--use_xla: there is no XLA here; the step is a replayed hipGraph already')
  if flags.profile:
    refused.append('--profile: the TensorBoard profiler is not built; profile the process from outside')
  if flags.steps_per_execution != 1:
    refused.append('--steps_per_execution=%d: only 1 is built (fit does not wait for the device per step as it is)'
                   % flags.steps_per_execution)
  if flags.batch_size < 1:
    refused.append('--batch_size=%d' % flags.batch_size)
  if refused:
    raise ValueError('; '.join(refused))
  return flags


def steps_per_epoch_of(flags):
  steps = flags.num_examples_per_epoch // flags.batch_size      # tf2/train.py:215
  if steps < 1:
    raise ValueError('--num_examples_per_epoch=%d holds no batch of %d' % (flags.num_examples_per_epoch, flags.batch_size))
  return steps


def build_config(flags):
  """tf2/train.py:155-158 and :215-229: the named config, --hparams, --num_epochs, then the run's own keys."""
  from automl_amd import hparams_config
  config = hparams_config.get_detection_config(flags.model_name)
  config.override(flags.hparams)
  if flags.num_epochs:
    config.num_epochs = flags.num_epochs
  config.override(dict(profile=False, model_name=flags.model_name, steps_per_execution=1, model_dir=flags.model_dir,
                       steps_per_epoch=steps_per_epoch_of(flags), strategy='', batch_size=flags.batch_size,
                       tf_random_seed=flags.tf_random_seed, debug=flags.debug, val_json_file=flags.val_json_file,
                       eval_samples=flags.eval_samples, num_shards=1), True)
  return config


def init_experimental(config):
  """Serialize train config to model directory (tf2/train.py:145-150): written once, never overwritten."""
  os.makedirs(config.model_dir, exist_ok=True)
  config_file = os.path.join(config.model_dir, 'config.yaml')
  if not os.path.exists(config_file):
    with open(config_file, 'w') as f:
      f.write(str(config))
  return config_file


def initial_epoch_of(iterations, steps_per_epoch):
  return int(iterations) // int(steps_per_epoch)      # tf2/train.py:282


def get_dataset(flags, config, is_training):
  from automl_amd import dataloader
  pattern = flags.train_file_pattern if is_training else flags.val_file_pattern
  if not pattern:
    raise ValueError('No matching files.')      # tf2/train.py:239-240
  params = config.as_dict()
  if not is_training:
    params['drop_remainder'] = False      # tf2/eval.py:53
  return dataloader.InputReader(pattern, is_training=is_training, use_fake_data=flags.use_fake_data,
                                max_instances_per_image=config.max_instances_per_image, debug=flags.debug)(
                                    params, batch_size=flags.batch_size, canvas=flags.canvas)


def main(argv=None):
  """-> fit's History (train, traineval) or the metrics (eval).  Never replaces the process."""
  flags = parse_flags(sys.argv[1:] if argv is None else argv)
  if not flags.model_dir:
    raise ValueError('--model_dir is needed')
  from automl_amd import tf_checkpoint, train_lib, util_keras
  config = build_config(flags)
  steps_per_epoch = config.steps_per_epoch
  model = train_lib.EfficientDetNetTrain(config=config, dtype=flags.dtype, seed=flags.tf_random_seed or 0,
                                         steps_per_epoch=steps_per_epoch, global_batch_size=flags.batch_size,
                                         use_graph=not flags.debug, lion=lion_of(flags, config),
                                         iou_loss=iou_loss_of(flags))
  latest = tf_checkpoint.latest_checkpoint(flags.model_dir) if os.path.isdir(flags.model_dir) else None

  if flags.mode == 'eval':
    if latest is None:
      raise FileNotFoundError('no checkpoint found in directory %s' % flags.model_dir)
    util_keras.restore_ckpt(model, latest, config.moving_average_decay)
    try:
      current_epoch = int(os.path.basename(latest).split('-')[1])      # tf2/train.py:297-300
    except (IndexError, ValueError):
      current_epoch = 0
    val = get_dataset(flags, config, False)
    try:
      coco_eval = train_lib.COCOCallback(val, 1)
      coco_eval.set_model(model)
      results = coco_eval.on_epoch_end(current_epoch)
    finally:
      val.close()
    print('eval results for %s: %s' % (latest, results), flush=True)
    return results

  train = get_dataset(flags, config, True)
  val = None
  try:
    if latest is not None:
      util_keras.restore_ckpt(model, latest, config.moving_average_decay)
      state_file = train_lib.train_state_path(latest)
      if os.path.exists(state_file):
        train_lib.restore_train_state(model, state_file, reader=train)
      else:
        logging.warning('%s has no training-state file: the weights are restored, the optimizer slots, the step count and '
                        'the reader start afresh', latest)
    elif flags.pretrained_ckpt:
      util_keras.restore_ckpt(model, flags.pretrained_ckpt, config.moving_average_decay,
                              exclude_layers=['class_net', 'optimizer', 'box_net'])
    init_experimental(config)
    if 'eval' in flags.mode:
      val = train_lib.RepeatableReader(get_dataset(flags, config, False))
    return model.fit(train, epochs=config.num_epochs, steps_per_epoch=steps_per_epoch,
                     initial_epoch=initial_epoch_of(model.iterations, steps_per_epoch),
                     callbacks=train_lib.get_callbacks(config.as_dict(), val), validation_data=val,
                     validation_steps=flags.eval_samples // flags.batch_size)
  finally:
    train.close()
    if val is not None:
      val.close()


if __name__ == '__main__':
  logging.basicConfig(level=logging.INFO)
  main()
