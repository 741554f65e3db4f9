"""The classifier training driver on the device, bit for bit: the reader's batches against JpegDecoder by hand, fit against a
hand loop of train_step (graph and eager, plain and with crop, RandAugment, mixup and cutmix on), evaluate against test_step by
hand with the training state untouched, exact resume through model_dir into a new model and a new reader (cut inside a stage
and at a stage boundary), and effnetv2_main in-process (train, continue, eval).  efficientnetv2-b0 with 24 classes, training
sizes 32 and 48, batch 4, a 56 x 56 canvas; the shards are written here from tests/golden/jpeg_cases.npz."""
import os

import numpy as np
import pytest
import torch

from automl_amd import effnetv2_datasets as ds, effnetv2_main as main_lib, effnetv2_train as et, jpeg, tf_checkpoint, tfrecord, \
    train_lib, util_keras, v2_preprocessing as vp
from tests import v2_datasets_ref as ref

pytestmark = pytest.mark.gpu

CLASSES, BATCH, CANVAS, SEED = 24, 4, (56, 56), 5
TRAIN_SIZES = [2] * 20 + [7, 5, 6, 9]      # 'train' = files [20:]: 27 records, six batches an epoch
VAL_SIZES = [5, 4, 6]
ARENA_KEYS = ('params_flat', 'grads_flat', 'velocity', 'ema', 'adam_v', 'state_flat')
EVERYTHING = dict(augname='randaug', ra_magnitude=9, mixup_alpha=0.3, cutmix_alpha=0.3, ema_decay=0.99)
STAGES = [dict(start_epoch=0, end_epoch=2, image_size=32, ra_magnitude=5.0, mixup_alpha=0.1, cutmix_alpha=0.2),
          dict(start_epoch=2, end_epoch=4, image_size=48, ra_magnitude=9.0, mixup_alpha=0.3, cutmix_alpha=0.3)]


@pytest.fixture(scope='module')
def data(tmp_path_factory):
  folder = tmp_path_factory.mktemp('imagenet')
  jpegs = ref.load_jpegs()
  content = ref.write_shards(folder, jpegs, TRAIN_SIZES, VAL_SIZES, CLASSES, tfrecord.TFRecordWriter, tfrecord.encode_example)
  decoded = {j: jpeg.decode_jpeg(j).cpu() for j in jpegs}      # each image once, by hand
  return str(folder), content, decoded


def reader_of(folder, training, split=None, **kw):
  return ds.ImageNetInput(training, folder, split, seed=SEED, cfg={'num_classes': CLASSES})(BATCH, canvas=CANVAS, **kw)


def net(**kw):
  args = dict(learning_rate=0.02, weight_decay=1e-5, label_smoothing=0.1, seed=4, image_size=32, dtype='bf16')
  args.update(kw)
  return et.TrainableModel('efficientnetv2-b0', 'num_classes=%d' % CLASSES, **args)


def take(reader, n):
  out = []
  for batch in reader:
    out.append(batch)
    if len(out) == n:
      break
  return out


def snapshot(model):
  torch.cuda.synchronize()
  arena = model.engine.arena
  snap = {k: getattr(arena, k).clone() for k in ARENA_KEYS if getattr(arena, k) is not None}
  snap.update({'state.' + k: np.array(v, copy=True) for k, v in model.get_optimizer_state().items()})
  snap['iterations'] = model.iterations
  return snap


def assert_same(a, b):
  assert sorted(a) == sorted(b)
  for k in a:
    same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else np.array_equal(a[k], b[k])
    assert same, k


def host_logs(sums, batch, prefix=''):
  """The issue's table on the host: float32 sums in step order, float32 divisions."""
  acc = np.zeros(4, np.float32)
  for s in sums:
    acc += s.astype(np.float32)
  n, rows = np.float32(len(sums)), np.float32(len(sums)) * np.float32(batch)
  return {prefix + 'loss': float((acc[0] + acc[3]) / n), prefix + 'reg_l2_loss': float(acc[3] / n),
          prefix + 'acc_top1': float(acc[1] / rows), prefix + 'acc_top5': float(acc[2] / rows)}


# ------------------------------------------------------------------------------------------------------------ the reader
@pytest.mark.parametrize('training', [True, False])
def test_reader_batches_equal_the_decoder_by_hand(data, training):
  folder, content, decoded = data
  reader, host = reader_of(folder, training), ds.ImageNetInput(training, folder, seed=SEED, cfg={'num_classes': CLASSES}).host_reader(BATCH)
  got, index = take(reader, 3), [b.index for b in take(host, 3)]
  reader.close(), host.close()
  assert len(got) == 3
  for ((raw, sizes), labels), pairs in zip(got, index):
    rows = [content[os.path.basename(reader.files[f])][r] for f, r in pairs]
    want_raw, want_sizes = vp.pad_batch([decoded[image] for image, _ in rows], CANVAS)
    assert raw.is_cuda and raw.dtype == torch.uint8 and tuple(raw.shape) == (BATCH,) + CANVAS + (3,)
    assert torch.equal(raw.cpu(), want_raw) and sizes.dtype == np.int32 and np.array_equal(sizes, want_sizes)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.tolist() == [c for _, c in rows]
    by_hand, hand_sizes = jpeg.JpegDecoder(BATCH, *CANVAS).decode([image for image, _ in rows])
    assert torch.equal(raw, by_hand) and np.array_equal(sizes, hand_sizes)


def test_reader_oversize_and_fallback(data, tmp_path):
  _, _, decoded = data
  jpegs = ref.load_jpegs()
  big, wide = ref.load_jpegs(ref.OVERSIZE)
  with tfrecord.TFRecordWriter(tmp_path / 'val-00000-of-00001') as w:
    for r, image in enumerate((jpegs[1], big, jpegs[3], wide)):
      w.write(tfrecord.encode_example({'image/encoded': image, 'image/class/label': [r + 1]}))
  reader = reader_of(str(tmp_path), False)
  with pytest.raises(ValueError, match='val-00000-of-00001 record 1: contents.1. is not decoded: an image larger than the canvas'):
    next(reader)
  reader.close()
  patch = np.arange(7 * 9 * 3, dtype=np.uint8).reshape(7, 9, 3)
  reader = reader_of(str(tmp_path), False, fallback=lambda contents: patch)
  (raw, sizes), labels = next(reader)
  reader.close()
  want, want_sizes = vp.pad_batch([decoded[jpegs[1]], patch, decoded[jpegs[3]], patch], CANVAS)
  assert torch.equal(raw.cpu(), want) and np.array_equal(sizes, want_sizes) and labels.tolist() == [0, 1, 2, 3]


# --------------------------------------------------------------------------------------------------------------- fit
@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('everything', [False, True])
def test_fit_equals_a_hand_loop_of_train_step(data, use_graph, everything):
  folder = data[0]
  kw = dict(EVERYTHING if everything else {}, use_graph=use_graph)
  fitted, reader = net(**kw), reader_of(folder, True)
  history = fitted.fit(reader, epochs=2, steps_per_epoch=3, verbose=0)
  by_hand, hand_reader, sums, lrs = net(**kw), reader_of(folder, True), [], []
  for batch in take(hand_reader, 6):
    lrs.append(by_hand.train_step(batch, sync_loss=False)['learning_rate'])
    sums.append(by_hand.engine.cls_sums.cpu().numpy().copy())
  assert_same(snapshot(fitted), snapshot(by_hand))
  assert fitted.iterations == 6 and history.epoch == [0, 1]
  if everything:
    assert all(k in fitted.get_optimizer_state() for k in ('rng_state', 'mix_rng_state', 'randaug_rng_state', 'crop_rng_state', 'rms', 'ema'))
  for epoch in range(2):
    want = host_logs(sums[3 * epoch:3 * epoch + 3], BATCH)
    want['learning_rate'] = lrs[3 * epoch + 2]
    assert {k: v[epoch] for k, v in history.history.items()} == want, epoch
    assert np.isfinite(want['loss']) and want['reg_l2_loss'] > 0
  assert reader.get_state() == hand_reader.get_state()      # fit took six batches and no more
  reader.close(), hand_reader.close()


# ----------------------------------------------------------------------------------------------------------- evaluate
def test_evaluate_equals_test_step_by_hand_and_moves_nothing(data):
  folder = data[0]
  model = net(**EVERYTHING)
  for batch in take(reader_of(folder, True), 2):
    model.train_step(batch, sync_loss=False)
  before = snapshot(model)
  val = train_lib.RepeatableReader(reader_of(folder, False))
  got = model.evaluate(val)
  assert_same(before, snapshot(model))      # variables, slots, shadows, BatchNorm statistics, generators, count, gradient arena
  sums, full = [], []
  for batch in val:
    full.append(model.test_step(batch))
    sums.append(model.engine.cls_sums.cpu().numpy().copy())
  assert len(sums) == sum(VAL_SIZES) // BATCH == 3 and got == host_logs(sums, BATCH)
  assert model.test_step(batch, sync_loss=False) == {} and set(full[0]) == set(et.METRIC_KEYS)
  assert model.evaluate(val, steps=2) == host_logs(sums[:2], BATCH)
  # as validation_data its values enter the epoch's logs under val_*, and the training state is what fit alone leaves
  history = model.fit(reader_of(folder, True), epochs=1, steps_per_epoch=2, validation_data=val, validation_steps=2, verbose=0)
  alone = net(**EVERYTHING)
  for batch in take(reader_of(folder, True), 2) + take(reader_of(folder, True), 2):
    alone.train_step(batch, sync_loss=False)
  assert_same(snapshot(model), snapshot(alone))
  sums = []
  for batch in take(iter(val), 2):
    model.test_step(batch)
    sums.append(model.engine.cls_sums.cpu().numpy().copy())
  want = host_logs(sums, BATCH, 'val_')
  assert {k: v[0] for k, v in history.history.items() if k.startswith('val_')} == want
  val.close()


# ------------------------------------------------------------------------------------------------------------- resume
def staged_run(folder, model_dir, epochs, model=None, reader=None, initial_epoch=0):
  model = model or net(**dict(EVERYTHING, image_size=48))
  reader = reader or reader_of(folder, True)
  ckpt = et.ModelCheckpoint(os.path.join(model_dir, 'ckpt-{epoch:d}'))
  history = model.fit(reader, epochs=epochs, steps_per_epoch=3, initial_epoch=initial_epoch, callbacks=[ckpt], stages=STAGES, verbose=0)
  return model, reader, history


@pytest.fixture(scope='module')
def in_one_go(data, tmp_path_factory):
  model, reader, history = staged_run(data[0], str(tmp_path_factory.mktemp('whole')), 4)
  out = snapshot(model), reader.get_state(), history
  reader.close()
  return out


@pytest.mark.parametrize('cut', [1, 2])      # inside the first stage; at the boundary, where the first restored step is at 48
def test_exact_resume_from_model_dir(data, in_one_go, tmp_path, cut):
  folder = data[0]
  want, want_reader, want_history = in_one_go
  model_dir = str(tmp_path / 'run')
  first, reader, _ = staged_run(folder, model_dir, cut)
  reader.close()
  del first
  latest = tf_checkpoint.latest_checkpoint(model_dir)
  assert os.path.basename(latest) == 'ckpt-%d' % cut and os.path.exists(train_lib.train_state_path(latest))
  model, reader = net(**dict(EVERYTHING, image_size=48)), reader_of(folder, True)      # new, as a new process makes them
  util_keras.restore_ckpt(model, latest, ema_decay=0, skip_mismatch=False)
  et.restore_train_state(model, train_lib.train_state_path(latest), reader=reader)
  assert model.engine is None and model.iterations == 3 * cut and model.current_stage()['image_size'] == 32
  _, _, history = staged_run(folder, model_dir, 4, model, reader, initial_epoch=model.iterations // 3)
  assert_same(want, snapshot(model))
  assert reader.get_state() == want_reader
  assert history.epoch == list(range(cut, 4)) and model.engine.image_size == (48, 48)
  for k, v in want_history.history.items():
    assert history.history[k] == v[cut:], k
  reader.close()


# ---------------------------------------------------------------------------------------------------------------- main
def test_main_trains_continues_and_evaluates(data, tmp_path, capsys):
  import shutil
  folder = data[0]
  hparams = ('data.num_classes=%d,data.augname=randaug,train.isize=48,eval.isize=32,data.ibase=16,train.stages=2,train.batch_size=4,'
             'eval.batch_size=4,train.lr_warmup_epoch=1,data.splits.train.num_images=12,data.splits.eval.num_images=12,'
             'data.mixup_alpha=0.2,data.cutmix_alpha=0.2,data.ram=8' % CLASSES)

  def argv(model_dir, mode, epochs=2):
    return ['--mode=' + mode, '--model_name=efficientnetv2-b0', '--data_dir=' + folder, '--model_dir=' + model_dir, '--canvas=56x56',
            '--seed=3', '--hparam_str=%s,train.epochs=%d' % (hparams, epochs)]
  whole, run = str(tmp_path / 'whole'), str(tmp_path / 'run')
  first = main_lib.main(argv(whole, 'train'))      # two stages of one epoch each: 32, then 48
  assert first.epoch == [0, 1] and os.path.exists(os.path.join(whole, 'config.yaml'))
  assert os.path.basename(tf_checkpoint.latest_checkpoint(whole)) == 'ckpt-2'
  # what a run killed inside its second epoch leaves behind: ckpt-1 with its training state
  shutil.copytree(whole, run)
  for name in os.listdir(run):
    if name.startswith('ckpt-2'):
      os.remove(os.path.join(run, name))
  tf_checkpoint.update_checkpoint_state(run, os.path.join(run, 'ckpt-1'))
  second = main_lib.main(argv(run, 'train'))
  assert second.epoch == [1] and os.path.basename(tf_checkpoint.latest_checkpoint(run)) == 'ckpt-2'
  assert {k: v[0] for k, v in second.history.items()} == {k: v[1] for k, v in first.history.items()}
  a, b = tf_checkpoint.CheckpointReader(os.path.join(run, 'ckpt-2')), tf_checkpoint.CheckpointReader(os.path.join(whole, 'ckpt-2'))
  names = sorted(a.get_variable_to_shape_map())
  assert names == sorted(b.get_variable_to_shape_map()) and int(a.get_tensor('global_step')) == 6
  assert all(np.array_equal(a.get_tensor(n), b.get_tensor(n)) for n in names)
  with np.load(train_lib.train_state_path(os.path.join(run, 'ckpt-2'))) as x, np.load(train_lib.train_state_path(os.path.join(whole, 'ckpt-2'))) as y:
    assert sorted(x.files) == sorted(y.files) and all(np.array_equal(x[k], y[k]) for k in x.files)
  assert main_lib.main(argv(run, 'train')).epoch == []      # nothing is left of two epochs
  third = main_lib.main(argv(run, 'traineval', 3))          # one more, with validation
  assert third.epoch == [2] and 'val_acc_top5' in third.history and os.path.basename(tf_checkpoint.latest_checkpoint(run)) == 'ckpt-3'
  # eval: the four values of evaluate on the restored model
  capsys.readouterr()
  results = main_lib.main(argv(run, 'eval', 3))
  printed = capsys.readouterr().out
  flags = main_lib.parse_flags(argv(run, 'eval', 3))
  config = main_lib.build_config(flags)
  plan = main_lib.plan_of(config)
  model = main_lib.build_model(flags, config, plan)
  util_keras.restore_ckpt(model, tf_checkpoint.latest_checkpoint(run), ema_decay=0, skip_mismatch=False)
  val = main_lib.get_dataset(flags, config, plan, False)
  want = model.evaluate(val, steps=3)
  val.close()
  assert results == want and set(results) == set(et.METRIC_KEYS) and plan['validation_steps'] == 3
  assert all('%s: %.6g' % (k, want[k]) in printed for k in et.METRIC_KEYS) and 'ckpt-3' in printed
