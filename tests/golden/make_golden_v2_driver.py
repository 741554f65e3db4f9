"""Generates tests/golden/reference_v2_driver.json by EXECUTING the reference's efficientnetv2/hparams.py and
efficientnetv2/datasets.py -- unmodified -- on the torch stand-in of mini_keras (TensorFlow, tensorflow_datasets, absl and the
reference's own preprocessing module are stubs: nothing of them runs while the tables are built):

  base_config        hparams.base_config's train / eval / data / runtime sections (hparams.py:245-312)
  imagenet_input     datasets.ImageNetInput.cfg (datasets.py:78-91), slices as [start, stop]
  dataset_configs    datasets.get_dataset_config(name) for 'imagenet' and 'imagenetft' (datasets.py:646-663, :699-727, :764-768)
  dataset_classes    the names datasets.get_dataset_class serves (datasets.py:631-641)
  unbuilt            per data set that automl_amd/effnetv2_datasets.py refuses: multiclass and tfds_name of its class table

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_v2_driver.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mini_keras   # noqa
from mini_keras import stub_module   # noqa

REF = '/root/reference/efficientnetv2'


def plain(value):
  if hasattr(value, 'as_dict'):
    value = value.as_dict()
  if isinstance(value, dict):
    return {k: plain(v) for k, v in value.items()}
  if isinstance(value, (list, tuple)):
    return [plain(v) for v in value]
  if isinstance(value, slice):
    return [value.start, value.stop]
  return value


def main():
  mini_keras.install(mini_keras.build_tf())
  for name in ('tensorflow_datasets', 'tensorflow_addons.image', 'preprocessing'):
    sys.modules.setdefault(name, stub_module(name))
  sys.modules.pop('hparams', None)
  sys.path.insert(0, REF)
  import hparams as ref_hparams     # noqa: the reference module
  import datasets as ref_datasets   # noqa: the reference module
  base = ref_hparams.base_config
  out = {
      'base_config': {k: plain(base[k] if hasattr(base, '__getitem__') else getattr(base, k)) for k in ('train', 'eval', 'data', 'runtime')},
      'imagenet_input': plain(ref_datasets.ImageNetInput.cfg),
      'dataset_configs': {name: plain(ref_datasets.get_dataset_config(name)) for name in ('imagenet', 'imagenetft')},
      'dataset_classes': sorted(n for n in ('imagenet', 'imagenet21k', 'imagenettfds', 'cifar10', 'cifar100', 'flowers',
                                            'tfflowers', 'cars') if ref_datasets.get_dataset_class(n) is not None),
      'unbuilt': {n: {'multiclass': ref_datasets.get_dataset_class(n).cfg.multiclass,
                      'tfds_name': ref_datasets.get_dataset_class(n).cfg.get('tfds_name', None)}
                  for n in ('imagenet21k', 'imagenettfds', 'cifar10', 'cifar100', 'flowers', 'tfflowers', 'cars')},
  }
  path = os.path.join(HERE, 'reference_v2_driver.json')
  with open(path, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
  print('wrote', path)


if __name__ == '__main__':
  main()
