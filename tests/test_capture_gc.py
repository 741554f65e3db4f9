"""layer_engine.capture_graph keeps the cyclic garbage collector out of a hipGraph capture: what is dead is collected before
the capture begins, automatic collection is off while the body runs and is back -- if it was on -- afterwards, also when the
body raises.  (torch.cuda.graph itself no longer collects on entry, and a dead cycle that owns graphs, events or pinned
buffers must not be finalised while a stream is capturing.)"""
import gc
import types
import weakref

import pytest
import torch

from automl_amd import layer_engine
from tests import gpu_util as gu


class Node(object):
  pass


def dead_cycle():
  a, b = Node(), Node()
  a.other, b.other = b, a
  return weakref.ref(a)


@pytest.mark.gpu
def test_the_collector_stays_out_of_the_capture():
  arena = types.SimpleNamespace(version=3, step_count=7)
  x = torch.zeros(64, device=gu.DEV)
  seen = {}
  assert gc.isenabled()
  gc.disable()      # (so that the cycle below is still there when capture_graph is called)
  try:
    ref = dead_cycle()
    assert ref() is not None
  finally:
    gc.enable()

  def body():
    seen['enabled'], seen['dead'] = gc.isenabled(), ref() is None
    arena.version += 1
    x.add_(1.0)
  graph = layer_engine.capture_graph(arena, body)
  assert seen == {'enabled': False, 'dead': True} and gc.isenabled()
  assert (arena.version, arena.step_count) == (3, 7)
  graph.replay()
  torch.cuda.synchronize()
  assert float(x[0]) == 1.0      # the capture pass executed nothing

  def fails():
    x.add_(1.0)
    raise RuntimeError('in the body')
  with pytest.raises(RuntimeError, match='in the body'):
    layer_engine.capture_graph(arena, fails)
  assert gc.isenabled()
  gc.disable()      # a caller that had it off keeps it off
  try:
    layer_engine.capture_graph(arena, lambda: x.add_(1.0))
    assert not gc.isenabled()
  finally:
    gc.enable()
