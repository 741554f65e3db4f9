"""Layer machinery of the MI355X engines: launches the gfx950 kernels through the C ABI.

Host side is plain Python (as BASELINE.json's north_star asks): LayerEngine owns the HBM buffers (torch tensors are used
only as device allocations), the variables (ParamArena) and the layer primitives; a network is a subclass that builds its
graph from them (engine.Engine: EfficientDet, effnetv2_model.V2Engine: the EfficientNetV2 classifier).
Design:
  * every conv output is stored ONCE, raw (pre-BatchNorm); BatchNorm + swish + SE gate are applied
    on load by the consumer ("activated view"), BatchNorm statistics come out of the producing
    kernel's epilogue as deterministic per-workgroup partials;
  * backward mirrors it: a data-gradient kernel chains through the consumer-side activation and
    emits the BatchNorm-backward sums; the BatchNorm backward itself is applied on load
    (dy = a*dz + b*y + c) by the producer's wgrad / dgrad kernels;
  * forward records a tape of closures, backward replays it in reverse.
Reference structure followed: efficientdet/backbone/efficientnet_model.py:360-416,710-779, tf2/train_lib.py:176-199,486-491,675-683.
"""
import collections
import contextlib
import ctypes
import gc
import re
import math

import numpy as np
import torch

from automl_amd import _lib
from automl_amd import netspec as netspec_lib
from automl_amd import utils
from automl_amd._lib import ACT_NONE, EDET_BF16, EDET_F32, BwdEpi, GView, TView, call, ptr


def _pad8(c):
  return (c + 7) // 8 * 8


class Raw(object):
  """A stored NHWC tensor and (lazily) its gradient buffer."""

  def __init__(self, eng, key, n, h, w, c, ld=None, needs_grad=True, dtype=None):
    self.eng, self.key = eng, key
    self.n, self.h, self.w, self.c = n, h, w, c
    self.ld = ld or _pad8(c)
    self.data = eng.buf(key, (n, h, w, self.ld), dtype or eng.tdtype)
    self.needs_grad = needs_grad
    self.grad = None
    self.grad_written = False

  def ensure_grad(self):
    if self.grad is None:
      self.grad = self.eng.buf(self.key + '#grad', (self.n, self.h, self.w, self.ld), self.eng.tdtype)
    return self.grad

  @property
  def rows(self):
    return self.n * self.h * self.w


class BN(object):
  """BatchNorm layer state: parameter slices + per-step derived vectors (fp32 [c])."""

  def __init__(self, eng, name, c):
    self.name, self.c = name, c
    self.gamma = eng.param(name + '/gamma')
    self.beta = eng.param(name + '/beta')
    self.mm = eng.param(name + '/moving_mean')
    self.mv = eng.param(name + '/moving_variance')
    self.dgamma = eng.arena.grad(name + '/gamma')     # per-layer variables: always the main gradient arena
    self.dbeta = eng.arena.grad(name + '/beta')
    v = eng.buf('bn:' + name, (7, c), torch.float32)
    self.scale, self.shift, self.mean, self.rstd, self.a, self.b, self.cc = (v[i] for i in range(7))
    self.count = 0
    self.bwd_ready = False
    self.eval_done = False


class View(object):
  """act(bn(raw)) * gate -- what a consumer kernel sees (edet_tview_t)."""

  def __init__(self, raw, bn=None, act=ACT_NONE, gate=None):
    self.raw, self.bn, self.act, self.gate = raw, bn, act, gate
    self.consumers = 0

  def tview(self):
    r = self.raw
    return TView(ptr(r.data), ptr(self.bn.scale) if self.bn else None,
                 ptr(self.bn.shift) if self.bn else None, ptr(self.gate), self.act,
                 r.n, r.h, r.w, r.c, r.ld)


class ParamArena(object):
  """The model's variables on the device, independent of batch and image size: one flat fp32 master arena of the
  trainable variables (+ gradient, momentum and EMA arenas of the same layout), one of the BatchNorm moving
  statistics, the segment table for per-tensor clipping, and the optimizer's iteration count.  Every Engine of a
  model (one per batch / image shape) works on the SAME arena, so a shape change keeps the optimizer slots, as the
  reference's Keras variables do (train_lib.py:176-199)."""

  def __init__(self, spec, device, values):
    train = [p for p in spec.params if p.trainable]
    state = [p for p in spec.params if not p.trainable]
    self.offsets = {}
    off = 0
    seg = [0]
    flags = []
    for p in train:
      n = int(np.prod(p.shape)) if p.shape else 1
      self.offsets[p.name] = (off, n, p.shape, True)
      off += n
      off_al = (off + 3) // 4 * 4  # keep every tensor 16-byte aligned
      seg.append(off)
      flags.append(1 if netspec_lib.is_l2_regularised(p.name) else 0)
      if off_al != off:
        seg.append(off_al)  # padding segment (zeros, never regularised)
        flags.append(0)
        off = off_al
    self.n_train_elems = off
    self.seg_names = [p.name for p in train]
    soff = 0
    for p in state:
      n = int(np.prod(p.shape))
      self.offsets[p.name] = (soff, n, p.shape, False)
      soff = (soff + n + 3) // 4 * 4
    dev = self.device = torch.device(device)
    self.params_flat = torch.zeros(off, dtype=torch.float32, device=dev)
    self.grads_flat = torch.zeros(off, dtype=torch.float32, device=dev)
    self.velocity = torch.zeros(off, dtype=torch.float32, device=dev)
    self.ema = torch.zeros(off, dtype=torch.float32, device=dev)
    self.adam_v = None        # the second slot arena, allocated on first use (second_moment)
    self.state_flat = torch.zeros(max(soff, 4), dtype=torch.float32, device=dev)
    self.seg_offsets = torch.tensor(seg, dtype=torch.int64, device=dev)
    self.seg_flags = torch.tensor(flags, dtype=torch.int32, device=dev)
    self.nseg = len(flags)
    self._l2_flags = list(flags)          # as built: set_frozen starts from these every time
    self.seg_sqnorm = torch.zeros(2 * self.nseg * _lib.OPT_SPLIT, dtype=torch.float32, device=dev)   # norms | L2 partials
    self.seg_factor = torch.ones(self.nseg, dtype=torch.float32, device=dev)
    self.version = 0          # bumped whenever a variable changes: engines re-make their compute copies
    self.step_count = 0       # optimizer iterations applied to this arena
    self.frozen_expr = None
    self.frozen_ranges = []   # [begin, end) element ranges of the frozen variables in the flat arrays (set_frozen)
    self.set_params(values)

  def set_frozen(self, expr):
    """config.var_freeze_expr (tf2/train_lib.py:478-491): the trainable variables whose name -- with the ':0' TensorFlow
    appends -- matches the expression from its start are left out of the L2 term, of the gradient list (per-tensor and
    global clip norms) and of the update.  Here: their segment carries EDET_SEG_FROZEN instead of the L2 flag -- the
    optimizer kernels zero their gradient, count nothing of them in the norms and never touch their value, momentum
    slot or EMA shadow (so an optimizer state restored from an un-frozen run cannot move them either).  The flags are
    rebuilt from the arena's original ones on every call: another expression un-freezes what no longer matches, an
    empty one un-freezes everything.  Returns the frozen names."""
    frozen = []
    if expr:
      pat = re.compile(expr)
      frozen = [n for n in self.seg_names if pat.match(n + ':0')]
    seg_index = {int(o): i for i, o in enumerate(self.seg_offsets.cpu().tolist()[:-1])}
    flags = list(self._l2_flags)
    ranges = []
    for n in frozen:
      off, cnt, _, _ = self.offsets[n]
      flags[seg_index[off]] = _lib.SEG_FROZEN
      if ranges and off - ranges[-1][1] <= 3:      # adjacent up to the alignment padding (zeros): one range
        ranges[-1][1] = off + cnt
      else:
        ranges.append([off, off + cnt])
    self.seg_flags.copy_(torch.tensor(flags, dtype=torch.int32))
    self.frozen_expr = expr or None
    self.frozen_ranges = [(a, b) for a, b in ranges]
    for a, b in self.frozen_ranges:
      self.velocity[a:b].zero_()
    return frozen

  def _slice(self, flat_train, flat_state, name):
    off, n, _, tr = self.offsets[name]
    return (flat_train if tr else flat_state)[off:off + n]

  def param(self, name):
    return self._slice(self.params_flat, self.state_flat, name)

  def grad(self, name):
    off, n, _, tr = self.offsets[name]
    assert tr, name
    return self.grads_flat[off:off + n]

  def set_params(self, values):
    """values: name -> array-like in reference layouts.  Until the first optimizer step the EMA shadow follows the
    variables (TFA MovingAverage seeds the average with the variable's value at its first apply)."""
    for name, v in values.items():
      if name not in self.offsets:
        raise KeyError('unknown variable %s' % name)
      off, n, shape, tr = self.offsets[name]
      t = torch.as_tensor(np.asarray(v, dtype=np.float32)).reshape(-1)
      if t.numel() != n:
        raise ValueError('variable %s: expected %d elements, got %d' % (name, n, t.numel()))
      self.param(name).copy_(t)
      if self.step_count == 0 and tr:
        self._slice(self.ema, None, name).copy_(t)
    self.version += 1

  def _export(self, flat_train, flat_state, names):
    out = {}
    for name in (names or self.offsets.keys()):
      shape = self.offsets[name][2]
      out[name] = self._slice(flat_train, flat_state, name).detach().cpu().numpy().reshape(shape)
    return out

  def get_params(self, names=None):
    return self._export(self.params_flat, self.state_flat, names)

  def get_ema_params(self, names=None):
    """The variables as an EMA evaluation would load them: the TFA MovingAverage shadow of every trainable variable
    (train_lib.py:193-197 wraps the optimizer, which averages the variables it updates) and the BatchNorm moving
    statistics as they are (they have no shadow in the Keras train step)."""
    return self._export(self.ema, self.state_flat, names)

  def set_ema_params(self, values):
    """EMA shadows (the MovingAverage optimizer's 'average' slots) of trainable variables, by name."""
    for name, v in values.items():
      if name not in self.offsets:
        raise KeyError('unknown variable %s' % name)
      off, n, shape, tr = self.offsets[name]
      if not tr:
        raise KeyError('%s has no EMA shadow (not a trainable variable)' % name)
      t = torch.as_tensor(np.asarray(v, dtype=np.float32)).reshape(-1)
      if t.numel() != n:
        raise ValueError('variable %s: expected %d elements, got %d' % (name, n, t.numel()))
      self._slice(self.ema, None, name).copy_(t)

  def get_optimizer_state(self):
    """Host copy of the optimizer slots: momentum (Adam: first moment), EMA shadows, iteration count; the second slot when
    an optimizer that has one has run -- under 'adam_v' (Adam's second moment) or 'rms' (RMSprop's mean square)."""
    state = {'velocity': self.velocity.cpu().numpy().copy(), 'ema': self.ema.cpu().numpy().copy(),
             'iterations': self.step_count}
    if self.adam_v is not None:
      state[self.second_slot_key] = self.adam_v.cpu().numpy().copy()
    return state

  def set_optimizer_state(self, state):
    self.velocity.copy_(torch.as_tensor(state['velocity']))
    self.ema.copy_(torch.as_tensor(state['ema']))
    for key in ('adam_v', 'rms'):
      if key in state:
        self.use_second_slot(key)
        self.second_moment().copy_(torch.as_tensor(state[key]))
    self.step_count = int(state['iterations'])

  second_slot_key = 'adam_v'

  def use_second_slot(self, key):
    """Names the optimizer that owns the second slot arena: 'adam_v' (Adam's v, the default) or 'rms' (RMSprop's mean
    square, effnetv2_train.TrainableModel) -- the key it has in get_optimizer_state.  One optimizer per arena: once
    steps have been applied with the slot allocated, another owner is refused (Adam's v is not RMSprop's ms)."""
    assert key in ('adam_v', 'rms'), key
    if key != self.second_slot_key and self.adam_v is not None and self.step_count > 0:
      raise ValueError('the second optimizer slot of this arena holds %r after %d steps; it cannot become %r'
                       % (self.second_slot_key, self.step_count, key))
    self.second_slot_key = key

  def second_moment(self):
    """The second slot arena (attribute `adam_v`: the name plans and state files know it by), allocated on first use (the
    SGD configurations never pay for it): Adam's v, or RMSprop's ms when use_second_slot('rms') said so."""
    if self.adam_v is None:
      self.adam_v = torch.zeros_like(self.velocity)
    return self.adam_v

  def count_step(self):
    """One optimizer step has been applied to the variables, by an eager update or by a replayed graph."""
    self.version += 1
    self.step_count += 1


def capture_graph(arena, body, pool=None):
  """body() captured into a new hipGraph.  thread_local: other threads of the process (the RCCL watchdog) may touch the
  HIP runtime meanwhile.  The capture pass runs the body's host bookkeeping once WITHOUT executing anything, so the
  arena's counters are put back where they were (also when the capture raises); ParamArena.count_step accounts for every
  replay.
  The cyclic garbage collector stays out of the capture.  torch.cuda.graph collected on entry up to torch 2.8 and does so now
  only with TORCH_CUDAGRAPH_GC set, so a dead cycle that owns device objects -- a model that was dropped with its captured
  graphs, events and pinned buffers, as a test or a driver that builds a second model leaves behind -- could be finalised by
  an automatic collection in the middle of the body: releasing a graph and its pool, or recording the event behind a pinned
  buffer, while a stream of this thread is capturing is an error raised inside a destructor, which ends the process.  So what
  is dead is collected before the capture begins, and automatic collection is off until it has ended."""
  counters = (arena.version, arena.step_count)
  graph = torch.cuda.CUDAGraph()
  gc.collect()
  collecting = gc.isenabled()
  gc.disable()
  try:
    with torch.cuda.graph(graph, pool=pool, capture_error_mode='thread_local'):
      body()
  finally:
    if collecting:
      gc.enable()
    arena.version, arena.step_count = counters
  return graph


# What an engine's update step runs: kind = 'sgd' (Keras SGD; momentum), 'adam' (momentum = beta_1, beta2, epsilon),
# 'rmsprop' (rho, momentum, epsilon) or 'lion' (momentum = beta_1, beta2 = beta_2, wd).  Scalars a kind does not use stay None.
Update = collections.namedtuple('Update', 'kind momentum beta2 epsilon rho wd', defaults=(None, None, None, None))
LION_BETA2, LION_WD = 0.99, 0.0       # lion/lion_tf2.py:23-28


def lion_options(options, beta_2=LION_BETA2, wd=LION_WD):
  """The two Lion scalars that are no configuration keys, checked: `options` (a dict with 'beta_2' and / or 'wd', or None) over
  the given current values -> (beta_2, wd)."""
  options = dict(options or {})
  unknown = sorted(set(options) - {'beta_2', 'wd'})
  if unknown:
    raise ValueError('lion: unknown option %s (beta_2 and wd are what there is)' % ', '.join(unknown))
  if options.get('beta_2') is not None:
    beta_2 = float(options['beta_2'])
  if options.get('wd') is not None:
    wd = float(options['wd'])
  if not 0.0 <= beta_2 < 1.0:
    raise ValueError('lion: beta_2 %r outside [0, 1)' % (beta_2,))
  if not wd >= 0.0:
    raise ValueError('lion: wd %r must be >= 0' % (wd,))
  return beta_2, wd


class Branch(object):
  """What an independent chain of launches needs of its own: a HIP stream, the BatchNorm partial-sum rows and the
  weight-gradient workspace its kernels scribble on, and -- for a chain that shares variables with another one (the
  class / box towers use the same kernels on every pyramid level, efficientdet_keras.py:336-480) -- a private
  gradient arena that is added to the main one after the join (deterministic, no atomics)."""

  def __init__(self, stream, partials, workspace, grads=None):
    self.stream, self.partials, self.workspace, self.grads = stream, partials, workspace, grads
    self.ws_off = 0       # bytes of the workspace that hold partial sums of deferred reductions (LayerEngine._ws_mark)


class LayerEngine(object):
  """Buffers for (spec, batch, image size, dtype), the layer primitives with their backward closures, and the update step
  that `update` names.  The subclass's forward() calls _begin, stem and the primitives; backward() replays their tape."""
  ADAM_BETA2, ADAM_EPSILON = 0.999, 1e-7      # tf.keras.optimizers.Adam defaults

  def __init__(self, spec, batch_size, image_size, dtype='bf16', device='cuda:0', seed=0, params=None, arena=None,
               stochastic_depth=True, *, update):
    if not torch.cuda.is_available():
      raise _lib.EdetError('no HIP device visible: the EfficientDet engine has no CPU path')
    _lib.load()
    self.spec = spec
    self.act = spec.act_code     # the model's activation
    self.bn_momentum, self.bn_epsilon = spec.bn_momentum, spec.bn_epsilon
    self.update = update
    self.device = torch.device(device)
    torch.cuda.set_device(self.device)
    self.dtype = EDET_BF16 if dtype in ('bf16', EDET_BF16) else EDET_F32
    self.tdtype = torch.bfloat16 if self.dtype == EDET_BF16 else torch.float32
    self.batch = batch_size
    self.image_size = utils.parse_image_size(image_size)
    self._bufs = {}
    self._zero_list = []
    self._zfree, self._zcur = 0, None
    self.tape = []
    self.training = False
    self._nparts = ctypes.c_int(0)
    self._cast_version = -1
    self._build_params(params, seed, arena)
    # batched weight-gradient reductions (see _ws); False = one reduction launch per layer, as in round 3 (the tests
    # compare both forms)
    self.defer_reduce = True
    self._deferring = False
    self._defer_streams = set()
    self._main = self._branch = self._new_branch()      # the chain the primitives work on, unless a network forks another
    self.bns = {}
    self.hyper = torch.zeros(4, dtype=torch.float32, device=self.device)   # lr, ema decay, 1/normalizer, -
    self.gnorm = torch.zeros(1, dtype=torch.float32, device=self.device)
    self.stochastic_depth = stochastic_depth
    self._cast_items = {}      # weight name -> descriptors of its compute copies (filled by the first pass)
    self._cast_table = None
    self._f32_island = False
    # head of an MBConv block (expansion -> BatchNorm -> activation -> depthwise) in one kernel where the library has one
    # (mbconv_fused.hip: bf16, <= 32 block-input channels): the expanded tensor is not read back by the depthwise
    # convolution -- and never stored at all in inference (always on; bench.py reports it)
    self.fused_mbconv_head = True
    self.fused_heads = set()     # block scopes whose head ran fused in the last forward pass (inference: no ':exp' tensor)
    # cross-replica BatchNorm (utils.SyncBatchNormalization / TpuBatchNormalization, utils.py:166-241):
    # (all_reduce_fn, world_size) or None.  Set by train_lib when sync_bn=True.
    self.sync_bn = None
    self.bn_bessel = True        # Keras fused BatchNorm: Bessel-corrected batch variance into moving_variance
    self.drop_masks = {}      # block scope -> (mask [n,c] fp32 = floor(p + u_n) / p, survival probability p)
    self._rng = torch.Generator(device=self.device)
    self._rng.manual_seed(1000003 * seed + 17)

  @property
  def adam(self):
    return self.update.kind == 'adam'

  @property
  def esize(self):
    return 2 if self.dtype == EDET_BF16 else 4

  # ------------------------------------------------------------------ memory
  @property
  def stream(self):
    return torch.cuda.current_stream(self.device).cuda_stream

  @property
  def partials(self):
    return self._branch.partials

  def _new_branch(self, stream=None, grads=None):
    """A chain's own BatchNorm partial rows and 256 MiB of weight-gradient workspace (deferred reductions, see _ws)."""
    cmax = max([p.shape[0] for p in self.spec.params if len(p.shape) == 1] + [64])
    return Branch(stream, torch.empty(_lib.MAX_PARTS * 2 * cmax, dtype=torch.float32, device=self.device),
                  torch.empty(64 * 1024 * 1024, dtype=torch.float32, device=self.device), grads)

  # ---- deferred weight-gradient reductions (edet_reduce_defer): the backward pass records the ~190 "dW += partial sums"
  # of a step and adds them in a handful of batched launches; until a flush every call gets the workspace BEHIND the
  # partial sums still waiting there
  WS_RESERVE = 64 * 1024 * 1024       # what a single call may need (the round-3 workspace size)

  def _ws(self):
    """(pointer, bytes) of the free part of the current chain's workspace."""
    b = self._branch
    return b.workspace.data_ptr() + b.ws_off, b.workspace.numel() * 4 - b.ws_off

  def _ws_mark(self):
    """After a call that may have left partial sums for a deferred reduction: the next call starts behind them."""
    if not self._deferring:
      return
    b = self._branch
    hi = ctypes.c_void_p()
    call('edet_reduce_deferred_end', self.stream, ctypes.byref(hi))
    if hi.value:
      b.ws_off = (hi.value - b.workspace.data_ptr() + 255) // 256 * 256
      if b.workspace.numel() * 4 - b.ws_off < self.WS_RESERVE:
        call('edet_reduce_flush', self.stream)
        b.ws_off = 0

  def _defer_begin(self):
    if self.defer_reduce and not self._deferring:
      self._deferring = True
      self._defer_streams = set()
    if self._deferring and self.stream not in self._defer_streams:
      call('edet_reduce_defer', self.stream, 1)
      self._defer_streams.add(self.stream)

  def _defer_end(self):
    """Flushes what the current chain recorded and returns its stream to the immediate mode."""
    if self._deferring and self.stream in self._defer_streams:
      call('edet_reduce_defer', self.stream, 0)
      self._defer_streams.discard(self.stream)
      self._branch.ws_off = 0
      if not self._defer_streams:
        self._deferring = False

  def buf(self, key, shape, dtype):
    t = self._bufs.get(key)
    if t is None:
      t = torch.empty(shape, dtype=dtype, device=self.device)
      self._bufs[key] = t
    assert tuple(t.shape) == tuple(shape), (key, tuple(t.shape), tuple(shape))
    return t

  ZCHUNK = 4 * 1024 * 1024      # floats per zero-arena chunk (16 MiB)

  def zbuf(self, key, shape):
    """fp32 buffer that is zeroed at the start of every step: the kernels ADD into it, in a fixed order and without
    atomics (SE pooled sums; gate gradients, which k_gate_sums / k_gate_finish add into; fusion-weight gradients, loss
    sums).  Carved out of a few large chunks so that the ~60 buffers of a
    step cost one fill launch per chunk instead of one each."""
    t = self._bufs.get(key)
    if t is None:
      n = int(np.prod(shape))
      padded = (n + 63) // 64 * 64                   # every buffer starts 256-byte aligned
      if padded > self.ZCHUNK:
        chunk = torch.zeros(padded, dtype=torch.float32, device=self.device)
        self._zero_list.append(chunk)
        t = chunk[:n].view(shape)
      else:
        if self._zcur is None or self._zfree + padded > self.ZCHUNK:
          self._zero_list.append(torch.zeros(self.ZCHUNK, dtype=torch.float32, device=self.device))
          self._zfree = 0
          self._zcur = self._zero_list[-1]
        t = self._zcur[self._zfree:self._zfree + n].view(shape)
        self._zfree += padded
      self._bufs[key] = t
    return t

  def _build_params(self, params, seed, arena):
    if arena is None:
      values = params if params is not None else netspec_lib.init_params(self.spec, seed)
      if any(p.name not in values for p in self.spec.params):
        # a partial set (e.g. a checkpoint restored with skip_mismatch): the other variables keep their initial values
        values = {**netspec_lib.init_params(self.spec, seed), **values}
      arena = ParamArena(self.spec, self.device, values)
    self.arena = arena
    for k in ('offsets', 'n_train_elems', 'seg_names', 'params_flat', 'grads_flat', 'velocity', 'ema', 'state_flat',
              'seg_offsets', 'seg_flags', 'nseg', 'seg_sqnorm', 'seg_factor'):
      setattr(self, k, getattr(arena, k))

  def param(self, name):
    return self.arena.param(name)

  def grad(self, name):
    """Gradient slice of a variable in the arena the current chain accumulates into (Branch.grads)."""
    if self._branch.grads is not None:
      off, n, _, tr = self.offsets[name]
      assert tr, name
      return self._branch.grads[off:off + n]
    return self.arena.grad(name)

  def set_params(self, values):
    """values: name -> array-like in reference layouts."""
    self.arena.set_params(values)

  def get_params(self, names=None):
    return self.arena.get_params(names)

  def get_grads(self):
    return {name: self.grad(name).detach().cpu().numpy().reshape(self.offsets[name][2])
            for name in self.seg_names}

  # ------------------------------------------------------------------ compute copies of 1x1 kernels
  def _pw_copies(self, name, cin, cout):
    """(Wt [cout][ldk], ldk, W [cin][ldn], ldn) compute-dtype copies of an HWIO 1x1 kernel."""
    ldk, ldn = _pad8(cin), _pad8(cout)
    sfx = ':f32' if self._f32_island else ''      # fp32 copies of a layer that runs in fp32 inside a bf16 engine
    wt = self.buf('wt:' + name + sfx, (cout, ldk), self.tdtype)
    w = self.buf('w:' + name + sfx, (cin, ldn), self.tdtype)
    if name + sfx not in self._cast_done:
      src = ptr(self.param(name))
      call('edet_cast_matrix', src, ptr(wt), cin, cout, ldk, 1, self.dtype, self.stream)
      call('edet_cast_matrix', src, ptr(w), cin, cout, ldn, 0, self.dtype, self.stream)
      self._cast_done.add(name + sfx)
      if not sfx:        # (the batched re-cast of a step makes the engine's own compute type only)
        self._cast_items[name] = [(src, ptr(wt), cin, cout, ldk, 1), (src, ptr(w), cin, cout, ldn, 0)]
    return wt, ldk, w, ldn

  @contextlib.contextmanager
  def _fp32_island(self):
    """Layers built inside run through the fp32 kernels of the library although the engine stores bf16 (their inputs
    must be fp32 tensors: _to_f32).  Inference only -- the detection box-predict layer, engine.Engine._head_level."""
    saved = (self.dtype, self.tdtype, self._f32_island)
    self.dtype, self.tdtype, self._f32_island = EDET_F32, torch.float32, True
    try:
      yield
    finally:
      self.dtype, self.tdtype, self._f32_island = saved

  def _to_f32(self, key, v):
    """fp32 copy of a stored tensor, same view (BatchNorm / activation are applied on load by the fp32 kernels)."""
    r = v.raw
    out = Raw(self, key, r.n, r.h, r.w, r.c, r.ld, needs_grad=False, dtype=torch.float32)
    call('edet_cast_to_f32', ptr(r.data), ptr(out.data), r.data.numel(), EDET_BF16 if r.data.dtype == torch.bfloat16 else EDET_F32,
         self.stream)
    return View(out, v.bn, v.act, v.gate)

  def _cast_all(self):
    """Every compute copy recorded by an earlier pass, re-made in one launch (edet_cast_batch)."""
    names = list(self._cast_items)
    if self._cast_table is None or self._cast_table[0] != names:
      if torch.cuda.is_current_stream_capturing():
        return                 # no host-to-device copy inside a capture: this pass casts layer by layer
      import struct
      flat = [it for n in names for it in self._cast_items[n]]
      raw = b''.join(struct.pack('<QQiiii', s or 0, d, r, c, ld, t) for (s, d, r, c, ld, t) in flat)
      dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
      biggest = max((t and c or r) * ld for (_, _, r, c, ld, t) in flat)
      self._cast_table = (names, dev, len(flat), max(1, min(64, (biggest + 255) // 256)))
    _, dev, count, blocks = self._cast_table
    call('edet_cast_batch', ptr(dev), count, blocks, self.dtype, self.stream)
    self._cast_done.update(names)

  # ------------------------------------------------------------------ BatchNorm plumbing
  def get_bn(self, name, c):
    bn = self.bns.get(name)
    if bn is None:
      bn = BN(self, name, c)
      self.bns[name] = bn
    return bn

  def _sync_partials(self, nparts, c):
    """Cross-replica sum of the [nparts][2][c] partial rows -> one row at partials[0:2c] (every replica
    normalises with the statistics of the GLOBAL batch: mean of the shard means / mean squares over equal
    shards, utils.py:176-195,215-241).  Returns the local sums."""
    reduce_fn, _ = self.sync_bn
    local = self.partials[:nparts * 2 * c].view(nparts, 2 * c).sum(0)
    total = local.clone()
    reduce_fn(total)
    self.partials[:2 * c].copy_(total)
    return local

  def _bn_forward(self, bn, count, nparts):
    if self.training:
      if self.sync_bn is not None:
        self._sync_partials(nparts, bn.c)
        nparts, count = 1, count * self.sync_bn[1]
      bn.count = count
      call('edet_bn_finalize', ptr(self.partials), nparts, bn.c, float(count), ptr(bn.gamma), ptr(bn.beta),
           self.bn_epsilon, self.bn_momentum if self.update_moving else -1.0, 1 if (self.bn_bessel and self.sync_bn is None) else 0,
           ptr(bn.mm), ptr(bn.mv), ptr(bn.scale), ptr(bn.shift), ptr(bn.mean), ptr(bn.rstd), self.stream)
      bn.bwd_ready = False
      bn.eval_done = False
      self.arena.version += 1          # moving statistics (and soon the weights) change
    elif not bn.eval_done:
      call('edet_bn_eval', bn.c, ptr(bn.gamma), ptr(bn.beta), self.bn_epsilon, ptr(bn.mm), ptr(bn.mv),
           ptr(bn.scale), ptr(bn.shift), self.stream)
      bn.eval_done = True

  def _bn_bwd_finalize(self, bn, nparts):
    dgamma, dbeta = ptr(bn.dgamma), ptr(bn.dbeta)
    if self.sync_bn is not None:
      # gamma / beta gradients from the LOCAL sums (the gradient all-reduce adds the replicas up), the
      # on-load coefficients (a, b, cc) from the GLOBAL sums over the global count
      call('edet_bn_bwd_finalize', ptr(self.partials), nparts, bn.c, float(bn.count), ptr(bn.gamma),
           ptr(bn.mean), ptr(bn.rstd), dgamma, dbeta, None, ptr(bn.a), ptr(bn.b), ptr(bn.cc), self.stream)
      self._sync_partials(nparts, bn.c)
      nparts, dgamma, dbeta = 1, None, None
    call('edet_bn_bwd_finalize', ptr(self.partials), nparts, bn.c, float(bn.count), ptr(bn.gamma),
         ptr(bn.mean), ptr(bn.rstd), dgamma, dbeta, None, ptr(bn.a), ptr(bn.b), ptr(bn.cc),
         self.stream)
    bn.bwd_ready = True

  def _ensure_bn_bwd(self, v):
    """Make the on-load BatchNorm-backward coefficients of view v available (multi-consumer case)."""
    if v.bn is None or v.bn.bwd_ready:
      return
    r = v.raw
    call('edet_bn_bwd_reduce', ptr(r.grad), ptr(r.data), r.rows, r.c, r.ld, ptr(v.bn.mean), ptr(v.bn.rstd),
         ptr(self.partials), ctypes.byref(self._nparts), self.dtype, self.stream)
    self._bn_bwd_finalize(v.bn, self._nparts.value)

  def _gview(self, v):
    """dy of the conv that produced v.raw, as an on-load gradient view."""
    self._ensure_bn_bwd(v)
    r = v.raw
    if v.bn is not None:
      return GView(ptr(r.grad), ptr(r.data), ptr(v.bn.a), ptr(v.bn.b), ptr(v.bn.cc), r.n, r.h, r.w, r.c, r.ld)
    return GView(ptr(r.grad), None, None, None, None, r.n, r.h, r.w, r.c, r.ld)

  def _epi(self, vin, dgate=None):
    """Epilogue descriptor for writing d(vin) into vin.raw.grad; returns (epi, fused_stats)."""
    r = vin.raw
    g = r.ensure_grad()
    beta = 1 if r.grad_written else 0
    fused = (vin.bn is not None and vin.consumers == 1 and vin.gate is None and beta == 0)
    epi = BwdEpi(ptr(g), beta,
                 ptr(vin.bn.mean) if fused else None, ptr(vin.bn.rstd) if fused else None,
                 ptr(self.partials) if fused else None, ptr(dgate))
    return epi, fused

  # ------------------------------------------------------------------ layers
  def pw(self, key, vin, wname, cout, bias=None, bn=None, act=ACT_NONE, ld=None, f32out=False, bias_grad=False):
    """1x1 conv (+bias) [-> BN -> act as a view].  f32out (inference, bf16 storage): the output is stored as fp32 --
    the class / box logits, whose bf16 rounding alone is 3e-3 of their range (engine.Engine._head_level)."""
    r = vin.raw
    cin = r.c
    wt, ldk, w, ldn = self._pw_copies(wname, cin, cout)
    if f32out and not self.training and self.dtype == EDET_BF16 and bn is None:
      out = Raw(self, key + ':f32', r.n, r.h, r.w, cout, ld, needs_grad=False, dtype=torch.float32)
      call('edet_pw_fwd_f32out', ctypes.byref(vin.tview()), ptr(wt), ldk, ptr(self.param(bias)) if bias else None,
           ptr(out.data), cout, out.ld, self.stream, nbytes=r.rows * (cin * 2 + cout * 4),
           tag='%dx%dx%d->%d f32' % (r.h, r.w, cin, cout))
      vin.consumers += 1
      return View(out, None, act)
    out = Raw(self, key, r.n, r.h, r.w, cout, ld)
    bnl = self.get_bn(bn, cout) if bn else None
    stats = ptr(self.partials) if (bnl and self.training) else None
    call('edet_pw_fwd', ctypes.byref(vin.tview()), ptr(wt), ldk, ptr(self.param(bias)) if bias else None,
         ptr(out.data), cout, out.ld, stats, ctypes.byref(self._nparts), self.dtype, self.stream,
         nbytes=r.rows * (cin + cout) * self.esize, tag='%dx%dx%d->%d' % (r.h, r.w, cin, cout))
    if bnl:
      self._bn_forward(bnl, out.rows, self._nparts.value)
    vout = View(out, bnl, act)
    vin.consumers += 1
    if self.training:
      self.tape.append(lambda: self._pw_bwd(vin, vout, wname, w, ldn, bias is None))
      if bias_grad and bias and bnl is None:
        self.tape.append(lambda: self._bias_grad(vout, bias))      # (replayed BEFORE _pw_bwd: the gradient is complete by then)
    return vout

  def _bias_grad(self, vout, bias):
    """d(bias) += column sums of the output gradient, for a biased convolution with NO BatchNorm behind it that is not a
    predict layer (those get theirs from the loss kernels; behind a BatchNorm the gradient is analytically zero): the
    resample convolutions under apply_bn_for_resampling=False.  The BatchNorm-backward pair with mean 0 / rstd 1 / gamma 1:
    its dbeta is exactly that sum."""
    r = vout.raw
    assert r.grad is not None and r.grad_written, 'bias gradient of %s before its output gradient is complete' % bias
    # main chain only: the constant vector is filled once, on the stream that is current at its creation, and nothing
    # orders a later reader on ANOTHER stream against that fill (the resample convolutions are BiFPN layers)
    assert self._branch is self._main, 'bias gradient of %s on the side chain' % bias
    fresh = ('ones:c:%d' % r.c) not in self._bufs
    ones = self.buf('ones:c:%d' % r.c, (r.c,), torch.float32)
    if fresh:
      ones.fill_(1.0)          # (once, at creation: not a launch of every replayed step)
    zeros = self.zbuf('zeros:c:%d' % r.c, (r.c,))
    scr = self.buf('biasgrad:scr:%d' % r.c, (3, r.c), torch.float32)
    call('edet_bn_bwd_reduce', ptr(r.grad), ptr(r.data), r.rows, r.c, r.ld, ptr(zeros), ptr(ones), ptr(self.partials),
         ctypes.byref(self._nparts), self.dtype, self.stream)
    call('edet_bn_bwd_finalize', ptr(self.partials), self._nparts.value, r.c, float(r.rows), ptr(ones), ptr(zeros),
         ptr(ones), None, ptr(self.grad(bias)), None, ptr(scr[0]), ptr(scr[1]), ptr(scr[2]), self.stream)

  def _pw_bwd(self, vin, vout, wname, w, ldn, no_bias=False):
    g = self._gview(vout)
    nb = vin.raw.rows * (vin.raw.c + vout.raw.c) * self.esize
    tag = '%dx%dx%d->%d' % (vin.raw.h, vin.raw.w, vin.raw.c, vout.raw.c)
    if vin.raw.needs_grad:
      # both gradients in one call: one pass over (dz, y, x) where the layer fits the fused kernel
      dgate = vin.dgate if vin.gate is not None else None
      epi, fused = self._epi(vin, dgate)
      if no_bias:
        epi.flags = _lib.EPI_Y_IS_CONV_OF_INPUT      # y = view(x) W exactly: the library need not read it
      call('edet_pw_bwd', ctypes.byref(g), ptr(w), ldn, ctypes.byref(vin.tview()), ctypes.byref(epi),
           ctypes.byref(self._nparts), ptr(self.grad(wname)), *self._ws(),
           self.dtype, self.stream, nbytes=2 * nb, tag=tag)
      self._ws_mark()
      vin.raw.grad_written = True
      if fused:
        self._bn_bwd_finalize(vin.bn, self._nparts.value)
      return
    call('edet_pw_bwd_weight', ctypes.byref(vin.tview()), ctypes.byref(g), ptr(self.grad(wname)),
         *self._ws(), self.dtype, self.stream, nbytes=nb, tag=tag)
    self._ws_mark()

  def conv(self, key, vin, wname, k, stride, cout, bn=None, act=ACT_NONE):
    """Dense k x k convolution, TF 'SAME', no bias [-> BN -> act as a view] (Fused-MBConv,
    efficientnetv2/effnetv2_model.py:338-346,362-371).  Forward only: the V2 classifier's training
    is outside the hot path, so the tape entry refuses to run."""
    r = vin.raw
    cin = r.c
    if cin % 8 != 0 or r.ld != cin:
      raise ValueError('dense convolution needs an input channel count divisible by 8, got %d' % cin)
    kk = k * k * cin
    wt = self.buf('wtc:' + wname, (cout, kk), self.tdtype)
    if wname not in self._cast_done:
      call('edet_cast_matrix', ptr(self.param(wname)), ptr(wt), kk, cout, kk, 1, self.dtype, self.stream)
      self._cast_done.add(wname)
    oh, _, _ = utils.same_padding(r.h, k, stride)
    ow, _, _ = utils.same_padding(r.w, k, stride)
    out = Raw(self, key, r.n, oh, ow, cout)
    bnl = self.get_bn(bn, cout) if bn else None
    stats = ptr(self.partials) if (bnl and self.training) else None
    call('edet_conv_fwd', ctypes.byref(vin.tview()), ptr(wt), kk, k, stride, ptr(out.data), cout, out.ld,
         stats, ctypes.byref(self._nparts), self.dtype, self.stream,
         nbytes=(r.rows * cin + out.rows * cout) * self.esize,
         tag='%dx%dx%d->%d k%ds%d' % (r.h, r.w, cin, cout, k, stride))
    if bnl:
      self._bn_forward(bnl, out.rows, self._nparts.value)
    vout = View(out, bnl, act)
    vin.consumers += 1
    if self.training:
      self.tape.append(lambda: self._conv_bwd(vin, vout, wname, k, stride, cin, cout))
    return vout

  def _conv_bwd(self, vin, vout, wname, k, stride, cin, cout):
    """Both gradients of a dense convolution (edet_conv_bwd_weight / edet_conv_bwd_data)."""
    g = self._gview(vout)
    nb = (vin.raw.rows * cin + vout.raw.rows * cout) * self.esize
    tag = '%dx%dx%d->%d k%ds%d' % (vin.raw.h, vin.raw.w, cin, cout, k, stride)
    call('edet_conv_bwd_weight', ctypes.byref(vin.tview()), ctypes.byref(g), k, stride, ptr(self.grad(wname)),
         *self._ws(), self.dtype, self.stream, nbytes=nb, tag=tag)
    self._ws_mark()
    if vin.raw.needs_grad:
      # compute copy for the data gradient: HWIO -> [cin][k][k][cout] (reduction index (tap, co) contiguous)
      wperm = self.buf('wtd:' + wname, (cin, k * k * cout), self.tdtype)
      wperm.copy_(self.param(wname).view(k, k, cin, cout).permute(2, 0, 1, 3).reshape(cin, k * k * cout))
      epi, fused = self._epi(vin)
      call('edet_conv_bwd_data', ctypes.byref(g), ptr(wperm), k * k * cout, k, stride, ctypes.byref(vin.tview()),
           ctypes.byref(epi), ctypes.byref(self._nparts), self.dtype, self.stream, nbytes=nb, tag=tag)
      vin.raw.grad_written = True
      if fused:
        self._bn_bwd_finalize(vin.bn, self._nparts.value)

  def dw(self, key, vin, wname, k, stride, bn=None, act=ACT_NONE):
    r = vin.raw
    oh, _, _ = utils.same_padding(r.h, k, stride)
    ow, _, _ = utils.same_padding(r.w, k, stride)
    out = Raw(self, key, r.n, oh, ow, r.c)
    bnl = self.get_bn(bn, r.c) if bn else None
    stats = ptr(self.partials) if (bnl and self.training) else None
    wp = ptr(self.param(wname))
    call('edet_dw_fwd', ctypes.byref(vin.tview()), wp, k, stride, ptr(out.data), out.ld, stats,
         ctypes.byref(self._nparts), self.dtype, self.stream, nbytes=(r.rows + out.rows) * r.c * self.esize,
         tag='%dx%dx%d k%ds%d' % (r.h, r.w, r.c, k, stride))
    if bnl:
      self._bn_forward(bnl, out.rows, self._nparts.value)
    vout = View(out, bnl, act)
    vin.consumers += 1
    if self.training:
      self.tape.append(lambda: self._dw_bwd(vin, vout, wname, k, stride))
    return vout

  def _dw_bwd(self, vin, vout, wname, k, stride):
    g = self._gview(vout)
    nb = (vin.raw.rows + vout.raw.rows) * vin.raw.c * self.esize
    tag = '%dx%dx%d k%ds%d' % (vin.raw.h, vin.raw.w, vin.raw.c, k, stride)
    if not vin.raw.needs_grad:
      call('edet_dw_bwd_weight', ctypes.byref(vin.tview()), ctypes.byref(g), k, stride, ptr(self.grad(wname)),
           *self._ws(), self.dtype, self.stream, nbytes=nb, tag=tag)
      self._ws_mark()
      return
    # both gradients in one call (bf16: ONE kernel, any stride)
    epi, fused = self._epi(vin)
    call('edet_dw_bwd', ctypes.byref(g), ptr(self.param(wname)), k, stride, ctypes.byref(vin.tview()),
         ctypes.byref(epi), ctypes.byref(self._nparts), ptr(self.grad(wname)), *self._ws(), self.dtype, self.stream, nbytes=2 * nb, tag=tag)
    self._ws_mark()
    vin.raw.grad_written = True
    if fused:
      self._bn_bwd_finalize(vin.bn, self._nparts.value)

  def se(self, key, v, scope, se_filters):
    """Squeeze-and-excitation: returns the gated view of v (efficientnet_model.py:183-195)."""
    r = v.raw
    n, c = r.n, r.c
    inv_hw = 1.0 / (r.h * r.w)
    pooled = self.buf(key + ':pool', (n, c), torch.float32)
    hidden = self.buf(key + ':hid', (n, se_filters), torch.float32)
    gate = self.buf(key + ':gate', (n, c), torch.float32)
    w1, b1 = scope + '/se/conv2d/kernel', scope + '/se/conv2d/bias'
    w2, b2 = scope + '/se/conv2d_1/kernel', scope + '/se/conv2d_1/bias'
    # pooling (chunk sums in the BatchNorm partial-row scratch, free between two layers) + both 1x1 layers; no atomics,
    # batch-independent summation order
    call('edet_se_squeeze_excite', ctypes.byref(v.tview()), ptr(self.partials), self.partials.numel() * 4,
         se_filters, inv_hw, ptr(self.param(w1)), ptr(self.param(b1)), ptr(self.param(w2)), ptr(self.param(b2)),
         ptr(pooled), ptr(hidden), ptr(gate), v.act, self.dtype, self.stream, nbytes=r.rows * c * self.esize)
    vg = View(r, v.bn, v.act, gate)
    vg.dgate = self.zbuf(key + ':dgate', (n, c)) if self.training else None
    v.consumers += 1
    if self.training:
      dpool = self.buf(key + ':dpool', (n, c), torch.float32)
      scratch = self.buf(key + ':scr', (_lib.se_bwd_scratch_floats(n, c, se_filters),), torch.float32)

      def bwd():
        call('edet_se_fc_bwd', ptr(pooled), ptr(hidden), ptr(gate), ptr(vg.dgate), n, c, se_filters, inv_hw,
             ptr(self.param(w1)), ptr(self.param(w2)), ptr(self.grad(w1)), ptr(self.grad(b1)),
             ptr(self.grad(w2)), ptr(self.grad(b2)), ptr(dpool), ptr(scratch), v.act, self.stream)
        call('edet_se_gate_bwd', ctypes.byref(vg.tview()), ptr(r.grad), ptr(dpool), ptr(v.bn.mean),
             ptr(v.bn.rstd), ptr(self.partials), ctypes.byref(self._nparts), self.dtype, self.stream,
             nbytes=2 * r.rows * c * self.esize)
        self._bn_bwd_finalize(v.bn, self._nparts.value)

      self.tape.append(bwd)
    return vg

  def drop_rng_state(self):
    """The state of the generator behind the stochastic-depth draws (uint8 numpy, 16 bytes: seed and offset), for a
    training-state file; set_drop_rng_state puts it back, so the next refresh_drop_masks draws what it would have drawn."""
    return self._rng.get_state().cpu().numpy().copy()

  def set_drop_rng_state(self, state):
    self._rng.set_state(torch.as_tensor(np.asarray(state, dtype=np.uint8)))

  def refresh_drop_masks(self):
    """New stochastic-depth draws: mask[n, :] = floor(p + u_n) / p, u_n ~ U[0,1) per image
    (utils.drop_connect, utils.py:329-344).  Device-side torch ops, outside any captured graph."""
    for mask, p in self.drop_masks.values():
      u = torch.rand(mask.shape[0], 1, device=self.device, generator=self._rng)
      mask.copy_(((u + p).floor() / p).expand_as(mask))

  def bn_res(self, key, vy, residual, survival_prob=None):
    """Materialise a block output: bn(y) [* stochastic-depth scale] (+ residual)."""
    r = vy.raw
    if residual is not None and (residual.bn is not None or residual.act != ACT_NONE or residual.gate is not None):
      raise ValueError('bn_res: the residual operand must be a stored (plain) tensor')
    out = Raw(self, key, r.n, r.h, r.w, r.c)
    mask = None
    if self.training and self.stochastic_depth and survival_prob and residual is not None:
      if key not in self.drop_masks:
        self.drop_masks[key] = (self.buf(key + ':dc', (r.n, r.c), torch.float32), float(survival_prob))
        if not torch.cuda.is_current_stream_capturing():
          saved = self.drop_masks
          self.drop_masks = {key: saved[key]}
          self.refresh_drop_masks()
          self.drop_masks = saved
      mask = self.drop_masks[key][0]
      vy.consumers += 1
      vy = View(r, vy.bn, vy.act, mask)
    call('edet_bn_res', ctypes.byref(vy.tview()), ptr(residual.raw.data) if residual else None, ptr(out.data),
         out.ld, self.dtype, self.stream, nbytes=(3 if residual else 2) * r.rows * r.c * self.esize)
    vout = View(out)
    vy.consumers += 1
    if residual is not None:
      residual.consumers += 1
    if self.training:
      act_view = vy.act != ACT_NONE

      def bwd():
        assert out.grad_written, key
        if act_view:
          # out = act(bn(y)) [* mask] (+ residual): the residual takes d(out) as it is, then d(out) becomes
          # dz = d(out) * mask * act'(z) in place (edet_se_gate_bwd with gate = mask or ones, dpool = 0), which
          # also yields the BatchNorm-backward sums of y's BatchNorm
          if residual is not None and residual.raw.needs_grad:
            rr = residual.raw
            call('edet_add', ptr(rr.ensure_grad()), ptr(out.grad), rr.rows, rr.c, rr.ld,
                 1 if rr.grad_written else 0, self.dtype, self.stream)
            rr.grad_written = True
          ones = mask if mask is not None else self.buf('ones:%d:%d' % (r.n, r.c), (r.n, r.c), torch.float32)
          if mask is None:
            ones.fill_(1.0)
          zeros = self.zbuf('zeros:%d:%d' % (r.n, r.c), (r.n, r.c))
          gv = TView(ptr(r.data), ptr(vy.bn.scale), ptr(vy.bn.shift), ptr(ones), vy.act, r.n, r.h, r.w, r.c, r.ld)
          call('edet_se_gate_bwd', ctypes.byref(gv), ptr(out.grad), ptr(zeros), ptr(vy.bn.mean), ptr(vy.bn.rstd),
               ptr(self.partials), ctypes.byref(self._nparts), self.dtype, self.stream,
               nbytes=2 * r.rows * r.c * self.esize)
          self._bn_bwd_finalize(vy.bn, self._nparts.value)
          r.grad = out.grad
          r.grad_written = True
          return
        if mask is not None:
          # d(bn output) = d(block output) * mask[n]: the same kernel, applied to the gradient
          gbuf = self.buf(key + ':dcg', (r.n, r.h, r.w, r.ld), self.tdtype)
          gv = TView(ptr(out.grad), None, None, ptr(mask), ACT_NONE, r.n, r.h, r.w, r.c, out.ld)
          call('edet_bn_res', ctypes.byref(gv), None, ptr(gbuf), r.ld, self.dtype, self.stream,
               nbytes=2 * r.rows * r.c * self.esize)
          r.grad = gbuf
        else:
          r.grad = out.grad         # d(bn output) aliases d(block output)
        r.grad_written = True
        if residual is not None and residual.raw.needs_grad:
          rr = residual.raw
          call('edet_add', ptr(rr.ensure_grad()), ptr(out.grad), rr.rows, rr.c, rr.ld,
               1 if rr.grad_written else 0, self.dtype, self.stream)
          rr.grad_written = True
      self.tape.append(bwd)
    return vout

  # ------------------------------------------------------------------ a pass: begin, shared blocks, backward
  def _begin(self, training, update_moving=True):
    self.training = training
    self.update_moving = update_moving
    self.tape = []
    self.fused_heads = set()
    # compute copies of the kernels and the inference BatchNorm vectors are rebuilt only when a variable
    # changed since they were made (every training step; in inference only after set_params)
    if self._cast_version != self.arena.version:
      self._cast_done = set()
      if self._cast_items:           # every compute copy of a step in one edet_cast_batch launch
        self._cast_all()
      for bn in self.bns.values():
        bn.eval_done = False
      self._cast_version = self.arena.version
    for bn in self.bns.values():
      bn.bwd_ready = False
    for t in self._zero_list:      # buffers the kernels add into (SE pooled sums, gate gradients, ...) start every pass at zero
      call('edet_zero', ptr(t), t.numel() * 4, self.stream)
    if training:
      call('edet_zero', ptr(self.grads_flat), self.grads_flat.numel() * 4, self.stream)

  def stem(self, name_prefix, images, act):
    """The stem: images [B,H,W,3] (device tensor, engine dtype) -> 3x3 stride-2 convolution -> BatchNorm -> act as a view.
    Variables: name_prefix + '/stem/conv2d/kernel', name_prefix + '/stem/tpu_batch_normalization'."""
    n, (h, w), cout = self.batch, self.image_size, self.spec.stem_filters
    assert tuple(images.shape) == (n, h, w, 3), images.shape
    assert images.dtype == self.tdtype and images.is_contiguous()
    self.images = images
    oh, _, _ = utils.same_padding(h, 3, 2)
    ow, _, _ = utils.same_padding(w, 3, 2)
    y0 = Raw(self, 'stem', n, oh, ow, cout)
    bn0 = self.get_bn(name_prefix + '/stem/tpu_batch_normalization', cout)
    wstem = name_prefix + '/stem/conv2d/kernel'
    nbytes = (n * h * w * 3 + y0.rows * y0.c) * self.esize
    call('edet_stem_fwd', ptr(images), n, h, w, ptr(self.param(wstem)), ptr(y0.data), cout, y0.ld,
         ptr(self.partials) if self.training else None, ctypes.byref(self._nparts), self.dtype, self.stream, nbytes=nbytes)
    self._bn_forward(bn0, y0.rows, self._nparts.value)
    v0 = View(y0, bn0, act)
    if self.training:
      def stem_bwd():
        g = self._gview(v0)
        # behind the partial sums that earlier layers left for the deferred reductions (_ws / _ws_mark)
        call('edet_stem_bwd_weight', ptr(images), n, h, w, ctypes.byref(g), ptr(self.grad(wstem)), *self._ws(), self.dtype,
             self.stream, nbytes=nbytes)
        self._ws_mark()
      self.tape.append(stem_bwd)
    return v0

  def _mbconv(self, xin, b, scope):
    cexp = b.input_filters * b.expand_ratio
    bn_names = ['tpu_batch_normalization', 'tpu_batch_normalization_1', 'tpu_batch_normalization_2']
    conv_names = ['conv2d', 'conv2d_1']
    bi = ci = 0
    x = xin
    if b.expand_ratio != 1 and self._mbconv_head_fusable(x, cexp, b.kernel_size, b.stride):
      x = self.mbconv_head(scope, x, '%s/%s/kernel' % (scope, conv_names[ci]), cexp, '%s/%s' % (scope, bn_names[bi]),
                           scope + '/depthwise_conv2d/depthwise_kernel', b.kernel_size, b.stride,
                           '%s/%s' % (scope, bn_names[bi + 1]))
      ci += 1
      bi += 2
    else:
      if b.expand_ratio != 1:
        x = self.pw(scope + ':exp', x, '%s/%s/kernel' % (scope, conv_names[ci]), cexp,
                    bn='%s/%s' % (scope, bn_names[bi]), act=self.act)
        ci += 1
        bi += 1
      x = self.dw(scope + ':dw', x, scope + '/depthwise_conv2d/depthwise_kernel', b.kernel_size, b.stride,
                  bn='%s/%s' % (scope, bn_names[bi]), act=self.act)
      bi += 1
    if b.se_filters:
      x = self.se(scope + ':se', x, scope, b.se_filters)
    y = self.pw(scope + ':proj', x, '%s/%s/kernel' % (scope, conv_names[ci]), b.output_filters,
                bn='%s/%s' % (scope, bn_names[bi]), act=ACT_NONE)
    return self.bn_res(scope + ':out', y, xin if b.has_residual else None,
                       survival_prob=self.spec.survival_probs[b.index])

  def _mbconv_head_fusable(self, vin, cexp, k, stride):
    if self.dtype != EDET_BF16 or self.act == ACT_NONE:
      return False
    return _lib.load().edet_mbconv_fused_supported(ctypes.byref(vin.tview()), cexp, k, stride, self.dtype) == 1

  def mbconv_head(self, scope, vin, wexp, cexp, bn_exp, wdw, k, stride, bn_dw):
    """x = act(bn0(expand_conv(x))); x = act(bn1(depthwise_conv(x))) (efficientnet_model.py:378-392) through
    edet_mbconv_expand_dw_fwd.  Training: the expansion's batch statistics first (edet_mbconv_expand_stats, the block
    input only), the raw expanded tensor stored for the backward pass, whose tape entries are those of the two-kernel
    path (pw, dw).  Inference: the expanded tensor is never stored."""
    r = vin.raw
    cin = r.c
    self.fused_heads.add(scope)
    wt, ldk, w, ldn = self._pw_copies(wexp, cin, cexp)
    bne, bnd = self.get_bn(bn_exp, cexp), self.get_bn(bn_dw, cexp)
    oh, _, _ = utils.same_padding(r.h, k, stride)
    ow, _, _ = utils.same_padding(r.w, k, stride)
    tv = vin.tview()
    tag = '%dx%dx%d->%d k%ds%d' % (r.h, r.w, cin, cexp, k, stride)
    e_raw = None
    if self.training:
      e_raw = Raw(self, scope + ':exp', r.n, r.h, r.w, cexp)
      call('edet_mbconv_expand_stats', ctypes.byref(tv), ptr(wt), ldk, cexp, ptr(self.partials),
           ctypes.byref(self._nparts), self.dtype, self.stream, nbytes=r.rows * cin * self.esize, tag=tag)
    self._bn_forward(bne, r.rows, self._nparts.value)
    out = Raw(self, scope + ':dw', r.n, oh, ow, cexp)
    stats = ptr(self.partials) if self.training else None
    call('edet_mbconv_expand_dw_fwd', ctypes.byref(tv), ptr(wt), ldk, cexp, ptr(bne.scale), ptr(bne.shift), self.act,
         ptr(e_raw.data) if e_raw is not None else None, e_raw.ld if e_raw is not None else 0,
         ptr(self.param(wdw)), k, stride, ptr(out.data), out.ld, stats, ctypes.byref(self._nparts), self.dtype, self.stream,
         nbytes=(r.rows * cin + (r.rows * cexp if e_raw is not None else 0) + out.rows * cexp) * self.esize, tag=tag)
    self._bn_forward(bnd, out.rows, self._nparts.value)
    vout = View(out, bnd, self.act)
    vin.consumers += 1
    if self.training:
      ve = View(e_raw, bne, self.act)
      ve.consumers = 1
      self.tape.append(lambda: self._pw_bwd(vin, ve, wexp, w, ldn, True))
      self.tape.append(lambda: self._dw_bwd(ve, vout, wdw, k, stride))
    return vout

  def backward(self):
    """The tape in reverse; the weight-gradient sums of the pass are recorded and added in a few batched launches."""
    self._defer_begin()
    try:
      for fn in reversed(self.tape):
        fn()
    finally:
      self._defer_end()
    self.tape = []

  # ------------------------------------------------------------------ update
  def set_hyper(self, lr, ema_decay=None):
    """Per-step scalars -> device (hyper[0] = learning rate, hyper[1] = EMA decay).  Stream-ordered H2D
    copy from pageable memory (staged synchronously by the runtime, so the host values may change at once);
    kept OUTSIDE the captured step."""
    if self.update.kind == 'adam':
      # tf.keras Adam's bias-corrected rate of THIS step (t = iterations + 1), ResourceApplyAdam's alpha
      t = self.arena.step_count + 1
      b1, b2 = self.update.momentum, self.update.beta2
      lr = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    self.hyper[:2].copy_(torch.tensor([lr, ema_decay or 0.0], dtype=torch.float32), non_blocking=True)

  def optimizer_local(self, scale_for_reduce, weight_decay, clip, l2_sum, first=0, end=None, sqnorm=None, gnorm=None):
    """L2 (train_lib.py:486-491) + per-tensor and global-norm clip factors of the LOCAL gradient (:675-682);
    scale_for_reduce applies the factors in place (the data-parallel path all-reduces the clipped gradient).
    l2_sum is where the L2 loss is added.  first / end: the segment range (every segment by default); sqnorm: scratch for
    the squared norms (seg_sqnorm); gnorm: where the norm of the range goes (self.gnorm)."""
    st = self.stream
    s0, s1 = first, self.nseg if end is None else end
    sq = self.seg_sqnorm if sqnorm is None else sqnorm
    gn = self.gnorm if gnorm is None else gnorm
    offs, factor = self.seg_offsets.data_ptr() + 8 * s0, self.seg_factor.data_ptr() + 4 * s0
    # (frozen variables -- ParamArena.set_frozen -- are handled by the kernels through their segment flag)
    call('edet_opt_l2_norms', ptr(self.grads_flat), ptr(self.params_flat), offs, self.seg_flags.data_ptr() + 4 * s0,
         s1 - s0, float(weight_decay), ptr(sq), st)
    call('edet_opt_clip_factors', ptr(sq), s1 - s0, float(clip), factor, ptr(gn), ptr(l2_sum), st)
    if scale_for_reduce:
      call('edet_opt_scale', ptr(self.grads_flat), offs, factor, s1 - s0, st)

  def optimizer_apply(self, use_ema, already_scaled):
    """The update the engine's description names (train_lib.py:176-199; build_tf2_optimizer, main_tf2.py:36-59) + EMA,
    with lr / decay from self.hyper (set_hyper)."""
    u = self.update
    tail = (ptr(self.ema) if use_ema else None, ptr(self.seg_offsets), None if already_scaled else ptr(self.seg_factor),
            ptr(self.seg_flags), self.nseg, ptr(self.hyper))
    head = (ptr(self.params_flat), ptr(self.grads_flat))
    if u.kind == 'sgd':
      call('edet_opt_sgd_ema', *head, ptr(self.velocity), *tail, float(u.momentum), self.stream)
    elif u.kind == 'adam':
      call('edet_opt_adam_ema', *head, ptr(self.velocity), ptr(self.arena.second_moment()), *tail, float(u.momentum),
           u.beta2, u.epsilon, self.stream)
    elif u.kind == 'rmsprop':
      call('edet_opt_rmsprop_ema', *head, ptr(self.arena.second_moment()), ptr(self.velocity), *tail, u.rho,
           float(u.momentum), u.epsilon, self.stream)
    elif u.kind == 'lion':
      # one slot (the velocity arena holds m); the rate is the schedule's, uncorrected (set_hyper)
      call('edet_opt_lion_ema', *head, ptr(self.velocity), *tail, float(u.momentum), float(u.beta2), float(u.wd or 0.0),
           self.stream)
    else:
      raise ValueError('unknown optimizer %r' % (u.kind,))
    self.arena.count_step()
