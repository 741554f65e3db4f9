"""The EfficientDet network on one MI355X: the graph, the losses and the data-parallel reduce on the layer engine.

Engine is layer_engine.LayerEngine (buffers, variables, layer primitives, tape, update step) plus what only the
detector has: the forward graph (backbone -> BiFPN -> class / box towers), the BiFPN node fusion, the towers of the
small pyramid levels as a second chain on its own stream, the focal and box losses, and the bucketed gradient all-reduce
under the backward pass.  The update description and the L2 / clip settings come from the detection config here.
Reference structure followed: efficientdet/tf2/efficientdet_keras.py:787-915 (EfficientDetNet),
efficientdet/tf2/train_lib.py:493-684.
"""
import ctypes

import torch

from automl_amd import _lib
from automl_amd import iou_utils
from automl_amd import netspec as netspec_lib
from automl_amd._lib import ACT_NONE, ACT_SWISH, EDET_BF16, RS_IDENTITY, RS_POOL, RS_UP2, call, ptr
from automl_amd.layer_engine import BN, LayerEngine, ParamArena, Raw, Update, View, capture_graph, lion_options  # noqa: F401


class Engine(LayerEngine):
  """Builds buffers for (config, batch, image size, dtype) and runs forward / backward / update."""

  def __init__(self, config, batch_size, image_size=None, dtype='bf16', device='cuda:0', seed=0,
               params=None, spec=None, stochastic_depth=True, arena=None, lion=None, iou_loss=None):
    self.config = config
    # iou_loss = (type, weight): BoxIouLoss (tf2/train_lib.py:440-464, :580-600) fused into the box-loss pass -- loss_backward and
    # loss_only launch edet_box_iou_loss[_eval] in the place of edet_box_loss[_eval]; None: exactly the launches without it
    self.iou_loss = None
    if iou_loss is not None:
      kind, weight = iou_loss
      self.iou_loss = (iou_utils.iou_type_id(kind), str(kind), float(weight))
    # optimizer = 'adam' (train_lib.py:183-186: beta_1 = momentum, Keras defaults for what the reference does not set),
    # 'lion' (lion/lion_tf2.py's Lion in the optimizer's place: beta_1 = momentum by the same convention; beta_2 and wd are
    # no configuration keys and come in `lion`, a dict, with the reference's defaults), anything else Keras SGD
    momentum = float(config.momentum)
    kind = str(config.optimizer).lower()
    adam = kind == 'adam'
    if kind == 'lion':
      beta_2, wd = lion_options(lion)
      update = Update('lion', momentum, beta_2, wd=wd)
    elif lion:
      raise ValueError('lion options %r with optimizer=%r' % (lion, config.optimizer))
    else:
      update = Update('adam', momentum, self.ADAM_BETA2, self.ADAM_EPSILON) if adam else Update('sgd', momentum)
    super().__init__(spec if spec is not None else netspec_lib.NetSpec(config), batch_size,
                     image_size if image_size is not None else config.image_size, dtype=dtype, device=device, seed=seed,
                     params=params, arena=arena, stochastic_depth=stochastic_depth, update=update)
    if adam:
      self.arena.second_moment()
    self._side = None
    # The class / box towers of the SMALL pyramid levels (20x20 and below: ~300 latency-bound launches per step that
    # each use a fraction of the chip) run as one chain on a second HIP stream, forked and joined with events (a
    # parallel branch of the captured hipGraph), under the chain of the 80x80 / 40x40 levels: r02m/n 69.04 -> 67.7 /
    # 68.3 ms per step.  What was measured and NOT kept: one stream per level (five chains, the big kernels of levels
    # 3 and 4 compete: 71.7 -> 75.1 ms, r02g); every weight-gradient kernel deferred to the side stream (nothing on
    # the data-gradient chain waits for them: 68.3 -> 69.7 ms, r02n).
    self.small_level_stream = True
    self._side_pending = False
    self.loss_sums = self.zbuf('loss_sums', (4,))
    self.pool_argmax = True      # max-pool backward through the recorded winning tap (edet_fuse_bwd_pre)
    # bucketed gradient all-reduce overlapped with the backward pass (set_overlap_reduce): None = off
    self._overlap_reduce = None
    self._reduce_marks = {}
    self._comm_stream = None
    self._bucket_no = 0

  # ------------------------------------------------------------------ a second chain on its own stream
  def _side_branch(self):
    if self._side is None:
      names = [n for n in self.seg_names if n.startswith('class_net/') or n.startswith('box_net/')]
      lo = min(self.offsets[n][0] for n in names)
      hi = max(self.offsets[n][0] + self.offsets[n][1] for n in names)
      self._side_range = (lo, hi)       # the slice of the arena that holds the tower variables
      self._side_grads = torch.zeros(self.n_train_elems, dtype=torch.float32, device=self.device)
      self._side = self._new_branch(torch.cuda.Stream(device=self.device), self._side_grads)
    return self._side

  def _fork_join(self, main_job, side_job):
    """main_job() on the current stream, side_job() on the side stream between an event recorded now and an event
    the current stream waits for afterwards (legal inside a stream capture: the side stream joins it)."""
    side = self._side_branch()
    main = torch.cuda.current_stream(self.device)
    rec = _lib.recorder          # a step plan being recorded (automl_amd/plan.py) sees the fork and the join as events
    fork = torch.cuda.Event()
    fork.record(main)
    side.stream.wait_event(fork)
    if rec is not None:
      rec.stream_wait(side.stream.cuda_stream, rec.event_record(main.cuda_stream))
    try:
      self._branch = side
      with torch.cuda.stream(side.stream):
        b = side_job()
        done = torch.cuda.Event()
        done.record(side.stream)
        rec_done = rec.event_record(side.stream.cuda_stream) if rec is not None else None
      self._branch = self._main
      a = main_job()
    finally:
      self._branch = self._main
    main.wait_event(done)
    if rec is not None:
      rec.stream_wait(main.cuda_stream, rec_done)
    return a, b

  def _join_side(self):
    """Adds (and clears) the side chain's gradient arena; called once at the end of the backward pass, after the join."""
    if self._side_pending:
      lo, hi = self._side_range
      call('edet_axpy_clear', self.grads_flat.data_ptr() + 4 * lo, self._side_grads.data_ptr() + 4 * lo, hi - lo, 1,
           self.stream)
      self._side_pending = False

  def fuse(self, key, inputs, modes, wnames, oh, ow, act=ACT_SWISH):
    """BiFPN node fusion: act(sum_i wn_i * resample_i(input_i))."""
    c = inputs[0].raw.c
    n = inputs[0].raw.n
    nin = len(inputs)
    out = Raw(self, key, n, oh, ow, c)
    wm = self.spec.fpn.weight_method
    wc = c if (wnames and wm.startswith('channel_')) else 1       # per-channel weight vectors (WSM shape [c])
    wn = self.buf(key + ':wn', (max(4, 3 * wc),), torch.float32)
    method = (2 if wm in ('attn', 'channel_attn') else 0) if wnames else 1
    wp = [ptr(self.param(w)) for w in wnames] + [None] * (3 - len(wnames)) if wnames else [None] * 3
    # scalar fusion variables: normalised inside the fusion kernel, their gradient inside the ordered finish of dwn (no
    # edet_fuse_weights / edet_fuse_weights_bwd launches: 50 of them per D0 step); per-channel weight vectors still take
    # those launches
    wfold = wc == 1
    wraw = (ctypes.c_void_p * 3)(*wp) if wfold else None
    if not wfold:
      call('edet_fuse_weights', wp[0], wp[1], wp[2], nin, method, ptr(wn), wc, self.stream)
    tv = [v.tview() for v in inputs]
    tvp = [ctypes.byref(t) for t in tv] + [None] * (3 - nin)
    marr = (ctypes.c_int * 3)(*(list(modes) + [0] * (3 - nin)))
    fbytes = (sum(v.raw.rows for v in inputs) + out.rows) * c * self.esize
    call('edet_fuse_fwd', tvp[0], tvp[1], tvp[2], marr, nin, ptr(wn), wc, act, ptr(out.data), oh, ow, out.ld,
         wraw, method, self.dtype, self.stream, nbytes=fbytes)
    vout = View(out)
    for v in inputs:
      v.consumers += 1
    if self.training:
      dwn = self.zbuf(key + ':dwn', (max(4, 3 * wc),))
      npool = sum(1 for m in modes if m == RS_POOL)
      amax = self.buf(key + ':amax', (npool, n, oh, ow, c), torch.uint8) if npool and self.pool_argmax else None

      def bwd():
        assert out.grad_written, key
        tv2 = [v.tview() for v in inputs]
        tvp2 = [ctypes.byref(t) for t in tv2] + [None] * (3 - nin)
        # identity inputs that need a gradient: written by the fusion kernel itself (no edet_fuse_bwd_input launch, no
        # second read of ds); so is the 2x up-sampled input of a top-down node {identity, up-sample} with scalar weights
        # (a thread of the kernel then owns the 2x2 output pixels of one of its pixels); ds is stored only when another
        # resampled input still has to read it
        up2_merged = (wc == 1 and list(modes) == [RS_IDENTITY, RS_UP2] and
                      oh == 2 * inputs[1].raw.h and ow == 2 * inputs[1].raw.w)
        merged = [(modes[i] == RS_IDENTITY or (i == 1 and up2_merged)) and v.raw.needs_grad
                  for i, v in enumerate(inputs)]
        gin = (ctypes.c_void_p * 3)()
        gbeta = (ctypes.c_int * 3)()
        for i, v in enumerate(inputs):
          if merged[i]:
            gin[i] = ptr(v.raw.ensure_grad())
            gbeta[i] = 1 if v.raw.grad_written else 0
            v.raw.grad_written = True
        write_ds = 1 if any(v.raw.needs_grad and not merged[i] for i, v in enumerate(inputs)) else 0
        # (a node that stores no ds has no ds buffer: nothing stale under that key for whoever reads the buffers)
        ds = self.buf(key + ':ds', (n, oh, ow, out.ld), self.tdtype) if write_ds else None
        wgrad_folded = wfold and bool(wnames) and method != 1
        dwraw = (ctypes.c_void_p * 3)(*([ptr(self.grad(w)) for w in wnames] + [None] * (3 - len(wnames)))) if wgrad_folded else None
        call('edet_fuse_bwd_pre', tvp2[0], tvp2[1], tvp2[2], marr, nin, ptr(wn), wc, act, ptr(out.grad), oh, ow,
             out.ld, ptr(ds), ptr(dwn), ptr(amax), gin, gbeta, write_ds, *self._ws(),
             wraw if wgrad_folded else None, method, dwraw, self.dtype, self.stream,
             nbytes=fbytes + out.rows * c * self.esize)
        plane = 0
        for i, v in enumerate(inputs):
          am = None
          if modes[i] == RS_POOL and amax is not None:
            am = amax[plane].data_ptr()
            plane += 1
          if not v.raw.needs_grad or merged[i]:
            continue
          g = v.raw.ensure_grad()
          call('edet_fuse_bwd_input', ctypes.byref(tv2[i]), modes[i], ptr(wn), wc, i, ptr(ds), oh, ow, out.ld, am,
               ptr(g), 1 if v.raw.grad_written else 0, self.dtype, self.stream,
               nbytes=(out.rows + v.raw.rows) * c * self.esize,
               tag='%dx%dx%d %s' % (v.raw.h, v.raw.w, c, ('id', 'up2', 'pool')[modes[i]]))
          v.raw.grad_written = True
        if wnames and not wgrad_folded:
          gp = [ptr(self.grad(w)) for w in wnames] + [None] * (3 - len(wnames))
          call('edet_fuse_weights_bwd', wp[0], wp[1], wp[2], nin, method, ptr(dwn), gp[0], gp[1], gp[2],
               wc, self.stream)

      self.tape.append(bwd)
    return vout

  # ------------------------------------------------------------------ network
  def forward(self, images, training=False, update_moving=True):
    """images: device tensor [B,H,W,3] in the engine dtype. Returns (cls_views, box_views)."""
    c = self.config
    spec = self.spec
    self._begin(training, update_moving)
    if training and self.drop_masks and not torch.cuda.is_current_stream_capturing():
      # an eager training pass draws its own stochastic-depth masks; a captured one reads what the trainer drew outside
      # the graph (train_lib: refresh_drop_masks in front of every replay)
      self.refresh_drop_masks()
    bb = c.backbone_name
    x = self.stem(bb, images, self.act)
    # ---- MBConv blocks
    reds = []
    self._reduce_marks = {}
    bucket_blocks = self._bucket_blocks() if (training and self._overlap_reduce is not None) else ()
    for b in spec.blocks:
      if b.index in bucket_blocks:
        # everything the tape holds from here on belongs to variables at or behind this block's first one
        self._reduce_marks[len(self.tape)] = bucket_blocks[b.index]
      x = self._mbconv(x, b, '%s/blocks_%d' % (bb, b.index))
      if b.index in spec.reductions:
        reds.append(x)
    all_feats = [None] + reds
    feats = list(all_feats[c.min_level:c.max_level + 1])
    wf = c.fpn_num_filters
    if training and self._overlap_reduce is not None:
      self._reduce_marks[0] = 0                                     # stem + first blocks: the last bucket
      self._reduce_marks[len(self.tape)] = self._first_non_backbone_elem()   # BiFPN + heads: the first one
    # ---- extra levels P6.. (efficientdet_keras.py:823-836,900-901)
    for level in range(6, c.max_level + 1):
      f = feats[-1]
      th, tw = (f.raw.h + 1) // 2, (f.raw.w + 1) // 2
      s = 'resample_p%d' % level
      if f.raw.c != wf and getattr(c, 'conv_after_downsample', False):
        # ResampleFeatureMap with conv_after_downsample (efficientdet_keras.py:316-324): the 1x1 convolution (+ BN) runs on
        # the POOLED map -- a quarter of the rows -- instead of before the pool
        pooled = self.fuse(s + ':pool', [f], [RS_POOL], [], th, tw, act=ACT_NONE)
        feats.append(self.pw(s, pooled, s + '/conv2d/kernel', wf, bias=s + '/conv2d/bias', bn=(s + '/bn') if c.apply_bn_for_resampling else None, bias_grad=True))
        continue
      if f.raw.c != wf:
        f = self.pw(s, f, s + '/conv2d/kernel', wf, bias=s + '/conv2d/bias', bn=(s + '/bn') if c.apply_bn_for_resampling else None, bias_grad=True)
      feats.append(self.fuse(s + ':pool', [f], [RS_POOL], [], th, tw, act=ACT_NONE))
    # ---- BiFPN
    for rep in range(c.fpn_cell_repeats):
      feats = self._fpn_cell(feats, 'fpn_cells/cell_%d' % rep)
    self.fpn_feats = feats
    # ---- heads
    na = spec.num_anchors
    # side chain = the levels of at most 20x20 pixels (r02q: also moving the 40x40 level there 68.3 -> 68.5 ms, only the
    # 10x10 and 5x5 levels 69.0 ms)
    nbig = sum(1 for f in feats if f.raw.h * f.raw.w > 400)
    if self.small_level_stream and self.sync_bn is None and 0 < nbig < len(feats):
      cls, box = self._heads_two_chains(feats, nbig, c.num_classes * na, 4 * na)
    else:
      cls = self._head(feats, 'class_net', 'class', c.num_classes * na)
      box = self._head(feats, 'box_net', 'box', 4 * na)
    self.cls_views, self.box_views = cls, box
    if self._cast_items and not torch.cuda.is_current_stream_capturing() and \
        (self._cast_table is None or self._cast_table[0] != list(self._cast_items)):
      self._cast_all()         # builds the descriptor table now (outside any capture); the casts it repeats are idempotent
    return cls, box

  def _fpn_cell(self, feats, cell_scope):
    c = self.config
    wf = c.fpn_num_filters
    fpn = self.spec.fpn
    feats = list(feats)
    num_in = len(feats)
    for n, node in enumerate(fpn.nodes):
      scope = '%s/fnode%d' % (cell_scope, n)
      lvl = node['feat_level'] - c.min_level
      th, tw = feats[lvl].raw.h, feats[lvl].raw.w
      ins, modes = [], []
      for i, off in enumerate(node['inputs_offsets']):
        f = feats[off]
        if f.raw.c != wf:
          if getattr(c, 'conv_after_downsample', False) and f.raw.h > th and f.raw.w > tw:
            # (no BiFPN of fpn_configs.py feeds a node a wider AND larger map; the extra levels P6.. are handled above)
            raise ValueError('conv_after_downsample inside a BiFPN node is not built')
          rs = '%s/resample_%d_%d_%d' % (scope, i, off, len(feats))
          f = self.pw(rs, f, rs + '/conv2d/kernel', wf, bias=rs + '/conv2d/bias', bn=(rs + '/bn') if c.apply_bn_for_resampling else None, bias_grad=True)
        fh, fw = f.raw.h, f.raw.w
        if fh > th and fw > tw:
          if (fh - 1) // th + 1 != 2 or (fw - 1) // tw + 1 != 2:
            raise ValueError('only 2x down-sampling between pyramid levels is supported')
          modes.append(RS_POOL)
        elif fh <= th and fw <= tw:
          modes.append(RS_IDENTITY if (fh == th and fw == tw) else RS_UP2)
        else:
          raise ValueError('Incompatible Resampling : feat shape {}x{} target_shape: {}x{}'.format(
              fh, fw, th, tw))
        ins.append(f)
      wnames = []
      if fpn.weight_method in ('fastattn', 'attn', 'channel_fastattn', 'channel_attn'):
        wnames = [scope + '/WSM' + ('' if i == 0 else '_%d' % i) for i in range(len(ins))]
      x = self.fuse(scope + ':fuse', ins, modes, wnames, th, tw, act=self.act)
      oc = '%s/op_after_combine%d' % (scope, len(feats))
      d = self.dw(oc + ':dw', x, oc + '/conv/depthwise_kernel', 3, 1)
      y = self.pw(oc + ':pw', d, oc + '/conv/pointwise_kernel', wf, bias=oc + '/conv/bias', bn=oc + '/bn')
      feats.append(y)
    out = []
    for level in range(c.min_level, c.max_level + 1):
      for i, node in enumerate(reversed(fpn.nodes)):
        if node['feat_level'] == level:
          out.append(feats[-1 - i])
          break
    assert len(out) == num_in
    return out

  def _head_level(self, feat, level, net, prefix, out_ch):
    """One tower (class or box net) on one pyramid level (efficientdet_keras.py:336-480, 483-641)."""
    c = self.config
    wf = c.fpn_num_filters
    x = feat
    sp = getattr(c, 'survival_prob', None)
    for i in range(c.box_class_repeats):
      s = '%s/%s-%d' % (net, prefix, i)
      key = '%s:l%d' % (s, level)
      d = self.dw(key + ':dw', x, s + '/depthwise_kernel', 3, 1)
      y = self.pw(key + ':pw', d, s + '/pointwise_kernel', wf, bias=s + '/bias',
                  bn='%s/%s-%d-bn-%d' % (net, prefix, i, level), act=self.act)
      if sp:
        # config.survival_prob (efficientdet_keras.py:434-436, 612-614): from the second tower layer on
        # image = drop_connect(act(bn(conv(image)))) + image -- a residual connection in inference too, a per-image
        # floor(p + u) / p scale on the branch in training (utils.py:329-344; own draws per layer, level and tower).  The
        # residual operand is a stored tensor, so the first layer's activated output is materialised as well.
        x = self.bn_res(key + ':out', y, x if i > 0 else None, survival_prob=sp if i > 0 else None)
      else:
        x = y
    s = '%s/%s-predict' % (net, prefix)
    key = '%s:l%d' % (s, level)
    if net == 'box_net' and not self.training and self.dtype == EDET_BF16:
      # Inference, bf16 storage: the BOX-predict layer (depthwise 3x3 + 64 -> 36 pointwise) runs in fp32.  Error budget
      # of the box logits against the fp32 oracle (scripts/precision_sweep.py, d0 640x640): bf16 matrix-core operands of
      # this one layer 1.1e-3 of the range, its depthwise output stored as bf16 6.1e-4, everything else together 3e-4
      # -- the class logits are at 1e-4 with bf16 operands and need no such treatment.
      with self._fp32_island():
        d = self.dw(key + ':dw:f32', self._to_f32(key + ':x:f32', x), s + '/depthwise_kernel', 3, 1)
        return self.pw(key + ':pw:f32', d, s + '/pointwise_kernel', out_ch, bias=s + '/bias')
    # inference forward with bf16 storage: the class / box logits are stored as fp32 (edet_pw_fwd_f32out) -- rounding them to
    # bf16 is 3e-3 of their range and the whole of what separated the path from the 1e-3 of north_star
    # (scripts/precision_sweep.py); the training step keeps bf16 logits (they only feed the loss)
    d = self.dw(key + ':dw', x, s + '/depthwise_kernel', 3, 1)
    return self.pw(key + ':pw', d, s + '/pointwise_kernel', out_ch, bias=s + '/bias', f32out=True)

  def _head(self, feats, net, prefix, out_ch):
    return [self._head_level(feat, self.config.min_level + li, net, prefix, out_ch) for li, feat in enumerate(feats)]

  def _heads_two_chains(self, feats, nbig, cls_ch, box_ch):
    """Both towers as two chains: the big levels (the first nbig) on the current stream, the small ones on the side
    stream (Engine.small_level_stream); the backward pass replays each chain's tape the same way, the side chain's
    gradients of the shared tower kernels going to its own arena, which _join_side adds after the join."""
    c = self.config
    for net, prefix, out_ch in (('class_net', 'class', cls_ch), ('box_net', 'box', box_ch)):
      # compute copies of the shared tower kernels are made BEFORE the fork (the chain that would otherwise make them
      # first runs concurrently with the one that uses them)
      for i in range(c.box_class_repeats):
        self._pw_copies('%s/%s-%d/pointwise_kernel' % (net, prefix, i), c.fpn_num_filters, c.fpn_num_filters)
      self._pw_copies('%s/%s-predict/pointwise_kernel' % (net, prefix), c.fpn_num_filters, out_ch)
    if not self.training and self.dtype == EDET_BF16:
      # ... and the fp32 copies of the box-predict kernel (_head_level's fp32 island): the chain that casts them first would
      # otherwise do so on ITS stream while the other chain reads the same buffer with no event in between
      with self._fp32_island():
        self._pw_copies('box_net/box-predict/pointwise_kernel', c.fpn_num_filters, box_ch)
    main_tape = self.tape
    tapes = {}
    # which chain runs which (level, tower): the big levels on the main chain, the small ones on the side chain.  Both
    # towers of a level stay on ONE chain: they accumulate into the same feature gradient, and only stream order
    # orders the beta = 0 writer before the beta = 1 one (r05 lab: splitting a level lost 0.5 ms anyway)
    towers = (('class_net', 'class', cls_ch), ('box_net', 'box', box_ch))
    work = {'main': [], 'side': []}
    for li in range(len(feats)):
      for tw in towers:
        on_main = li < nbig
        work['main' if on_main else 'side'].append((li, tw))

    def chain(which):
      def job():
        self.tape = []
        out = {}
        for li, (net, prefix, out_ch) in work[which]:
          out[li, net] = self._head_level(feats[li], c.min_level + li, net, prefix, out_ch)
        tapes[which] = self.tape
        return out
      return job
    try:
      done, side_done = self._fork_join(chain('main'), chain('side'))
    finally:
      self.tape = main_tape
    done.update(side_done)
    outs = [(done[li, 'class_net'], done[li, 'box_net']) for li in range(len(feats))]
    if self.training:
      def bwd():
        def replay(which):
          def job():
            self._defer_begin()        # (the side chain records on its own stream and flushes before the join)
            try:
              for fn in reversed(tapes[which]):
                fn()
            finally:
              if which == 'side':
                self._defer_end()
          return job
        self._fork_join(replay('main'), replay('side'))
        self._side_pending = True
      self.tape.append(bwd)
    return [o[0] for o in outs], [o[1] for o in outs]

  # ------------------------------------------------------------------ outputs
  def outputs(self):
    """(list of [B,h,w,A*classes], list of [B,h,w,A*4]) strided torch views of the logits buffers."""
    cls = [v.raw.data[..., :v.raw.c] for v in self.cls_views]
    box = [v.raw.data[..., :v.raw.c] for v in self.box_views]
    return cls, box

  # ------------------------------------------------------------------ loss + backward + update
  def _loss_front(self, labels, inv_norm_dev):
    """What loss_backward and loss_only open with -> (normalizer, norm_dev, levels).  labels['normalizer'] == 'device':
    1 / normalizer lives in the device scalar `inv_norm_dev` (hyper[2:], set_normalizer; eval_inv_norm), nothing of the step
    depends on a host value, so its launches can be captured once and replayed for every batch; a host float supplied by the
    caller: no device sync; else sum(mean_num_positives) + 1 through the host.  levels: per level (cls_raw, box_raw,
    cls_targets, box_targets), the targets checked."""
    c = self.config
    norm_dev = None
    if labels.get('normalizer') == 'device':
      normalizer, norm_dev = 1.0, ptr(inv_norm_dev)
    elif 'normalizer' in labels:
      normalizer = float(labels['normalizer'])
    else:
      normalizer = float(labels['mean_num_positives'].sum().item()) + 1.0
    levels = []
    for li, (cv, bv) in enumerate(zip(self.cls_views, self.box_views)):
      ct = labels['cls_targets_%d' % (c.min_level + li)]
      bt = labels['box_targets_%d' % (c.min_level + li)]
      assert ct.dtype == torch.int32 and ct.is_contiguous() and bt.dtype == torch.float32 and bt.is_contiguous()
      levels.append((cv.raw, bv.raw, ct, bt))
    return normalizer, norm_dev, levels

  def loss_backward(self, labels):
    """Detection loss forward+backward (train_lib.py:493-604) then the tape in reverse.

    labels: dict with device tensors cls_targets_L int32 [B,h,w,A], box_targets_L fp32 [B,h,w,4A],
    mean_num_positives fp32 [B] (or [B,1]).
    """
    c = self.config
    assert self.training
    normalizer, norm_dev, levels = self._loss_front(labels, self.hyper[2:])
    na = self.spec.num_anchors
    ls = float(getattr(c, 'label_smoothing', 0.0) or 0.0)
    anchors, anchor_row = (self._iou_anchors(), 0) if self.iou_loss is not None else (None, 0)
    for r, rb, ct, bt in levels:
      if ls:      # FocalLoss(label_smoothing), train_lib.py:400-402
        call('edet_focal_loss_smooth', ptr(r.data), r.ld, ptr(ct), r.rows, na, c.num_classes, c.alpha, c.gamma, ls,
             1.0 / normalizer, norm_dev, ptr(r.ensure_grad()), ptr(self.grad('class_net/class-predict/bias')),
             ptr(self.loss_sums), *self._ws(), self.dtype, self.stream,
             nbytes=2 * r.rows * r.c * self.esize)
      else:
        call('edet_focal_loss', ptr(r.data), r.ld, ptr(ct), r.rows, na, c.num_classes, c.alpha, c.gamma,
             1.0 / normalizer, norm_dev, ptr(r.ensure_grad()), ptr(self.grad('class_net/class-predict/bias')),
             ptr(self.loss_sums), *self._ws(), self.dtype, self.stream,
             nbytes=2 * r.rows * r.c * self.esize)
      r.grad_written = True
      box_args = (ptr(rb.data), rb.ld, ptr(bt), rb.rows, 4 * na, c.delta, 1.0 / (normalizer * 4.0),
                  float(c.box_loss_weight), norm_dev, ptr(rb.ensure_grad()), ptr(self.grad('box_net/box-predict/bias')),
                  ptr(self.loss_sums), *self._ws(), self.dtype, self.stream)
      if self.iou_loss is None:
        call('edet_box_loss', *box_args)
      else:
        hw = rb.rows // self.batch
        call('edet_box_iou_loss', *box_args, anchors.data_ptr() + 16 * anchor_row, hw, self.iou_loss[0], self.iou_loss[2])
        anchor_row += hw * na
      rb.grad_written = True
    self.backward()

  def loss_only(self, labels):
    """test_step's losses (train_lib.py:717-732) of the last forward pass into eval_sums [cls, box, L2, -]: per level
    edet_focal_loss_eval and edet_box_loss_eval -- the training kernels' sums bit for bit, nothing of the size of the logits
    written -- then edet_l2_loss.  Nothing the training step owns is touched: the sums, the reciprocal normalizer
    (eval_inv_norm, read when labels['normalizer'] == 'device') and the L2 scratch are buffers of their own, the gradient
    arena is neither read nor written.  The logits are read in the dtype they were stored in (an inference pass with bf16
    storage keeps them in fp32, _head_level)."""
    c = self.config
    sums = self.eval_sums
    call('edet_zero', ptr(sums), sums.numel() * 4, self.stream)
    normalizer, norm_dev, levels = self._loss_front(labels, self.eval_inv_norm)
    na = self.spec.num_anchors
    ls = float(getattr(c, 'label_smoothing', 0.0) or 0.0)
    anchors, anchor_row = (self._iou_anchors(), 0) if self.iou_loss is not None else (None, 0)
    for r, rb, ct, bt in levels:
      call('edet_focal_loss_eval', ptr(r.data), r.ld, ptr(ct), r.rows, na, c.num_classes, c.alpha, c.gamma, ls,
           1.0 / normalizer, norm_dev, ptr(sums), *self._ws(), _lib.EDET_F32 if r.data.dtype == torch.float32 else EDET_BF16,
           self.stream, nbytes=r.rows * r.c * r.data.element_size())
      box_args = (ptr(rb.data), rb.ld, ptr(bt), rb.rows, 4 * na, c.delta, 1.0 / (normalizer * 4.0), norm_dev,
                  ptr(sums), *self._ws(), _lib.EDET_F32 if rb.data.dtype == torch.float32 else EDET_BF16, self.stream)
      if self.iou_loss is None:
        call('edet_box_loss_eval', *box_args)
      else:
        hw = rb.rows // self.batch
        call('edet_box_iou_loss_eval', *box_args, anchors.data_ptr() + 16 * anchor_row, hw, self.iou_loss[0])
        anchor_row += hw * na
    seg_l2 = self.buf('eval:seg_l2', (self.nseg * _lib.OPT_SPLIT,), torch.float32)
    call('edet_l2_loss', ptr(self.params_flat), ptr(self.seg_offsets), ptr(self.seg_flags), self.nseg, float(c.weight_decay),
         ptr(seg_l2), sums.data_ptr() + 8, self.stream)

  def _iou_anchors(self):
    """The anchor table [sum over the levels of h * w * A, 4] fp32 of this engine's image size on its device, in the order
    of anchors.Anchors.boxes (level, y, x, anchor): the cached table of postprocess._anchor_boxes.  A level's first row is
    the running sum of h * w * A; every row of the box outputs is paired with its own anchor whatever the batch size."""
    from automl_amd import postprocess
    c = self.config
    a = postprocess._anchor_boxes({'min_level': c.min_level, 'max_level': c.max_level, 'num_scales': c.num_scales,
                                   'aspect_ratios': c.aspect_ratios, 'anchor_scale': c.anchor_scale,
                                   'image_size': tuple(self.image_size)}, self.device)
    rows = sum(bv.raw.rows // self.batch for bv in self.box_views) * self.spec.num_anchors
    if a.shape[0] != rows:
      raise ValueError('the IoU loss pairs %d box outputs per image with %d anchors' % (rows, a.shape[0]))
    return a

  def _with_iou(self, s, values):
    """loss_values / eval_loss_values with the IoU loss on: 'box_iou_loss' = sums[3], folded into det_loss and loss
    (train_lib.py:592-601); the values as they are with it off."""
    if self.iou_loss is None:
      return values
    det = float(s.dtype.type(values['det_loss']) + s.dtype.type(self.iou_loss[2]) * s[3])
    values.update({'box_iou_loss': float(s[3]), 'det_loss': det, 'loss': det + float(s[2])})
    return values

  @property
  def eval_sums(self):
    return self.buf('eval:loss_sums', (4,), torch.float32)

  @property
  def eval_inv_norm(self):
    """1 / normalizer of the evaluation step, a device scalar of its own (the training step's is hyper[2])."""
    return self.buf('eval:inv_norm', (1,), torch.float32)

  def eval_loss_values(self):
    s = self.eval_sums.detach().cpu().numpy()
    c = self.config
    det = float(s[0] + c.box_loss_weight * s[1])
    return self._with_iou(s, {'cls_loss': float(s[0]), 'box_loss': float(s[1]), 'det_loss': det, 'reg_l2_loss': float(s[2]),
                              'loss': det + float(s[2])})

  def backward(self):
    """The base pass; with set_overlap_reduce, every range of the arena is handed to the reduce as soon as the tape entry
    that completes it (_reduce_marks) has run."""
    marks = self._reduce_marks if self._overlap_reduce is not None else {}
    self._bucket_hi = self.n_train_elems
    self._bucket_no = 0
    if marks:
      tape = []
      for i, fn in enumerate(self.tape):       # (replayed in reverse: the reduce follows the entry it is put in front of)
        if i in marks:
          tape.append(lambda lo=marks[i]: self._reduce_bucket(lo))
        tape.append(fn)
      self.tape = tape
    super().backward()
    self._join_side()
    if marks:
      self._finish_buckets()

  # ---- gradient all-reduce overlapped with the backward pass (north_star; legal only without the global-norm clip) ----
  def set_overlap_reduce(self, reduce_fn, buckets=6):
    """reduce_fn(flat_slice) = in-place SUM all-reduce.  The reference clips the LOCAL gradient by its GLOBAL norm before
    apply_gradients reduces it (train_lib.py:675-683), which needs every gradient of the step: with clip_gradients_norm > 0
    nothing may be reduced before the backward pass has ended.  With clip_gradients_norm = 0 (hparams_config.py:220 allows
    it) the local gradient of a variable is final as soon as its layer's backward has run, so the arena is reduced in
    `buckets` contiguous ranges in the order the backward pass completes them -- BiFPN + heads first, then the backbone
    stages last to first (the arena is laid out in forward order) -- on a communication stream, under the backward
    kernels of the earlier layers.  The L2 gradient (train_lib.py:486-491) is added per range just before its reduce."""
    clip = abs(self.config.clip_gradients_norm) if self.config.clip_gradients_norm else 0.0
    if reduce_fn is not None and clip > 0:
      raise ValueError('overlapping the gradient all-reduce with the backward pass needs clip_gradients_norm=0: the '
                       'reference clips the local gradient by its global norm BEFORE the reduce (train_lib.py:675-683)')
    self._overlap_reduce = reduce_fn
    self._overlap_buckets = int(buckets)
    if reduce_fn is not None and self._comm_stream is None:
      self._comm_stream = torch.cuda.Stream(device=self.device)
      self._seg_host = [int(o) for o in self.arena.seg_offsets.cpu().tolist()]
      self._bucket_gn = torch.zeros(64, dtype=torch.float32, device=self.device)

  def _first_non_backbone_elem(self):
    bb = self.config.backbone_name + '/'
    return min(self.offsets[n][0] for n in self.seg_names if not n.startswith(bb))

  def _bucket_blocks(self):
    """{block index: first arena element of the block} for the blocks that open a backbone bucket: walking the blocks
    from the last one, a bucket is closed once it holds its share of the backbone's elements."""
    bb = self.config.backbone_name
    first = {}
    for b in self.spec.blocks:
      pre = '%s/blocks_%d/' % (bb, b.index)
      first[b.index] = min(self.offsets[n][0] for n in self.seg_names if n.startswith(pre))
    end = self._first_non_backbone_elem()
    share = end / max(self._overlap_buckets - 1, 1)
    out, hi = {}, end
    for idx in sorted(first, reverse=True):
      if hi - first[idx] >= share and first[idx] > 0:
        out[idx] = first[idx]
        hi = first[idx]
    return out

  def _reduce_bucket(self, lo):
    """The arena range [lo, previous lo) is final: flush its deferred weight-gradient sums, add the L2 gradient, and hand it
    to the communication stream."""
    hi = self._bucket_hi
    if lo >= hi:
      return
    self._defer_end()                 # the partial sums recorded so far -> the arena
    self._join_side()                 # (first bucket: the side chain's share of the tower gradients)
    seg = self._seg_host
    s0, s1 = seg.index(lo), seg.index(hi)
    no = self._bucket_no
    sq = self.buf('ovl:sq%d' % no, (2 * (s1 - s0) * _lib.OPT_SPLIT,), torch.float32)
    self.optimizer_local(False, clip=0.0, first=s0, end=s1, sqnorm=sq, gnorm=self._bucket_gn[no:])
    main = torch.cuda.current_stream(self.device)
    ready = torch.cuda.Event()
    ready.record(main)
    self._comm_stream.wait_event(ready)
    with torch.cuda.stream(self._comm_stream):
      self._overlap_reduce(self.grads_flat[lo:hi])
    self._bucket_hi = lo
    self._bucket_no = no + 1
    self._defer_begin()

  def _finish_buckets(self):
    assert self._bucket_hi == 0, self._bucket_hi
    done = torch.cuda.Event()
    done.record(self._comm_stream)
    torch.cuda.current_stream(self.device).wait_event(done)
    gn = self._bucket_gn[:self._bucket_no]
    self.gnorm.copy_(torch.sqrt((gn * gn).sum()).reshape(1))      # the local gradient's norm (reported only)

  def set_normalizer(self, mean_num_positives):
    """hyper[2] = 1 / (sum(mean_num_positives) + 1) computed on the device (train_lib.py:517), no host sync."""
    m = mean_num_positives.reshape(-1)
    if m.dtype != torch.float32 or not m.is_contiguous():
      m = m.float().contiguous()
    call('edet_loss_normalizer', ptr(m), m.numel(), self.hyper.data_ptr() + 8, self.stream)

  def optimizer_local(self, scale_for_reduce, clip=None, **segments):
    """With the detection config's weight decay and clip (unless the caller gives one), the L2 loss into loss_sums[2]."""
    c = self.config
    if clip is None:
      clip = abs(c.clip_gradients_norm) if c.clip_gradients_norm else 0.0
    super().optimizer_local(scale_for_reduce, c.weight_decay, clip, self.loss_sums[2:], **segments)

  def optimizer_step(self, lr, ema_decay=None, all_reduce=None):
    """L2 + clip (local, before the reduce) + [all-reduce SUM] + SGD momentum + EMA."""
    self.set_hyper(lr, ema_decay)
    if self._overlap_reduce is not None:       # L2 + reduce already done range by range inside backward()
      self.optimizer_apply(ema_decay is not None, True)
      return
    self.optimizer_local(all_reduce is not None)
    if all_reduce is not None:
      all_reduce(self.grads_flat)
    self.optimizer_apply(ema_decay is not None, all_reduce is not None)

  # the five values of loss_values / eval_loss_values, in the order loss_vector writes them
  LOSS_KEYS = ('cls_loss', 'box_loss', 'det_loss', 'reg_l2_loss', 'loss')

  def loss_vector(self, sums, out):
    """LOSS_KEYS of a step on the device, for a caller that sums them over steps without reading them (train_lib's fit and
    evaluate): sums = loss_sums or eval_sums [cls, box, L2, -] -> out float32 [5], formed in float32 with the roundings
    loss_values makes on the host -- box_loss_weight * box rounded, then added to cls; det + L2 -- so a value read from
    `out` is the float32 of the one loss_values reports.  Small torch launches on the current stream; nothing waits.
    With the IoU loss on, sums = [cls, box, L2, iou] and out is float32 [6] (loss_keys): iou_loss_weight * iou, rounded, is
    added to det before L2 is, and the sixth entry is box_iou_loss."""
    torch.mul(sums[1:2], float(self.config.box_loss_weight), out=out[2:3])
    out[2:3].add_(sums[0:1])
    out[0:2].copy_(sums[0:2])
    out[3:4].copy_(sums[2:3])
    if self.iou_loss is not None:      # out [6]: det += iou_loss_weight * box_iou_loss (rounded), the value itself last
      torch.mul(sums[3:4], self.iou_loss[2], out=out[5:6])
      out[2:3].add_(out[5:6])
      torch.add(out[2:3], sums[2:3], out=out[4:5])
      out[5:6].copy_(sums[3:4])
      return out
    torch.add(out[2:3], sums[2:3], out=out[4:5])
    return out

  @property
  def loss_keys(self):
    """The names of loss_vector's entries: LOSS_KEYS, and 'box_iou_loss' behind them with the IoU loss on."""
    return self.LOSS_KEYS + (('box_iou_loss',) if self.iou_loss is not None else ())

  def loss_values(self):
    s = self.loss_sums.detach().cpu().numpy()
    c = self.config
    det = float(s[0] + c.box_loss_weight * s[1])
    return self._with_iou(s, {'cls_loss': float(s[0]), 'box_loss': float(s[1]), 'det_loss': det, 'reg_l2_loss': float(s[2]),
                              'loss': det + float(s[2]), 'gradient_norm': float(self.gnorm.item())})
