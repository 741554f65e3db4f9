"""Step plans: the launches of an engine pass, recorded at the C ABI and written to a file that a host WITHOUT a Python
interpreter replays (behind include/edet_net.h: edet_create / edet_forward / edet_train_step; csrc/plan_file.cpp decodes and
checks the whole file on the host before csrc/net_runtime.cpp allocates anything on the device, then replays it).

Why a recorded plan and not a second engine in C++: every launch of a step already goes through `_lib.call` (the layers,
and since round 6 the clears, the side chain's gradient join and the loss normalizer: edet_zero / edet_axpy_clear /
edet_loss_normalizer), the arguments of a step are a pure function of (config, batch, image size, dtype), and the captured
hipGraph the Python host replays is exactly such a recording made by the HIP runtime.  The plan is the same recording made
one level up, where it can be written to disk: buffers (size, optional initial contents: variables, optimizer slots, moving
statistics, tables), named handles into them (images, targets, logits, hyper-parameters), and per program ('forward',
'train_step') the list of C-ABI calls with every device pointer expressed as (buffer, offset), the stream forks / joins of
the two head chains as event operations, and a marker where the data-parallel gradient exchange goes
(tf2/train_lib.py:675-683 -> edet_dp_init).

The reference interfaces this gives a compiled host: efficientdet_keras.EfficientDetNet.__init__/call
(efficientdet/tf2/efficientdet_keras.py:790-799, 893-915) and EfficientDetNetTrain.train_step (tf2/train_lib.py:606-684).

File layout (little endian), version 1:
  'EDETPLAN' u32 version u32 nbuf u32 nnames u32 nstreams u32 nevents u32 nprog u32 nfn u32 ndevreloc
  nfn   x { u16 len, name }                                   entry-point names (index = fn id)
  nbuf  x { u64 bytes, u64 init_offset (0 = none: zero-filled) }
  nnames x { u16 len, name, u32 buf, u64 offset, u64 bytes }   (buf 0xffffffff: an integer property, value in `offset`)
  ndevreloc x { u32 buf, u64 at, u32 target buf, u64 target offset }   device pointers stored INSIDE initial contents (the
                                                                       descriptor table of edet_cast_batch): patched after upload
  nprog x { u16 len, name, u32 nops, ops }
  op: u8 kind
    0 CALL   u16 fn, u8 nargs, args: u8 type { 0 int64 | 1 double | 2 devptr u32 buf u64 off (buf 0xffffffff = NULL)
                                                | 3 stream u32 idx | 4 host blob u32 nbytes, bytes, u16 nreloc x {u32 at, u32 buf, u64 off} | 5 NULL }
    1 EVENT_RECORD u32 event u32 stream      2 STREAM_WAIT u32 stream u32 event      3 ALLREDUCE_SUM_F32 u32 buf u64 off u64 count u32 stream
  [variable table, optional: present exactly when the names section holds the integer property 'num_variables']
    'EDETVARS' u32 nvars, nvars x { u16 len, name, u8 trainable, u8 rank (<= 4), rank x u64 dim, u64 offset, u64 count }
    one entry per variable of ParamArena.offsets, in its order: the reference name, the shape in the reference layout, and
    the ELEMENT offset / count inside its fp32 arena -- trainable variables in 'params' (and, at the same offset, in the
    slots 'ema', 'velocity' and, for Adam, 'adam_v'), BatchNorm moving statistics in 'bn_state'.  It follows the last
    program, in front of the padding, where a reader that knows nothing of it never looks; the properties 'optimizer'
    (0 sgd, 1 adam, 2 lion), 'iterations' (optimizer steps behind the state the plan starts from) and, for Adam,
    'adam_beta1_bits' / 'adam_beta2_bits' / 'adam_epsilon_bits' (the doubles' bit patterns), for Lion 'lion_beta1_bits' /
    'lion_beta2_bits' / 'lion_wd_bits' in the same convention, go with it (optimizer_props).  Lion keeps its one slot in
    'velocity', as SGD does: a Lion plan has no 'adam_v' and its state files no slot 3.
  initial contents, 256-byte aligned, at the offsets the buffer table names.

State files (edet_net_save_state / edet_net_load_state, read_state / write_state below), little endian, version 1:
  'EDETSTAT' u32 version u32 nrecords i64 iterations
  nrecords x { u16 len, name, u8 slot (0 value | 1 ema | 2 momentum | 3 adam_v), u8 rank (<= 4), rank x u64 dim, u64 count,
               count x f32 }
"""
import bisect
import contextlib
import ctypes
import gc
import mmap
import os
import re
import struct

import numpy as np
import torch

from automl_amd import _lib

MAGIC = b'EDETPLAN'
VERSION = 1
NULL_BUF = 0xffffffff
VARS_MAGIC = b'EDETVARS'
STATE_MAGIC = b'EDETSTAT'
STATE_VERSION = 1
STATE_SLOTS = ('variables', 'ema', 'momentum', 'adam_v')      # slot id = index (EDET_SLOT_* of edet_net.h)
MAX_RANK = 4
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'edet_hip.h')


def header_prototypes(path=_HEADER):
  """name -> list of parameter declarations, parsed from include/edet_hip.h (the same parse as tests/test_abi.py)."""
  src = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
  out = {}
  for m in re.finditer(r'\b(?:int|const char\*)\s+(edet_\w+)\s*\(([^;]*?)\)\s*;', src, flags=re.S):
    out[m.group(1)] = [a.strip() for a in m.group(2).split(',') if a.strip() and a.strip() != 'void']
  return out


def stream_arg_index():
  """name -> position of the `void* stream` parameter (None if the entry point takes none)."""
  out = {}
  for name, args in header_prototypes().items():
    idx = [i for i, a in enumerate(args) if re.search(r'\bvoid\s*\*\s*stream$', a)]
    out[name] = idx[0] if idx else None
  return out


def _blob_of(obj):
  """(bytes, [(offset, pointer value)]) of a ctypes structure / array / scalar passed by reference."""
  raw = ctypes.string_at(ctypes.addressof(obj), ctypes.sizeof(obj))
  relocs = []
  if isinstance(obj, ctypes.Structure):
    for fname, ftype in obj._fields_:
      if ftype is ctypes.c_void_p:
        v = getattr(obj, fname)
        if v:
          relocs.append((getattr(type(obj), fname).offset, int(v)))
  elif isinstance(obj, ctypes.Array) and obj._type_ is ctypes.c_void_p:
    for i in range(len(obj)):
      if obj[i]:
        relocs.append((8 * i, int(obj[i])))
  elif isinstance(obj, ctypes.c_void_p):
    if obj.value:
      relocs.append((0, int(obj.value)))
  return raw, relocs


class Recorder(object):
  """Collects the operations of one or more programs; `install()` hooks `_lib.call` and the engine's fork / join."""

  def __init__(self):
    self.programs = []          # (name, ops)
    self._ops = None
    self.streams = {}           # stream handle -> index (0 = the caller's stream)
    self.nevents = 0
    self.names = {}             # name -> (pointer, bytes)
    self.props = {}             # name -> integer property of the network (batch, image size, levels, ...)
    self.dev_relocs = []        # (address of an 8-byte slot in device memory, device pointer stored there)
    self.variables = []         # (name, shape, trainable, element offset, element count) inside the variable's arena
    self._stream_pos = stream_arg_index()
    self._keep = []             # tensors that must stay allocated until the plan is written

  # ---- recording ------------------------------------------------------------------------------------------------
  def begin(self, program, main_stream=None):
    assert self._ops is None, 'a program is already being recorded'
    main = torch.cuda.current_stream().cuda_stream if main_stream is None else main_stream
    if not self.streams:
      self.streams[main] = 0
    assert self.streams.get(main) == 0, 'every program must be recorded on the same main stream'
    self._ops = []
    self._program = program
    _lib.recorder = self

  def end(self):
    _lib.recorder = None
    self.programs.append((self._program, self._ops))
    self._ops = None

  def _stream(self, handle):
    handle = int(handle or 0)
    if handle not in self.streams:
      self.streams[handle] = len(self.streams)
    return self.streams[handle]

  def on_call(self, name, args):
    if self._ops is None:
      return
    argtypes = _lib.SIGNATURES[name]
    spos = self._stream_pos.get(name)
    enc = []
    for i, (a, t) in enumerate(zip(args, argtypes)):
      if i == spos:
        enc.append(('s', self._stream(a)))
      elif t in (_lib.c_int, _lib.c_int64, ctypes.c_size_t):
        enc.append(('i', int(a)))
      elif t in (_lib.c_float, _lib.c_double):
        enc.append(('f', float(a)))
      elif t is _lib.c_void_p and (isinstance(a, (ctypes.Array, ctypes.Structure)) or hasattr(a, '_obj')):
        # a HOST array / out-parameter behind a void* parameter (edet_preprocess_infer's mean, std and scale)
        enc.append(('b',) + _blob_of(getattr(a, '_obj', a)))
      elif t is _lib.c_void_p:
        if isinstance(a, ctypes.c_void_p):
          a = a.value
        enc.append(('p', int(a)) if a else ('n',))
      elif a is None:
        enc.append(('n',))
      else:      # pointer to a structure / array / scalar on the host
        obj = getattr(a, '_obj', a)
        enc.append(('b',) + _blob_of(obj))
    self._ops.append(('call', name, enc))

  def event_record(self, stream_handle):
    """-> event id; the event is recorded on the stream at this point of the program."""
    if self._ops is None:
      return None
    ev = self.nevents
    self.nevents += 1
    self._ops.append(('evrec', ev, self._stream(stream_handle)))
    return ev

  def stream_wait(self, stream_handle, ev):
    if self._ops is not None and ev is not None:
      self._ops.append(('wait', self._stream(stream_handle), ev))

  def allreduce(self, tensor, stream_handle):
    """Marks the data-parallel gradient exchange (SUM over the replicas, in place) at this point of the program."""
    if self._ops is not None:
      self._ops.append(('allreduce', tensor.data_ptr(), tensor.numel(), self._stream(stream_handle)))

  def name_buffer(self, name, tensor):
    self.names[name] = (tensor.data_ptr(), tensor.numel() * tensor.element_size())
    self._keep.append(tensor)

  def device_table(self, tensor, relocs):
    """A device buffer whose (initial) contents hold device pointers: relocs = [(byte offset, pointer value)]."""
    self._keep.append(tensor)
    for at, p in relocs:
      if p:
        self.dev_relocs.append((tensor.data_ptr() + at, int(p)))

  # ---- resolution against the allocator + writing ----------------------------------------------------------------
  def live_blocks(self):
    """Sorted [(address, bytes)] of the caching allocator's allocated blocks."""
    out = []
    for seg in torch.cuda.memory_snapshot():
      addr = seg['address']
      for b in seg['blocks']:
        a = b.get('address', addr)
        if b['state'] == 'active_allocated':
          out.append((a, b['size']))
        addr = a + b['size']
    out.sort()
    return out

  def snapshot_initial_state(self, persistent, max_bytes=32 << 20, without=()):
    """Copies to the host what the replay must start from: every live block that holds a `persistent` tensor, and every
    other live block of at most max_bytes (tables, scalars, inputs).  The blocks of the tensors in `without` (inputs the
    host writes before it runs anything) get no initial contents whatever their size.  Call AFTER a warm-up pass (all
    buffers exist) and BEFORE the recorded passes."""
    # an executor that is garbage but not yet collected (it sits in reference cycles) still owns live blocks; collected
    # while the copies below run, its private pool is released and a listed block is gone: collect first
    gc.collect()
    torch.cuda.synchronize()
    blocks = self.live_blocks()
    starts = [a for a, _ in blocks]

    def block_of(t):
      i = bisect.bisect_right(starts, t.data_ptr()) - 1
      assert i >= 0 and t.data_ptr() < blocks[i][0] + blocks[i][1], 'persistent tensor outside the allocator'
      return i
    must = {block_of(t) for t in persistent}
    skip = {block_of(t) for t in without}
    assert not (must & skip), 'an input shares its allocation with persistent state'
    self._initial = {}
    for i, (a, n) in enumerate(blocks):
      if i in skip:
        continue
      if i in must or n <= max_bytes:
        from automl_amd import net_c
        self._initial[a] = net_c.copy_to_host(a, n)

  def write(self, path):
    """Resolves every recorded device pointer to (buffer, offset) and writes the plan."""
    assert self._ops is None
    blocks = self.live_blocks()
    starts = [a for a, _ in blocks]
    used = {}          # block index -> buffer id

    def resolve(p):
      i = bisect.bisect_right(starts, p) - 1
      if i < 0 or p >= blocks[i][0] + blocks[i][1]:
        raise _lib.EdetError('plan: device pointer 0x%x is not inside a live allocation (a temporary freed during '
                             'the recorded pass?)' % p)
      if i not in used:
        used[i] = len(used)
      return used[i], p - blocks[i][0]

    fn_ids = {}
    progs = []
    for pname, ops in self.programs:
      body = bytearray()
      for op in ops:
        if op[0] == 'call':
          _, name, enc = op
          fid = fn_ids.setdefault(name, len(fn_ids))
          body += struct.pack('<BHB', 0, fid, len(enc))
          for e in enc:
            if e[0] == 'i':
              body += struct.pack('<Bq', 0, e[1])
            elif e[0] == 'f':
              body += struct.pack('<Bd', 1, e[1])
            elif e[0] == 'p':
              b, off = resolve(e[1])
              body += struct.pack('<BIQ', 2, b, off)
            elif e[0] == 's':
              body += struct.pack('<BI', 3, e[1])
            elif e[0] == 'n':
              body += struct.pack('<B', 5)
            else:
              _, raw, relocs = e
              body += struct.pack('<BI', 4, len(raw)) + raw + struct.pack('<H', len(relocs))
              for at, p in relocs:
                b, off = resolve(p)
                body += struct.pack('<IIQ', at, b, off)
        elif op[0] == 'evrec':
          body += struct.pack('<BII', 1, op[1], op[2])
        elif op[0] == 'wait':
          body += struct.pack('<BII', 2, op[1], op[2])
        else:
          b, off = resolve(op[1])
          body += struct.pack('<BIQQI', 3, b, off, op[2], op[3])
      progs.append((pname, len(ops), bytes(body)))
    names = []
    for n, (p, nbytes) in sorted(self.names.items()):
      b, off = resolve(p)
      names.append((n, b, off, nbytes))
    props = dict(self.props)
    if self.variables:
      props['num_variables'] = len(self.variables)
    for n, v in sorted(props.items()):
      names.append((n, NULL_BUF, int(v), 0))
    devrel = []
    for at, p in self.dev_relocs:
      devrel.append(resolve(at) + resolve(p))

    def s16(text):
      raw = text.encode()
      return struct.pack('<H', len(raw)) + raw

    by_id = sorted(used.items(), key=lambda kv: kv[1])
    head = bytearray(MAGIC + struct.pack('<IIIIIIII', VERSION, len(by_id), len(names), len(self.streams), self.nevents,
                                         len(progs), len(fn_ids), len(devrel)))
    for name, _ in sorted(fn_ids.items(), key=lambda kv: kv[1]):
      head += s16(name)
    table_at = len(head)
    head += b'\0' * (16 * len(by_id))
    for n, b, off, nbytes in names:
      head += s16(n) + struct.pack('<IQQ', b, off, nbytes)
    for b, at, tb, toff in devrel:
      head += struct.pack('<IQIQ', b, at, tb, toff)
    for pname, nops, body in progs:
      head += s16(pname) + struct.pack('<I', nops) + body
    if self.variables:
      head += VARS_MAGIC + struct.pack('<I', len(self.variables))
      for name, shape, trainable, off, count in self.variables:
        shape = tuple(int(d) for d in shape)
        assert len(shape) <= MAX_RANK, (name, shape)
        head += s16(name) + struct.pack('<BB%dQQQ' % len(shape), 1 if trainable else 0, len(shape), *shape, int(off), int(count))
    pos = (len(head) + 255) // 256 * 256
    table = bytearray()
    payload = []
    for bi, _ in by_id:
      a, n = blocks[bi]
      init = getattr(self, '_initial', {}).get(a)
      if init is not None and len(init) == n:
        table += struct.pack('<QQ', n, pos)
        payload.append((pos, init))
        pos = (pos + n + 255) // 256 * 256
      else:
        table += struct.pack('<QQ', n, 0)
    head[table_at:table_at + len(table)] = table
    with open(path, 'wb') as f:
      f.write(head)
      for at, init in payload:
        f.seek(at)
        f.write(init.tobytes())
    return {'buffers': len(by_id), 'initialised': len(payload), 'bytes': pos, 'programs': {p: n for p, n, _ in progs},
            'entry_points': len(fn_ids), 'streams': len(self.streams), 'events': self.nevents}


class _Cursor(object):
  """The one reader of plan and state files: forward through a file's bytes, every read checked against what remains.
  ValueError (path, what was being read) for a read past the end."""

  def __init__(self, path, kind):
    self.path, self.kind, self.pos = path, kind, 0
    with open(path, 'rb') as f:      # mapped, not read: a plan carries its initial contents, of which nothing is decoded
      self.size = os.fstat(f.fileno()).st_size
      self.data = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if self.size else b''

  def fail(self, what):
    return ValueError('%s: %s' % (self.path, what))

  def raw(self, n, what):
    if n > len(self.data) - self.pos:
      raise self.fail('truncated %s (%s)' % (self.kind, what))
    self.pos += n
    return self.data[self.pos - n:self.pos]

  def take(self, fmt, what):
    vals = struct.unpack('<' + fmt, self.raw(struct.calcsize('<' + fmt), what))
    return vals if len(vals) > 1 else vals[0]

  def s16(self, what):
    return self.raw(self.take('H', what), what).decode(errors='replace')

  def count(self, n, min_record, what):
    """n records of at least min_record bytes each must fit what remains (asked before anything loops n times)."""
    if n > (len(self.data) - self.pos) // min_record:
      raise self.fail('truncated %s (%s)' % (self.kind, what))
    return n


def _fits(off, n, cap):
  return n <= cap and off <= cap - n


def read_plan(path):
  """The whole plan decoded and checked (CPU; the mirror of csrc/plan_file.cpp, except that the variable table is not held
  against its arenas and the optimizer properties are not read): 'version', 'entry_points', 'buffers' [(bytes, init offset)],
  'names' {name: (buf, offset, bytes)}, 'streams', 'events', 'programs', 'device_relocations' (counts); 'ops': program ->
  list of ('call', entry point, [args]) / ('evrec', event, stream) / ('wait', stream, event) / ('allreduce', buf, off, count,
  stream); args: ('i', v) ('f', v) ('p', buf, off) ('s', idx) ('b', bytes, [(at, buf, off)]) ('n',);
  'device_relocation_table' [(buf, at, target buf, target offset)]; 'variables': the variable table as [{'name', 'shape',
  'trainable', 'offset', 'count'}] (offset / count in elements of the variable's arena), empty for a plan written without
  one.  ValueError for a file that is not a plan or that the library's loader would refuse for its structure."""
  c = _Cursor(path, 'plan')
  if c.data[:8] != MAGIC:
    raise c.fail('not a plan file')
  c.pos = 8
  version, nbuf, nnames, nstreams, nevents, nprog, nfn, ndevreloc = c.take('IIIIIIII', 'header')
  if version != VERSION:
    raise c.fail('plan version %d (this reader knows version %d)' % (version, VERSION))
  if not 1 <= nstreams <= 255:
    raise c.fail('bad stream count %d' % nstreams)
  arity = {name: len(args) for name, args in header_prototypes().items()}
  fns = [c.s16('entry-point names') for _ in range(c.count(nfn, 2, 'entry-point names'))]
  for name in fns:
    if name not in arity:
      raise c.fail('the plan calls %s, which this library does not export' % name)
  bufs = [c.take('QQ', 'buffer table') for _ in range(c.count(nbuf, 16, 'buffer table'))]

  def ref(b, off, null=False):
    return (null and b == NULL_BUF) or (b < nbuf and off <= bufs[b][0])
  names = {}
  for _ in range(c.count(nnames, 22, 'names')):
    n = c.s16('names')
    b, off, nbytes = names[n] = c.take('IQQ', 'names')
    if b != NULL_BUF and not (b < nbuf and _fits(off, nbytes, bufs[b][0])):
      raise c.fail("bad named buffer '%s'" % n)
  devrel = [c.take('IQIQ', 'device relocations') for _ in range(c.count(ndevreloc, 24, 'device relocations'))]
  for b, at, tb, toff in devrel:
    if not (b < nbuf and _fits(at, 8, bufs[b][0]) and ref(tb, toff)):
      raise c.fail('bad device relocation')
  progs = {}
  for _ in range(c.count(nprog, 6, 'programs')):
    name = c.s16('program header')
    what = "program '%s'" % name
    ops = []
    for _ in range(c.count(c.take('I', 'program header'), 4, 'program header')):
      kind = c.take('B', what)
      if kind == 0:
        fid, nargs = c.take('HB', what)
        if fid >= nfn:
          raise c.fail('bad entry-point index in %s' % what)
        if nargs != arity[fns[fid]]:
          raise c.fail('%s takes %d arguments, the plan passes %d' % (fns[fid], arity[fns[fid]], nargs))
        args = []
        for _ in range(nargs):
          t = c.take('B', what)
          if t == 0:
            args.append(('i', c.take('q', what)))
          elif t == 1:
            args.append(('f', c.take('d', what)))
          elif t == 2:
            args.append(('p',) + c.take('IQ', what))
            if not ref(*args[-1][1:], null=True):
              raise c.fail('bad device pointer')
          elif t == 3:
            args.append(('s', c.take('I', what)))
            if args[-1][1] >= nstreams:
              raise c.fail('bad stream index')
          elif t == 4:
            n = c.take('I', what)
            if n > 1 << 20:
              raise c.fail('bad argument blob')
            raw = c.raw(n, 'blob')
            relocs = [c.take('IIQ', what) for _ in range(c.count(c.take('H', what), 16, 'blob relocations'))]
            if not all(_fits(at, 8, n) and ref(b, off) for at, b, off in relocs):
              raise c.fail('bad blob relocation')
            args.append(('b', raw, relocs))
          elif t == 5:
            args.append(('n',))
          else:
            raise c.fail('unknown argument type %d' % t)
        ops.append(('call', fns[fid], args))
      elif kind in (1, 2):
        a, b = c.take('II', what)
        ev, st = (a, b) if kind == 1 else (b, a)
        if ev >= nevents or st >= nstreams:
          raise c.fail('bad event operation')
        ops.append(('evrec' if kind == 1 else 'wait', a, b))
      elif kind == 3:
        b, off, count, stream = c.take('IQQI', what)
        if not (b < nbuf and count <= bufs[b][0] // 4 and _fits(off, 4 * count, bufs[b][0]) and stream < nstreams):
          raise c.fail('bad all-reduce operation')
        ops.append(('allreduce', b, off, count, stream))
      else:
        raise c.fail('unknown operation %d' % kind)
    progs[name] = ops
  variables = []
  if 'num_variables' in names:
    if c.data[c.pos:c.pos + 8] != VARS_MAGIC:
      raise c.fail('the plan announces a variable table and holds none')
    c.pos += 8
    nvars = c.count(c.take('I', 'variable table'), 20, 'variable table')
    if nvars != names['num_variables'][1]:
      raise c.fail('variable table of %d entries, property num_variables = %d' % (nvars, names['num_variables'][1]))
    seen = set()
    for _ in range(nvars):
      name = c.s16('variable table')
      trainable, rank = c.take('BB', name)
      if rank > MAX_RANK:
        raise c.fail('bad variable table (variable %s of rank %d)' % (name, rank))
      shape = tuple(c.take('Q', name) for _ in range(rank))
      off, count = c.take('QQ', name)
      if count != int(np.prod(shape, dtype=object)) or name in seen:
        raise c.fail("bad variable table (variable '%s': count %d of shape %s, or twice)" % (name, count, shape))
      seen.add(name)
      variables.append({'name': name, 'shape': shape, 'trainable': bool(trainable), 'offset': off, 'count': count})
  for i, (nbytes, at) in enumerate(bufs):
    if at and not _fits(at, nbytes, c.size):
      raise c.fail('truncated plan (the initial contents of buffer %d lie outside the file)' % i)
  return {'version': version, 'entry_points': fns, 'buffers': bufs, 'names': names, 'streams': nstreams, 'events': nevents,
          'programs': nprog, 'device_relocations': ndevreloc, 'ops': progs, 'device_relocation_table': devrel,
          'variables': variables}


def read_summary(path):
  """read_plan without the operations and the device relocation table (the format test and `python -m automl_amd.plan
  FILE`)."""
  out = read_plan(path)
  del out['ops'], out['device_relocation_table']
  return out


OPTIMIZER_IDS = {'sgd': 0, 'adam': 1, 'lion': 2}      # property 'optimizer'


def double_bits(v):
  return struct.unpack('<Q', struct.pack('<d', float(v)))[0]


def bits_double(bits):
  return struct.unpack('<d', struct.pack('<Q', int(bits) & 0xffffffffffffffff))[0]


def optimizer_props(update, iterations):
  """The properties a plan carries of its update step (layer_engine.Update): the optimizer's id, the iteration count and the
  optimizer's constants as the bit patterns of doubles.  Pure Python."""
  if update.kind not in OPTIMIZER_IDS:
    raise ValueError('plans record the sgd, adam and lion updates, not %r' % (update.kind,))
  props = {'optimizer': OPTIMIZER_IDS[update.kind], 'iterations': int(iterations)}
  if update.kind == 'adam':
    constants = (('adam_beta1_bits', update.momentum), ('adam_beta2_bits', update.beta2), ('adam_epsilon_bits', update.epsilon))
  elif update.kind == 'lion':
    constants = (('lion_beta1_bits', update.momentum), ('lion_beta2_bits', update.beta2), ('lion_wd_bits', update.wd or 0.0))
  else:
    constants = ()
  for key, v in constants:
    props[key] = double_bits(v)
  return props


def write_state(path, variables, ema=None, momentum=None, adam_v=None, iterations=0):
  """Writes a state file (the format edet_net_save_state writes and edet_net_load_state reads): name -> fp32 array in the
  reference layout per slot -- the variables' values, the EMA shadows, the momentum slots (Adam: first moments), Adam's
  second moments -- and the optimizer's iteration count.  Pure numpy."""
  records = []
  for slot, values in enumerate((variables, ema, momentum, adam_v)):
    for name, v in (values or {}).items():
      a = np.asarray(v, dtype='<f4')      # (ascontiguousarray would turn a 0-d variable into [1]; tobytes is C order)
      if a.ndim > MAX_RANK:
        raise ValueError('variable %s: rank %d (at most %d)' % (name, a.ndim, MAX_RANK))
      raw = name.encode()
      records.append(struct.pack('<H', len(raw)) + raw + struct.pack('<BB%dQQ' % a.ndim, slot, a.ndim, *a.shape, a.size)
                     + a.tobytes())
  with open(path, 'wb') as f:
    f.write(STATE_MAGIC + struct.pack('<IIq', STATE_VERSION, len(records), int(iterations)))
    for r in records:
      f.write(r)


def read_state(path):
  """-> {'variables': {name: array}, 'ema': {...}, 'momentum': {...}, 'adam_v': {...}, 'iterations': n} of a state file;
  ValueError for a file that is not one, is truncated or carries bytes after its last record."""
  c = _Cursor(path, 'state file')
  if c.data[:8] != STATE_MAGIC:
    raise ValueError('%s is not a state file' % path)
  c.pos = 8
  version, nrec, iterations = c.take('IIq', 'header')
  if version != STATE_VERSION:
    raise c.fail('state file version %d (this reader knows version %d)' % (version, STATE_VERSION))
  out = {k: {} for k in STATE_SLOTS}
  for _ in range(c.count(nrec, 12, 'records')):
    name = c.s16('name')
    slot, rank = c.take('BB', name)
    if slot >= len(STATE_SLOTS) or rank > MAX_RANK:
      raise c.fail('variable %s: bad slot %d / rank %d' % (name, slot, rank))
    shape = tuple(c.take('Q', name) for _ in range(rank))
    count = c.take('Q', name)
    if count != int(np.prod(shape, dtype=object)):
      raise c.fail('bad count (variable %s, %d elements of shape %s)' % (name, count, shape))
    if name in out[STATE_SLOTS[slot]]:
      raise c.fail('variable %s twice in slot %s' % (name, STATE_SLOTS[slot]))
    payload = c.raw(4 * c.count(count, 4, name), name)
    out[STATE_SLOTS[slot]][name] = np.frombuffer(payload, '<f4').reshape(shape).copy()
  if c.pos != len(c.data):
    raise c.fail('%d bytes after the last record' % (len(c.data) - c.pos))
  out['iterations'] = iterations
  return out


def train_pass(eng, images, dlabels, learning_rate, ema_decay):
  """One training step in the structure the plan records (and edet_train_step replays): per-step scalars, forward with
  batch statistics, device-side normalizer, losses + backward, L2 + clip applied locally, [gradient exchange], update."""
  eng.set_hyper(learning_rate, ema_decay)
  eng.forward(images, training=True)
  eng.set_normalizer(dlabels['mean_num_positives'])
  glabels = dict(dlabels)
  glabels['normalizer'] = 'device'
  eng.loss_backward(glabels)
  eng.optimizer_local(True)
  if _lib.recorder is not None:
    _lib.recorder.allreduce(eng.grads_flat, eng.stream)
  eng.optimizer_apply(bool(ema_decay), True)


class _Detect(object):
  """Buffers and launches of the `detect` program: EfficientDetModel.call with pre_mode='infer', post_mode='global'
  (efficientdet_keras.py:920-1000) -- edet_preprocess_infer, the network, the level outputs without their padding columns,
  pre_nms (tf2/postprocess.py:120-157), global NMS + clip + rescale (:375-406).  Every buffer exists BEFORE the recorded
  pass (the Python host's own path, automl_amd/postprocess.py, allocates its temporaries inside the calls)."""

  def __init__(self, net, eng, images, raw_hw):
    from automl_amd import anchors as anchors_lib, postprocess, utils
    c = eng.config
    self.eng, self.params = eng, c.as_dict()
    dev = images.device
    b = int(images.shape[0])
    rh, rw = int(raw_hw[0]), int(raw_hw[1])
    self.b, self.rh, self.rw = b, rh, rw
    self.oh, self.ow = int(images.shape[1]), int(images.shape[2])
    self.raw = torch.zeros((b, rh, rw, 3), dtype=torch.uint8, device=dev)
    self.images = torch.empty_like(images)
    self.mean = (ctypes.c_float * 3)(*[float(v) for v in np.broadcast_to(np.asarray(c.mean_rgb, np.float32).reshape(-1), (3,))])
    self.std = (ctypes.c_float * 3)(*[float(v) for v in np.broadcast_to(np.asarray(c.stddev_rgb, np.float32).reshape(-1), (3,))])
    self.scale = ctypes.c_float(0.0)
    self.tdt = _lib.EDET_BF16 if images.dtype == torch.bfloat16 else _lib.EDET_F32
    a = anchors_lib.Anchors(c.min_level, c.max_level, c.num_scales, c.aspect_ratios, c.anchor_scale, (self.oh, self.ow))
    self.anchors = torch.as_tensor(np.asarray(a.boxes, np.float32)).to(dev).contiguous()
    self.n = int(self.anchors.shape[0])
    self.na = eng.spec.num_anchors
    self.k = int(c.nms_configs.get('max_nms_inputs', 0) or 0)
    kk = self.k if self.k > 0 else self.n
    self.boxes = torch.empty((b, kk, 4), dtype=torch.float32, device=dev)
    self.scores = torch.empty((b, kk), dtype=torch.float32, device=dev)
    self.classes = torch.empty((b, kk), dtype=torch.int32, device=dev)
    self.ws_topk = None
    if self.k > 0:
      need = ctypes.c_size_t(0)
      _lib.call('edet_pre_nms_topk_workspace_bytes', b, self.k, ctypes.byref(need))
      self.ws_topk = torch.empty((max(need.value, 8),), dtype=torch.uint8, device=dev)
    self.cfg = postprocess._tf_nms_cfg(c.nms_configs)
    self.m = int(self.cfg.max_output_size)
    need = ctypes.c_size_t(0)
    _lib.call('edet_nms_workspace_bytes', b, kk, 1, self.m, ctypes.byref(need))
    self.ws_nms = torch.empty((max(need.value, 8),), dtype=torch.uint8, device=dev)
    self.out_index = torch.empty((b, self.m), dtype=torch.int32, device=dev)
    self.out_score = torch.empty((b, self.m), dtype=torch.float32, device=dev)
    self.valid = torch.empty((b,), dtype=torch.int32, device=dev)
    self.nms_boxes = torch.empty((b, self.m, 4), dtype=torch.float32, device=dev)
    self.nms_scores = torch.empty((b, self.m), dtype=torch.float32, device=dev)
    self.nms_classes = torch.empty((b, self.m), dtype=torch.float32, device=dev)
    # image_scales of preprocess_infer: one value per image, a function of the two sizes only (the library returns it on
    # the host); kept on the device as postprocess_global's rescale wants it
    self.scales = torch.zeros((b,), dtype=torch.float32, device=dev)
    self.compact = None      # per level (cls, box) without padding columns: made by the first pass (needs the views)
    self.clip_hw = utils.parse_image_size((self.oh, self.ow))

  def run(self):
    eng = self.eng
    st = eng.stream
    _lib.call('edet_preprocess_infer', self.raw.data_ptr(), 0, self.b, self.rh, self.rw, self.oh, self.ow, self.mean, self.std,
              self.images.data_ptr(), ctypes.byref(self.scale), self.tdt, st)
    if not float(self.scales[0]):
      self.scales.fill_(self.scale.value)      # (before the recorded pass: the warm-up pass does this once)
    eng.forward(self.images, training=False)
    views = list(zip(eng.cls_views, eng.box_views))
    if self.compact is None:
      self.compact = [tuple(torch.empty((v.raw.n, v.raw.h, v.raw.w, v.raw.c), dtype=v.raw.data.dtype, device=self.raw.device)
                            for v in pair) for pair in views]
    dts = {pair[i].raw.data.dtype for pair in views for i in (0, 1)}
    assert len(dts) == 1, 'class and box outputs of one storage type'
    dt = dts.pop()
    for pair, outs in zip(views, self.compact):
      for v, o in zip(pair, outs):
        r = v.raw
        _lib.call('edet_compact_rows', _lib.ptr(r.data), r.n * r.h * r.w, r.c, r.ld, _lib.ptr(o), r.data.element_size(), st)
    nlev = len(views)
    cp = (ctypes.c_void_p * nlev)(*[o[0].data_ptr() for o in self.compact])
    bp = (ctypes.c_void_p * nlev)(*[o[1].data_ptr() for o in self.compact])
    lp = (ctypes.c_int * nlev)(*[pair[0].raw.h * pair[0].raw.w for pair in views])
    edt = _lib.EDET_BF16 if dt == torch.bfloat16 else _lib.EDET_F32
    nc = eng.config.num_classes
    if self.k > 0:
      _lib.call('edet_pre_nms_topk', cp, bp, lp, nlev, self.b, self.na, nc, self.anchors.data_ptr(), edt, self.k,
                self.ws_topk.data_ptr(), self.ws_topk.numel(), self.boxes.data_ptr(), self.scores.data_ptr(),
                self.classes.data_ptr(), st)
    else:
      _lib.call('edet_pre_nms', cp, bp, lp, nlev, self.b, self.na, nc, self.anchors.data_ptr(), edt, self.boxes.data_ptr(),
                self.scores.data_ptr(), self.classes.data_ptr(), st)
    kk = int(self.scores.shape[1])
    _lib.call('edet_nms', self.boxes.data_ptr(), self.scores.data_ptr(), self.classes.data_ptr(), self.b, kk, 1,
              ctypes.byref(self.cfg), self.ws_nms.data_ptr(), self.ws_nms.numel(), self.out_index.data_ptr(),
              self.out_score.data_ptr(), self.valid.data_ptr(), st)
    _lib.call('edet_nms_gather', self.boxes.data_ptr(), self.classes.data_ptr(), self.out_index.data_ptr(),
              self.out_score.data_ptr(), self.b, kk, self.m, _lib.NMS_PAD_INDEX0, float(self.clip_hw[0]), float(self.clip_hw[1]),
              self.scales.data_ptr(), self.nms_boxes.data_ptr(), self.nms_scores.data_ptr(), self.nms_classes.data_ptr(), st)


def record_network(net, images, labels=None, path='efficientdet.plan', learning_rate=0.01, ema_decay=0.0,
                   max_init_bytes=32 << 20, detect_raw_hw=None, raw_images=None, keep_inputs=True):
  """Records `forward` (EfficientDetNet.call, inference BatchNorm) and -- with labels -- `train_step` of a network
  (efficientdet_net.EfficientDetNet / train_lib.EfficientDetNetTrain) on device tensors `images` [B,H,W,3] and the label
  dictionary of train_step, and writes the plan.  Returns (summary, expected): `expected` holds what the Python host
  computed in the recorded passes (numpy), for a replay to be compared with.

  detect_raw_hw = (H, W): also records `detect` (EfficientDetModel.call on raw uint8 images of that size: preprocessing,
  network, global-NMS post-processing; edet_detect); raw_images [B,H,W,3] uint8 are the recorded inputs (default zeros).

  keep_inputs=False: "images", the target buffers and "raw_images" get no initial contents (zero-filled at edet_create; the
  host writes them before it runs a program), and the file loses their bytes.

  The plan also holds the variable table (one entry per variable of ParamArena.offsets: what edet_get_variable /
  edet_set_variable / edet_net_save_state address by name) and the optimizer's kind, constants and iteration count.

  The state the plan starts from is the network's state after one un-recorded warm-up pass of each program.
  """
  b, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
  # A plan carries whole allocator blocks.  A buffer that the caching allocator serves from a cached block of an earlier,
  # larger tensor drags that block's slack into the file (up to 1 MiB per large buffer; a block beyond max_init_bytes loses
  # its initial contents instead), so the file would follow whatever the process did before.  A network that gets its
  # executor here gets it -- with the buffers of the warm-up passes and the device copies of the inputs -- from an allocator
  # pool of its own: the same network recorded twice has the same blocks.  (The pool lives as long as the executor.)
  fresh = net.engine is None
  pool = torch.cuda.MemPool() if fresh else None
  with (torch.cuda.use_mem_pool(pool) if fresh else contextlib.nullcontext()):
    eng = net._ensure_engine(b, h, w)
    assert eng.sync_bn is None and eng._overlap_reduce is None, 'plans record the default step structure'
    # The recorder takes any entry point a pass calls, by its ctypes signature: edet_box_iou_loss would be recorded without a
    # word, with the cached anchor table as one more buffer that neither the network-level C ABI nor the plan tests know of.
    if getattr(eng, 'iou_loss', None) is not None:
      raise ValueError('recording a plan of a model with the IoU loss on (set_iou_loss) is not built: plans record the '
                       'detection loss without BoxIouLoss')
    images = net._to_device_images(images, eng)
    dl = None
    if labels is not None:
      dl = net._labels_to_device(labels, eng)
      assert 'mean_num_positives' in dl, "the recorded step computes the normalizer on the device: labels['mean_num_positives']"

    det = None
    if detect_raw_hw is not None:
      det = _Detect(net, eng, images, detect_raw_hw)
      if raw_images is not None:
        det.raw.copy_(torch.as_tensor(raw_images).to(det.raw.device))
    # warm-up: every buffer of both programs exists afterwards
    eng.forward(images, training=False)
    if det is not None:
      det.run()
    if dl is not None:
      train_pass(eng, images, dl, learning_rate, ema_decay)
    torch.cuda.synchronize()
  if fresh:
    eng._plan_pool = pool
  rec = Recorder()
  persistent = [eng.params_flat, eng.velocity, eng.ema, eng.state_flat, eng.seg_flags, eng.seg_offsets, eng.seg_factor,
                eng.hyper]
  inputs = [images]
  if dl is not None:
    inputs += [t for t in dl.values() if torch.is_tensor(t)]
  if getattr(eng.arena, 'adam_v', None) is not None:
    persistent.append(eng.arena.adam_v)
  if det is not None:
    persistent += [det.anchors, det.scales]
    inputs.append(det.raw)
  if keep_inputs:
    rec.snapshot_initial_state(persistent + inputs, max_init_bytes)
  else:
    rec.snapshot_initial_state(persistent, max_init_bytes, without=inputs)
  rec.variables = [(name, shape, tr, off, n) for name, (off, n, shape, tr) in eng.arena.offsets.items()]
  rec.props.update(optimizer_props(eng.update, eng.arena.step_count))
  expected = {}
  # every program re-makes the compute copies of the variables (and, in inference, the BatchNorm vectors): a replayed step
  # follows other replayed steps, whose updates the host-side version counter of this engine has not seen
  eng._cast_version = -1
  rec.begin('forward')
  eng.forward(images, training=False)
  rec.end()
  torch.cuda.synchronize()
  # the logits buffers as stored: [B, h, w, ld] with ld = channels rounded up to 8 (fp32 in an inference pass of a bf16
  # engine, see Engine.logits_f32); the first `channels` of a pixel are the outputs of efficientdet_keras.py:893-915
  for li, (cv, bv) in enumerate(zip(eng.cls_views, eng.box_views)):
    level = eng.config.min_level + li
    for kind, v in (('cls', cv), ('box', bv)):
      t = v.raw.data
      rec.name_buffer('%s_outputs_%d' % (kind, level), t)
      rec.props['%s_outputs_%d.channels' % (kind, level)] = v.raw.c
      rec.props['%s_outputs_%d.ld' % (kind, level)] = v.raw.ld
      rec.props['%s_outputs_%d.height' % (kind, level)] = v.raw.h
      rec.props['%s_outputs_%d.width' % (kind, level)] = v.raw.w
      rec.props['%s_outputs_%d.elem_bytes' % (kind, level)] = t.element_size()
      expected['%s_outputs_%d' % (kind, level)] = t.detach().view(torch.uint8).cpu().numpy().reshape(-1).copy()
  rec.props.update({'batch': b, 'height': h, 'width': w, 'min_level': eng.config.min_level,
                    'max_level': eng.config.max_level, 'num_classes': eng.config.num_classes,
                    'num_anchors': eng.spec.num_anchors, 'storage_elem_bytes': eng.esize,
                    'num_train_elems': int(eng.params_flat.numel())})
  if eng._cast_table is not None:
    names, dev, _, _ = eng._cast_table
    flat = [it for n in names for it in eng._cast_items[n]]
    rec.device_table(dev, [(32 * i + 8 * j, it[j]) for i, it in enumerate(flat) for j in (0, 1)])
  if det is not None:
    eng._cast_version = -1
    rec.begin('detect')
    det.run()
    rec.end()
    torch.cuda.synchronize()
    for name, t in (('raw_images', det.raw), ('detections.boxes', det.nms_boxes), ('detections.scores', det.nms_scores),
                    ('detections.classes', det.nms_classes), ('detections.valid_len', det.valid),
                    ('image_scales', det.scales)):
      rec.name_buffer(name, t)
    rec.props.update({'raw_height': det.rh, 'raw_width': det.rw, 'max_output_size': det.m})
    for k in ('boxes', 'scores', 'classes', 'valid_len'):
      t = {'boxes': det.nms_boxes, 'scores': det.nms_scores, 'classes': det.nms_classes, 'valid_len': det.valid}[k]
      expected['detections.' + k] = t.cpu().numpy().copy()
    rec._keep.append(det)
  if dl is not None:
    eng._cast_version = -1
    rec.begin('train_step')
    train_pass(eng, images, dl, learning_rate, ema_decay)
    rec.end()
    torch.cuda.synchronize()
    expected['params'] = eng.params_flat.cpu().numpy().copy()
    expected['ema'] = eng.ema.cpu().numpy().copy()
    expected['velocity'] = eng.velocity.cpu().numpy().copy()
    expected['bn_state'] = eng.state_flat.cpu().numpy().copy()
    expected['loss_sums'] = eng.loss_sums.cpu().numpy().copy()
    if eng.adam:
      expected['adam_v'] = eng.arena.adam_v.cpu().numpy().copy()
    for k, t in dl.items():
      if torch.is_tensor(t):
        rec.name_buffer(k, t)
  rec.name_buffer('images', images)
  rec.name_buffer('params', eng.params_flat)
  rec.name_buffer('ema', eng.ema)
  rec.name_buffer('velocity', eng.velocity)
  if eng.adam and getattr(eng.arena, 'adam_v', None) is not None:
    rec.name_buffer('adam_v', eng.arena.adam_v)
  rec.name_buffer('bn_state', eng.state_flat)
  rec.name_buffer('loss_sums', eng.loss_sums)
  rec.name_buffer('hyper', eng.hyper)
  for scope, (mask, _) in eng.drop_masks.items():
    rec.name_buffer('drop_mask:%s' % scope, mask)
  return rec.write(path), expected


if __name__ == '__main__':
  import json
  import sys
  s = read_summary(sys.argv[1])
  s['buffers'] = {'count': len(s['buffers']), 'bytes': sum(b[0] for b in s['buffers']),
                  'initialised_bytes': sum(b[0] for b in s['buffers'] if b[1])}
  s['variables'] = len(s['variables'])
  print(json.dumps(s, indent=1))
