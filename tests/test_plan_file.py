"""The host-side parser of plan and state files (automl_amd/csrc/plan_file.cpp) without a GPU, through the stand-alone
checker tests/c_host/plan_check.cpp (the parser and nothing else, built here with the host C++ compiler): it reads what
automl_amd/plan.py reads, it refuses every field value that made the old loader's bounds arithmetic wrap -- and so does the
Python reader, with the one exception named at ARENA -- and it refuses a file cut at any byte."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from automl_amd import _lib, plan
from tests.test_plan import _FakeRecorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the first two names are of one length: the 'twice' case overwrites the second with the first
VARS = [('stem/conv2d/kernel', (3, 3, 3, 32), True, 0, 864),
        ('head/conv2d/kernel', (810,), True, 864, 810),
        ('fpn_cells/cell_0/fnode0/WSM', (), True, 1676, 1),
        ('stem/tpu_batch_normalization/moving_mean', (32,), False, 0, 32)]
PARAMS_ELEMS = 2048
# plan.py reads the variable table without holding it against the named arenas (tests/test_plan_vars.py writes tables
# next to a 'params' buffer that is too small for them, and must keep passing): the one case only the C++ parser refuses
ARENA = 'variable off + count past the arena'


class _Tensor(object):
  def __init__(self, ptr, n):
    self._ptr, self._n = ptr, n

  def data_ptr(self):
    return self._ptr

  def numel(self):
    return self._n


@pytest.fixture(scope='session')
def checker(tmp_path_factory):
  cxx = shutil.which('g++') or next((p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/bin/amdclang++') if os.path.exists(p)), None)
  if cxx is None:
    pytest.skip('no host C++ compiler on this box')
  exe = str(tmp_path_factory.mktemp('plan_check') / 'plan_check')
  cmd = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', os.path.join(ROOT, 'tests', 'c_host', 'plan_check.cpp'),
         os.path.join(ROOT, 'automl_amd', 'csrc', 'plan_file.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr

  def run(*args):
    r = subprocess.run((exe,) + args, capture_output=True, text=True, errors='replace')
    assert r.returncode in (0, 1), (r.returncode, r.stdout, r.stderr)      # anything else: a crash of the parser
    return r.returncode, r.stdout
  return run


def _record(rec, with_table):
  rec.begin('forward', main_stream=0)
  tv = _lib.TView(0x20000 + 512, 0x10000, 0x10000 + 64, None, 1, 2, 8, 8, 16, 16)
  nparts = ctypes.c_int(5)
  rec.on_call('edet_pw_fwd', (ctypes.byref(tv), 0x20000 + 4096, 16, None, 0x20000 + 8192, 24, 24, 0x400000,
                              ctypes.byref(nparts), 1, 0))
  ev = rec.event_record(0)
  rec.stream_wait(0x77, ev)
  rec.on_call('edet_zero', (0x10000 + 128, 256, 0x77))
  rec.on_call('edet_bn_eval', (16, 0x10000, 0x10000, 1e-3, 0x10000, 0x10000, 0x10000, 0x10000, 0))
  rec.end()
  rec.begin('train_step', main_stream=0)
  rec.on_call('edet_zero', (0x20000, 4 * PARAMS_ELEMS, 0))
  rec.allreduce(_Tensor(0x20000, PARAMS_ELEMS), 0)
  rec.end()
  rec.names['params'] = (0x20000, 4 * PARAMS_ELEMS)
  rec.names['bn_state'] = (0x10000 + 1024, 256)
  rec.names['weights'] = (0x20000 + 4096, 1024)
  rec.props['batch'] = 2
  rec.dev_relocs.append((0x10000 + 8, 0x20000 + 4096))
  if with_table:
    rec.variables = list(VARS)
    bits = lambda x: struct.unpack('<Q', struct.pack('<d', x))[0]
    rec.props.update({'optimizer': 1, 'iterations': 7, 'adam_beta1_bits': bits(0.9), 'adam_beta2_bits': bits(0.999)})
  else:
    rec._initial = {0x10000: np.arange(4096, dtype=np.uint8)}


@pytest.fixture(scope='module')
def files(tmp_path_factory):
  """'plain': a plan with initial contents and no variable table; 'table': one with a variable table, Adam's properties
  and no initial contents; 'state': a state file of the table's variables."""
  d = tmp_path_factory.mktemp('plan_files')
  out = {'dir': d}
  for key, with_table in (('plain', False), ('table', True)):
    rec = _FakeRecorder()
    _record(rec, with_table)
    out[key] = str(d / (key + '.plan'))
    rec.write(out[key])
  rng = np.random.default_rng(3)
  values = {name: np.asarray(rng.standard_normal(shape), np.float32) for name, shape, _, _, _ in VARS}
  train = {name: values[name] for name, _, tr, _, _ in VARS if tr}
  out['state'] = str(d / 'net.state')
  plan.write_state(out['state'], values, ema={k: v * 2 for k, v in train.items()}, momentum={k: v * 3 for k, v in train.items()},
                   adam_v={k: v * v for k, v in train.items()}, iterations=12345678901)
  return out


def _fnv1a(raw):
  h = 14695981039346656037
  for b in bytes(raw):
    h = ((h ^ b) * 1099511628211) & 0xffffffffffffffff
  return h


def _render_plan(p):
  """plan.read_plan's dictionary as tests/c_host/plan_check.cpp prints a PlanFile."""
  lines = ['plan version %d buffers %d names %d streams %d events %d programs %d entry_points %d device_relocations %d '
           'variables %d' % (p['version'], len(p['buffers']), len(p['names']), p['streams'], p['events'], p['programs'],
                             len(p['entry_points']), p['device_relocations'], len(p['variables']))]
  lines += ['fn %d %s' % (i, n) for i, n in enumerate(p['entry_points'])]
  lines += ['buffer %d bytes %d init %d' % (i, b[0], b[1]) for i, b in enumerate(p['buffers'])]
  lines += ['name %s buf %d off %d bytes %d' % ((n,) + v) for n, v in p['names'].items()]
  lines += ['devreloc %d+%d to %d+%d' % d for d in p['device_relocation_table']]
  for name, ops in p['ops'].items():
    lines.append('program %s ops %d' % (name, len(ops)))
    for op in ops:
      if op[0] == 'allreduce':
        lines.append('op allreduce %d+%d %d %d' % op[1:])
      elif op[0] != 'call':
        lines.append('op %s %d %d' % op)
      else:
        args = []
        for a in op[2]:
          if a[0] == 'f':
            args.append('f:%016x' % struct.unpack('<Q', struct.pack('<d', a[1]))[0])
          elif a[0] == 'p':
            args.append('p:%d+%d' % a[1:])
          elif a[0] == 'b':
            args.append('b:%d:%016x[%s]' % (len(a[1]), _fnv1a(a[1]), ''.join('%d>%d+%d,' % q for q in a[2])))
          else:
            args.append(':'.join(str(x) for x in a))      # i:<value>, s:<index>, n
        lines.append(' '.join(['op call', op[1]] + args))
  for v in p['variables']:
    lines.append(' '.join(['var', v['name'], 'trainable %d shape' % v['trainable']] + [str(d) for d in v['shape']]
                          + ['off %d count %d' % (v['offset'], v['count'])]))
  return '\n'.join(lines) + '\n'


def _render_state(s):
  recs = [(name, slot, a) for slot, key in enumerate(plan.STATE_SLOTS) for name, a in s[key].items()]
  lines = ['state records %d iterations %d' % (len(recs), s['iterations'])]
  for name, slot, a in recs:
    lines.append(' '.join(['rec', name, 'slot %d shape' % slot] + [str(d) for d in a.shape]
                          + ['count %d fnv %016x' % (a.size, _fnv1a(a.astype('<f4').tobytes()))]))
  return '\n'.join(lines) + '\n'


@pytest.mark.parametrize('key', ['plain', 'table'])
def test_the_two_plan_readers_agree(checker, files, key):
  rc, text = checker(files[key])
  assert rc == 0, text
  got = plan.read_plan(files[key])
  assert text == _render_plan(got)
  assert 'op allreduce' in text and ' b:' in text and 'devreloc' in text and ('var ' in text) == (key == 'table')


def test_the_two_state_readers_agree(checker, files):
  rc, text = checker('--state', files['state'])
  assert rc == 0, text
  assert text == _render_state(plan.read_state(files['state']))
  assert text.count('\nrec ') == 4 + 3 * 3


def _locate(path):
  """Byte offsets of the fields the cases below patch, found by walking the file with plan.py's own cursor."""
  c = plan._Cursor(path, 'plan')
  at, head = {}, {}
  c.pos = 8
  for k in ('version', 'nbuf', 'nnames', 'nstreams', 'nevents', 'nprog', 'nfn', 'ndevreloc'):
    at[k] = c.pos
    head[k] = c.take('I', k)
  for _ in range(head['nfn']):
    c.s16('fn')
  at['buffers'] = c.pos
  head['buffers'] = [c.take('QQ', 'buffer') for _ in range(head['nbuf'])]
  for _ in range(head['nnames']):
    name = c.s16('name')
    at['name:' + name] = c.pos      # -> u32 buf, u64 off, u64 bytes
    c.take('IQQ', 'name')
  at['devreloc'] = c.pos      # -> u32 buf, u64 at, ...
  c.pos += 24 * head['ndevreloc']
  for _ in range(head['nprog']):
    c.s16('program')
    at.setdefault('nops', c.pos)
    for _ in range(c.take('I', 'nops')):
      at.setdefault('op_kind', c.pos)
      kind = c.take('B', 'kind')
      if kind == 0:
        c.take('H', 'fn')
        at.setdefault('nargs', c.pos)
        for _ in range(c.take('B', 'nargs')):
          at.setdefault('arg_type', c.pos)
          t = c.take('B', 'type')
          if t == 3:
            at.setdefault('stream_arg', c.pos)
          if t == 4:
            c.raw(c.take('I', 'blob'), 'blob')
            for _ in range(c.take('H', 'nreloc')):
              at.setdefault('blob_reloc', c.pos)      # -> u32 at, ...
              c.take('IIQ', 'reloc')
          else:
            c.pos += {0: 8, 1: 8, 2: 12, 3: 4, 5: 0}[t]
      elif kind == 3:
        at.setdefault('allreduce', c.pos)      # -> u32 buf, u64 off, u64 count, u32 stream
        c.take('IQQI', 'allreduce')
      else:
        at.setdefault('evrec' if kind == 1 else 'wait', c.pos)      # evrec -> u32 event, u32 stream
        c.take('II', 'event')
  if 'name:num_variables' in at:
    c.pos += 8
    at['nvars'] = c.pos
    for i in range(c.take('I', 'nvars')):
      at['var%d.name' % i] = c.pos + 2
      c.s16('var')
      at['var%d.rank' % i] = c.pos + 1
      _, rank = c.take('BB', 'var')
      c.pos += 8 * rank
      at['var%d.off' % i] = c.pos
      at['var%d.count' % i] = c.pos + 8
      c.take('QQ', 'var')
  return at, head


def _cases(files):
  """(what, file, [(offset, packed value)]) per row of the table of refused values."""
  at, head = _locate(files['plain'])
  vat, vhead = _locate(files['table'])
  size = os.path.getsize(files['plain'])
  (big,) = [i for i, b in enumerate(head['buffers']) if b[0] == 4096]
  assert head['buffers'][big][1] > 0, 'the 4096-byte buffer carries initial contents'
  u8, u32, u64 = (lambda v: struct.pack('<B', v)), (lambda v: struct.pack('<I', v)), (lambda v: struct.pack('<Q', v))
  raw = open(files['plain'], 'rb').read()
  tab = open(files['table'], 'rb').read()
  nargs = raw[at['nargs']]
  n0 = len(VARS[0][0])
  cases = [
      ('blob relocation at', 'plain', [(at['blob_reloc'], u32(0xfffffff8))]),
      ('name off / bytes', 'plain', [(at['name:weights'] + 4, u64(2**64 - 8) + u64(16))]),
      ('device relocation at', 'plain', [(at['devreloc'] + 4, u64(2**64 - 4))]),
      ('all-reduce off / count', 'plain', [(at['allreduce'] + 4, u64(8) + u64(2**62))]),
      ('init_offset', 'plain', [(at['buffers'] + 16 * big + 8, u64(size - 1))]),
      ('stream index', 'plain', [(at['stream_arg'], u32(head['nstreams']))]),
      ('event index', 'plain', [(at['evrec'], u32(head['nevents']))]),
      ('nargs', 'plain', [(at['nargs'], u8(nargs + 1))]),
      ('argument type', 'plain', [(at['arg_type'], u8(9))]),
      ('op kind', 'plain', [(at['op_kind'], u8(9))]),
      ('variable rank', 'table', [(vat['var0.rank'], u8(5))]),
      ('variable count', 'table', [(vat['var0.count'], u64(VARS[0][4] + 1))]),
      (ARENA, 'table', [(vat['var1.off'], u64(PARAMS_ELEMS - VARS[1][4] + 1))]),
      ('variable name twice', 'table', [(vat['var1.name'], tab[vat['var0.name']:vat['var0.name'] + n0])]),
      ('nvars', 'table', [(vat['nvars'], u32(0xffffffff))]),
  ]
  cases += [(k, 'plain', [(at[k], u32(0xffffffff))]) for k in ('nfn', 'nbuf', 'nnames', 'ndevreloc', 'nprog', 'nops')]
  assert len(VARS[1][0]) == n0 and vhead['nnames'] > head['nnames']
  return cases


CASE_NAMES = ['blob relocation at', 'name off / bytes', 'device relocation at', 'all-reduce off / count', 'init_offset',
              'stream index', 'event index', 'nargs', 'argument type', 'op kind', 'variable rank', 'variable count', ARENA,
              'variable name twice', 'nvars', 'nfn', 'nbuf', 'nnames', 'ndevreloc', 'nprog', 'nops']


@pytest.mark.parametrize('what', CASE_NAMES)
def test_a_field_that_wraps_or_is_out_of_range_is_refused(checker, files, what):
  (case,) = [c for c in _cases(files) if c[0] == what]
  raw = bytearray(open(files[case[1]], 'rb').read())
  for off, value in case[2]:
    raw[off:off + len(value)] = value
  bad = str(files['dir'] / ('bad_%s.plan' % CASE_NAMES.index(what)))
  with open(bad, 'wb') as f:
    f.write(raw)
  rc, text = checker(bad)
  assert rc == 1 and text.startswith('error: ') and len(text) > len('error: \n'), (rc, text)
  if what != ARENA:
    with pytest.raises(ValueError):
      plan.read_plan(bad)


def test_every_case_of_the_table_has_a_test(files):
  assert sorted(c[0] for c in _cases(files)) == sorted(CASE_NAMES)


@pytest.mark.parametrize('key', ['plain', 'table'])
def test_every_prefix_of_the_head_is_refused(checker, files, key):
  rc, text = checker('--prefixes', files[key])
  assert rc == 0, text
  first = min([b[1] for b in plan.read_plan(files[key])['buffers'] if b[1]] or [os.path.getsize(files[key])])
  assert text == '%d prefixes refused\n' % first
  raw = open(files[key], 'rb').read()
  for cut in (0, 7, 8, 39, 40, first // 2, first - 1):      # and the Python reader on a few of them
    bad = files['dir'] / ('cut%d_%s.plan' % (cut, key))
    bad.write_bytes(raw[:cut])
    with pytest.raises(ValueError):
      plan.read_plan(str(bad))


def test_a_cut_state_file_and_a_trailing_byte_are_refused(checker, files):
  raw = open(files['state'], 'rb').read()
  for cut in (4, 12, 30, len(raw) // 2, len(raw) - 1):      # the cuts of tests/test_plan_vars.py
    bad = files['dir'] / ('cut%d.state' % cut)
    bad.write_bytes(raw[:cut])
    rc, text = checker('--state', str(bad))
    assert rc == 1 and text.startswith('error: '), (cut, rc, text)
  # the last cut lies inside the last payload: the message names the variable
  assert text == "error: truncated state file (variable '%s')\n" % [v[0] for v in VARS if v[2]][-1]
  bad = files['dir'] / 'tail.state'
  bad.write_bytes(raw + b'\0')
  rc, text = checker('--state', str(bad))
  assert rc == 1 and 'after its last record' in text
