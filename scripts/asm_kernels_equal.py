#!/usr/bin/env python3
"""Compares two `hipcc --cuda-device-only -S` outputs of one source kernel by kernel.

usage: asm_kernels_equal.py PARENT.s CHANGE.s [CHANGE2.s ...]
       asm_kernels_equal.py PARENT.s [PARENT2.s ...] -- CHANGE.s [CHANGE2.s ...]

The compiler emits the kernels of a file in the order in which the host code first names their instantiations, so a
change that only reorders the host code's launch tables moves whole kernels in the assembly.  This script cuts both
files into one block per kernel (its .text, kernel descriptor and resource comment sections) plus the metadata entry of
each kernel and the rest of the file, drops the lines of the per-compilation `__hip_cuid_<hash>` symbol and the function
ordinal from local labels and the comments that quote them (`.LBB<ordinal>_<block>`, `.Lfunc_end<ordinal>`; the comment
column moves with the label's length), and compares the blocks by kernel name.  Prints the names that differ or exist on one side only; exit status 0 = every kernel and
the rest of the file are identical.

Several CHANGE files: the parent source was split.  Their kernels are compared with the parent's as one set; the parts that
exist once per file (what precedes the first kernel, what follows the last, the metadata frame) are then left out.
Several PARENT files before a `--`: kernels moved between sources; both sides are compared as one set each.
"""
import re
import sys

SECTION = re.compile(r'^\t\.section\t\.text\.([^,]+),')
ORDINAL = re.compile(r'(?<![A-Za-z0-9])(L?BB|Lfunc_begin|Lfunc_end)\d+')


def cut(path):
  lines = [re.sub(' +;', ' ;', ORDINAL.sub(r'\1', l)) for l in open(path) if '__hip_cuid_' not in l]
  meta_at = next(i for i, l in enumerate(lines) if l.startswith('\t.amdgpu_metadata'))
  blocks, name, cur = {}, 'HEAD', []
  for l in lines[:meta_at]:
    m = SECTION.match(l)
    if m and m.group(1) != name:
      blocks[name] = cur
      name, cur = m.group(1), []
    cur.append(l)
  # what follows the last kernel (register maximums of the file, ident, stack note) is not part of that kernel
  stop = next((i for i, l in enumerate(cur) if l.startswith('\t.section\t.AMDGPU.gpr_maximums')), len(cur))
  blocks[name], blocks['TAIL'] = cur[:stop], cur[stop:]
  entry, rest = None, []
  for l in lines[meta_at:]:
    if l.startswith('  - .'):
      entry = []
      rest.append(entry)
    elif not l.startswith('    ') and not l.startswith('  - '):
      entry = None
    if entry is not None:
      entry.append(l)
    else:
      blocks.setdefault('META', []).append(l)
  for e in rest:
    key = next(l.split()[-1] for l in e if l.strip().startswith('.name:'))
    blocks['meta:' + key] = e
  return blocks


PER_FILE = ('HEAD', 'TAIL', 'META')


def cut_all(paths, side):
  blocks = {}
  for path in paths:
    part = cut(path)
    twice = sorted(k for k in part if k in blocks and k not in PER_FILE)
    assert not twice, 'in more than one %s file: %s' % (side, twice)
    blocks.update(part)
  return blocks


def main():
  args = sys.argv[1:]
  cutoff = args.index('--') if '--' in args else 1
  parents, changes = args[:cutoff], [p for p in args[cutoff:] if p != '--']
  a, b = cut_all(parents, 'parent'), cut_all(changes, 'change')
  if len(args) > 2:
    for k in PER_FILE:
      a.pop(k, None)
      b.pop(k, None)
  bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
  kernels = [k for k in a if not k.startswith('meta:') and k not in PER_FILE]
  same_order = [k for k in a] == [k for k in b]
  print('%d kernels in %s, %d blocks differ%s' % (len(kernels), ' + '.join(parents), len(bad), '' if same_order else ' (emission order differs)'))
  for k in bad[:10]:
    print('  differs:', k, '(parent only)' if k not in b else '(change only)' if k not in a else '')
  return 1 if bad else 0


if __name__ == '__main__':
  sys.exit(main())
