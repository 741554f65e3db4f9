"""-m gpu: the copy and cast kernels of csrc/tensor_ops.hip through the C ABI at the edges of their loops and grids: edet_zero's
vector part / byte tail / memset path, edet_cast, edet_cast_to_f32 and edet_axpy_clear one element past what their capped
grids cover in one stride, edet_compact_rows with 2-byte elements and no padding.  Every comparison is exact.
(edet_cast_matrix, edet_cast_batch and the other edet_compact_rows shapes: tests/test_gpu_inference_kernels.py.)"""
import pytest
import torch

from automl_amd import _lib
from automl_amd._lib import call, ptr
from tests import gpu_util as gu

pytestmark = pytest.mark.gpu

THREADS = 256


def _synced(name, *args):
  call(name, *args)
  torch.cuda.synchronize()


# (offset, lengths): a 16-byte-aligned start -- the kernel: no vector part (1, 15), vector only (16), vector + tail (17, 31,
# 37) -- and a start 4 bytes behind a boundary -- the memset path, shorter (1, 12) and longer (13, 40) than the way to the next
ZERO_RANGES = [(16, (1, 15, 16, 17, 31, 37)), (4, (1, 12, 13, 40))]


@pytest.mark.parametrize('offset,lengths', ZERO_RANGES, ids=['aligned', 'offset4'])
def test_zero_ranges(offset, lengths):
  for n in lengths:
    buf = torch.full((128,), 0xA5, dtype=torch.uint8, device=gu.DEV)
    assert buf.data_ptr() % 16 == 0
    _synced('edet_zero', buf.data_ptr() + offset, n, gu.stream())
    got = buf.cpu()
    assert not got[offset:offset + n].any(), (offset, n, got)
    assert bool((got[:offset] == 0xA5).all()) and bool((got[offset + n:] == 0xA5).all()), (offset, n, got)


def test_zero_of_nothing():
  call('edet_zero', None, 0, gu.stream())      # returns 0: call raises on anything else


# the last: 2048 workgroups cover 2048 * 256 elements in one stride; three more
@pytest.mark.parametrize('dt', gu.DTYPES, ids=lambda d: d[0])
@pytest.mark.parametrize('count', [1, 255, 256, 257, 2048 * THREADS + 3])
def test_cast(dt, count):
  name, edt, tdt = dt
  gen = torch.Generator(device=gu.DEV)
  gen.manual_seed(gu.seed_of(('cast', count)))
  src = torch.randn(count, generator=gen, device=gu.DEV, dtype=torch.float32)
  ties = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], device=gu.DEV)[:count]     # ties: to even
  src[:ties.numel()] = ties
  dst = torch.full((count + 1,), 3.0, dtype=tdt, device=gu.DEV)      # one guard element behind the destination
  _synced('edet_cast', ptr(src), ptr(dst), count, edt, gu.stream())
  idt = torch.int16 if tdt == torch.bfloat16 else torch.int32
  assert torch.equal(dst[:count].view(idt), src.to(tdt).view(idt))
  assert float(dst[count]) == 3.0, 'written behind the destination'


def test_widen_and_axpy_past_one_stride():
  """edet_cast_to_f32 (bf16 source, grid cap 4096) and edet_axpy_clear (cap 2048), each one element past its grid's stride."""
  gen = torch.Generator(device=gu.DEV)
  gen.manual_seed(gu.seed_of('past_one_stride'))
  n = 4096 * THREADS + 1
  h = torch.randn(n, generator=gen, device=gu.DEV, dtype=torch.float32).to(torch.bfloat16)
  f = torch.full((n + 1,), 3.0, dtype=torch.float32, device=gu.DEV)
  _synced('edet_cast_to_f32', ptr(h), ptr(f), n, _lib.EDET_BF16, gu.stream())
  assert torch.equal(f[:n].view(torch.int32), h.float().view(torch.int32)) and float(f[n]) == 3.0
  n = 2048 * THREADS + 1
  a = torch.randn(n + 1, generator=gen, device=gu.DEV, dtype=torch.float32)
  b = torch.randn(n + 1, generator=gen, device=gu.DEV, dtype=torch.float32)
  want, a_guard, b_guard = a[:n] + b[:n], float(a[n]), float(b[n])
  _synced('edet_axpy_clear', ptr(a), ptr(b), n, 1, gu.stream())
  assert torch.equal(a[:n], want) and not b[:n].any()
  assert float(a[n]) == a_guard and float(b[n]) == b_guard, 'touched behind the arenas'


# (rows, c, ld, elem_bytes).  test_gpu_inference_kernels.test_compact_rows has c < ld with both element sizes, c == ld with
# 4-byte elements and rows == 0 with 4-byte elements; here: c == ld with 2-byte elements, rows == 0 with 2-byte elements,
# and c < ld one row past the 4096 * 256 words the capped grid covers in one stride
COMPACT_CASES = [(9, 10, 10, 2), (0, 8, 16, 2), (4097, 256, 264, 4)]


@pytest.mark.parametrize('case', COMPACT_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_compact_rows_edges(case):
  rows, c, ld, eb = case
  idt = torch.int16 if eb == 2 else torch.int32
  info = torch.iinfo(idt)
  gen = torch.Generator(device=gu.DEV)
  gen.manual_seed(gu.seed_of(('compact_rows_edges', case)))
  src = torch.randint(info.min, info.max, (max(rows, 1), ld), generator=gen, device=gu.DEV, dtype=idt)
  dst = torch.full((rows * c + 64,), 0x5a5a, dtype=idt, device=gu.DEV)
  _synced('edet_compact_rows', ptr(src), rows, c, ld, ptr(dst), eb, gu.stream())      # (rows == 0 returns 0: call raises otherwise)
  assert bool((dst[rows * c:] == 0x5a5a).all()), 'written behind the destination'
  if rows:
    assert torch.equal(dst[:rows * c].view(rows, c), src[:, :c])
