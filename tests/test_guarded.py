"""tests/guarded.py driven on the CPU by fake "kernels" written in torch.

Each fake kernel gets the arena's payload view and the raw allocation around it (a real kernel gets the payload's
address and may store anywhere near it), so the cases can misbehave exactly as a kernel with a wrong store limit
would: one element past the end, one before the start, the last element forgotten, a 100 KiB overrun.
"""

import re

import pytest
import torch

from tests import guarded
from tests.guarded import Arena, Plain, GUARD

CPU = torch.device('cpu')


def _raw_floats(arena, view):
    """(the allocation as the fake kernel sees it: floats, index 0 = the payload's first element)"""
    buf = next(b for b in arena.bufs if b.view.data_ptr() == view.data_ptr())
    assert buf.start % 4 == 0
    raw = buf.raw[buf.start % 4:]
    n = raw.numel() // 4 * 4
    return raw[:n].view(torch.float32), buf.start // 4


def _kernel(arena, view, lo, hi):
    """Store 1.0 to elements [lo, hi) relative to the payload's first element."""
    raw, origin = _raw_floats(arena, view)
    raw[origin + lo:origin + hi] = 1.0


@pytest.mark.parametrize('shape,dtype', [((37, 288), torch.float32), ((5, 64), torch.float64), ((1,), torch.float32),
                                         ((3, 7), torch.int32), ((9,), torch.int64)])
def test_layout(shape, dtype):
    """Exact payload bytes, 256-byte aligned start, trailing guard at the last byte + 1, sentinel everywhere."""
    arena = Arena(CPU)
    t = arena.out(shape, dtype, name='y')
    buf = arena.bufs[0]
    numel = 1
    for s in shape:
        numel *= s
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous()
    assert buf.nbytes == numel * t.element_size()
    assert t.data_ptr() % 256 == 0
    assert buf.guard('trailing').data_ptr() == t.data_ptr() + buf.nbytes
    assert buf.guard('leading').data_ptr() + GUARD == t.data_ptr()
    assert buf.guard('leading').numel() == GUARD == buf.guard('trailing').numel() == 128 * 1024
    want = guarded.SENTINEL32 if t.element_size() == 4 else guarded.SENTINEL64
    assert bool((guarded.bits(t) == want).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())          # a quiet NaN with a payload
    assert bool((buf.guard('leading').view(torch.int32) == guarded.SENTINEL32).all())
    arena.check_untouched()


def test_workspace_has_exactly_the_bytes_asked_for():
    arena = Arena(CPU)
    for nbytes in (1, 63, 73728 + 36864, 2 * GUARD + 5):
        w = arena.ws(nbytes)
        buf = arena.bufs[-1]
        assert w.dtype == torch.uint8 and w.numel() == nbytes and w.data_ptr() % 256 == 0
        assert buf.guard('trailing').data_ptr() == w.data_ptr() + nbytes
    arena.check()              # workspaces may stay unwritten
    arena.check_untouched()
    arena.bufs[-1].view[2 * GUARD + 4] = 0
    with pytest.raises(AssertionError, match='payload changed'):
        arena.check_untouched()


def test_clean_kernel_passes():
    arena = Arena(CPU)
    y = arena.out((37, 288), name='y')
    part = arena.out((3, 32, 2), torch.float64, name='part')
    ws = arena.ws(1000, name='ws')
    acc = arena.acc((32,), name='dw')
    rm = arena.inout(torch.arange(8.0), name='running_mean')
    _kernel(arena, y, 0, y.numel())
    part.fill_(2.0)
    ws[:10] = 7
    acc += 1.0
    rm.mul_(0.9)
    arena.check()
    assert bool((acc == 1.0).all()) and torch.equal(rm, torch.arange(8.0) * 0.9)


def test_one_element_past_the_end_is_caught():
    arena = Arena(CPU)
    y = arena.out((37, 288), name='y')
    _kernel(arena, y, 0, y.numel() + 1)
    with pytest.raises(AssertionError, match=r'y \(42624-byte payload\): trailing guard dirty, 4 bytes, '
                                             r'bytes 0 \.\. 3 past the payload end'):
        arena.check()


def test_one_element_before_the_start_is_caught():
    arena = Arena(CPU)
    y = arena.out((37, 288), name='y')
    _kernel(arena, y, -1, y.numel())
    with pytest.raises(AssertionError, match=r'y .*leading guard dirty, 4 bytes, bytes 4 \.\. 1 before the payload '
                                             r'start'):
        arena.check()


def test_last_element_left_unwritten_is_caught():
    arena = Arena(CPU)
    y = arena.out((37, 288), name='y')
    _kernel(arena, y, 0, y.numel() - 1)
    with pytest.raises(AssertionError, match=r'y \(10656 elements\): 1 never written, first at element 10655'):
        arena.check()
    # the same for an 8-byte output, and a hole in the middle
    arena = Arena(CPU)
    part = arena.out((4, 32, 2), torch.float64, name='part')
    part.fill_(0.5)
    part.view(-1)[100].copy_(arena.out((1,), torch.float64)[0])
    arena.bufs.pop()
    with pytest.raises(AssertionError, match=r'part \(256 elements\): 1 never written, first at element 100'):
        arena.check()


def test_overrun_by_100_kib_is_still_caught():
    arena = Arena(CPU)
    y = arena.out((37, 288), name='y')
    far = 100 * 1024 // 4
    _kernel(arena, y, 0, y.numel())
    _kernel(arena, y, y.numel() + far - 1, y.numel() + far)     # one float, 100 KiB past the end
    with pytest.raises(AssertionError, match=r'trailing guard dirty, 4 bytes, bytes 102396 \.\. 102399 past'):
        arena.check()
    arena = Arena(CPU)
    y = arena.out((37, 288), name='y')
    _kernel(arena, y, 0, y.numel() + far)                       # a run of 100 KiB past the end
    with pytest.raises(AssertionError, match=r'trailing guard dirty, 102400 bytes, bytes 0 \.\. 102399 past'):
        arena.check()


def test_a_dirty_guard_of_any_kind_of_buffer_is_caught():
    for make in (lambda a: a.ws(1001, name='b'), lambda a: a.acc((5,), name='b'),
                 lambda a: a.inout(torch.ones(3), name='b')):
        arena = Arena(CPU)
        make(arena)
        buf = arena.bufs[0]
        buf.raw[buf.start + buf.nbytes] ^= 0xff          # the first byte past the payload, at any alignment
        with pytest.raises(AssertionError, match=r'b .*trailing guard dirty, 1 bytes, bytes 0 \.\. 0 past'):
            arena.check()
        with pytest.raises(AssertionError, match='trailing guard dirty'):
            arena.check_untouched()


def test_a_stored_sentinel_value_is_compared_as_bits():
    """A legitimate NaN (another payload) or a float equal to nothing is not the sentinel: integers, not floats."""
    arena = Arena(CPU)
    y = arena.out((4,), name='y')
    y.copy_(torch.tensor([float('nan'), 0.0, -0.0, float('inf')]))
    arena.check()
    assert re.match('0x7fc5a5a5', hex(guarded.SENTINEL32))


def test_untouched_detects_a_written_payload():
    arena = Arena(CPU)
    y = arena.out((8,), name='y')
    acc = arena.acc((8,), name='dw')
    rm = arena.inout(torch.ones(8), name='rm')
    arena.check_untouched()
    for t in (y, acc, rm):
        keep = t[3].clone()
        t[3] = 2.0
        with pytest.raises(AssertionError, match='payload changed'):
            arena.check_untouched()
        t[3] = keep
    arena.check_untouched()


def test_plain_allocator_has_the_same_interface():
    plain = Plain(CPU)
    assert bool((plain.out((3, 4)) == 0).all()) and plain.out((2,), torch.float64).dtype == torch.float64
    assert plain.ws(17).numel() == 17 and plain.ws(17).dtype == torch.uint8
    src = torch.arange(4.0)
    t = plain.inout(src)
    t += 1
    assert torch.equal(src, torch.arange(4.0)) and bool((plain.acc((2,)) == 0).all())
    plain.check()
