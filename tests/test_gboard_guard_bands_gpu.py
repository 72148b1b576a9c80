"""Guard bands around every output and workspace of csrc/hrl_gboard.hip's entry points.

The scheme of tests/test_guard_bands_gpu.py, for the file it left out.  Every entry point is called directly through
``_native``, twice on the same inputs:

  run A  outputs and workspaces from ``tests.guarded.Arena``: exact-size payloads prefilled with a NaN sentinel between
         two 128 KiB guards; workspaces of exactly the bytes the ``*_workspace_bytes`` / ``hrl_gboard_pack_bytes``
         function returned; the gradients the weight-gradient kernels are "ADDED into" through ``Arena.acc`` (zeros);
         a y that is a channel slice of a wider buffer through ``Arena.inout`` (random prefill);
  run B  plain zero-filled tensors (the wide buffer: a copy of the same prefill).

After run A no guard byte may have changed and no ``out`` word may still hold the sentinel; every output of run A is
bit-equal to run B's.  Where y is a slice of a wider buffer the channels outside the slice keep their bits and the slice
is bit-equal to the contiguous run's y.  One byte short of the size function's value, every entry point that takes a
size returns HRL_EINVAL with every payload and guard untouched.  The conv runs under each ``hrl_gboard_set_nctw`` value
the shape allows and both ``hrl_gboard_set_whole_ring`` settings (put back in ``finally``), the launch counters showing
that the forced form ran.  No value tolerance appears here: bit equality only (the values are compared with fp64 in
tests/test_gboard_gpu.py and tests/test_gboard_forms_gpu.py).
"""

import contextlib
import ctypes
import types

import pytest
import torch

from handyrl_amd import _native
from tests.guarded import Arena, Plain, bits

pytestmark = pytest.mark.gpu

P = _native.ptr
HW = 36


@contextlib.contextmanager
def _switch(setter, value):
    """Set a process-wide kernel-form switch for the block and put the previous value back."""
    if value is None:
        yield
        return
    fn = getattr(_native.load(), setter)
    prev = fn(value)
    try:
        yield
    finally:
        fn(prev)


def _gen(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return lambda *s: torch.randn(*s, device=dev, generator=g)


def _run(fn, alloc, **kw):
    """One call of a case on one allocator.  A HIP error leaves the process's GPU context unusable: end the session."""
    try:
        outs = fn(alloc, **kw)
        alloc.check()
    except RuntimeError as e:
        if 'HIP' in str(e) or 'hip' in str(e) or 'failed (' in str(e):
            pytest.exit('GPU error, nothing more is launched: %s' % e, returncode=3)
        raise
    return {k: v for k, v in outs.items() if v is not None}


def _ab(dev, fn):
    """Run A guarded, run B plain; A's guards intact, A's outputs fully written and bit-equal to B's.  Returns A's."""
    a = _run(fn, Arena(dev))
    b = _run(fn, Plain(dev))
    assert a and a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape, k
        same = bits(a[k]) == bits(b[k])
        if not bool(same.all()):
            bad = (~same).flatten().nonzero()
            raise AssertionError('%s: run A (guarded) differs from run B (zero-filled) in %d of %d elements, first %d, '
                                 'last %d' % (k, bad.numel(), same.numel(), int(bad[0]), int(bad[-1])))
    return a


def _short(dev, fn):
    """One byte short: HRL_EINVAL before any launch, every payload and guard untouched."""
    arena = Arena(dev)
    with pytest.raises(ValueError):     # _native.check raises ValueError for HRL_EINVAL only
        fn(arena, short=1)
    arena.check_untouched()


def _ok(rc, what):
    _native.check(rc, what)


def _same_bits(a, b):
    return bool((bits(a) == bits(b)).all())


# ------------------------------------------------------------------------------------- hrl_gboard_pack / _pack_adjoint

def _pack(dev, cout, cin_g, adjoint):
    """adjoint: Cin_slice = cout outputs from Cout_fwd = cin_g inputs.  The weight's input slice starts at channel 3."""
    lib, stream = _native.load(), _native.stream_of(dev)
    w = _gen(dev, cout + cin_g)(cin_g, cout + 5, 3, 3) if adjoint else _gen(dev, cout + cin_g)(cout, cin_g + 5, 3, 3)

    def fn(al, short=0):
        nbytes = lib.hrl_gboard_pack_bytes(cout, cin_g)
        assert nbytes > 0 and nbytes % 4 == 0
        packed = al.out((nbytes // 4,), torch.int32, name='packed')
        if adjoint:
            _ok(lib.hrl_gboard_pack_adjoint(P(w), cin_g, cout + 5, 3, cout, P(packed), nbytes - short, stream),
                'hrl_gboard_pack_adjoint')
        else:
            _ok(lib.hrl_gboard_pack(P(w), cout, cin_g, cin_g + 5, 3, P(packed), nbytes - short, stream),
                'hrl_gboard_pack')
        return {'packed': packed}
    return fn


PACK = [(32, 25, False), (8, 64, False), (384, 32, False), (32, 128, True)]
PACK_IDS = ['%dx%d%s' % (co, ci, '-adjoint' if adj else '') for co, ci, adj in PACK]


@pytest.mark.parametrize('cout,cin_g,adjoint', PACK, ids=PACK_IDS)
def test_hrl_gboard_pack(cuda, cout, cin_g, adjoint):
    """One thread per packed 32-bit word, 256 per workgroup: ceil(Cout / 16) x ceil(Cin_g / 32) x 27 x 64 x 4 words,
    the whole buffer and nothing else (a ragged channel tile and a partial column tile are written as zeros)."""
    _ab(cuda, _pack(cuda, cout, cin_g, adjoint))


@pytest.mark.parametrize('cout,cin_g,adjoint', PACK, ids=PACK_IDS)
def test_hrl_gboard_pack_one_byte_short(cuda, cout, cin_g, adjoint):
    _short(cuda, _pack(cuda, cout, cin_g, adjoint))


# ----------------------------------------------------------------------------------------------- hrl_gboard_forward

def _stats(reset=0):
    arr = (ctypes.c_int64 * 11)()
    _native.load().hrl_gboard_launch_stats(ctypes.cast(arr, ctypes.c_void_p), 11, reset)
    return list(arr)


_CONV = {}


def _conv_in(dev, N, cout, cin_g, groups=1):
    key = (N, cout, cin_g, groups)
    if key not in _CONV:
        lib = _native.load()
        r = _gen(dev, 7 * N + cout + cin_g)
        c = types.SimpleNamespace(x=r(N, cin_g * groups, 6, 6), bias=r(cout), wide=r(N, cout + 20, 6, 6))
        w = r(cout, cin_g, 3, 3) * 0.2
        c.pk = torch.zeros(lib.hrl_gboard_pack_bytes(cout, cin_g), dtype=torch.uint8, device=dev)
        _ok(lib.hrl_gboard_pack(P(w), cout, cin_g, cin_g, 0, P(c.pk), c.pk.numel(), _native.stream_of(dev)), 'pack')
        torch.cuda.synchronize(dev)
        _CONV[key] = c
    return _CONV[key]


def _forward(dev, N, cout, cin_g, nctw, wide):
    """wide: y is channels 8 .. 8 + Cout of an (N, Cout + 20, 6, 6) buffer (y_stride = (Cout + 20) x 36)."""
    lib, c, stream = _native.load(), _conv_in(dev, N, cout, cin_g), _native.stream_of(dev)

    def fn(al):
        if wide:
            buf = al.inout(c.wide, name='wide y')
            y = buf[:, 8:8 + cout]
        else:
            buf = y = al.out((N, cout, 6, 6), name='y')
        _stats(reset=1)
        _ok(lib.hrl_gboard_forward(P(c.x), c.x.stride(0), None, 0, N, cin_g, 1, P(c.pk), c.pk.numel(), cout,
                                   P(c.bias), None, None, 1, P(y), y.stride(0), stream), 'hrl_gboard_forward')
        st = _stats()
        assert st[0] == 1 and st[2:5] == [int(nctw == 1), int(nctw == 2), int(nctw == 4)], (nctw, st)
        return {'y': buf}
    return fn


FWD = [(8, 32), (24, 32), (32, 32), (8, 64)]


@pytest.mark.parametrize('N', [1, 15, 16, 17, 33])
@pytest.mark.parametrize('cout,cin_g', FWD, ids=['%dfrom%d' % t for t in FWD])
def test_hrl_gboard_forward(cuda, cout, cin_g, N):
    """16-game tiles: N = 1, 15, 16, 17, 33.  Cout = 8 and 24 end in a partial column tile (8 of 16 channels stored:
    a store of the unstored channels of the last game would land in the trailing guard), Cout = 32 in a full one;
    Cin_g = 64 is the move head's two k-steps.  A lane stores its (game, channel)'s 36 cells as 9 float4.  Each run
    with y_stride = Cout x 36 exactly and with y a channel slice of a wider buffer, whose other channels keep their
    bits; under each NCTW dividing the column tiles and both ring settings."""
    c = _conv_in(cuda, N, cout, cin_g)
    nct = (cout + 15) // 16
    for nctw in [v for v in (1, 2, 4) if nct % v == 0]:
        for ring in ((1, 0) if cin_g <= 32 else (None,)):
            with _switch('hrl_gboard_set_nctw', nctw), _switch('hrl_gboard_set_whole_ring', ring):
                y = _ab(cuda, _forward(cuda, N, cout, cin_g, nctw, False))['y']
                wide = _ab(cuda, _forward(cuda, N, cout, cin_g, nctw, True))['y']
            assert _same_bits(wide[:, 8:8 + cout], y), (nctw, ring)
            assert _same_bits(wide[:, :8], c.wide[:, :8]) and _same_bits(wide[:, 8 + cout:], c.wide[:, 8 + cout:]), \
                (nctw, ring)


@pytest.mark.parametrize('ring', [1, 0], ids=['R9', 'R3'])
@pytest.mark.parametrize('nctw', [1, 2])
def test_hrl_gboard_forward_groups(cuda, nctw, ring):
    """L = 3 groups of 32 -> 32 channels, each reading its own tensor, N = 17; y exactly (17, 96, 6, 6)."""
    lib, stream = _native.load(), _native.stream_of(cuda)
    N, H, L = 17, 32, 3
    c = _conv_in(cuda, N, H * L, H, L)
    xs = [c.x[:, H * i:H * (i + 1)] for i in range(L)]

    def fn(al):
        y = al.out((N, H * L, 6, 6), name='y')
        _stats(reset=1)
        _ok(lib.hrl_gboard_forward_groups(_native.ptr_array(xs), _native.i64_array([x.stride(0) for x in xs]), N, H, L,
                                          P(c.pk), c.pk.numel(), H * L, P(y), y.stride(0), stream),
            'hrl_gboard_forward_groups')
        st = _stats()
        assert st[0] == 1 and st[6] == 1 and st[1] == ring and st[2:5] == [int(nctw == 1), int(nctw == 2), 0], st
        return {'y': y}
    with _switch('hrl_gboard_set_nctw', nctw), _switch('hrl_gboard_set_whole_ring', ring):
        _ab(cuda, fn)


# --------------------------------------------------------------------------------------------- hrl_gboard_pointwise

@pytest.mark.parametrize('N', [1, 7, 57])
@pytest.mark.parametrize('O', [1, 2, 4, 8])
def test_hrl_gboard_pointwise(cuda, O, N):
    """A thread per (game, cell), 256 per workgroup: N = 57 is 2,052 cell rows, one more than eight workgroups.  x2 a
    channel slice of a wider tensor; y_stride = O x 36 exactly, and y a channel slice of a wider buffer whose other
    channels keep their bits."""
    lib, stream = _native.load(), _native.stream_of(cuda)
    r = _gen(cuda, 13 * N + O)
    x1, x2w, w, al_, be = r(N, 16, 6, 6), r(N, 24, 6, 6), r(O, 24), r(O).abs() + 0.5, r(O)
    x2 = x2w[:, 8:16]
    wide0 = r(N, O + 20, 6, 6)

    def case(wide):
        def fn(al):
            if wide:
                buf = al.inout(wide0, name='wide y')
                y = buf[:, 8:8 + O]
            else:
                buf = y = al.out((N, O, 6, 6), name='y')
            _ok(lib.hrl_gboard_pointwise(P(x1), x1.stride(0), 16, P(x2), x2.stride(0), 8, N, P(w), O, P(al_), P(be), 1,
                                         P(y), y.stride(0), stream), 'hrl_gboard_pointwise')
            return {'y': buf}
        return fn
    y = _ab(cuda, case(False))['y']
    wide = _ab(cuda, case(True))['y']
    assert _same_bits(wide[:, 8:8 + O], y)
    assert _same_bits(wide[:, :8], wide0[:, :8]) and _same_bits(wide[:, 8 + O:], wide0[:, 8 + O:])


# ------------------------------------------------------------------------------------------------- hrl_gboard_wgrad

# the five instantiated 32-channel tile shapes (Cout tiles x Cin tiles)
WGRAD_SHAPES = {'4x1': (128, 32), '2x2': (64, 64), '2x1': (64, 32), '1x2': (8, 64), '1x1': (32, 25)}
# one segment of one game; two ragged segments; 25 segments of 2 games (25 tiles for 50 games: far more than
# games / 16); 20 x 300 games = 380 tiles over 256 workgroups (accumulators carried across tiles)
WGRAD_SEGS = {'1': (1,), '17+5': (17, 5), '25x2': (2,) * 25, '20x300': (300,) * 20}
_WGRAD = {}


def _wgrad(dev, shape, segs):
    lib, stream = _native.load(), _native.stream_of(dev)
    cout, cin = WGRAD_SHAPES[shape]
    ns = WGRAD_SEGS[segs]
    total = sum(ns)
    if (shape, total) not in _WGRAD:
        r = _gen(dev, cout + cin + total)
        _WGRAD.clear()      # one set of inputs at a time: the largest is 6,000 games x 160 channels
        _WGRAD[(shape, total)] = (r(total, cin, 6, 6), r(total, cout, 6, 6))
    X, DY = _WGRAD[(shape, total)]
    xs, dys, n0 = [], [], 0
    for n in ns:        # the segments are game ranges of one tensor: nothing is concatenated
        xs.append(X[n0:n0 + n])
        dys.append(DY[n0:n0 + n])
        n0 += n
    tiles = sum((n + 15) // 16 for n in ns)
    bias = cout >= 64
    cin_total, ci0 = cin + 8, 4     # the gradient of a wider weight: input channels 4 .. 4 + Cin of Cin + 8

    def fn(al, short=0):
        dw = al.acc((cout, cin_total, 3, 3), name='dweight')
        db = al.acc((cout,), name='dbias') if bias else None
        wsb = lib.hrl_gboard_wgrad_workspace_bytes(cout, cin, 16 * tiles)
        assert wsb > 0
        ws = al.ws(wsb - short, name='workspace')
        _ok(lib.hrl_gboard_wgrad(_native.ptr_array(xs), _native.i64_array([x.stride(0) for x in xs]),
                                 _native.ptr_array(dys), _native.i64_array([d.stride(0) for d in dys]),
                                 _native.i64_array(list(ns)), len(ns), cout, cin, P(dw), cin_total, ci0, P(db), P(ws),
                                 wsb - short, stream), 'hrl_gboard_wgrad')
        return {'dweight': dw, 'dbias': db}
    return fn, ci0, cin


@pytest.mark.parametrize('segs', list(WGRAD_SEGS))
@pytest.mark.parametrize('shape', list(WGRAD_SHAPES))
def test_hrl_gboard_wgrad(cuda, shape, segs):
    """dweight and dbias are ADDED into (Arena.acc: zeros), the workspace holds exactly
    hrl_gboard_wgrad_workspace_bytes(Cout, Cin, 16 x tiles) bytes: one partial slab (and 32 x cto bias sums) per
    workgroup, min(tiles, 256) workgroups.  The input channels outside the w_ci0 slice keep their zeros."""
    fn, ci0, cin = _wgrad(cuda, shape, segs)
    a = _ab(cuda, fn)
    dw = a['dweight']
    assert bool((bits(dw[:, :ci0]) == 0).all()) and bool((bits(dw[:, ci0 + cin:]) == 0).all())
    assert bool((dw[:, ci0:ci0 + cin] != 0).any())


@pytest.mark.parametrize('shape', list(WGRAD_SHAPES))
def test_hrl_gboard_wgrad_one_byte_short(cuda, shape):
    _short(cuda, _wgrad(cuda, shape, '17+5')[0])


# --------------------------------------------------------------------------------------- hrl_gboard_pointwise_wgrad

def _pw_wgrad(dev, O, C, N):
    lib, stream = _native.load(), _native.stream_of(dev)
    r = _gen(dev, 31 * O + C + N)
    x, dy = r(N, C, 6, 6), r(N, O, 6, 6)

    def fn(al, short=0):
        dw = al.acc((O, C), name='dweight')
        wsb = lib.hrl_gboard_pointwise_wgrad_workspace_bytes(C, O, N)
        assert wsb > 0
        ws = al.ws(wsb - short, name='workspace')
        _ok(lib.hrl_gboard_pointwise_wgrad(P(x), x.stride(0), P(dy), dy.stride(0), N, C, O, P(dw), P(ws), wsb - short,
                                           stream), 'hrl_gboard_pointwise_wgrad')
        return {'dweight': dw}
    return fn


PW_WGRAD = [(1, 64, 1), (8, 256, 64), (4, 8, 513)]


@pytest.mark.parametrize('O,C,N', PW_WGRAD)
def test_hrl_gboard_pointwise_wgrad(cuda, O, C, N):
    """One O x C partial per workgroup, min(N, 512) workgroups, in a workspace of exactly
    hrl_gboard_pointwise_wgrad_workspace_bytes(C, O, N) bytes: one game, 256 channels (one slot per thread), and
    N = 513, one game more than the 512 workgroups (two games each, the last workgroups empty)."""
    a = _ab(cuda, _pw_wgrad(cuda, O, C, N))
    assert bool((a['dweight'] != 0).any())


@pytest.mark.parametrize('O,C,N', PW_WGRAD)
def test_hrl_gboard_pointwise_wgrad_one_byte_short(cuda, O, C, N):
    _short(cuda, _pw_wgrad(cuda, O, C, N))
