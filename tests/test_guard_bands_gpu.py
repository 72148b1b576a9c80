"""Guard bands around every output of the tiled conv, BatchNorm, stem, heads and torus entry points.

The value tests compare these kernels with references; they cannot see whether a kernel writes only where it may
and everything it must, because every output there is a fresh ``torch.empty`` (rounded up by the caching allocator,
and on a second run usually the first run's block, still holding correct values).  Here every entry point is called
directly through ``_native``, twice on the same inputs:

  run A  every output and workspace from ``tests.guarded.Arena``: exact-size payloads prefilled with a NaN sentinel
         between two 128 KiB guards; workspaces of exactly the bytes the ``*_workspace_bytes`` function returned;
         side buffers (``part`` rows, partial rows) of exactly the rows the row-count functions returned;
  run B  plain tensors prefilled with zeros (the call the value tests compare with the references).

After run A no guard byte may have changed and no output word may still hold the sentinel; every output of run A is
bit-equal to run B's (the kernels are deterministic; equality also catches a kernel that relies on its output's
previous contents).  Every process-wide switch runs at every value that still exists and is put back in ``finally``.
With ``workspace_bytes - 1`` every entry point that takes a workspace returns HRL_EINVAL and leaves every payload and
guard untouched.

Outputs that accumulate by contract would go through ``Arena.acc``: no header sentence of the entry points covered
here says so, so none does (``hrl_gboard_wgrad``'s "ADDED into" and the rest of csrc/hrl_gboard.hip have a module of
their own, tests/test_gboard_guard_bands_gpu.py).  The running statistics are updated in place ("running stats updated
in place", hrl_bn_forward_train) and go through ``Arena.inout``.

Row counts are the smallest at which a tile limit can go wrong (the constants are quoted in each case's docstring):
1, tile - 1, tile, tile + 1, one row more than one workgroup covers and, where that is at most about 20,000 rows,
one row more than one full grid-stride pass.  No value tolerance appears here: bit equality only.
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
EPS, MOM = 1e-5, 0.1


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
    """Run A guarded, run B plain; A's guards intact, A's outputs fully written and bit-equal to B's."""
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


def _short(dev, fn):
    """workspace_bytes - 1: HRL_EINVAL before any launch, every payload and guard untouched."""
    arena = Arena(dev)
    with pytest.raises(ValueError):     # _native.check raises ValueError for HRL_EINVAL only
        fn(arena, short=1)
    arena.check_untouched()


def _ok(rc, what):
    _native.check(rc, what)


# ------------------------------------------------------------------------------------------- board conv (hrl_conv.hip)

CONV_M = [1, 15, 16, 17, 65, 16385]
_CONV = {}


def _conv_in(dev, M):
    if M not in _CONV:
        lib = _native.load()
        r = _gen(dev, 100 + M)
        c = types.SimpleNamespace(
            x=r(M, 288), ref=r(M, 288), dy=r(M, 288), y=r(M, 288), w=r(32, 32, 3, 3) * 0.1, bias=r(32),
            a=r(32).abs() + 0.5, b=r(32) * 0.3, em=r(32) * 0.1, ea=r(32).abs() + 0.5, eb=r(32) * 0.3,
            gamma=r(32).abs() + 0.5, beta=r(32) * 0.2, mean=r(32) * 0.1, invstd=r(32).abs() + 0.5,
            kcoef=r(32) * 0.1, gmean=r(32) * 0.1, w1p=r(2, 32), w1v=r(1, 32), dz=r(M, 28))
        c.dz[:, 27] = 0
        c.packed = torch.empty(1, 2, 9216, device=dev)
        _ok(lib.hrl_conv3x3_pack_n(_native.ptr_array([c.w]), 1, P(c.packed), _native.stream_of(dev)), 'pack')
        torch.cuda.synchronize(dev)
        _CONV[M] = c
    return _CONV[M]


def _conv_forward_ex(dev, M, epi, pro, packed):
    lib, c, stream = _native.load(), _conv_in(dev, M), _native.stream_of(dev)
    flip = (1 if epi >= 2 else 0) | (2 if packed else 0)      # epilogues 2 and 3 belong to the input gradient
    weight = c.packed[0, flip & 1] if packed else c.w
    bias = c.bias if epi == 0 else None
    a, b = (c.a, c.b) if pro else (None, None)

    def fn(al, short=0):
        y = al.out((M, 288), name='y')
        part = al.out((lib.hrl_conv3x3_stats_blocks(M), 32, 2), torch.float64, name='part') if epi in (1, 2) else None
        wsb = lib.hrl_conv3x3_workspace_bytes(M) - short
        ws = al.ws(wsb, name='workspace')
        _ok(lib.hrl_conv3x3_forward_ex(P(c.x), M, P(a), P(b), P(weight), P(bias), flip, P(y), epi,
                                       P(c.ref) if epi >= 2 else None, P(c.em), P(c.ea), P(c.eb), P(part), P(ws), wsb,
                                       stream), 'hrl_conv3x3_forward_ex')
        return {'y': y, 'part': part}
    return fn


@pytest.mark.parametrize('M', CONV_M)
@pytest.mark.parametrize('split', [1, 0], ids=['split', 'fp32'])
@pytest.mark.parametrize('packed', [True, False], ids=['packed', 'unpacked'])
@pytest.mark.parametrize('pro', [False, True], ids=['raw', 'prologue'])
@pytest.mark.parametrize('epi', [0, 1, 2, 3])
def test_hrl_conv3x3_forward_ex(cuda, epi, pro, packed, split, M):
    """kTile = 16 rows per wave, kWaves = 4 (64 rows per workgroup; the tile-shared and DMA-ring forms: 8 waves, one
    16-row tile per step), kGrid = 256: M = 1, 15, 16, 17, 65 and 256 x 64 + 1.  The statistics forward (epilogue 1,
    packed, split) runs every hrl_conv3x3_set_fwd_form value: 2 the DMA ring, 1 tile-shared, 0 per-wave."""
    forms = (2, 1, 0) if (epi == 1 and packed and split) else (None,)
    with _switch('hrl_conv3x3_set_split', split):
        for form in forms:
            with _switch('hrl_conv3x3_set_fwd_form', form):
                _ab(cuda, _conv_forward_ex(cuda, M, epi, pro, packed))


def _conv_wgrad_ex(dev, M, pro):
    lib, c, stream = _native.load(), _conv_in(dev, M), _native.stream_of(dev)
    a, b = (c.a, c.b) if pro else (None, None)

    def fn(al, short=0):
        dw = al.out((32, 32, 3, 3), name='dweight')
        wsb = lib.hrl_conv3x3_workspace_bytes(M) - short
        ws = al.ws(wsb, name='workspace')
        _ok(lib.hrl_conv3x3_wgrad_ex(P(c.x), P(a), P(b), P(c.dy), M, P(dw), P(ws), wsb, stream),
            'hrl_conv3x3_wgrad_ex')
        off = ctypes.c_int64(0)
        rows = lib.hrl_conv3x3_wgrad_partials(M, ctypes.byref(off))
        return {'dweight': dw, 'partial rows': ws[off.value:off.value + rows * 9216 * 4].view(torch.float32)}
    return fn


@pytest.mark.parametrize('M', CONV_M)
@pytest.mark.parametrize('split', [1, 0], ids=['split', 'fp32'])
@pytest.mark.parametrize('pro', [False, True], ids=['raw', 'prologue'])
def test_hrl_conv3x3_wgrad_ex(cuda, pro, split, M):
    """16-row tiles, 4 waves, 256 workgroups; one partial row of 9216 floats per workgroup behind the packed weights
    in the workspace, located by hrl_conv3x3_wgrad_partials."""
    with _switch('hrl_conv3x3_set_split', split):
        _ab(cuda, _conv_wgrad_ex(cuda, M, pro))


def _conv_block_backward(dev, M, epi, pro, defer, dz=False):
    """epi None: no input gradient.  defer: dweight NULL, the partial rows stay in the workspace."""
    lib, c, stream = _native.load(), _conv_in(dev, M), _native.stream_of(dev)
    a, b = (c.a, c.b) if pro else (None, None)

    def fn(al, short=0):
        dw = None if defer else al.out((32, 32, 3, 3), name='dweight')
        gin = None if epi is None else al.out((M, 288), name='gin')
        part = al.out((lib.hrl_conv3x3_block_sum_blocks(M), 32, 2), torch.float64, name='part') if epi == 2 else None
        wsb = lib.hrl_conv3x3_workspace_bytes(M) - short
        ws = al.ws(wsb, name='workspace')
        tail = (P(c.y), M, P(c.gamma), P(c.beta), P(c.mean), P(c.invstd), P(c.kcoef), P(c.gmean), P(c.x), P(a), P(b),
                P(c.packed[0, 1]), P(dw), P(gin), epi or 0, P(c.em), P(c.ea), P(c.eb), P(part), P(ws), wsb, stream)
        if dz:
            _ok(lib.hrl_conv3x3_block_backward_dz(P(c.dz), P(c.w1p), P(c.w1v), *tail), 'hrl_conv3x3_block_backward_dz')
        else:
            _ok(lib.hrl_conv3x3_block_backward(P(c.dy), *tail), 'hrl_conv3x3_block_backward')
        off = ctypes.c_int64(0)
        rows = lib.hrl_conv3x3_wgrad_partials(M, ctypes.byref(off))
        prow = ws[off.value:off.value + rows * 9216 * 4].view(torch.float32)
        return {'dweight': dw, 'gin': gin, 'part': part, 'partial rows': prow}
    return fn


@pytest.mark.parametrize('M', CONV_M)
@pytest.mark.parametrize('form', [1, 0], ids=['tile-shared', 'per-wave'])
@pytest.mark.parametrize('defer', [False, True], ids=['dweight', 'partials'])
@pytest.mark.parametrize('pro', [False, True], ids=['raw', 'prologue'])
@pytest.mark.parametrize('epi', [None, 0, 2, 3], ids=['nogin', 'epi0', 'epi2', 'epi3'])
def test_hrl_conv3x3_block_backward(cuda, epi, pro, defer, form, M):
    """16-row tiles; form 1: 8 waves share one tile per step, form 0 (and no input gradient): 4 waves x 16 rows;
    one workgroup per 64 rows up to 256.  part: hrl_conv3x3_block_sum_blocks(M) rows."""
    with _switch('hrl_conv3x3_set_block_form', form):
        _ab(cuda, _conv_block_backward(cuda, M, epi, pro, defer))


@pytest.mark.parametrize('M', CONV_M)
@pytest.mark.parametrize('defer', [False, True], ids=['dweight', 'partials'])
@pytest.mark.parametrize('pro', [False, True], ids=['raw', 'prologue'])
def test_hrl_conv3x3_block_backward_dz(cuda, pro, defer, M):
    """The tile-shared form with epilogue 2 only, dL/d out rebuilt from dz (M, 28): the same tiles as above."""
    with _switch('hrl_conv3x3_set_block_form', 1):
        _ab(cuda, _conv_block_backward(cuda, M, 2, pro, defer, dz=True))


@pytest.mark.parametrize('n', [1, 8])
def test_hrl_conv3x3_pack_n(cuda, n):
    """One thread per packed float, 256 per workgroup: n x 2 x 9216 floats (a multiple of 256)."""
    lib = _native.load()
    r = _gen(cuda, 7 + n)
    ws = [r(32, 32, 3, 3) for _ in range(n)]

    def fn(al):
        packed = al.out((n, 2, 9216), name='packed')
        _ok(lib.hrl_conv3x3_pack_n(_native.ptr_array(ws), n, P(packed), _native.stream_of(cuda)), 'hrl_conv3x3_pack_n')
        return {'packed': packed}
    _ab(cuda, fn)


def _colsum(dev, M, N):
    lib = _native.load()
    x = _gen(dev, M + N)(M, N)

    def fn(al, short=0):
        out = al.out((N,), name='out')
        wsb = lib.hrl_colsum_workspace_bytes(M, N) - short
        ws = al.ws(wsb, name='workspace')
        _ok(lib.hrl_colsum(P(x), M, N, P(out), P(ws), wsb, _native.stream_of(dev)), 'hrl_colsum')
        return {'out': out}
    return fn


@pytest.mark.parametrize('M,N', [(1, 1), (1, 256), (127, 9), (128, 32), (129, 256), (4099, 9), (131073, 3)])
def test_hrl_colsum(cuda, M, N):
    """128 rows per workgroup up to 1024 workgroups (then more rows each): M = 1, 127, 128, 129, 1024 x 128 + 1;
    N = 1 .. 256 columns."""
    _ab(cuda, _colsum(cuda, M, N))


# ------------------------------------------------------------------------------------------- BatchNorm (hrl_bn.hip)

# (N, C, H, W): 256 threads own fixed columns of the (N, C*HW) view, rp = 256 / ncol rows per pass (ncol = C*HW / 4
# float4 columns, or C*HW floats when C*HW % 4 != 0); above 256 columns kc = ceil(ncol / 256) slots per thread.
#   (1, 8, 3, 3)      N = 1
#   (17, 8, 3, 3)     ncol 18, rp 14: one workgroup, the second pass ragged (3 of 14 rows)
#   (4099, 8, 1, 1)   ncol 2, rp 128: 17 workgroups of 242 rows (1.9 passes), the last of 227
#   (10, 3, 3, 3)     27 scalar columns (no float4), rp 9: the second pass has 1 row
#   (5, 32, 7, 11)    616 float4 columns: kc = 3 slots, the third ragged (104 of 256)
BN_SHAPES = [(1, 8, 3, 3), (17, 8, 3, 3), (4099, 8, 1, 1), (10, 3, 3, 3), (5, 32, 7, 11)]
BN_G = 3
_BN = {}


def _bn_in(dev, shape):
    if shape not in _BN:
        N, C, H, W = shape
        r = _gen(dev, N + 31 * C + H)
        _BN[shape] = types.SimpleNamespace(
            x=r(*shape), dy=r(*shape), out=r(*shape), res=r(*shape), weight=r(C).abs() + 0.5, bias=r(C) * 0.3,
            mean=r(BN_G, C) * 0.1, invstd=r(BN_G, C).abs() + 0.5, kcoef=r(C) * 0.1, gmean=r(C) * 0.1,
            alpha=r(C).abs() + 0.5, beta=r(C) * 0.3, rm=r(C) * 0.1, rv=r(C).abs() + 0.5,
            part=r(N, C, 2).double().abs() * 3.0)
    return _BN[shape]


BN_ENTRIES = ['hrl_bn_forward_train', 'hrl_bn_backward', 'hrl_bn_forward_train_grouped', 'hrl_bn_backward_grouped',
              'hrl_bn_finalize_stats', 'hrl_bn_finalize_backward', 'hrl_bn_apply', 'hrl_bn_apply_residual',
              'hrl_bn_backward_apply', 'hrl_bn_forward_eval', 'hrl_bn_backward_masked', 'hrl_bn_backward_masked_coefs',
              'hrl_bn_backward_apply_masked']
BN_WITH_WS = ['hrl_bn_forward_train', 'hrl_bn_backward', 'hrl_bn_forward_train_grouped', 'hrl_bn_backward_grouped',
              'hrl_bn_backward_masked', 'hrl_bn_backward_masked_coefs']
BN_WITH_RELU = ['hrl_bn_forward_train', 'hrl_bn_backward', 'hrl_bn_forward_train_grouped', 'hrl_bn_backward_grouped',
                'hrl_bn_apply', 'hrl_bn_backward_apply', 'hrl_bn_forward_eval']


def _bn(dev, entry, shape, relu):
    lib, stream = _native.load(), _native.stream_of(dev)
    grouped = entry.endswith('_grouped')
    if grouped:     # three groups of the shape's N rows each
        shape = (shape[0] * BN_G,) + shape[1:]
    N, C, H, W = shape
    HW = H * W
    c = _bn_in(dev, shape)
    G = BN_G if grouped else 1
    mean, invstd = c.mean[:G].contiguous(), c.invstd[:G].contiguous()
    call = getattr(lib, entry)

    def fn(al, short=0):
        o = {}
        new = lambda name, *s: o.setdefault(name, al.out(s, name=name))   # noqa: E731
        wsb = ws = None
        if entry in BN_WITH_WS:
            wsb = (lib.hrl_bn_workspace_bytes_grouped(N, C, HW, G) if grouped else
                   lib.hrl_bn_workspace_bytes(N, C, HW)) - short
            ws = al.ws(wsb, name='workspace')
        if entry in ('hrl_bn_forward_train', 'hrl_bn_forward_train_grouped', 'hrl_bn_finalize_stats'):
            o['running_mean'], o['running_var'] = al.inout(c.rm, name='running_mean'), al.inout(c.rv, name='running_var')
        if entry == 'hrl_bn_forward_train':
            rc = call(P(c.x), N, C, HW, P(c.weight), P(c.bias), P(o['running_mean']), P(o['running_var']), MOM, EPS,
                      relu, P(new('y', *shape)), P(new('save_mean', C)), P(new('save_invstd', C)), P(ws), wsb, stream)
        elif entry == 'hrl_bn_forward_train_grouped':
            rc = call(P(c.x), N, C, HW, G, P(c.weight), P(c.bias), P(o['running_mean']), P(o['running_var']), MOM,
                      EPS, relu, P(new('y', *shape)), P(new('save_mean', G, C)), P(new('save_invstd', G, C)), P(ws),
                      wsb, stream)
        elif entry == 'hrl_bn_backward':
            rc = call(P(c.x), P(c.dy), N, C, HW, P(c.weight), P(c.bias), P(mean), P(invstd), relu,
                      P(new('dx', *shape)), P(new('dweight', C)), P(new('dbias', C)), P(ws), wsb, stream)
        elif entry == 'hrl_bn_backward_grouped':
            rc = call(P(c.x), P(c.dy), N, C, HW, G, P(c.weight), P(c.bias), P(mean), P(invstd), relu,
                      P(new('dx', *shape)), P(new('dweight', C)), P(new('dbias', C)), P(ws), wsb, stream)
        elif entry == 'hrl_bn_finalize_stats':      # N rows of per-block sums
            rc = call(P(c.part), N, C, N * HW, P(c.weight), P(c.bias), P(o['running_mean']), P(o['running_var']), MOM,
                      EPS, P(new('save_mean', C)), P(new('save_invstd', C)), P(new('alpha', C)), P(new('beta', C)),
                      stream)
        elif entry == 'hrl_bn_finalize_backward':
            rc = call(P(c.part), N, C, N * HW, P(c.weight), P(invstd), P(new('dweight', C)), P(new('dbias', C)),
                      P(new('kcoef', C)), P(new('gmean', C)), stream)
        elif entry == 'hrl_bn_apply':
            rc = call(P(c.x), N, C, HW, P(c.alpha), P(c.beta), relu, P(new('y', *shape)), stream)
        elif entry == 'hrl_bn_apply_residual':      # relu: with the residual input; else res NULL
            rc = call(P(c.x), P(c.res) if relu else None, N, C, HW, P(c.alpha), P(c.beta), P(new('y', *shape)), stream)
        elif entry == 'hrl_bn_backward_apply':
            rc = call(P(c.x), P(c.dy), N, C, HW, P(c.weight), P(c.bias), P(mean), P(invstd), relu, P(c.kcoef),
                      P(c.gmean), P(new('dx', *shape)), stream)
        elif entry == 'hrl_bn_forward_eval':
            rc = call(P(c.x), N, C, HW, P(c.weight), P(c.bias), P(c.rm), P(c.rv), EPS, relu, P(new('y', *shape)),
                      P(new('coef', 2 * C)), stream)
        elif entry == 'hrl_bn_backward_masked':
            rc = call(P(c.x), P(c.dy), P(c.out), N, C, HW, P(c.weight), P(mean), P(invstd), P(new('dx', *shape)),
                      P(new('dweight', C)), P(new('dbias', C)), P(ws), wsb, stream)
        elif entry == 'hrl_bn_backward_masked_coefs':
            rc = call(P(c.x), P(c.dy), P(c.out), N, C, HW, P(c.weight), P(mean), P(invstd), P(new('kcoef', C)),
                      P(new('gmean', C)), P(new('dweight', C)), P(new('dbias', C)), P(ws), wsb, stream)
        else:
            assert entry == 'hrl_bn_backward_apply_masked'
            rc = call(P(c.x), P(c.dy), P(c.out), N, C, HW, P(c.weight), P(mean), P(invstd), P(c.kcoef), P(c.gmean),
                      P(new('dx', *shape)), stream)
        _ok(rc, entry)
        return o
    return fn


# relu: the fused ReLU where the entry has one; hrl_bn_apply_residual: with the residual input (else res NULL)
BN_CASES = [(e, r) for e in BN_ENTRIES for r in ((0, 1) if e in BN_WITH_RELU + ['hrl_bn_apply_residual'] else (0,))]


@pytest.mark.parametrize('shape', BN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('entry,relu', BN_CASES, ids=['%s%s' % (e, '-relu' if r else '') for e, r in BN_CASES])
def test_bn(cuda, entry, relu, shape):
    """BN_SHAPES above; the _grouped entries run G = 3 groups of the shape's N rows each."""
    _ab(cuda, _bn(cuda, entry, shape, relu))


# ------------------------------------------------------------------------------------------- stem (hrl_stem.hip)

STEM_N = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 129]
_STEM = {}


def _stem_in(dev, N, cin):
    if (N, cin) not in _STEM:
        r = _gen(dev, 5 * N + cin)
        _STEM[(N, cin)] = types.SimpleNamespace(x=r(N, cin, 3, 3), w=r(32, cin, 3, 3), b=r(32), dy=r(N, 288))
    return _STEM[(N, cin)]


def _stem_forward(dev, N, cin, bias):
    lib, c = _native.load(), _stem_in(dev, N, cin)

    def fn(al):
        y = al.out((N, 32, 3, 3), name='y')
        _ok(lib.hrl_stem_forward(P(c.x), N, cin, P(c.w), P(c.b) if bias else None, P(y), _native.stream_of(dev)),
            'hrl_stem_forward')
        return {'y': y}
    return fn


@pytest.mark.parametrize('N', STEM_N)
@pytest.mark.parametrize('form', [2, 1], ids=['lane-per-channel', 'mfma'])
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('cin', [1, 3])
def test_hrl_stem_forward(cuda, cin, bias, form, N):
    """Form 2: kOct = 8-row octets, 4 waves (32 rows per workgroup): N = 1, 7, 8, 9, 33.  Form 1: 16-row tiles, 4 waves
    (64 rows): 15, 16, 17 and, with 31, 32, 129, the workgroup edges of both."""
    with _switch('hrl_stem_set_fwd_form', form):
        _ab(cuda, _stem_forward(cuda, N, cin, bias))


def _stem_wgrad(dev, N, cin, mode):
    """mode: 'both' dweight and dbias, 'nobias' dweight only, 'partials' both NULL (form 2 only)."""
    lib, c = _native.load(), _stem_in(dev, N, cin)

    def fn(al, short=0):
        dw = al.out((32, cin, 3, 3), name='dweight') if mode != 'partials' else None
        db = al.out((32,), name='dbias') if mode == 'both' else None
        wsb = lib.hrl_stem_workspace_bytes(N) - short
        ws = al.ws(wsb, name='workspace')
        _ok(lib.hrl_stem_wgrad(P(c.x), P(c.dy), N, cin, P(dw), P(db), P(ws), wsb, _native.stream_of(dev)),
            'hrl_stem_wgrad')
        rows = None
        if mode == 'partials':      # [dW (32, Cin, 3, 3) | db (32)] at the start of each row
            row = ctypes.c_int64(0)
            n = lib.hrl_stem_wgrad_partials(N, ctypes.byref(row))
            rows = ws[:n * row.value * 4].view(torch.float32).view(n, row.value)[:, :32 * cin * 9 + 32].contiguous()
        return {'dweight': dw, 'dbias': db, 'partial rows': rows}
    return fn


@pytest.mark.parametrize('N', STEM_N)
@pytest.mark.parametrize('form,mode', [(2, 'both'), (2, 'nobias'), (2, 'partials'), (1, 'both'), (1, 'nobias')])
@pytest.mark.parametrize('cin', [1, 3])
def test_hrl_stem_wgrad(cuda, cin, form, mode, N):
    """Form 2: 32-row blocks, 4 waves (128 rows per workgroup); form 1: 16-row tiles, 4 waves.  The partial rows are
    located by hrl_stem_wgrad_partials (the deferred mode needs form 2)."""
    with _switch('hrl_stem_set_wgrad_form', form):
        _ab(cuda, _stem_wgrad(cuda, N, cin, mode))


# ------------------------------------------------------------------------------------------- heads (hrl_heads.hip)

HEADS_N = [1, 31, 32, 33, 63, 64, 65, 129]
_HEADS = {}


def _heads_in(dev, N):
    if N not in _HEADS:
        r = _gen(dev, 9 * N)
        _HEADS[N] = types.SimpleNamespace(
            h=r(N, 288), w1p=r(2, 32), b1p=r(2), w1v=r(1, 32), b1v=r(1), wp=r(9, 18), wv=r(1, 9),
            al=r(32).abs() + 0.5, be=r(32) * 0.3, mu=r(32) * 0.1, a_p=r(N, 18), a_v=r(N, 9), dp=r(N, 9), dv=r(N, 1),
            vt=torch.tanh(r(N, 1)))
    return _HEADS[N]


def _heads_forward(dev, N, bn, acts):
    lib, c = _native.load(), _heads_in(dev, N)

    def fn(al):
        a_p = al.out((N, 18), name='a_p') if acts else None
        a_v = al.out((N, 9), name='a_v') if acts else None
        p, v = al.out((N, 9), name='p'), al.out((N, 1), name='v')
        _ok(lib.hrl_heads_forward(P(c.h), N, P(c.w1p), P(c.b1p), P(c.w1v), P(c.b1v), P(c.wp), P(c.wv),
                                  P(c.al) if bn else None, P(c.be) if bn else None, P(a_p), P(a_v), P(p), P(v),
                                  1 if acts else 0, _native.stream_of(dev)), 'hrl_heads_forward')
        return {'a_p': a_p, 'a_v': a_v, 'p': p, 'v': v}
    return fn


@pytest.mark.parametrize('N', HEADS_N)
@pytest.mark.parametrize('acts', [True, False], ids=['acts+tanh', 'inference'])
@pytest.mark.parametrize('bn', [True, False], ids=['bn', 'nobn'])
def test_hrl_heads_forward(cuda, bn, acts, N):
    """One-wave workgroups over 64-row blocks: N = 1, 63, 64, 65, 129 (and the backward's 31, 32, 33); with and
    without the BatchNorm input coefficients, with and without the saved activations (the latter with tanh_v = 1)."""
    _ab(cuda, _heads_forward(cuda, N, bn, acts))


def _heads_backward(dev, N, bn, vt, defer, dz=False):
    """bn: 0 none, 1 the BatchNorm prologue only, 2 also its backward sums (bn_part)."""
    lib, c, stream = _native.load(), _heads_in(dev, N), _native.stream_of(dev)

    def fn(al, short=0):
        nparts = lib.hrl_heads_bn_parts(N)
        part = al.out((nparts, 32, 2), torch.float64, name='bn_part') if bn == 2 else None
        dh = al.out((N, 28 if dz else 288), name='dz' if dz else 'dh')
        names = ('dw1p', 'db1p', 'dw1v', 'db1v', 'dwp', 'dwv')
        shapes = ((2, 32), (2,), (1, 32), (1,), (9, 18), (1, 9))
        grads = [None] * 6 if defer else [al.out(s, name=n) for n, s in zip(names, shapes)]
        wsb = lib.hrl_heads_workspace_bytes(N) - short
        ws = al.ws(wsb, name='workspace')
        entry = lib.hrl_heads_backward_dz if dz else lib.hrl_heads_backward
        _ok(entry(P(c.h), N, P(c.w1p), P(c.w1v), P(c.wp), P(c.wv), P(c.al) if bn else None, P(c.be) if bn else None,
                  P(c.mu) if bn else None, P(part), P(c.a_p), P(c.a_v), P(c.dp), P(c.dv), P(c.vt) if vt else None,
                  P(dh), *[P(g) for g in grads], P(ws), wsb, stream),
            'hrl_heads_backward_dz' if dz else 'hrl_heads_backward')
        o = dict(zip(names, grads), bn_part=part)
        o['dz' if dz else 'dh'] = dh
        if defer:       # hrl_heads_bn_parts(N) rows of 270 floats at the start of the workspace
            o['partial rows'] = ws[:nparts * 270 * 4].view(torch.float32)
        return o
    return fn


HEADS_BWD = [(0, False, False), (1, True, False), (2, True, False), (2, False, True), (0, True, True)]
HEADS_BWD_IDS = ['plain', 'bn-tanh', 'bnpart-tanh', 'bnpart-partials', 'tanh-partials']
# the deferred mode (partial rows) under form 1 is HRL_EINVAL by contract (test_heads_dz_gpu.py): no case
HEADS_BWD_FORMS = [(v, f) for v in zip(HEADS_BWD, HEADS_BWD_IDS) for f in (2, 1) if not (v[0][2] and f == 1)]


@pytest.mark.parametrize('N', HEADS_N)
@pytest.mark.parametrize('bn,vt,defer,form', [v[0] + (f,) for v, f in HEADS_BWD_FORMS],
                         ids=['%s-form%d' % (v[1], f) for v, f in HEADS_BWD_FORMS])
def test_hrl_heads_backward(cuda, bn, vt, defer, form, N):
    """Form 2: kBR = 32-row blocks, 4 waves (128 rows per workgroup), rows stored in groups of 8; form 1: one-wave
    workgroups over 64-row blocks.  N = 1, 31, 32, 33, 63, 64, 65, 129.  The deferred mode needs form 2."""
    with _switch('hrl_heads_set_bwd_form', form):
        _ab(cuda, _heads_backward(cuda, N, bn, vt, defer))


@pytest.mark.parametrize('N', HEADS_N)
@pytest.mark.parametrize('bn,vt,defer', HEADS_BWD, ids=HEADS_BWD_IDS)
def test_hrl_heads_backward_dz(cuda, bn, vt, defer, N):
    """Form 2 only; dz rows are 28 floats (112 B), the payload exactly N x 112 bytes."""
    with _switch('hrl_heads_set_bwd_form', 2):
        _ab(cuda, _heads_backward(cuda, N, bn, vt, defer, dz=True))


# ------------------------------------------------------------------------------------------- torus (hrl_torus.hip)

# one sample per wave, 4 waves per workgroup (the pre-split form: 8 waves, two such blocks), grid 512 (the weight
# gradients: 256): N = 1, 3, 4, 5 and 512 x 4 + 1 on the 7 x 11 board; a 3 x 3 board (one ragged 16-cell tile; 17
# channels x 9 cells is no multiple of 4: the scalar paths) and an 8 x 10 board (all 5 cell tiles full) at N = 5.
TORUS = [(1, 7, 11), (3, 7, 11), (4, 7, 11), (5, 7, 11), (2049, 7, 11), (5, 3, 3), (5, 8, 10)]
TORUS_IDS = ['%dx%dx%d' % t for t in TORUS]
_TORUS = {}


def _torus_in(dev, N, H, W):
    key = (N, H, W)
    if key not in _TORUS:
        r = _gen(dev, N + 3 * H + W)
        _TORUS[key] = types.SimpleNamespace(
            x17=r(N, 17, H, W), x32=r(N, 32, H, W), y=r(N, 32, H, W), g=r(N, 32, H, W), out=r(N, 32, H, W),
            hm=r(N, 32, H, W), add17=r(N, 17, H, W), mask17=r(N, 17, H, W), w17=r(32, 17, 3, 3) * 0.1,
            w32=r(32, 32, 3, 3) * 0.1, bias=r(32), alpha=r(32).abs() + 0.5, beta=r(32) * 0.3, gamma=r(32).abs() + 0.5,
            mean=r(32) * 0.1, invstd=r(32).abs() + 0.5, kcoef=r(32) * 0.1, gmean=r(32) * 0.1, dhead=r(N, 32),
            davg=r(N, 32))
    return _TORUS[key]


def _torus(dev, entry, variant, N, H, W):
    lib, c, stream = _native.load(), _torus_in(dev, N, H, W), _native.stream_of(dev)
    cin = 17 if '17' in variant else 32
    x, w = (c.x17, c.w17) if cin == 17 else (c.x32, c.w32)

    def fn(al, short=0):
        o = {}
        new = lambda name, *s: o.setdefault(name, al.out(s, name=name))   # noqa: E731
        stats = lambda: o.setdefault('part', al.out((lib.hrl_torus_stats_blocks(N), 32, 2), torch.float64,   # noqa: E731
                                                    name='part'))
        wsb = ws = None
        if entry not in ('hrl_torus_head_pool', 'hrl_torus_head_unpool'):
            wsb = lib.hrl_torus_workspace_bytes(N) - short
            ws = al.ws(wsb, name='workspace')
        if entry == 'hrl_torus_conv_forward':
            if 'flip' in variant:       # the input gradient: (N, 32, H, W) -> (N, Cin, H, W), with or without add
                add, mask = ((c.add17, c.mask17) if cin == 17 else (c.g, c.out)) if 'add' in variant else (None, None)
                rc = lib.hrl_torus_conv_forward(P(c.y), N, cin, 32, H, W, P(w), None, 1, P(new('y', N, cin, H, W)),
                                                None, P(add), P(mask), P(ws), wsb, stream)
            else:
                rc = lib.hrl_torus_conv_forward(P(x), N, cin, 32, H, W, P(w), P(c.bias) if 'bias' in variant else None,
                                                0, P(new('y', N, 32, H, W)), P(stats()) if 'part' in variant else None,
                                                None, None, P(ws), wsb, stream)
        elif entry == 'hrl_torus_unit_forward':
            rc = lib.hrl_torus_unit_forward(P(c.y), P(c.x32) if 'res' in variant else None, P(c.alpha), P(c.beta),
                                            P(new('h', N, 32, H, W)), N, H, W, P(c.w32), P(c.bias),
                                            P(new('y', N, 32, H, W)), P(stats()), P(ws), wsb, stream)
        elif entry == 'hrl_torus_unit_input_grad':
            rc = lib.hrl_torus_unit_input_grad(P(c.y), N, H, W, P(c.w32), P(c.g), P(c.out), P(new('dh', N, 32, H, W)),
                                               P(c.hm), P(c.x32), P(c.mean), P(stats()), P(ws), wsb, stream)
        elif entry == 'hrl_torus_conv_wgrad':
            rc = lib.hrl_torus_conv_wgrad(P(x), P(c.g), N, cin, 32, H, W, P(new('dweight', 32, cin, 3, 3)),
                                          P(new('dbias', 32)) if 'bias' in variant else None, P(ws), wsb, stream)
        elif entry == 'hrl_torus_conv_wgrad_bn':
            rc = lib.hrl_torus_conv_wgrad_bn(P(x), N, cin, H, W, P(c.y), P(c.g), P(c.alpha), P(c.beta),
                                             1 if 'res' in variant else 0, P(c.gamma) if 'gamma' in variant else None,
                                             P(c.mean), P(c.invstd), P(c.kcoef), P(c.gmean),
                                             P(new('dy', N, 32, H, W)), P(new('dweight', 32, cin, 3, 3)),
                                             P(new('dbias', 32)) if 'bias' in variant else None, P(ws), wsb, stream)
        elif entry == 'hrl_torus_head_pool':
            rc = lib.hrl_torus_head_pool(P(c.x32), P(c.x17), N, H, W, 17 * H * W, P(new('head', N, 32)),
                                         P(new('avg', N, 32)), stream)
        else:
            assert entry == 'hrl_torus_head_unpool'
            rc = lib.hrl_torus_head_unpool(P(c.dhead), P(c.davg), P(c.x17), N, H, W, 17 * H * W,
                                           P(new('g', N, 32, H, W)), stream)
        _ok(rc, entry)
        return o
    return fn


TORUS_CASES = [('hrl_torus_conv_forward', v) for v in ('17-bias', '17-bias-part', '32-bias-part', '32', '17-flip',
                                                       '17-flip-add', '32-flip', '32-flip-add')] + \
              [('hrl_torus_unit_forward', 'res'), ('hrl_torus_unit_forward', 'first'),
               ('hrl_torus_unit_input_grad', '32')]


@pytest.mark.parametrize('N,H,W', TORUS, ids=TORUS_IDS)
@pytest.mark.parametrize('split,form', [(1, 2), (1, 1), (0, 2)], ids=['presplit', 'pertap', 'fp32'])
@pytest.mark.parametrize('entry,variant', TORUS_CASES, ids=['%s-%s' % t for t in TORUS_CASES])
def test_torus_conv(cuda, entry, variant, split, form, N, H, W):
    """The forward / input-gradient kernel under hrl_torus_set_split x hrl_torus_set_form (the form only matters with
    the split on).  conv_forward: 17 and 32 input channels, with and without bias, statistics (part) and, as the
    input gradient (flip), with and without the masked add; unit_forward: with the residual prologue and without."""
    with _switch('hrl_torus_set_split', split), _switch('hrl_torus_set_form', form):
        _ab(cuda, _torus(cuda, entry, variant, N, H, W))


# hrl_torus_conv_wgrad_bn is split arithmetic only (HRL_EINVAL otherwise, by contract)
TORUS_WGRAD = [('hrl_torus_conv_wgrad', v, s) for v in ('17-bias', '32-bias', '32') for s in (1, 0)] + \
              [('hrl_torus_conv_wgrad_bn', v, 1) for v in ('17-gamma-bias', '32-res-gamma-bias', '32')]


@pytest.mark.parametrize('N,H,W', TORUS, ids=TORUS_IDS)
@pytest.mark.parametrize('entry,variant,split', TORUS_WGRAD,
                         ids=['%s-%s-%s' % (e, v, 'split' if s else 'fp32') for e, v, s in TORUS_WGRAD])
def test_torus_wgrad(cuda, entry, variant, split, N, H, W):
    """One sample per wave, 4 waves, grid 256 (2049 = two passes + 1); one partial row of 9248 floats per workgroup
    behind the packed weights.  hrl_torus_conv_wgrad_bn also writes dy (N, 32, H, W)."""
    with _switch('hrl_torus_set_split', split):
        _ab(cuda, _torus(cuda, entry, variant, N, H, W))


@pytest.mark.parametrize('N,H,W', TORUS, ids=TORUS_IDS)
@pytest.mark.parametrize('entry', ['hrl_torus_head_pool', 'hrl_torus_head_unpool'])
def test_torus_head(cuda, entry, N, H, W):
    """One sample per wave, 4 waves per workgroup, up to 2048 workgroups; the net input's plane 0 is read with a
    17-channel sample stride."""
    _ab(cuda, _torus(cuda, entry, '', N, H, W))


def _board_conv_pack(dev, cout, total=64, ci0=32):
    lib = _native.load()
    w = _gen(dev, cout)(cout, total, 3, 3) * 0.1

    def fn(al, short=0):
        nbytes = lib.hrl_board_conv_workspace_bytes(cout)
        packed = al.out((nbytes // 4,), name='packed')
        _ok(lib.hrl_board_conv_pack(P(w), total, ci0, cout, P(packed), nbytes - short, _native.stream_of(dev)),
            'hrl_board_conv_pack')
        return {'packed': packed}
    return fn


@pytest.mark.parametrize('cout', [32, 64])
def test_hrl_board_conv_pack(cuda, cout):
    """One thread per packed float: Cout / 32 chunks of 9 x 8 x 2 x 64 floats, the whole buffer."""
    _ab(cuda, _board_conv_pack(cuda, cout))


@pytest.mark.parametrize('N', [1, 3, 4, 5, 2049])
@pytest.mark.parametrize('split', [1, 0], ids=['split', 'fp32'])
@pytest.mark.parametrize('H,W', [(3, 3), (4, 4)], ids=['3x3', '4x4'])
@pytest.mark.parametrize('cout', [32, 64])
def test_hrl_board_conv_forward_packed(cuda, cout, H, W, split, N):
    """One sample per wave, 4 waves, 512 / (Cout / 32) workgroups per 32-channel chunk: 2049 is one row more than a
    full pass for Cout 32 and two passes + 1 for Cout 64.  3 x 3 and 4 x 4: one ragged / one full 16-cell tile."""
    lib = _native.load()
    r = _gen(cuda, N + cout + H)
    x, bias = r(N, 32, H, W), r(cout)
    packed = Plain(cuda).out((lib.hrl_board_conv_workspace_bytes(cout) // 4,))
    w = r(cout, 32, 3, 3) * 0.1
    _ok(lib.hrl_board_conv_pack(P(w), 32, 0, cout, P(packed), packed.numel() * 4, _native.stream_of(cuda)), 'pack')

    def fn(al):
        y = al.out((N, cout, H, W), name='y')
        _ok(lib.hrl_board_conv_forward_packed(P(x), N, 32, H, W, P(packed), cout, P(bias), P(y),
                                              _native.stream_of(cuda)), 'hrl_board_conv_forward_packed')
        return {'y': y}
    with _switch('hrl_torus_set_split', split):
        _ab(cuda, fn)


# ------------------------------------------------------------------------------------------- workspace_bytes - 1

SHORT = {
    'hrl_conv3x3_forward_ex': lambda d: _conv_forward_ex(d, 65, 2, True, True),
    'hrl_conv3x3_wgrad_ex': lambda d: _conv_wgrad_ex(d, 65, True),
    'hrl_conv3x3_block_backward': lambda d: _conv_block_backward(d, 65, 2, True, False),
    'hrl_conv3x3_block_backward_dz': lambda d: _conv_block_backward(d, 65, 2, True, False, dz=True),
    'hrl_colsum': lambda d: _colsum(d, 129, 256),
    'hrl_stem_wgrad': lambda d: _stem_wgrad(d, 33, 3, 'both'),
    'hrl_heads_backward': lambda d: _heads_backward(d, 65, 2, True, False),
    'hrl_heads_backward_dz': lambda d: _heads_backward(d, 65, 2, True, False, dz=True),
    'hrl_torus_conv_forward': lambda d: _torus(d, 'hrl_torus_conv_forward', '17-bias-part', 5, 7, 11),
    'hrl_torus_unit_forward': lambda d: _torus(d, 'hrl_torus_unit_forward', 'res', 5, 7, 11),
    'hrl_torus_unit_input_grad': lambda d: _torus(d, 'hrl_torus_unit_input_grad', '32', 5, 7, 11),
    'hrl_torus_conv_wgrad': lambda d: _torus(d, 'hrl_torus_conv_wgrad', '32-bias', 5, 7, 11),
    'hrl_torus_conv_wgrad_bn': lambda d: _torus(d, 'hrl_torus_conv_wgrad_bn', '32-res-gamma-bias', 5, 7, 11),
    'hrl_board_conv_pack': lambda d: _board_conv_pack(d, 64),
}
SHORT.update({e: (lambda d, e=e: _bn(d, e, (17, 8, 3, 3), 1 if e in BN_WITH_RELU else 0)) for e in BN_WITH_WS})


@pytest.mark.parametrize('entry', sorted(SHORT))
def test_workspace_one_byte_short(cuda, entry):
    """Every entry point that takes workspace_bytes (hrl_board_conv_pack: packed_bytes), one byte below what its size
    function returns: HRL_EINVAL, and every payload, workspace and guard still holds its prefill."""
    _short(cuda, SHORT[entry](cuda))
