"""Every launch form of csrc/hrl_gboard.hip's board convolution against the fp64 convolution, at a few games.

``gboard_conv_kernel<KC, PADC, NCTW, R>`` has 24 forms (KC k-steps of 32 input channels, PADC a ragged channel count,
NCTW column tiles per workgroup -- 4 / NCTW output-cell bands per tile --, R the staging ring: 3 quads, or the whole
k-step's 9 for KC == 1 with one task per workgroup).  The launcher picks NCTW and R from the task count against its
256 workgroups, so at the sizes the value tests use (at most 96 tasks) only NCTW = 1 and, for KC == 1, only R = 9 ever
run.  Here ``hrl_gboard_set_nctw`` and ``hrl_gboard_set_whole_ring`` force each form at N = 17 games (two tiles, the
second with one game) and ``hrl_gboard_launch_stats`` proves the forced form is the one that ran: the setter silently
ignores a value that does not divide the column tiles, which would otherwise run NCTW = 1 again.

The reference is ``F.conv2d(x.double(), w.double(), padding=1, groups=g)`` on the CPU and the epilogue in fp64 in the
kernel's order (+ bias, * alpha + beta, relu).
  * integer data (x, w in [-8, 8], bias and beta in [-4, 4], alpha in {1, 2, 3}): at most 128 x 9 products of at
    most 64, every sum below 2^24, the bf16 three-way split of such integers exact -> ``torch.equal``;
  * random data: ``_close`` of tests/test_gboard_gpu.py, 4e-6 of max |ref|.  No other tolerance appears.

Forms that ran against fp64 (asserted from the launch counters), all 24:
    KC 1 (Cin_g 32; PADC: 25)    NCTW 1, 2, 4  x  R 9 (whole k-step) and R 3
    KC 2 (Cin_g 64; PADC: 48)    NCTW 1, 2, 4  x  R 3
    KC 4 (Cin_g 128; PADC: 100)  NCTW 1, 2, 4  x  R 3
and, with more tasks than workgroups (R 3, a workgroup walks two tasks), KC 1 at NCTW 1, 2, 4.
"""

import contextlib
import ctypes

import pytest
import torch
import torch.nn.functional as F

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from tests.test_gboard_gpu import _close

pytestmark = pytest.mark.gpu

P = _native.ptr
N_STATS = 11
NAN = float('nan')


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


@contextlib.contextmanager
def _gpu_errors_end_the_session():
    """A HIP error leaves the process's GPU context unusable: end the session, nothing more is launched."""
    try:
        yield
    except RuntimeError as e:
        if 'HIP' in str(e) or 'hip' in str(e) or 'failed (' in str(e):
            pytest.exit('GPU error, nothing more is launched: %s' % e, returncode=3)
        raise


def _stats(reset=0):
    arr = (ctypes.c_int64 * N_STATS)()
    assert _native.load().hrl_gboard_launch_stats(ctypes.cast(arr, ctypes.c_void_p), N_STATS, reset) == N_STATS
    return list(arr)


def _assert_form(st, nctw, whole, what=''):
    """One conv launch, with exactly the expected one of the NCTW counters and the expected whole-ring counter."""
    assert st[0] == 1, (what, st)
    assert st[2:5] == [int(nctw == 1), int(nctw == 2), int(nctw == 4)], (what, nctw, st)
    assert st[1] == int(whole), (what, whole, st)


@contextlib.contextmanager
def _forced(nctw, whole_ring, expect_whole, what=''):
    """Force a launch form for the block's one conv launch; afterwards assert from the counters that it ran."""
    with _gpu_errors_end_the_session(), _switch('hrl_gboard_set_nctw', nctw), \
            _switch('hrl_gboard_set_whole_ring', whole_ring):
        _stats(reset=1)
        yield
        st = _stats()
        torch.cuda.synchronize()
    _assert_form(st, nctw, expect_whole, what)


def _pack(w, cin_g=None, ci0=0):
    lib = _native.load()
    cout, total = w.shape[0], w.shape[1]
    cin_g = total - ci0 if cin_g is None else cin_g
    nbytes = lib.hrl_gboard_pack_bytes(cout, cin_g)
    assert nbytes > 0
    pk = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    with _gpu_errors_end_the_session():
        _native.check(lib.hrl_gboard_pack(P(w), cout, cin_g, total, ci0, P(pk), nbytes, _native.stream_of(w.device)),
                      'hrl_gboard_pack')
    return pk


def _forward(x, pk, cout, cin_g, groups=1, x2=None, bias=None, alpha=None, beta=None, relu=False):
    """hrl_gboard_forward into a NaN-filled y (an element the kernel skips fails every comparison)."""
    N = x.shape[0]
    y = torch.full((N, cout, 6, 6), NAN, device=x.device)
    _native.check(_native.load().hrl_gboard_forward(
        P(x), x.stride(0), P(x2), 0 if x2 is None else x2.stride(0), N, cin_g, groups, P(pk), pk.numel(), cout,
        P(bias), P(alpha), P(beta), int(relu), P(y), y.stride(0), _native.stream_of(x.device)), 'hrl_gboard_forward')
    return y


def _ref(x, w, groups=1, bias=None, alpha=None, beta=None, relu=False):
    y = F.conv2d(x.double(), w.double(), padding=1, groups=groups)
    if bias is not None:
        y = y + bias.double()[None, :, None, None]
    if alpha is not None:
        y = y * alpha.double()[None, :, None, None] + beta.double()[None, :, None, None]
    if relu:
        y = y.clamp_min(0)
    return y


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


class _Case:
    """The inputs of one (N, Cin, Cout, groups) shape on the CPU and the device, integer or random, with the fp64
    references of the bare conv and of the full epilogue: computed once, shared, never modified."""

    def __init__(self, dev, N, cin_g, cout, groups, integer):
        g = torch.Generator().manual_seed(1000 * N + 10 * cin_g + cout + groups + int(integer))
        if integer:
            self.x, self.w = _ints(g, -8, 8, N, cin_g * groups, 6, 6), _ints(g, -8, 8, cout, cin_g, 3, 3)
            self.bias, self.beta, self.alpha = _ints(g, -4, 4, cout), _ints(g, -4, 4, cout), _ints(g, 1, 3, cout)
        else:
            self.x = torch.randn(N, cin_g * groups, 6, 6, generator=g)
            self.w = torch.randn(cout, cin_g, 3, 3, generator=g) * 0.2
            self.bias, self.beta = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
            self.alpha = torch.rand(cout, generator=g) + 0.5
        self.N, self.cin_g, self.cout, self.groups = N, cin_g, cout, groups
        self.ref = {False: _ref(self.x, self.w, groups),
                    True: _ref(self.x, self.w, groups, self.bias, self.alpha, self.beta, True)}
        self.dx, self.dbias, self.dalpha, self.dbeta = (t.to(dev) for t in (self.x, self.bias, self.alpha, self.beta))
        self.pk = _pack(self.w.to(dev))

    def run(self, epilogue):
        if epilogue:
            return _forward(self.dx, self.pk, self.cout, self.cin_g, self.groups, bias=self.dbias, alpha=self.dalpha,
                            beta=self.dbeta, relu=True)
        return _forward(self.dx, self.pk, self.cout, self.cin_g, self.groups)


_CASES = {}


def _case(dev, N, cin_g, cout=64, groups=1, integer=True):
    key = (N, cin_g, cout, groups, integer)
    if key not in _CASES:
        _CASES[key] = _Case(dev, *key)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------- the form matrix

# (Cin_g, NCTW, whole_ring): KC 1, 2, 4 each without and with PADC (100: the 97..128 window), every NCTW; for KC == 1
# both rings (whole_ring 1 -> R = 9, 0 -> R = 3), for KC > 1 only R = 3 exists (the switch stays at its default)
FORMS = [(cin, nctw, wr) for cin in (32, 25, 64, 48, 128, 100) for nctw in (1, 2, 4)
         for wr in ((1, 0) if cin <= 32 else (None,))]


def _form_id(f):
    cin, nctw, wr = f
    return 'cin%d-nctw%d-%s' % (cin, nctw, 'R9' if wr == 1 else 'R3')


@pytest.mark.parametrize('cin,nctw,whole_ring', FORMS, ids=[_form_id(f) for f in FORMS])
def test_gboard_form_matches_fp64(cuda, cin, nctw, whole_ring):
    """Cout = 64 (4 column tiles: every NCTW divides them), N = 17: two tiles, the second holding one game (the
    min(.., N - 1) clamp of the staging rows).  Integer data with the full epilogue and with none: exactly the fp64
    result; random data with the full epilogue: within 4e-6 of max |ref|."""
    whole = whole_ring == 1      # 2 tiles x (4 / NCTW) tasks <= 256: the whole-ring form whenever KC == 1 allows it
    for integer, epilogue in ((True, True), (True, False), (False, True)):
        c = _case(cuda, 17, cin, integer=integer)
        what = '%s data, %s' % ('integer' if integer else 'random', 'full epilogue' if epilogue else 'no epilogue')
        with _forced(nctw, whole_ring, whole, what):
            y = c.run(epilogue)
        y = y.cpu().double()
        if integer:
            assert torch.equal(y, c.ref[epilogue]), what
        else:
            assert _close(y, c.ref[epilogue]), what


# one form per NCTW at the other game counts: a lone game, a tile less one, exactly one tile
EDGE_FORMS = [(25, 1, 1), (64, 2, None), (32, 4, 0)]


@pytest.mark.parametrize('N', [1, 15, 16])
@pytest.mark.parametrize('cin,nctw,whole_ring', EDGE_FORMS, ids=[_form_id(f) for f in EDGE_FORMS])
def test_gboard_form_game_count_edges(cuda, cin, nctw, whole_ring, N):
    for epilogue in (True, False):
        c = _case(cuda, N, cin)
        with _forced(nctw, whole_ring, whole_ring == 1):
            y = c.run(epilogue)
        assert torch.equal(y.cpu().double(), c.ref[epilogue]), epilogue


@pytest.mark.parametrize('nctw,N', [(1, 170), (2, 341), (4, 675)])
def test_gboard_workgroups_walk_several_tasks(cuda, nctw, N):
    """Cout = 384 (24 column tiles), Cin_g = 32, integer data, a ragged last tile: 11 tiles x 24 = 264, 22 x 12 = 264
    and 43 x 6 = 258 tasks over 256 workgroups, so some workgroups do two tasks (the ring restarts between them, the
    accumulators are cleared) and the rest one; more than 256 tasks also turns the whole-ring form off although the
    switch is on.  The CPU fp64 reference of the largest case (N = 675) was measured at 0.06 s (the whole case, data and
both references included, at 0.16 s), so it stays on the CPU."""
    tiles = (N + 15) // 16
    assert tiles * (24 // nctw) > 256 and N % 16
    c = _case(cuda, N, 32, cout=384)
    for epilogue in (True, False):
        with _forced(nctw, 1, False):
            y = c.run(epilogue)
        assert torch.equal(y.cpu().double(), c.ref[epilogue]), epilogue


# ------------------------------------------------------------------------------- groups and sources under forced forms

@pytest.mark.parametrize('whole_ring', [1, 0], ids=['R9', 'R3'])
@pytest.mark.parametrize('nctw', [1, 2, 4])
def test_gboard_grouped_h_halves_from_a_channel_slice(cuda, nctw, whole_ring):
    """Cout = 384 in 3 groups of Cin_g = 32 (8 column tiles per group: every NCTW keeps a workgroup inside one group),
    x channels 16..111 of a 128-channel tensor (game stride 128 x 36), N = 33 (three tiles, the last with one game)."""
    g = torch.Generator().manual_seed(41)
    N = 33
    wide = _ints(g, -8, 8, N, 128, 6, 6)
    w = _ints(g, -8, 8, 384, 32, 3, 3)
    ref = _ref(wide[:, 16:112], w, 3)
    dwide = wide.to(cuda)
    pk = _pack(w.to(cuda))
    with _forced(nctw, whole_ring, whole_ring == 1):
        y = _forward(dwide[:, 16:112], pk, 384, 32, 3)
    assert torch.equal(y.cpu().double(), ref)


@pytest.mark.parametrize('nctw', [1, 2, 4])
def test_gboard_forward_groups_own_pointers(cuda, nctw):
    """hrl_gboard_forward_groups: each of the 3 groups reads its own tensor (slices of differently wide tensors, so
    three game strides) == the grouped fp64 conv of the stacked inputs, exactly on integer data; counter 6 counts."""
    lib = _native.load()
    g = torch.Generator().manual_seed(43)
    N, H, L = 33, 32, 3
    wides = [_ints(g, -8, 8, N, H + 8 * i, 6, 6) for i in range(L)]
    hs = [wd[:, 4 * i:4 * i + H] for i, wd in enumerate(wides)]
    w = _ints(g, -8, 8, 4 * H * L, H, 3, 3)
    ref = _ref(torch.cat(hs, 1), w, L)
    dh = [wd.to(cuda)[:, 4 * i:4 * i + H] for i, wd in enumerate(wides)]
    pk = _pack(w.to(cuda))
    y = torch.full((N, 4 * H * L, 6, 6), NAN, device=cuda)
    with _forced(nctw, None, True):
        _native.check(lib.hrl_gboard_forward_groups(
            _native.ptr_array(dh), _native.i64_array([h.stride(0) for h in dh]), N, H, L, P(pk), pk.numel(),
            4 * H * L, P(y), y.stride(0), _native.stream_of(cuda)), 'hrl_gboard_forward_groups')
        assert _stats()[6] == 1
    assert torch.equal(y.cpu().double(), ref)


@pytest.mark.parametrize('nctw', [1, 2, 4])
def test_gboard_adjoint_split_under_forced_forms(cuda, nctw):
    """nn.gboard_adjoint_split with cout_fwd = 128: one grouped launch of S = 4 groups of 32 outputs each (counter 5),
    two column tiles per group, so the launcher accepts NCTW 1 and 2 and ignores a forced 4 (it then runs its own
    choice, which the counters must show).  Exactly the fp64 input gradient on integer data, 4e-6 on random data."""
    N, cout_fwd, ci0, cin = 37, 128, 32, 32
    for integer in (True, False):
        g = torch.Generator().manual_seed(47 + int(integer))
        mk = (lambda *s: _ints(g, -8, 8, *s)) if integer else (lambda *s: torch.randn(*s, generator=g))
        w, dy = mk(cout_fwd, ci0 + cin + 3, 3, 3), mk(N, cout_fwd, 6, 6)
        x = torch.zeros(N, cin, 6, 6, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w[:, ci0:ci0 + cin].double(), padding=1).backward(dy.double())
        ref = x.grad
        rec = hnn.DeferredGrads()
        with _gpu_errors_end_the_session(), _switch('hrl_gboard_set_nctw', nctw):
            _stats(reset=1)
            y = hnn.gboard_adjoint_split(dy.to(cuda), w.to(cuda), ci0, cin, rec)
            st = _stats()
            torch.cuda.synchronize()
        assert st[0] == 1 and st[5] == 1, st
        if nctw == 4:       # not accepted: the launcher's own choice runs (below 257 tasks that is NCTW = 1)
            assert st[2:5] == [1, 0, 0] and st[1] == 1, st
        else:
            _assert_form(st, nctw, True)
        y = y.cpu().double()
        if integer:
            assert torch.equal(y, ref)
        else:
            assert _close(y, ref)


@pytest.mark.parametrize('cout,nctw', [(64, 1), (64, 2), (64, 4), (8, 1)])
def test_gboard_two_sources(cuda, cout, nctw):
    """Cin_g = 64 from two sources (x: channels 0..31, x2: channels 32..63, a channel slice of a 96-channel tensor)
    with Cout = 64 at every NCTW and the net's own Cout = 8 (one partial column tile); two k-steps, so R = 3."""
    g = torch.Generator().manual_seed(53 + cout)
    N = 33
    he, st = _ints(g, -8, 8, N, 32, 6, 6), _ints(g, -8, 8, N, 96, 6, 6)
    w, bias = _ints(g, -8, 8, cout, 64, 3, 3), _ints(g, -4, 4, cout)
    ref = _ref(torch.cat([he, st[:, 64:96]], 1), w, 1, bias)
    dst = st.to(cuda)
    pk = _pack(w.to(cuda))
    with _forced(nctw, None, False):
        y = _forward(he.to(cuda), pk, cout, 64, x2=dst[:, 64:96], bias=bias.to(cuda))
    assert torch.equal(y.cpu().double(), ref)


# ------------------------------------------------------------------------------------------------------- rejections

def test_gboard_forward_rejections(cuda):
    """Each returns HRL_EINVAL (the size function: -1) before any launch and leaves a sentinel-filled y unchanged."""
    lib = _native.load()
    stream = _native.stream_of(cuda)
    N, cout = 5, 64
    sentinel = -12345.0
    x = torch.zeros(N, 128, 6, 6, device=cuda)
    pk = torch.zeros(lib.hrl_gboard_pack_bytes(cout, 128), dtype=torch.uint8, device=cuda)
    al = torch.ones(cout, device=cuda)
    ybuf = torch.full((N * cout * 36 + 4,), sentinel, device=cuda)
    y = ybuf[:N * cout * 36]

    def rejected(what, cin_g=32, groups=1, cout=cout, x_stride=128 * 36, packed_bytes=None, alpha=None, beta=None,
                 yp=y):
        nbytes = lib.hrl_gboard_pack_bytes(cout, cin_g) if packed_bytes is None else packed_bytes
        lib.hrl_gboard_launch_stats(None, 0, 1)
        rc = lib.hrl_gboard_forward(P(x), x_stride, None, 0, N, cin_g, groups, P(pk), nbytes, cout, None, P(alpha),
                                    P(beta), 0, P(yp), cout * 36, stream)
        assert rc == _native.HRL_EINVAL, (what, rc)
        assert _stats()[0] == 0, what
        torch.cuda.synchronize()
        assert bool((ybuf == sentinel).all()), what

    for cin_g in (65, 80, 96):
        assert lib.hrl_gboard_pack_bytes(cout, cin_g) == -1
        rejected('Cin_g %d' % cin_g, cin_g=cin_g, packed_bytes=pk.numel())
    assert lib.hrl_gboard_pack_bytes(cout, 64) > 0 and lib.hrl_gboard_pack_bytes(cout, 97) > 0
    rejected('packed_bytes one byte short', packed_bytes=lib.hrl_gboard_pack_bytes(cout, 32) - 1)
    rejected('x_stride % 4', x_stride=128 * 36 - 2)
    rejected('misaligned y', yp=ybuf[1:])
    rejected('alpha without beta', alpha=al)
    rejected('beta without alpha', beta=al)
    rejected('cout_g % 16', cout=40, groups=2)
    # the same call with nothing wrong is accepted (the rejections above are not an artefact of the harness here)
    rc = lib.hrl_gboard_forward(P(x), 128 * 36, None, 0, N, 32, 1, P(pk), pk.numel(), cout, None, None, None, 0, P(y),
                                cout * 36, stream)
    with _gpu_errors_end_the_session():
        _native.check(rc, 'hrl_gboard_forward')
        torch.cuda.synchronize()
    assert bool((y == 0).all()) and bool((ybuf[-4:] == sentinel).all())
