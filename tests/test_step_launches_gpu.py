"""Launches folded into their neighbours in the learner step, each against the launch it replaces (torch.equal):

* hrl_conv3x3_pack_n_zero: the weight packing plus a zero of a 4-byte aligned float region (the flat gradient
  buffer) -- region zero, its NaN guards untouched, the packed weights equal to hrl_conv3x3_pack_n's;
* hrl_grad_fold_norm_ex: loss_reduce_kernel's fold of the fused loss's partials by one more workgroup of the step
  tail's first launch -- the loss vector equal to hrl_loss_forward's, the gradient folds and norm_part equal to
  hrl_grad_fold_norm's;
* three LearnerStep updates of the TicTacToe net with the three switches (train.RAW_LOSS, nn.LOSS_FOLD,
  nn.PACK_ZERO) all on and each alone against all off, eager and graph-captured, the flat gradient buffer filled
  with NaN before every step so a missed zero shows;
* the fallbacks: the data-parallel step (no fold deferral) and a net without a conv chain (the plain zero).
"""

import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')


# ---- hrl_conv3x3_pack_n_zero

@pytest.mark.parametrize('count', [0, 1, 3, 4, 5, 1023, 30001])
@pytest.mark.parametrize('offset', [0, 1])
def test_pack_n_zero(cuda, count, offset):
    """Regions that are empty, shorter than the head, head only, one vector with and without ragged ends, several
    vectors in one workgroup and 30 workgroups; starting on a 16-byte boundary and 4 bytes past one."""
    from handyrl_amd import _native
    lib = _native.load()
    P = _native.ptr
    stream = _native.stream_of(cuda)
    g0 = torch.Generator(device=cuda).manual_seed(count + offset)
    weights = [torch.randn(32, 32, 3, 3, device=cuda, generator=g0) for _ in range(3)]
    ref = torch.empty(3, 2, 9216, device=cuda)
    _native.check(lib.hrl_conv3x3_pack_n(_native.ptr_array(weights), 3, P(ref), stream), 'pack_n')
    guard = 64
    buf = torch.full((guard + offset + count + guard,), NAN, device=cuda)
    assert buf.data_ptr() % 16 == 0
    region = buf[guard + offset:guard + offset + count]
    assert count == 0 or region.data_ptr() % 16 == 4 * offset
    packed = torch.full((3, 2, 9216), NAN, device=cuda)
    _native.check(lib.hrl_conv3x3_pack_n_zero(_native.ptr_array(weights), 3, P(packed), P(region), count, stream),
                  'pack_n_zero')
    torch.cuda.synchronize(cuda)
    assert torch.equal(packed, ref)
    assert bool((region == 0).all())
    assert bool(torch.isnan(buf[:guard + offset]).all()) and bool(torch.isnan(buf[guard + offset + count:]).all())


def test_pack_n_zero_argument_checks(cuda):
    from handyrl_amd import _native
    lib = _native.load()
    P = _native.ptr
    w = [torch.zeros(32, 32, 3, 3, device=cuda)]
    packed = torch.full((1, 2, 9216), 5.0, device=cuda)
    z = torch.full((16,), 5.0, device=cuda)
    E = _native.HRL_EINVAL
    st = _native.stream_of(cuda)
    assert lib.hrl_conv3x3_pack_n_zero(_native.ptr_array(w), 1, P(packed), None, 4, st) == E
    assert lib.hrl_conv3x3_pack_n_zero(_native.ptr_array(w), 1, P(packed), P(z), -1, st) == E
    assert lib.hrl_conv3x3_pack_n_zero(_native.ptr_array(w), 1, P(packed), ctypes.c_void_p(z.data_ptr() + 2), 4,
                                       st) == E
    assert lib.hrl_conv3x3_pack_n_zero(_native.ptr_array(w), 0, P(packed), P(z), 4, st) == E
    assert lib.hrl_conv3x3_pack_n_zero(_native.ptr_array(w), 9, P(packed), P(z), 4, st) == E
    assert lib.hrl_conv3x3_pack_n_zero(_native.ptr_array(w), 1, None, P(z), 4, st) == E
    torch.cuda.synchronize(cuda)
    assert bool((packed == 5.0).all()) and bool((z == 5.0).all())


# ---- hrl_grad_fold_norm_ex

def _loss_call(lib, cuda, batch, B, T, ex, ws, losses):
    from handyrl_amd import _native
    P = _native.ptr
    head = (P(batch['tpol']), P(batch['policy']), P(batch['action']), B, T, 2, 1, 9, P(batch['episode_mask']),
            P(batch['turn_mask']), P(batch['observation_mask']), P(batch['progress']), P(batch['value']),
            P(batch['outcome']), None, None, None, 3, 2, 1, 0.7, 0.8, 0.1, 0.1, P(ws), ws.numel(), P(losses))
    st = _native.stream_of(cuda)
    if ex:
        return lib.hrl_loss_forward_ex(*head, None, None, None, 0, 0, st)
    return lib.hrl_loss_forward(*head, st)


@pytest.mark.parametrize('B,nparts', [(1, 1), (255, 255), (256, 256), (257, 257), (4096, 2048)])
def test_grad_fold_norm_ex_folds_the_loss_partials(cuda, B, nparts):
    """One partial, one short of / exactly / one past the 256 fold threads, and 8 per thread.  The loss partials come
    from the fused kernel itself (reduce = 0); the same launch folds gradient partials as hrl_grad_fold_norm does."""
    from handyrl_amd import _native
    from handyrl_amd.synthetic import tictactoe_batch
    lib = _native.load()
    P = _native.ptr
    T = 2
    batch = tictactoe_batch(B, T, cuda, seed=B)
    g0 = torch.Generator(device=cuda).manual_seed(B)
    batch['tpol'] = torch.randn(B, T, 1, 9, device=cuda, generator=g0) - batch['action_mask']
    ws_bytes = lib.hrl_loss_workspace_bytes(B, T, 2, 1)
    off = ctypes.c_int64(0)
    assert lib.hrl_loss_partials(B, T, 2, 1, ctypes.byref(off)) == nparts
    assert off.value % 16 == 0 and off.value + nparts * 48 <= ws_bytes
    ws0 = torch.zeros(ws_bytes, dtype=torch.uint8, device=cuda)
    ws1 = torch.zeros(ws_bytes, dtype=torch.uint8, device=cuda)
    ref = torch.full((6,), NAN, device=cuda)
    got = torch.full((6,), NAN, device=cuda)
    _native.check(_loss_call(lib, cuda, batch, B, T, False, ws0, ref), 'hrl_loss_forward')
    _native.check(_loss_call(lib, cuda, batch, B, T, True, ws1, got), 'hrl_loss_forward_ex')
    torch.cuda.synchronize(cuda)
    assert bool(torch.isnan(got).all()), 'reduce = 0 wrote the loss vector'
    part = ws1[off.value:off.value + nparts * 48].view(torch.float64)
    assert torch.equal(part, ws0[off.value:off.value + nparts * 48].view(torch.float64))

    n = 9216 + 300 + 41
    flat0 = torch.randn(n, device=cuda, generator=g0)
    flat1 = flat0.clone()
    p1 = torch.randn(130, 9216, device=cuda, generator=g0)
    p0 = torch.randn(300, 270, device=cuda, generator=g0)
    folds = [(p1, 9216, 0, 130, 0, 9216, 1), (p0, 270, 99, 300, 9216 + 10, 162, 0)]
    nb = lib.hrl_grad_fold_norm_blocks(n)
    i64 = _native.i64_array
    outs = []
    for flat, ex in ((flat0, False), (flat1, True)):
        step = torch.zeros((), device=cuda)
        ctr = [torch.zeros((), dtype=torch.int64, device=cuda) for _ in range(2)]
        norm_part = torch.full((nb,), NAN, dtype=torch.float64, device=cuda)
        head = (P(flat), n, _native.ptr_array([f[0] for f in folds]), i64([f[1] for f in folds]),
                i64([f[2] for f in folds]), i64([f[3] for f in folds]), i64([f[4] for f in folds]),
                i64([f[5] for f in folds]), (ctypes.c_int * 2)(*[f[6] for f in folds]), 2, P(step),
                _native.ptr_array(ctr), i64([1, 5]), 2, P(norm_part), nb * 8)
        if ex:
            _native.check(lib.hrl_grad_fold_norm_ex(*head, P(part), nparts, 0.1, P(got), _native.stream_of(cuda)),
                          'hrl_grad_fold_norm_ex')
        else:
            _native.check(lib.hrl_grad_fold_norm(*head, _native.stream_of(cuda)), 'hrl_grad_fold_norm')
        torch.cuda.synchronize(cuda)
        outs.append((flat, norm_part, step, ctr[0], ctr[1]))
    assert torch.equal(got, ref) and bool(torch.isfinite(ref).all())
    for a, b in zip(outs[1], outs[0]):
        assert torch.equal(a, b)
    # argument checks: partials without a count, a loss vector or 8-byte alignment
    E = _native.HRL_EINVAL
    st = _native.stream_of(cuda)
    assert lib.hrl_grad_fold_norm_ex(*head, P(part), 0, 0.1, P(got), st) == E
    assert lib.hrl_grad_fold_norm_ex(*head, P(part), nparts, 0.1, None, st) == E
    assert lib.hrl_grad_fold_norm_ex(*head, ctypes.c_void_p(part.data_ptr() + 4), nparts, 0.1, P(got), st) == E


# ---- the learner step

@contextlib.contextmanager
def _switches(raw, fold, zero):
    from handyrl_amd import nn as hnn, train
    prev = (train.RAW_LOSS, hnn.LOSS_FOLD, hnn.PACK_ZERO)
    train.RAW_LOSS, hnn.LOSS_FOLD, hnn.PACK_ZERO = raw, fold, zero
    try:
        yield
    finally:
        train.RAW_LOSS, hnn.LOSS_FOLD, hnn.PACK_ZERO = prev


def _three_steps(cuda, make_net, switches, graph=False, **kw):
    """Three updates from identical state; everything the step leaves behind, as clones."""
    from handyrl_amd.synthetic import tictactoe_batch, default_args
    from handyrl_amd.trainer import LearnerStep
    B, T = 64, 8
    args = default_args(T, B)
    batch = tictactoe_batch(B, T, cuda, seed=21)
    torch.manual_seed(5)
    net = make_net()
    res = {}
    with _switches(*switches):
        step = LearnerStep(net, args, cuda, graph=graph, **kw)
        for i in range(3):
            step.grads.flat.fill_(NAN)
            out = step.step(batch)
            torch.cuda.synchronize()
            for k, v in out.items():
                res['out%d.%s' % (i, k)] = v.detach().clone()
            for n, p in step.net.named_parameters():
                res['grad%d.%s' % (i, n)] = p.grad.detach().clone()
        sums, cnt = step.pop_stats()
    assert cnt == 3
    res.update(('stat.' + k, torch.tensor(v)) for k, v in sums.items())
    res.update(('param.' + n, p.detach().clone()) for n, p in step.net.named_parameters())
    res.update(('buffer.' + n, b.detach().clone()) for n, b in step.net.named_buffers())
    if step.tail is not None:
        res.update(('adam.%d' % i, t.detach().clone()) for i, t in enumerate(step.tail.state_tensors()))
    assert all(bool(torch.isfinite(v.float()).all()) for v in res.values())
    return res


def _assert_same(got, ref):
    assert set(got) == set(ref) and len(ref) > 20
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


def _tictactoe_net():
    from handyrl_amd.envs.tictactoe import SimpleConv2dModel
    return SimpleConv2dModel()


_PARENT = {}


def _parent(cuda, graph):
    """The parent path (all three switches off), computed once per mode and left unchanged."""
    if graph not in _PARENT:
        _PARENT[graph] = _three_steps(cuda, _tictactoe_net, (False, False, False), graph)
    return _PARENT[graph]


@pytest.mark.parametrize('graph', [False, True])
@pytest.mark.parametrize('switches', [(True, True, True), (True, False, False), (False, True, False),
                                      (False, False, True)])
def test_learner_step_equal_to_the_parent_path(cuda, switches, graph):
    ref = _parent(cuda, graph)
    for k in ('out0.p', 'out0.v', 'out0.ent', 'out0.total', 'out0.dcnt', 'out0.grad_norm', 'stat.total',
              'adam.0', 'adam.1', 'adam.2'):
        assert k in ref, k
    _assert_same(_three_steps(cuda, _tictactoe_net, switches, graph), ref)


class _IdentityWork:
    def wait(self):
        return True


def test_data_parallel_step_takes_the_fallbacks(cuda, monkeypatch):
    """world_size forced to 2 builds the data-parallel step: a reducer and no fold deferral, so the loss launches
    its own reduce.  The SUM all-reduce of a one-rank communicator is the identity, which is what stands in for it
    here (no process group, no second process)."""
    from handyrl_amd import distributed as hdist
    monkeypatch.setattr(hdist.dist, 'all_reduce', lambda t, **kw: _IdentityWork())
    kw = dict(world_size=2, lr=3e-8 * 64 * 8)
    ref = _three_steps(cuda, _tictactoe_net, (False, False, False), **kw)
    got = _three_steps(cuda, _tictactoe_net, (True, True, True), **kw)
    _assert_same(got, ref)


class _Mlp(torch.nn.Module):
    """A net without a conv chain: nobody takes the posted zero, LearnerStep zeroes the buffer itself."""

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(27, 32)
        self.head_p = torch.nn.Linear(32, 9)
        self.head_v = torch.nn.Linear(32, 1)

    def forward(self, x, hidden=None):
        h = torch.relu(self.fc(x.flatten(1)))
        return {'policy': self.head_p(h), 'value': torch.tanh(self.head_v(h))}


@pytest.mark.parametrize('graph', [False, True])
def test_net_without_a_conv_chain_takes_the_plain_zero(cuda, graph):
    from handyrl_amd import nn as hnn
    ref = _three_steps(cuda, _Mlp, (False, False, False), graph)
    got = _three_steps(cuda, _Mlp, (True, True, True), graph)
    _assert_same(got, ref)
    assert hnn._PENDING_ZERO is None
