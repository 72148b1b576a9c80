"""hrl_board_infer / hrl_board_infer_pack on the GPU (csrc/hrl_infer.hip, nn.BoardInference).

* exactness on integer data (board_infer_util.integer_net: every intermediate exact in fp32, so the fp32 and fp64
  torch forwards agree exactly -- test_board_infer_abi.py checks that on the CPU): the policy equals the reference bit
  for bit, the value is within 1e-6 of tanh of the exact pre-activation (16 fp32 ulps at 1);
* seeded nets with BatchNorm statistics off their initial values against the fp64 torch-CPU forward at abs 1e-5, the
  project's tolerance for policies and values;
* ragged row counts around the kernel's 16-row tile, which is also its workgroup's rows: 1, 15, 16, 17 and 1003;
* guard bands, sessions (in-place refresh, graph replay), groups.
"""

import functools

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn

from . import board_infer_util as util
from .guarded import Arena, bits

pytestmark = pytest.mark.gpu

TILE = 16                                   # rows per tile = rows per workgroup
SIZES = (1, TILE - 1, TILE, TILE + 1, 1003)
CASES = [(L, n) for L in (1, 3) for n in SIZES] + [(8, TILE + 1)]
INPUTS = {'planes': util.planes, 'floats': util.floats, 'quarters': util.quarters}


@functools.lru_cache(maxsize=None)
def _net(kind, L):
    return util.integer_net(L) if kind == 'int' else util.seeded_net(L)


@functools.lru_cache(maxsize=None)
def _reference(kind, L, inp, n):
    """(policy, value, value pre-activation) of the fp64 CPU forward; computed once per case."""
    net, x = _net(kind, L), INPUTS[inp](n)
    p, v = util.forward64(net, x)
    return p, v, util.value_preact64(net, x)


@functools.lru_cache(maxsize=None)
def _wrapped(kind, L):
    import copy
    return hnn.BoardInference(copy.deepcopy(_net(kind, L)).to('cuda:0').eval())


def _run(kind, L, inp, n):
    w = _wrapped(kind, L)
    x = INPUTS[inp](n).to('cuda:0')
    with torch.no_grad(), w.inference_session():
        out = w(x, None)
    assert out['policy'].shape == (n, 9) and out['value'].shape == (n, 1)
    return out['policy'].cpu(), out['value'].cpu()


@pytest.mark.parametrize('inp', ['planes', 'quarters'])
@pytest.mark.parametrize('L,n', CASES)
def test_integer_exact(cuda, L, n, inp):
    p64, _, pre = _reference('int', L, inp, n)
    policy, value = _run('int', L, inp, n)
    assert torch.equal(policy.double(), p64)
    err = (value.double() - torch.tanh(pre)).abs().max().item()
    print('L=%d n=%d %s: value err %.3g' % (L, n, inp, err))
    assert err <= 1e-6


@pytest.mark.parametrize('inp', ['planes', 'floats'])
@pytest.mark.parametrize('L,n', CASES)
def test_against_fp64(cuda, L, n, inp):
    p64, v64, _ = _reference('seeded', L, inp, n)
    policy, value = _run('seeded', L, inp, n)
    ep = (policy.double() - p64).abs().max().item()
    ev = (value.double() - v64).abs().max().item()
    print('L=%d n=%d %s: policy err %.3g value err %.3g' % (L, n, inp, ep, ev))
    assert ep <= 1e-5 and ev <= 1e-5


def _direct(arena, w, pack, x, span):
    n = x.shape[0]
    policy = arena.out((n, 9), name='policy')
    value = arena.out((n, 1), name='value')
    _native.check(_native.load().hrl_board_infer(
        _native.ptr(pack), pack.numel() * pack.element_size(), len(span) - 1, _native.i64_array(span),
        _native.ptr(x), n, w.layers, _native.ptr(policy), _native.ptr(value), _native.stream_of(x.device)),
        'hrl_board_infer')
    return policy, value


@pytest.mark.parametrize('n', [1, TILE + 1, 1003])
def test_guard_bands(cuda, n):
    w = _wrapped('seeded', 3)
    nbytes = _native.load().hrl_board_infer_pack_bytes(3)
    arena = Arena(cuda)
    pack = arena.out(nbytes // 4, torch.int32, name='pack')      # exactly pack_bytes, every word to be written
    x = arena.inout(util.floats(n), name='obs')
    with torch.no_grad():
        w._refresh(cuda, out=pack)
    policy, value = _direct(arena, w, pack, x, [0, n])
    arena.check()                                                # guards intact, outputs and pack fully written
    assert torch.equal(bits(x.cpu()), bits(util.floats(n)))      # the observations are unchanged
    p64, v64, _ = _reference('seeded', 3, 'floats', n)
    assert (policy.cpu().double() - p64).abs().max() <= 1e-5
    assert (value.cpu().double() - v64).abs().max() <= 1e-5


def test_zero_rows_launch_nothing(cuda):
    w = _wrapped('seeded', 3)
    arena = Arena(cuda)
    pack = arena.out(_native.load().hrl_board_infer_pack_bytes(3) // 4, torch.int32, name='pack')
    x = arena.inout(util.floats(4), name='obs')
    policy = arena.out((4, 9), name='policy')
    value = arena.out((4, 1), name='value')
    lib = _native.load()
    for K, span in ((1, [0, 0]), (3, [0, 0, 0, 0])):
        assert lib.hrl_board_infer(_native.ptr(pack), pack.numel() * 4, K, _native.i64_array(span), _native.ptr(x), 0,
                                   3, _native.ptr(policy), _native.ptr(value), _native.stream_of(cuda)) == 0
    arena.check_untouched()
    with torch.no_grad(), w.inference_session():
        out = w(torch.zeros(0, 3, 3, 3, device=cuda))
    assert out['policy'].shape == (0, 9) and out['value'].shape == (0, 1)


def test_sessions_refresh_in_place(cuda):
    import copy
    net = copy.deepcopy(util.seeded_net(3)).to(cuda).eval()
    w = hnn.BoardInference(net)
    x = util.floats(40).to(cuda)
    with pytest.raises(RuntimeError):
        w(x)                                                     # the GPU outside a session
    with torch.no_grad():
        with w.inference_session():
            ptr = w.pack().data_ptr()
            a = w(x)['policy'].clone()
            net.head_p.fc.weight.mul_(2.0)                       # in place, inside the session: not seen yet
            net.blocks[0].bn.running_mean.add_(0.05)
            b = w(x)['policy'].clone()
        assert torch.equal(a, b)
        with w.inference_session():
            c = w(x)
            assert w.pack().data_ptr() == ptr
        assert not torch.equal(a, c['policy'])
        p64, v64 = util.forward64(net, x)
        assert (c['policy'].cpu().double() - p64).abs().max() <= 1e-5
        assert (c['value'].cpu().double() - v64).abs().max() <= 1e-5


def test_graph_replays_with_a_later_sessions_weights(cuda):
    import copy
    net = copy.deepcopy(util.seeded_net(3)).to(cuda).eval()
    w = hnn.BoardInference(net)
    x = util.floats(40).to(cuda)
    with torch.no_grad():
        with w.inference_session():
            side = torch.cuda.Stream(cuda)
            side.wait_stream(torch.cuda.current_stream(cuda))
            with torch.cuda.stream(side):
                w(x)
            torch.cuda.current_stream(cuda).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = w(x)
            g.replay()
            first = out['policy'].clone()
        net.conv.weight.mul_(0.5)
        net.blocks[2].bn.weight.add_(0.25)
        with w.inference_session():
            g.replay()
            second = {k: v.clone() for k, v in out.items()}
            eager = w(x)
        assert not torch.equal(first, second['policy'])
        assert torch.equal(second['policy'], eager['policy']) and torch.equal(second['value'], eager['value'])
        p64, v64 = util.forward64(net, x)
        assert (second['policy'].cpu().double() - p64).abs().max() <= 1e-5
        assert (second['value'].cpu().double() - v64).abs().max() <= 1e-5


@pytest.mark.parametrize('span', [[0, 5, 5, 40], [0, 16, 33, 64]])
def test_grouped_equals_single(cuda, span):
    import contextlib
    import copy
    nets = [copy.deepcopy(util.seeded_net(3, seed=s)).to(cuda).eval() for s in range(3)]
    group = hnn.board_inference_group(nets)
    singles = [hnn.BoardInference(n) for n in nets]
    x = util.floats(span[-1]).to(cuda)
    with torch.no_grad(), contextlib.ExitStack() as stack:
        for m in list(group) + singles:
            stack.enter_context(m.inference_session())
        buf = group.buffer()
        assert all(m.pack().data_ptr() == buf[k].data_ptr() for k, m in enumerate(group))
        out = group.forward(x, span)
        assert out['policy'].shape == (span[-1], 9) and out['value'].shape == (span[-1], 1)
        for k in range(3):
            rows = x[span[k]:span[k + 1]]
            for one in (singles[k](rows), group[k](rows)):       # a separate wrapper, and the member used alone
                assert torch.equal(bits(out['policy'][span[k]:span[k + 1]]), bits(one['policy']))
                assert torch.equal(bits(out['value'][span[k]:span[k + 1]]), bits(one['value']))
    for k in range(3):
        p64, v64 = util.forward64(nets[k], x[span[k]:span[k + 1]])
        if p64.numel():
            assert (out['policy'][span[k]:span[k + 1]].cpu().double() - p64).abs().max() <= 1e-5
            assert (out['value'][span[k]:span[k + 1]].cpu().double() - v64).abs().max() <= 1e-5
