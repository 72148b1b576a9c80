"""The bf16 one-launch GeeseNet forward on the GPU (csrc/hrl_geesenet_bf16.hip), at the C entry with guard-band
outputs (tests/guarded.py) and through nn.GeeseInference(precision='bf16').

Contract (include/hrl_nn.h): conv weights and conv inputs rounded to bf16, fp32 everywhere else.  On integer data
of magnitude <= 256 the rounding is the identity, so the forward must equal the fp64 one; on a random net it must be
as close to fp64 as a plain torch emulation of the contract (twice its error + 1e-6, the margin the tower's test gives
the tower against the module path).  Measured on an MI355X: see DESIGN 4.26.

One pass is P = 512 workgroups x 8 waves = 4096 samples; the batch sizes are the wave count +- 1 and the pass +- 1."""

import copy

import pytest
import torch
import torch.nn.functional as F

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.hungry_geese import GeeseNet
from tests.guarded import Arena
from tests.test_geesenet_infer_gpu import forward64, observations, on_gpu, random_stats, same_bits, seeded

pytestmark = pytest.mark.gpu

P = 4096
SIZES = (1, 7, 8, 9, P - 1, P, P + 1, 2 * P + 1)


def c_forward(w, x):
    """hrl_geesenet_infer_bf16 on ``x`` with guarded outputs."""
    arena = Arena(x.device)
    N, _, H, W = x.shape
    policy, value = arena.out((N, 4), name='policy'), arena.out((N, 1), name='value')
    code = _native.load().hrl_geesenet_infer_bf16(_native.ptr(w.pack(x.device)), w.layers, _native.ptr(x), N, H, W,
                                                  _native.ptr(policy), _native.ptr(value), _native.stream_of(x.device))
    assert code == _native.HRL_OK, code
    arena.check()
    return policy.clone(), value.clone()


def wrapper(net, cuda):
    return hnn.GeeseInference(on_gpu(net, cuda), precision='bf16')


def emulate(net, x):
    """The contract in plain torch on the CPU: bf16-rounded weights and conv inputs, fp32 elsewhere."""
    r = lambda t: t.bfloat16().float()
    h = None
    with torch.no_grad():
        for i, u in enumerate([net.conv0, *net.blocks]):
            al = (1.0 / torch.sqrt(u.bn.running_var.double() + u.bn.eps)).float() * u.bn.weight
            be = u.bn.bias - u.bn.running_mean * al
            acc = F.conv2d(u.wrap(r(x if i == 0 else h)), r(u.conv.weight))
            v = (acc + u.conv.bias.view(1, -1, 1, 1)) * al.view(1, -1, 1, 1) + be.view(1, -1, 1, 1)
            h = torch.relu(v if i == 0 else h + v)
        h_head, h_avg = (h * x[:, :1]).flatten(2).sum(-1), h.flatten(2).mean(-1)
        return net.head_p(h_head), torch.tanh(net.head_v(torch.cat([h_head, h_avg], 1)))


def err(got, ref):
    return float((got.cpu().double() - ref).abs().max())


def as_good_as_the_emulation(net, x, p, v):
    """Kernel and emulation against fp64: the kernel's error at most twice the emulation's + 1e-6."""
    p64, v64 = forward64(net, x)
    pe, ve = emulate(net, x.cpu())
    ep_k, ev_k, ep_e, ev_e = err(p, p64), err(v, v64), err(pe, p64), err(ve, v64)
    print('max |error| against fp64: policy kernel %.3e emulation %.3e; value kernel %.3e emulation %.3e '
          '(policy range %.2f)' % (ep_k, ep_e, ev_k, ev_e, float(p64.abs().max())))
    assert ep_e > 0 and ev_e > 0                                # bf16 rounding is visible: not a vacuous bound
    assert ep_k <= 2 * ep_e + 1e-6 and ev_k <= 2 * ev_e + 1e-6, (ep_k, ep_e, ev_k, ev_e)


# ------------------------------------------------------------------------------------------------ integers
def integer_net(layers, seed):
    """Conv weights in {-1, 0, 1}, integer biases and heads, BatchNorm with var + eps = 1 exactly: alpha a power of
    two (1 or 2 in the stem, 1 in the blocks: the residual sums must stay within 256) and beta an integer.  (torch refuses eps = 0, so eps = 2^-10 and var = 1 - 2^-10, both exact in fp32; their
    sum is 1 in the kernel's double and in the fp64 reference alike.)"""
    g = torch.Generator().manual_seed(seed)
    net = GeeseNet(layers=layers).eval()
    ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float()
    with torch.no_grad():
        for u in [net.conv0, *net.blocks]:
            keep = torch.rand(u.conv.weight.shape, generator=g) < (0.3 if u is net.conv0 else 0.02)
            u.conv.weight.copy_(ri(u.conv.weight.shape, 0, 1).mul(2).sub(1) * keep)
            u.conv.bias.copy_(ri((32,), -1, 1) * 2)
            u.bn.eps = 2.0 ** -10
            u.bn.running_var.fill_(1.0 - 2.0 ** -10)
            u.bn.running_mean.copy_(ri((32,), -1, 1) * 2)
            u.bn.weight.copy_(2.0 ** ri((32,), 0, 1)) if u is net.conv0 else u.bn.weight.fill_(1.0)
            u.bn.bias.copy_(ri((32,), -2, 2))
        net.head_p.weight.copy_(ri((4, 32), -2, 2))
        net.head_v.weight.copy_(ri((1, 64), -1, 1))
    return net


@pytest.mark.parametrize('layers', [1, 2])
@pytest.mark.parametrize('H,W', [(7, 11), (4, 5), (8, 10), (1, 3)])
def test_integer_data_is_exact(cuda, H, W, layers):
    net = integer_net(layers, seed=30 + layers)
    g = torch.Generator().manual_seed(H * W)
    x = (torch.rand(9, 17, H, W, generator=g) < 0.2).float()
    n64, h, peak = copy.deepcopy(net).double(), x.double(), 0.0
    with torch.no_grad():                                       # every activation an integer of magnitude <= 256
        for i, u in enumerate([n64.conv0, *n64.blocks]):
            h = torch.relu(u(h) if i == 0 else h + u(h))
            assert torch.equal(h, h.round()) and float(h.max()) <= 256
            peak = max(peak, float(h.max()))
    assert peak >= 2                                            # and not all zero
    p64, v64 = forward64(net, x)
    w = wrapper(net, cuda)
    with torch.no_grad(), w.inference_session():
        p, v = c_forward(w, x.to(cuda))
    assert torch.equal(p.cpu().double(), p64)
    assert err(v, v64) <= 2e-7


# ------------------------------------------------------------------------------------------------ statistics
def test_random_net_against_the_emulation(cuda):
    net = random_stats(seeded(12, seed=3), seed=4)
    x = observations(64, seed=5)
    w = wrapper(net, cuda)
    with torch.no_grad(), w.inference_session():
        p, v = c_forward(w, x.to(cuda))
        out = w(x.to(cuda))
    as_good_as_the_emulation(net, x, p, v)
    assert same_bits(out['policy'], p) and same_bits(out['value'], v)


# ------------------------------------------------------------------------------------------------ rows and passes
@pytest.fixture(scope='module', params=[1, 12])
def big(request, cuda):
    """Per depth: the wrapper inside a session, 2P + 1 observations and their one forward."""
    net = random_stats(seeded(request.param, seed=6), seed=7, gain=0.25)
    x = observations(2 * P + 1, seed=8).to(cuda)
    w = wrapper(net, cuda)
    with w.inference_session():
        p, v = c_forward(w, x)
        yield {'net': net, 'w': w, 'x': x, 'p': p, 'v': v}


def test_full_batch_at_both_ends(big):
    rows = list(range(16)) + list(range(2 * P + 1 - 16, 2 * P + 1))
    as_good_as_the_emulation(big['net'], big['x'][rows].cpu(), big['p'][rows], big['v'][rows])


@pytest.mark.parametrize('N', SIZES)
def test_batch_sizes_give_the_same_rows(big, N):
    p, v = c_forward(big['w'], big['x'][:N].contiguous())
    assert same_bits(p, big['p'][:N]) and same_bits(v, big['v'][:N])


def test_rows_are_independent_and_calls_repeat(big):
    n = P + 9                                                   # the garbage row's wave also runs a clean second pass
    bad = big['x'][:n].clone()
    bad[5] = 1e30
    p, v = c_forward(big['w'], bad)
    keep = torch.arange(n, device=bad.device) != 5
    assert same_bits(p[keep], big['p'][:n][keep]) and same_bits(v[keep], big['v'][:n][keep])
    again = c_forward(big['w'], bad)
    assert same_bits(again[0], p) and same_bits(again[1], v)


# ------------------------------------------------------------------------------------------------ sessions
def test_sessions_share_the_pack_and_a_forward_is_one_launch(cuda):
    from torch.profiler import ProfilerActivity, profile
    first, second = random_stats(seeded(2, seed=12), seed=13), random_stats(seeded(2, seed=14), seed=15)
    net = on_gpu(first, cuda)
    w = hnn.GeeseInference(net, precision='bf16')
    x = observations(70, seed=16).to(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad():
        with w.inference_session():
            ptr = w.pack().data_ptr()
            out1 = w(x)
            side = torch.cuda.Stream(cuda)
            side.wait_stream(torch.cuda.current_stream(cuda))
            with torch.cuda.stream(side):
                w(x)
            torch.cuda.current_stream(cuda).wait_stream(side)
            with torch.cuda.graph(graph):
                captured = w(x)
            for _ in range(3):
                graph.replay()
                torch.cuda.synchronize(cuda)
                assert same_bits(captured['policy'], out1['policy']) and same_bits(captured['value'], out1['value'])
        net.load_state_dict(second.state_dict())
        with w.inference_session():
            assert w.pack().data_ptr() == ptr
            out2 = w(x)
            graph.replay()
            torch.cuda.synchronize(cuda)
            assert not same_bits(out2['policy'], out1['policy'])
            assert same_bits(captured['policy'], out2['policy']) and same_bits(captured['value'], out2['value'])
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                w(x)
                torch.cuda.synchronize(cuda)
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(names) == 1 and 'geese_bf16_kernel' in names[0], names
    as_good_as_the_emulation(second, x.cpu(), out2['policy'], out2['value'])
