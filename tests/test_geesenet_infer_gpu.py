"""The GeeseNet inference tower on the GPU (csrc/hrl_geesenet.hip), called at the C entry with guard-band buffers
(tests/guarded.py: outputs and the workspace sit between sentinels, checked after every call) and through
nn.GeeseInference.

References: the reference project's recorded eval forward (tests/golden/geese_net.npz, 1e-5 as
tests/test_geese_golden.py sets it for the GPU eval forward) and the fp64 torch-CPU forward of the same net.

Launch shapes: batches of up to 1024 rows run workgroups of 2 waves on a grid of at most 512 (one sample per wave),
larger ones workgroups of 8 waves on a grid of at most 256, so a wave takes a second sample -- and the prefetch path
first runs -- at N = 2049; forcing the 2-wave shape (hrl_geesenet_infer_set_form(2)) puts that boundary at 1025.  The
batch sizes are the wave counts of both workgroups +- 1 (1, 2, 3, 7, 8, 9), the switch between the shapes (1023,
1024, 1025) and the second-sample boundary (2047, 2049).  A row's result does not depend on N, so the large batches
are compared bit for bit with the rows of one N = 2049 forward, and that one with the fp64 forward on the rows at
both ends."""

import copy

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.hungry_geese import GeeseNet
from tests.conftest import load_golden
from tests.guarded import Arena, bits

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 7, 8, 9, 1023, 1024, 1025, 2047, 2049)
NMAX = max(SIZES)


def seeded(layers, seed=21):
    torch.manual_seed(seed)
    return GeeseNet(layers=layers).eval()


def random_stats(net, seed, gain=1.0):
    """BN running means / vars, BN weights / biases and conv biases seeded random: vars in [0.25, 4], the rest O(1);
    ``gain`` scales the BN weights (below 1 the residual tower's activations grow less with depth)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for u in [net.conv0, *net.blocks]:
            u.bn.running_mean.copy_(torch.randn(32, generator=g) * 0.5)
            u.bn.running_var.copy_(torch.rand(32, generator=g) * 3.75 + 0.25)
            u.bn.weight.copy_((torch.rand(32, generator=g) + 0.5) * gain)
            u.bn.bias.copy_(torch.randn(32, generator=g) * 0.5)
            u.conv.bias.copy_(torch.randn(32, generator=g) * 0.5)
    return net


def observations(N, H=7, W=11, seed=0):
    """Geese-like planes: mostly binary, plane 0 (the pool's weights) one-hot-ish, a few real values."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, 17, H, W, generator=g) < 0.15).float()
    x[:, 16] = torch.rand(N, H, W, generator=g)
    x[:, 0] = (torch.rand(N, H, W, generator=g) < 0.05).float() * (1 + torch.rand(N, H, W, generator=g))
    return x


def forward64(net, x):
    n64 = copy.deepcopy(net).cpu().double().eval()
    with torch.no_grad():
        out = n64(x.cpu().double())
    return out['policy'], out['value']


def on_gpu(net, cuda):
    return hnn.accelerate(copy.deepcopy(net).to(cuda)).eval()


def c_forward(wrapper, x, arena=None):
    """hrl_geesenet_infer on ``x`` with guarded outputs and a workspace of exactly the bytes asked for."""
    lib = _native.load()
    arena = arena or Arena(x.device)
    N, _, H, W = x.shape
    policy, value = arena.out((N, 4), name='policy'), arena.out((N, 1), name='value')
    nbytes = lib.hrl_geesenet_infer_workspace_bytes(N, H, W)
    ws = arena.ws(nbytes, name='ws')
    code = lib.hrl_geesenet_infer(_native.ptr(wrapper.pack(x.device)), wrapper.layers, _native.ptr(x), N, H, W,
                                  _native.ptr(policy), _native.ptr(value), _native.ptr(ws), nbytes,
                                  _native.stream_of(x.device))
    assert code == _native.HRL_OK, code
    arena.check()
    return policy.clone(), value.clone()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ golden
def test_golden_eval_forward(cuda):
    """The reference's eval forward follows its train forward (running statistics after one batch), as in
    tests/test_geese_golden.py::_forward_check."""
    _, arrays = load_golden('geese_net')
    x = torch.from_numpy(arrays['fwd.x']).to(cuda)
    torch.manual_seed(21)
    net = hnn.accelerate(GeeseNet().to(cuda))
    net.train()
    net(x)
    net.eval()
    w = hnn.GeeseInference(net)
    with torch.no_grad(), w.inference_session():
        out = w(x)
        p, v = c_forward(w, x)
    for got_p, got_v in ((out['policy'], out['value']), (p, v)):
        torch.testing.assert_close(got_p.cpu(), torch.from_numpy(arrays['fwd.eval_policy']), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(got_v.cpu(), torch.from_numpy(arrays['fwd.eval_value']), rtol=1e-5, atol=1e-5)
    assert same_bits(out['policy'], p) and same_bits(out['value'], v)


# ------------------------------------------------------------------------------------------------ statistics
def test_non_trivial_statistics_against_fp64(cuda):
    """Wrapper and module-by-module GPU eval forward against the fp64 CPU forward: the wrapper's largest absolute
    error may be twice the module path's plus 1e-6 (the fold and the summation order differ; 1e-6 is the golden
    test's CPU atol).  Measured on an MI355X (printed below): policy 9.33e-06 against the module path's 9.33e-06
    (logits up to 22.3), value 7.4e-08 against 8.7e-08."""
    net = random_stats(seeded(12, seed=3), seed=4)
    x = observations(64, seed=5)
    p64, v64 = forward64(net, x)
    gnet = on_gpu(net, cuda)
    w = hnn.GeeseInference(gnet)
    with torch.no_grad():
        mod = gnet(x.to(cuda))
        with w.inference_session():
            p, v = c_forward(w, x.to(cuda))
    err = lambda got, ref: float((got.cpu().double() - ref).abs().max())
    ep_m, ev_m = err(mod['policy'], p64), err(mod['value'], v64)
    ep_w, ev_w = err(p, p64), err(v, v64)
    print('max |error| against fp64: policy wrapper %.3e module %.3e; value wrapper %.3e module %.3e  '
          '(policy range %.2f, value range %.2f)' % (ep_w, ep_m, ev_w, ev_m, float(p64.abs().max()),
                                                     float(v64.abs().max())))
    assert float(p64.abs().max()) > 0.1 and float(v64.abs().min()) < 0.9        # neither dead nor all saturated
    assert ep_w <= 2 * ep_m + 1e-6, (ep_w, ep_m)
    assert ev_w <= 2 * ev_m + 1e-6, (ev_w, ev_m)


# ------------------------------------------------------------------------------------------------ shapes
@pytest.fixture(scope='module', params=[1, 2, 12])
def big(request, cuda):
    """Per depth: the net's wrapper inside a session, NMAX observations, their forward at N = NMAX."""
    layers = request.param
    net = random_stats(seeded(layers, seed=6), seed=7, gain=0.25)
    x = observations(NMAX, seed=8).to(cuda)
    w = hnn.GeeseInference(on_gpu(net, cuda))
    with w.inference_session():
        p, v = c_forward(w, x)
        yield {'net': net, 'w': w, 'x': x, 'p': p, 'v': v, 'layers': layers}


def close64(p, v, p64, v64):
    """The project's forward bound, 1e-5, relative to the scale of the logits (the residual tower's activations, and
    with them the fp32 rounding of every forward, grow with depth: up to 26 at 12 blocks here); the value, a tanh of
    a sum of the same features, to the same bound."""
    tol = 1e-5 * max(1.0, float(p64.abs().max()))
    ep, ev = float((p.cpu().double() - p64).abs().max()), float((v.cpu().double() - v64).abs().max())
    assert ep <= tol and ev <= tol, (ep, ev, tol)


def test_full_batch_against_fp64_at_both_ends(big):
    rows = list(range(24)) + list(range(1016, 1032)) + list(range(NMAX - 24, NMAX))   # incl. each wave's 2nd sample
    p64, v64 = forward64(big['net'], big['x'][rows])
    close64(big['p'][rows], big['v'][rows], p64, v64)


@pytest.mark.parametrize('N', SIZES)
def test_batch_sizes_give_the_same_rows(big, N):
    p, v = c_forward(big['w'], big['x'][:N].contiguous())
    assert same_bits(p, big['p'][:N]) and same_bits(v, big['v'][:N])


@pytest.mark.parametrize('form,N', [(1, 9), (1, 1025), (2, 1023), (2, 1025), (2, 2049)])
def test_launch_shapes_are_bit_identical(big, form, N):
    """The 8-wave shape on small batches and the 2-wave shape past its one-pass grid (1024 samples): the same bits."""
    lib = _native.load()
    prev = lib.hrl_geesenet_infer_set_form(form)
    try:
        p, v = c_forward(big['w'], big['x'][:N].contiguous())
    finally:
        lib.hrl_geesenet_infer_set_form(prev)
    assert same_bits(p, big['p'][:N]) and same_bits(v, big['v'][:N])


@pytest.mark.parametrize('H,W', [(4, 5), (8, 10), (1, 3)])
def test_other_boards_against_the_fp64_torus_forward(cuda, H, W):
    """Nothing is fixed at 77 cells: a 4x5 board, the largest (80 cells), and one narrower than the kernel."""
    net = random_stats(seeded(2, seed=9), seed=10)
    x = observations(19, H, W, seed=11)
    p64, v64 = forward64(net, x)
    w = hnn.GeeseInference(on_gpu(net, cuda))
    with torch.no_grad(), w.inference_session():
        p, v = c_forward(w, x.to(cuda))
        out = w(x.to(cuda))
    close64(p, v, p64, v64)
    assert same_bits(out['policy'], p) and same_bits(out['value'], v)


def test_empty_batch(cuda):
    w = hnn.GeeseInference(on_gpu(seeded(1), cuda))
    with torch.no_grad(), w.inference_session():
        out = w(torch.empty(0, 17, 7, 11, device=cuda))
    assert out['policy'].shape == (0, 4) and out['value'].shape == (0, 1)


# ------------------------------------------------------------------------------------------------ rows
def test_rows_are_independent(big):
    N = 1100                                                   # the 8-wave shape; 300: the 2-wave one
    for n in (N, 300):
        x = big['x'][:n]
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(x.device)
        p, v = c_forward(big['w'], x[perm].contiguous())
        assert same_bits(p, big['p'][:n][perm]) and same_bits(v, big['v'][:n][perm])
        bad = x.clone()
        bad[n // 2] = 1e30                                     # a finite garbage row
        p, v = c_forward(big['w'], bad)
        keep = torch.arange(n, device=x.device) != n // 2
        assert same_bits(p[keep], big['p'][:n][keep]) and same_bits(v[keep], big['v'][:n][keep])


def test_deterministic(big):
    x = big['x'][:1500].contiguous()
    a, b = c_forward(big['w'], x), c_forward(big['w'], x)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


# ------------------------------------------------------------------------------------------------ sessions
def test_wrapper_raises_outside_a_session_and_in_training_mode(cuda):
    w = hnn.GeeseInference(on_gpu(seeded(1), cuda))
    x = observations(3).to(cuda)
    with pytest.raises(RuntimeError, match='inference_session'):
        w(x)
    with w.inference_session():
        w.train()
        with pytest.raises(RuntimeError, match='training'):
            w(x)
        w.eval()
        with pytest.raises(ValueError, match='observations'):
            w(x.double())
        with pytest.raises(ValueError, match='observations'):
            w(torch.zeros(3, 17, 9, 9, device=cuda))
        with torch.no_grad():
            assert w(x)['policy'].shape == (3, 4)
    assert w._live == 0


def test_repack_in_place_and_graph_replay(cuda):
    """A second session refreshes the same pack buffer: the wrapper follows the new weights, and so does a forward
    captured in a graph during the first session."""
    first, second = random_stats(seeded(2, seed=12), seed=13), random_stats(seeded(2, seed=14), seed=15)
    net = on_gpu(first, cuda)
    w = hnn.GeeseInference(net)
    x = observations(70, seed=16).to(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad():
        with w.inference_session():
            ptr = w.pack().data_ptr()
            out1 = w(x)
            side = torch.cuda.Stream(cuda)
            side.wait_stream(torch.cuda.current_stream(cuda))
            with torch.cuda.stream(side):
                w(x)                                            # warm on the capture stream's side
            torch.cuda.current_stream(cuda).wait_stream(side)
            with torch.cuda.graph(graph):
                captured = w(x)
            graph.replay()
            torch.cuda.synchronize(cuda)
            assert same_bits(captured['policy'], out1['policy']) and same_bits(captured['value'], out1['value'])
        net.load_state_dict(second.state_dict())                # in place: the net's tensors keep their addresses
        with w.inference_session():
            assert w.pack().data_ptr() == ptr
            out2 = w(x)
            graph.replay()
            torch.cuda.synchronize(cuda)
            mod = net(x)
    assert not same_bits(out2['policy'], out1['policy'])
    assert same_bits(captured['policy'], out2['policy']) and same_bits(captured['value'], out2['value'])
    p64, v64 = forward64(second, x)
    close64(out2['policy'], out2['value'], p64, v64)
    close64(mod['policy'], mod['value'], p64, v64)


def test_forward_is_layers_plus_one_launches(cuda):
    from torch.profiler import ProfilerActivity, profile
    for layers in (1, 12):
        w = hnn.GeeseInference(on_gpu(seeded(layers), cuda))
        x = observations(40).to(cuda)
        with torch.no_grad(), w.inference_session():
            w(x)
            torch.cuda.synchronize(cuda)
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                w(x)
                torch.cuda.synchronize(cuda)
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        assert len(names) == layers + 1 and all('geese_unit_kernel' in n for n in names), names
