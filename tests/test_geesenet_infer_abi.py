"""The GeeseNet inference tower (csrc/hrl_geesenet.hip, nn.GeeseInference): exports, the pack size, argument
validation (before any HIP call) and the Python layer's CPU behaviour (no GPU)."""

import copy
import ctypes

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.geister import GeisterNet
from handyrl_amd.envs.hungry_geese import GeeseNet
from handyrl_amd.envs.tictactoe import SimpleConv2dModel

EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK
NAMES = ('hrl_geesenet_infer_pack_bytes', 'hrl_geesenet_infer_pack', 'hrl_geesenet_infer_workspace_bytes',
         'hrl_geesenet_infer', 'hrl_geesenet_infer_set_form')


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def _infer(null=(), layers=12, N=5, H=7, W=11, short=0):
    lib = _native.load()
    a = {n: None if n in null else _p(i) for i, n in enumerate(('pack', 'x', 'policy', 'value', 'ws'))}
    need = max(lib.hrl_geesenet_infer_workspace_bytes(N, H, W), 0)
    return lib.hrl_geesenet_infer(a['pack'], layers, a['x'], N, H, W, a['policy'], a['value'], a['ws'], need - short,
                                  None)


PER_UNIT = ('conv_w', 'conv_b', 'bn_w', 'bn_b', 'bn_mean', 'bn_var')
PACK_PTRS = PER_UNIT + ('eps', 'head_p', 'head_v', 'pack')


def _pack(null=(), layers=3, null_unit=None):
    k = min(max(layers, 1), 16) + 1
    a = {}
    for i, n in enumerate(PACK_PTRS):
        if n in PER_UNIT:
            a[n] = (ctypes.c_void_p * k)(*[None if null_unit == (n, u) else 4096 * (32 * i + u + 1) for u in range(k)])
        elif n == 'eps':
            a[n] = (ctypes.c_double * k)(*([1e-5] * k))
        else:
            a[n] = _p(512 + i)
        if n in null:
            a[n] = None
    return _native.load().hrl_geesenet_infer_pack(a['conv_w'], a['conv_b'], a['bn_w'], a['bn_b'], a['bn_mean'],
                                                  a['bn_var'], a['eps'], layers, a['head_p'], a['head_v'], a['pack'],
                                                  None)


def test_exports_and_abi_version():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    for name in NAMES:
        assert name in _native.SIGNATURES and hasattr(lib, name)


def test_pack_bytes():
    lib = _native.load()
    for layers in (0, 17, -1):
        assert lib.hrl_geesenet_infer_pack_bytes(layers) == 0
    sizes = [lib.hrl_geesenet_infer_pack_bytes(l) for l in range(1, 17)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert all(b > a for a, b in zip(sizes, sizes[1:]))


def test_workspace_bytes():
    lib = _native.load()
    assert lib.hrl_geesenet_infer_workspace_bytes(0, 7, 11) == 0
    assert lib.hrl_geesenet_infer_workspace_bytes(3, 7, 11) == 3 * 32 * 77 * 4
    assert lib.hrl_geesenet_infer_workspace_bytes(3, 8, 10) == 3 * 32 * 80 * 4
    for bad in ((-1, 7, 11), (3, 9, 9), (3, 0, 11), (3, 7, 0)):
        assert lib.hrl_geesenet_infer_workspace_bytes(*bad) == -1, bad


def test_infer_validates_arguments():
    assert _infer(N=0) == OK                                  # N == 0: no launch
    assert _infer(N=0, null=('ws',)) == OK
    for name in ('pack', 'x', 'policy', 'value'):
        for N in (0, 5):
            assert _infer(null=(name,), N=N) == EINVAL, (name, N)
    assert _infer(null=('ws',)) == EINVAL
    for kw in ({'layers': 0}, {'layers': 17}, {'layers': -1}, {'H': 9, 'W': 9}, {'H': 0}, {'W': 0}, {'N': -1},
               {'short': 1}):
        assert _infer(**kw) == EINVAL, kw


def test_infer_wants_aligned_buffers():
    lib = _native.load()
    assert lib.hrl_geesenet_infer(_p(0), 12, _p(1), 5, 7, 11, _p(2), _p(3), ctypes.c_void_p(4096 * 9 + 8),
                                  5 * 32 * 77 * 4, None) == EINVAL          # a ws that is not 16-byte aligned
    assert lib.hrl_geesenet_infer(ctypes.c_void_p(4096 + 4), 12, _p(1), 5, 7, 11, _p(2), _p(3), _p(4),
                                  5 * 32 * 77 * 4, None) == EINVAL          # nor the pack


def test_pack_validates_arguments():
    for name in PACK_PTRS:
        assert _pack(null=(name,)) == EINVAL, name
    for layers in (0, 17, -1):
        assert _pack(layers=layers) == EINVAL, layers
    for name in PER_UNIT:
        for u in (0, 3):
            assert _pack(null_unit=(name, u)) == EINVAL, (name, u)


def test_set_form_queries_and_sets():
    lib = _native.load()
    prev = lib.hrl_geesenet_infer_set_form(-1)
    try:
        assert lib.hrl_geesenet_infer_set_form(2) == prev
        assert lib.hrl_geesenet_infer_set_form(7) == 2        # any other value only queries
        assert lib.hrl_geesenet_infer_set_form(1) == 2
        assert lib.hrl_geesenet_infer_set_form(0) == 1
    finally:
        lib.hrl_geesenet_infer_set_form(prev)


def test_geese_inference_ok():
    for net in (GeeseNet(), GeeseNet(layers=1), GeeseNet(layers=16)):
        assert hnn.geese_inference_ok(net)
        acc = hnn.accelerate(copy.deepcopy(net))
        assert acc.conv0.use_hip and hnn.geese_inference_ok(acc)
        assert list(acc.state_dict()) == list(net.state_dict())
    assert not hnn.geese_inference_ok(SimpleConv2dModel(32, 3))
    assert not hnn.geese_inference_ok(GeisterNet())
    assert not hnn.geese_inference_ok(GeeseNet(filters=16))
    assert not hnn.geese_inference_ok(GeeseNet(layers=17))
    net = GeeseNet(layers=2)
    net.blocks[1].bn = torch.nn.BatchNorm2d(32, track_running_stats=False)
    assert not hnn.geese_inference_ok(net)
    with pytest.raises(ValueError):
        hnn.GeeseInference(net)
    net = GeeseNet(layers=2)
    net.head_v = torch.nn.Linear(64, 1)                       # a bias the tail does not apply
    assert not hnn.geese_inference_ok(net)
    net = GeeseNet(layers=2)
    net.init_hidden = lambda *a: None
    assert not hnn.geese_inference_ok(net)


def _seeded(layers=2):
    torch.manual_seed(5)
    return GeeseNet(layers=layers).eval()


def test_cpu_wrapper_is_the_net():
    net = _seeded()
    wrapped = hnn.GeeseInference(net)
    x = torch.randn(9, 17, 7, 11, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = net(x, None)
        for out in (wrapped(x, None), wrapped(x)):
            assert set(out) == {'policy', 'value'}
            assert torch.equal(out['policy'], ref['policy']) and torch.equal(out['value'], ref['value'])
        with wrapped.inference_session(inplace_state=True):       # nothing to prepare on the CPU
            assert torch.equal(wrapped(x)['policy'], ref['policy'])
    assert wrapped.stateless_session and wrapped.layers == 2
    assert [k for k, _ in wrapped.state_dict().items()] == list(net.state_dict())
    assert list(wrapped.parameters())[0] is list(net.parameters())[0]
    assert [b.data_ptr() for b in wrapped.buffers()] == [b.data_ptr() for b in net.buffers()]
    assert wrapped.eval() is wrapped and not wrapped.training
    assert wrapped.train(False) is wrapped and not net.training
    assert wrapped.to('cpu') is wrapped
    wrapped.load_state_dict(copy.deepcopy(net.state_dict()))
    assert not hasattr(wrapped, 'init_hidden') and not hasattr(wrapped, 'inference_hidden')


def test_training_mode_raises():
    net = _seeded(1)
    wrapped = hnn.GeeseInference(net)
    wrapped.train()
    assert net.training and wrapped.training
    with pytest.raises(RuntimeError):
        wrapped(torch.zeros(2, 17, 7, 11))


def test_configured_inference_names_the_key():
    cpu = torch.device('cpu')
    with pytest.raises(ValueError, match='inference'):
        hnn.configured_inference('fused', [GeeseNet()], cpu)
    nets = [GeeseNet(layers=1)]
    assert hnn.configured_inference(None, nets, cpu) is nets
    # the choice of wrapper is by structure and needs no device: a mixed list, or any other net, names the key
    cuda = torch.device('cuda')
    for bad in ([GeeseNet(layers=1), SimpleConv2dModel(32, 3)], [SimpleConv2dModel(32, 3), GeeseNet(layers=1)],
                [GeisterNet()], [GeeseNet(filters=16)]):
        with pytest.raises(ValueError, match='inference'):
            hnn.configured_inference('fused', bad, cuda)
    out = hnn.configured_inference('fused', [GeeseNet(layers=1), GeeseNet(layers=2)], cuda)
    assert [type(w) for w in out] == [hnn.GeeseInference] * 2 and [w.layers for w in out] == [1, 2]
