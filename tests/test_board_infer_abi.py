"""The one-launch TicTacToe inference (csrc/hrl_infer.hip, nn.BoardInference): exports, argument validation (before
any HIP call) and the Python layer's CPU behaviour (no GPU)."""

import copy
import ctypes

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.geister import GeisterNet
from handyrl_amd.envs.tictactoe import SimpleConv2dModel

from . import board_infer_util as util

EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def _infer(null=(), K=1, span=(0, 0), N=0, layers=3, stride=None):
    lib = _native.load()
    a = {n: None if n in null else _p(i) for i, n in enumerate(('pack', 'obs', 'policy', 'value'))}
    sp = None if 'span' in null else _native.i64_array(list(span))
    stride = lib.hrl_board_infer_pack_bytes(min(max(layers, 1), 8)) if stride is None else stride
    return lib.hrl_board_infer(a['pack'], stride, K, sp, a['obs'], N, layers, a['policy'], a['value'], None)


PACK_PTRS = ('stem_w', 'stem_b', 'conv_w', 'bn_w', 'bn_b', 'bn_mean', 'bn_var', 'eps', 'w1p', 'b1p', 'w1v', 'b1v',
             'fcp', 'fcv', 'pack')


def _pack(null=(), layers=3, null_layer=None):
    k = min(max(layers, 1), 8)
    a = {}
    for i, n in enumerate(PACK_PTRS):
        if n in ('conv_w', 'bn_w', 'bn_b', 'bn_mean', 'bn_var'):
            vals = [None if null_layer == (n, l) else 4096 * (16 * i + l + 1) for l in range(k)]
            a[n] = (ctypes.c_void_p * k)(*vals)
        elif n == 'eps':
            a[n] = (ctypes.c_double * k)(*([1e-5] * k))
        else:
            a[n] = _p(64 + i)
        if n in null:
            a[n] = None
    return _native.load().hrl_board_infer_pack(a['stem_w'], a['stem_b'], a['conv_w'], a['bn_w'], a['bn_b'],
                                               a['bn_mean'], a['bn_var'], a['eps'], layers, a['w1p'], a['b1p'],
                                               a['w1v'], a['b1v'], a['fcp'], a['fcv'], a['pack'], None)


def test_exports_and_abi_version():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    for name in ('hrl_board_infer_pack_bytes', 'hrl_board_infer_pack', 'hrl_board_infer'):
        assert name in _native.SIGNATURES and hasattr(lib, name)


def test_pack_bytes_monotone():
    lib = _native.load()
    sizes = [lib.hrl_board_infer_pack_bytes(l) for l in range(1, 9)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    assert lib.hrl_board_infer_pack_bytes(0) == 0 == lib.hrl_board_infer_pack_bytes(9)


def test_infer_validates_arguments():
    assert _infer() == OK                                    # N == 0: no launch
    assert _infer(K=3, span=(0, 0, 0, 0)) == OK              # empty spans are legal
    for name in ('pack', 'obs', 'policy', 'value', 'span'):
        assert _infer(null=(name,)) == EINVAL, name
    for kw in ({'layers': 0}, {'layers': 9}, {'N': -1, 'span': (0, -1)}, {'K': 0}, {'K': -1},
               {'K': 2, 'span': (0, 5, 3), 'N': 3},            # not ascending
               {'K': 2, 'span': (0, 2, 4), 'N': 5},            # last offset != N
               {'K': 2, 'span': (0, 2, 4), 'N': 3},
               {'K': 1, 'span': (1, 4), 'N': 4},               # first offset != 0
               {'K': 2, 'span': (0, 0, 0), 'stride': 16}):     # packs closer than a pack
        assert _infer(**kw) == EINVAL, kw


def test_pack_validates_arguments():
    for name in PACK_PTRS:
        assert _pack(null=(name,)) == EINVAL, name
    for layers in (0, 9, -1):
        assert _pack(layers=layers) == EINVAL, layers
    for name in ('conv_w', 'bn_w', 'bn_b', 'bn_mean', 'bn_var'):
        assert _pack(null_layer=(name, 2)) == EINVAL, name


def test_board_inference_ok():
    for L in (1, 3, 8):
        net = SimpleConv2dModel(32, L)
        assert hnn.board_inference_ok(net)
        acc = hnn.accelerate(copy.deepcopy(net))
        assert hnn.board_inference_ok(acc)
        hnn.fuse_bn_relu(acc)
        assert hnn.board_inference_ok(acc)
        assert list(acc.state_dict()) == list(net.state_dict())
    assert not hnn.board_inference_ok(SimpleConv2dModel(16, 3))
    assert not hnn.board_inference_ok(SimpleConv2dModel(32, 9))
    assert not hnn.board_inference_ok(GeisterNet())
    net = SimpleConv2dModel(32, 3)
    net.blocks[1].bn = torch.nn.BatchNorm2d(32, track_running_stats=False)
    assert not hnn.board_inference_ok(net)
    with pytest.raises(ValueError):
        hnn.BoardInference(net)


def test_cpu_wrapper_is_the_net():
    net = util.seeded_net(3)
    wrapped = hnn.BoardInference(net)
    x = util.floats(37)
    with torch.no_grad():
        ref = net(x, None)
        for out in (wrapped(x, None), wrapped(x)):
            assert set(out) == {'policy', 'value'}
            assert torch.equal(out['policy'], ref['policy']) and torch.equal(out['value'], ref['value'])
        with wrapped.inference_session(inplace_state=True):       # nothing to prepare on the CPU
            assert torch.equal(wrapped(x)['policy'], ref['policy'])
    assert [k for k, _ in wrapped.state_dict().items()] == list(net.state_dict())
    assert list(wrapped.parameters())[0] is list(net.parameters())[0]
    assert wrapped.eval() is wrapped and not wrapped.training
    assert wrapped.train(False) is wrapped and not net.training
    assert not hasattr(wrapped, 'init_hidden') and not hasattr(wrapped, 'inference_hidden')


def test_training_mode_raises():
    net = util.seeded_net(1)
    wrapped = hnn.BoardInference(net)
    wrapped.train()
    assert net.training and wrapped.training
    with pytest.raises(RuntimeError):
        wrapped(util.planes(4))


def test_group_cpu_and_depths():
    nets = [util.seeded_net(3, seed=s) for s in range(3)]
    group = hnn.board_inference_group(nets)
    assert len(group) == 3 and all(isinstance(m, hnn.BoardInference) for m in group)
    x = util.floats(40)
    span = [0, 5, 5, 40]
    with torch.no_grad():
        out = group.forward(x, span)
        ref = torch.cat([nets[k](x[span[k]:span[k + 1]], None)['policy'] for k in range(3)])
    assert torch.equal(out['policy'], ref)
    with pytest.raises(ValueError):
        hnn.board_inference_group([util.seeded_net(3), util.seeded_net(1)])
    with pytest.raises(ValueError):
        group.forward(x, [0, 40])


def test_reference_precision_of_the_seeded_data():
    """The bound of the GPU tests is 1e-5 against the fp64 forward: the plain fp32 CPU forward of the same nets and
    inputs must itself sit well inside it."""
    for L in (1, 3, 8):
        net = util.seeded_net(L)
        for x in (util.planes(1003), util.floats(1003)):
            p64, v64 = util.forward64(net, x)
            with torch.no_grad():
                out = net(x, None)
            assert (out['policy'].double() - p64).abs().max() < 1e-6
            assert (out['value'].double() - v64).abs().max() < 1e-6


def test_integer_data_is_exact():
    """The exactness data: fp32 and fp64 torch forwards agree exactly, every head pre-activation is >= 0."""
    for L in (1, 3, 8):
        net = util.integer_net(L)
        for x in (util.planes(1003), util.quarters(1003)):
            p64, _ = util.forward64(net, x)
            with torch.no_grad():
                out = net(x, None)
            assert torch.equal(out['policy'].double(), p64)
            hp, hv = util.head_preacts64(net, x)
            assert hp.min() >= 0 and hv.min() >= 0
            pre = util.value_preact64(net, x)
            assert ((pre.abs() < 3).float().mean() > 0.1)        # tanh is not saturated everywhere
