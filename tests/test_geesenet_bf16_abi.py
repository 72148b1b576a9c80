"""The bf16 one-launch GeeseNet forward (csrc/hrl_geesenet_bf16.hip, nn.GeeseInference(precision='bf16')): exports,
the pack size, argument validation before any HIP call, and the Python layer's CPU behaviour (no GPU)."""

import ctypes

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.hungry_geese import GeeseNet
from handyrl_amd.envs.tictactoe import SimpleConv2dModel

EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def _infer(null=(), layers=12, N=5, H=7, W=11, pack=None):
    a = {n: None if n in null else _p(i) for i, n in enumerate(('pack', 'x', 'policy', 'value'))}
    return _native.load().hrl_geesenet_infer_bf16(pack or a['pack'], layers, a['x'], N, H, W, a['policy'], a['value'],
                                                  None)


def test_exports_and_abi_version():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    for name in ('hrl_geesenet_infer_bf16_pack_bytes', 'hrl_geesenet_infer_bf16_pack', 'hrl_geesenet_infer_bf16'):
        assert name in _native.SIGNATURES and hasattr(lib, name)


def test_pack_bytes():
    lib = _native.load()
    assert [lib.hrl_geesenet_infer_bf16_pack_bytes(l) for l in (0, 17, -1)] == [0, 0, 0]
    sizes = [lib.hrl_geesenet_infer_bf16_pack_bytes(l) for l in range(1, 17)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and all(b > a for a, b in zip(sizes, sizes[1:]))


@pytest.mark.parametrize('kw', [{'null': ('pack',)}, {'null': ('x',)}, {'null': ('policy',)}, {'null': ('value',)},
                                {'layers': 0}, {'layers': 17}, {'H': 9, 'W': 9}, {'H': 0}, {'W': 0}, {'N': -1},
                                {'pack': ctypes.c_void_p(4096 + 4)}])
def test_infer_refuses_before_any_hip_call(kw):
    assert _infer(**kw) == EINVAL
    assert 'N' in kw or _infer(**dict(kw, N=0)) == EINVAL      # checked before the empty batch returns


def test_empty_batch_returns_before_any_launch():
    assert _infer(N=0) == OK                                   # the pointers are not device memory: nothing ran


def test_pack_refuses_like_the_tower():
    k = 4
    arr = lambda: (ctypes.c_void_p * k)(*[4096 * (u + 1) for u in range(k)])
    eps = (ctypes.c_double * k)(*([1e-5] * k))
    call = lambda layers, pack: _native.load().hrl_geesenet_infer_bf16_pack(
        arr(), arr(), arr(), arr(), arr(), arr(), eps, layers, _p(40), _p(41), pack, None)
    for layers, pack in ((0, _p(50)), (17, _p(50)), (3, None), (3, ctypes.c_void_p(4096 + 8))):
        assert call(layers, pack) == EINVAL, (layers, pack)


def test_cpu_batch_runs_the_net_and_a_bad_precision_raises():
    torch.manual_seed(5)
    net = GeeseNet(layers=2).eval()
    w = hnn.GeeseInference(net, precision='bf16')
    x = torch.randn(9, 17, 7, 11, generator=torch.Generator().manual_seed(1))
    with torch.no_grad(), w.inference_session():
        out, ref = w(x), net(x, None)
    assert torch.equal(out['policy'], ref['policy']) and torch.equal(out['value'], ref['value'])
    assert w.precision == 'bf16' and hnn.GeeseInference(net).precision == 'fp32'
    with pytest.raises(ValueError, match='precision'):
        hnn.GeeseInference(net, precision='fp16')


def test_configured_inference_fused_bf16():
    cuda = torch.device('cuda')
    with pytest.raises(ValueError, match='inference'):
        hnn.configured_inference('fused_bf16', [GeeseNet()], torch.device('cpu'))
    for bad in ([SimpleConv2dModel(32, 3)], [GeeseNet(layers=1), SimpleConv2dModel(32, 3)]):
        with pytest.raises(ValueError, match='inference'):
            hnn.configured_inference('fused_bf16', bad, cuda)
    with pytest.raises(ValueError, match='inference'):
        hnn.configured_inference('fused_fp8', [GeeseNet()], cuda)
    out = hnn.configured_inference('fused_bf16', [GeeseNet(layers=1), GeeseNet(layers=2)], cuda)
    assert [(type(w), w.precision, w.layers) for w in out] == [(hnn.GeeseInference, 'bf16', 1),
                                                              (hnn.GeeseInference, 'bf16', 2)]
    assert hnn.configured_inference('fused', [GeeseNet(layers=1)], cuda)[0].precision == 'fp32'
