"""The bf16 one-launch GeisterNet inference without a GPU: the three C entries as include/hrl_nn.h declares them,
``precision`` on nn.GeisterInference and the ``inference`` key's ``fused_geister_bf16`` value."""

import ctypes

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.geister import GeisterNet
from handyrl_amd.envs.hungry_geese import GeeseNet
from handyrl_amd.envs.tictactoe import SimpleConv2dModel


def test_entries_are_exported_with_the_header_signatures():
    lib, sig = _native.load(), _native.SIGNATURES
    assert lib.hrl_abi_version() == 30
    for name, res, nargs in (('_pack_bytes', ctypes.c_int64, 2), ('_pack', ctypes.c_int, 20), ('', ctypes.c_int, 15)):
        new, old = sig['hrl_geister_infer_bf16' + name], sig['hrl_geister_infer' + name]
        assert new[0] is res and len(new[1]) == nargs and list(new[1]) == list(old[1])
        assert getattr(lib, 'hrl_geister_infer_bf16' + name).argtypes == new[1]
    # fragment sets of 9 taps x 64 lanes x 16 B (the stem's 2, 16 per layer, the move head's 2), then 496 + 128 L floats
    for L, pf in ((1, 1), (2, 2), (3, 8), (4, 4)):
        nbytes = lib.hrl_geister_infer_bf16_pack_bytes(L, pf)
        assert nbytes == (4 + 16 * L) * 9216 + (496 + 128 * L) * 4 and nbytes % 16 == 0
    assert [lib.hrl_geister_infer_bf16_pack_bytes(L, pf) for L, pf in ((0, 8), (5, 8), (3, 3), (3, 16))] == [0] * 4


def test_precision_argument_and_the_cpu_wrapper():
    torch.manual_seed(2)
    net = GeisterNet().eval()
    assert hnn.GeisterInference(net).precision == 'fp32'
    for bad in ('fp16', 'BF16', None, 16):
        with pytest.raises(ValueError, match='precision'):
            hnn.GeisterInference(net, precision=bad)
    w = hnn.GeisterInference(net, precision='bf16')
    assert w.precision == 'bf16' and not w.stateless_session and (w.layers, w.p_filters) == (3, 8)
    obs = {'board': torch.rand(5, 7, 6, 6), 'scalar': torch.rand(5, 18)}
    hidden = net.init_hidden([5])
    with torch.no_grad(), w.inference_session(inplace_state=True):
        got, ref = w(obs, hidden), net(obs, hidden)   # off the GPU: the net's own (exact) forward
    assert all(torch.equal(got[k], ref[k]) for k in ('policy', 'value', 'return'))
    assert all(torch.equal(a, b) for a, b in zip(got['hidden'][0] + got['hidden'][1],
                                                  ref['hidden'][0] + ref['hidden'][1]))
    assert w.inference_hidden(4, 2, 'cpu')[0][1].shape == (2, 4, 32, 6, 6) and len(w.init_hidden([4])[0]) == 3
    w.train()
    with pytest.raises(RuntimeError, match='training'):
        w(obs, hidden)


def test_configured_inference_fused_geister_bf16():
    cuda = torch.device('cuda')
    out = hnn.configured_inference('fused_geister_bf16', [GeisterNet(), GeisterNet(layers=2)], cuda)
    assert [type(w) for w in out] == [hnn.GeisterInference] * 2 and [w.layers for w in out] == [3, 2]
    assert [w.precision for w in out] == ['bf16'] * 2
    assert hnn.configured_inference('fused_geister', [GeisterNet()], cuda)[0].precision == 'fp32'
    for bad in ([GeeseNet()], [SimpleConv2dModel(32, 3)], [GeisterNet(filters=16)], [GeisterNet(), GeeseNet()],
                [SimpleConv2dModel(32, 3), GeisterNet()]):
        with pytest.raises(ValueError, match='inference'):
            hnn.configured_inference('fused_geister_bf16', bad, cuda)
    with pytest.raises(ValueError, match='inference'):
        hnn.configured_inference('fused_geister_bf16', [GeisterNet()], torch.device('cpu'))
    with pytest.raises(ValueError, match='fused_geister_bf16'):
        hnn.configured_inference('fused_geister_fp16', [GeisterNet()], cuda)
