"""The one-launch GeisterNet inference without a GPU: the three C entries as include/hrl_nn.h declares them,
geister_inference_ok's structure check, nn.GeisterInference off the GPU and the ``inference`` key."""

import copy
import ctypes

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.geister import GeisterNet
from handyrl_amd.envs.hungry_geese import GeeseNet
from handyrl_amd.envs.tictactoe import SimpleConv2dModel

I64 = ctypes.c_int64


def test_entries_are_exported_with_the_header_signatures():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30
    sig = _native.SIGNATURES
    assert sig['hrl_geister_infer_pack_bytes'][0] is I64 and len(sig['hrl_geister_infer_pack_bytes'][1]) == 2
    assert sig['hrl_geister_infer_pack'][0] is ctypes.c_int and len(sig['hrl_geister_infer_pack'][1]) == 20
    assert sig['hrl_geister_infer'][0] is ctypes.c_int and len(sig['hrl_geister_infer'][1]) == 15
    assert all(getattr(lib, name).argtypes == sig[name][1] for name in sig if name.startswith('hrl_geister_infer'))
    # fragment sets of 27,648 B (the stem's 2, 16 per layer, the move head's 2), then 496 + 128 L floats
    for L, pf in ((1, 1), (2, 2), (3, 8), (4, 4)):
        assert lib.hrl_geister_infer_pack_bytes(L, pf) == (4 + 16 * L) * 27648 + (496 + 128 * L) * 4
    assert [lib.hrl_geister_infer_pack_bytes(L, pf) for L, pf in ((0, 8), (5, 8), (3, 3), (3, 16))] == [0] * 4


def test_geister_inference_ok_is_by_structure():
    net = GeisterNet()
    assert hnn.geister_inference_ok(net) and hnn.geister_inference_ok(hnn.accelerate(copy.deepcopy(net)))
    assert hnn.geister_inference_ok(GeisterNet(layers=1, p_filters=2, num_repeats=8))
    assert not hnn.geister_inference_ok(GeisterNet(filters=16))
    assert not hnn.geister_inference_ok(GeisterNet(layers=5))
    assert not hnn.geister_inference_ok(GeisterNet(num_repeats=9))
    assert not hnn.geister_inference_ok(SimpleConv2dModel(32, 3))
    assert not hnn.geister_inference_ok(GeeseNet())
    with pytest.raises(ValueError):
        hnn.GeisterInference(GeisterNet(layers=5))


def test_wrapper_off_the_gpu():
    torch.manual_seed(2)
    net = GeisterNet().eval()
    w = hnn.GeisterInference(net)
    assert not w.stateless_session and (w.layers, w.p_filters) == (3, 8)
    obs = {'board': torch.rand(5, 7, 6, 6), 'scalar': torch.rand(5, 18)}
    hidden = net.init_hidden([5])
    with torch.no_grad(), w.inference_session(inplace_state=True):
        got, ref = w(obs, hidden), net(obs, hidden)
    for k in ('policy', 'value', 'return'):
        assert torch.equal(got[k], ref[k])
    assert all(torch.equal(a, b) for a, b in zip(got['hidden'][0] + got['hidden'][1],
                                                  ref['hidden'][0] + ref['hidden'][1]))
    h = w.inference_hidden(4, 2, 'cpu')
    assert h[0][1].shape == (2, 4, 32, 6, 6) and len(w.init_hidden([4])[0]) == 3
    w.train()
    assert net.training
    with pytest.raises(RuntimeError, match='training'):
        w(obs, hidden)


@pytest.mark.gpu
def test_gpu_outside_a_session_raises(cuda):
    w = hnn.GeisterInference(GeisterNet().to(cuda).eval())
    with pytest.raises(RuntimeError, match='inference_session'):
        w({'board': torch.zeros(1, 7, 6, 6, device=cuda), 'scalar': torch.zeros(1, 18, device=cuda)})


def test_configured_inference_fused_geister():
    """``fused_geister`` wraps GeisterNets, each on its own; ``fused`` and ``fused_bf16`` keep refusing them (the
    suite already pins ``fused``'s refusal), and the refusal names the value that does."""
    cuda = torch.device('cuda')
    out = hnn.configured_inference('fused_geister', [GeisterNet(), GeisterNet(layers=2)], cuda)
    assert [type(w) for w in out] == [hnn.GeisterInference] * 2 and [w.layers for w in out] == [3, 2]
    for bad in ([GeisterNet(), GeeseNet()], [GeeseNet(), GeisterNet()], [SimpleConv2dModel(32, 3), GeisterNet()],
                [GeisterNet(filters=16)]):
        with pytest.raises(ValueError, match='inference'):
            hnn.configured_inference('fused_geister', bad, cuda)
        with pytest.raises(ValueError, match='inference'):
            hnn.configured_inference('fused', bad, cuda)
    with pytest.raises(ValueError, match='fused_geister'):
        hnn.configured_inference('fused', [GeisterNet()], cuda)
    with pytest.raises(ValueError, match='inference'):
        hnn.configured_inference('fused_bf16', [GeisterNet()], cuda)
    with pytest.raises(ValueError, match='inference'):
        hnn.configured_inference('fused_geister', [GeisterNet()], torch.device('cpu'))
