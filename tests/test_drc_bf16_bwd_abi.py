"""The one-launch bf16 backward of the DRC time step (csrc/hrl_drc_bf16_bwd.hip, train_args precision: bf16_drc_bwd):
exports, argument validation before any HIP call, and the option's rules in the Python layer (no GPU)."""

import ctypes

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.geister import GeisterNet
from handyrl_amd.envs.hungry_geese import GeeseNet
from handyrl_amd.envs.tictactoe import SimpleConv2dModel

EINVAL = _native.HRL_EINVAL


def test_exports_and_pack_bytes():
    lib = _native.load()
    for name in ('hrl_drc_bf16_adjoint_pack_bytes', 'hrl_drc_bf16_adjoint_pack', 'hrl_drc_bf16_step_backward'):
        assert name in _native.SIGNATURES and getattr(lib, name)
    # L * 9 taps * 4 k-steps * 2 column tiles * 64 lanes * 16 B
    assert [lib.hrl_drc_bf16_adjoint_pack_bytes(L) for L in (0, 1, 3, 4, 5)] == [0, 73728, 221184, 294912, 0]


def _backward(lib, L=2, R=3, H=32, N=9, ghs=32 * 36, gcs=32 * 36, pack_bytes=None, pack=4096, layer=None, null=None,
              odd=None):
    """hrl_drc_bf16_step_backward on made-up pointers (not device memory: a launch would fault)."""
    tab = lambda base, n=32: (ctypes.c_void_p * n)(*[base + 65536 * i for i in range(n)])
    i64 = lambda *v: (ctypes.c_int64 * 4)(*(v * 4 if len(v) == 1 else v))
    arrays = {'gates': tab(1 << 20), 'c': tab(1 << 24), 'c_out': tab(1 << 25), 'gh': tab(1 << 26, 4),
              'gc': tab(1 << 27, 4), 'dz': tab(1 << 28), 'dzx': tab(1 << 29, 4), 'dh_in': tab(1 << 30, 4),
              'dc_in': tab(1 << 31, 4)}
    last = max(0, min(L, 4) * min(max(R, 1), 8) - 1)
    if null:
        arrays[null][last if len(arrays[null]) == 32 else 0] = None
    if odd:
        arrays[odd][0] = arrays[odd][0] + 8
    layers = i64(0, 1, 2, 3) if layer is None else i64(layer)
    need = 73728 * 4 if pack_bytes is None else pack_bytes
    a = arrays
    return lib.hrl_drc_bf16_step_backward(ctypes.c_void_p(pack), need, layers, L, R, H, a['gates'], a['c'], a['c_out'],
                                          a['gh'], i64(ghs), a['gc'], i64(gcs), N, a['dz'], a['dzx'], a['dh_in'],
                                          a['dc_in'], None)


@pytest.mark.parametrize('kw', [dict(L=0), dict(L=5), dict(R=0), dict(R=9), dict(H=16), dict(H=64), dict(null='gates'),
                                dict(null='c'), dict(null='c_out'), dict(null='dz'), dict(odd='gates'),
                                dict(odd='gh'), dict(odd='dzx'), dict(odd='dh_in'), dict(odd='dc_in'), dict(pack=4104),
                                dict(pack=0), dict(ghs=32 * 36 + 2), dict(gcs=32 * 36 + 1), dict(ghs=31 * 36),
                                dict(gcs=28 * 36), dict(pack_bytes=2 * 73728 - 16), dict(layer=4), dict(layer=-1),
                                dict(N=-1), dict(N=(1 << 24) + 1)],
                         ids=lambda kw: '%s=%s' % next(iter(kw.items())))
def test_backward_einval_returns_before_any_hip_call(kw):
    assert _backward(_native.load(), **kw) == EINVAL


def test_backward_of_no_rows_is_ok_and_null_options_are_valid():
    lib = _native.load()
    # gh, gc, dzx, dh_in, dc_in entries may be NULL ("zero" / "not wanted"); N = 0 launches nothing
    for null in (None, 'gh', 'gc', 'dzx', 'dh_in', 'dc_in'):
        assert _backward(lib, N=0, null=null) == _native.HRL_OK
    assert _backward(lib, N=0, R=9) == EINVAL      # validated all the same


def test_train_args_precision_rules():
    cpu, cuda = torch.device('cpu'), torch.device('cuda')
    assert 'bf16_drc_bwd' in hnn.LEARNER_PRECISIONS
    net = GeisterNet()
    assert hnn.configured_precision('bf16_drc_bwd', net, cuda) == net.body.step_precision == 'bf16_drc_bwd'
    assert hnn.configured_precision(None, net, cuda) == 'fp32' and net.body.step_precision == 'fp32'
    for other in (SimpleConv2dModel(), GeeseNet(layers=1)):
        with pytest.raises(ValueError, match='precision'):
            hnn.configured_precision('bf16_drc_bwd', other, cuda)
    with pytest.raises(ValueError, match='precision'):
        hnn.configured_precision('bf16_drc_bwd', GeisterNet(), cpu)
