"""The one-launch bf16 DRC repeat (csrc/hrl_drc_bf16.hip, train_args precision: bf16_drc): exports, argument validation
before any HIP call, and the option's rules in the Python layer (no GPU)."""

import ctypes

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.geister import GeisterNet
from handyrl_amd.envs.hungry_geese import GeeseNet
from handyrl_amd.envs.tictactoe import SimpleConv2dModel
from handyrl_amd.trainer import LearnerStep

EINVAL = _native.HRL_EINVAL
ARGS = {'batch_size': 2, 'forward_steps': 2}


def test_exports_and_pack_bytes():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    for name in ('hrl_drc_bf16_pack_bytes', 'hrl_drc_bf16_pack', 'hrl_drc_bf16_repeat_forward'):
        assert name in _native.SIGNATURES and getattr(lib, name)
    # L * 8 column tiles * 9 taps * 64 lanes * 16 B
    assert [lib.hrl_drc_bf16_pack_bytes(L) for L in (0, 1, 3, 4, 5)] == [0, 73728, 221184, 294912, 0]


def _repeat(lib, L=3, H=32, N=17, zxs=128 * 36, hs=32 * 36, cs=32 * 36, pack_bytes=None, null=False, pack=4096):
    """hrl_drc_bf16_repeat_forward on made-up pointers (not device memory: a launch would fault)."""
    tab = lambda base: (ctypes.c_void_p * 4)(*[base + 65536 * i for i in range(4)])
    h_in = tab(1 << 24)
    if null:
        h_in[max(0, min(L, 4) - 1)] = None
    i64 = lambda v: (ctypes.c_int64 * 4)(v, v, v, v)
    need = 73728 * L if pack_bytes is None else pack_bytes
    return lib.hrl_drc_bf16_repeat_forward(ctypes.c_void_p(pack), need, L, H, tab(1 << 20), i64(zxs), h_in, i64(hs),
                                           tab(1 << 25), i64(cs), N, tab(1 << 26), tab(1 << 27), None, None)


@pytest.mark.parametrize('kw', [dict(H=16), dict(H=64), dict(L=0), dict(L=5), dict(zxs=128 * 36 + 2),
                                dict(hs=32 * 36 + 1), dict(cs=32 * 36 + 3), dict(zxs=127 * 36), dict(hs=31 * 36),
                                dict(pack_bytes=3 * 73728 - 16), dict(null=True), dict(pack=4104), dict(N=-1)],
                         ids=lambda kw: '%s=%s' % next(iter(kw.items())))
def test_repeat_einval_returns_before_any_hip_call(kw):
    assert _repeat(_native.load(), **kw) == EINVAL


def test_repeat_of_no_rows_is_ok():
    assert _repeat(_native.load(), N=0) == _native.HRL_OK
    assert _repeat(_native.load(), N=0, H=16) == EINVAL      # validated all the same


@pytest.mark.parametrize('kind', ['layers', 'null', 'align', 'bytes', 'slice'])
def test_pack_einval_returns_before_any_hip_call(kind):
    ws = (ctypes.c_void_p * 3)(4096, 8192, None if kind == 'null' else 12288)
    assert _native.load().hrl_drc_bf16_pack(
        ws, 5 if kind == 'layers' else 3, 64, 33 if kind == 'slice' else 32,
        ctypes.c_void_p(65544 if kind == 'align' else 65536), 3 * 73728 - (1 if kind == 'bytes' else 0), None) == EINVAL


def test_train_args_precision_rules():
    cpu, cuda = torch.device('cpu'), torch.device('cuda')
    assert 'bf16_drc' in hnn.LEARNER_PRECISIONS
    net = GeisterNet()
    assert LearnerStep(net, ARGS, cpu).precision == 'fp32' and 'step_precision' not in vars(net.body)   # absent: nothing set
    assert hnn.configured_precision('bf16_drc', net, cuda) == 'bf16_drc' and net.body.step_precision == 'bf16_drc'
    assert hnn.configured_precision(None, net, cuda) == 'fp32' and net.body.step_precision == 'fp32'
    for other in (SimpleConv2dModel(), GeeseNet(layers=1)):
        with pytest.raises(ValueError, match='precision'):
            hnn.configured_precision('bf16_drc', other, cuda)
    with pytest.raises(ValueError, match='precision'):
        LearnerStep(GeisterNet(), dict(ARGS, precision='bf16_drc'), cpu)
    with pytest.raises(ValueError, match='precision'):
        hnn.configured_precision('bf16', GeisterNet(), cuda)       # the tower's values stay GeeseNet's
    with pytest.raises(ValueError, match='precision'):
        hnn.drc_step([], [], [], [], (32, 64), (1, 1), None, 1, precision='bf16')

