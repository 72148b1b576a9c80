"""The mixed-precision GeeseNet tower (csrc/hrl_torus_bf16.hip, train_args precision: bf16): exports, argument
validation before any HIP call, and the option's rules in the Python layer (no GPU)."""

import ctypes

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.hungry_geese import GeeseNet
from handyrl_amd.envs.tictactoe import SimpleConv2dModel
from handyrl_amd.trainer import LearnerStep, split_torus_tower

EINVAL = _native.HRL_EINVAL
ENTRIES = ('hrl_torus_bf16_pack_bytes', 'hrl_torus_bf16_workspace_bytes', 'hrl_torus_bf16_stats_blocks',
           'hrl_torus_bf16_pack', 'hrl_torus_bf16_unit_forward', 'hrl_torus_bf16_output',
           'hrl_torus_bf16_masked_sums', 'hrl_torus_bf16_wgrad_bn', 'hrl_torus_bf16_unit_input_grad')
ARGS = {'batch_size': 2, 'forward_steps': 2}


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def test_exports_and_sizes():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    for name in ENTRIES:
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert [lib.hrl_torus_bf16_pack_bytes(u) for u in (0, 18, 1, 13)] == [-1, -1, 36864, 13 * 36864]
    assert [lib.hrl_torus_bf16_stats_blocks(n) for n in (0, 1, 9, 4096, 4097)] == [-1, 1, 2, 512, 512]
    assert lib.hrl_torus_bf16_workspace_bytes(0) == -1 and lib.hrl_torus_bf16_workspace_bytes(1025) == 256 * 9248 * 4


# every call below is complete but for one argument; the pointers are not device memory, so a launch would fault
CALLS = {
    'pack': lambda lib, k: lib.hrl_torus_bf16_pack(
        (ctypes.c_void_p * 2)(4096, None if k == 'null' else 8192), 2, 16 if k == 'cin' else 17,
        _p(3) if k != 'align' else ctypes.c_void_p(4104), 0 if k == 'bytes' else 2 * 36864, None),
    'stem': lambda lib, k: lib.hrl_torus_bf16_unit_forward(
        _p(0), _p(1) if k == 'null' else None, None, None, None, None, -1 if k == 'bytes' else 5, 7,
        12 if k == 'cin' else 11, _p(2), 0, _p(3), _p(4) if k != 'align' else ctypes.c_void_p(4104), _p(5), None),
    'unit': lambda lib, k: lib.hrl_torus_bf16_unit_forward(
        None, _p(1), None, None if k == 'null' else _p(2), _p(3), _p(4) if k != 'align' else ctypes.c_void_p(4104),
        5, 7, 11, _p(5), 0 if k == 'cin' else 17 if k == 'bytes' else 1, _p(6), _p(7), _p(8), None),
    'output': lambda lib, k: lib.hrl_torus_bf16_output(
        _p(0) if k != 'align' else ctypes.c_void_p(4104), None, _p(1), _p(2), 0 if k == 'bytes' else 5,
        9 if k == 'cin' else 7, 11, None if k == 'null' else _p(3), None),
    'sums': lambda lib, k: lib.hrl_torus_bf16_masked_sums(
        _p(0), _p(1), _p(2) if k != 'align' else ctypes.c_void_p(4104), _p(3), 0 if k == 'bytes' else 5,
        9 if k == 'cin' else 7, 11, _p(4), None if k == 'null' else _p(5), None),
    'wgrad': lambda lib, k: lib.hrl_torus_bf16_wgrad_bn(
        _p(9) if k == 'cin' else None, _p(0), 5, 7, 11, _p(1) if k != 'align' else ctypes.c_void_p(4104), _p(2), 0,
        _p(3), _p(4), 1, _p(5), _p(6), _p(7), _p(8), None if k == 'null' else _p(10), _p(11), _p(12), _p(13), _p(14),
        0 if k == 'bytes' else 1 << 30, None),
    'adjoint': lambda lib, k: lib.hrl_torus_bf16_unit_input_grad(
        _p(0) if k != 'align' else ctypes.c_void_p(4104), 0 if k == 'bytes' else 5, 7, 11, _p(1), 0 if k == 'cin' else 1,
        _p(2), 0, None if k == 'null' else _p(3), _p(4), _p(5), _p(6), _p(7), _p(8), None),
}


@pytest.mark.parametrize('kind', ['null', 'align', 'bytes', 'cin'])
@pytest.mark.parametrize('entry', sorted(CALLS))
def test_einval_returns_before_any_hip_call(entry, kind):
    assert CALLS[entry](_native.load(), kind) == EINVAL


def test_torus_tower_validates_precision_before_any_work():
    units = [u for u in GeeseNet(layers=2).modules() if hasattr(u, 'edge_size')]
    x = torch.zeros(2, 17, 7, 11)
    with pytest.raises(ValueError, match='precision'):
        hnn.torus_tower(x, units, precision='fp16')
    units[0].tower_split = 2
    with pytest.raises(NotImplementedError, match='bf16.*tower_split'):
        hnn.torus_tower(x, units, precision='bf16')


def test_train_args_precision_rules():
    cpu, cuda = torch.device('cpu'), torch.device('cuda')
    with pytest.raises(ValueError, match='precision'):
        LearnerStep(SimpleConv2dModel(), dict(ARGS, precision='bf16'), cpu)          # not a GeeseNet
    with pytest.raises(ValueError, match='precision'):
        LearnerStep(GeeseNet(layers=1), dict(ARGS, precision='bf16'), cpu)           # not on the GPU
    with pytest.raises(ValueError, match='precision'):
        LearnerStep(GeeseNet(layers=1), dict(ARGS, precision='fp16'), cpu)           # not a value
    with pytest.raises(ValueError, match='precision'):
        hnn.configured_precision('bf16', GeeseNet(filters=16), cuda)                 # outside the shape check
    split = GeeseNet(layers=3)
    split_torus_tower(split)
    with pytest.raises(NotImplementedError, match='precision.*tower_split'):
        hnn.configured_precision('bf16', split, cuda)
    net = GeeseNet(layers=1)
    assert hnn.configured_precision('bf16', net, cuda) == 'bf16' and net.tower_precision == 'bf16'
    assert hnn.configured_precision(None, net, cuda) == 'fp32' and net.tower_precision == 'fp32'


@pytest.mark.parametrize('args', [ARGS, dict(ARGS, precision='fp32')])
def test_fp32_or_absent_is_the_existing_path(args, monkeypatch):
    net = GeeseNet(layers=1)
    assert LearnerStep(net, args, torch.device('cpu')).precision == 'fp32' and not hasattr(net, 'tower_precision')
    seen = []
    monkeypatch.setattr(hnn, '_tower_part', lambda x, units, residual_in, function=None: seen.append(function))
    hnn.torus_tower(torch.zeros(1, 17, 7, 11), [net.conv0, *net.blocks], getattr(net, 'tower_precision', 'fp32'))
    assert seen == [None]                                       # _TorusTower, not the bf16 Function
