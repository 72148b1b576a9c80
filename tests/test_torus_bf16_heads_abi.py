"""The mixed-precision tower's fused tail (hrl_torus_bf16_heads_*, train_args precision: bf16_heads): exports,
argument validation before any HIP call, and the option's rules in the Python layer (no GPU)."""

import ctypes

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.hungry_geese import GeeseNet
from handyrl_amd.envs.tictactoe import SimpleConv2dModel
from handyrl_amd.trainer import LearnerStep, split_torus_tower

ARGS = {'batch_size': 2, 'forward_steps': 2}
FWD = ('y', 'h_prev', 'alpha', 'beta', 'x', 'head_p', 'head_v', 'policy', 'value', 'pooled')
BWD = ('dpolicy', 'dvalue', 'value', 'pooled', 'head_p', 'head_v', 'x', 'y', 'h_prev', 'alpha', 'beta', 'mean', 'gm',
       'part', 'dhead_p', 'dhead_v', 'ws')
OPTIONAL = ('h_prev', 'dpolicy', 'dvalue')
ALIGNED = {'forward': ('y', 'h_prev', 'pooled'), 'backward': ('y', 'h_prev', 'gm', 'ws')}


def call(entry, N=5, H=7, W=11, x_stride=17 * 77, ws_short=0, **ptrs):
    """The entry on fake addresses (never dereferenced); ptrs overrides one pointer with None or an address."""
    lib = _native.load()
    names = FWD if entry == 'forward' else BWD
    p = {n: ctypes.c_void_p(ptrs[n]) if ptrs.get(n) else (None if n in ptrs else ctypes.c_void_p(4096 * (i + 1)))
         for i, n in enumerate(names)}
    if entry == 'forward':
        return lib.hrl_torus_bf16_heads_forward(p['y'], p['h_prev'], p['alpha'], p['beta'], p['x'], x_stride,
                                                p['head_p'], p['head_v'], N, H, W, p['policy'], p['value'],
                                                p['pooled'], None)
    size = max(lib.hrl_torus_bf16_heads_workspace_bytes(N), 0) - ws_short
    return lib.hrl_torus_bf16_heads_backward(p['dpolicy'], p['dvalue'], p['value'], p['pooled'], p['head_p'],
                                             p['head_v'], p['x'], x_stride, p['y'], p['h_prev'], p['alpha'], p['beta'],
                                             p['mean'], N, H, W, p['gm'], p['part'], p['dhead_p'], p['dhead_v'],
                                             p['ws'], size, None)


def test_exports_and_sizes():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    for name in ('hrl_torus_bf16_heads_forward', 'hrl_torus_bf16_heads_backward', 'hrl_torus_bf16_heads_workspace_bytes'):
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert [lib.hrl_torus_bf16_heads_workspace_bytes(n) for n in (-1, 0, 1, 9, 4097)] == [-1, 0, 1536, 3072, 512 * 1536]


@pytest.mark.parametrize('entry,names', [('forward', FWD), ('backward', BWD)])
def test_einval_before_any_hip_call_and_empty_batch(entry, names):
    EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK
    for name in names:
        if name in OPTIONAL:                     # NULL is a value: only the empty batch is safe to call without a GPU
            assert call(entry, N=0, **{name: None}) == OK, name
        else:
            assert call(entry, **{name: None}) == EINVAL and call(entry, N=0, **{name: None}) == EINVAL, name
    for name in ALIGNED[entry]:
        assert call(entry, **{name: 4104}) == EINVAL, name
    assert call(entry, H=9, W=9) == EINVAL and call(entry, H=0) == EINVAL        # 81 cells; no board
    assert call(entry, N=-1) == EINVAL and call(entry, x_stride=76) == EINVAL
    assert call(entry, N=0) == OK and call(entry, N=0, H=8, W=10) == OK
    if entry == 'backward':
        assert call(entry, ws_short=1) == EINVAL


def test_train_args_precision_rules():
    cpu, cuda = torch.device('cpu'), torch.device('cuda')
    with pytest.raises(ValueError, match='precision'):
        LearnerStep(SimpleConv2dModel(), dict(ARGS, precision='bf16_heads'), cpu)    # not a GeeseNet
    with pytest.raises(ValueError, match='precision'):
        LearnerStep(GeeseNet(layers=1), dict(ARGS, precision='bf16_heads'), cpu)     # not on the GPU
    biased = GeeseNet(layers=1)
    biased.head_p = torch.nn.Linear(32, 4, bias=True)
    for bad in (GeeseNet(filters=16), biased):                                       # outside the shape check; a bias
        with pytest.raises(ValueError, match='precision'):
            hnn.configured_precision('bf16_heads', bad, cuda)
    split = GeeseNet(layers=3)
    split_torus_tower(split)
    with pytest.raises(NotImplementedError, match='precision.*tower_split'):
        hnn.configured_precision('bf16_heads', split, cuda)
    net = GeeseNet(layers=1)                     # absent / fp32 / bf16: tests/test_torus_bf16_abi.py, unchanged
    assert LearnerStep(net, ARGS, cpu).precision == 'fp32' and not hasattr(net, 'tower_precision')
    assert hnn.configured_precision('bf16_heads', net, cuda) == 'bf16_heads' == net.tower_precision
    with pytest.raises(ValueError, match='torus_tower_heads'):
        hnn.torus_tower(torch.zeros(2, 17, 7, 11), [net.conv0, *net.blocks], precision='bf16_heads')
