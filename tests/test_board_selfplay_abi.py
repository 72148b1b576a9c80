"""Whole TicTacToe self-play games in one launch (csrc/hrl_boardplay.hip, ``DeviceGenerator(fused_game=True)``):
the export, its argument validation (before any HIP call, on fake pointers) and the Python layer off the GPU."""

import ctypes

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.loop import SelfPlayTrainer
from handyrl_amd.rollout import DeviceGenerator, ParallelTicTacToeBatch, TicTacToeBatch

from . import board_infer_util as util
from .test_board_infer_rollout import _equal_tree
from .test_main_entry import _oracle_loss, _small

EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK
PTRS = ('pack', 'U', 'board', 'color', 'nmoves', 'winner', 'obs', 'policy', 'amask', 'action', 'value', 'turn')


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def _play(null=(), layers=3, E=0, Tm=9, t0=0, t1=9, pack=None):
    a = {n: None if n in null else _p(i) for i, n in enumerate(PTRS)}
    if pack is not None:
        a['pack'] = ctypes.c_void_p(pack)
    return _native.load().hrl_board_selfplay(a['pack'], layers, E, Tm, t0, t1, a['U'], a['board'], a['color'],
                                             a['nmoves'], a['winner'], a['obs'], a['policy'], a['amask'],
                                             a['action'], a['value'], a['turn'], None)


def test_export_and_abi_version():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    assert 'hrl_board_selfplay' in _native.SIGNATURES and hasattr(lib, 'hrl_board_selfplay')


def test_entry_validates_arguments():
    # nothing to play: OK without a launch (the pointers are fake)
    assert _play(E=0) == OK
    assert _play(E=5, t0=4, t1=4) == OK
    assert _play(E=5, t0=0, t1=0) == OK
    assert _play(E=5, Tm=1, t0=1, t1=1) == OK
    for name in PTRS:
        assert _play(null=(name,), E=5) == EINVAL, name
    for kw in ({'layers': 0}, {'layers': 9}, {'pack': 4096 + 8}, {'pack': 4096 + 4}, {'E': -1}, {'Tm': 0, 't1': 0},
               {'Tm': 10, 't1': 10}, {'t0': -1}, {'Tm': 9, 't1': 10}, {'Tm': 5, 't1': 6}, {'t0': 5, 't1': 4}):
        assert _play(**{'E': 5, **kw}) == EINVAL, kw
        assert _play(**{'E': 0, **kw}) == EINVAL, kw        # validated before the E == 0 return


def test_generator_option_refuses_what_it_cannot_play():
    cpu = torch.device('cpu')
    net = util.seeded_net(3)
    wrapped = hnn.BoardInference(net)
    with pytest.raises(ValueError, match='fused_game'):
        DeviceGenerator(ParallelTicTacToeBatch(4, cpu), wrapped, fused_game=True)
    with pytest.raises(ValueError, match='fused_game'):
        DeviceGenerator(TicTacToeBatch(4, cpu), wrapped, observation=True, fused_game=True)
    with pytest.raises(ValueError, match='fused_game'):
        DeviceGenerator(TicTacToeBatch(4, cpu), wrapped, per_player=True, fused_game=True)
    with pytest.raises(ValueError, match='fused_game'):
        DeviceGenerator(TicTacToeBatch(4, cpu), net, fused_game=True)
    # a group member is accepted (it plays from its row of the group's buffer); the option off takes anything
    DeviceGenerator(TicTacToeBatch(4, cpu), hnn.board_inference_group([net, util.seeded_net(3, 1)])[1],
                    fused_game=True)
    DeviceGenerator(ParallelTicTacToeBatch(4, cpu), net)


def test_trainer_option_requires_fused_inference_and_lockstep():
    cpu = torch.device('cpu')
    args = _small()['train_args']
    with pytest.raises(ValueError, match='fused_game'):
        SelfPlayTrainer(util.seeded_net(3), args, cpu, games_per_round=8, capacity=16, fused_game=True)
    with pytest.raises(ValueError, match='fused_game'):
        SelfPlayTrainer(util.seeded_net(3), args, cpu, games_per_round=8, capacity=16, fused_inference=True,
                        stream=True, fused_game=True)


def test_self_play_key_raises_by_name_off_the_gpu(tmp_path):
    from handyrl_amd.main import train_main
    for value in ('fused', 'quick'):
        args = _small()
        args['train_args'].update(self_play=value, epochs=1)
        with pytest.raises(ValueError, match='self_play'):
            train_main(args, device=torch.device('cpu'), loss_fn=_oracle_loss, model_dir=str(tmp_path),
                       log=lambda *_: None)


def test_cpu_generator_with_the_option_equals_plain():
    cpu = torch.device('cpu')
    net = util.seeded_net(3)
    eps = []
    for fused in (False, True):
        gen = DeviceGenerator(TicTacToeBatch(16, cpu), hnn.BoardInference(net), fused_game=fused)
        eps.append(gen.generate(generator=torch.Generator().manual_seed(3)))
    _equal_tree(eps[0], eps[1])
    assert int(eps[0]['length'].min()) >= 5
