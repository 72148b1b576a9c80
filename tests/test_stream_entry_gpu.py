"""The entry points with ``self_play: stream``: ``main.train_main`` and ``loop.SelfPlayTrainer(stream=True)``."""

import os

import pytest
import torch

from handyrl_amd.main import load_config, train_main

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(**kw):
    args = load_config(os.path.join(ROOT, 'config.yaml'))
    args['env_args']['env'] = 'TicTacToe'
    args['train_args'].update(update_episodes=16, minimum_episodes=32, maximum_episodes=64, batch_size=8,
                              forward_steps=6, epochs=2, self_play='stream', **kw)
    return args


def test_train_main_streams_two_epochs(cuda, tmp_path, monkeypatch):
    from handyrl_amd import main as hm
    built = []
    real = hm.StreamGenerator

    def spy(*a, **k):
        built.append(real(*a, **k))
        return built[-1]
    monkeypatch.setattr(hm, 'StreamGenerator', spy)
    logs = []
    model = train_main(_args(stream_slots=8), device=cuda, model_dir=str(tmp_path), log=logs.append)
    assert len(logs) == 2 and os.path.exists(tmp_path / '2.pth')
    for v in model.state_dict().values():
        assert torch.isfinite(v.float()).all()
    gen, = built
    assert gen.env.E == 8                         # stream_slots, not update_episodes
    # minimum_episodes in two or more calls, then one call per epoch, each of 16 games or more; the log counts
    # what was emitted
    assert gen._emitted >= 32 + 2 * 16 and gen.games_started == 8 + gen._emitted
    assert gen.replay.count == 64 and gen.replay.ptr == gen._emitted % 64
    assert ('episodes %d,' % gen._emitted) in logs[-1]


@pytest.mark.parametrize('kw,env', [({'observation': True}, 'TicTacToe'), ({'turn_based_training': False}, 'TicTacToe'),
                                    ({}, 'ParallelTicTacToe'), ({'generator': 'host'}, 'TicTacToe')])
def test_train_main_refuses_stream_outside_its_scope(cuda, tmp_path, kw, env):
    args = _args(**kw)
    args['env_args']['env'] = env
    with pytest.raises(ValueError, match='lockstep'):
        train_main(args, device=cuda, model_dir=str(tmp_path), log=lambda *_: None)
    assert not os.listdir(tmp_path)


def test_train_main_refuses_an_unknown_self_play(cuda, tmp_path):
    args = _args()
    args['train_args']['self_play'] = 'continuous'
    with pytest.raises(ValueError, match='self_play'):
        train_main(args, device=cuda, model_dir=str(tmp_path), log=lambda *_: None)


def test_selfplay_trainer_streams(cuda):
    from handyrl_amd.envs.tictactoe import SimpleConv2dModel
    from handyrl_amd.loop import SelfPlayTrainer
    from handyrl_amd.synthetic import default_args
    torch.manual_seed(0)
    net = SimpleConv2dModel().to(cuda)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    tr = SelfPlayTrainer(net, default_args(4, 64), cuda, games_per_round=128, capacity=512, graph=True, seed=3,
                         stream=True)
    tr.run(2, 3)
    torch.cuda.synchronize()
    assert tr.steps == 6 and tr.episodes >= 256 and tr.replay.count == min(tr.episodes, 512)
    assert tr.gen.games_started == 128 + tr.episodes
    after = net.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)
    for v in after.values():
        assert torch.isfinite(v.float()).all()
