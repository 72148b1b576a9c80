"""nn.GeeseInference where the project plays Hungry Geese on the GPU: ``PlayerEvaluator`` (against random agents and
against the rule-based geese), ``PlayerStreamGenerator`` and ``main --eval`` with ``inference: fused`` play the games
the module-by-module forward plays.

The two forwards agree to the last bits, not bit for bit, so a greedy or sampled move could differ only at a
near-tie; with the seeds below none does (no seed was changed to get there)."""

import copy

import pytest
import torch

from handyrl_amd import nn as hnn
from handyrl_amd.envs.geese import GeeseNet, HungryGeeseBatch
from handyrl_amd.evaluation import PlayerEvaluator, eval_main
from handyrl_amd.rollout import PlayerReplay, PlayerStreamGenerator
from tests.test_player_eval_entry import _args
from tests.test_player_eval_rollout import SEED
from tests.test_player_stream_rollout import ring_rows

pytestmark = pytest.mark.gpu

E, G = 8, 24


def _net(cuda, seed=11):
    torch.manual_seed(seed)
    return hnn.accelerate(GeeseNet().to(cuda)).eval()


@pytest.mark.parametrize('kw', [{}, {'opponent': 'rule'}], ids=['random', 'rule'])
def test_evaluator_plays_the_same_games(cuda, kw):
    net = _net(cuda)
    res = []
    for n in (net, hnn.GeeseInference(net)):
        b = HungryGeeseBatch(E, cuda)
        b.seed(SEED)
        res.append(PlayerEvaluator(b, n, seed=SEED, **kw).evaluate(G))
    plain, fused = res
    assert plain['games'] == fused['games'] == G
    assert torch.equal(plain['outcome'].cpu(), fused['outcome'].cpu())
    assert torch.equal(plain['length'].cpu(), fused['length'].cpu())
    assert plain['results'] == fused['results'] and plain['win_rate'] == fused['win_rate']
    assert int(plain['length'].max()) > 1


def test_stream_generator_plays_the_same_episodes(cuda):
    net = _net(cuda)
    N = 32
    recs = []
    for n in (net, hnn.GeeseInference(net)):
        env = HungryGeeseBatch(E, cuda, seed=5)
        replay = PlayerReplay(N, env.MAX_PLIES, env.OBS_SHAPE, env.A, env.P, cuda, obs_dtype=torch.uint8)
        gen = PlayerStreamGenerator(env, n, replay, gamma=0.8, seed=5)
        gen.generate(N)
        recs.append(ring_rows(replay, gen, list(range(N))))
    plain, fused = recs
    for k in ('game', 'action', 'outcome', 'length', 'obs', 'amask', 'tmask', 'omask', 'reward'):
        assert torch.equal(plain[k], fused[k]), k
    assert int(plain['length'].max()) > 1 and int((plain['game'] >= 0).sum()) == N
    for k in ('policy', 'value', 'ret'):
        torch.testing.assert_close(fused[k], plain[k], rtol=0, atol=1e-5, msg=k)


def test_train_main_with_fused_inference(cuda, tmp_path, monkeypatch):
    """``inference: fused`` with ``env: Geese``: self-play runs through the wrapper, the learner trains the net."""
    import os
    from handyrl_amd.main import train_main
    made = []
    real = hnn.GeeseInference.__init__
    monkeypatch.setattr(hnn.GeeseInference, '__init__', lambda self, net: (made.append(1), real(self, net))[1])
    args = _args(inference='fused', epochs=1, update_episodes=16, minimum_episodes=16, maximum_episodes=64,
                 batch_size=8, forward_steps=8, seed=4)
    logs = []
    model = train_main(args, device=cuda, model_dir=str(tmp_path), log=logs.append)
    assert os.path.isfile(os.path.join(str(tmp_path), '1.pth')) and len(logs) == 1 and len(made) == 1
    torch.manual_seed(4)
    fresh = GeeseNet().state_dict()
    state = model.state_dict()
    assert list(state) == list(fresh)
    assert all(torch.isfinite(v.float()).all() for v in state.values())
    assert any(not torch.equal(v.cpu(), fresh[k]) for k, v in state.items() if 'weight' in k)


def test_eval_entry_with_fused_inference_prints_the_same_line(cuda, tmp_path, monkeypatch):
    torch.manual_seed(4)
    torch.save(GeeseNet().state_dict(), tmp_path / 'a.pth')
    made = []
    real = hnn.GeeseInference.__init__
    monkeypatch.setattr(hnn.GeeseInference, '__init__', lambda self, net: (made.append(1), real(self, net))[1])
    lines = []
    for kw in ({}, {'inference': 'fused'}):
        logs = []
        res = eval_main(_args(**kw), [str(tmp_path / 'a.pth'), str(G), str(E)], device=cuda, log=logs.append)
        assert res['games'] == G and logs[-1].startswith('total ')
        lines.append(logs[-1])
    assert lines[0] == lines[1]
    assert len(made) == 1                                      # only the run with the key wrapped its net
