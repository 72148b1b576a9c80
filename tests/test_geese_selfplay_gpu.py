"""Device self-play of Hungry Geese: ``DeviceGenerator`` over ``HungryGeeseBatch`` and GeeseNet, refereed by the
Python rules, then the replay and the entry point.  A seeded-init net plays nearly uniformly, so the games are
short; the long-game clauses are tests/test_geese_kernels_gpu.py's."""

import os
import random

import numpy as np
import pytest
import torch

from handyrl_amd.envs import geese
from handyrl_amd.envs.geese import GeeseNet, HungryGeeseBatch
from handyrl_amd.rollout import DeviceGenerator, PlayerReplay, player_episodes_to_wire

pytestmark = pytest.mark.gpu

E, KEY, BASE = 32, 3, 1000


@pytest.fixture(scope='module')
def runs(cuda):
    """With the graph and without: a first call (which captures), then a call on games BASE .. BASE + E - 1 with the
    same uniforms.  {graph: (games of the first call, second episodes, games of the second call)}, and the net."""
    from handyrl_amd.nn import accelerate
    torch.manual_seed(0)
    net = accelerate(GeeseNet().to(cuda))
    out = {}
    for graph in (True, False):
        env = HungryGeeseBatch(E, cuda, seed=KEY)
        gen = DeviceGenerator(env, net, gamma=0.8, graph=graph)
        gen.generate(generator=torch.Generator(device=cuda).manual_seed(1))
        first = env.game.cpu().tolist()
        env.next_game = BASE
        ep = gen.generate(generator=torch.Generator(device=cuda).manual_seed(2))
        out[graph] = (first, {k: v.cpu() for k, v in ep.items()}, env.game.cpu().tolist())
    return net, out


def test_graph_and_eager_play_the_same_episodes(runs):
    _, out = runs
    with_graph, eager = out[True][1], out[False][1]
    assert set(with_graph) == set(eager)
    for k in with_graph:
        assert torch.equal(with_graph[k], eager[k]), k
    assert int(with_graph['length'].max()) > 1


def test_successive_calls_play_new_games(runs):
    _, out = runs
    first, _, second = out[False]
    # the constructor's reset took games 0 .. E - 1; every reset after it takes the next E (a capture resets twice)
    assert first == list(range(E, 2 * E)) and second == list(range(BASE, BASE + E))
    first_graph, _, second_graph = out[True]
    assert first_graph == list(range(2 * E, 3 * E)) and second_graph == second


def test_every_episode_is_a_game_of_the_rules(runs):
    net, out = runs
    ep = out[True][1]
    obs, tmask, omask, action = ep['observation'].numpy(), ep['tmask'].numpy(), ep['omask'].numpy(), ep['action']
    rows = []
    for e in range(E):
        st = geese.new_game(KEY, BASE + e)
        L = int(ep['length'][e])
        for t in range(L):
            turns = geese.turns_of(st)
            assert turns and tmask[e, t].tolist() == omask[e, t].tolist() == [p in turns for p in range(4)], (e, t)
            for p in range(4):
                want = geese.observation_of(st, p) if p in turns else np.zeros((17, 7, 11), np.float32)
                assert np.array_equal(obs[e, t, p], want), (e, t, p)
                if p in turns:
                    rows.append((e, t, p))
            geese.step_game(st, action[e, t].tolist(), KEY)
        assert not st['live'] and st['step'] == L, e
        assert not tmask[e, L:].any() and not omask[e, L:].any() and not obs[e, L:].any(), e
        assert ep['outcome'][e].tolist() == [float(np.float32(x)) for x in geese.outcome_of(st)], e
    # the recorded policies and values are the net's on the recorded observations (a CPU forward)
    cpu = GeeseNet()
    cpu.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    cpu.eval()
    idx = tuple(torch.tensor(x) for x in zip(*rows))
    with torch.no_grad():
        want = cpu(ep['observation'][idx])
    assert len(rows) > 4 * E
    torch.testing.assert_close(ep['policy'][idx], want['policy'], rtol=0, atol=1e-5)
    torch.testing.assert_close(ep['value'][idx], want['value'].view(-1), rtol=0, atol=1e-5)
    assert bool((ep['action_mask'][idx] == 0).all())


def test_solo_replay_windows_equal_make_batch(runs, cuda):
    from handyrl_amd.batch import make_batch
    ep = runs[1][True][1]
    T, B = 8, 20
    rep = PlayerReplay(E, geese.MAX_PLIES, (17, 7, 11), 4, 4, cuda, obs_dtype=torch.uint8, solo=True)
    rep.add({k: v.to(cuda) for k, v in ep.items()})
    slots, start = rep.sample_windows(B, T, generator=torch.Generator(device=cuda).manual_seed(1))
    random.seed(5)
    players = torch.tensor([random.choice([0, 1, 2, 3]) for _ in range(B)])
    random.seed(5)
    wire = player_episodes_to_wire(ep)
    windows = []
    for s, st in zip(slots.tolist(), start.tolist()):
        e = wire[s]
        windows.append({'args': {}, 'outcome': e['outcome'], 'moment': e['moment'], 'base': 0, 'start': st,
                        'end': min(st + T, e['steps']), 'total': e['steps']})
    ref = make_batch(windows, {'turn_based_training': False, 'observation': False, 'forward_steps': T})
    batch = rep.gather(slots, start, T, players.to(cuda))
    for k, v in ref.items():
        got = batch[k].cpu()
        assert got.shape == v.shape and got.dtype == v.dtype, (k, got.shape, v.shape, got.dtype, v.dtype)
        np.testing.assert_array_equal(got.numpy(), v.numpy(), err_msg=k)


def test_train_main_trains_geese_on_the_device(cuda, tmp_path):
    from handyrl_amd.main import train_main
    args = {'env_args': {'env': 'Geese'},
            'train_args': {'turn_based_training': False, 'observation': False, 'update_episodes': 16,
                           'minimum_episodes': 16, 'maximum_episodes': 64, 'batch_size': 8, 'forward_steps': 8,
                           'epochs': 2, 'seed': 4}}
    logs = []
    model = train_main(args, device=cuda, model_dir=str(tmp_path), log=logs.append)
    assert os.path.isfile(os.path.join(str(tmp_path), '2.pth')) and len(logs) == 2
    torch.manual_seed(4)
    fresh = GeeseNet().state_dict()
    assert any(not torch.equal(v.cpu(), fresh[k]) for k, v in model.state_dict().items() if 'weight' in k)
    with pytest.raises(ValueError, match='alternating-move envs'):
        args['train_args']['eval_rate'] = 0.5
        train_main(args, device=cuda, model_dir=str(tmp_path / 'eval'), log=logs.append)
