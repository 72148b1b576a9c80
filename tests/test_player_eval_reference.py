"""PlayerEvaluator against the reference's own matches (tests/golden/geese_eval.*, written by
tests/golden/make_geese_eval_golden.py from the reference's ``exec_match``, ``Agent``, ``RandomAgent`` and
``ModelWrapper`` over this project's host Hungry Geese env): eight games of one greedy net against three random agents
and eight of net A against net B on the three other seats, game g being Geese game number g under the stored seed.

The recorded moves are replayed through ``forced`` with ``trace=True``.  Outcomes, lengths and actions are exact; the
traced policy of every net seat agrees with the reference's raw policy within 1e-5 (the project's self-play bound);
``picked`` -- the evaluator's own decision, also where a move was forced -- is the reference agent's own choice
wherever the fixture's top-two margin is at least 1e-4, and within 1e-4 of the maximum elsewhere.  The share of net
plies under the margin is a condition of the fixture (at most 5% per set), asserted by the maker and again here.
"""

import json
import os

import numpy as np
import pytest
import torch

from handyrl_amd.envs.geese import GeeseNet, HungryGeeseBatch
from handyrl_amd.evaluation import PlayerEvaluator, wp_func

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
META = json.load(open(os.path.join(HERE, 'geese_eval.json')))
DATA = np.load(os.path.join(HERE, 'geese_eval.npz'))
TOL, MARGIN = 1e-5, 1e-4
DEVICES = ['cpu', pytest.param('cuda-eager', marks=pytest.mark.gpu), pytest.param('cuda-graph', marks=pytest.mark.gpu)]


def test_the_fixture_meets_its_condition():
    assert META['margin'] == MARGIN and META['max_share_under_margin'] == 0.05
    assert META['torch_seeds'][0] >= META['first_torch_seed_tried'] == 7
    for key, m in META['sets'].items():
        assert m['games'] == 8 and m['net_plies'] > 0
        assert m['net_plies_under_margin'] <= 0.05 * m['net_plies'], key
        # the counts are the arrays' own
        alive, pol = DATA[key + '_alive'].astype(bool), DATA[key + '_policy']
        net = alive & (DATA[key + '_choice'] >= 0)
        top = np.sort(pol[net], axis=-1)
        assert int(net.sum()) == m['net_plies']
        assert int((top[:, -1] - top[:, -2] < MARGIN).sum()) == m['net_plies_under_margin']
        assert [int(a.any(-1).sum()) for a in alive] == m['length']


def _nets(dev):
    nets = []
    for seed in META['torch_seeds']:
        torch.manual_seed(seed)
        net = GeeseNet()
        net.eval()
        if dev.type == 'cuda':
            from handyrl_amd.nn import accelerate
            gpu = accelerate(GeeseNet().to(dev))
            gpu.load_state_dict(net.state_dict())
            net = gpu
        nets.append(net)
    return nets


@pytest.mark.parametrize('key', ['random', 'match'])
@pytest.mark.parametrize('where', DEVICES)
def test_replayed_reference_games(request, where, key):
    dev = torch.device('cpu') if where == 'cpu' else request.getfixturevalue('cuda')
    m = META['sets'][key]
    G, P = m['games'], 4
    alive = torch.from_numpy(DATA[key + '_alive'].astype(bool))
    action = torch.from_numpy(DATA[key + '_action'].astype(np.int64))
    choice = torch.from_numpy(DATA[key + '_choice'].astype(np.int64))
    policy = torch.from_numpy(DATA[key + '_policy'])
    T = alive.shape[1]
    a, b = _nets(dev)
    env = HungryGeeseBatch(G, dev)
    env.seed(META['env_seed'])
    ev = PlayerEvaluator(env, a, seed=99, graph=where == 'cuda-graph', opponent=b if key == 'match' else None)
    res = ev.evaluate(G, forced=action, trace=True)
    tr = {k: v.cpu()[:, :T] for k, v in res['trace'].items()}
    assert res['length'].tolist() == m['length']
    assert torch.equal(res['outcome'].cpu(), torch.from_numpy(DATA[key + '_outcome']))
    assert torch.equal(tr['alive'], alive) and torch.equal(tr['action'], action)
    assert not bool(res['trace']['alive'][:, T:].any())
    mine = [float(DATA[key + '_outcome'][g, g % P]) for g in range(G)]
    assert res['win_rate'] == wp_func({o: mine.count(o) for o in sorted(set(mine), reverse=True)})
    net = alive & (choice >= 0)
    assert bool((tr['picked'][~alive] == -1).all())
    assert float((tr['policy'][net] - policy[net]).abs().max()) <= TOL
    assert not bool(tr['policy'][~net].any())
    top = policy[net].sort(-1).values
    clear = top[:, -1] - top[:, -2] >= MARGIN
    picked, want = tr['picked'][net], choice[net]
    assert torch.equal(picked[clear], want[clear])
    near = policy[net].gather(1, picked.view(-1, 1)).view(-1)
    assert bool((near[~clear] >= top[~clear, -1] - MARGIN).all())
    if key == 'random':      # the random seats' own picks are legal labels; their recorded moves were played
        rnd = alive & (choice < 0)
        assert int(rnd.sum()) > 0 and bool(((tr['picked'][rnd] >= 0) & (tr['picked'][rnd] < 4)).all())
