"""Reference parity of a match: games the reference's ``exec_match`` played with one greedy ``Agent`` per net
(tests/golden/match.*, written by tests/golden/make_match_golden.py) are replayed move for move through ``forced``
and the evaluator's own decisions are compared with the reference's.

Nets A and B are the env's seeded ``env.net()()`` (the fixture holds the two torch seeds); A sits on seat g mod 2.
The first k plies of a fixture game were replaced by Python ``random`` moves, so they are given, not compared: the
evaluator runs with ``opening_plies=0`` and its ``picked`` is the mover's net's argmax at every ply.  Past the opening
it is compared with the reference's move wherever the fixture's top-two margin is at least 1e-4 -- the net tolerance
is 1e-5, so above that margin the argmax cannot flip -- and must be a label within 1e-4 of the fixture maximum
elsewhere (opening plies and plies under the margin).
"""

import json
import os

import numpy as np
import pytest
import torch

from handyrl_amd.environment import make_env
from handyrl_amd.evaluation import DeviceEvaluator, batched_env, wp_func

SETS = ('tictactoe', 'geister', 'geister_obs')
MODES = [('cpu', None), pytest.param('cuda', False, marks=pytest.mark.gpu),
         pytest.param('cuda', True, marks=pytest.mark.gpu)]
MARGIN = 1e-4


@pytest.fixture(scope='module')
def golden():
    base = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'match')
    with open(base + '.json') as f:
        meta = json.load(f)
    return meta, np.load(base + '.npz')


def _nets(env_name, seeds, dev):
    env = make_env({'env': env_name})
    nets = []
    for seed in seeds:
        torch.manual_seed(seed)
        net = env.net()()
        if dev.type == 'cuda':
            from handyrl_amd.nn import accelerate
            net = accelerate(net.to(dev))
        nets.append(net)
    return type(env).__module__, nets


@pytest.mark.parametrize('device,graph', MODES)
@pytest.mark.parametrize('key', SETS)
def test_reference_matches_replayed(request, golden, key, device, graph):
    meta, arrays = golden
    dev = request.getfixturevalue('cuda') if device == 'cuda' else torch.device('cpu')
    info = meta['sets'][key]
    assert meta['margin'] == MARGIN
    G, lengths, opening = info['games'], info['length'], info['opening']
    mover, action = arrays[key + '_mover'], arrays[key + '_action'].astype(np.int64)
    ref_policy, outcome = arrays[key + '_policy'], arrays[key + '_outcome']
    assert len(ref_policy) == info['plies'] == sum(lengths)
    assert info['plies_under_margin'] <= 0.05 * info['plies']
    module, (home, opp) = _nets(info['env'], meta['torch_seeds'], dev)
    cls = batched_env(module)
    state = torch.get_rng_state()
    ev = DeviceEvaluator(cls(max(1, G - 1), dev), home, observation=info['observation'], seed=5, graph=graph,
                         opponent=opp)
    res = ev.evaluate(G, forced=torch.from_numpy(action), trace=True)
    assert torch.equal(torch.get_rng_state(), state)
    tr = {k: v.cpu().numpy() for k, v in res['trace'].items()}
    # outcomes and lengths: exact
    assert res['length'].tolist() == lengths
    assert np.array_equal(res['outcome'].cpu().numpy(), outcome)
    assert res['seat'].tolist() == [g % 2 for g in range(G)]
    close, worst, row = 0, 0.0, 0
    for g in range(G):
        L = lengths[g]
        assert np.array_equal(tr['action'][g, :L], action[g, :L]) and (tr['action'][g, L:] == -1).all()
        assert np.array_equal(tr['model_ply'][g, :L], mover[g, :L] == g % 2)      # net A sits on seat g mod 2
        for t in range(L):
            p, p_ref = tr['policy'][g, t], ref_policy[row]
            row += 1
            legal = p > -1e31
            d = float(np.abs(p[legal] - p_ref[legal]).max())
            worst = max(worst, d)
            assert d <= 1e-5, (key, g, t, d)
            top = np.sort(p_ref[legal])[::-1]
            picked = int(tr['picked'][g, t])
            assert legal[picked], (key, g, t)
            under = len(top) > 1 and top[0] - top[1] < MARGIN
            close += under
            if t >= opening[g] and not under:
                assert picked == int(action[g, t]), (key, g, t, float(top[0] - top[1]) if len(top) > 1 else None)
            else:
                assert p_ref[picked] >= top[0] - MARGIN, (key, g, t)
    assert close == info['plies_under_margin']
    print('%s on %s: max |policy - fixture| %.3g over %d plies, %d under the margin' % (key, device, worst, row, close))
    # both tables are the reference's wp_func of the fixture's outcomes, from either side
    mine, theirs = {}, {}
    for g in range(G):
        for table, o in ((mine, float(outcome[g, g % 2])), (theirs, float(outcome[g, 1 - g % 2]))):
            table[o + 0.0] = table.get(o + 0.0, 0) + 1
    assert res['results'] == mine and res['win_rate'] == wp_func(mine)
    assert res['opponent_results'] == theirs and res['opponent_win_rate'] == wp_func(theirs)
