"""Reference parity of the device evaluator: games the reference's ``exec_match`` played with its greedy ``Agent``
against ``RandomAgent`` (tests/golden/evaluation.*, written by tests/golden/make_eval_golden.py) are replayed move
for move through ``forced``, and the evaluator's own decisions are compared with the reference's.

The net is the env's seeded ``env.net()()`` (the fixture holds the torch seed).  The random seat's moves come from
Python's ``random`` in the reference, so they are given, not compared; the model's move is compared wherever the
fixture's top-two margin is at least 1e-4 -- the net tolerance is 1e-5, so above that margin the argmax cannot
flip -- and must be one of the labels within 1e-4 of the fixture maximum elsewhere.
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
    base = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evaluation')
    with open(base + '.json') as f:
        meta = json.load(f)
    return meta, np.load(base + '.npz')


def _net(env_name, seed, dev):
    env = make_env({'env': env_name})
    torch.manual_seed(seed)
    net = env.net()()
    if dev.type == 'cuda':
        from handyrl_amd.nn import accelerate
        net = accelerate(net.to(dev))
    return type(env).__module__, net


@pytest.mark.parametrize('device,graph', MODES)
@pytest.mark.parametrize('key', SETS)
def test_reference_games_replayed(request, golden, key, device, graph):
    meta, arrays = golden
    dev = request.getfixturevalue('cuda') if device == 'cuda' else torch.device('cpu')
    info = meta['sets'][key]
    assert meta['margin'] == MARGIN
    G, lengths = info['games'], info['length']
    mover, action = arrays[key + '_mover'], arrays[key + '_action'].astype(np.int64)
    ref_policy, at, outcome = arrays[key + '_policy'], arrays[key + '_policy_at'], arrays[key + '_outcome']
    assert len(at) == info['model_plies'] and info['plies_under_margin'] <= 0.05 * info['model_plies']
    module, net = _net(info['env'], meta['torch_seed'], dev)
    cls = batched_env(module)
    state = torch.get_rng_state()
    ev = DeviceEvaluator(cls(max(1, G - 1), dev), net, observation=info['observation'], seed=5, graph=graph)
    res = ev.evaluate(G, forced=torch.from_numpy(action), trace=True)
    assert torch.equal(torch.get_rng_state(), state)
    tr = {k: v.cpu().numpy() for k, v in res['trace'].items()}
    # outcomes and lengths: exact
    assert res['length'].tolist() == lengths
    assert np.array_equal(res['outcome'].cpu().numpy(), outcome)
    assert res['seat'].tolist() == [g % 2 for g in range(G)]
    for g in range(G):
        L = lengths[g]
        assert np.array_equal(tr['action'][g, :L], action[g, :L]) and (tr['action'][g, L:] == -1).all()
        assert np.array_equal(tr['model_ply'][g, :L], mover[g, :L] == g % 2)      # the model sits on seat g mod 2
        # the random seat: given through forced, so trivially the move played
        rnd = ~tr['model_ply'][g, :L]
        assert np.array_equal(tr['action'][g, :L][rnd], action[g, :L][rnd])
    # the model's plies
    close = 0
    worst = 0.0
    for (g, t), p_ref in zip(at.tolist(), ref_policy):
        assert tr['model_ply'][g, t]
        p = tr['policy'][g, t]
        legal = p > -1e31
        d = float(np.abs(p[legal] - p_ref[legal]).max())
        worst = max(worst, d)
        assert d <= 1e-5, (key, g, t, d)
        top = np.sort(p_ref[legal])[::-1]
        picked = int(tr['picked'][g, t])
        assert legal[picked], (key, g, t)
        if len(top) == 1 or top[0] - top[1] >= MARGIN:
            assert picked == int(action[g, t]), (key, g, t, float(top[0] - top[1]) if len(top) > 1 else None)
        else:
            close += 1
            assert p_ref[picked] >= top[0] - MARGIN, (key, g, t)
    assert close == info['plies_under_margin']
    print('%s on %s: max |policy - fixture| %.3g over %d model plies, %d under the margin'
          % (key, device, worst, len(at), close))
    # the win rate is the reference's wp_func of the fixture's outcomes from the model's side
    table = {}
    for g in range(G):
        o = float(outcome[g, g % 2]) + 0.0
        table[o] = table.get(o, 0) + 1
    assert res['results'] == table and res['win_rate'] == wp_func(table)


def test_wp_func_is_the_references():
    """evaluation.py:139-144 on hand-made tables (None keys are skipped, no game gives 0.0)."""
    assert wp_func({1: 87, -1: 12, 0: 1}) == 0.875
    assert wp_func({None: 4, 1.0: 1, -1.0: 1}) == 0.5
    assert wp_func({None: 3}) == 0.0
