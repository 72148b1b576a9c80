"""Generate the Hungry Geese env fixtures ``geese_env.npz`` / ``geese_env.json``.

Runs ONLY where the reference HandyRL tree is readable at ``$HANDYRL_REF`` (default ``/root/reference``).  The
reference's ``Environment`` (handyrl/envs/kaggle/hungry_geese.py) is built with ``object.__new__`` -- its
``__init__`` needs ``kaggle_environments``, which is stubbed in ``sys.modules`` as in make_golden.py -- and fed
``obs_list`` entries in the interpreter's format from states of games played by THIS package's rules
(handyrl_amd/envs/geese.py).  What the reference answers for them is recorded: ``observation(p)`` for all p,
``outcome()``, ``turns()`` and ``terminal()``.  The fixtures hold the states (as JSON) and those answers: data only.

Usage:  python tests/golden/make_geese_env_golden.py
"""

import copy
import json
import os
import random
import sys
import types

import numpy as np

REF = os.environ.get('HANDYRL_REF', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

if 'kaggle_environments' not in sys.modules:
    stub = types.ModuleType('kaggle_environments')

    def make(*_a, **_k):
        raise RuntimeError('kaggle_environments stub: the rules are not available')
    stub.make = make
    sys.modules['kaggle_environments'] = stub

from handyrl.envs.kaggle.hungry_geese import Environment as RefEnvironment   # noqa: E402
from handyrl_amd.envs import geese                                           # noqa: E402

SEED = 11


def interpreter_obs(state):
    """One ``obs_list`` entry: per agent status and reward; agent 0's observation carries geese and food."""
    out = []
    for p in range(4):
        active = state['live'] and bool(state['geese'][p])
        obs = {'index': p}
        if p == 0:
            obs.update(geese=copy.deepcopy(state['geese']), food=[f for f in state['food'] if f >= 0])
        out.append({'status': 'ACTIVE' if active else 'DONE', 'reward': state['reward'][p], 'observation': obs})
    return out


def reference_answers(before, state):
    env = object.__new__(RefEnvironment)
    env.obs_list = ([] if before is None else [interpreter_obs(before)]) + [interpreter_obs(state)]
    env.last_actions = {}
    obs = np.stack([env.observation(p) for p in range(4)])
    outcome = env.outcome()
    return obs, {'outcome': [outcome[p] for p in range(4)], 'turns': env.turns(), 'terminal': env.terminal()}


def main():
    rng = random.Random(1)
    picked = {}     # tag -> list of (before, state)

    def keep(tag, before, state, limit):
        if len(picked.setdefault(tag, [])) < limit:
            picked[tag].append((copy.deepcopy(before), copy.deepcopy(state)))

    for game in range(64):
        state = geese.new_game(SEED, game)
        keep('reset', None, state, 3)
        while state['live']:
            before = copy.deepcopy(state)
            actions = []
            for p in range(4):
                a = rng.randrange(4)
                while state['last'][p] >= 0 and a == geese.OPPOSITE[state['last'][p]]:
                    a = rng.randrange(4)
                actions.append(a)
            geese.step_game(state, actions, SEED)
            died = sum(bool(b) and not g for b, g in zip(before['geese'], state['geese']))
            dead = sum(not g for g in state['geese'])
            if died and state['live']:
                keep('after_death', before, state, 6)
            elif dead and state['live']:
                keep('dead_geese', before, state, 6)
            elif state['step'] % 40 == 0:
                keep('hunger', before, state, 3)
            elif max(len(g) for g in state['geese']) >= 4:
                keep('long', before, state, 6)
            if not state['live']:
                r = state['reward']
                tied = len(set(r)) < 4
                none_left = not any(state['geese'])
                keep('end_none_left' if none_left else 'end_tied' if tied else 'end', before, state, 6)
    cases, arrays, answers = [], {}, []
    for tag in sorted(picked):
        for before, state in picked[tag]:
            obs, ans = reference_answers(before, state)
            arrays['obs_%02d' % len(cases)] = obs
            cases.append({'tag': tag, 'state': state})
            answers.append(ans)
    np.savez_compressed(os.path.join(OUT, 'geese_env.npz'), **arrays)
    with open(os.path.join(OUT, 'geese_env.json'), 'w') as f:
        json.dump({'seed': SEED, 'cases': cases, 'answers': answers}, f)
    print('%d cases: %s' % (len(cases), {t: len(v) for t, v in picked.items()}))


if __name__ == '__main__':
    main()
