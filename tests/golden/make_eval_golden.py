"""Writes tests/golden/evaluation.{json,npz}: games of the reference's greedy Agent against its RandomAgent.

Runs ONLY where the reference HandyRL tree is available, at ``$HANDYRL_REF`` (default ``/root/reference``); it is
never imported by a test.  The games are the reference's own ``exec_match`` (evaluation.py:64-87) with
``Agent(ModelWrapper(net), observation)`` (agent.py:55-110) on seat g mod 2 and ``RandomAgent`` (agent.py:13-19) on
the other; ``net`` is the env's seeded ``env.net()()`` -- the fixture stores the torch seed, not the weights.  Data
only: per ply the mover and the action, the model's RAW policy at its plies, per game the outcome.

    python tests/golden/make_eval_golden.py
"""

import json
import os
import random
import sys

import numpy as np
import torch

REF = os.environ.get('HANDYRL_REF', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from handyrl.agent import Agent, RandomAgent          # noqa: E402
from handyrl.environment import make_env              # noqa: E402
from handyrl.evaluation import exec_match             # noqa: E402
from handyrl.model import ModelWrapper                # noqa: E402

TORCH_SEED = 7
MARGIN = 1e-4          # the test lets the device pick any label within this of the maximum
MAX_CLOSE = 0.05       # at most this share of a set's model plies may have a top-two margin under MARGIN
SETS = (('tictactoe', 'TicTacToe', False, 16), ('geister', 'Geister', False, 2), ('geister_obs', 'Geister', True, 2))


class Recorder(ModelWrapper):
    """Keeps a copy of the last raw policy (Agent.action masks its array in place)."""

    def inference(self, x, hidden, **kwargs):
        out = super().inference(x, hidden, **kwargs)
        self.last = np.array(out['policy'], dtype=np.float32, copy=True)
        return out


class ModelSeat(Agent):
    def action(self, env, player, show=False):
        a = super().action(env, player, show=show)
        legal = env.legal_actions(player)
        self.log.append((player, int(a), self.model.last, legal))
        return a


class RandomSeat(RandomAgent):
    def action(self, env, player, show=False):
        a = super().action(env, player, show=show)
        self.log.append((player, int(a), None, None))
        return a


def play(env_name, observation, games):
    env = make_env({'env': env_name})
    torch.manual_seed(TORCH_SEED)
    net = env.net()()
    net.eval()
    model = Recorder(net)
    out = []
    for g in range(games):
        random.seed(1000 + g)
        seat = g % 2
        log = []
        agents = {seat: ModelSeat(model, observation), 1 - seat: RandomSeat()}
        for a in agents.values():
            a.log = log
        outcome = exec_match(env, agents, None)
        out.append((seat, log, [float(outcome[p]) for p in env.players()]))
    return out


def main():
    meta = {'torch_seed': TORCH_SEED, 'margin': MARGIN, 'sets': {}}
    arrays = {}
    for key, env_name, observation, games in SETS:
        played = play(env_name, observation, games)
        Tm = max(len(log) for _, log, _ in played)
        mover = np.full((games, Tm), -1, dtype=np.int8)
        action = np.full((games, Tm), -1, dtype=np.int16)
        policy, where, close, total = [], [], 0, 0
        for g, (seat, log, outcome) in enumerate(played):
            for t, (player, a, p, legal) in enumerate(log):
                mover[g, t], action[g, t] = player, a
                if p is not None:
                    assert player == seat
                    top = np.sort(p[legal])[::-1]
                    total += 1
                    close += len(top) > 1 and top[0] - top[1] < MARGIN
                    policy.append(p)
                    where.append((g, t))
        assert close <= MAX_CLOSE * total, (key, close, total)
        arrays[key + '_mover'], arrays[key + '_action'] = mover, action
        arrays[key + '_policy'] = np.stack(policy).astype(np.float32)
        arrays[key + '_policy_at'] = np.array(where, dtype=np.int32)
        arrays[key + '_outcome'] = np.array([o for _, _, o in played], dtype=np.float32)
        meta['sets'][key] = {'env': env_name, 'observation': observation, 'games': games,
                             'length': [len(log) for _, log, _ in played], 'model_plies': total,
                             'plies_under_margin': int(close)}
        print(key, meta['sets'][key])
    np.savez_compressed(os.path.join(OUT, 'evaluation.npz'), **arrays)
    with open(os.path.join(OUT, 'evaluation.json'), 'w') as f:
        json.dump(meta, f, indent=1)


if __name__ == '__main__':
    main()
