"""Writes tests/golden/match.{json,npz}: games of two of the reference's greedy Agents against each other.

Runs ONLY where the reference HandyRL tree is available, at ``$HANDYRL_REF`` (default ``/root/reference``); it is
never imported by a test.  The games are the reference's own ``exec_match`` (evaluation.py:64-87) with one
``Agent(ModelWrapper(net), observation)`` (agent.py:55-110) per seat: nets A and B are the env's ``env.net()()`` under
two torch seeds -- the fixture stores the seeds, not the weights -- and game g seats A on g mod 2.  The first k plies
of a game (k is listed per game) have their move replaced by a seeded ``random.choice`` of the legal
actions AFTER ``Agent.action`` has run, so the agent's recurrent state advances as the evaluator's forward does on a
forced ply.  Data only: per ply the mover and the action, the mover's RAW policy at every ply, per game the outcome
and k.

    python tests/golden/make_match_golden.py
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

from handyrl.agent import Agent                       # noqa: E402
from handyrl.environment import make_env              # noqa: E402
from handyrl.evaluation import exec_match             # noqa: E402
from handyrl.model import ModelWrapper                # noqa: E402

TORCH_SEEDS = (7, 8)   # nets A and B
MARGIN = 1e-4          # the test lets the device pick any label within this of the maximum
MAX_CLOSE = 0.05       # at most this share of a set's plies may have a top-two margin under MARGIN
# key, env, observation, k of every game (0 .. 4 for TicTacToe, 0 .. 12 for Geister)
SETS = (('tictactoe', 'TicTacToe', False, [g % 5 for g in range(16)]), ('geister', 'Geister', False, [12, 5]),
        ('geister_obs', 'Geister', True, [0, 9]))


class Recorder(ModelWrapper):
    """Keeps a copy of the last raw policy (Agent.action masks its array in place)."""

    def inference(self, x, hidden, **kwargs):
        out = super().inference(x, hidden, **kwargs)
        self.last = np.array(out['policy'], dtype=np.float32, copy=True)
        return out


class Seat(Agent):
    def action(self, env, player, show=False):
        a = super().action(env, player, show=show)
        legal = env.legal_actions(player)
        if len(self.log) < self.opening:
            a = random.choice(legal)
        self.log.append((player, int(a), self.model.last, legal))
        return a


def play(env_name, observation, openings):
    env = make_env({'env': env_name})
    models = []
    for seed in TORCH_SEEDS:
        torch.manual_seed(seed)
        net = env.net()()
        net.eval()
        models.append(Recorder(net))
    out = []
    for g, k in enumerate(openings):
        random.seed(2000 + g)
        seat = g % 2
        log = []
        agents = {seat: Seat(models[0], observation), 1 - seat: Seat(models[1], observation)}
        for a in agents.values():
            a.log, a.opening = log, k
        outcome = exec_match(env, agents, None)
        out.append((seat, k, log, [float(outcome[p]) for p in env.players()]))
    return out


def main():
    meta = {'torch_seeds': list(TORCH_SEEDS), 'margin': MARGIN, 'sets': {}}
    arrays = {}
    for key, env_name, observation, openings in SETS:
        games = len(openings)
        played = play(env_name, observation, openings)
        Tm = max(len(log) for _, _, log, _ in played)
        mover = np.full((games, Tm), -1, dtype=np.int8)
        action = np.full((games, Tm), -1, dtype=np.int16)
        policy, close, total = [], 0, 0
        for g, (seat, k, log, outcome) in enumerate(played):
            for t, (player, a, p, legal) in enumerate(log):
                mover[g, t], action[g, t] = player, a
                top = np.sort(p[legal])[::-1]
                total += 1
                close += len(top) > 1 and top[0] - top[1] < MARGIN
                policy.append(p)
        assert close <= MAX_CLOSE * total, (key, close, total)
        arrays[key + '_mover'], arrays[key + '_action'] = mover, action
        arrays[key + '_policy'] = np.stack(policy).astype(np.float32)      # game-major, ply by ply
        arrays[key + '_outcome'] = np.array([o for _, _, _, o in played], dtype=np.float32)
        meta['sets'][key] = {'env': env_name, 'observation': observation, 'games': games,
                             'length': [len(log) for _, _, log, _ in played],
                             'opening': [k for _, k, _, _ in played], 'plies': total,
                             'plies_under_margin': int(close)}
        print(key, meta['sets'][key])
    np.savez_compressed(os.path.join(OUT, 'match.npz'), **arrays)
    with open(os.path.join(OUT, 'match.json'), 'w') as f:
        json.dump(meta, f, indent=1)


if __name__ == '__main__':
    main()
