"""Shared by the Hungry Geese tests: seeded games of the Python rules (played once per session) and one hand-built
position per rule clause.  Cells are row * 11 + col; actions 0 NORTH 1 SOUTH 2 WEST 3 EAST."""

import copy
import functools
import random

from handyrl_amd.envs import geese

SEED = 5
N, S, W, E = 0, 1, 2, 3


def cell(r, c):
    return r * 11 + c


def state(gs, food=(-1, -1), last=(-1, -1, -1, -1), step=0, reward=(0, 0, 0, 0), game=0):
    gs = [list(g) for g in gs]
    return {'geese': gs, 'food': list(food), 'last': list(last), 'prev': [g[0] if g else -1 for g in gs],
            'reward': list(reward), 'step': step, 'game': game, 'live': sum(bool(g) for g in gs) >= 2}


def no_reversal(rng, st):
    out = []
    for p in range(4):
        a = rng.randrange(4)
        while st['last'][p] >= 0 and a == geese.OPPOSITE[st['last'][p]]:
            a = rng.randrange(4)
        out.append(a)
    return out


def uniform(rng, st):
    return [rng.randrange(4) for _ in range(4)]


@functools.lru_cache(maxsize=None)
def played(policy, games, seed=SEED, first=0):
    """``games`` games number first.. under ``policy`` ('no_reversal' / 'uniform', random.Random(1)): per game the
    start state, the action rows and the state after every step; and the summed events.  Read-only for callers."""
    rng = random.Random(1)
    choose = {'no_reversal': no_reversal, 'uniform': uniform}[policy]
    out, events = [], {}
    for g in range(first, first + games):
        st = geese.new_game(seed, g)
        rec = {'start': copy.deepcopy(st), 'actions': [], 'states': []}
        while st['live']:
            a = choose(rng, st)
            for k, v in geese.step_game(st, a, seed).items():
                events[k] = events.get(k, 0) + v
            rec['actions'].append(a)
            rec['states'].append(copy.deepcopy(st))
        events['steps'] = events.get('steps', 0) + st['step']
        events['reached_40'] = events.get('reached_40', 0) + (st['step'] >= 40)
        events['no_survivor'] = events.get('no_survivor', 0) + (not any(st['geese']))
        events['tied'] = events.get('tied', 0) + (len(set(st['reward'])) < 4)
        out.append(rec)
    return out, events


FAR = ([cell(3, 5)], [cell(5, 2)], [cell(5, 8)])      # three geese out of everybody's way (they move NORTH)
ROW = [cell(6, c) for c in range(11)]


def two_rows(r):
    """A goose filling rows r and r + 1 as one cycle: head (r, 0), tail (r + 1, 0); it came WEST and may go SOUTH."""
    return [cell(r, c) for c in range(11)] + [cell(r + 1, c) for c in range(10, -1, -1)]


FULL = [two_rows(0), two_rows(2), two_rows(4)]

# name -> (state, [one action row per step])
CLAUSES = {
    'reversal_kills_after_the_first_step': (state([[cell(1, 1)], *FAR], last=(E, -1, -1, -1), step=1), [[W, N, N, N]]),
    'reversal_is_free_at_the_first_step': (state([[cell(1, 1)], *FAR], last=(E, -1, -1, -1), step=0), [[W, N, N, N]]),
    'growth_on_food': (state([[cell(1, 1)], *FAR], food=(cell(1, 2), -1), step=3), [[E, N, N, N]]),
    'self_collision': (state([[cell(1, 1), cell(1, 2), cell(2, 2), cell(2, 1), cell(2, 0)], *FAR],
                             last=(W, -1, -1, -1), step=3), [[S, N, N, N]]),
    'own_vacated_tail_is_safe': (state([[cell(1, 1), cell(1, 2), cell(2, 2), cell(2, 1)], *FAR],
                                       last=(W, -1, -1, -1), step=3), [[S, N, N, N]]),
    'hunger_at_40': (state([[cell(1, 1), cell(1, 2)], [cell(3, 5)], [cell(5, 2), cell(5, 3), cell(5, 4)],
                            [cell(5, 8), cell(5, 9)]], last=(W, N, W, W), step=39), [[W, N, W, W]]),
    'hunger_at_80': (state([[cell(1, 1), cell(1, 2)], [cell(3, 5)], [cell(5, 2), cell(5, 3), cell(5, 4)],
                            [cell(5, 8), cell(5, 9)]], last=(W, N, W, W), step=79), [[W, N, W, W]]),
    'head_on': (state([[cell(1, 1)], [cell(1, 3)], [cell(5, 2)], [cell(5, 8)]], step=3), [[E, W, N, N]]),
    'into_a_body': (state([[cell(1, 1)], [cell(2, 2), cell(1, 2), cell(1, 3)], [cell(5, 2)], [cell(5, 8)]],
                          last=(-1, S, -1, -1), step=3), [[E, S, N, N]]),
    'vacated_tail_of_another_is_safe': (state([[cell(1, 1)], [cell(3, 2), cell(2, 2), cell(1, 2)], [cell(5, 5)],
                                               [cell(5, 8)]], last=(-1, S, -1, -1), step=3), [[E, S, N, N]]),
    'two_geese_on_one_food': (state([[cell(1, 1)], [cell(1, 3), cell(1, 4)], [cell(5, 2)], [cell(5, 8)]],
                                    food=(cell(1, 2), cell(0, 0)), last=(-1, W, -1, -1), step=3), [[E, W, N, N]]),
    'respawn_with_no_free_cell': (state([*FULL, ROW], last=(W, W, W, W), step=3), [[S, S, S, W]]),
    'respawn_with_one_free_cell': (state([*FULL, ROW[:10]], last=(W, W, W, W), step=3), [[S, S, S, W]]),
    'reward_kept_after_death': (state([[cell(1, 1)], [cell(1, 3)], [cell(5, 2), cell(5, 3)], [cell(5, 8)]],
                                      reward=(301, 301, 302, 301), step=3), [[E, W, W, N], [E, W, W, N]]),
    'last_survivor': (state([[cell(1, 1)], [cell(1, 3), cell(1, 4)], [], []], last=(E, W, N, N),
                            reward=(701, 702, 0, 301), step=7), [[N, N, N, N], [S, W, N, N]]),
    'all_dead_in_one_step': (state([[cell(1, 1)], [cell(1, 3)], [], []], last=(E, W, N, N), reward=(701, 701, 0, 0),
                                   step=7), [[E, W, N, N]]),
    'truncation_at_199': (state([[cell(r, c) for c in range(8, 0, -1)] for r in (0, 2, 4, 6)], last=(E, E, E, E),
                                food=(cell(1, 0), cell(3, 0)), step=197), [[E, E, E, E], [E, E, E, E]]),
}


def run_clause(name, seed=SEED):
    """The states after every step of a clause position under the Python rules."""
    st, rows = CLAUSES[name]
    st = copy.deepcopy(st)
    out = []
    for a in rows:
        geese.step_game(st, a, seed)
        out.append(copy.deepcopy(st))
    return out
