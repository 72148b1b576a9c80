"""The greedy rule-based goose on the host (``geese.greedy_action_of``, ``Environment.greedy_action``): hand-built
states for every clause of the rule, the plugin method, and a sanity run -- one uniform random goose against three
greedy ones loses nearly always, and those games are long.  ``rule_based_action`` (Kaggle's GreedyAgent, which this
package does not have) keeps raising: the project's own rule has its own name."""

import copy

import pytest

from handyrl_amd.envs import geese
from handyrl_amd.envs.geese import Environment, greedy_action_of
from handyrl_amd.evaluation import eval_pick_player
from tests.geese_greedy_states import CASES, E, N, S, W, cell, state


@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_built_states(name):
    st, want = CASES[name]
    before = copy.deepcopy(st)
    for p, w in enumerate(want):
        got = greedy_action_of(st, p)
        assert got in (-1, 0, 1, 2, 3)
        if w is not None:
            assert got == w, (name, p)
    assert st == before                     # the rule reads the state only


def test_the_plain_distance_case_as_the_issue_states_it():
    st = state([[cell(3, 1)]], food=(cell(3, 10), -1))
    blocked = {c for g in st['geese'] for c in g}
    assert all(geese.translate(cell(3, 1), a) not in blocked for a in range(4))      # all four neighbours free
    assert greedy_action_of(st, 0) == E
    # d(EAST) = 8 on the plain grid; around the torus WEST is one step from the food
    assert abs(2 - 10) == 8 and geese.translate(geese.translate(cell(3, 1), W), W) == cell(3, 10)


def test_order_is_north_east_south_west():
    assert geese.GREEDY_ORDER == (N, E, S, W) == (0, 3, 1, 2)
    assert [geese.ACTION[a] for a in geese.GREEDY_ORDER] == ['NORTH', 'EAST', 'SOUTH', 'WEST']


def test_environment_greedy_action_is_the_rule_or_a_legal_label():
    env = Environment({'seed': 3})
    seen_rule = 0
    for _ in range(40):
        if env.terminal():
            break
        acts = {}
        for p in env.turns():
            rule = greedy_action_of(env.state, p)
            a = env.greedy_action(p)
            assert a in env.legal_actions(p)
            if rule >= 0:
                assert a == rule
                seen_rule += 1
            acts[p] = a
        env.step(acts)
    assert seen_rule > 20
    # no candidate: a uniform random legal label
    env.state = copy.deepcopy(CASES['boxed_in'][0])
    assert greedy_action_of(env.state, 0) == -1
    assert {env.greedy_action(0) for _ in range(200)} == {0, 1, 2, 3}


def test_rule_based_action_still_raises():
    with pytest.raises(NotImplementedError, match='GreedyAgent'):
        Environment().rule_based_action(0)


def test_a_random_goose_loses_to_three_greedy_geese():
    """200 games ``new_game(5, g)``: seat 0 uniform random (``eval_pick_player``), seats 1-3 greedy with the same
    fallback.  Loose bounds that catch a broken rule (with Python's ``random`` as the fallback a trial gave a mean
    outcome of -0.984 and 84.4 plies): seat 0's mean outcome below -0.8, mean length above 40 plies."""
    seed, games, legal = 5, 200, [True] * 4
    total, plies = 0.0, 0
    for g in range(games):
        st, t = geese.new_game(seed, g), 0
        while st['live']:
            acts = [eval_pick_player(seed, g, t, 0, legal)]
            for p in (1, 2, 3):
                a = greedy_action_of(st, p)
                acts.append(a if a >= 0 or not st['geese'][p] else eval_pick_player(seed, g, t, p, legal))
            geese.step_game(st, acts, seed)
            t += 1
        total += geese.outcome_of(st)[0]
        plies += t
    print('seat 0 mean outcome %.3f, mean length %.1f plies' % (total / games, plies / games))
    assert total / games < -0.8
    assert plies / games > 40
