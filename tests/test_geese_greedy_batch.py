"""``HungryGeeseBatch.greedy_players`` on a CPU batch against ``geese.greedy_action_of`` on the decoded tensors, at
every ply of greedy-vs-random games played to the end (this is the form the kernel is tested against)."""

import pytest
import torch

from handyrl_amd.envs.geese import GEESE, HungryGeeseBatch, greedy_action_of
from handyrl_amd.evaluation import eval_pick_player

SEED = 0x5eed0123456789


@pytest.mark.parametrize('E', [1, 5])
def test_cpu_batch_equals_the_rule_at_every_ply(E):
    b = HungryGeeseBatch(E, 'cpu')
    b.seed(SEED)
    b.reset()
    assert HungryGeeseBatch.RULE_AGENT == 'greedy_players'
    t, dead_seen, rule_seen = 0, 0, 0
    while bool(b.live.any()):
        rule = b.greedy_players()
        assert rule.shape == (E, GEESE) and rule.dtype == torch.long
        states = b.dump_games()
        want = [[greedy_action_of(st, p) for p in range(GEESE)] for st in states]
        assert rule.tolist() == want, t
        actions = torch.zeros(E, GEESE, dtype=torch.long)
        for e, st in enumerate(states):
            for p in range(GEESE):
                if not st['geese'][p]:
                    assert int(rule[e, p]) == -1
                    dead_seen += 1
                    continue
                rule_seen += int(rule[e, p]) >= 0
                random_seat = p == e % GEESE            # one random goose per slot, greedy geese on the other seats
                a = -1 if random_seat else int(rule[e, p])
                actions[e, p] = a if a >= 0 else eval_pick_player(SEED, st['game'], t, p, [True] * 4)
        b.step_players(actions, None, b.live.clone(), None)
        t += 1
    assert t > 10 and dead_seen > 0 and rule_seen > 10 * E
    # a finished game is still a state: the rule is given for it too
    assert b.greedy_players().tolist() == [[greedy_action_of(st, p) for p in range(GEESE)] for st in b.dump_games()]


def test_no_slots():
    rule = HungryGeeseBatch(0, 'cpu').greedy_players()
    assert rule.shape == (0, GEESE) and rule.dtype == torch.long
