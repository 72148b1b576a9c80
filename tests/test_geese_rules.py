"""Hungry Geese rules (handyrl_amd/envs/geese.py) on the CPU: the reference-held parts against goldens, one
hand-built position per rule clause, the pick rule, the plugin API and the CPU batch against the one-game function."""

import copy
import json
import os

import numpy as np
import pytest
import torch

from handyrl_amd.environment import ENVS, make_env
from handyrl_amd.envs import geese
from handyrl_amd.envs.geese import HungryGeeseBatch
from handyrl_amd.rollout import philox4x32
from tests.geese_games import SEED, cell, played, run_clause

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ---- what the reference plugin itself holds: observation, outcome, turns, terminal

def test_goldens_of_the_reference_plugin():
    with open(os.path.join(GOLDEN, 'geese_env.json')) as f:
        meta = json.load(f)
    obs = np.load(os.path.join(GOLDEN, 'geese_env.npz'))
    tags = {c['tag'] for c in meta['cases']}
    assert {'reset', 'after_death', 'dead_geese', 'end_tied', 'end_none_left'} <= tags and len(meta['cases']) >= 40
    env = make_env({'env': 'Geese'})
    for k, (case, want) in enumerate(zip(meta['cases'], meta['answers'])):
        env.update(case['state'], False)
        got = np.stack([env.observation(p) for p in range(4)])
        assert got.dtype == np.float32 and np.array_equal(got, obs['obs_%02d' % k]), (k, case['tag'])
        assert [env.outcome()[p] for p in range(4)] == want['outcome'], (k, case['tag'])
        assert env.turns() == want['turns'] and env.terminal() == want['terminal'], (k, case['tag'])
        assert np.array_equal(env.observation(None), got[0])


# ---- one position per clause

def _after(name):
    return run_clause(name)[-1]


def test_reversal():
    st = _after('reversal_kills_after_the_first_step')
    assert st['geese'][0] == [] and st['reward'][0] == 0 and st['last'][0] == 2
    st = _after('reversal_is_free_at_the_first_step')
    assert st['geese'][0] == [cell(1, 0)] and st['reward'][0] == 101


def test_growth_on_food():
    st = _after('growth_on_food')
    assert st['geese'][0] == [cell(1, 2), cell(1, 1)] and st['reward'][0] == 402
    assert cell(1, 2) not in st['food'] and -1 not in st['food']       # eaten, and two new cells


def test_self_collision_but_not_with_the_vacated_tail():
    assert _after('self_collision')['geese'][0] == []
    assert _after('own_vacated_tail_is_safe')['geese'][0] == [cell(2, 1), cell(1, 1), cell(1, 2), cell(2, 2)]


@pytest.mark.parametrize('s', (40, 80))
def test_hunger_and_starvation(s):
    st = _after('hunger_at_%d' % s)
    assert st['step'] == s
    assert st['geese'] == [[cell(1, 0)], [], [cell(5, 1), cell(5, 2)], [cell(5, 7)]]
    assert st['reward'] == [s * 100 + 1, 0, s * 100 + 2, s * 100 + 1]


def test_collisions_between_geese():
    st = _after('head_on')
    assert st['geese'][0] == [] and st['geese'][1] == [] and st['geese'][2] and st['live']
    st = _after('into_a_body')
    assert st['geese'][0] == [] and st['geese'][1] == [cell(3, 2), cell(2, 2), cell(1, 2)]
    st = _after('vacated_tail_of_another_is_safe')
    assert st['geese'][0] == [cell(1, 2)] and st['geese'][1] == [cell(4, 2), cell(3, 2), cell(2, 2)]


def test_two_geese_on_one_food():
    st = _after('two_geese_on_one_food')
    assert st['geese'][0] == [] and st['geese'][1] == []
    assert st['food'][1] == cell(0, 0) and st['food'][0] not in (-1, cell(1, 2))


def test_respawn_on_a_full_board():
    st = _after('respawn_with_no_free_cell')
    assert all(st['geese']) and sum(len(g) for g in st['geese']) == 77 and st['food'] == [-1, -1]
    st = _after('respawn_with_one_free_cell')
    assert sum(len(g) for g in st['geese']) == 76 and st['food'] == [cell(6, 9), -1]


def test_rewards():
    first, second = run_clause('reward_kept_after_death')
    assert first['reward'] == [301, 301, 402, 401] and first['live']
    assert second['reward'] == [301, 301, 502, 501] and second['geese'][:2] == [[], []]


def test_endings():
    first, second = run_clause('last_survivor')
    assert first['live'] and geese.turns_of(first) == [0, 1]
    assert not second['live'] and second['geese'][0] == [] and second['reward'] == [801, 902, 0, 301]
    assert geese.turns_of(second) == [] and geese.outcome_of(second) == [1 / 3, 1.0, -1.0, -1 / 3]
    st = _after('all_dead_in_one_step')
    assert not st['live'] and not any(st['geese']) and geese.outcome_of(st) == [2 / 3, 2 / 3, -2 / 3, -2 / 3]
    first, second = run_clause('truncation_at_199')
    assert first['step'] == 198 and first['live'] and second['step'] == 199 and not second['live']
    assert all(len(g) == 8 for g in second['geese']) and second['reward'] == [19908] * 4
    assert geese.outcome_of(second) == [0, 0, 0, 0]


# ---- the pick rule

KNOWN = (   # (counter, key, output): Philox4x32-10's all-zero known answer; then a counter and key with every word
            # different, expanded by the array form (which tests/test_stream_abi.py pins to the known answers)
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x00000001), (0xa4093822, 0x299f31d0), None),
)


def test_geese_picks_layout():
    # seed 0, game 0, step 0: the all-zero known answer is words 0-3
    assert ['%08x' % w for w in geese.geese_picks(0, 0, 0)[:4]] == KNOWN[0][2].split()
    # key from the seed's halves, counter (game lo, game hi, step, word // 4), checked against the array form
    counter, key, _ = KNOWN[1]
    seed, game = key[0] | (key[1] << 32), counter[0] | (counter[1] << 32)
    w = geese.geese_picks(seed, game, counter[2])
    assert len(w) == 8
    for block in (0, 1):
        want = philox4x32((counter[0], counter[1], counter[2], block), key)
        assert w[4 * block:4 * block + 4] == [int(x) for x in want]
    assert geese.geese_picks(seed, game, counter[2]) != geese.geese_picks(seed + 1, game, counter[2])


def test_picks_stay_in_range():
    n = np.arange(1, 78, dtype=np.uint64)
    g = np.arange(1300, dtype=np.uint64)
    words = np.stack(philox4x32((g, g >> np.uint64(32), 3, 0), (SEED, 0)))                  # 5200 words
    r = (words.reshape(-1, 1) * n.reshape(1, -1)) >> np.uint64(32)                         # 400,400 draws
    assert r.size > 10 ** 5 and (r < n.reshape(1, -1)).all()
    assert geese.pick_index(0xffffffff, 77) == 76 and geese.pick_index(0, 77) == 0
    assert all(geese.pick_index(int(x), 5) == int(x) * 5 >> 32 for x in words[0][:8])


def test_reset_places_heads_then_food():
    st = geese.new_game(SEED, 9)
    w = geese.geese_picks(SEED, 9, 0)
    free = list(range(77))
    want = []
    for k in range(6):
        want.append(free.pop(geese.pick_index(w[k], len(free))))
    assert [g[0] for g in st['geese']] == want[:4] and st['food'] == want[4:]
    assert st['prev'] == [-1] * 4 and st['last'] == [-1] * 4 and st['step'] == 0 and st['live']
    assert geese.new_game(SEED, 10)['geese'] != st['geese']


# ---- plugin API

def test_plugin_api():
    assert ENVS['Geese'] == 'handyrl_amd.envs.geese'
    env = make_env({'env': 'Geese', 'seed': 3})
    assert type(env).__module__ == 'handyrl_amd.envs.geese' and env.net().__name__ == 'GeeseNet'
    assert env.players() == [0, 1, 2, 3] and env.turns() == [0, 1, 2, 3] and not env.terminal()
    assert env.legal_actions(2) == [0, 1, 2, 3] and env.action_length() == 4 and env.reward() == {}
    assert [env.action2str(a) for a in range(4)] == ['NORTH', 'SOUTH', 'WEST', 'EAST'] and env.str2action('WEST') == 2
    assert env.state == geese.new_game(3, 0)
    env.step({0: 1, 1: 2, 2: 3, 3: 0})
    other = make_env({'env': 'Geese', 'seed': 3})
    other.update(env.diff_info(0), False)
    assert other.state == env.state and other.state is not env.state
    assert 'step 1' in str(env)
    env.reset()
    assert env.state == geese.new_game(3, 1)                            # games 0, 1, ... per instance
    with pytest.raises(NotImplementedError, match='kaggle_environments'):
        env.rule_based_action(0)


def test_host_generator_plays_a_game():
    from handyrl_amd.hostgen import HostBatchGenerator
    torch.manual_seed(0)
    env = make_env({'env': 'Geese'})
    net = env.net()()
    args = {'turn_based_training': False, 'observation': False, 'gamma': 0.8, 'compress_steps': 4}
    gen = HostBatchGenerator(lambda: make_env({'env': 'Geese'}), net, args, E=1, seed=1)
    ep, = gen.generate(1)
    assert 1 <= ep['steps'] <= 199 and set(ep['outcome']) == {0, 1, 2, 3}


# ---- the CPU batch against the one-game function

def _batch_equals_games(policy, games, E):
    recs, _ = played(policy, games)
    batch = HungryGeeseBatch(E, 'cpu', seed=SEED)
    steps = 0
    for lo in range(0, games, E):
        if lo:
            batch.reset()
        chunk = recs[lo:lo + E]
        assert batch.dump_games()[:len(chunk)] == [r['start'] for r in chunk]
        t = 0
        while any(t < len(r['actions']) for r in chunk):
            actions = torch.zeros(E, 4, dtype=torch.long)
            active = torch.zeros(E, dtype=torch.bool)
            for e, r in enumerate(chunk):
                if t < len(r['actions']):
                    actions[e] = torch.tensor(r['actions'][t])
                    active[e] = True
            assert torch.equal(batch.active()[:len(chunk)], active[:len(chunk)])
            batch.step_players(actions, batch.turns_mask(), active, None)
            got = batch.dump_games()
            for e, r in enumerate(chunk):
                assert got[e] == r['states'][min(t, len(r['states']) - 1)], (lo + e, t)
            t += 1
            steps += int(active.sum())
    return steps


def test_cpu_batch_equals_the_game_function_no_reversal_policy():
    _, ev = played('no_reversal', 256)
    # the set cannot be trivial games: every kind of event happens (a prototype with random.sample placement gave
    # mean length 40, 136 games past step 40, 713 food, 705 collisions, 348 hunger pops, 128 starvations, 7 self-collisions)
    for kind in ('ate', 'collision', 'hunger', 'starved', 'self', 'reached_40', 'no_survivor', 'tied'):
        assert ev[kind] >= 1, (kind, ev)
    assert ev['reversal'] == 0
    assert _batch_equals_games('no_reversal', 256, 64) == ev['steps']


def test_cpu_batch_equals_the_game_function_uniform_policy():
    _, ev = played('uniform', 64)
    assert ev['reversal'] >= 64 and ev['steps'] / 64 < 12              # mostly reversal deaths, short games
    assert _batch_equals_games('uniform', 64, 64) == ev['steps']


def test_batch_views_outcome_and_masks():
    recs, _ = played('no_reversal', 256)
    states = [r['states'][-1] for r in recs[:24]] + [r['states'][len(r['states']) // 2] for r in recs[:24]]
    batch = HungryGeeseBatch(len(states), 'cpu', seed=SEED)
    batch.load_games(states, range(len(states)))
    assert batch.dump_games() == states
    want = np.stack([np.stack([geese.observation_of(s, p) for s in states]) for p in range(4)])
    assert np.array_equal(batch.views_torch().numpy(), want)
    player = torch.arange(len(states)) % 4
    assert np.array_equal(batch.observation(player).numpy(),
                          np.stack([geese.observation_of(s, e % 4) for e, s in enumerate(states)]))
    assert np.array_equal(batch.outcome().numpy(), np.array([geese.outcome_of(s) for s in states], dtype=np.float32))
    assert batch.turns_mask().tolist() == [[p in geese.turns_of(s) for p in range(4)] for s in states]
    assert batch.terminal().tolist() == [not s['live'] for s in states] and batch.legal().all()
    assert batch.plies().tolist() == [s['step'] for s in states]


def test_reset_numbers_new_games_and_reset_where():
    batch = HungryGeeseBatch(5, 'cpu', seed=SEED)
    assert batch.game.tolist() == [0, 1, 2, 3, 4] and batch.next_game == 5
    batch.reset()
    assert batch.game.tolist() == [5, 6, 7, 8, 9]
    before = copy.deepcopy(batch.dump_games())
    batch.reset_where(torch.tensor([False, True, False, True, True]))
    after = batch.dump_games()
    assert [g['game'] for g in after] == [5, 10, 7, 11, 12] and batch.next_game == 13
    assert after[0] == before[0] and after[2] == before[2] and after[1] == geese.new_game(SEED, 10)
    batch.seed(SEED + 1)
    batch.reset()
    assert batch.dump_games()[0] == geese.new_game(SEED + 1, 13)


@pytest.mark.parametrize('generator', ['auto', 'host'])
def test_train_main_on_the_cpu(tmp_path, generator, monkeypatch):
    import handyrl_amd.main as hm
    from handyrl_amd.main import train_main
    args = {'env_args': {'env': 'Geese'},
            'train_args': {'turn_based_training': False, 'observation': False, 'update_episodes': 4,
                           'minimum_episodes': 4, 'maximum_episodes': 8, 'batch_size': 2, 'forward_steps': 4,
                           'epochs': 1, 'seed': 2, 'generator': generator, 'host_envs': 2}}
    made = []
    real = hm.make_env
    monkeypatch.setattr(hm, 'make_env', lambda a: (made.append(a.get('seed')), real(a))[1])
    batches = []
    real_batch = HungryGeeseBatch.seed
    monkeypatch.setattr(HungryGeeseBatch, 'seed', lambda self, s: (batches.append(s), real_batch(self, s))[1])

    def oracle_loss(outputs, batch, targs):     # the learner's HIP losses need a GPU: the CPU oracle stands in
        from oracle.learner import loss_from_outputs
        losses, dcnt = loss_from_outputs(outputs, batch, targs)
        return losses, torch.tensor(dcnt)
    model = train_main(args, device=torch.device('cpu'), loss_fn=oracle_loss, model_dir=str(tmp_path),
                       log=lambda *_: None)
    assert os.path.isfile(os.path.join(str(tmp_path), '1.pth'))
    if generator == 'host':     # the host Environment, every slot under a seed of its own
        assert made[0] is None and len(made) == 3 and len(set(made[1:])) == 2 and not batches
    else:                       # the device twin, keyed by the rank's seed
        assert made == [None] and batches[-1] == 2
    torch.manual_seed(2)
    fresh = geese.GeeseNet()
    assert any(not torch.equal(a, b) for a, b in zip(model.state_dict().values(), fresh.state_dict().values()))
