"""rollout.PlayerStreamGenerator: the public sampling rules, and every episode it puts into the ring refereed on its
own.

A game's randomness depends on (seed, game number, ply) only -- the players' uniforms (``stream_player_uniforms``),
the played player (``stream_select_uniform``) and, for Hungry Geese, the food (``geese.geese_picks``) -- so a ring
row with game number n is checked without knowing in which slot or when it was played: the game is replayed from its
start on the recorded actions by the env's own rules (observations, masks, length, outcome), the sampling is redone
from the rule on the recorded policies with the same torch ops on the same device (exact), the reset values are
checked past the end, and the recorded policies / values are compared with a CPU eval forward on the recorded
observations (1e-5 absolute, the project's self-play bound of tests/test_geese_selfplay_gpu.py).
"""

import numpy as np
import pytest
import torch

from handyrl_amd import rollout
from handyrl_amd.envs import geese
from handyrl_amd.envs.geese import HungryGeeseBatch
from handyrl_amd.envs.hungry_geese import GeeseNet
from handyrl_amd.envs.tictactoe import SimpleConv2dModel
from handyrl_amd.rollout import (DeviceReplay, ParallelTicTacToeBatch, PlayerReplay, PlayerStreamGenerator,
                                 TicTacToeBatch, stream_player_uniforms, stream_select_uniform, stream_uniforms)

GAMMA = 0.8
RECORDS = ('policy', 'amask', 'action', 'value', 'tmask', 'omask', 'reward', 'ret', 'length', 'outcome')


def make(name, dev, E, N, seed, net_seed=11, **kw):
    """(generator, replay, CPU twin of its net) for 'geese' or 'ptt' on ``dev``."""
    dev = torch.device(dev)
    Net = GeeseNet if name == 'geese' else SimpleConv2dModel
    torch.manual_seed(net_seed)
    cpu = Net()
    cpu.eval()
    net = cpu
    if dev.type == 'cuda':
        from handyrl_amd.nn import accelerate
        net = Net().to(dev)
        net.load_state_dict(cpu.state_dict())
        net = accelerate(net)
    env = HungryGeeseBatch(E, dev, seed=seed) if name == 'geese' else ParallelTicTacToeBatch(E, dev)
    replay = PlayerReplay(N, env.MAX_PLIES, env.OBS_SHAPE, env.A, env.P, dev, obs_dtype=torch.uint8)
    gen = PlayerStreamGenerator(env, net, replay, gamma=GAMMA, seed=seed, **kw)
    return gen, replay, cpu


def ring_rows(replay, gen, rows):
    """The ring rows ``rows`` as CPU tensors."""
    idx = torch.as_tensor(rows, device=replay.policy.device)
    out = {k: getattr(replay, k)[idx].cpu() for k in RECORDS}
    out['obs'] = replay.obs[idx].cpu()
    out['game'] = gen.ring_game[idx].cpu()
    return out


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


class GeeseGame:
    """One Hungry Geese game replayed by ``step_game``."""
    P, A, Tm = 4, 4, geese.MAX_PLIES

    def __init__(self, seed, n):
        self.seed, self.state = seed, geese.new_game(seed, n)

    def live(self):
        return self.state['live']

    def turns(self):
        alive = geese.turns_of(self.state)
        return [p in alive for p in range(4)]

    def observation(self, p):
        return torch.from_numpy(geese.observation_of(self.state, p))

    def legal(self, p):
        return torch.ones(4, dtype=torch.bool)

    def step(self, actions, u):
        geese.step_game(self.state, actions, self.seed)

    def outcome(self):
        return torch.tensor([float(np.float32(x)) for x in geese.outcome_of(self.state)])


class ParallelGame:
    """One ParallelTicTacToe game replayed by the batch env's own rules on a one-game CPU batch."""
    P, A, Tm = 2, 9, 9

    def __init__(self, seed, n):
        self.b = ParallelTicTacToeBatch(1, 'cpu')

    def live(self):
        return not bool(self.b.terminal())

    def turns(self):
        return [True, True]

    def observation(self, p):
        return self.b.observation(torch.tensor([p]))[0]

    def legal(self, p):
        return self.b.legal()[0]

    def step(self, actions, u):
        one = torch.ones(1, dtype=torch.bool)
        self.b.step_players(torch.tensor([actions]), one.view(1, 1).expand(1, 2), one, torch.tensor([u]))

    def outcome(self):
        return self.b.outcome()[0].float()


def referee(game_cls, gen, replay, cpu_net, rows):
    """Every check of the module doc for the ring rows ``rows``; returns their lengths."""
    P, A, Tm = game_cls.P, game_cls.A, game_cls.Tm
    rec = ring_rows(replay, gen, rows)
    where = []
    for i, row in enumerate(rows):
        n, L = int(rec['game'][i]), int(rec['length'][i])
        assert 0 <= n < gen.games_started and 1 <= L <= Tm, (row, n, L)
        g = game_cls(gen.seed, n)
        for t in range(L):
            assert g.live(), (row, t)
            turns = g.turns()
            assert rec['tmask'][i, t].tolist() == rec['omask'][i, t].tolist() == turns, (row, t)
            for p in range(P):
                if turns[p]:
                    assert torch.equal(rec['obs'][i, t, p].float(), g.observation(p)), (row, t, p)
                    assert torch.equal(rec['amask'][i, t, p], torch.where(g.legal(p), 0.0, 1e32)), (row, t, p)
                    assert bool(g.legal(p)[int(rec['action'][i, t, p])]), (row, t, p)
                    where.append((i, t, p, n))
                else:       # a player that neither moves nor infers: the reset values, not an earlier game's
                    assert not bool(rec['obs'][i, t, p].any()), (row, t, p)
                    assert not bool(rec['policy'][i, t, p].any()) and bool((rec['amask'][i, t, p] == 1e32).all())
                    assert int(rec['action'][i, t, p]) == 0 and float(rec['value'][i, t, p]) == 0.0, (row, t, p)
            g.step(rec['action'][i, t].tolist(), float(stream_select_uniform(gen.seed, n, t)))
        assert not g.live() or L == Tm, (row, L)
        assert torch.equal(rec['outcome'][i], g.outcome()), row
        # the reset values past the end
        assert not bool(rec['obs'][i, L:].any()) and not bool(rec['policy'][i, L:].any()), row
        assert bool((rec['amask'][i, L:] == 1e32).all()), row
        for k in ('action', 'value', 'tmask', 'omask', 'reward', 'ret'):
            assert not bool(rec[k][i, L:].any()), (row, k)
        assert not bool(rec['reward'][i].any()) and not bool(rec['ret'][i].any()), row     # these envs have no reward
    ii, tt, pp, nn = (torch.tensor(x) for x in zip(*where))
    # the sampling, redone from the public rule on the recorded policy with the same ops on the generator's device
    dev = replay.policy.device
    u = torch.from_numpy(stream_player_uniforms(gen.seed, nn.numpy(), tt.numpy(), P, A))[torch.arange(len(nn)), pp]
    pol = rec['policy'][ii, tt, pp].to(dev)
    act = torch.argmax(pol - torch.log(-torch.log(u.to(dev))), dim=-1).cpu()
    assert torch.equal(act, rec['action'][ii, tt, pp])
    # the recorded policies (at the legal labels) and values are the net's on the recorded observations
    with torch.no_grad():
        want = cpu_net(rec['obs'][ii, tt, pp].float(), None)
    legal = rec['amask'][ii, tt, pp] == 0
    dp = torch.where(legal, (rec['policy'][ii, tt, pp] - want['policy'].float()).abs(), 0.0).max()
    dv = (rec['value'][ii, tt, pp] - want['value'].float().reshape(-1)).abs().max()
    assert float(dp) <= 1e-5 and float(dv) <= 1e-5, (float(dp), float(dv))
    return rec['length'].tolist()


def bookkeeping(gen, replay, outs, ptr0=0):
    emitted = sum(o['episodes'] for o in outs)
    ring_ptr, dev_emitted, next_game = gen._state()['state'].tolist()
    assert dev_emitted == emitted and replay.ptr == ring_ptr == (ptr0 + emitted) % replay.N
    assert replay.count == min(emitted, replay.N)
    assert gen.games_started == next_game == gen.env.E + emitted
    if hasattr(gen.env, 'next_game'):
        assert gen.env.next_game == next_game
    games = gen.ring_game[:replay.count].tolist()
    assert len(set(games)) == len(games) and all(0 <= g < gen.games_started for g in games)
    assert bool((gen.ring_game[replay.count:] == -1).all())
    return emitted


# ---- the rules

def test_player_rules_equal_their_torch_twins():
    game = np.array([0, 5, (1 << 33) + 7, 1000003])
    ply = np.array([0, 3, 198, 8])
    for seed, P, A in ((7, 4, 4), (0x9e3779b97f4a7c15, 2, 9), (3, 3, 214)):
        u = stream_player_uniforms(seed, game, ply, P, A)
        ut = rollout.stream_player_uniforms_torch(seed, torch.from_numpy(game), torch.from_numpy(ply), P, A)
        assert u.shape == (4, P, A) and u.dtype == np.float32 and np.array_equal(u, ut.numpy())
        assert float(u.min()) > 0.0 and float(u.max()) < 1.0
        assert np.array_equal(stream_player_uniforms(seed, 5, 3, P, A), u[1])
        s = stream_select_uniform(seed, game, ply)
        st = rollout.stream_select_uniform_torch(seed, torch.from_numpy(game), torch.from_numpy(ply))
        assert s.shape == (4,) and s.dtype == np.float32 and np.array_equal(s, st.numpy())
        # player 0's uniforms are not the mover rule's, nor is the select uniform one of either
        assert not np.array_equal(u[:, 0], stream_uniforms(seed, game, ply, A))
        assert not np.isin(s, u).any()


def test_counter_words_of_the_streams_are_disjoint():
    P, A = 4, 4
    blocks = (A + 3) // 4
    w3 = {rollout.PLAYER_W3 + p * blocks + a // 4 for p in range(P) for a in range(A)}
    assert len(w3) == P * blocks
    assert not w3 & {0, 1, 0xffffffff, rollout.SELECT_W3}
    assert all(rollout.PLAYER_W3 <= w < rollout.SELECT_W3 for w in w3)
    # the rule's first word is what the generator's key and counter give, by the array form of Philox
    x = rollout.philox4x32((5, 0, 3, rollout.PLAYER_W3 + 2 * blocks), (7, 0))[1]
    want = np.float32((int(x) >> 9) + 0.5) * np.float32(2.0 ** -23)
    assert stream_player_uniforms(7, 5, 3, P, A)[2, 1] == want
    with pytest.raises(ValueError, match='0x40000000'):
        stream_player_uniforms(0, 0, 0, 1 << 29, 8)
    with pytest.raises(ValueError, match='0x40000000'):
        rollout.stream_player_uniforms_torch(0, torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long),
                                             1 << 29, 8)


# ---- the generator on the CPU

def test_geese_stream_is_refereed():
    gen, replay, cpu = make('geese', 'cpu', 5, 64, seed=3)
    out = gen.generate(24)
    assert out['episodes'] >= 24 and out['plies'] % 16 == 0
    emitted = bookkeeping(gen, replay, [out])
    assert emitted > 2 * 5                       # the slots restarted
    lengths = referee(GeeseGame, gen, replay, cpu, list(range(replay.count)))    # every emitted row
    assert out['env_steps'] == sum(lengths) and max(lengths) > 1
    dead = replay.tmask[:emitted].sum(-1)
    assert bool(((dead > 0) & (dead < 4)).any())     # plies with a dead goose were among those refereed


def test_parallel_tictactoe_stream_is_refereed():
    gen, replay, cpu = make('ptt', 'cpu', 7, 32, seed=5)
    out = gen.generate(40)
    assert out['episodes'] >= 40
    bookkeeping(gen, replay, [out])
    assert replay.count == 32                    # the ring wrapped
    lengths = referee(ParallelGame, gen, replay, cpu, list(range(32)))
    assert all(3 <= n <= 9 for n in lengths)
    assert int(gen.ring_game.min()) == int(gen.ring_game[replay.ptr])     # the oldest game sits at the ring pointer


def test_stream_is_deterministic_and_independent_of_the_slot_count():
    runs = {}
    for key, E, calls in (('one', 5, (32,)), ('two', 5, (16, 16)), ('few', 3, (24,))):
        gen, replay, _ = make('geese', 'cpu', E, 64, seed=3)
        outs = [gen.generate(n) for n in calls]
        emitted = bookkeeping(gen, replay, outs)
        assert sum(o['env_steps'] for o in outs) == int(replay.length[:emitted].sum())
        runs[key] = (emitted, ring_rows(replay, gen, list(range(emitted))))
    n = min(runs['one'][0], runs['two'][0])
    assert n >= 32
    same({k: v[:32] for k, v in runs['one'][1].items()}, {k: v[:32] for k, v in runs['two'][1].items()})
    # a game's row does not depend on E: the games both runs emitted, by number (the forward's batch differs, so
    # the net's outputs agree to rounding and everything the rules and the sampling decide agrees exactly)
    a, b = runs['one'][1], runs['few'][1]
    ia = {int(g): i for i, g in enumerate(a['game'])}
    common = [(ia[int(g)], j) for j, g in enumerate(b['game']) if int(g) in ia]
    assert len(common) >= 12
    for i, j in common:
        for k in ('obs', 'action', 'tmask', 'omask', 'amask', 'length', 'outcome'):
            assert torch.equal(a[k][i], b[k][j]), (k, int(a['game'][i]))
        assert float((a['policy'][i] - b['policy'][j]).abs().max()) <= 1e-5


def test_a_game_of_full_length_is_harvested_whole():
    """A game at step 198 with every goose alive, put into slot 0 by load_games: one more step ends it at
    L = Tm = 199, the last slot of the records."""
    gen, replay, _ = make('geese', 'cpu', 2, 8, seed=3, check_every=1)
    st = gen._state()
    st['pending'].zero_()                        # the constructor's games stay in the slots
    late = geese.new_game(3, 77)
    late['step'] = 198
    gen.env.load_games([late], [0])
    st['ply'][0] = st['played'][0] = 198
    st['game'][0] = 77
    st['obs'][0].fill_(1)                        # the plies before the injection: whatever the slot holds
    out = gen.generate(1)
    assert out['plies'] == 1 and out['episodes'] >= 1
    row = gen.ring_game.tolist().index(77)
    assert int(replay.length[row]) == geese.MAX_PLIES == 199
    assert bool((replay.obs[row, :198] == 1).all())
    assert replay.tmask[row, 198].tolist() == [True] * 4
    for p in range(4):
        assert torch.equal(replay.obs[row, 198, p].float(), torch.from_numpy(geese.observation_of(late, p)))
    geese.step_game(late, replay.action[row, 198].tolist(), 3)
    assert late['step'] == 199 and not late['live']
    assert replay.outcome[row].tolist() == [float(np.float32(x)) for x in geese.outcome_of(late)]
    assert int(st['ply'][0]) == 0 and int(st['game'][0]) >= 2


def _harvest_state(E, Tm, P, A, w, g):
    return {'obs': torch.randint(0, 2, (E, Tm, P, w), generator=g, dtype=torch.uint8),
            'policy': torch.randn(E, Tm, P, A, generator=g), 'amask': torch.randn(E, Tm, P, A, generator=g),
            'action': torch.randint(0, A, (E, Tm, P), generator=g), 'value': torch.randn(E, Tm, P, generator=g),
            'tmask': torch.rand(E, Tm, P, generator=g) < 0.5, 'omask': torch.rand(E, Tm, P, generator=g) < 0.5,
            'rows': torch.arange(E)}


def test_ring_wrap_and_more_done_slots_than_rows():
    # play: N = 3 rows, E = 5 slots
    gen, replay, cpu = make('ptt', 'cpu', 5, 3, seed=9)
    outs = [gen.generate(4), gen.generate(7)]
    emitted = bookkeeping(gen, replay, outs)
    assert emitted >= 11 and replay.count == 3 and replay.ptr == emitted % 3
    referee(ParallelGame, gen, replay, cpu, [0, 1, 2])
    newest = sorted(gen.ring_game.tolist())
    assert int(gen.ring_game[replay.ptr]) == newest[0]
    # c = 4 done slots > N = 3 rows in one call: the highest slot that claims a row wins
    E, Tm, P, A, N = 5, 4, 2, 3, 3
    g = torch.Generator().manual_seed(1)
    st = _harvest_state(E, Tm, P, A, 6, g)
    st.update(ply=torch.tensor([2, 4, 3, 1, 3]), game=torch.tensor([10, 11, 12, 13, 14]),
              pending=torch.zeros(E, dtype=torch.bool), state=torch.tensor([1, 100, 50]))
    rep = PlayerReplay(N, Tm, (6,), A, P, 'cpu', obs_dtype=torch.uint8)
    ring_game = torch.full((N,), -1, dtype=torch.long)
    outcome = torch.randn(E, P, generator=g)
    done = torch.tensor([1, 1, 0, 1, 1], dtype=torch.bool)
    lengths = st['ply'].clone()
    rollout.harvest_players_torch(st, done, outcome, GAMMA, rep, ring_game)
    # slots 0, 1, 3, 4 -> rows 1, 2, 0, 1: row 1 keeps slot 4
    assert ring_game.tolist() == [13, 14, 11]
    for row, e in ((0, 3), (1, 4), (2, 1)):
        L = int(lengths[e])
        assert int(rep.length[row]) == L and torch.equal(rep.outcome[row], outcome[e])
        for k in ('policy', 'amask', 'action', 'value', 'tmask', 'omask'):
            assert torch.equal(getattr(rep, k)[row, :L], st[k][e, :L]), (k, row)
        assert torch.equal(rep.obs[row, :L], st['obs'][e, :L]) and not bool(rep.obs[row, L:].any())
        assert not bool(rep.policy[row, L:].any()) and bool((rep.amask[row, L:] == 1e32).all())
        assert not bool(rep.tmask[row, L:].any()) and not bool(rep.omask[row, L:].any())
    assert st['state'].tolist() == [(1 + 4) % 3, 104, 54]
    assert st['game'].tolist() == [50, 51, 12, 52, 53] and st['ply'].tolist() == [0, 0, 3, 0, 0]
    assert st['pending'].tolist() == [True, True, False, True, True]


def test_out_of_scope_requests_name_the_lockstep_generator():
    cls = ParallelTicTacToeBatch
    preplay = PlayerReplay(8, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P, 'cpu')
    replay = DeviceReplay(8, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P, 'cpu')
    net = SimpleConv2dModel()

    class Recurrent(SimpleConv2dModel):
        def init_hidden(self, batch_size=None):
            return None
    for env, n, rep in ((TicTacToeBatch(4, 'cpu'), net, preplay), (cls(4, 'cpu'), Recurrent(), preplay),
                        (cls(4, 'cpu'), net, replay),
                        (cls(4, 'cpu'), net, PlayerReplay(8, cls.MAX_PLIES, cls.OBS_SHAPE, 4, cls.P, 'cpu'))):
        with pytest.raises(ValueError, match='DeviceGenerator'):
            PlayerStreamGenerator(env, n, rep)
    PlayerStreamGenerator(cls(4, 'cpu'), net, preplay)
