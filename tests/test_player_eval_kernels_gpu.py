"""hrl_players_act against its torch formulation (evaluation.players_act_torch) and hrl_geese_observe_seats against
the views of hrl_geese_observe gathered by (seat + k) mod 4, bit for bit, on guard-band buffers (tests/guarded.py):
a store outside a buffer or into a slot that must store nothing fails the run.  The buffers indexed by game number
have exactly G rows for the kernel (the torch ops use a spare row G for the slots that store nothing)."""

import copy

import numpy as np
import pytest
import torch

from handyrl_amd import evaluation as ev
from handyrl_amd.envs.geese import GEESE, RING, HungryGeeseBatch
from tests.geese_games import CLAUSES, SEED, played
from tests.guarded import Arena, bits

pytestmark = pytest.mark.gpu

# one slot; TicTacToe's shape; whole workgroups of 4 waves plus a ragged one; P = 5 reaches the second pick counter
# word (player 4) and A = 70 takes a second pass of the wave over the labels
SHAPES = ((1, 4, 4), (3, 2, 9), (65, 4, 4), (5, 5, 70))
TM = 5


def _same(a, b, what):
    assert torch.equal(bits(a), bits(b)), what


def _slots(rng, E, P, G, dev):
    """E slots with distinct game numbers: every fourth retired (game = G), every fifth waiting (inactive with a
    game), slot E-2 active at ply == Tm and slot E-3 active with a negative game (both store nothing), the rest
    active at a ply in [0, Tm); the seat is the rule's."""
    game = torch.from_numpy(rng.permutation(G)[:E].astype(np.int64))
    ply = torch.from_numpy(rng.integers(0, TM, E))
    active = torch.ones(E, dtype=torch.bool)
    e = torch.arange(E)
    if E > 1:
        active[(e % 4 == 3) | (e % 5 == 4)] = False
        game[e % 4 == 3] = G
        if E > 2:
            ply[E - 2] = TM
        if E > 4:
            game[E - 3] = -1
    seat = torch.where((game >= 0) & (game < G), game % P, torch.zeros_like(game))
    st = {'Tm': TM, 'P': P, 'game': game, 'ply': ply, 'active': active, 'seat': seat.long()}
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in st.items()}


def _legal(rng, E, P, A, per_player, mode):
    shape = (E, P, A) if per_player else (E, A)
    if mode == 'all':
        return torch.ones(shape, dtype=torch.bool)
    legal = torch.from_numpy(rng.random(shape) < 0.4)
    legal[..., int(rng.integers(0, A))] = True
    if mode == 'last':
        legal[..., :A - 1] = False
        legal[..., A - 1] = True
    return legal


def _logits(rng, rows, A, mode, stride):
    x = torch.from_numpy(rng.standard_normal((rows, stride)).astype(np.float32))
    if mode == 'equal':
        x.fill_(0.25)
    elif mode == 'pairs':                    # exact ties between labels, not all equal
        x = torch.from_numpy(rng.integers(0, 2, (rows, stride)).astype(np.float32))
    elif mode == 'nan':
        x[torch.arange(rows), torch.from_numpy(rng.integers(0, A, rows))] = float('nan')
    return x


def _trace(G, P, A, dev, rows):
    g = torch.Generator().manual_seed(1)
    return {'action': torch.randint(-9, -1, (rows, TM, P), generator=g).to(dev),
            'picked': torch.randint(-9, -1, (rows, TM, P), generator=g).to(dev),
            'policy': torch.rand(rows, TM, P, A, generator=g).to(dev),
            'alive': (torch.rand(rows, TM, P, generator=g) < 0.5).to(dev)}


def _run(cuda, E, P, A, opp_on, per_player, legal_mode, logit_mode, temps, opening, forced_on, trace_on, seed=0):
    rng = np.random.default_rng([E, P, A, seed])
    G = E + 3
    st = _slots(rng, E, P, G, cuda)
    stride = A + (3 if seed % 2 else 0)               # rows with a stride beyond A
    home = _logits(rng, E, A, logit_mode, stride).to(cuda)
    opp = _logits(rng, (P - 1) * E, A, logit_mode, stride + 1).to(cuda) if opp_on else None
    legal = _legal(rng, E, P, A, per_player, legal_mode).to(cuda)
    turns = torch.from_numpy(rng.random((E, P)) < 0.75).to(cuda)        # dead players in live games
    forced = None
    if forced_on:
        forced = torch.from_numpy(np.where(rng.random((G + 1, TM, P)) < 0.5, rng.integers(0, A, (G + 1, TM, P)),
                                           -1)).to(cuda)
    ref_tr = _trace(G, P, A, cuda, G + 1) if trace_on else None
    want_a, want_u = ev.players_act_torch(st, home, opp, legal, turns, 12345, temps[0], temps[1], opening, G, forced,
                                          ref_tr)
    arena = Arena(cuda)
    hip_st = dict(st)
    for k in ('game', 'ply', 'active', 'seat'):
        hip_st[k] = arena.inout(st[k], name=k)
    tr = None
    if trace_on:
        tr = {k: arena.inout(v[:G], name='trace_' + k) for k, v in _trace(G, P, A, cuda, G + 1).items()}
    f = None if forced is None else arena.inout(forced[:G].contiguous(), name='forced')
    lh = arena.inout(home, name='home')
    lo = None if opp is None else arena.inout(opp, name='opp')
    lm = arena.inout(legal, name='legal')
    tm = arena.inout(turns, name='turns')
    got_a, got_u = ev.players_act_hip(hip_st, lh, lo, lm, tm, 12345, temps[0], temps[1], opening, G, f, tr)
    arena.check()
    what = (E, P, A, opp_on, per_player, legal_mode, logit_mode, temps, opening, forced_on, trace_on)
    _same(got_a, want_a, what)
    _same(got_u, want_u, what)
    ok = st['active'] & (st['ply'] < TM) & (st['game'] >= 0) & (st['game'] < G)
    assert int(got_a[~(turns & ok.view(-1, 1))].abs().sum()) == 0
    for k in ('game', 'ply', 'active', 'seat'):
        _same(hip_st[k], st[k], (k,) + what)          # inputs untouched
    if trace_on:
        for k in tr:
            _same(tr[k], ref_tr[k][:G], (k,) + what)
    return got_a


@pytest.mark.parametrize('E,P,A', SHAPES)
def test_players_act_equals_torch_formulation(cuda, E, P, A):
    """With and without an opponent, both legal strides, every logit pattern (exact ties, a NaN), both temperatures,
    opening plies, forced moves and the trace on and off, over slots that are inactive, retired, out of range or
    have dead players."""
    n = 0
    for opp_on in (False, True):
        for per_player in (False, True):
            for logit_mode in ('random', 'equal', 'pairs', 'nan'):
                for temps in ((0.0, 0.0), (0.5, 1.5)):
                    _run(cuda, E, P, A, opp_on, per_player, ('mixed', 'all', 'last')[n % 3], logit_mode, temps,
                         opening=(0, 2)[(n // 2) % 2], forced_on=n % 4 in (1, 3), trace_on=n % 4 in (2, 3), seed=n)
                    n += 1


def test_players_act_mixed_temperatures_and_every_forced_trace_pair(cuda):
    for forced_on in (False, True):
        for trace_on in (False, True):
            for temps in ((0.0, 0.7), (0.7, 0.0)):
                _run(cuda, 65, 4, 4, True, False, 'mixed', 'random', temps, 1, forced_on, trace_on, seed=3)


def test_players_act_ties_go_to_the_lowest_label_and_a_nan_wins(cuda):
    a = _run(cuda, 65, 4, 4, True, False, 'all', 'equal', (0.0, 0.0), 0, False, False)
    assert int(a.abs().sum()) == 0                                    # all logits equal, all legal: label 0
    rng = np.random.default_rng(5)
    E, P, A, G = 8, 4, 70, 8
    st = {'Tm': TM, 'P': P, 'game': torch.arange(E, device=cuda), 'ply': torch.zeros(E, dtype=torch.long, device=cuda),
          'active': torch.ones(E, dtype=torch.bool, device=cuda), 'seat': torch.arange(E, device=cuda) % P}
    home = torch.from_numpy(rng.standard_normal((E, A)).astype(np.float32))
    where = torch.from_numpy(rng.integers(0, A, E))
    home[torch.arange(E), where] = float('nan')
    legal = torch.ones(E, A, dtype=torch.bool, device=cuda)
    turns = torch.ones(E, P, dtype=torch.bool, device=cuda)
    a, _ = ev.players_act_hip(st, home.to(cuda), None, legal, turns, 1, 0.0, 0.0, 0, G)
    assert a[torch.arange(E), torch.arange(E) % P].tolist() == where.tolist()


# ---- hrl_geese_observe_seats ----

def _position_pool():
    """(state, the action row that follows it): one hand-built position per rule clause (dead geese, missing food,
    geese that fill two rows) and the states of seeded games."""
    pool = [(copy.deepcopy(st), rows[0]) for st, rows in CLAUSES.values()]
    for rec in played('no_reversal', 12)[0]:
        for j in range(len(rec['states']) - 1):
            pool.append((rec['states'][j], rec['actions'][j + 1]))
    return pool


def _geese_batch(cuda, E):
    """E positions of the pool; two slots in three then play one step, which moves the ring's head index from 0 to 79:
    every longer goose of those slots wraps around the ring's end."""
    pool = _position_pool()
    picks = [pool[e % len(pool)] for e in range(E)] if E > 3 else [pool[10], pool[12], pool[40]][:E]
    b = HungryGeeseBatch(E, cuda)
    b.seed(SEED)
    b.load_games([copy.deepcopy(st) for st, _ in picks], range(E))
    step = b.live.clone() & (torch.arange(E, device=cuda) % 3 != 1)
    actions = torch.tensor([a for _, a in picks], dtype=torch.long, device=cuda)
    b.step_players(actions, None, step, None)
    return b


@pytest.mark.parametrize('K', [1, 2, 4])
@pytest.mark.parametrize('E', [1, 3, 130])
def test_observe_seats_equals_the_gathered_views(cuda, E, K):
    b = _geese_batch(cuda, E)
    if E == 130:       # what the positions must cover
        head, length = b.head.long(), b.length.long()
        assert bool((length == 0).any()) and bool((length == 1).any()) and bool((b.food < 0).any())
        assert bool(((length > 1) & (head + length > RING)).any())            # a ring that wraps
    seat = (torch.arange(E, device=cuda) * 3 + 1) % GEESE
    views = b._views()                                                        # (4, E, 17, 7, 11)
    rows = torch.arange(E, device=cuda)
    want = torch.cat([views[(seat + k) % GEESE, rows] for k in range(K)])
    assert float(want.sum()) > 0
    _same(b.observe_seats(seat, K), want, (E, K))
    # the entry itself on guard bands: every word of the K * E rows written, nothing outside them
    from handyrl_amd import _native
    arena = Arena(cuda)
    out = arena.out((K, E, *b.OBS_SHAPE), name='rows')
    state = [arena.inout(t, name=n) for n, t in (('body', b.body), ('head', b.head), ('length', b.length),
                                                  ('food', b.food), ('prev', b.prev), ('seat', seat))]
    _native.check(_native.load().hrl_geese_observe_seats(*[_native.ptr(t) for t in state], _native.ptr(out), E, 4, K,
                                                         _native.stream_of(cuda)), 'hrl_geese_observe_seats')
    arena.check()
    _same(out.view(K * E, *b.OBS_SHAPE), want, (E, K, 'guarded'))
    for t, src in zip(state, (b.body, b.head, b.length, b.food, b.prev, seat)):
        _same(t, src, 'state untouched')
