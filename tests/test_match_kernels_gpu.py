"""hrl_match_act against its torch formulation (evaluation.match_act_torch), bit for bit, on guard-band buffers
(tests/guarded.py): a store outside a buffer or into a slot that must store nothing fails the run.  The buffers
indexed by game number have exactly G rows for the kernel (the torch ops use a spare row G for the slots that store
nothing).  Without an opponent and without opening plies the kernel is hrl_eval_act."""

import numpy as np
import pytest
import torch

from handyrl_amd import evaluation as ev
from tests.guarded import Arena, bits

pytestmark = pytest.mark.gpu

ES = (1, 5, 64, 67)          # one wave, less than a workgroup of 4 slots, whole workgroups, a ragged last one
AS = (1, 9, 65, 214)         # one label, TicTacToe, one label past a wave, Geister (3.3 waves)
TM = 5
TEMPS = ((0.0, 0.0), (0.0, 0.5), (0.5, 0.0))
SEED = 12345


def _same(a, b, what):
    assert torch.equal(bits(a), bits(b)), what


def _slots(rng, E, G, P, seats, mover, dev, big=False):
    """E slots: distinct game numbers; every fourth slot retired (game = G), every fifth waiting (inactive with a
    game), slot E-2 active at ply == Tm (stores nothing), the rest active at a ply in [0, Tm)."""
    if big:
        game = torch.from_numpy(np.concatenate([rng.integers(1 << 32, 1 << 40, E - E // 2),
                                                (1 << 40) - 1 - np.arange(E // 2)]).astype(np.int64))
    else:
        game = torch.from_numpy(rng.permutation(G)[:E].astype(np.int64))
    ply = torch.from_numpy(rng.integers(0, TM, E))
    active = torch.ones(E, dtype=torch.bool)
    e = torch.arange(E)
    if E > 1:
        active[(e % 4 == 3) | (e % 5 == 4)] = False
        game[e % 4 == 3] = G
        if E > 2:
            ply[E - 2] = TM
    seat = {'rule': game % P, 'home': torch.full((E,), mover), 'away': torch.full((E,), (mover + 1) % P)}[seats]
    st = {'Tm': TM, 'P': P, 'game': game, 'ply': ply, 'active': active, 'seat': seat.long()}
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in st.items()}


def _legal(rng, E, A, mode):
    legal = torch.zeros(E, A, dtype=torch.bool)
    if mode == 'single':
        legal[torch.arange(E), torch.from_numpy(rng.integers(0, A, E))] = True
    elif mode == 'all':
        legal[:] = True
    elif mode == 'last':
        legal[:, A - 1] = True
    else:
        legal = torch.from_numpy(rng.random((E, A)) < 0.4)
        legal[torch.arange(E), torch.from_numpy(rng.integers(0, A, E))] = True
    return legal


def _logits(rng, E, A, mode, stride):
    x = torch.from_numpy(rng.standard_normal((E, stride)).astype(np.float32))
    if mode == 'equal':
        x.fill_(0.25)
    elif mode == 'nan':
        x[torch.arange(E), torch.from_numpy(rng.integers(0, A, E))] = float('nan')
    return x


def _trace(G, A, dev, rows):
    g = torch.Generator().manual_seed(1)
    return {'action': torch.randint(-9, -1, (rows, TM), generator=g).to(dev),
            'picked': torch.randint(-9, -1, (rows, TM), generator=g).to(dev),
            'policy': torch.rand(rows, TM, A, generator=g).to(dev),
            'model_ply': (torch.rand(rows, TM, generator=g) < 0.5).to(dev)}


def _run(cuda, E, A, P=2, mover=0, seats='rule', legal_mode='mixed', modes=('random', 'random'), temps=(0.0, 0.0),
         opening=0, opp=True, forced_on=False, trace_on=False, seed=0, big=False):
    rng = np.random.default_rng([E, A, P, mover, seed])
    G = (1 << 40) if big else E + 3
    st = _slots(rng, E, G, P, seats, mover, cuda, big)
    home = _logits(rng, E, A, modes[0], A + (3 if E % 2 else 0)).to(cuda)
    away = _logits(rng, E, A, modes[1], A + 5).to(cuda) if opp else None     # stride_opp > A, and not the home stride
    legal = _legal(rng, E, A, legal_mode).to(cuda)
    forced = None
    if forced_on:
        forced = torch.from_numpy(np.where(rng.random((G + 1, TM)) < 0.5, rng.integers(0, A, (G + 1, TM)), -1)).to(cuda)
    ref_tr = _trace(G, A, cuda, G + 1) if trace_on else None
    want = ev.match_act_torch(st, home, away, legal, mover, SEED, temps[0], temps[1], opening, G, forced, ref_tr)
    arena = Arena(cuda)
    hip_st = dict(st)
    for k in ('game', 'ply', 'active', 'seat'):
        hip_st[k] = arena.inout(st[k], name=k)
    tr = None
    if trace_on:
        tr = {k: arena.inout(v[:G], name='trace_' + k) for k, v in _trace(G, A, cuda, G + 1).items()}
    f = None if forced is None else arena.inout(forced[:G].contiguous(), name='forced')
    lh = arena.inout(home, name='logits_home')
    lo = arena.inout(away, name='logits_opp') if opp else None
    lm = arena.inout(legal, name='legal')
    got = ev.match_act_hip(hip_st, lh, lo, lm, mover, SEED, temps[0], temps[1], opening, G, f, tr)
    arena.check()
    what = (E, A, P, mover, seats, legal_mode, modes, temps, opening, opp, forced_on, trace_on)
    _same(got, want, what)
    assert int(got[~st['active']].abs().sum()) == 0
    for k in ('game', 'ply', 'active', 'seat'):
        _same(hip_st[k], st[k], (k,) + what)          # inputs untouched
    _same(lh, home, what)
    if trace_on:
        for k in tr:
            _same(tr[k], ref_tr[k][:G], (k,) + what)
    return {'got': got, 'st': st, 'legal': legal, 'home': home, 'away': away, 'trace': tr, 'forced': forced, 'G': G}


@pytest.mark.parametrize('A', AS)
@pytest.mark.parametrize('E', ES)
def test_match_act_equals_torch_formulation(cuda, E, A):
    """Every legal set x temperature pair x opening in {0, 1, Tm}; P in {2, 3}, every mover, the seat assignments,
    the logit patterns (random, an exact tie, a NaN in either net) and forced / trace cycle through them."""
    patterns = (('random', 'random'), ('equal', 'equal'), ('nan', 'random'), ('random', 'nan'))
    n = 0
    for legal_mode in ('single', 'all', 'last', 'mixed'):
        for temps in TEMPS:
            for opening in (0, 1, TM):
                P = 2 + n % 2
                _run(cuda, E, A, P=P, mover=(n // 2) % P, seats=('rule', 'home', 'away')[n % 3], legal_mode=legal_mode,
                     modes=patterns[(n // 3) % 4], temps=temps, opening=opening, forced_on=n % 4 in (1, 3),
                     trace_on=n % 4 in (2, 3), seed=n)
                n += 1
    for P in (2, 3):                                   # both (all) movers with every forced / trace pair
        for mover in range(P):
            for forced_on in (False, True):
                for trace_on in (False, True):
                    _run(cuda, E, A, P=P, mover=mover, opening=1, temps=(0.5, 0.0), forced_on=forced_on,
                         trace_on=trace_on, seed=90 + mover)


@pytest.mark.parametrize('A', AS)
def test_each_seat_plays_its_own_net(cuda, A):
    """Distinct nets: past the opening the home rows follow logits_home and the others logits_opp; an exact tie goes
    to the lowest legal label and a NaN logit wins, in either net; an opening ply is eval_pick and still traces the
    mover's policy; a forced move changes the action and not ``picked``."""
    E = 67

    def live_of(r):
        st = r['st']
        live = st['active'] & (st['ply'] < TM)
        return live, st['game'][live], st['ply'][live]

    for seats in ('home', 'away'):
        r = _run(cuda, E, A, seats=seats, trace_on=True, seed=5)
        live, g, t = live_of(r)
        p = r[seats][:, :A] - torch.where(r['legal'], 0.0, 1e32)
        assert torch.equal(r['got'][live], p.argmax(-1)[live])
        _same(r['trace']['policy'][g, t], p[live], seats)
        assert bool((r['trace']['model_ply'][g, t] == (seats == 'home')).all())
        # every ply an opening ply: eval_pick whichever net would move, the policy still traced
        r = _run(cuda, E, A, seats=seats, opening=TM, trace_on=True, seed=5)
        legal = r['legal'].cpu()
        for e in live.nonzero().flatten().tolist():
            want = ev.eval_pick(SEED, int(r['st']['game'][e]), int(r['st']['ply'][e]), legal[e].tolist())
            assert int(r['got'][e]) == want, (seats, e)
        _same(r['trace']['policy'][g, t], p[live], seats)
        r = _run(cuda, E, A, seats=seats, forced_on=True, trace_on=True, seed=5)
        f = r['forced'][g, t]
        assert torch.equal(r['trace']['picked'][g, t], p.argmax(-1)[live])
        assert torch.equal(r['trace']['action'][g, t], torch.where(f >= 0, f, p.argmax(-1)[live]))
        # an exact tie and a NaN
        r = _run(cuda, E, A, seats=seats, modes=('equal', 'equal'), seed=6)
        live = live_of(r)[0]
        assert torch.equal(r['got'][live], r['legal'].long().argmax(-1)[live])
        r = _run(cuda, E, A, seats=seats, legal_mode='all', modes=('nan', 'nan'), seed=7)
        live = live_of(r)[0]
        assert torch.equal(r['got'][live], torch.isnan(r[seats][:, :A]).long().argmax(-1)[live])


@pytest.mark.parametrize('A', (9, 214))
def test_game_numbers_up_to_2_40(cuda, A):
    """Game numbers with a high counter word, both nets at a temperature and one opening ply: the streams and
    eval_pick are addressed by the whole 64-bit number (no trace: the buffers would have 2**40 rows)."""
    for mover, temps in ((0, (0.5, 0.25)), (1, (0.0, 0.5))):
        r = _run(cuda, 67, A, mover=mover, temps=temps, opening=1, big=True, seed=3)
        assert int(r['st']['game'].max()) == (1 << 40)           # the retired slots' number, G itself
        assert int(r['st']['game'][r['st']['active']].max()) >= (1 << 40) - 67


@pytest.mark.parametrize('A', AS)
@pytest.mark.parametrize('E', ES)
def test_without_opponent_and_opening_it_is_eval_act(cuda, E, A):
    """logits_opp = NULL, opening = 0: the action and the four trace records equal hrl_eval_act's bit for bit."""
    n = 0
    for legal_mode in ('single', 'all', 'last', 'mixed'):
        for mode in ('random', 'equal', 'nan'):
            for temperature in (0.0, 0.5):
                mover, forced_on = n % 2, n % 3 == 1
                r = _run(cuda, E, A, mover=mover, legal_mode=legal_mode, modes=(mode, 'random'),
                         temps=(temperature, 0.25), opp=False, forced_on=forced_on, trace_on=True, seed=n)
                G = r['G']
                tr = _trace(G, A, cuda, G + 1)
                tr = {k: v[:G].contiguous() for k, v in tr.items()}
                f = None if r['forced'] is None else r['forced'][:G].contiguous()
                a = ev.act_hip(r['st'], r['home'], r['legal'], mover, SEED, temperature, G, f, tr)
                _same(a, r['got'], (E, A, legal_mode, mode, temperature))
                for k in tr:
                    _same(tr[k], r['trace'][k], (k, E, A, legal_mode, mode, temperature))
                n += 1
