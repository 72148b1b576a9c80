"""hrl_eval_act, hrl_eval_finish and hrl_masked_rows_fill against their torch formulation (handyrl_amd.evaluation),
bit for bit, on guard-band buffers (tests/guarded.py): a store outside a buffer or into a slot that must store
nothing fails the run.  The buffers indexed by game number have exactly G rows for the kernels (the torch ops use a
spare row G for the slots that store nothing)."""

import numpy as np
import pytest
import torch

from handyrl_amd import evaluation as ev
from tests.guarded import Arena, bits

pytestmark = pytest.mark.gpu

ES = (1, 5, 64, 67)          # one wave, less than a workgroup of 4 slots, whole workgroups, a ragged last one
AS = (1, 9, 65, 214)         # one label, TicTacToe, one label past a wave, Geister (3.3 waves)
TM, P = 5, 2


def _same(a, b, what):
    assert torch.equal(bits(a), bits(b)), what


def _slots(rng, E, G, seats, mover, dev):
    """E slots: distinct game numbers; every fourth slot retired (game = G), every fifth waiting (inactive with a
    game), slot E-2 active at ply == Tm (stores nothing), the rest active at a ply in [0, Tm)."""
    game = torch.from_numpy(rng.permutation(G)[:E].astype(np.int64))
    ply = torch.from_numpy(rng.integers(0, TM, E))
    active = torch.ones(E, dtype=torch.bool)
    e = torch.arange(E)
    if E > 1:
        active[(e % 4 == 3) | (e % 5 == 4)] = False
        game[e % 4 == 3] = G
        if E > 2:
            ply[E - 2] = TM
    seat = {'rule': game % P, 'model': torch.full((E,), mover), 'random': torch.full((E,), 1 - mover)}[seats]
    st = {'Tm': TM, 'P': P, 'game': game, 'ply': ply, 'active': active, 'seat': seat.long()}
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in st.items()}


def _legal(rng, E, A, mode):
    if mode == 'single':
        legal = torch.zeros(E, A, dtype=torch.bool)
        legal[torch.arange(E), torch.from_numpy(rng.integers(0, A, E))] = True
    elif mode == 'all':
        legal = torch.ones(E, A, dtype=torch.bool)
    elif mode == 'last':
        legal = torch.zeros(E, A, dtype=torch.bool)
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


def _run_act(cuda, E, A, legal_mode, logit_mode, seats, mover, temperature, forced_on, trace_on, seed=0):
    rng = np.random.default_rng([E, A, mover, seed])
    G = E + 3
    st = _slots(rng, E, G, seats, mover, cuda)
    stride = A + (3 if E % 2 else 0)                  # rows with a stride beyond A
    logits = _logits(rng, E, A, logit_mode, stride).to(cuda)
    legal = _legal(rng, E, A, legal_mode).to(cuda)
    forced = None
    if forced_on:
        forced = torch.from_numpy(np.where(rng.random((G + 1, TM)) < 0.5, rng.integers(0, A, (G + 1, TM)), -1)).to(cuda)
    ref_tr = _trace(G, A, cuda, G + 1) if trace_on else None
    want = ev.act_torch(st, logits, legal, mover, 12345, temperature, G, forced, ref_tr)
    arena = Arena(cuda)
    hip_st = dict(st)
    for k in ('game', 'ply', 'active', 'seat'):
        hip_st[k] = arena.inout(st[k], name=k)
    tr = None
    if trace_on:
        tr = {k: arena.inout(v[:G], name='trace_' + k) for k, v in _trace(G, A, cuda, G + 1).items()}
    f = None if forced is None else arena.inout(forced[:G].contiguous(), name='forced')
    lg = arena.inout(logits, name='logits')
    lm = arena.inout(legal, name='legal')
    got = ev.act_hip(hip_st, lg, lm, mover, 12345, temperature, G, f, tr)
    arena.check()
    what = (E, A, legal_mode, logit_mode, seats, mover, temperature, forced_on, trace_on)
    _same(got, want, what)
    assert int(got[~st['active']].abs().sum()) == 0
    for k in ('game', 'ply', 'active', 'seat'):
        _same(hip_st[k], st[k], (k,) + what)          # inputs untouched
    if trace_on:
        for k in tr:
            _same(tr[k], ref_tr[k][:G], (k,) + what)
    return got, st, legal


@pytest.mark.parametrize('A', AS)
@pytest.mark.parametrize('E', ES)
def test_act_equals_torch_formulation(cuda, E, A):
    """Every legal set, logit pattern, seat assignment, mover, temperature, with and without forced and trace."""
    n = 0
    for legal_mode in ('single', 'all', 'last', 'mixed'):
        for logit_mode, seats in (('random', 'rule'), ('equal', 'model'), ('nan', 'model'), ('random', 'random')):
            for temperature in (0.0, 0.5):
                variant = n % 4
                _run_act(cuda, E, A, legal_mode, logit_mode, seats, n % P, temperature, forced_on=variant in (1, 3),
                         trace_on=variant in (2, 3), seed=n)
                n += 1
    for forced_on in (False, True):                    # every forced / trace pair at the mixed case
        for trace_on in (False, True):
            _run_act(cuda, E, A, 'mixed', 'random', 'rule', 1, 0.0, forced_on, trace_on, seed=99)


@pytest.mark.parametrize('A', AS)
def test_act_ties_nan_and_single_labels(cuda, A):
    """Equal logits: the lowest legal label.  One NaN logit: that label (torch.argmax's order).  A single legal
    label: that label on both seats."""
    E = 67
    got, st, legal = _run_act(cuda, E, A, 'mixed', 'equal', 'model', 0, 0.0, False, False)
    live = st['active'] & (st['ply'] < TM)
    assert torch.equal(got[live], legal.long().argmax(-1)[live])
    for seats in ('model', 'random'):
        got, st, legal = _run_act(cuda, E, A, 'single', 'random', seats, 0, 0.0, False, False)
        live = st['active'] & (st['ply'] < TM)
        assert torch.equal(got[live], legal.long().argmax(-1)[live])
    rng = np.random.default_rng(3)
    st = _slots(rng, E, E + 3, 'model', 0, cuda)
    logits = _logits(rng, E, A, 'nan', A).to(cuda)
    got = ev.act_hip(st, logits, torch.ones(E, A, dtype=torch.bool, device=cuda), 0, 1, 0.0, E + 3)
    live = st['active'] & (st['ply'] < TM)
    assert torch.equal(got[live], torch.isnan(logits).long().argmax(-1)[live])


@pytest.mark.parametrize('n', (1, 2, 3, 70, 214))
def test_eval_pick_equals_the_kernel(cuda, n):
    """4,096 (game, ply) pairs, game numbers up to 2**40: the kernel's random seat is eval_pick exactly."""
    E, A, Tm = 4096, 214, 202
    rng = np.random.default_rng(n)
    game = np.concatenate([np.arange(1024), rng.integers(0, 1 << 31, 1024), (1 << 32) + np.arange(1024),
                           rng.integers(1 << 32, 1 << 40, 1024)]).astype(np.int64)
    ply = rng.integers(0, Tm, E)
    labels = np.sort(rng.permutation(A)[:n])
    legal = torch.zeros(E, A, dtype=torch.bool)
    legal[:, torch.from_numpy(labels)] = True
    st = {'Tm': Tm, 'P': 2, 'game': torch.from_numpy(game).to(cuda), 'ply': torch.from_numpy(ply).to(cuda),
          'active': torch.ones(E, dtype=torch.bool, device=cuda), 'seat': torch.ones(E, dtype=torch.long, device=cuda)}
    got = ev.act_hip(st, torch.zeros(E, A, device=cuda), legal.to(cuda), 0, 0xfeedfacecafebeef, 0.0, 1 << 41).tolist()
    row = legal[0].tolist()
    want = [ev.eval_pick(0xfeedfacecafebeef, int(game[e]), int(ply[e]), row) for e in range(E)]
    assert got == want
    assert set(got) <= set(labels.tolist()) and (n > 3 or len(set(got)) == n)


def _run_finish(cuda, E, pattern, next_game, G, seed=0):
    rng = np.random.default_rng([E, seed])
    dev = cuda
    Tm = TM
    game = torch.from_numpy(rng.permutation(G)[:E].astype(np.int64)) if G >= E else torch.arange(E) % max(G, 1)
    active = torch.from_numpy(rng.random(E) < 0.8)
    e = torch.arange(E)
    terminal = {'none': torch.zeros(E, dtype=torch.bool), 'all': torch.ones(E, dtype=torch.bool),
                'ends': (e == 0) | (e == E - 1), 'length': torch.zeros(E, dtype=torch.bool),
                'mixed': torch.from_numpy(rng.random(E) < 0.5)}[pattern]
    ply = torch.from_numpy(rng.integers(0, Tm - 1, E))
    if pattern in ('all', 'ends'):
        active[0] = active[E - 1] = True
    if pattern == 'none':
        ply.clamp_(max=Tm - 3)
    if pattern == 'length':                            # ply == Tm - 1: the game ends by its length
        ply[::2] = Tm - 1
        active[0] = True
    st = {'Tm': Tm, 'P': P, 'game': game, 'ply': ply, 'active': active, 'seat': game % P,
          'pending': (~active) & torch.from_numpy(rng.random(E) < 0.5),
          'state': torch.tensor([7, next_game])}
    st = {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in st.items()}
    outcome = torch.from_numpy(rng.integers(-1, 2, (E, P)).astype(np.float32)).to(dev)
    terminal = terminal.to(dev)
    keys = ('game', 'ply', 'active', 'seat', 'pending', 'state')
    ref = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
    ref_out = torch.full((G + 1, P), 9.0, device=dev)
    ref_len = torch.full((G + 1,), -9, dtype=torch.long, device=dev)
    ev.finish_torch(ref, terminal, outcome, G, ref_out, ref_len)
    arena = Arena(dev)
    hip = dict(st)
    for k in keys:
        hip[k] = arena.inout(st[k], name=k)
    rows = max(G, 1)                                   # G == 0: a row nobody may write (an empty tensor has no pointer)
    out = arena.inout(torch.full((rows, P), 9.0, device=dev), name='outcome_out')
    ln = arena.inout(torch.full((rows,), -9, dtype=torch.long, device=dev), name='length_out')
    ev.finish_hip(hip, arena.inout(terminal, name='terminal'), arena.inout(outcome, name='outcome'), G, out, ln)
    arena.check()
    what = (E, pattern, next_game, G)
    for k in keys:
        _same(hip[k], ref[k], (k,) + what)
    _same(out[:G], ref_out[:G], ('outcome_out',) + what)
    _same(ln[:G], ref_len[:G], ('length_out',) + what)
    if G == 0:
        assert bool((out == 9.0).all()) and bool((ln == -9).all())
    return hip, st, terminal


@pytest.mark.parametrize('E', ES + (300,))
def test_finish_equals_torch_formulation(cuda, E):
    """Done patterns (none, all, slots {0, E-1}, by length at ply == Tm - 1, mixed) at every edge of the game count:
    plenty left, fewer games left than done slots, next_game one below G, G already reached."""
    G = 2 * E + 5
    for pattern in ('none', 'all', 'ends', 'length', 'mixed'):
        for next_game in (E, G - max(1, E // 3), G - 1, G):
            hip, st, terminal = _run_finish(cuda, E, pattern, next_game, G)
            done = st['active'] & (terminal | (st['ply'] + 1 >= TM))
            c = int(done.sum())
            assert hip['state'].tolist() == [7 + c, min(next_game + c, G)]
            if pattern == 'none':
                assert c == 0
            new = hip['game'][done].tolist()           # slot order: next_game, next_game + 1, ... then retired
            assert new == [min(next_game + r, G) for r in range(c)]
            assert not bool(hip['active'][done].any())
            assert torch.equal(hip['pending'][done], hip['game'][done] < G)
    _run_finish(cuda, E, 'mixed', 0, 0)                # G == 0: every done slot retires, nothing is stored


@pytest.mark.parametrize('E', ES)
def test_rows_fill_equals_masked_fill(cuda, E):
    """Up to 16 leaves, contiguous and channel slices of one stacked tensor (row stride > row length); the masks
    none, all, ends and mixed.  Rows outside the mask keep their bits."""
    rng = np.random.default_rng(E)
    arena = Arena(cuda)
    stacked = arena.inout(torch.from_numpy(rng.standard_normal((E, 3 * 8, 6, 6)).astype(np.float32)), name='stacked')
    flat = arena.inout(torch.from_numpy(rng.standard_normal((E, 37)).astype(np.float32)), name='flat')
    one = arena.inout(torch.from_numpy(rng.standard_normal((E, 1)).astype(np.float32)), name='one')
    big = arena.inout(torch.from_numpy(rng.standard_normal((E, 1030)).astype(np.float32)), name='big')
    leaves = [stacked[:, 8 * i:8 * (i + 1)] for i in range(3)] + [flat, one, big]
    e = torch.arange(E)
    for mode in ('none', 'all', 'ends', 'mixed'):
        mask = {'none': torch.zeros(E, dtype=torch.bool), 'all': torch.ones(E, dtype=torch.bool),
                'ends': (e == 0) | (e == E - 1), 'mixed': torch.from_numpy(rng.random(E) < 0.5)}[mode].to(cuda)
        want = [x.clone() for x in leaves]
        ev.rows_fill_torch(want, mask)
        ev.rows_fill_hip(leaves, mask)
        arena.check()
        for l, (a, b) in enumerate(zip(leaves, want)):
            _same(a, b, (E, mode, l))
    many = [arena.inout(torch.ones(E, 3 + l, device=cuda), name='leaf%d' % l) for l in range(16)]
    mask = (e % 2 == 0).to(cuda)
    ev.rows_fill_hip(many, mask)
    arena.check()
    for x in many:
        assert not bool(x[mask].any()) and bool((x[~mask] == 1).all())
