"""csrc/hrl_geese.hip against the CPU batch (the Python rules): every state tensor after every ply, inactive games
and guard bands bit-identical, the clause positions, reset_where, and the four views with their record."""

import numpy as np
import pytest
import torch

from handyrl_amd import _native
from handyrl_amd.envs import geese
from handyrl_amd.envs.geese import HungryGeeseBatch
from tests.geese_games import CLAUSES, SEED, played, run_clause
from tests.guarded import Arena

pytestmark = pytest.mark.gpu

NAMES = [name for name, _, _ in geese._STATE]
VIEW = (17, 7, 11)


def _guarded_batch(E, cuda, arena):
    """A device batch whose state lives in guard-band buffers, reset to games 0 .. E - 1 by the kernel."""
    batch = HungryGeeseBatch(E, cuda, seed=SEED)
    for name in NAMES:
        setattr(batch, name, arena.inout(getattr(batch, name), name=name))
    batch.next_game = 0
    batch.reset()
    return batch


def _assert_same_state(dev, cpu, what):
    for name, a, b in zip(NAMES, dev.state_tensors(), cpu.state_tensors()):
        assert torch.equal(a.cpu(), b), (name, what)


def _lockstep(cuda, policy, games, E, skip_even_once=False):
    recs, _ = played(policy, games)
    arena = Arena(cuda)
    dev, cpu = _guarded_batch(E, cuda, arena), HungryGeeseBatch(E, 'cpu', seed=SEED)
    _assert_same_state(dev, cpu, 'reset')
    for lo in range(0, games, E):
        if lo:
            dev.reset()
            cpu.reset()
            _assert_same_state(dev, cpu, ('reset', lo))
        chunk = recs[lo:lo + E]
        for t in range(max(len(r['actions']) for r in chunk)):
            actions = torch.zeros(E, 4, dtype=torch.long)
            active = torch.zeros(E, dtype=torch.bool)
            for e, r in enumerate(chunk):
                if t < len(r['actions']):
                    actions[e] = torch.tensor(r['actions'][t])
                    active[e] = True
            if skip_even_once and t == 1:
                # games that are live but not active this time stay as they are, on both sides
                hold = active.clone()
                hold[::2] = False
                dev.step_players(actions.to(cuda), None, hold.to(cuda), None)
                cpu.step_players(actions, None, hold, None)
                _assert_same_state(dev, cpu, (lo, t, 'hold'))
                active &= ~hold
            dev.step_players(actions.to(cuda), None, active.to(cuda), None)
            cpu.step_players(actions, None, active, None)
            _assert_same_state(dev, cpu, (lo, t))
        assert not bool(cpu.active()[:len(chunk)].any())
    arena.check()


def test_reset_and_step_equal_the_cpu_batch_no_reversal_policy(cuda):
    _lockstep(cuda, 'no_reversal', 256, 64)


def test_reset_and_step_equal_the_cpu_batch_uniform_policy(cuda):
    _lockstep(cuda, 'uniform', 64, 64)


def test_reset_and_step_at_a_size_that_is_no_multiple_of_a_wave(cuda):
    _lockstep(cuda, 'no_reversal', 67, 67, skip_even_once=True)


def test_clause_positions(cuda):
    names = sorted(CLAUSES)
    arena = Arena(cuda)
    dev = _guarded_batch(len(names), cuda, arena)
    dev.load_games([CLAUSES[n][0] for n in names], range(len(names)))
    assert dev.dump_games() == [CLAUSES[n][0] for n in names]
    want = {n: run_clause(n) for n in names}
    for t in range(2):
        active = torch.tensor([t < len(CLAUSES[n][1]) for n in names])
        actions = torch.tensor([CLAUSES[n][1][min(t, len(CLAUSES[n][1]) - 1)] for n in names])
        dev.step_players(actions.to(cuda), None, active.to(cuda), None)
        got = dev.dump_games()
        for n, g in zip(names, got):
            assert g == want[n][min(t, len(want[n]) - 1)], (n, t)
    arena.check()


def test_reset_where(cuda):
    arena = Arena(cuda)
    dev, cpu = _guarded_batch(67, cuda, arena), HungryGeeseBatch(67, 'cpu', seed=SEED)
    actions = torch.arange(67 * 4).view(67, 4) % 4
    for _ in range(2):
        dev.step_players(actions.to(cuda), None, dev.active().clone(), None)
        cpu.step_players(actions, None, cpu.active().clone(), None)
    mask = torch.arange(67) % 3 == 1
    dev.reset_where(mask.to(cuda))
    cpu.reset_where(mask)
    _assert_same_state(dev, cpu, 'reset_where')
    assert dev.next_game == cpu.next_game == 67 + int(mask.sum())
    assert dev.game.cpu()[mask].tolist() == list(range(67, 67 + int(mask.sum())))
    arena.check()


def _positions(E):
    """E game states of every kind: fresh, mid-game with dead geese, long geese, finished."""
    recs, _ = played('no_reversal', 256)
    out = [recs[0]['start']]
    for r in recs:
        out += [r['states'][len(r['states']) // 2], r['states'][-1], r['states'][0]]
    long_ones = sorted((s for r in recs for s in r['states'][::7]), key=lambda s: -max(len(g) for g in s['geese']))
    return (long_ones[:8] + out)[:E]


def _observe(batch, views, rec, t, infer, Tm):
    ptr = _native.ptr
    _native.check(_native.load().hrl_geese_observe(
        ptr(batch.body), ptr(batch.head), ptr(batch.length), ptr(batch.food), ptr(batch.prev), ptr(views), ptr(rec),
        ptr(t), ptr(infer), batch.E, 4, Tm, _native.stream_of(views.device)), 'hrl_geese_observe')


@pytest.mark.parametrize('E', [1, 67])
def test_observe_views_and_record(cuda, E):
    states = _positions(E)
    want = np.stack([np.stack([geese.observation_of(s, p) for s in states]) for p in range(4)])   # (4, E, 17, 7, 11)
    Tm = 3
    gen = torch.Generator().manual_seed(E)
    infer = torch.rand(E, 4, generator=gen) < 0.6
    infer[0, 0], infer[-1, -1] = True, False
    for tt in (0, Tm - 1):
        arena = Arena(cuda)
        dev = _guarded_batch(E, cuda, arena)
        dev.load_games(states, range(E))
        views = arena.out((4, E, *VIEW), name='views')
        rec = arena.acc((E, Tm, 4, *VIEW), name='record')
        t = torch.full((1,), tt, dtype=torch.long, device=cuda)
        _observe(dev, views, rec, t, infer.to(cuda), Tm)
        arena.check()
        assert np.array_equal(views.cpu().numpy(), want), tt
        slot = np.where(infer.numpy()[:, :, None, None, None], want.transpose(1, 0, 2, 3, 4), 0)
        want_rec = np.zeros((E, Tm, 4, *VIEW), dtype=np.float32)
        want_rec[:, tt] = slot
        assert np.array_equal(rec.cpu().numpy(), want_rec), tt           # only slot t, only where infer
        assert dev.dump_games() == states                                # the state is read only
    # without a record: the views alone; the batch's own methods and the torch formulation agree
    arena = Arena(cuda)
    dev = _guarded_batch(E, cuda, arena)
    dev.load_games(states, range(E))
    views = arena.out((4, E, *VIEW), name='views')
    _observe(dev, views, None, None, None, 0)
    arena.check()
    assert np.array_equal(views.cpu().numpy(), want)
    assert np.array_equal(dev.views_torch().cpu().numpy(), want)
    player = (torch.arange(E) % 4).to(cuda)
    assert np.array_equal(dev.observation(player).cpu().numpy(), want[np.arange(E) % 4, np.arange(E)])
    assert np.array_equal(dev.outcome().cpu().numpy(), np.array([geese.outcome_of(s) for s in states], np.float32))


def test_a_ply_index_outside_the_record_stores_nothing(cuda):
    arena = Arena(cuda)
    dev = _guarded_batch(3, cuda, arena)
    views = arena.out((4, 3, *VIEW), name='views')
    rec = arena.acc((3, 2, 4, *VIEW), name='record')
    infer = torch.ones(3, 4, dtype=torch.bool, device=cuda)
    _observe(dev, views, rec, torch.full((1,), 2, dtype=torch.long, device=cuda), infer, 2)
    arena.check()
    assert not bool(rec.any())
