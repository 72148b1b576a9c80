"""The replay's new Python surface on the CPU: the torch formulation of the integer draw rule (the reference of
hrl_replay_draw's GPU test), ``out=`` / ``alloc_batch`` on the torch path, the ``draw`` switch.
"""

import numpy as np
import pytest
import torch

from handyrl_amd import rollout

CPU = torch.device('cpu')


def _ring(N=10, count=10, ptr=0, M=20, Tm=9, P=2, **kw):
    rep = rollout.DeviceReplay(N, Tm, (3, 3, 3), 9, P, CPU, maximum_episodes=M, **kw)
    rep.count, rep.ptr = count, ptr
    rep.length.fill_(Tm)
    return rep


def test_integer_rule_follows_the_recency_weighting():
    """test_rollout.py::test_window_choice_recency_weighting's setup and tolerance for ``draw_windows``."""
    rep = _ring()
    slots, start, players = rep.draw_windows(200000, 9, generator=torch.Generator().manual_seed(0))
    freq = torch.bincount(slots, minlength=10).double() / slots.numel()
    w = 1 - (9 - torch.arange(10, dtype=torch.float64)) / 20
    assert torch.allclose(freq, w / w.sum(), atol=4e-3)
    assert int(start.max()) == 0
    assert torch.allclose(torch.bincount(players, minlength=2).double() / players.numel(),
                          torch.full((2,), 0.5, dtype=torch.float64), atol=4e-3)


@pytest.mark.parametrize('N,count,ptr,M', [(16, 8, 8, 16), (16, 16, 5, 16), (16, 12, 12, 6), (16, 1, 1, 16),
                                           (16, 16, 3, 1), (7, 7, 6, 100)])
def test_integer_rule_equals_a_scalar_search(N, count, ptr, M):
    """The vectorised formulation against the rule written out per window in Python integers."""
    Tm, T, P = 9, 3, 3
    rep = _ring(N, count, ptr, M, Tm, P)
    g = torch.Generator().manual_seed(2)
    rep.length = torch.randint(1, Tm + 1, (N,), generator=g)
    n = min(count, M)
    C = [(i + 1) * (M - n + 1) + i * (i + 1) // 2 for i in range(n)]
    one = float(np.nextafter(np.float32(1), np.float32(0)))
    u = torch.rand(3, 300, generator=g)
    edges = torch.tensor([c / C[-1] for c in C], dtype=torch.float64).float().clamp_(max=one)
    u[0, :n] = edges
    u[0, n:n + 2] = torch.tensor([0.0, one])
    slots, start, players = rep.draw_windows(300, T, u=u)
    for b in range(300):
        x = int(np.floor(float(u[0, b]) * float(C[-1])))
        pick = next((i for i in range(n) if C[i] > x), n - 1)
        slot = (ptr - n + pick) % N
        cand = 1 + max(int(rep.length[slot]) - T, 0)
        assert int(slots[b]) == slot
        assert int(start[b]) == min(int(np.float32(u[1, b]) * np.float32(cand)), cand - 1)
        assert int(players[b]) == min(int(np.float32(u[2, b]) * np.float32(P)), P - 1)


def test_draw_switch_and_errors():
    with pytest.raises(ValueError):
        rollout.DeviceReplay(4, 9, (3, 3, 3), 9, 2, CPU, draw='uniform')
    with pytest.raises(ValueError):
        rollout.PlayerReplay(4, 9, (3, 3, 3), 9, 2, CPU, draw='uniform')
    with pytest.raises(ValueError):
        _ring(count=0).draw_windows(4, 3)
    assert rollout.DeviceReplay(4, 9, (3, 3, 3), 9, 2, CPU).draw == 'multinomial'
    assert rollout.FUSED_GATHER is True


def _random_player_ring(solo, mover, seed=0):
    g = torch.Generator().manual_seed(seed)
    rep = rollout.PlayerReplay(6, 5, {'a': (3,), 'b': (2, 2)}, 4, 3, CPU, solo=solo, mover=mover, draw='inverse')
    rep.obs = {k: torch.randn(v.shape, generator=g) for k, v in rep.obs.items()}
    rep.policy, rep.value = torch.randn(rep.policy.shape, generator=g), torch.randn(rep.value.shape, generator=g)
    rep.tmask = torch.rand(rep.tmask.shape, generator=g) < 0.5
    rep.omask = torch.rand(rep.omask.shape, generator=g) < 0.5
    rep.length = torch.randint(1, 6, (6,), generator=g)
    rep.count = 6
    return rep


@pytest.mark.parametrize('solo,mover', [(False, False), (True, False), (False, True)])
def test_out_is_filled_and_returned_on_the_torch_path(solo, mover):
    rep = _random_player_ring(solo, mover)
    B, T = 7, 4
    out = rep.alloc_batch(B, T)
    got = rep.sample(B, T, generator=torch.Generator().manual_seed(5), out=out)
    assert got is out
    ref = rep.sample(B, T, generator=torch.Generator().manual_seed(5))
    assert set(ref) == set(out)
    for k in ref:
        for a, b in zip(rollout._leaves(out[k]), rollout._leaves(ref[k])):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), k


def test_sample_windows_stream_is_unchanged_by_the_new_keywords():
    rep = _ring()
    a = rep.sample(8, 4, generator=torch.Generator().manual_seed(3))
    b = rep.sample(8, 4, generator=torch.Generator().manual_seed(3), out=rep.alloc_batch(8, 4))
    for k in a:
        assert torch.equal(a[k], b[k]), k
