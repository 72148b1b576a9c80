"""The device evaluator's C entries: exports, argument validation (before any HIP call, so no GPU is needed) and
the public rule ``evaluation.eval_pick`` against its torch twin."""

import ctypes

import numpy as np
import torch

from handyrl_amd import _native
from handyrl_amd.evaluation import eval_pick, eval_pick_torch, wp_func, eval_games
from handyrl_amd.rollout import philox4x32

EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK
NEW = ('hrl_eval_act', 'hrl_eval_finish', 'hrl_masked_rows_fill')


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def test_exports_and_abi_version():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    for name in NEW:
        assert name in _native.SIGNATURES and hasattr(lib, name), name


ACT_REQUIRED = ('logits', 'legal', 'game', 'ply', 'active', 'seat', 'action')
ACT_TRACE = ('trace_action', 'trace_picked', 'trace_policy', 'trace_model_ply')


def _act(null=(), E=5, A=9, Tm=4, P=2, G=6, stride=None, mover=0, temperature=0.0, forced=True, trace=ACT_TRACE):
    names = ACT_REQUIRED + ('forced',) + ACT_TRACE
    a = {n: None if n in null else _p(i) for i, n in enumerate(names)}
    if not forced:
        a['forced'] = None
    for n in ACT_TRACE:
        if n not in trace:
            a[n] = None
    return _native.load().hrl_eval_act(
        a['logits'], A if stride is None else stride, a['legal'], 7, temperature, a['game'], a['ply'], a['active'],
        a['seat'], mover, a['forced'], E, A, Tm, P, G, a['action'], a['trace_action'], a['trace_picked'],
        a['trace_policy'], a['trace_model_ply'], None)


def test_act_validates_arguments():
    for name in ACT_REQUIRED:
        assert _act(null=(name,)) == EINVAL, name
        assert _act(null=(name,), E=0) == EINVAL, name
    for kw in ({'E': -1}, {'A': 0}, {'Tm': 0}, {'P': 0}, {'G': -1}, {'stride': 8}, {'mover': 2}, {'mover': -1},
               {'temperature': -0.5}, {'temperature': float('nan')}):
        assert _act(**kw) == EINVAL, kw
    for k in range(1, 4):       # some but not all trace buffers
        assert _act(trace=ACT_TRACE[:k]) == EINVAL, k
    assert _act(E=0) == OK
    assert _act(E=0, forced=False, trace=()) == OK
    assert _act(E=0, G=0) == OK and _act(E=0, temperature=0.5, mover=1) == OK


FINISH_PTRS = ('terminal', 'outcome', 'active', 'ply', 'game', 'seat', 'pending', 'state', 'outcome_out',
               'length_out')


def _finish(null=(), E=5, Tm=4, P=2, G=6):
    a = {n: None if n in null else _p(i) for i, n in enumerate(FINISH_PTRS)}
    return _native.load().hrl_eval_finish(a['terminal'], a['outcome'], E, Tm, P, G, a['active'], a['ply'], a['game'],
                                          a['seat'], a['pending'], a['state'], a['outcome_out'], a['length_out'],
                                          None)


def test_finish_validates_arguments():
    for name in FINISH_PTRS:
        assert _finish(null=(name,)) == EINVAL, name
        assert _finish(null=(name,), E=0) == EINVAL, name
    for kw in ({'E': -1}, {'Tm': 0}, {'P': 0}, {'G': -1}):
        assert _finish(**kw) == EINVAL, kw
    assert _finish(E=0) == OK and _finish(E=0, G=0) == OK


def _fill(n=2, E=5, null=(), F=(8, 3), stride=(8, 5), leaf_null=None):
    dst = (ctypes.c_void_p * max(n, 1))(*[None if l == leaf_null else 4096 * (l + 1) for l in range(max(n, 1))])
    a = {'dst': dst, 'stride': _native.i64_array([stride[l % 2] for l in range(max(n, 1))]),
         'F': _native.i64_array([F[l % 2] for l in range(max(n, 1))]), 'mask': _p(40)}
    for k in null:
        a[k] = None
    return _native.load().hrl_masked_rows_fill(n, a['dst'], a['stride'], a['F'], a['mask'], E, None)


def test_rows_fill_validates_arguments():
    for name in ('dst', 'stride', 'F', 'mask'):
        assert _fill(null=(name,)) == EINVAL, name
        assert _fill(null=(name,), E=0) == EINVAL, name
    for n in (0, -1, 17):
        assert _fill(n=n) == EINVAL, n
    assert _fill(E=-1) == EINVAL and _fill(leaf_null=1) == EINVAL
    assert _fill(F=(0, 3)) == EINVAL and _fill(stride=(7, 5)) == EINVAL
    assert _fill(E=0) == OK and _fill(E=0, n=16) == OK


# ---- the public rules

def test_eval_pick_spelled_out():
    """Key and counter layout, the integer scaling and the k-th legal label in ascending order."""
    seed, game, ply = 0x299f31d0a4093822, (0x85a308d3 << 32) | 0x243f6a88, 0x131
    legal = [a % 3 != 1 for a in range(214)]
    labels = [a for a in range(214) if legal[a]]
    x = int(philox4x32((0x243f6a88, 0x85a308d3, ply, 0xffffffff), (0xa4093822, 0x299f31d0))[0])
    assert eval_pick(seed, game, ply, legal) == labels[((x >> 9) * len(labels)) >> 23]
    assert eval_pick(seed, game, ply, [False] * 8 + [True]) == 8
    # the extreme words stay inside: w = 2**23 - 1 gives k = n - 1, never n
    for n in (1, 2, 3, 70, 214, 1 << 20):
        assert (((1 << 23) - 1) * n) >> 23 == n - 1


def test_eval_pick_torch_twin_and_spread():
    g = np.random.default_rng(5)
    E, A = 512, 214
    game = torch.from_numpy(g.integers(0, 1 << 40, E))
    ply = torch.from_numpy(g.integers(0, 202, E))
    legal = torch.from_numpy(g.random((E, A)) < 0.2)
    legal[:, 7] = True
    got = eval_pick_torch(99, game, ply, legal).tolist()
    want = [eval_pick(99, int(game[e]), int(ply[e]), legal[e].tolist()) for e in range(E)]
    assert got == want
    # uniform over the legal labels: 3 labels, 3,000 (game, ply) pairs, every label within 5 sigma of a third
    picks = eval_pick_torch(1, torch.arange(3000), torch.arange(3000) % 9, torch.ones(3000, 3, dtype=torch.bool))
    counts = torch.bincount(picks, minlength=3).tolist()
    assert all(abs(c - 1000) < 5 * (3000 * (1 / 3) * (2 / 3)) ** 0.5 for c in counts), counts


def test_wp_func_and_eval_games():
    assert wp_func({}) == 0.0
    assert wp_func({1.0: 3, 0.0: 2, -1.0: 5}) == (3 + 1) / 10
    # train.py:429-430, 564: at least update_episodes ** 0.85 games
    assert eval_games(0.1, 200) == int(np.ceil(max(0.1, 200 ** 0.85 / 200) * 200)) == 91
    assert eval_games(0.5, 16) == 11 and eval_games(1.0, 16) == 16
