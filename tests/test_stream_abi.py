"""The streaming generator's C entries: exports, argument validation (before any HIP call, so no GPU is needed)
and the public sampling rule ``rollout.stream_uniforms`` against Philox4x32-10's known answers."""

import ctypes

import numpy as np
import pytest

from handyrl_amd import _native
from handyrl_amd.rollout import philox4x32, stream_uniforms

EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK
NEW = ('hrl_selfplay_sample_record_stream', 'hrl_geister_observation_record_at', 'hrl_selfplay_harvest')


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def test_exports_and_abi_version():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    for name in NEW:
        assert name in _native.SIGNATURES and hasattr(lib, name), name


# ---- hrl_selfplay_sample_record_stream

TAIL_PTRS = ('logits', 'legal', 'game', 'ply', 'value', 'active', 'player', 'reward', 'action', 'policy_buf',
             'amask_buf', 'action_buf', 'value_buf', 'turn_buf', 'reward_buf')


def _tail(null=(), E=5, A=9, Tm=4, P=2, stride=None):
    a = {n: None if n in null else _p(i) for i, n in enumerate(TAIL_PTRS)}
    return _native.load().hrl_selfplay_sample_record_stream(
        a['logits'], A if stride is None else stride, a['legal'], 7, a['game'], a['ply'], a['value'], a['active'],
        a['player'], a['reward'], E, A, Tm, P, a['action'], a['policy_buf'], a['amask_buf'], a['action_buf'],
        a['value_buf'], a['turn_buf'], a['reward_buf'], None)


def test_tail_validates_arguments():
    for name in TAIL_PTRS:
        if name not in ('reward', 'reward_buf'):
            assert _tail(null=(name,)) == EINVAL, name
            assert _tail(null=(name,), E=0) == EINVAL, name
    assert _tail(null=('reward',)) == EINVAL and _tail(null=('reward_buf',)) == EINVAL
    for kw in ({'E': -1}, {'A': 0}, {'Tm': 0}, {'P': 0}, {'stride': 8}):
        assert _tail(**kw) == EINVAL, kw
    assert _tail(E=0) == OK
    assert _tail(E=0, null=('reward', 'reward_buf')) == OK


# ---- hrl_geister_observation_record_at

OBS_PTRS = ('board', 'color', 'cnt', 'player', 'planes', 'scalar', 'active', 'ply', 'rec_planes', 'rec_scalar')


def _obs(null=(), E=5, Tm=4):
    a = {n: None if n in null else _p(i) for i, n in enumerate(OBS_PTRS)}
    return _native.load().hrl_geister_observation_record_at(
        a['board'], a['color'], a['cnt'], a['player'], E, 0, a['planes'], a['scalar'], a['active'], a['ply'], Tm,
        a['rec_planes'], a['rec_scalar'], None)


def test_observation_record_at_validates_arguments():
    for name in OBS_PTRS:
        assert _obs(null=(name,)) == EINVAL, name
    assert _obs(E=-1) == EINVAL and _obs(Tm=0) == EINVAL
    assert _obs(E=0) == OK


# ---- hrl_selfplay_harvest

HARVEST_PTRS = ('done', 'slots', 'ply', 'outcome', 'ring', 'ring_game', 'game', 'pending', 'state')
SLOT_RECORDS = ('policy', 'amask', 'action', 'value', 'turn')
RING_RECORDS = ('policy', 'amask', 'action', 'value', 'reward', 'ret', 'length', 'outcome', 'turn')


def _harvest(null=(), E=5, Tm=4, P=2, A=9, N=6, leaves=2, ring_kw=None, slot_kw=None, slot_null=(), ring_null=(),
             obs_type=(0, 1), width=(27, 18), ring_width=None, reward=True):
    slots = _native.SelfplaySlots()
    slots.E, slots.Tm, slots.P, slots.A, slots.nleaves = E, Tm, P, A, leaves
    ring = _native.ReplayRing()
    ring.N, ring.Tm, ring.P, ring.A, ring.nleaves = N, Tm, P, A, leaves
    for l in range(max(0, min(leaves, _native.REPLAY_MAX_LEAVES))):
        slots.obs[l], ring.obs[l] = 4096 * (l + 1), 4096 * (l + 20)
        slots.obs_width[l] = width[l % len(width)]
        ring.obs_width[l] = (ring_width or width)[l % len(width)]
        ring.obs_type[l] = obs_type[l % len(obs_type)]
    for i, k in enumerate(SLOT_RECORDS):
        setattr(slots, k, None if k in slot_null else 4096 * (40 + i))
    slots.reward = 4096 * 50 if reward else None
    for i, k in enumerate(RING_RECORDS):
        setattr(ring, k, None if k in ring_null else 4096 * (60 + i))
    for k, v in (slot_kw or {}).items():
        setattr(slots, k, v)
    for k, v in (ring_kw or {}).items():
        setattr(ring, k, v)
    a = {n: None if n in null else _p(80 + i) for i, n in enumerate(HARVEST_PTRS)}
    a['slots'] = None if 'slots' in null else ctypes.byref(slots)
    a['ring'] = None if 'ring' in null else ctypes.byref(ring)
    return _native.load().hrl_selfplay_harvest(a['done'], a['slots'], a['ply'], a['outcome'], 0.8, a['ring'],
                                               a['ring_game'], a['game'], a['pending'], a['state'], None)


def test_harvest_validates_arguments():
    for name in HARVEST_PTRS:
        assert _harvest(null=(name,)) == EINVAL, name
        assert _harvest(null=(name,), E=0) == EINVAL, name
    for kw in ({'E': -1}, {'Tm': 0}, {'P': 0}, {'A': 0}, {'N': 0}, {'N': -3}):
        assert _harvest(**kw) == EINVAL, kw
    for k in SLOT_RECORDS:
        assert _harvest(slot_null=(k,)) == EINVAL, k
    for k in RING_RECORDS:
        assert _harvest(ring_null=(k,)) == EINVAL, k
    # the observation leaves: count, type, width, a NULL leaf, a ring that does not match the slots
    for leaves in (0, -1, 9):
        assert _harvest(leaves=leaves) == EINVAL, leaves
    assert _harvest(ring_kw={'nleaves': 1}) == EINVAL
    assert _harvest(obs_type=(0, 2)) == EINVAL and _harvest(obs_type=(-1, 1)) == EINVAL
    assert _harvest(width=(27, 0)) == EINVAL and _harvest(width=(-5, 18)) == EINVAL
    assert _harvest(ring_width=(27, 17)) == EINVAL
    for kw in ({'Tm': 5}, {'P': 3}, {'A': 10}):
        assert _harvest(ring_kw=kw) == EINVAL, kw
    assert _harvest(E=0) == OK
    assert _harvest(E=0, reward=False) == OK and _harvest(E=0, leaves=8) == OK


# ---- the sampling rule

KNOWN = (
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     'd16cfe09 94fdcceb 5001e420 24126ea1'),
)


@pytest.mark.parametrize('counter,key,expect', KNOWN)
def test_philox_known_answers(counter, key, expect):
    assert ' '.join('%08x' % int(w) for w in philox4x32(counter, key)) == expect


def test_stream_uniforms_reproduce_the_known_answers():
    """The key and counter layout of the rule: seed -> key, (game, ply, a // 4) -> counter, word a % 4."""
    for counter, key, expect in KNOWN:
        seed = key[0] | (key[1] << 32)
        game = counter[0] | (counter[1] << 32)
        if game >= 1 << 63:
            game -= 1 << 64          # an int64 game number with the same bits
        block = counter[3]
        if 4 * (block + 1) > 1 << 20:
            continue                 # a label count nobody has; the other two cases cover the layout
        A = 4 * (block + 1)
        u = stream_uniforms(seed, game, counter[2], A)
        assert u.shape == (A,) and u.dtype == np.float32
        words = [int(w, 16) for w in expect.split()]
        want = [np.float32((w >> 9) + 0.5) * np.float32(2.0 ** -23) for w in words]
        assert [float(x) for x in u[-4:]] == [float(x) for x in want]


def test_stream_uniforms_third_known_answer_through_the_block_index():
    """The third known answer's counter word 3 (0x03707344) is a label block of its own: too many labels for one
    call, so it is reached through philox4x32 and the uniform formula, with the rule's counter spelled out."""
    counter, key, expect = KNOWN[2]
    seed, game = key[0] | (key[1] << 32), counter[0] | (counter[1] << 32)
    out = philox4x32((game & 0xffffffff, game >> 32, counter[2], counter[3]), (seed & 0xffffffff, seed >> 32))
    assert ' '.join('%08x' % int(w) for w in out) == expect


def test_stream_uniforms_key_and_counter_layout():
    seed, game, ply, A = 0x299f31d0a4093822, (0x85a308d3 << 32) | 0x243f6a88, 0x13198a2e, 11
    u = stream_uniforms(seed, game - (1 << 64), ply, A)
    for a in range(A):
        out = philox4x32((0x243f6a88, 0x85a308d3, ply, a // 4), (0xa4093822, 0x299f31d0))
        assert float(u[a]) == ((int(out[a % 4]) >> 9) + 0.5) * 2.0 ** -23, a


def test_stream_uniforms_range_and_exactness():
    u = stream_uniforms(12345, np.arange(64), 3, 214)
    assert u.shape == (64, 214)
    lo, hi = np.float32(2.0 ** -24), np.float32(1.0) - np.float32(2.0 ** -24)
    assert u.min() >= lo and u.max() <= hi
    # the extreme words: x = 0 and x = 0xffffffff stay inside, exactly
    for x, want in ((0, 2.0 ** -24), (0xffffffff, 1.0 - 2.0 ** -24)):
        got = (np.float32(x >> 9) + np.float32(0.5)) * np.float32(2.0 ** -23)
        assert float(got) == want
    # a game's uniforms depend on (seed, game, ply, label) only: a batch equals the single calls
    assert np.array_equal(u[17], stream_uniforms(12345, 17, 3, 214))
    assert not np.array_equal(u[17], stream_uniforms(12346, 17, 3, 214))
    assert not np.array_equal(u[17], stream_uniforms(12345, 17, 4, 214))
