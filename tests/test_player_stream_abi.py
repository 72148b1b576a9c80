"""The C ABI of the per-player streaming generator (include/hrl_env.h, include/hrl_geese.h): the three entries are
declared and exported, their struct is laid out as declared, and every argument check answers before any HIP call
(no GPU is needed: a call either fails its validation or has E == 0 and launches nothing)."""

import ctypes

from handyrl_amd import _native

ENTRIES = ('hrl_geese_observe_at', 'hrl_selfplay_sample_record_players_stream', 'hrl_selfplay_harvest_players')
FAKE = ctypes.c_void_p(0x1000)      # never dereferenced: validation precedes every launch, and E == 0 launches nothing


def test_entries_are_declared_and_exported():
    lib = _native.load()
    for name in ENTRIES:
        res, args = _native.SIGNATURES[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p, name
        assert getattr(lib, name).argtypes == args, name
    assert len(_native.SIGNATURES['hrl_geese_observe_at'][1]) == 14
    assert len(_native.SIGNATURES['hrl_selfplay_sample_record_players_stream'][1]) == 24
    assert len(_native.SIGNATURES['hrl_selfplay_harvest_players'][1]) == 11
    assert lib.hrl_abi_version() == _native.ABI_VERSION == 30      # the new entries are additive


def test_player_slots_struct_is_laid_out_as_declared():
    s = _native.SelfplayPlayerSlots
    names = [n for n, _ in s._fields_]
    assert names == ['E', 'Tm', 'P', 'A', 'nleaves', 'obs_type', 'obs_width', 'obs', 'policy', 'amask', 'action',
                     'value', 'tmask', 'omask', 'reward']
    L = _native.REPLAY_MAX_LEAVES
    assert s.E.offset == 0 and s.nleaves.offset == 32 and s.obs_type.offset == 36
    assert s.obs_width.offset == 72 and s.obs.offset == 72 + 8 * L and s.policy.offset == 72 + 16 * L
    assert s.reward.offset == ctypes.sizeof(s) - 8 and ctypes.sizeof(s) == 72 + 16 * L + 7 * 8


def _observe(**kw):
    a = dict(body=FAKE, hd=FAKE, len=FAKE, food=FAKE, prev=FAKE, views=FAKE, record=FAKE, ply=FAKE, infer=FAKE,
             active=FAKE, E=0, P=4, Tm=199)
    a.update(kw)
    return _native.load().hrl_geese_observe_at(*a.values(), None)


def test_observe_at_validates():
    assert _observe() == _native.HRL_OK
    for k in ('body', 'hd', 'len', 'food', 'prev', 'views', 'record', 'ply', 'infer', 'active'):
        assert _observe(**{k: None}) == _native.HRL_EINVAL, k
    for kw in ({'E': -1}, {'P': 2}, {'Tm': 0}, {'E': 1 << 31}):
        assert _observe(**kw) == _native.HRL_EINVAL, kw


def _tail(**kw):
    a = dict(logits=FAKE, logit_stride=4, value=FAKE, legal=FAKE, legal_player_stride=0, turns=FAKE, infer=FAKE,
             active=FAKE, seed=7, game=FAKE, ply=FAKE, E=0, P=4, A=4, Tm=199, action=FAKE, usel=FAKE,
             policy_buf=FAKE, amask_buf=FAKE, action_buf=FAKE, value_buf=FAKE, tmask_buf=FAKE, omask_buf=FAKE)
    a.update(kw)
    return _native.load().hrl_selfplay_sample_record_players_stream(*a.values(), None)


def test_sample_record_players_stream_validates():
    assert _tail() == _native.HRL_OK
    assert _tail(legal_player_stride=4) == _native.HRL_OK
    for k in ('logits', 'value', 'legal', 'turns', 'infer', 'active', 'game', 'ply', 'action', 'usel', 'policy_buf',
              'amask_buf', 'action_buf', 'value_buf', 'tmask_buf', 'omask_buf'):
        assert _tail(**{k: None}) == _native.HRL_EINVAL, k
    for kw in ({'E': -1}, {'P': 0}, {'A': 0}, {'A': (1 << 20) + 1, 'logit_stride': 1 << 21}, {'Tm': 0},
               {'logit_stride': 3}, {'legal_player_stride': 1}, {'legal_player_stride': 8},
               {'P': 1 << 29, 'A': 8, 'logit_stride': 8}, {'P': 1 << 16, 'E': 1 << 14}):
        assert _tail(**kw) == _native.HRL_EINVAL, kw


def _harvest(slot_kw=None, ring_kw=None, **kw):
    slots, ring = _native.SelfplayPlayerSlots(), _native.ReplayRing()
    slots.E, slots.Tm, slots.P, slots.A, slots.nleaves = 0, 9, 2, 9, 2
    ring.N, ring.Tm, ring.P, ring.A, ring.nleaves = 8, 9, 2, 9, 2
    for l, w in enumerate((27, 5)):
        slots.obs[l] = ring.obs[l] = FAKE.value
        slots.obs_width[l] = ring.obs_width[l] = w
        slots.obs_type[l], ring.obs_type[l] = _native.REPLAY_F32, _native.REPLAY_U8
    for k in ('policy', 'amask', 'action', 'value', 'tmask', 'omask', 'reward'):
        setattr(slots, k, FAKE.value)
    for k in ('policy', 'amask', 'action', 'value', 'reward', 'ret', 'length', 'outcome', 'tmask', 'omask'):
        setattr(ring, k, FAKE.value)
    for obj, changes in ((slots, slot_kw), (ring, ring_kw)):
        for k, v in (changes or {}).items():
            if isinstance(k, tuple):
                getattr(obj, k[0])[k[1]] = v
            else:
                setattr(obj, k, v)
    a = dict(done=FAKE, slots=ctypes.byref(slots), ply=FAKE, outcome=FAKE, gamma=0.8, ring=ctypes.byref(ring),
             ring_game=FAKE, game=FAKE, pending=FAKE, state=FAKE)
    a.update(kw)
    return _native.load().hrl_selfplay_harvest_players(*a.values(), None)


def test_harvest_players_validates():
    assert _harvest() == _native.HRL_OK
    assert _harvest(slot_kw={'reward': None}) == _native.HRL_OK          # no reward: allowed
    assert _harvest(ring_kw={'turn': None}) == _native.HRL_OK            # the PLAYERS layouts have no turn record
    for k in ('done', 'slots', 'ply', 'outcome', 'ring', 'ring_game', 'game', 'pending', 'state'):
        assert _harvest(**{k: None}) == _native.HRL_EINVAL, k
    for k in ('policy', 'amask', 'action', 'value', 'tmask', 'omask', ('obs', 1)):
        assert _harvest(slot_kw={k: None}) == _native.HRL_EINVAL, k
    for k in ('policy', 'amask', 'action', 'value', 'reward', 'ret', 'length', 'outcome', 'tmask', 'omask', ('obs', 0)):
        assert _harvest(ring_kw={k: None}) == _native.HRL_EINVAL, k
    for kw in ({'E': -1}, {'Tm': 0}, {'P': 0}, {'A': 0}, {'Tm': 8}, {'P': 4}, {'A': 4}, {'nleaves': 0},
               {'nleaves': 9}, {'nleaves': 1}, {('obs_width', 0): 0}, {('obs_width', 1): 6}, {('obs_type', 0): 2},
               {'Tm': 1 << 31}):
        assert _harvest(slot_kw=kw) == _native.HRL_EINVAL, kw
    for kw in ({'N': 0}, {('obs_type', 1): 7}, {('obs_width', 0): 28}):
        assert _harvest(ring_kw=kw) == _native.HRL_EINVAL, kw

