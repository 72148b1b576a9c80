"""The C ABI of the evaluator of simultaneous-move envs (include/hrl_env.h, include/hrl_geese.h): both entries are
declared and exported, and every argument check answers before any HIP call (no GPU is needed: a call either fails its
validation or has E == 0 and launches nothing)."""

import ctypes

from handyrl_amd import _native

FAKE = ctypes.c_void_p(0x1000)      # never dereferenced: validation precedes every launch, and E == 0 launches nothing
NAN = float('nan')


def test_entries_are_declared_and_exported():
    lib = _native.load()
    for name, n in (('hrl_players_act', 28), ('hrl_geese_observe_seats', 11)):
        res, args = _native.SIGNATURES[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p and len(args) == n, name
        assert getattr(lib, name).argtypes == args, name
    assert lib.hrl_abi_version() == _native.ABI_VERSION == 30      # the new entries are additive


def _act(**kw):
    a = dict(logits_home=FAKE, stride_home=4, logits_opp=FAKE, stride_opp=4, legal=FAKE, legal_player_stride=0,
             turns=FAKE, seed=7, temperature_home=0.0, temperature_opp=0.0, opening=0, game=FAKE, ply=FAKE,
             active=FAKE, seat=FAKE, forced=FAKE, E=0, P=4, A=4, Tm=199, G=5, action=FAKE, usel=FAKE,
             trace_action=FAKE, trace_picked=FAKE, trace_policy=FAKE, trace_alive=FAKE)
    a.update(kw)
    return _native.load().hrl_players_act(*a.values(), None)


def test_players_act_validates():
    assert _act() == _native.HRL_OK                                   # E == 0: no launch
    assert _act(legal_player_stride=4) == _native.HRL_OK
    assert _act(G=0) == _native.HRL_OK
    assert _act(temperature_home=0.5, temperature_opp=2.0, opening=3) == _native.HRL_OK
    # optional: the second net, the forced moves, the trace (all four or none)
    assert _act(logits_opp=None, stride_opp=0, forced=None) == _native.HRL_OK
    assert _act(trace_action=None, trace_picked=None, trace_policy=None, trace_alive=None) == _native.HRL_OK
    for k in ('logits_home', 'legal', 'turns', 'game', 'ply', 'active', 'seat', 'action', 'usel'):
        assert _act(**{k: None}) == _native.HRL_EINVAL, k
    for kw in ({'E': -1}, {'P': 0}, {'A': 0}, {'Tm': 0}, {'G': -1}, {'stride_home': 3}, {'stride_opp': 3},
               {'legal_player_stride': 1}, {'legal_player_stride': 8}, {'temperature_home': -0.1},
               {'temperature_home': NAN}, {'temperature_opp': -1.0}, {'temperature_opp': NAN}, {'opening': -1},
               {'P': 1 << 16, 'E': 1 << 14},                                       # P * E == 0x40000000
               {'P': 1 << 29, 'A': 8, 'stride_home': 8, 'stride_opp': 8},          # P * ceil(A / 4) == 0x40000000
               {'A': (1 << 20) + 1, 'stride_home': 1 << 21, 'stride_opp': 1 << 21}):
        assert _act(**kw) == _native.HRL_EINVAL, kw
    trace = ('trace_action', 'trace_picked', 'trace_policy', 'trace_alive')
    for k in trace:                                                   # some but not all
        assert _act(**{k: None}) == _native.HRL_EINVAL, k
        assert _act(**{j: None for j in trace if j != k}) == _native.HRL_EINVAL, k
    assert _act(stride_opp=0) == _native.HRL_EINVAL                   # a second net needs its stride


def _seats(**kw):
    a = dict(body=FAKE, hd=FAKE, len=FAKE, food=FAKE, prev=FAKE, seat=FAKE, rows=FAKE, E=0, P=4, K=1)
    a.update(kw)
    return _native.load().hrl_geese_observe_seats(*a.values(), None)


def test_observe_seats_validates():
    for K in (1, 2, 3, 4):
        assert _seats(K=K) == _native.HRL_OK
    for k in ('body', 'hd', 'len', 'food', 'prev', 'seat', 'rows'):
        assert _seats(**{k: None}) == _native.HRL_EINVAL, k
    for kw in ({'E': -1}, {'E': 1 << 31}, {'P': 2}, {'P': 5}, {'K': 0}, {'K': 5}, {'K': -1}):
        assert _seats(**kw) == _native.HRL_EINVAL, kw
