"""The C ABI of the rule-based Geese opponent (include/hrl_geese.h: hrl_geese_greedy; include/hrl_env.h:
hrl_players_act_rule): both entries are declared in the derived binding and exported, and every argument check answers
before any HIP call (no GPU is needed: a call either fails its validation or has E == 0 and launches nothing)."""

import ctypes

from handyrl_amd import _native

FAKE = ctypes.c_void_p(0x1000)      # never dereferenced: validation precedes every launch, and E == 0 launches nothing
NAN = float('nan')


def test_entries_are_declared_and_exported():
    lib = _native.load()
    for name, n in (('hrl_geese_greedy', 9), ('hrl_players_act_rule', 29)):
        res, args = _native.SIGNATURES[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p and len(args) == n, name
        assert getattr(lib, name).argtypes == args, name
    # the old entry's argument list plus the rule pointer after `forced`
    old, new = _native.SIGNATURES['hrl_players_act'][1], _native.SIGNATURES['hrl_players_act_rule'][1]
    assert new[:16] == old[:16] and new[16] is ctypes.c_void_p and new[17:] == old[16:]
    assert lib.hrl_abi_version() == _native.ABI_VERSION == 30      # the new entries are additive


def _greedy(**kw):
    a = dict(body=FAKE, hd=FAKE, len=FAKE, food=FAKE, last=FAKE, rule=FAKE, E=0, P=4)
    a.update(kw)
    return _native.load().hrl_geese_greedy(*a.values(), None)


def test_geese_greedy_validates():
    assert _greedy() == _native.HRL_OK                                # E == 0: no launch
    for k in ('body', 'hd', 'len', 'food', 'last', 'rule'):
        assert _greedy(**{k: None}) == _native.HRL_EINVAL, k
        assert _greedy(**{k: None}, E=3) == _native.HRL_EINVAL, k
    for kw in ({'E': -1}, {'E': 1 << 31}, {'P': 0}, {'P': 2}, {'P': 3}, {'P': 5}, {'E': 3, 'P': 2}):
        assert _greedy(**kw) == _native.HRL_EINVAL, kw


def _act(**kw):
    a = dict(logits_home=FAKE, stride_home=4, logits_opp=None, stride_opp=0, legal=FAKE, legal_player_stride=0,
             turns=FAKE, seed=7, temperature_home=0.0, temperature_opp=0.0, opening=0, game=FAKE, ply=FAKE,
             active=FAKE, seat=FAKE, forced=FAKE, rule=FAKE, E=0, P=4, A=4, Tm=199, G=5, action=FAKE, usel=FAKE,
             trace_action=FAKE, trace_picked=FAKE, trace_policy=FAKE, trace_alive=FAKE)
    a.update(kw)
    return _native.load().hrl_players_act_rule(*a.values(), None)


def test_players_act_rule_validates():
    assert _act() == _native.HRL_OK                                   # E == 0: no launch
    assert _act(legal_player_stride=4) == _native.HRL_OK
    assert _act(G=0) == _native.HRL_OK
    assert _act(temperature_home=0.5, temperature_opp=2.0, opening=3) == _native.HRL_OK
    # optional: the rule, the second net (not both), the forced moves, the trace (all four or none)
    assert _act(rule=None) == _native.HRL_OK
    assert _act(rule=None, logits_opp=FAKE, stride_opp=4) == _native.HRL_OK
    assert _act(forced=None) == _native.HRL_OK
    assert _act(trace_action=None, trace_picked=None, trace_policy=None, trace_alive=None) == _native.HRL_OK
    # one meaning per call: a rule and a second net together are refused
    assert _act(logits_opp=FAKE, stride_opp=4) == _native.HRL_EINVAL
    assert _act(logits_opp=FAKE, stride_opp=4, E=3) == _native.HRL_EINVAL
    # everything hrl_players_act refuses, with and without a rule
    for rule in (FAKE, None):
        for k in ('logits_home', 'legal', 'turns', 'game', 'ply', 'active', 'seat', 'action', 'usel'):
            assert _act(rule=rule, **{k: None}) == _native.HRL_EINVAL, k
        for kw in ({'E': -1}, {'P': 0}, {'A': 0}, {'Tm': 0}, {'G': -1}, {'stride_home': 3},
                   {'legal_player_stride': 1}, {'legal_player_stride': 8}, {'temperature_home': -0.1},
                   {'temperature_home': NAN}, {'temperature_opp': -1.0}, {'temperature_opp': NAN}, {'opening': -1},
                   {'P': 1 << 16, 'E': 1 << 14},                                       # P * E == 0x40000000
                   {'P': 1 << 29, 'A': 8, 'stride_home': 8},                           # P * ceil(A / 4) == 0x40000000
                   {'A': (1 << 20) + 1, 'stride_home': 1 << 21}):
            assert _act(rule=rule, **kw) == _native.HRL_EINVAL, kw
        trace = ('trace_action', 'trace_picked', 'trace_policy', 'trace_alive')
        for k in trace:                                               # some but not all
            assert _act(rule=rule, **{k: None}) == _native.HRL_EINVAL, k
            assert _act(rule=rule, **{j: None for j in trace if j != k}) == _native.HRL_EINVAL, k
    assert _act(rule=None, logits_opp=FAKE, stride_opp=3) == _native.HRL_EINVAL   # a second net needs its stride
    assert _act(rule=None, logits_opp=FAKE, stride_opp=0) == _native.HRL_EINVAL
