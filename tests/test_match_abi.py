"""hrl_match_act's C entry: the export and its argument validation, which comes before any HIP call (no GPU)."""

import ctypes

from handyrl_amd import _native

EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK

REQUIRED = ('logits_home', 'legal', 'game', 'ply', 'active', 'seat', 'action')
TRACE = ('trace_action', 'trace_picked', 'trace_policy', 'trace_model_ply')


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def _match(null=(), E=5, A=9, Tm=4, P=2, G=6, stride_home=None, stride_opp=None, opp=True, mover=0, t_home=0.0,
           t_opp=0.0, opening=0, forced=True, trace=TRACE):
    names = REQUIRED + ('logits_opp', 'forced') + TRACE
    a = {n: None if n in null else _p(i) for i, n in enumerate(names)}
    if not opp:
        a['logits_opp'] = None
    if not forced:
        a['forced'] = None
    for n in TRACE:
        if n not in trace:
            a[n] = None
    return _native.load().hrl_match_act(
        a['logits_home'], A if stride_home is None else stride_home, a['logits_opp'],
        A if stride_opp is None else stride_opp, a['legal'], 7, t_home, t_opp, opening, a['game'], a['ply'],
        a['active'], a['seat'], mover, a['forced'], E, A, Tm, P, G, a['action'], a['trace_action'], a['trace_picked'],
        a['trace_policy'], a['trace_model_ply'], None)


def test_export_and_abi_version():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    assert 'hrl_match_act' in _native.SIGNATURES and hasattr(lib, 'hrl_match_act')


def test_match_act_validates_arguments():
    for name in REQUIRED:
        assert _match(null=(name,)) == EINVAL, name
        assert _match(null=(name,), E=0) == EINVAL, name
    for kw in ({'E': -1}, {'E': 1 << 31}, {'A': 0}, {'A': (1 << 20) + 1}, {'Tm': 0}, {'P': 0}, {'G': -1},
               {'mover': 2}, {'mover': -1}, {'stride_home': 8}, {'stride_opp': 8}, {'t_home': -0.5},
               {'t_home': float('nan')}, {'t_opp': -0.5}, {'t_opp': float('nan')}, {'opening': -1}):
        assert _match(**kw) == EINVAL, kw
        assert _match(E=0, **{k: v for k, v in kw.items() if k != 'E'}) == (OK if 'E' in kw else EINVAL), kw
    for k in range(1, 4):       # some but not all trace buffers
        assert _match(trace=TRACE[:k]) == EINVAL, k
        assert _match(trace=TRACE[k:]) == EINVAL, k


def test_optional_arguments_and_no_slots():
    assert _match(E=0) == OK
    assert _match(E=0, opp=False, stride_opp=0) == OK         # without an opponent its stride is not looked at
    assert _match(E=0, forced=False, trace=()) == OK
    assert _match(E=0, G=0, opening=1 << 40, t_home=0.5, t_opp=2.0, mover=1) == OK
