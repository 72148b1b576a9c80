"""The Hungry Geese C entries (include/hrl_geese.h): exports and argument validation, which happens before any HIP
call, so no GPU is needed."""

import ctypes

from handyrl_amd import _native

EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK
STATE = ('body', 'hd', 'len', 'food', 'last', 'prev', 'reward', 'step', 'game', 'live')


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def _args(names, null):
    return {n: None if n in null else _p(i) for i, n in enumerate(names)}


def test_exports_and_abi_version():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    for name in ('hrl_geese_reset', 'hrl_geese_step', 'hrl_geese_observe'):
        assert name in _native.SIGNATURES and hasattr(lib, name), name


def _reset(null=(), E=5, P=4):
    a = _args(STATE + ('mask', 'rank'), null)
    return _native.load().hrl_geese_reset(*[a[n] for n in STATE], a['mask'], a['rank'], 7, 3, E, P, None)


def test_reset_validates_arguments():
    for name in STATE:
        assert _reset(null=(name,)) == EINVAL, name
        assert _reset(null=(name,), E=0) == EINVAL, name
    assert _reset(E=-1) == EINVAL
    for P in (0, 2, 5):
        assert _reset(P=P) == EINVAL, P
    assert _reset(E=0) == OK
    assert _reset(E=0, null=('mask', 'rank')) == OK      # both optional: every slot, game number base + slot


def _step(null=(), E=5, P=4, A=4):
    names = STATE + ('actions', 'active')
    a = _args(names, null)
    return _native.load().hrl_geese_step(*[a[n] for n in names], 3, E, P, A, None)


def test_step_validates_arguments():
    for name in STATE + ('actions', 'active'):
        assert _step(null=(name,)) == EINVAL, name
        assert _step(null=(name,), E=0) == EINVAL, name
    assert _step(E=-1) == EINVAL
    for kw in ({'P': 2}, {'P': 5}, {'A': 3}, {'A': 5}, {'A': 0}):
        assert _step(**kw) == EINVAL, kw
    assert _step(E=0) == OK


OBSERVE = ('body', 'hd', 'len', 'food', 'prev', 'views', 'record', 't', 'infer')


def _observe(null=(), E=5, P=4, Tm=6):
    a = _args(OBSERVE, null)
    return _native.load().hrl_geese_observe(*[a[n] for n in OBSERVE], E, P, Tm, None)


def test_observe_validates_arguments():
    for name in OBSERVE[:6]:
        assert _observe(null=(name,)) == EINVAL, name
        assert _observe(null=(name,), E=0) == EINVAL, name
    # a record needs the ply index, the infer mask and a ply count
    assert _observe(null=('t',)) == EINVAL and _observe(null=('infer',)) == EINVAL and _observe(Tm=0) == EINVAL
    assert _observe(E=-1) == EINVAL and _observe(E=1 << 31) == EINVAL
    for P in (0, 2, 5):
        assert _observe(P=P) == EINVAL, P
    assert _observe(E=0) == OK
    assert _observe(E=0, null=('record', 't', 'infer'), Tm=0) == OK      # no record: views only
