"""hrl_league_finish's and hrl_rows_permute's C entries: the exports and their argument validation, which comes before
any HIP call (no GPU)."""

import ctypes

from handyrl_amd import _native

EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK

FINISH = ('terminal', 'outcome', 'active', 'ply', 'game', 'pending', 'state', 'outcome_out', 'length_out')


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def _finish(null=(), E=12, S=4, Tm=9, P=2, G=7):
    a = {n: None if n in null else _p(i) for i, n in enumerate(FINISH)}
    return _native.load().hrl_league_finish(a['terminal'], a['outcome'], E, S, Tm, P, G, a['active'], a['ply'],
                                            a['game'], a['pending'], a['state'], a['outcome_out'], a['length_out'],
                                            None)


def _permute(nleaves=2, n=0, F=(3, 8), dst_stride=(3, 8), src_stride=(5, 8), null=(), null_leaf=None,
             src_index=True, dst_index=True):
    k = max(nleaves, 1)
    dst = [None if null_leaf == ('dst', l) else 4096 * (l + 1) for l in range(k)]
    src = [None if null_leaf == ('src', l) else 4096 * (l + 33) for l in range(k)]
    pad = lambda v: (list(v) + [v[-1]] * k)[:k]   # noqa: E731
    arrays = {'dst': (ctypes.c_void_p * k)(*dst), 'src': (ctypes.c_void_p * k)(*src),
              'dst_stride': _native.i64_array(pad(dst_stride)), 'src_stride': _native.i64_array(pad(src_stride)),
              'F': _native.i64_array(pad(F))}
    a = {key: None if key in null else v for key, v in arrays.items()}
    return _native.load().hrl_rows_permute(nleaves, a['dst'], a['dst_stride'], a['src'], a['src_stride'], a['F'],
                                           _p(70) if src_index else None, _p(71) if dst_index else None, n, None)


def test_exports_and_abi_version():
    lib = _native.load()
    assert lib.hrl_abi_version() == 30 == _native.ABI_VERSION
    for name in ('hrl_league_finish', 'hrl_rows_permute'):
        assert name in _native.SIGNATURES and hasattr(lib, name)


def test_league_finish_validates_arguments():
    for name in FINISH:
        assert _finish(null=(name,)) == EINVAL, name
        assert _finish(null=(name,), E=0) == EINVAL, name
    for kw in ({'E': -4}, {'E': 1 << 31}, {'S': 0}, {'S': 1}, {'S': 3}, {'S': -2}, {'S': 8}, {'E': 10}, {'Tm': 0},
               {'P': 0}, {'P': 1 << 31}, {'G': -1}):
        assert _finish(**kw) == EINVAL, kw
    for kw in ({'S': 1}, {'S': 3}, {'S': 0}, {'Tm': 0}, {'P': 0}, {'G': -1}):     # checked before E == 0 returns
        assert _finish(E=0, **kw) == EINVAL, kw
    assert _finish(E=0) == OK
    assert _finish(E=0, S=2, G=0, Tm=1, P=1) == OK


def test_rows_permute_validates_arguments():
    assert _permute() == OK                                   # n == 0: no launch
    assert _permute(src_index=False, dst_index=False) == OK   # both indices optional
    assert _permute(nleaves=16) == OK
    for kw in ({'nleaves': 0}, {'nleaves': 17}, {'nleaves': -1}, {'n': -1}, {'n': 1 << 31}, {'F': (0, 8)},
               {'F': (3, -1)}, {'dst_stride': (2, 8)}, {'src_stride': (5, 7)}, {'null': ('dst',)}, {'null': ('src',)},
               {'null': ('dst_stride',)}, {'null': ('src_stride',)}, {'null': ('F',)}, {'null_leaf': ('dst', 1)},
               {'null_leaf': ('src', 0)}):
        assert _permute(**kw) == EINVAL, kw
    # a bad argument is refused whatever n is (nothing is launched at these made-up addresses: n stays 0 or invalid)
    assert _permute(n=-1, src_index=False) == EINVAL
