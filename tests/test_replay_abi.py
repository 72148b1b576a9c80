"""hrl_replay_gather / hrl_replay_draw: exports and argument validation, which returns before any HIP call (no GPU
needed).  The pointers are fake device addresses that are never dereferenced.
"""

import ctypes

import pytest

from handyrl_amd import _native

RING_PTRS = ('policy', 'amask', 'action', 'value', 'reward', 'ret', 'length', 'outcome', 'turn', 'tmask', 'omask')
BATCH_PTRS = ('policy', 'amask', 'action', 'value', 'outcome', 'reward', 'ret', 'episode_mask', 'turn_mask',
              'observation_mask', 'progress')
MOVER_RECORDS, PLAYERS_ALL, PLAYERS_SOLO, PLAYERS_MOVER = range(4)


def _gather(layout=MOVER_RECORDS, B=4, T=8, N=16, Tm=9, P=2, A=9, widths=(27,), types=None, nleaves=None,
            players=None, ring_null=(), out_null=(), null=()):
    lib = _native.load()
    ring, out = _native.ReplayRing(), _native.ReplayBatch()
    ring.N, ring.Tm, ring.P, ring.A = N, Tm, P, A
    ring.nleaves = len(widths) if nleaves is None else nleaves
    for l, w in enumerate(widths[:_native.REPLAY_MAX_LEAVES]):
        ring.obs_width[l] = w
        ring.obs_type[l] = _native.REPLAY_U8 if types is None else types[l]
        ring.obs[l] = None if ('obs', l) in ring_null else 4096 * (l + 1)
        out.obs[l] = None if ('obs', l) in out_null else 4096 * (l + 101)
    for i, k in enumerate(RING_PTRS):
        setattr(ring, k, None if k in ring_null else 4096 * (i + 20))
    for i, k in enumerate(BATCH_PTRS):
        setattr(out, k, None if k in out_null else 4096 * (i + 40))
    if players is None:
        players = layout == PLAYERS_SOLO
    arg = lambda name, addr: None if name in null else ctypes.c_void_p(addr)
    return lib.hrl_replay_gather(layout, None if 'ring' in null else ctypes.byref(ring), arg('slots', 4096 * 60),
                                 arg('start', 4096 * 61), ctypes.c_void_p(4096 * 62) if players else None, B, T,
                                 None if 'out' in null else ctypes.byref(out), None)


def _draw(B=4, ptr=3, count=8, N=16, M=16, T=4, P=2, null=(), players=True):
    lib = _native.load()
    arg = lambda name, addr: None if name in null else ctypes.c_void_p(addr)
    return lib.hrl_replay_draw(arg('u', 4096), B, ptr, count, N, M, arg('length', 8192), T, P, arg('slots', 12288),
                               arg('start', 16384), ctypes.c_void_p(20480) if players else None, None)


def test_symbols_exist_and_abi_version_stays_30():
    lib = _native.load()
    assert hasattr(lib, 'hrl_replay_gather') and hasattr(lib, 'hrl_replay_draw')
    assert 'hrl_replay_gather' in _native.SIGNATURES and 'hrl_replay_draw' in _native.SIGNATURES
    assert _native.ABI_VERSION == 30 and lib.hrl_abi_version() == 30


@pytest.mark.parametrize('kw', [
    {'B': -1},
    {'T': 0}, {'T': -3},
    {'null': ('ring',)}, {'null': ('out',)}, {'null': ('slots',)}, {'null': ('start',)},
    {'ring_null': ('policy',)}, {'ring_null': ('length',)}, {'ring_null': ('outcome',)},
    {'ring_null': (('obs', 0),)}, {'out_null': (('obs', 0),)},
    {'ring_null': ('turn',)},                                        # mover records need `turn`
    {'layout': PLAYERS_ALL, 'ring_null': ('tmask',)},                # per-player records need both masks
    {'layout': PLAYERS_MOVER, 'ring_null': ('omask',)},
    {'out_null': ('progress',)}, {'out_null': ('action',)}, {'out_null': ('observation_mask',)},
    {'widths': (3,) * 9},                                            # more than 8 observation leaves
    {'nleaves': 0},
    {'layout': 4}, {'layout': -1},                                   # unknown layout
    {'types': (2,)}, {'types': (-1,)},                               # unknown element type
    {'widths': (27, 0), 'types': (0, 1)},
    {'layout': PLAYERS_SOLO, 'players': False},                      # solo without players
    {'layout': MOVER_RECORDS, 'players': True}, {'layout': PLAYERS_ALL, 'players': True},
    {'N': 0}, {'Tm': 0}, {'P': 0}, {'A': 0}, {'Tm': 1 << 31},
    # the largest output must stay below 2^31 elements: the kernel indexes outputs with an int
    {'B': 1 << 16, 'T': 1 << 7, 'A': 1 << 8},                        # policy: 2^31 elements
    {'B': 1 << 20, 'T': 64, 'widths': (32,)},                        # an observation leaf: 2^31 elements
    {'layout': PLAYERS_ALL, 'B': 1 << 19, 'T': 64, 'P': 4, 'A': 16},  # (B, T, P, A): 2^31
    {'B': 1 << 40, 'T': 1 << 40},
])
def test_gather_rejects_without_gpu(kw):
    assert _gather(**kw) == _native.HRL_EINVAL


@pytest.mark.parametrize('kw', [
    {}, {'layout': PLAYERS_ALL}, {'layout': PLAYERS_SOLO}, {'layout': PLAYERS_MOVER},
    {'layout': PLAYERS_MOVER, 'players': True},
    {'widths': (3,) * 8, 'types': (0, 1) * 4},
    {'layout': PLAYERS_ALL, 'ring_null': ('turn',)},                 # a record its layout does not read
    {'ring_null': ('tmask', 'omask')},
])
def test_gather_empty_batch_is_ok_and_launches_nothing(kw):
    assert _gather(B=0, **kw) == _native.HRL_OK


def test_gather_empty_batch_is_still_validated():
    assert _gather(B=0, T=0) == _native.HRL_EINVAL
    assert _gather(B=0, ring_null=('policy',)) == _native.HRL_EINVAL


@pytest.mark.parametrize('kw', [
    {'B': -1}, {'T': 0}, {'P': 0}, {'N': 0},
    {'count': 17},                                                   # count > N
    {'count': 0},
    {'M': 0}, {'M': -5}, {'M': 1 << 31},
    {'ptr': -1}, {'ptr': 16},
    {'null': ('u',)}, {'null': ('length',)}, {'null': ('slots',)}, {'null': ('start',)},
])
def test_draw_rejects_without_gpu(kw):
    assert _draw(**kw) == _native.HRL_EINVAL


def test_draw_empty_batch_is_ok():
    assert _draw(B=0) == _native.HRL_OK
    assert _draw(B=0, players=False) == _native.HRL_OK
    assert _draw(B=0, count=16, ptr=0, M=4) == _native.HRL_OK
    assert _draw(B=0, count=17) == _native.HRL_EINVAL
