"""ctypes binding of the C ABI in ``include/*.h`` (libhrl.so).

The library is the ONLY compute path for the kernels it exports: if it is
missing or fails to load, every caller gets a RuntimeError — there is no CPU
or eager-PyTorch fallback.

torch is imported first so that the HIP runtime torch ships
(libamdhip64.so.7) is already in the process; libhrl.so's DT_NEEDED entry for
the same soname then binds to that copy, and the hipStream_t handles torch
hands us are valid in the library.
"""

import ctypes
import os

import torch  # noqa: F401  (must precede loading libhrl.so, see module doc)

from . import _cabi

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_lib', 'libhrl.so')
# diagnostic builds (tools/*): HRL_LIB_PATH names another build of the same sources
LIB_PATH = os.environ.get('HRL_LIB_PATH', LIB_PATH)

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')


def _headers():
    """{name: text} of include/*.h, the single definition of the ABI; there is no hand-written copy to fall back on."""
    names = sorted(f for f in os.listdir(INCLUDE_DIR) if f.endswith('.h')) if os.path.isdir(INCLUDE_DIR) else []
    if not names:
        raise RuntimeError('C headers directory %s is missing or empty: the ctypes binding of libhrl.so is derived '
                           'from its *.h (there is no hand-written fallback)' % INCLUDE_DIR)
    headers = {}
    for f in names:
        with open(os.path.join(INCLUDE_DIR, f)) as h:
            headers[f] = h.read()
    return headers


# symbol -> (restype, argtypes), the structs and the integer constants, all as include/*.h declares them
SIGNATURES, _structs, _constants = _cabi.parse(_headers())

HRL_OK = _constants['HRL_OK']
HRL_EINVAL = _constants['HRL_EINVAL']

ALG = {k[len('HRL_ALG_'):]: v for k, v in _constants.items() if k.startswith('HRL_ALG_')}

# include/hrl_replay.h
REPLAY_MAX_LEAVES = _constants['HRL_REPLAY_MAX_LEAVES']
REPLAY_U8, REPLAY_F32 = _constants['HRL_REPLAY_U8'], _constants['HRL_REPLAY_F32']
REPLAY_LAYOUT = {k: _constants['HRL_REPLAY_' + k.upper()]
                 for k in ('mover_records', 'players_all', 'players_solo', 'players_mover')}

ReplayRing = _structs['hrl_replay_ring']
ReplayBatch = _structs['hrl_replay_batch']
SelfplaySlots = _structs['hrl_selfplay_slots']   # include/hrl_env.h
SelfplayPlayerSlots = _structs['hrl_selfplay_player_slots']

# the version this package expects of the library (hrl_abi_version()); no header states it
ABI_VERSION = 30

_lib = None


def bind(lib):
    """Set restype and argtypes of every entry point of `lib` (libhrl.so or a diagnostic build of its sources)."""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load libhrl.so (once) and bind every signature; raise if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('HIP library %s is missing: run `python -m handyrl_amd.build` '
                           '(there is no CPU fallback for the learner kernels)' % LIB_PATH)
    lib = bind(ctypes.CDLL(LIB_PATH))
    if lib.hrl_abi_version() != ABI_VERSION:
        raise RuntimeError('libhrl.so ABI %d != expected %d' % (lib.hrl_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(code, what):
    if code != HRL_OK:
        msg = load().hrl_strerror(code).decode()
        if code == HRL_EINVAL:
            raise ValueError('%s: %s' % (what, msg))
        raise RuntimeError('%s failed (%d): %s' % (what, code, msg))


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ptr_array(tensors):
    """A C array of device pointers (None -> NULL) for the multi-tensor entry points."""
    arr = (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])
    return arr


def i64_array(values):
    return (ctypes.c_int64 * len(values))(*values)


def stream_of(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
