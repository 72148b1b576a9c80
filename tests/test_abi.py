"""libhrl.so loads on a CPU-only host and exports exactly the C ABI of include/*.h.

No compute call is made here (no GPU): only the argument-validation paths,
which return before any HIP call.
"""

import ctypes
import glob
import os
import re
import subprocess

import pytest

from handyrl_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    syms = set()
    for h in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        text = open(h).read()
        text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
        syms |= set(re.findall(r'\b(hrl_[a-z0-9_]+)\s*\(', text))
    return syms


def test_header_symbols_bound():
    syms = declared_symbols()
    assert 'hrl_compute_target' in syms and 'hrl_compute_targets_fused' in syms
    # the binding is derived from the headers by a strict parser: it missed nothing this loose reading sees
    assert syms == set(_native.SIGNATURES), 'derived ctypes signatures out of sync with include/*.h'
    assert len(_native.SIGNATURES) >= 130


def test_derived_signatures_match_a_reading_by_hand():
    """A sample of include/*.h read by hand (not a second table): every scalar type and both return kinds in use."""
    I, I64, U64, D, P = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p
    pinned = {
        'hrl_compute_target': (I, [I, P, P, P, P, P, I64, I64, I64, I64, I64, I64, D, D, P, P, P]),
        'hrl_match_act': (I, [P, I64, P, I64, P, U64, D, D, I64, P, P, P, P, I64, P, I64, I64, I64, I64, I64,
                              P, P, P, P, P, P]),
        'hrl_bn_workspace_bytes': (I64, [I64, I64, I64]),
        'hrl_strerror': (ctypes.c_char_p, [I]),
        'hrl_abi_version': (I, []),
        'hrl_replay_gather': (I, [I, P, P, P, P, I64, I64, P, P]),
    }
    for name, (res, args) in pinned.items():
        assert _native.SIGNATURES[name] == (res, args), name


def test_derived_struct_layouts_match_a_reading_by_hand():
    """sizeof and offsets of the three descriptor structs, laid out by hand from the headers for the LP64 target
    (offsetof / sizeof in a C program that includes the headers give the same numbers)."""
    offsets = lambda cls, names: {n: getattr(cls, n).offset for n in names}   # noqa: E731
    ring, batch, slots = _native.ReplayRing, _native.ReplayBatch, _native.SelfplaySlots
    assert (ctypes.sizeof(ring), ctypes.sizeof(batch), ctypes.sizeof(slots)) == (288, 152, 216)
    assert offsets(ring, ('nleaves', 'obs_type', 'obs_width', 'obs', 'policy', 'omask')) == {
        'nleaves': 32, 'obs_type': 36, 'obs_width': 72, 'obs': 136, 'policy': 200, 'omask': 280}
    assert offsets(batch, ('obs', 'policy', 'progress')) == {'obs': 0, 'policy': 64, 'progress': 144}
    assert offsets(slots, ('nleaves', 'obs_width', 'obs', 'policy', 'reward')) == {
        'nleaves': 32, 'obs_width': 40, 'obs': 104, 'policy': 168, 'reward': 208}
    assert [n for n, _ in ring._fields_] == [
        'N', 'Tm', 'P', 'A', 'nleaves', 'obs_type', 'obs_width', 'obs', 'policy', 'amask', 'action', 'value',
        'reward', 'ret', 'length', 'outcome', 'turn', 'tmask', 'omask']
    assert ring._fields_[-1][0] == 'omask' and batch._fields_[-1][0] == 'progress'
    assert slots._fields_[-1][0] == 'reward'
    assert all(t is ctypes.c_void_p for _, t in batch._fields_[1:])


def test_derived_constants():
    assert _native.HRL_OK == 0 and _native.HRL_EINVAL == -22
    assert _native.REPLAY_MAX_LEAVES == 8 and (_native.REPLAY_U8, _native.REPLAY_F32) == (0, 1)
    assert _native.ALG == {'MC': 0, 'TD': 1, 'UPGO': 2, 'VTRACE': 3}
    assert _native.REPLAY_LAYOUT == {'mover_records': 0, 'players_all': 1, 'players_solo': 2, 'players_mover': 3}
    assert _native.ABI_VERSION == 30


def test_missing_headers_fail_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_native, 'INCLUDE_DIR', str(tmp_path / 'include'))
    with pytest.raises(RuntimeError, match=str(tmp_path / 'include')):
        _native._headers()


def test_library_exports_every_declared_symbol():
    lib = _native.load()
    for s in declared_symbols():
        assert hasattr(lib, s), s
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (hrl_[a-z0-9_]+)', out))
    # equality: an exported function with no prototype would have no binding
    assert declared_symbols() == exported


def test_abi_version_and_errors():
    lib = _native.load()
    assert lib.hrl_abi_version() == _native.ABI_VERSION
    assert b'invalid' in lib.hrl_strerror(_native.HRL_EINVAL)
    assert lib.hrl_strerror(0) == b'success'


@pytest.mark.parametrize('alg,kw', [
    (7, {}),                                  # unknown algorithm
    (1, {'T': 0}),                            # empty time axis
    (1, {'C': 65}),                           # more columns than a wave
    (1, {'ret_T': 3}),                        # returns time extent not in {1, T}
    (3, {'rho_C': 2, 'rho_div': 2, 'C': 2}),  # rho columns do not tile value columns
    (3, {'null_rho': True}),                  # V-trace without rhos
    (0, {'targets': True}),                   # MC writes no targets
])
def test_invalid_arguments_rejected_without_gpu(alg, kw):
    lib = _native.load()
    dummy = ctypes.c_void_p(16)
    B, T, C = 4, kw.get('T', 8), kw.get('C', 2)
    rho_C, rho_div = kw.get('rho_C', 1), kw.get('rho_div', C)
    rho = None if kw.get('null_rho') else dummy
    tgt = dummy if kw.get('targets') else None
    code = lib.hrl_compute_target(alg, dummy, dummy, None, rho, rho, B, T, C, kw.get('ret_T', 1),
                                  rho_C, rho_div, 0.7, 1.0, tgt, dummy, None)
    assert code == _native.HRL_EINVAL


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_native, '_lib', None)
    monkeypatch.setattr(_native, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _native.load()


def test_gboard_wgrad_rejects_workspace_sized_by_games_not_tiles():
    """hrl_gboard_wgrad runs one workgroup partial per 16-game tile of each record, so 24 records of 2 games need
    24 partials, not ceil(48 / 16) = 3: a workspace sized from the game total is rejected before any launch."""
    lib = _native.load()
    n = 24
    ptrs = (ctypes.c_void_p * n)(*[4096 * (i + 1) for i in range(n)])
    strides = (ctypes.c_int64 * n)(*[32 * 36] * n)
    dstrides = (ctypes.c_int64 * n)(*[128 * 36] * n)
    ns = (ctypes.c_int64 * n)(*[2] * n)
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)   # noqa: E731
    small = lib.hrl_gboard_wgrad_workspace_bytes(128, 32, 2 * n)
    enough = lib.hrl_gboard_wgrad_workspace_bytes(128, 32, 16 * n)
    assert 0 < small < enough
    code = lib.hrl_gboard_wgrad(cast(ptrs), cast(strides), cast(ptrs), cast(dstrides), cast(ns), n, 128, 32,
                                ctypes.c_void_p(16), 64, 32, None, ctypes.c_void_p(16), small, None)
    assert code == _native.HRL_EINVAL


def test_gboard_forward_rejects_undersized_packed_buffer():
    """hrl_gboard_forward / hrl_gboard_forward_groups take the packed buffer's size (ABI 19) and return HRL_EINVAL,
    before any launch, when it is below hrl_gboard_pack_bytes(Cout, Cin_g): a C caller binding the ABI directly
     cannot make the kernel read past the fragments.  Only argument validation runs here."""
    lib = _native.load()
    dummy = ctypes.c_void_p(4096)
    N, Cout, cin = 8, 64, 32
    need = lib.hrl_gboard_pack_bytes(Cout, cin)
    assert need > 0
    for size in (need - 16, need // 2, 0):
        code = lib.hrl_gboard_forward(dummy, cin * 36, None, 0, N, cin, 1, dummy, size, Cout, None, None, None, 0,
                                      dummy, Cout * 36, None)
        assert code == _native.HRL_EINVAL
    # the adjoint packing of the move head's 64 <- 8 input gradient (K = 8): Cout 64, Cin_g 8
    need_adj = lib.hrl_gboard_pack_bytes(64, 8)
    code = lib.hrl_gboard_forward(dummy, 8 * 36, None, 0, N, 8, 1, dummy, need_adj - 1, 64, None, None, None, 0,
                                  dummy, 64 * 36, None)
    assert code == _native.HRL_EINVAL
    L, H = 3, 32
    xs = (ctypes.c_void_p * L)(*[4096 * (i + 1) for i in range(L)])
    strides = (ctypes.c_int64 * L)(*[H * 36] * L)
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)   # noqa: E731
    need_g = lib.hrl_gboard_pack_bytes(4 * H * L, H)
    code = lib.hrl_gboard_forward_groups(cast(xs), cast(strides), N, H, L, dummy, need_g - 16, 4 * H * L, dummy,
                                         4 * H * L * 36, None)
    assert code == _native.HRL_EINVAL


def test_gboard_conv_refuses_packed_weights_of_another_shape():
    """The Python boundary refuses a packed buffer smaller than hrl_gboard_pack_bytes(Cout, Cin_g) (or of another
    dtype) before any launch (no GPU needed); the C entry checks the size again."""
    import torch
    from handyrl_amd import nn as hnn
    lib = _native.load()
    need = lib.hrl_gboard_pack_bytes(64, 32)
    x = torch.zeros(1, 32, 6, 6)
    with pytest.raises(ValueError):
        hnn.gboard_conv(x, torch.zeros(need - 16, dtype=torch.uint8), 64, 32)
    with pytest.raises(ValueError):
        hnn.gboard_conv(x, torch.zeros(need // 4, dtype=torch.float32), 64, 32)


# ---- the recurrent-state, masked-rows and LSTM-gate entry points: argument validation (before any HIP call)

def _fake(n, null_at=None):
    """n distinct non-NULL, 16-byte aligned fake device addresses (never dereferenced: every call below returns
    from the argument checks, or from the empty-batch exit)."""
    vals = [4096 * (i + 1) for i in range(max(n, 1))]
    if null_at is not None:
        vals[null_at] = None
    return (ctypes.c_void_p * len(vals))(*vals)


def _hidden_codes(n=2, F=(8, 12), B=4, P=2, Pn=1, null_leaf=False, add_strides=None, dgathered=True, dstate=True,
                  only=None):
    """The return code of every hrl_hidden_* entry point (or those named in `only`) for one argument set."""
    lib = _native.load()
    m = max(n, 1)
    Fv = (ctypes.c_int64 * m)(*[F[i % len(F)] for i in range(m)])
    null_at = m - 1 if null_leaf else None
    a, b, c, d = _fake(m, null_at), _fake(m), _fake(m, null_at), _fake(m)
    add = _fake(m)
    st = (ctypes.c_int64 * m)(*(add_strides or [Fv[i] + 4 for i in range(m)]))
    mask = ctypes.c_void_p(64)
    calls = {
        'gather': lambda s: lib.hrl_hidden_gather(a, mask, B, P, n, Fv, s, c, None),
        'gather_backward': lambda s: lib.hrl_hidden_gather_backward(a, mask, B, P, n, Fv, s, c, None),
        'gather_backward_add': lambda s: lib.hrl_hidden_gather_backward_add(a, mask, B, P, n, Fv, s, add, st, c,
                                                                            None),
        'update': lambda s: lib.hrl_hidden_update(a, b, Pn, mask, B, P, n, Fv, c, None),
        'update_backward': lambda s: lib.hrl_hidden_update_backward(a, mask, B, P, Pn, n, Fv, c, d, None),
        'update_backward_add': lambda s: lib.hrl_hidden_update_backward_add(a, mask, B, P, Pn, n, Fv, add, st, c, d,
                                                                            None),
        'update_gather': lambda s: lib.hrl_hidden_update_gather(a, b, Pn, mask, mask, B, P, n, Fv, s, c, d, None),
        'update_gather_backward': lambda s: lib.hrl_hidden_update_gather_backward(
            a if dgathered else _fake(m, 0), mask, mask, B, P, Pn, n, Fv, s, add if dstate else None, st, add, st,
            c, d, None),
    }
    return {(k, s): f(s) for k, f in calls.items() if only is None or k in only for s in (0, 1)}


def test_hidden_entry_points_validate_arguments():
    """hrl_hidden_*: HRL_EINVAL for 0 or 17 leaves, Pn not in {1, P}, F < 1, a NULL leaf pointer, an addend row
    stride below F and a leaf with neither a gathered-input nor a state gradient; HRL_OK for an empty batch."""
    EINVAL = _native.HRL_EINVAL
    assert set(_hidden_codes(B=0).values()) == {_native.HRL_OK}
    assert set(_hidden_codes(B=0, n=16, Pn=2).values()) == {_native.HRL_OK}
    for kw in ({'n': 0}, {'n': 17}, {'F': (8, 0)}, {'F': (-4, 8)}, {'null_leaf': True}):
        assert set(_hidden_codes(**kw).values()) == {EINVAL}, kw
    with_pn = ('update', 'update_backward', 'update_backward_add', 'update_gather', 'update_gather_backward')
    for Pn in (0, 2, 4):
        assert set(_hidden_codes(P=3, Pn=Pn, only=with_pn).values()) == {EINVAL}, Pn
    with_addend = ('gather_backward_add', 'update_backward_add', 'update_gather_backward')
    assert set(_hidden_codes(add_strides=[8, 11], only=with_addend).values()) == {EINVAL}
    assert set(_hidden_codes(add_strides=[7, 12], only=with_addend).values()) == {EINVAL}
    fused = ('update_gather_backward',)
    assert set(_hidden_codes(dgathered=False, dstate=False, only=fused).values()) == {EINVAL}
    # a NULL gathered-input gradient is fine when that leaf's state gradient is given
    assert set(_hidden_codes(B=0, dgathered=False, only=fused).values()) == {_native.HRL_OK}


def test_masked_rows_copy_validates_arguments():
    """hrl_masked_rows_copy: HRL_EINVAL for a row stride below F (either side) and for 17 leaves; E = 0 is OK."""
    lib = _native.load()
    mask = ctypes.c_void_p(64)

    def code(n=2, dst_stride=(40, 40), src_stride=(36, 72), E=5):
        m = max(n, 1)
        F = (ctypes.c_int64 * m)(*[36] * m)
        ds = (ctypes.c_int64 * m)(*[dst_stride[i % 2] for i in range(m)])
        ss = (ctypes.c_int64 * m)(*[src_stride[i % 2] for i in range(m)])
        return lib.hrl_masked_rows_copy(n, _fake(m), ds, _fake(m), ss, F, mask, E, None)

    assert code(E=0) == _native.HRL_OK and code(n=16, E=0) == _native.HRL_OK
    assert code(dst_stride=(40, 35)) == _native.HRL_EINVAL
    assert code(src_stride=(35, 72)) == _native.HRL_EINVAL
    assert code(n=17) == _native.HRL_EINVAL and code(n=17, E=0) == _native.HRL_EINVAL
    assert code(n=0) == _native.HRL_EINVAL


def test_lstm_gates_entry_points_validate_arguments():
    """hrl_lstm_gates_*: HRL_EINVAL for a bias without zx, zx_stride < 4 H HW, dh_parts < 1 and L = 5; HRL_OK for
    N = 0."""
    lib = _native.load()
    x = ctypes.c_void_p(4096)
    H, HW = 4, 9
    row = 4 * H * HW
    EINVAL, OK = _native.HRL_EINVAL, _native.HRL_OK

    def forward(N=2, zx=x, zx_stride=row, bias=None):
        return lib.hrl_lstm_gates_forward(zx, zx_stride, x, x, N, H, HW, bias, 1, x, x, None, None)

    def grouped(N=2, L=3, zx_strides=(row, row + 4, 2 * row), zh_extra=8):
        m = max(L, 1)
        st = (ctypes.c_int64 * m)(*[zx_strides[i % 3] for i in range(m)])
        return lib.hrl_lstm_gates_forward_grouped(L, x, L * row + zh_extra, _fake(m), st, _fake(m), N, H, HW,
                                                  _fake(m), _fake(m), None, None)

    def backward_ex(N=2, parts=4):
        return lib.hrl_lstm_gates_backward_ex(x, x, x, x, 4 * H * HW, parts, H * HW, x, N, H, HW, x, x, None, 1,
                                              None)

    assert forward(zx=None, zx_stride=0, bias=x) == EINVAL
    assert forward(zx_stride=row - 1) == EINVAL
    assert grouped(zx_strides=(row, row - 1, row)) == EINVAL
    assert grouped(zh_extra=-1) == EINVAL
    assert grouped(L=5) == EINVAL and grouped(L=0) == EINVAL
    assert backward_ex(parts=0) == EINVAL and backward_ex(parts=-1) == EINVAL
    assert forward(N=0) == OK and grouped(N=0) == OK and grouped(N=0, L=4) == OK and backward_ex(N=0) == OK
    assert lib.hrl_lstm_gates_backward(x, x, x, x, x, 0, H, HW, x, x, None) == OK


# ---- the fused loss entry points: argument validation (before any HIP call)

def _loss_forward_code(B=4, T=8, P=2, Pp=1, A=9, null=(), vt=3, pt=2, symmetrize=1, ws_short=0):
    """hrl_loss_forward on fake device addresses; `null` names the pointer arguments passed as NULL."""
    lib = _native.load()
    names = ('tpol', 'bpol', 'action', 'emask', 'tmask', 'omask', 'progress', 'value', 'outcome', 'ret_out', 'ret',
             'reward', 'workspace', 'losses')
    assert set(null) <= set(names)
    a = {n: None if n in null else ctypes.c_void_p(4096 * (i + 1)) for i, n in enumerate(names)}
    size = lib.hrl_loss_workspace_bytes(B, T, P, Pp)
    size = (size if size > 0 else 1 << 20) - ws_short
    return lib.hrl_loss_forward(a['tpol'], a['bpol'], a['action'], B, T, P, Pp, A, a['emask'], a['tmask'], a['omask'],
                                a['progress'], a['value'], a['outcome'], a['ret_out'], a['ret'], a['reward'], vt, pt,
                                symmetrize, 0.7, 0.8, 0.1, 0.1, a['workspace'], size, a['losses'], None)


def _loss_backward_code(B=4, T=8, P=2, Pp=1, A=9, null=(), ws_short=0):
    lib = _native.load()
    names = ('tpol', 'action', 'emask', 'tmask', 'omask', 'progress', 'value', 'ret_out', 'workspace', 'dlosses',
             'g_tpol', 'g_value', 'g_ret')
    assert set(null) <= set(names)
    a = {n: None if n in null else ctypes.c_void_p(4096 * (i + 1)) for i, n in enumerate(names)}
    size = lib.hrl_loss_workspace_bytes(B, T, P, Pp)
    size = (size if size > 0 else 1 << 20) - ws_short
    return lib.hrl_loss_backward(a['tpol'], a['action'], B, T, P, Pp, A, a['emask'], a['tmask'], a['omask'],
                                 a['progress'], a['value'], a['ret_out'], 0.1, 0.1, a['workspace'], size,
                                 a['dlosses'], a['g_tpol'], a['g_value'], a['g_ret'], None)


BAD_LOSS_DIMS = ({'B': 0}, {'B': -1}, {'T': 0}, {'P': 0, 'Pp': 0}, {'P': 0}, {'P': 65, 'Pp': 65}, {'P': 65},
                 {'P': 4, 'Pp': 2}, {'P': 4, 'Pp': 0}, {'P': 2, 'Pp': 3})


def test_loss_workspace_bytes_validates_dimensions():
    """hrl_loss_workspace_bytes: -1 for B < 1, T < 1, P in {0, 65} and Pp not in {1, P}; otherwise room for the
    3 policy-shaped, 5 value-shaped and 1 step-shaped float arrays the backward reads."""
    lib = _native.load()
    for kw in BAD_LOSS_DIMS:
        d = dict({'B': 4, 'T': 8, 'P': 2, 'Pp': 1}, **kw)
        assert lib.hrl_loss_workspace_bytes(d['B'], d['T'], d['P'], d['Pp']) == -1, kw
    for B, T, P, Pp in ((1, 1, 1, 1), (4, 8, 2, 1), (3, 33, 64, 64), (3, 100, 5, 1), (16389, 33, 8, 8),
                        (4097, 3, 2, 2)):
        BT = B * T
        assert lib.hrl_loss_workspace_bytes(B, T, P, Pp) >= 4 * (3 * BT * Pp + 5 * BT * P + BT), (B, T, P, Pp)


def test_loss_forward_validates_arguments():
    """hrl_loss_forward: HRL_EINVAL for bad dimensions, A < 1, each required pointer NULL, value without outcome,
    ret_out without ret or reward, symmetrize with P != 2, an algorithm outside MC..VTRACE and a workspace one
    byte short.  No case gets as far as a launch."""
    EINVAL = _native.HRL_EINVAL
    for kw in BAD_LOSS_DIMS:
        assert _loss_forward_code(symmetrize=0, **kw) == EINVAL, kw
    for A in (0, -3):
        assert _loss_forward_code(A=A) == EINVAL, A
    for name in ('tpol', 'bpol', 'action', 'emask', 'tmask', 'omask', 'progress', 'losses', 'workspace'):
        assert _loss_forward_code(null=(name,)) == EINVAL, name
    assert _loss_forward_code(null=('outcome',)) == EINVAL
    assert _loss_forward_code(null=('ret',)) == EINVAL
    assert _loss_forward_code(null=('reward',)) == EINVAL
    for P, Pp in ((1, 1), (3, 1), (3, 3), (64, 1)):
        assert _loss_forward_code(P=P, Pp=Pp, symmetrize=1) == EINVAL, (P, Pp)
    for vt, pt in ((-1, 0), (4, 0), (0, -1), (0, 4), (7, 7)):
        assert _loss_forward_code(vt=vt, pt=pt) == EINVAL, (vt, pt)
    assert _loss_forward_code(ws_short=1) == EINVAL
    assert _loss_forward_code(P=3, Pp=3, symmetrize=0, null=('value', 'outcome', 'ret_out', 'ret', 'reward'),
                              ws_short=1) == EINVAL


def test_loss_backward_validates_arguments():
    """hrl_loss_backward: HRL_EINVAL for bad dimensions, g_value without value, g_ret without ret_out, NULL dlosses
    or g_tpol (or any other required pointer) and a short workspace."""
    EINVAL = _native.HRL_EINVAL
    for kw in BAD_LOSS_DIMS:
        assert _loss_backward_code(**kw) == EINVAL, kw
    assert _loss_backward_code(A=0) == EINVAL
    assert _loss_backward_code(null=('value',)) == EINVAL
    assert _loss_backward_code(null=('ret_out',)) == EINVAL
    for name in ('dlosses', 'g_tpol', 'tpol', 'action', 'emask', 'tmask', 'omask', 'progress', 'workspace'):
        assert _loss_backward_code(null=(name,)) == EINVAL, name
    assert _loss_backward_code(ws_short=1) == EINVAL
    assert _loss_backward_code(null=('value', 'g_value', 'ret_out', 'g_ret'), ws_short=1) == EINVAL
