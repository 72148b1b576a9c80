"""The step tail and the clip (csrc/hrl_optim.hip): argument validation before any HIP call, and the size functions
(no GPU).  Every call below is complete but for one argument; the pointers are not device memory, so a launch would
fault."""

import ctypes

import pytest

from handyrl_amd import _native

EINVAL = _native.HRL_EINVAL
i64 = _native.i64_array


def _p(i):
    return ctypes.c_void_p(4096 * (i + 1))


def _ptrs(values):
    return (ctypes.c_void_p * max(len(values), 1))(*values)


def _ints(values):
    return (ctypes.c_int * max(len(values), 1))(*values)


# ------------------------------------------------------------------------------------------------ hrl_grad_fold_norm
N = 20000
FOLD = dict(parts=4096 * 20, strides=9300, col0=50, nparts=3, dst=100, count=64, modes=0)
TABLES = ('parts', 'strides', 'col0', 'nparts', 'dst', 'count', 'modes')


def fold_call(ex=False, n=N, folds=(FOLD,), null=None, step=True, counters=(4096 * 30,), increments=(1,),
              null_increments=False, ncounters=None, nfolds=None, norm_bytes=None, loss=None):
    """hrl_grad_fold_norm[_ex] with fake pointers; `null` names a table (or 'grads', 'norm_part', 'counters') passed as
    NULL."""
    lib = _native.load()
    tab = {k: [f[k] for f in folds] for k in TABLES}
    arrays = {k: (_ptrs(tab[k]) if k == 'parts' else _ints(tab[k]) if k == 'modes' else i64(tab[k] or [0]))
              for k in TABLES}
    arg = lambda k: None if null == k else arrays[k]
    blocks = (max(n, 1) + 63) // 64
    args = [None if null == 'grads' else _p(0), n, *[arg(k) for k in TABLES],
            len(folds) if nfolds is None else nfolds, _p(1) if step else None,
            None if null == 'counters' else _ptrs(list(counters)),
            None if null_increments else i64(list(increments) or [0]),
            len(counters) if ncounters is None else ncounters,
            None if null == 'norm_part' else _p(2), blocks * 8 if norm_bytes is None else norm_bytes]
    if ex or loss is not None:
        part, nparts, losses = loss if loss is not None else (None, 0, None)
        return lib.hrl_grad_fold_norm_ex(*args, part, nparts, 0.01, losses, None)
    return lib.hrl_grad_fold_norm(*args, None)


CONV = dict(FOLD, count=9216, strides=9300, col0=50, modes=1)
FOLD_CASES = {
    'n_0': dict(n=0, folds=()),
    'grads_null': dict(null='grads'),
    'norm_part_null': dict(null='norm_part'),
    'nfolds_17': dict(folds=[dict(FOLD, dst=64 * k) for k in range(17)]),
    'nfolds_negative': dict(folds=(), nfolds=-1),
    'ncounters_9': dict(counters=[4096 * (30 + k) for k in range(9)], increments=[1] * 9),
    'ncounters_negative': dict(counters=(), ncounters=-1),
    'norm_part_one_double_short': dict(norm_bytes=((N + 63) // 64 - 1) * 8),
    'dst_plus_count_past_n': dict(folds=[dict(FOLD, dst=N - 63)]),
    'dst_negative': dict(folds=[dict(FOLD, dst=-1)]),
    'col0_negative': dict(folds=[dict(FOLD, col0=-1)]),
    'stride_below_col0_plus_span': dict(folds=[dict(FOLD, strides=50 + 63)]),
    'stride_below_col0_plus_span_mode1': dict(folds=[dict(CONV, strides=50 + 9215)]),
    'nparts_0': dict(folds=[dict(FOLD, nparts=0)]),
    'count_0': dict(folds=[dict(FOLD, count=0)]),
    'mode_2': dict(folds=[dict(FOLD, modes=2)]),
    'mode_1_count_not_9216': dict(folds=[dict(CONV, count=9215)]),
    'part_null': dict(folds=[dict(FOLD, parts=None)]),
    'counter_null': dict(counters=(4096 * 30, None), increments=(1, 1)),
    'increment_negative': dict(counters=(4096 * 30, 4096 * 31), increments=(1, -1)),
    # the new rules: NULL tables, and two folds on one destination (the kernel would apply only the last)
    **{'%s_table_null' % k: dict(null=k) for k in TABLES},
    'counters_table_null': dict(null='counters'),
    'folds_overlap_same_range': dict(folds=[FOLD, dict(FOLD, parts=4096 * 21)]),
    'folds_overlap_by_one': dict(folds=[FOLD, dict(FOLD, dst=100 + 63)]),
    'folds_overlap_by_one_before': dict(folds=[dict(FOLD, dst=100 + 63), FOLD]),
    'folds_overlap_contained': dict(folds=[dict(CONV, dst=0), dict(FOLD, dst=5000, count=1)]),
    'folds_overlap_third': dict(folds=[FOLD, dict(FOLD, dst=164), dict(CONV, dst=200)]),
    'loss_nparts_0': dict(loss=(_p(5), 0, _p(6))),
    'losses_null': dict(loss=(_p(5), 3, None)),
    'loss_part_misaligned': dict(loss=(ctypes.c_void_p(4096 * 6 + 4), 3, _p(6))),
}


@pytest.mark.parametrize('ex', [False, True])
@pytest.mark.parametrize('case', sorted(FOLD_CASES))
def test_grad_fold_norm_einval_before_any_hip_call(case, ex):
    assert fold_call(ex=ex, **FOLD_CASES[case]) == EINVAL


def test_grad_fold_norm_blocks():
    lib = _native.load()
    assert [lib.hrl_grad_fold_norm_blocks(n) for n in (-1, 0, 1, 63, 64, 65, 128, 129)] == [-1, -1, 1, 1, 1, 2, 2, 3]


# ------------------------------------------------------------------------------------------------ hrl_adam_clip
ADAM_POINTERS = ('grads', 'norm_part', 'total_norm', 'params', 'offsets', 'live', 'exp_avg', 'exp_avg_sq', 'lr', 'step')


def adam_call(null=None, n=1000, offsets=(0, 300, 300, 1000), params=None, nacc=0, acc_src=True, acc_dst=True,
              ntensors=None):
    lib = _native.load()
    nt = len(offsets) - 1 if ntensors is None else ntensors
    params = [4096 * (40 + k) for k in range(max(nt, 1))] if params is None else params
    ptr = {k: _p(10 + j) for j, k in enumerate(ADAM_POINTERS)}
    ptr.update(params=_ptrs(params), offsets=i64(list(offsets)), live=_ints([1] * max(nt, 1)))
    a = {k: (None if null == k else v) for k, v in ptr.items()}
    return lib.hrl_adam_clip(a['grads'], n, a['norm_part'], 4.0, a['total_norm'], a['params'], a['offsets'], a['live'],
                             nt, a['exp_avg'], a['exp_avg_sq'], a['lr'], a['step'], 0.9, 0.999, 1e-8, 1e-5,
                             _ptrs([None] * max(nacc, 1)) if acc_src else None, nacc, _p(30) if acc_dst else None, None)


ADAM_CASES = {
    **{'%s_null' % k: dict(null=k) for k in ADAM_POINTERS},
    'n_0': dict(n=0, offsets=(0, 0)),
    'ntensors_0': dict(offsets=(0,), ntensors=0),
    'ntensors_65': dict(offsets=tuple(range(65)) + (1000,)),
    'first_offset_not_0': dict(offsets=(1, 300, 1000)),
    'last_offset_not_n': dict(offsets=(0, 300, 999)),
    'last_offset_past_n': dict(offsets=(0, 300, 1001)),
    'offset_decreasing': dict(offsets=(0, 300, 299, 1000)),
    'param_null': dict(params=[4096 * 40, None, 4096 * 42]),
    'nacc_9': dict(nacc=9),
    'nacc_negative': dict(nacc=-1),
    'acc_src_null': dict(nacc=1, acc_src=False),
    'acc_dst_null': dict(nacc=1, acc_dst=False),
}


@pytest.mark.parametrize('case', sorted(ADAM_CASES))
def test_adam_clip_einval_before_any_hip_call(case):
    assert adam_call(**ADAM_CASES[case]) == EINVAL


# ------------------------------------------------------------------------------------------------ hrl_clip_grad_norm
def test_clip_grad_norm_einval_before_any_hip_call():
    lib = _native.load()
    for g, n, t in ((None, 8, _p(1)), (_p(0), 8, None), (ctypes.c_void_p(4096 + 4), 8, _p(1)), (_p(0), -1, _p(1))):
        assert lib.hrl_clip_grad_norm(g, n, 4.0, t, None) == EINVAL
        assert lib.hrl_clip_grad_norm_ws(g, n, 4.0, t, _p(2), 512, None) == EINVAL


@pytest.mark.parametrize('n', [65537, 1 << 20])
def test_clip_grad_norm_ws_workspace_rules_above_the_switch(n):
    lib = _native.load()
    need = lib.hrl_clip_workspace_bytes(n)
    assert need == 512
    for ws, nbytes in ((None, need), (_p(2), need - 1), (_p(2), 0), (ctypes.c_void_p(4096 * 3 + 4), need)):
        assert lib.hrl_clip_grad_norm_ws(_p(0), n, 4.0, _p(1), ws, nbytes, None) == EINVAL


def test_clip_workspace_bytes():
    lib = _native.load()
    assert [lib.hrl_clip_workspace_bytes(n) for n in (-1, 0, 1, 65536, 65537)] == [-1, 512, 512, 512, 512]
