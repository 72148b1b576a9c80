"""hrl_compute_targets_strided: argument validation, which returns before any HIP call (no GPU needed).

The pointers are fake device addresses that are never dereferenced.
"""

import ctypes

import pytest

from handyrl_amd import _native

VALUES, RETURNS, REWARDS, RHOS, CS = range(5)


def _call(tgt_alg=1, adv_alg=1, B=4, T=8, P=2, K=1, ret_T=1, strides='canonical', null=(), targets=False,
          edit=None):
    """The return code of one call.  `null` names operands passed as NULL, `edit` maps (operand, axis) to a stride
    that replaces the canonical one."""
    lib = _native.load()
    C = P * K
    rows = []
    for op in range(5):
        Tx = ret_T if op == RETURNS else T
        rows += [Tx * C, C, K, 1]
    for (op, axis), value in (edit or {}).items():
        rows[4 * op + axis] = value
    arr = None if strides is None else (ctypes.c_int64 * 20)(*rows)
    ops = [None if i in null else ctypes.c_void_p(4096 * (i + 1)) for i in range(5)]
    tgt = ctypes.c_void_p(4096 * 7) if targets else None
    adv = None if 'advantages' in null else ctypes.c_void_p(4096 * 8)
    return lib.hrl_compute_targets_strided(tgt_alg, adv_alg, ops[0], ops[1], ops[2], ops[3], ops[4], arr,
                                           B, T, P, K, ret_T, 0.7, 1.0, tgt, adv, None)


@pytest.mark.parametrize('kw', [
    {'strides': None},                                  # NULL strides
    {'edit': {(VALUES, 1): -2}},                        # a negative stride
    {'edit': {(CS, 0): -1}, 'tgt_alg': 3, 'adv_alg': 3},
    {'P': 13, 'K': 5},                                  # P*K = 65
    {'P': 65, 'K': 1},
    {'P': 0}, {'K': 0}, {'P': -1, 'K': -1},
    {'ret_T': 3},                                       # returns time extent not in {1, T}
    {'T': 0},
    {'tgt_alg': 0, 'adv_alg': 0, 'targets': True},      # MC writes no targets
    {'tgt_alg': 0, 'adv_alg': 1, 'targets': True},
    {'tgt_alg': 3, 'adv_alg': 3, 'null': (RHOS,)},      # V-trace without rhos
    {'tgt_alg': 1, 'adv_alg': 3, 'null': (CS,)},        # ... or cs, for either algorithm of the pair
    {'tgt_alg': 7, 'adv_alg': 1},                       # unknown algorithm
    {'tgt_alg': 1, 'adv_alg': -1},
    {'null': (VALUES,)}, {'null': (RETURNS,)}, {'null': ('advantages',)},
    # the inner offset (T-1)*sT + (P-1)*sP + (K-1)*sK must stay below 2^31 elements: the kernels add it as an int
    {'edit': {(VALUES, 1): 1 << 30}},                   # 7 * 2^30
    {'edit': {(REWARDS, 2): 1 << 31}},
    {'K': 3, 'edit': {(RETURNS, 3): 1 << 31}},
    {'B': 1 << 20, 'edit': {(VALUES, 0): 1 << 41}},     # largest offset 2^61 elements
])
def test_invalid_arguments_rejected_without_gpu(kw):
    assert _call(**kw) == _native.HRL_EINVAL


def test_empty_batch_is_ok_with_null_pointers():
    everything = (VALUES, RETURNS, REWARDS, RHOS, CS, 'advantages')
    assert _call(B=0, null=everything) == _native.HRL_OK
    assert _call(B=0, null=everything, tgt_alg=3, adv_alg=2, K=3) == _native.HRL_OK
    # the strides rows of NULL operands are not looked at
    assert _call(B=0, null=everything, edit={(REWARDS, 0): -5, (RHOS, 3): -1}) == _native.HRL_OK


def test_ignored_rows_and_axes_do_not_reject():
    """With B = 0 nothing is launched, so these reach the end of validation: a negative entry in the row of a NULL
    operand is ignored, one in the row of a present operand is not."""
    assert _call(B=0, null=(REWARDS,), edit={(REWARDS, 1): -7}) == _native.HRL_OK
    assert _call(B=0, edit={(REWARDS, 1): -7}) == _native.HRL_EINVAL


def test_abi_version_is_30():
    assert _native.ABI_VERSION == 30 and _native.load().hrl_abi_version() == 30
