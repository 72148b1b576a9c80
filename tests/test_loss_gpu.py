"""The fused learner loss (csrc/hrl_loss.hip, csrc/hrl_scan.h) called directly, against a float64 reference, at
the shapes where its control flow changes.

Every case (tests/test_loss_reference.py:make_case) is a set of leaf tensors for outputs['policy' | 'value' |
'return'] and a batch.  handyrl_amd.train.loss_terms runs on it on the GPU and sum_k w_k losses[k] is
backpropagated, w random with a zero and a negative entry.  Three parties:

    kernel     loss_terms, the two forward launches and the one backward launch of hrl_loss.hip
    oracle32   oracle.learner.loss_from_outputs in float32 on the CPU: the reference project's arithmetic
    ref64      tests/test_loss_reference.py:reference_loss in float64

Criterion, for each of the five losses and each gradient tensor (the form and the factor 4 of
tests/test_plumbing_gpu.py):

    err_kernel <= 4 err_oracle32 + c scale

with the errors against ref64 (largest element for a tensor), scale = max|ref64| for a tensor and the sum of
|terms| for a loss.  dcnt is exact.  c comes from the oracle alone: its own err / scale, largest over ALL the
cases below, rounded up to a power of two and never below 2^-23 (`python -m tests.test_loss_gpu` recomputes the
middle column on a CPU; the kernel is not involved).  Worst ratios err / scale over all cases:

    quantity    oracle32     c        kernel (MI355X)
    p           4.74e-07     2^-21    4.74e-07
    v           1.95e-07     2^-22    1.67e-07
    r           1.45e-07     2^-22    1.19e-07
    ent         1.81e-07     2^-22    9.80e-08
    total       2.47e-07     2^-21    2.47e-07
    dpolicy     7.65e-07     2^-20    5.70e-07
    dvalue      5.35e-07     2^-20    6.85e-07
    dreturn     2.74e-06     2^-18    2.29e-06

(The oracle's column is the larger of two hosts' figures: its sums depend on the CPU's vector width and thread
count; they differed only in ent, 1.59e-07 / 1.81e-07, and total, 2.38e-07 / 2.47e-07.)  The kernel's error was
at most 0.52 of its bound in any case (v at seam-T31-VTRACE-VTRACE); the gradients stayed below 0.27 of theirs.
The return head's gradient has the largest ratio on every side because its scale is at most |w| (the residual is
clamped to +-1) while its error is that of a target of magnitude ~10 summed over T steps.

Bit-level: hrl_scan.h promises the reference's float operations in the reference's order, so with an upstream
gradient that is one-hot on v (on r) the value (return) gradient is (value - target) omask
(clamp(ret - target, +-1) omask) and must EQUAL oracle32's for value_target in {MC, TD, UPGO} (V-trace runs the
device's expf inside its targets), at several tiles in T and several trajectories per wave.

Which case launches what (loss_fused_kernel<VT, PT, HV, HR, AK>; F/TOP are recur_chunk's chunk forms):

    (VT, PT)            all 16 at T = 35 with AK = 9 (pairs-*-A9) and AK = 0 (pairs-*-A70); the 8 seam pairs at
                        every T of seam-*
    (HV, HR)            heads-*: (1,1) (1,0) (0,1) (0,0) at P = 2 and 3, AK = 9 and 0; every other case (1,1).
                        The backward's NULL g_value / g_ret branches run in the same cases, loss_backward_kernel<9>
                        at A = 9 and loss_backward_wave_kernel at A = 70
    AK = 9              A = 9 (the default);  AK = 4: actions-A4-*, every ragged-* but ragged-B4097-*-A70;
    AK = 0              actions-A{1, 2, 63, 64, 65, 214}-*, pairs-*-A70, heads-*-A70, ragged-B4097-*-A70;
                        loss_backward_wave_kernel with BT = 85 (not a multiple of the 4 rows of a block): actions-*
    chunk forms         !F TOP alone, tc mod 4 = 1, 2, 3, 0: seam-T{1, 5}, T2, T{3, 15}, T4; F TOP alone: T16;
                        F below an !F TOP of 1, 2, 3 steps in one tile: T17, T18, T19; the same with the full chunks
                        in the tile below (the carry crosses the tile seam): T33, T34, T35 and T49, T65; T100: four
                        tiles, a full 4-step block on top; F TOP closing a tile: T32, T48, T64
    P, Pp               players-P{1, 2, 3, 5, 8, 64}-Pp{1, P}: the (g, c) lane map and the reciprocal divisions
                        by tc * P and P, Pp == P > 2 included; P = 2 without the symmetrisation: players-P2-*-solo
    G                   1: every case with B <= 5;  2: ragged-B4097-* (last wave 1 trajectory);  4: ragged-B8195-*
                        (3 of 4);  8: ragged-B16389-P2-* and -P8-* (5 of 8).  G P = 64: ragged-B8195-P16,
                        ragged-B16389-P8
    LDS                 ragged-B16389-P8-Pp1-T33 (TD, MC, both heads): 69 KB; the same with Pp = 8: 92 KB, the
                        largest request the dispatch can make (fused_lds_bytes)
"""

import math
import sys

import pytest
import torch

from tests.test_loss_reference import ALGS, error_ratios, evaluate, make_case, oracle32, reference64

pytestmark = pytest.mark.gpu

QUANTITIES = ('p', 'v', 'r', 'ent', 'total', 'dpolicy', 'dvalue', 'dreturn')
FLOOR = 2.0 ** -23
# the oracle's worst err / scale over CASES rounded up to a power of two (the table above), at least FLOOR
C = {'p': 2.0 ** -21, 'v': 2.0 ** -22, 'r': 2.0 ** -22, 'ent': 2.0 ** -22, 'total': 2.0 ** -21,
     'dpolicy': 2.0 ** -20, 'dvalue': 2.0 ** -20, 'dreturn': 2.0 ** -18}
assert all(c >= FLOOR for c in C.values()) and set(C) == set(QUANTITIES)

SEAM_T = (1, 2, 3, 4, 5, 15, 16, 17, 18, 19, 31, 32, 33, 34, 35, 48, 49, 64, 65, 100)
SEAM_PAIRS = [(a, a) for a in ALGS] + [('TD', 'VTRACE'), ('VTRACE', 'MC'), ('UPGO', 'TD'), ('MC', 'UPGO')]
RAGGED = ((4097, 2), (8195, 2), (16389, 2), (8195, 16), (16389, 8))


def _cases():
    """[(id, make_case arguments)]; lambda cycles through 0.7, 0, 1 and gamma through 0.8, 1 with the case index."""
    out = []

    def add(name, **kw):
        i = len(out)
        kw.setdefault('lmb', (0.7, 0.0, 1.0)[i % 3])
        kw.setdefault('gamma', (0.8, 1.0)[(i // 3) % 2])
        out.append((name, dict(kw, seed=i)))

    for T in SEAM_T:
        for vt, pt in SEAM_PAIRS:
            add('seam-T%d-%s-%s' % (T, vt, pt), B=3, T=T, vt=vt, pt=pt)
    for A in (9, 70):
        for vt in ALGS:
            for pt in ALGS:
                add('pairs-%s-%s-A%d' % (vt, pt, A), B=3, T=35, A=A, vt=vt, pt=pt)
    for A in (1, 2, 4, 9, 63, 64, 65, 214):
        for Pp in (1, 2):
            add('actions-A%d-Pp%d' % (A, Pp), B=5, T=17, A=A, Pp=Pp, vt='VTRACE', pt='UPGO')
    for P in (1, 2, 3, 5, 8, 64):
        for Pp in sorted({1, P}):
            add('players-P%d-Pp%d' % (P, Pp), B=3, T=33, P=P, Pp=Pp, vt='VTRACE', pt='UPGO')
    add('players-P2-Pp1-solo', B=3, T=33, P=2, Pp=1, vt='VTRACE', pt='TD', tbt=False)
    for P in (2, 3):
        for A in (9, 70):
            for heads in ((True, True), (True, False), (False, True), (False, False)):
                add('heads-v%dr%d-P%d-A%d' % (heads + (P, A)), B=3, T=33, P=P, A=A, heads=heads,
                    vt=('VTRACE', 'TD')[P % 2], pt=('UPGO', 'VTRACE')[P % 2])
    k = 0
    for B, P in RAGGED:
        for T in (3, 33):
            vt, pt = SEAM_PAIRS[k % len(SEAM_PAIRS)]
            k += 1
            if (B, P, T) == (16389, 8, 33):
                vt, pt = 'TD', 'MC'
            add('ragged-B%d-P%d-Pp1-T%d' % (B, P, T), B=B, T=T, P=P, A=4, vt=vt, pt=pt)
    add('ragged-B16389-P8-Pp8-T33', B=16389, T=33, P=8, Pp=8, A=4, vt='TD', pt='MC')
    add('ragged-B4097-P2-Pp1-T33-A70', B=4097, T=33, P=2, A=70, vt='VTRACE', pt='UPGO')
    return out


CASES = _cases()


def kernel(outputs, batch, args):
    """loss_terms, and the proof that the fused kernels (not the composed torch formulation) produced it."""
    from handyrl_amd.train import loss_terms
    losses, dcnt = loss_terms(outputs, batch, args)
    assert getattr(losses['total'], '_hrl_loss_vec', None) is not None, 'the composed path ran'
    return losses, dcnt


def _report(name, ek, eo):
    for q in ek:
        scale = ek[q][1]
        print('LOSSERR %s %s kernel %.4e oracle %.4e scale %.4e' % (name, q, ek[q][0], eo[q][0], scale))


@pytest.mark.parametrize('name,spec', CASES, ids=[n for n, _ in CASES])
def test_loss_vs_fp64(cuda, name, spec):
    case = make_case(**spec)
    ref, o32 = reference64(case), oracle32(case)
    got = evaluate(kernel, case, torch.float32, cuda)
    assert got['dcnt'] == ref['dcnt'] == o32['dcnt']
    assert set(got['losses']) == set(ref['losses']) and set(got['grads']) == set(ref['grads'])
    ek, eo = error_ratios(got, ref), error_ratios(o32, ref)
    _report(name, ek, eo)
    bad = {q: (ek[q][0], eo[q][0], ek[q][1]) for q in ek if not ek[q][0] <= 4 * eo[q][0] + C[q] * ek[q][1]}
    assert not bad, bad


def _bit_cases():
    shapes = [('T65', dict(B=3, T=65)), ('T35-P3-Pp3', dict(B=3, T=35, P=3, Pp=3)),
              ('B4097-T33', dict(B=4097, T=33, A=4)), ('B16389-T17', dict(B=16389, T=17, A=4))]
    out = []
    for i, vt in enumerate(('MC', 'TD', 'UPGO')):
        for j, (sname, kw) in enumerate(shapes):
            pt = ALGS[(i + j) % 4]
            out.append(('%s-%s-%s' % (sname, vt, pt), dict(kw, vt=vt, pt=pt, lmb=(0.7, 1.0)[j % 2],
                                                           gamma=(0.8, 1.0)[i % 2], seed=100 + 4 * i + j)))
    return out


BIT_CASES = _bit_cases()


@pytest.mark.parametrize('name,spec', BIT_CASES, ids=[n for n, _ in BIT_CASES])
def test_head_gradients_equal_the_oracle_bit_for_bit(cuda, name, spec):
    case = make_case(**spec)
    for k, head in ((1, 'value'), (2, 'return')):
        case['w'] = torch.zeros(5)
        case['w'][k] = 1.0
        o32 = oracle32(case)
        got = evaluate(kernel, case, torch.float32, cuda)
        assert got['losses'].keys() == o32['losses'].keys()
        assert torch.equal(got['grads'][head], o32['grads'][head]), \
            (name, head, float((got['grads'][head] - o32['grads'][head]).abs().max()))
        assert float(o32['grads'][head].abs().max()) > 0
        for other in ('policy', 'value', 'return'):
            if other != head:
                assert not bool(got['grads'][other].any()) and not bool(o32['grads'][other].any()), (name, other)


def test_ragged_wave_runs_are_deterministic(cuda):
    """Two runs of one case whose last wave holds 3 of its 4 trajectories: equal bits in every loss and gradient."""
    name, spec = next(c for c in CASES if c[0] == 'ragged-B8195-P16-Pp1-T33')
    case = make_case(**spec)
    a = evaluate(kernel, case, torch.float32, cuda)
    b = evaluate(kernel, case, torch.float32, cuda)
    assert a['losses'] == b['losses'] and a['dcnt'] == b['dcnt']
    for k in a['grads']:
        assert torch.equal(a['grads'][k], b['grads'][k]), k


def oracle_table(cases=CASES, out=sys.stdout):
    """The oracle's worst err / scale per quantity over the cases and the c that follows from it (CPU only)."""
    worst = {q: (0.0, '') for q in QUANTITIES}
    for name, spec in cases:
        case = make_case(**spec)
        eo = error_ratios(oracle32(case), reference64(case))
        for q, (err, scale) in eo.items():
            r = err / scale if scale > 0 else 0.0
            if r > worst[q][0]:
                worst[q] = (r, name)
    for q in QUANTITIES:
        r = worst[q][0]
        c = max(FLOOR, 2.0 ** math.ceil(math.log2(r))) if r > 0 else FLOOR
        print("%-9s oracle %.3e  c = 2^%d  (%s)" % (q, r, round(math.log2(c)), worst[q][1]), file=out)
    return worst


if __name__ == '__main__':
    oracle_table()
