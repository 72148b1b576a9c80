"""The step tail and the clip (csrc/hrl_optim.hip) at their C entries, on guard-band buffers (tests/guarded.py),
against the fp64 references of tests/step_tail_reference.py.

hrl_grad_fold_norm[_ex]: every partial-row count around the 8-chain main loop, folds inside, across and at the end
of 64-element blocks in both modes, NaN around every partial window, integer data (exact) and random data (one
rounding of the fold, one of the add, the fp64 accumulation).  hrl_adam_clip: sizes around the 256-workgroup cap,
tensor tables whose boundaries fall inside chunks, dead and zero-length tensors, parameters and both moments against
Adam in fp64 by the rounded-contract rule (the kernel's error at most twice the emulation's + 2^-24 |value|).
hrl_clip_grad_norm[_ws]: sizes around the float4 tail and the one-launch / two-launch switch.

Measured on an MI355X, the maxima over all 32 settings x 4 calls of test_adam_clip_against_fp64 (absolute error
against adam64, kernel / emulation): parameters 9.51e-8 / 9.51e-8, exp_avg 2.53e-8 / 2.53e-8, exp_avg_sq 1.61e-9 /
1.61e-9 -- the kernel rounds where the emulation rounds (in single settings the two differ in the last bit of a few
elements: 5.59e-8 against 5.87e-8 at the first).
"""

import ctypes
import math

import pytest
import torch

from handyrl_amd import _native
from tests.guarded import SENTINEL32, SENTINEL64, Arena, bits
from tests.step_tail_reference import (adam64, adam_emulated, block_sums64, clip64, fold64, fold_terms64)

pytestmark = pytest.mark.gpu
P = _native.ptr
i64 = _native.i64_array
NAN = float('nan')
EPS32 = 2.0 ** -24
MAX_NORM = 4.0


def ulp32(x):
    e = torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23)


# =========================================================================================== hrl_grad_fold_norm[_ex]
def make_fold(gen, stride_pad, col0, nparts, dst, count, mode, integer):
    """A fold whose partial rows have stride > col0 + span and NaN everywhere outside the windows."""
    span = 9216 if mode == 1 else count
    stride = col0 + span + stride_pad
    part = torch.full((nparts, stride), NAN)
    if integer:
        part[:, col0:col0 + span] = torch.randint(-4, 5, (nparts, span), generator=gen).float()
    else:
        part[:, col0:col0 + span] = torch.randn(nparts, span, generator=gen)
    return (part, stride, col0, nparts, dst, count, mode)


def launch_fold(cuda, flat, folds, step=0.0, counters=(), increments=None, loss=None, ex=False):
    """One hrl_grad_fold_norm[_ex] launch on guard-band buffers; returns what it left, on the CPU."""
    lib = _native.load()
    arena = Arena(cuda)
    n = flat.numel()
    g = arena.inout(flat, 'grads')
    parts = [arena.inout(f[0], 'part%d' % k) for k, f in enumerate(folds)]
    nb = lib.hrl_grad_fold_norm_blocks(n)
    assert nb == (n + 63) // 64
    norm_part = arena.out(nb, torch.float64, 'norm_part')
    step_t = arena.inout(torch.tensor(step), 'step') if step is not None else None
    ctrs = [arena.inout(torch.tensor(c, dtype=torch.int64), 'counter%d' % k) for k, c in enumerate(counters)]
    args = [P(g), n, _native.ptr_array(parts), i64([f[1] for f in folds] or [0]), i64([f[2] for f in folds] or [0]),
            i64([f[3] for f in folds] or [0]), i64([f[4] for f in folds] or [0]), i64([f[5] for f in folds] or [0]),
            (ctypes.c_int * max(len(folds), 1))(*[f[6] for f in folds]), len(folds), P(step_t),
            _native.ptr_array(ctrs), i64(list(increments)) if increments is not None else None, len(ctrs),
            P(norm_part), nb * 8]
    losses = None
    if loss is not None:
        lp = arena.inout(loss, 'loss_part')
        losses = arena.out(6, torch.float32, 'losses')
        rc = lib.hrl_grad_fold_norm_ex(*args, P(lp), loss.shape[0], 0.25, P(losses), _native.stream_of(cuda))
    elif ex:
        rc = lib.hrl_grad_fold_norm_ex(*args, None, 0, 0.0, None, _native.stream_of(cuda))
    else:
        rc = lib.hrl_grad_fold_norm(*args, _native.stream_of(cuda))
    _native.check(rc, 'hrl_grad_fold_norm')
    arena.check()
    for k, f in enumerate(folds):                       # the partial rows are inputs
        assert torch.equal(bits(parts[k].cpu()), bits(f[0])), 'partial rows %d changed' % k
    return dict(g=g.cpu(), norm_part=norm_part.cpu(), step=None if step_t is None else float(step_t),
                counters=[int(c) for c in ctrs], losses=None if losses is None else losses.cpu())


def covered(n, folds):
    c = torch.zeros(n, dtype=torch.bool)
    for f in folds:
        c[f[4]:f[4] + f[5]] = True
    return c


def check_fold(cuda, n, specs, integer, seed, step=0.0, counters=(), increments=None, ex=False):
    """Launch, and compare with fold64: the folded buffer, each block sum, the uncovered positions' bits, the step and
    the counters; then the same launch again on fresh copies of the inputs: the same bits."""
    gen = torch.Generator().manual_seed(seed)
    flat = (torch.randint(-5, 6, (n,), generator=gen).float() if integer else torch.randn(n, generator=gen))
    folds = [make_fold(gen, pad, col0, nparts, dst, count, mode, integer)
             for (pad, col0, nparts, dst, count, mode) in specs]
    got = launch_fold(cuda, flat, folds, step, counters, increments, ex=ex)
    ref, blocks = fold64(flat, folds)
    cov = covered(n, folds)
    assert torch.equal(bits(got['g'][~cov]), bits(flat[~cov])), 'a position outside every fold changed'
    assert not bool(got['g'].isnan().any()), 'a read outside a partial window (NaN) reached the gradients'
    if integer:
        assert torch.equal(got['g'].double(), ref)
        assert torch.equal(got['norm_part'], blocks)
    else:
        tol = torch.zeros(n, dtype=torch.float64)
        for f in folds:
            s, a = fold_terms64(f)
            sl = slice(f[4], f[4] + f[5])
            tol[sl] = EPS32 * (s.abs() + ref[sl].abs()) + f[3] * 2.0 ** -53 * a
        err = (got['g'].double() - ref).abs()
        assert bool((err <= tol).all()), 'fold: max error / bound %.3f' % float((err / tol.clamp_min(1e-300)).max())
        own = block_sums64(got['g'], n, folds)          # of the kernel's own stored values
        assert bool(((got['norm_part'] - own).abs() <= 64 * 2.0 ** -53 * own).all())
    assert got['step'] == (None if step is None else step + 1.0)
    incs = increments if increments is not None else [1] * len(counters)
    assert got['counters'] == [c + d for c, d in zip(counters, incs)]
    again = launch_fold(cuda, flat, folds, step, counters, increments, ex=ex)
    assert torch.equal(bits(again['g']), bits(got['g'])) and torch.equal(bits(again['norm_part']), bits(got['norm_part']))
    return flat, folds, got


# n = 37 + 9216 + 200 = 9453 (45 past a block boundary).  (stride pad, col0, nparts, dst, count, mode):
N_A = 9453


def layout_a(nparts):
    return [(7, 5, nparts, 37, 9216, 1),        # mode 1 at a dst that is no multiple of 64; ends inside block 144
            (5, 3, nparts, 9255, 10, 0),        # starts and ends inside block 144 ...
            (9, 1, nparts, 9265, 5, 0),         # ... and its neighbour in the same block, adjacent
            (3, 11, nparts, 9275, 70, 0),       # crosses the boundaries at 9280 and 9344
            (2, 4, nparts, 9400, 53, 0)]        # ends exactly at n, n % 64 != 0


@pytest.mark.parametrize('integer', [True, False], ids=['integers', 'random'])
@pytest.mark.parametrize('nparts', [1, 15, 16, 17, 127, 128, 129, 255, 256, 257])
def test_fold_partial_row_counts(cuda, nparts, integer):
    """16 waves take rows w, w + 16, ...; a round of the main loop is 128 rows.  1, 15: the remainder alone, some waves
    without a row; 16, 17: one row per wave, wave 0 a second; 127, 128, 129: wave 15 short of a round, exactly one
    round, wave 0 a round and a remainder; 255, 256, 257: the same around two rounds.  Random data: |got - ref| <=
    2^-24 (|fold| + |g + fold|) + nparts 2^-53 sum |terms|; each block sum within 64 2^-53 of the fp64 sum of
    squares of the stored values.  Integer data: everything equal."""
    check_fold(cuda, N_A, layout_a(nparts), integer, seed=100 + nparts, step=6.0, counters=(0, 41, 7),
               increments=(1, 16, 0))


@pytest.mark.parametrize('mode1_dst', [0, 64, 127])
def test_fold_mode1_destinations(cuda, mode1_dst):
    """The transposed fold at dst 0, at a multiple of 64 and one below the next, a mode-0 fold in front when there is
    room and one behind, n a multiple of 64."""
    n = 9216 + 192
    specs = [(1, 2, 19, mode1_dst, 9216, 1), (4, 6, 33, mode1_dst + 9216, 192 - mode1_dst, 0)]
    if mode1_dst:
        specs.append((2, 1, 5, 0, mode1_dst, 0))
    for integer in (True, False):
        check_fold(cuda, n, specs, integer, seed=7 + mode1_dst, step=None)


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_fold_smallest_buffers(cuda, n):
    """n of 1, 63, 64 and 65: no fold (nfolds 0: the buffer bit-unchanged, the block sums of it), one fold over the
    whole buffer, and folds of one element at both ends; step NULL; increments NULL (all 1); ncounters 0 and 8."""
    for integer in (True, False):
        check_fold(cuda, n, [], integer, seed=n, step=2.0, counters=tuple(range(8)), increments=None)
        check_fold(cuda, n, [(3, 2, 17, 0, n, 0)], integer, seed=n + 1, step=None, counters=(), increments=None)
        if n > 2:
            check_fold(cuda, n, [(1, 1, 3, 0, 1, 0), (6, 9, 130, n - 1, 1, 0)], integer, seed=n + 2, step=0.0,
                       counters=(5,), increments=(9,))


def test_fold_full_tables(cuda):
    """nfolds 16 (adjacent folds of 9 elements, so most cross a block boundary or share a block) and ncounters 8 with
    their own increments."""
    n = 16 * 9 + 5
    specs = [(1 + k % 3, k, 1 + 16 * k, 3 + 9 * k, 9, 0) for k in range(16)]
    for integer in (True, False):
        check_fold(cuda, n, specs, integer, seed=3, step=999.0, counters=tuple(10 * k for k in range(8)),
                   increments=tuple(range(8)))


def test_fold_with_the_loss_workgroup(cuda):
    """hrl_grad_fold_norm_ex with the loss workgroup behind the gradient blocks: the gradients and norm_part
    bit-identical to the launch without it (and to the _ex entry with loss_part NULL); the loss vector the fp64 sums
    of its partials."""
    gen = torch.Generator().manual_seed(21)
    flat = torch.randn(N_A, generator=gen)
    folds = [make_fold(gen, *spec, False) for spec in layout_a(37)]
    plain = launch_fold(cuda, flat, folds, 0.0, (3,), (2,))
    null = launch_fold(cuda, flat, folds, 0.0, (3,), (2,), ex=True)
    loss = torch.randn(300, 6, generator=gen, dtype=torch.float64)
    with_loss = launch_fold(cuda, flat, folds, 0.0, (3,), (2,), loss=loss)
    for other in (null, with_loss):
        assert torch.equal(bits(other['g']), bits(plain['g']))
        assert torch.equal(bits(other['norm_part']), bits(plain['norm_part']))
        assert other['step'] == 1.0 and other['counters'] == [5]
    s = loss.sum(0)
    want = torch.stack([s[0], s[1] / 2, s[2], s[3], s[0] + s[1] / 2 + s[2] - 0.25 * s[4], s[5]])
    assert bool(((with_loss['losses'].double() - want).abs() <= 4 * EPS32 * loss.abs().sum(0).max()).all())


# =========================================================================================== hrl_adam_clip
def tensor_table(kind, n):
    """(sizes, live) of a tensor table over n elements whose boundaries are no multiples of 256 (when n allows)."""
    if kind == 'one':
        return [n], [1]
    if kind == 'zero_length_middle':
        a = min(n, n * 2 // 5 + 1)
        return [a, 0, n - a], [1, 1, 1]
    if kind == 'dead_between_live':
        a, b = n * 3 // 10, n * 3 // 10 + (n * 9 // 20 + 1 if n > 2 else n)
        b = min(b, n)
        return [a, b - a, n - b], [1, 0, 1]
    assert kind == 'sixty_four'
    cuts = [0] + [int(n * (k + 0.37) / 64.5) for k in range(1, 64)] + [n]
    live = [1] * 64
    live[62] = live[5] = 0                              # tensor 63 (bit 63 of the mask) live, 62 dead
    return [b - a for a, b in zip(cuts, cuts[1:])], live


class AdamState:
    """Guard-band buffers of one hrl_adam_clip setting, reused over several steps."""

    def __init__(self, cuda, n, sizes, live, seed, nacc_sources=()):
        self.lib = _native.load()
        self.cuda, self.n, self.sizes, self.live = cuda, n, sizes, live
        self.gen = torch.Generator().manual_seed(seed)
        self.arena = a = Arena(cuda)
        self.g = a.inout(torch.zeros(n), 'grads')
        p0 = torch.randn(n, generator=self.gen) * 0.1
        # every tensor its own allocation; a zero-length one still needs a pointer: one float that must not change
        self.params = [a.inout(t.clone() if t.numel() else torch.tensor([123.0]), 'param%d' % k)
                       for k, t in enumerate(p0.split(sizes))]
        self.m = a.inout(torch.randn(n, generator=self.gen) * 0.01, 'exp_avg')
        self.v = a.inout(torch.rand(n, generator=self.gen) * 1e-4, 'exp_avg_sq')
        self.nb = self.lib.hrl_grad_fold_norm_blocks(n)
        self.norm_part = a.out(self.nb, torch.float64, 'norm_part')
        self.total = a.out((), torch.float32, 'total_norm')
        self.step = a.inout(torch.tensor(0.0), 'step')
        self.lr = a.inout(torch.tensor(0.0), 'lr')
        self.sources = [None if s is None else a.inout(torch.tensor(float(s)), 'acc_src%d' % k)
                        for k, s in enumerate(nacc_sources)]
        self.acc_dst = a.inout(torch.arange(8).float() * 0.5, 'acc_dst')
        offs = [0]
        for s in sizes:
            offs.append(offs[-1] + s)
        self.offsets = offs
        self.mask = torch.cat([torch.full((s,), bool(l)) for s, l in zip(sizes, live)]) if n else torch.zeros(0).bool()

    def p(self):
        for t, s in zip(self.params, self.sizes):
            assert s or float(t[0]) == 123.0, 'a zero-length tensor was written'
        return torch.cat([t.cpu().reshape(-1)[:s] for t, s in zip(self.params, self.sizes)])

    def call(self, grads, step, lr, wd):
        """The fold launch with nfolds 0 (norm_part, step + 1) and hrl_adam_clip; returns the state before and after."""
        lib, stream = self.lib, _native.stream_of(self.cuda)
        self.g.copy_(grads)
        self.step.fill_(step - 1)
        self.lr.fill_(lr)
        before = dict(p=self.p(), m=self.m.cpu(), v=self.v.cpu(), acc=self.acc_dst.cpu())
        _native.check(lib.hrl_grad_fold_norm(P(self.g), self.n, None, None, None, None, None, None, None, 0,
                                             P(self.step), None, None, 0, P(self.norm_part), self.nb * 8, stream),
                      'hrl_grad_fold_norm')
        nacc = len(self.sources)
        _native.check(lib.hrl_adam_clip(
            P(self.g), self.n, P(self.norm_part), MAX_NORM, P(self.total), _native.ptr_array(self.params),
            i64(self.offsets), (ctypes.c_int * len(self.live))(*self.live), len(self.live), P(self.m), P(self.v),
            P(self.lr), P(self.step), 0.9, 0.999, 1e-8, wd, _native.ptr_array(self.sources) if nacc else None, nacc,
            P(self.acc_dst) if nacc else None, stream), 'hrl_adam_clip')
        self.arena.check()
        assert float(self.step) == step
        after = dict(p=self.p(), m=self.m.cpu(), v=self.v.cpu(), g=self.g.cpu(), total=self.total.cpu(),
                     acc=self.acc_dst.cpu())
        return before, after


ERRORS = {}     # (quantity) -> (kernel's max error, emulation's max error), over every case of this process


def rounded_contract(name, got, emu, ref, mask):
    """The project's rule for a rounded contract (test_geesenet_bf16_gpu.as_good_as_the_emulation), per element of
    the live tensors: |kernel - fp64| <= 2 max|emulation - fp64| + 2^-24 |value|; NaN where the reference is NaN."""
    got, emu, ref = got.double()[mask], emu.double()[mask], ref[mask]
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan), '%s: NaN positions differ' % name
    ek, ee = (got - ref).abs()[~nan], (emu - ref).abs()[~nan]
    ee_max = float(ee.max()) if ee.numel() else 0.0
    ek_max = float(ek.max()) if ek.numel() else 0.0
    old = ERRORS.get(name, (0.0, 0.0))
    ERRORS[name] = (max(old[0], ek_max), max(old[1], ee_max))
    assert bool((ek <= 2 * ee_max + EPS32 * ref[~nan].abs()).all()), (name, ek_max, ee_max)
    return ek_max, ee_max


def check_adam_step(st, grads, step, lr, wd, expect_nonzero=True):
    """One call against the references, from the kernel's own state before it."""
    before, after = st.call(grads, step, lr, wd)
    g64 = grads.double()
    want, total_ref, coef_ref = clip64(grads, MAX_NORM)
    total = after['total']
    # the norm: within 2^-24 relative of fp64 (the same non-finite value when it is not finite)
    exact = g64.pow(2).sum().sqrt()
    if math.isfinite(float(exact)):
        assert abs(float(total) - float(exact)) <= EPS32 * float(exact), (float(total), float(exact))
    else:
        assert torch.equal(bits(total), bits(total_ref)) or (math.isnan(float(total)) and math.isnan(float(total_ref)))
    # the coefficient by clip_grad_norm_'s rule from the kernel's own norm (just checked), as clip64 forms it
    coef = torch.clamp(torch.tensor(MAX_NORM) / (total + torch.tensor(1e-6)), max=1.0)
    clipped = g64 * coef.double()
    nan = clipped.isnan()
    assert torch.equal(after['g'].isnan(), nan)
    if float(coef) == 1.0:
        assert torch.equal(bits(after['g']), bits(grads)), 'coef 1: the gradients keep their bits'
    assert bool(((after['g'].double() - clipped).abs()[~nan] <= ulp32(clipped)[~nan]).all())
    if torch.equal(bits(total), bits(total_ref)):       # the usual case: clip64 itself
        assert bool(((after['g'].double() - want).abs()[~nan] <= ulp32(want)[~nan]).all())
    # dead tensors: parameters and both moments keep their bits (the gradient above is scaled all the same)
    dead = ~st.mask
    for k in ('p', 'm', 'v'):
        assert torch.equal(bits(after[k][dead]), bits(before[k][dead])), 'dead tensor: %s changed' % k
    # live tensors: parameters and both moments against fp64 Adam on the clipped gradient
    lr32 = float(torch.tensor(lr, dtype=torch.float32))
    p64, m64, v64 = adam64(before['p'], clipped, before['m'], before['v'], step, lr32, wd=wd)
    pe, me, ve = adam_emulated(before['p'], after['g'], before['m'], before['v'], step, lr32, wd=wd)
    out = [rounded_contract(k, after[k], e, r, st.mask) for k, e, r in (('p', pe, p64), ('m', me, m64), ('v', ve, v64))]
    if expect_nonzero:
        assert all(ee > 0 for _, ee in out), 'the emulation shows no rounding: a vacuous bound'
    return before, after, out


def grads_of(st, scale):
    return torch.randn(st.n, generator=st.gen) * (scale / math.sqrt(st.n))


@pytest.mark.parametrize('table', ['one', 'sixty_four', 'zero_length_middle', 'dead_between_live'])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 65281, 65535, 65536, 65537])
def test_adam_clip_against_fp64(cuda, n, table):
    """Four calls per setting, each from the kernel's own state: step 1, 2, 1000 and 1e6, lr changed between calls,
    weight decay 1e-5 and 0 (the skipped branch), the norm below max_norm (coef exactly 1: the gradients keep their
    bits) and above it.  The norm within 2^-24 of fp64; the clipped gradient within one fp32 ulp of g coef; dead
    tensors' parameters and moments bit-unchanged; live parameters, exp_avg and exp_avg_sq within twice the
    emulation's error against adam64 plus 2^-24 |value| (the emulation's error non-zero).

    Measured on an MI355X, the maxima over all 32 settings (kernel / emulation, absolute, against adam64):
    parameters 9.51e-8 / 9.51e-8, exp_avg 2.53e-8 / 2.53e-8, exp_avg_sq 1.61e-9 / 1.61e-9 (the bound would allow
    twice the emulation's; it is not tightened to these)."""
    sizes, live = tensor_table(table, n)
    assert sum(sizes) == n and len(sizes) == len(live)
    st = AdamState(cuda, n, sizes, live, seed=n + len(sizes))
    nlive = int(st.mask.sum())
    for step, lr, wd, scale in ((1.0, 1e-3, 1e-5, 0.5), (2.0, 1e-3, 0.0, 40.0), (1000.0, 5e-4, 1e-5, 9.0),
                                (1e6, 2e-2, 0.0, 3.0)):
        _, after, out = check_adam_step(st, grads_of(st, scale), step, lr, wd, expect_nonzero=nlive >= 100)
        assert (float(after['total']) < MAX_NORM) == (scale < MAX_NORM) or n < 100
        print('n %d %s step %g: |error| against fp64, kernel / emulation: p %.3e / %.3e  exp_avg %.3e / %.3e  '
              'exp_avg_sq %.3e / %.3e' % (n, table, step, *out[0], *out[1], *out[2]))
    print('maxima so far (kernel, emulation):', ERRORS)


def test_adam_clip_exact_arithmetic(cuda):
    """Integer gradients with an integer norm: the norm equal; below max_norm the gradients keep their bits; with
    norm 8 (coef = 4 / (8 + 1e-6), one rounding) each gradient equals the float product."""
    st = AdamState(cuda, 260, [100, 60, 100], [1, 0, 1], seed=1)
    g = torch.zeros(260)
    g[3], g[150], g[259] = 1.0, -2.0, 2.0                            # norm 3
    _, after, _ = check_adam_step(st, g, 1.0, 1e-3, 0.0, expect_nonzero=False)
    assert float(after['total']) == 3.0 and torch.equal(bits(after['g']), bits(g))
    g = torch.zeros(260)
    g[0:64] = 1.0                                                    # norm 8
    _, after, _ = check_adam_step(st, g, 2.0, 1e-3, 1e-5, expect_nonzero=False)
    coef = torch.tensor(4.0) / (torch.tensor(8.0) + torch.tensor(1e-6))
    assert float(after['total']) == 8.0 and torch.equal(bits(after['g']), bits(g * coef))


@pytest.mark.parametrize('bad', ['nan', 'inf', '-inf'])
@pytest.mark.parametrize('n', [257, 65537])
def test_adam_clip_nonfinite(cuda, n, bad):
    """One NaN gradient: every gradient NaN, every live parameter NaN, dead ones unchanged.  One inf gradient: coef
    0, finite gradients 0, the inf element NaN; the parameters follow adam64 on those gradients."""
    sizes, live = tensor_table('dead_between_live', n)
    st = AdamState(cuda, n, sizes, live, seed=n)
    g = grads_of(st, 1.0)
    g[n // 7] = float(bad)                                           # in the first, live tensor
    assert bool(st.mask[n // 7])
    before, after, _ = check_adam_step(st, g, 3.0, 1e-3, 1e-5, expect_nonzero=False)
    if bad == 'nan':
        assert math.isnan(float(after['total'])) and bool(after['g'].isnan().all())
        assert bool(after['p'][st.mask].isnan().all())
    else:
        assert float(after['total']) == float('inf')
        finite = torch.ones(n, dtype=torch.bool)
        finite[n // 7] = False
        assert bool((after['g'][finite] == 0).all()) and math.isnan(float(after['g'][n // 7]))
        assert math.isnan(float(after['p'][n // 7])) and int(after['p'].isnan().sum()) == 1
    assert torch.equal(bits(after['p'][~st.mask]), bits(before['p'][~st.mask]))


@pytest.mark.parametrize('sources', [(None,), (1.5, None, -0.25, 3.0, None, 1e-3, 7.0, 0.0)], ids=['norm', 'eight'])
def test_adam_clip_accumulates_statistics(cuda, sources):
    """nacc 1 with a NULL source (the norm) and 8 with mixed sources: acc_dst[k] grows by exactly the source's fp32
    value, once per call, the rest of acc_dst untouched (nacc 0: every other test; acc_dst unchanged there)."""
    st = AdamState(cuda, 700, [300, 400], [1, 1], seed=4, nacc_sources=sources)
    for step in (1.0, 2.0):
        before, after, _ = check_adam_step(st, grads_of(st, 6.0), step, 1e-3, 0.0)
        src = torch.stack([after['total'] if s is None else torch.tensor(float(s)) for s in sources])
        k = len(sources)
        assert torch.equal(bits(after['acc'][:k]), bits(before['acc'][:k] + src))
        assert torch.equal(bits(after['acc'][k:]), bits(before['acc'][k:]))


def test_adam_clip_without_statistics_leaves_acc_dst(cuda):
    st = AdamState(cuda, 300, [300], [1], seed=5)
    before, after, _ = check_adam_step(st, grads_of(st, 1.0), 1.0, 1e-3, 0.0)
    assert torch.equal(bits(after['acc']), bits(before['acc']))


# =========================================================================================== hrl_clip_grad_norm[_ws]
CLIP_SIZES = [0, 1, 3, 4, 5, 4095, 4096, 4099, 65536, 65537, 65539, 65536 + 4 * 64 * 3 + 3]


def launch_clip(cuda, grads, n, ws):
    lib = _native.load()
    arena = Arena(cuda)
    g = arena.inout(grads, 'grads')
    total = arena.out((), torch.float32, 'total_norm')
    if ws:
        nbytes = lib.hrl_clip_workspace_bytes(n)
        assert nbytes == 512
        work = arena.ws(nbytes, 'workspace')
        rc = lib.hrl_clip_grad_norm_ws(P(g), n, MAX_NORM, P(total), P(work), nbytes, _native.stream_of(cuda))
    else:
        rc = lib.hrl_clip_grad_norm(P(g), n, MAX_NORM, P(total), _native.stream_of(cuda))
    _native.check(rc, 'hrl_clip_grad_norm')
    arena.check()
    if ws:
        # the switch: up to 65536 floats one launch that leaves the workspace alone, above it 64 chunk sums
        written = int((work.view(torch.int32) != SENTINEL32).sum())
        if n <= 65536:
            assert written == 0, 'the one-launch form wrote the workspace'
        else:
            sums = work.view(torch.float64).cpu()
            assert not bool((bits(sums) == SENTINEL64).any()), 'a chunk sum was never written'
            exact = float(grads[:n].double().pow(2).sum())
            assert abs(float(sums.sum()) - exact) <= 1e-12 * exact or not math.isfinite(exact)
    return g.cpu(), total.cpu()


def check_clip(grads, n, got, total):
    g64 = grads[:n].double()
    want, total_ref, coef_ref = clip64(grads[:n], MAX_NORM)
    assert torch.equal(bits(got[n:]), bits(grads[n:])), 'an element past n changed'
    exact = g64.pow(2).sum().sqrt()
    if math.isfinite(float(exact)):
        assert abs(float(total) - float(exact)) <= EPS32 * float(exact)
    else:
        assert torch.equal(bits(total), bits(total_ref)) or (math.isnan(float(total)) and math.isnan(float(total_ref)))
    coef = torch.clamp(torch.tensor(MAX_NORM) / (total + torch.tensor(1e-6)), max=1.0)
    clipped = g64 * coef.double()
    nan = clipped.isnan()
    assert torch.equal(got[:n].isnan(), nan)
    assert bool(((got[:n].double() - clipped).abs()[~nan] <= ulp32(clipped)[~nan]).all())
    if torch.equal(bits(total), bits(total_ref)):
        assert bool(((got[:n].double() - want).abs()[~nan] <= ulp32(want)[~nan]).all())
    if float(coef) == 1.0:
        assert torch.equal(bits(got), bits(grads)), 'coef 1: the gradients keep their bits'
    return coef


@pytest.mark.parametrize('ws', [False, True], ids=['plain', 'ws'])
@pytest.mark.parametrize('n', CLIP_SIZES)
def test_clip_sizes(cuda, n, ws):
    """The float4 body with 0..3 tail elements, one thread's stride (4096 = 4 x 1024), the last one-launch size
    (65536), the first two-launch sizes (the _ws entry; the plain entry stays one launch) and a two-launch size whose
    64 chunks are uneven with a tail, at a scale below max_norm and one above; n = 0 writes a norm of 0 and nothing
    else."""
    gen = torch.Generator().manual_seed(n)
    if n == 0:
        grads = torch.randn(4, generator=gen)
        got, total = launch_clip(cuda, grads, 0, ws)
        assert float(total) == 0.0 and torch.equal(bits(got), bits(grads))
        return
    for scale in (0.5, 300.0):
        grads = torch.randn(n, generator=gen) * (scale / math.sqrt(n))
        got, total = launch_clip(cuda, grads, n, ws)
        coef = check_clip(grads, n, got, total)
        assert (float(coef) == 1.0) == (scale < MAX_NORM) or n < 10


@pytest.mark.parametrize('n', [4099, 65539])
def test_clip_exact_and_nonfinite(cuda, n):
    """Integer gradients (norm 8: equal; each gradient the float product), NaN and inf as clip64, and below the
    switch the same bits from both entries."""
    g = torch.zeros(n)
    g[torch.arange(64) * (n // 64) + 3] = 1.0
    g[n - 1], g[3] = 1.0, 0.0                                       # one of the 64 in the scalar tail
    coef = torch.tensor(4.0) / (torch.tensor(8.0) + torch.tensor(1e-6))
    for ws in (False, True):
        got, total = launch_clip(cuda, g, n, ws)
        assert float(total) == 8.0 and torch.equal(bits(got), bits(g * coef))
    gen = torch.Generator().manual_seed(n)
    for bad in (NAN, float('inf')):
        grads = torch.randn(n, generator=gen)
        grads[n - 2] = bad                                          # in the scalar tail (n % 4 == 3)
        for ws in (False, True):
            got, total = launch_clip(cuda, grads, n, ws)
            check_clip(grads, n, got, total)
            if bad != bad:
                assert bool(got.isnan().all())
            else:
                assert float(total) == float('inf') and int(got.isnan().sum()) == 1 and float(got.abs().nan_to_num().max()) == 0
    grads = torch.randn(n, generator=gen) * 3
    a, ta = launch_clip(cuda, grads, n, False)
    b, tb = launch_clip(cuda, grads, n, True)
    if n <= 65536:
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(ta), bits(tb))
    else:                                                           # two launches: another fixed order, the same norm
        assert abs(float(ta) - float(tb)) <= 2 * EPS32 * float(ta)
