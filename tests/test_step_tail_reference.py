"""The step tail's plain references (tests/step_tail_reference.py) against torch and against Python loops (no GPU)."""

import math

import pytest
import torch
import torch.nn as nn

from tests.step_tail_reference import (adam64, adam_emulated, block_sums64, clip64, fold64, fold_terms64,
                                       lane_elements)

SHAPES = [(5, 3), (7,), (1,), (4, 2, 3)]


def ulp32(x):
    """The spacing of fp32 at |x| (fp64 tensor): 2^(floor(log2|x|) - 23), the smallest normal's below it."""
    e = torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23)


@pytest.mark.parametrize('wd', [0.0, 1e-5])
def test_clip_then_adam_is_torch_on_fp64(wd):
    """clip64 (in the parameters' own type, fp64) then adam64 = clip_grad_norm_ + torch.optim.Adam(foreach=False) on
    fp64 parameters: 5 steps, a changing lr, gradients below and above the threshold, to 1e-12 relative."""
    gen = torch.Generator().manual_seed(11)
    ps = [nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in SHAPES]
    opt = torch.optim.Adam(ps, lr=1e-3, weight_decay=wd, foreach=False)
    p = torch.cat([q.detach().reshape(-1) for q in ps]).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    lrs = [1e-3, 3e-3, 5e-4, 5e-4, 2e-2]
    for k, (lr, scale) in enumerate(zip(lrs, [0.1, 30.0, 1.0, 1e-3, 7.0])):
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * scale for s in SHAPES]
        for q, g in zip(ps, grads):
            q.grad = g.clone()
        for group in opt.param_groups:
            group['lr'] = lr
        total_t = nn.utils.clip_grad_norm_(ps, 4.0)
        opt.step()
        g, total, coef = clip64(torch.cat([x.reshape(-1) for x in grads]), 4.0, dtype=torch.float64)
        assert (float(coef) == 1.0) == (scale < 1.0)
        assert abs(float(total) - float(total_t)) <= 1e-12 * float(total_t)
        torch.testing.assert_close(g, torch.cat([q.grad.reshape(-1) for q in ps]), rtol=1e-12, atol=0)
        p, m, v = adam64(p, g, m, v, k + 1, lr, wd=wd)
        torch.testing.assert_close(p, torch.cat([q.detach().reshape(-1) for q in ps]), rtol=1e-12, atol=0)
        st = [opt.state[q] for q in ps]
        torch.testing.assert_close(m, torch.cat([s['exp_avg'].reshape(-1) for s in st]), rtol=1e-12, atol=1e-300)
        torch.testing.assert_close(v, torch.cat([s['exp_avg_sq'].reshape(-1) for s in st]), rtol=1e-12, atol=0)


@pytest.mark.parametrize('scale', [1e-3, 100.0])
def test_clip64_in_fp32_is_torch_on_fp32(scale):
    """The rule in the kernels' type: the norm within one fp32 rounding of torch's, the gradients within one ulp."""
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(1001, generator=gen) * scale
    q = nn.Parameter(torch.zeros(1001))
    q.grad = g.clone()
    total_t = float(nn.utils.clip_grad_norm_([q], 4.0))
    got, total, coef = clip64(g, 4.0)
    assert total.dtype == torch.float32 and coef.dtype == torch.float32
    assert abs(float(total) - total_t) <= 2.0 ** -23 * total_t
    assert (float(coef) == 1.0) == (scale < 1.0)
    assert bool(((got - q.grad.double()).abs() <= 2 * ulp32(got)).all())    # torch's coef may differ by an ulp too


def test_fold64_equals_python_loops():
    """Mode 0 and mode 1 on a tiny case against explicit loops over rows, taps and channels."""
    gen = torch.Generator().manual_seed(5)
    n = 9216 + 70
    flat = torch.randint(-3, 4, (n,), generator=gen).float()
    p1 = torch.randint(-2, 3, (3, 9300), generator=gen).float()          # stride 9300, col0 50
    p0 = torch.randint(-2, 3, (4, 40), generator=gen).float()            # stride 40, col0 7, 21 columns
    folds = [(p1, 9300, 50, 3, 33, 9216, 1), (p0, 40, 7, 4, 9216 + 40, 21, 0)]
    want = flat.double().clone()
    for r in range(3):
        for tap in range(9):
            for ci in range(32):
                for co in range(0, 32, 5):          # every fifth output channel by loop, the rest by the check below
                    want[33 + co * 288 + ci * 9 + tap] += float(p1[r, 50 + tap * 1024 + ci * 32 + co])
    for r in range(4):
        for j in range(21):
            want[9216 + 40 + j] += float(p0[r, 7 + j])
    got, blocks = fold64(flat, folds)
    conv = got[33:33 + 9216].view(32, 32, 9)
    assert torch.equal(conv[0::5], want[33:33 + 9216].view(32, 32, 9)[0::5])
    assert torch.equal(got[9216 + 33:], want[9216 + 33:]) and torch.equal(got[:33], want[:33])
    # a conv weight as conv2d sees it: weight[co, ci, ky, kx] is the sum of row element [ky * 3 + kx][ci][co]
    w = p1[:, 50:50 + 9216].double().sum(0).view(3, 3, 32, 32)
    for co, ci, ky, kx in ((0, 0, 0, 0), (31, 7, 2, 1), (4, 31, 1, 2), (17, 3, 0, 2)):
        assert float(conv[co, ci, ky * 3 + kx]) == float(flat[33 + co * 288 + ci * 9 + ky * 3 + kx]) + float(w[ky, kx, ci, co])
    s, a = fold_terms64(folds[1])
    assert torch.equal(s, p0[:, 7:28].double().sum(0)) and torch.equal(a, p0[:, 7:28].double().abs().sum(0))
    # the block sums: each element once (the total is the squared norm); outside the mode-1 fold by position
    assert float(blocks.sum()) == float((got * got).sum())
    holds = lane_elements(n, folds)
    assert torch.equal(torch.sort(holds).values, torch.arange(n))
    assert torch.equal(holds[:33], torch.arange(33)) and torch.equal(holds[33 + 9216:], torch.arange(33 + 9216, n))
    last = (n - 1) // 64
    assert float(blocks[last]) == float((got[last * 64:] ** 2).sum())
    for b in (0, 1, 77):                            # by loop: position i of the fold squares source column i - 33
        t = 0.0
        for i in range(b * 64, b * 64 + 64):
            if 33 <= i < 33 + 9216:
                j = i - 33
                tap, ci, co = j // 1024, (j // 32) % 32, j % 32
                t += float(got[33 + co * 288 + ci * 9 + tap]) ** 2
            else:
                t += float(got[i]) ** 2
        assert float(blocks[b]) == t
    assert torch.equal(block_sums64(got.float(), n, []), torch.cat([got, torch.zeros(-n % 64).double()])
                       .view(-1, 64).pow(2).sum(1))


@pytest.mark.parametrize('wd', [0.0, 1e-5])
def test_adam_emulated_is_within_an_ulp_of_torch_fp32(wd):
    """adam_emulated (moments formed in double, rounded once) against torch's CPU fp32 Adam (every operation rounded
    to float), 5 steps from the same state each step: parameters within one fp32 ulp.  The parameters are kept away
    from zero (0.5 <= |p| < 1.5) and lr <= 1e-2: the update is then at most lr / ((1 - beta1) sqrt(1 - beta2))...
    in practice a few lr, its own rounding error (a few 2^-24 of it) far below the parameter's ulp, so the two
    results are roundings of nearly one value.  (Next to zero the parameter's ulp is smaller than the update's
    rounding error and no such bound holds for torch's own float chain.)  The moments, each rounding at most 2^-24
    relative: torch's exp_avg is a float lerp (the weight's cast, the difference, the product, the sum: 4 roundings
    of values no larger than 2 max(|m|, |g|)) and its exp_avg_sq a float mul and addcmul (beta2's and 1 - beta2's
    casts, v beta2, g g, its scaling, the sum: 6 roundings of values no larger than the result, whose terms are all
    positive); the emulation adds one rounding of the result to each."""
    gen = torch.Generator().manual_seed(7)
    sign = torch.randint(0, 2, (4096,), generator=gen).float() * 2 - 1
    q = nn.Parameter(sign * (0.5 + torch.rand(4096, generator=gen)))
    opt = torch.optim.Adam([q], lr=1e-3, weight_decay=wd, foreach=False, fused=False)
    for k, lr in enumerate([1e-3, 1e-3, 3e-4, 1e-2, 1e-2]):
        g = torch.randn(4096, generator=gen) * (10.0 ** (k - 2))
        p0 = q.detach().clone()
        st = opt.state[q]
        m0 = st['exp_avg'].clone() if st else torch.zeros_like(p0)
        v0 = st['exp_avg_sq'].clone() if st else torch.zeros_like(p0)
        q.grad = g.clone()
        for group in opt.param_groups:
            group['lr'] = lr
        opt.step()
        p, m, v = adam_emulated(p0, g, m0, v0, k + 1, lr, wd=wd)
        assert p.dtype == m.dtype == v.dtype == torch.float32
        pt, mt, vt = q.detach().double(), opt.state[q]['exp_avg'].double(), opt.state[q]['exp_avg_sq'].double()
        assert bool(((p.double() - pt).abs() <= ulp32(torch.maximum(p.double().abs(), pt.abs()))).all()), k
        gd = g.double() + wd * p0.double()
        # torch forms the decayed gradient in float: two roundings, of wd p and of the sum, which may cancel
        dg = 2 * 2.0 ** -24 * torch.maximum(g.double().abs(), wd * p0.double().abs()) if wd else torch.zeros(())
        assert bool(((m.double() - mt).abs() <= 5 * 2.0 ** -24 * 2 * torch.maximum(m0.double().abs(), gd.abs()) + 0.1 * dg).all()), k
        assert bool(((v.double() - vt).abs() <= 7 * 2.0 ** -24 * vt + 1e-3 * (2 * gd.abs() * dg + dg * dg)).all()), k
        # and against fp64: the emulation is a rounding of adam64, not another rule
        p64, m64, v64 = adam64(p0, g, m0, v0, k + 1, float(torch.tensor(lr).float()), wd=wd)
        assert bool(((m.double() - m64).abs() <= ulp32(m64) + 0.1 * dg).all())
        assert bool(((v.double() - v64).abs() <= ulp32(v64) + 1e-3 * (2 * gd.abs() * dg + dg * dg)).all())
        assert float((p.double() - p64).abs().max()) <= 2.0 ** -22 * float(p64.abs().max())


def test_nonfinite_rules():
    """A NaN norm makes every gradient NaN; an inf norm gives coef = 0 (finite gradients 0, the inf element NaN)."""
    g = torch.tensor([1.0, -2.0, 0.0, 3.0])
    bad = g.clone()
    bad[1] = float('nan')
    got, total, coef = clip64(bad, 4.0)
    assert math.isnan(float(total)) and math.isnan(float(coef)) and bool(got.isnan().all())
    for inf in (float('inf'), float('-inf')):
        bad = g.clone()
        bad[3] = inf
        got, total, coef = clip64(bad, 4.0)
        assert float(total) == float('inf') and float(coef) == 0.0
        assert torch.equal(got[:3], torch.zeros(3, dtype=torch.float64)) and math.isnan(float(got[3]))
    # a finite fp32 buffer whose squares overflow fp32 but not fp64: the fp64 norm is finite
    big = torch.full((4,), 3e30)
    got, total, coef = clip64(big, 4.0)
    assert math.isfinite(float(total)) and 0.0 < float(coef) < 1e-29
    # the same as torch
    q = nn.Parameter(torch.zeros(4))
    q.grad = torch.tensor([1.0, float('inf'), 2.0, float('nan')])
    nn.utils.clip_grad_norm_([q], 4.0)
    assert bool(q.grad.isnan().all()) and bool(clip64(torch.tensor([1.0, float('inf'), 2.0, float('nan')]), 4.0)[0]
                                                .isnan().all())
