"""The one-launch bf16 DRC repeat on the GPU (csrc/hrl_drc_bf16.hip): at the C entry between guard bands, through
nn.drc_step(precision='bf16_drc') with its gradients, and in the whole learner step.

Reference: the ConvLSTM cell in fp64 on the CPU (``cell64``; ``rnd``: h and W_h through bf16 as the contract rounds,
straight-through for autograd).  Rules: on bf16-valued operands at most 4x the two-launch fp32 path's error + 1e-6
(DESIGN 4.9); over R repeats at most 2x the emulation's error + 1e-6 (4.29); gradients within (R + 1) * 2^-8 relative
L2 of fp64 autograd through the emulation (4.28: one term per rounding on the path, plus two)."""

import pytest
import torch
import torch.nn.functional as F

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from tests.guarded import Arena, bits

pytestmark = pytest.mark.gpu

CASES = [(1, 1), (3, 3), (4, 2)]
SL, PAD = (32, 64), (1, 1)


def bf(t):
    return t.float().bfloat16().double()


def cell64(zx, h, c, w_h, rnd):
    if rnd:
        h, w_h = h + (bf(h) - h).detach(), w_h + (bf(w_h) - w_h).detach()
    i, f, o, g = (zx + F.conv2d(h, w_h, padding=1)).chunk(4, 1)
    i, f, o, g = i.sigmoid(), f.sigmoid(), o.sigmoid(), g.tanh()
    c2 = f * c + i * g
    return o * c2.tanh(), c2, torch.cat([i, f, o, g], 1)


def unroll64(ws, zx, hs, cs, R, rnd):
    for _ in range(R):
        outs = [cell64(z, h, c, w[:, 32:], rnd) for z, h, c, w in zip(zx, hs, cs, ws)]
        hs, cs = [o[0] for o in outs], [o[1] for o in outs]
    return hs, cs


def operands(L, N, seed, pre_round, device):
    """Cell weights, zx as channel slices of a wider tensor, h with a non-contiguous row stride, c contiguous."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    q = (lambda t: t.bfloat16().float()) if pre_round else (lambda t: t)
    ws = [q(rnd(128, 64, 3, 3) * 0.08).to(device) for _ in range(L)]
    zwide, hwide = rnd(N, L * 128 + 4, 6, 6).to(device), q(torch.tanh(rnd(L, N, 40, 6, 6))).to(device)
    zx = [zwide[:, 128 * l:128 * (l + 1)] for l in range(L)]
    return ws, zx, [hwide[l, :, :32] for l in range(L)], [rnd(N, 32, 6, 6).to(device) for _ in range(L)]


to64 = lambda ts: [t.detach().cpu().double() for t in ts]
err = lambda a, r: float((a.detach().cpu().double() - r).abs().max())


def repeat(pack, zx, hs, cs, live):
    """hrl_drc_bf16_repeat_forward with every output between sentinels."""
    N, L, dev = hs[0].shape[0], len(hs), hs[0].device
    arena, A, I = Arena(dev), _native.ptr_array, _native.i64_array
    h_out, c_out = ([arena.out((N, 32, 6, 6)) for _ in range(L)] for _ in range(2))
    gates = [arena.out((N, 128, 6, 6)) if lv else None for lv in live]
    code = _native.load().hrl_drc_bf16_repeat_forward(
        _native.ptr(pack), pack.numel(), L, 32, A(zx), I([z.stride(0) for z in zx]), A(hs),
        I([h.stride(0) for h in hs]), A(cs), I([c.stride(0) for c in cs]), N, A(h_out), A(c_out), A(gates),
        _native.stream_of(dev))
    assert code == _native.HRL_OK, code
    arena.check()
    return h_out + c_out + [g for g in gates if g is not None]


@pytest.mark.parametrize('L,R', CASES)
def test_one_repeat_at_the_entry(cuda, L, R):
    """N = 1, 15, 16, 17 bit-identical to the same rows of N = 33 (two tiles and a row); N = 33 within the 4x rule."""
    ws, zx, hs, cs = operands(L, 33, L, True, cuda)
    live = [L == 1 or l > 0 for l in range(L)]
    pack = hnn.drc_bf16_pack(ws, 32)
    big = repeat(pack, zx, hs, cs, live)
    for N in (1, 15, 16, 17):
        got = repeat(pack, [t[:N] for t in zx], [t[:N] for t in hs], [t[:N] for t in cs], live)
        assert all(torch.equal(bits(a), bits(b[:N])) for a, b in zip(got, big)), N
    ref = [cell64(z, h, c, w[:, 32:], True) for z, h, c, w in zip(to64(zx), to64(hs), to64(cs), to64(ws))]
    old = []
    for z, h, c, w in zip(zx, hs, cs, ws):   # today's two launches per layer: exact-split conv, then the gates
        zh = hnn.gboard_conv(h, hnn.gboard_pack(w, 32, 32), 128, 32)
        o = [torch.empty_like(c), torch.empty_like(c), torch.empty_like(zh)]
        _native.check(_native.load().hrl_lstm_gates_forward(
            _native.ptr(z), z.stride(0), _native.ptr(zh), _native.ptr(c), 33, 32, 36, None, 1, *map(_native.ptr, o),
            _native.stream_of(cuda)), 'hrl_lstm_gates_forward')
        old.append(o)
    ref = [r[k] for k in (0, 1) for r in ref] + [r[2] for r, lv in zip(ref, live) if lv]
    old = [o[k] for k in (0, 1) for o in old] + [o[2] for o, lv in zip(old, live) if lv]
    for k, (a, o, r) in enumerate(zip(big, old, ref)):
        e_new, e_old = err(a, r), err(o, r)
        print('L %d output %d: one launch %.3g, two launches %.3g' % (L, k, e_new, e_old))
        assert e_new <= 4 * e_old + 1e-6, (k, e_new, e_old)


@pytest.mark.parametrize('L,R', CASES)
def test_drc_step_forward_and_gradients(cuda, L, R):
    """N = 17 through nn.drc_step: the state against the exact fp64 cell, the last layer's gradients of sum(h'u) +
    sum(c'v) against the emulation's; at (1, 1), bf16-valued operands, against the fp32 step's (4x + 1e-6)."""
    pre = (L, R) == (1, 1)
    ws, zx, hs, cs = operands(L, 17, 10 + L, pre, cuda)
    zx[-1], hs[-1] = zx[-1].contiguous(), hs[-1].contiguous()
    u, v = torch.randn(2, 17, 32, 6, 6, generator=torch.Generator().manual_seed(3)).to(cuda)
    leaves = [zx[-1], hs[-1], cs[-1], ws[-1]]

    def grads(precision):
        for t in leaves:
            t.requires_grad_(True).grad = None
        with hnn.deferred_weight_grads() as d:
            pk = None if precision == 'bf16_drc' else hnn.gboard_pack(torch.cat([w.detach()[:, 32:] for w in ws]))
            h2, c2 = hnn.drc_step(zx, hs, cs, ws, SL, PAD, pk, R, precision=precision)
            ((h2[-1] * u).sum() + (c2[-1] * v).sum()).backward()
            d.flush()
        return h2 + c2, [t.grad[:, 32:] if t is ws[-1] else t.grad for t in leaves]

    out, g_new = grads('bf16_drc')
    l64 = [t.requires_grad_(True) for t in to64(leaves)]
    a64 = [to64(ws[:-1]) + [l64[3]], to64(zx[:-1]) + [l64[0]], to64(hs[:-1]) + [l64[1]], to64(cs[:-1]) + [l64[2]]]
    with torch.no_grad():
        exact = unroll64(*a64, R, False)
    eh, ec = unroll64(*a64, R, True)
    (eh[-1] * u.cpu().double()).sum().add((ec[-1] * v.cpu().double()).sum()).backward()
    g64 = [l64[k].grad[:, 32:] if k == 3 else l64[k].grad for k in range(4)]
    for k, (a, e, r) in enumerate(zip(out, eh + ec, exact[0] + exact[1])):
        e_new, e_emu = err(a, r), err(e, r)
        print('L %d R %d state %d: kernel %.3g, emulation %.3g' % (L, R, k, e_new, e_emu))
        assert pre or (e_emu > 0 and e_new <= 2 * e_emu + 1e-6), (k, e_new, e_emu)   # pre: the entry test's rule
    g_old = grads('fp32')[1] if pre else None
    for k, (a, r) in enumerate(zip(g_new, g64)):
        rel = float((a.cpu().double() - r).norm() / r.norm())
        print('L %d R %d gradient %d (zx, h, c, W_h): relative L2 %.3g' % (L, R, k, rel))
        if pre:
            assert err(a, r) <= 4 * err(g_old[k], r) + 1e-6, k
        else:
            assert rel <= (R + 1) * 2.0 ** -8, (k, rel)


def _learner(cuda, graph, precision):
    """Three LearnerStep updates of a seeded GeisterNet (B = 8, T = 4): their losses, and a fourth step's kernels."""
    from torch.profiler import ProfilerActivity, profile
    from handyrl_amd.envs.geister import GeisterNet
    from handyrl_amd.synthetic import default_args, geister_batch
    from handyrl_amd.trainer import LearnerStep
    B, T = 8, 4
    torch.manual_seed(0)
    net = GeisterNet().to(cuda)
    batch = geister_batch(B, T, cuda, seed=5)
    hidden = tuple([t.to(cuda) for t in ts] for ts in net.init_hidden([B, 2]))
    args = default_args(T, B) if precision is None else dict(default_args(T, B), precision=precision)
    step = LearnerStep(net, args, cuda, graph=graph)
    losses = [{k: v.detach().clone() for k, v in step.step(batch, hidden).items()} for _ in range(3)]
    torch.cuda.synchronize(cuda)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step.step(batch, hidden)
        torch.cuda.synchronize(cuda)
    return losses, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_learner_step_eager_and_graph(cuda, monkeypatch):
    (absent, _), (fp32, names32) = _learner(cuda, True, None), _learner(cuda, True, 'fp32')
    assert not any('drc_bf16' in n for n in names32)

    def refused(*args):
        raise AssertionError("the fp32 pair was called under precision 'bf16_drc'")
    # a replay holds what its capture launched: with the pair's entries refusing, none of either can be in it (the
    # trace is read as well, but it can lose a replay's events, so it cannot show more than an absence)
    for entry in ('hrl_gboard_forward_groups', 'hrl_lstm_gates_forward_grouped'):
        monkeypatch.setattr(_native.load(), entry, refused)
    (eager, _), (graph, names) = _learner(cuda, False, 'bf16_drc'), _learner(cuda, True, 'bf16_drc')
    assert not any('lstm_fwd_grouped' in n for n in names)
    for a, b, c, d in zip(eager, graph, absent, fp32):
        assert set(a) == set(b) == set(c) and all(bool(torch.isfinite(x).all()) for x in a.values())
        assert all(torch.equal(bits(a[k]), bits(b[k])) and torch.equal(bits(c[k]), bits(d[k])) for k in a)
