"""The one-launch bf16 backward of the DRC time step on the GPU (csrc/hrl_drc_bf16_bwd.hip) against fp64 on the CPU.
Rules: every output's relative L2 error against the exact gradient is at most 2x the fp64 emulation's own (dz and W_h
through bf16 in the adjoint) + 1e-6 (DESIGN 4.31's rule); at R = 1 the outputs that see no bf16 are within 4x
hrl_lstm_gates_backward_ex's max error + 1e-6; drc_step's gradients are within (2R + 1) * 2^-8 relative L2 of fp64
autograd through the forward emulation (one bf16 unit per rounded operand on the longest path: R of h, R of dz, W)."""

import pytest
import torch
import torch.nn.functional as F

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.geister import GeisterNet
from handyrl_amd.synthetic import default_args, geister_batch
from handyrl_amd.trainer import LearnerStep
from tests.guarded import Arena, bits

pytestmark = pytest.mark.gpu

CASES = [(1, 1), (3, 3), (4, 2)]
G = 4            # the kernel's game tile
SL, PAD = (32, 64), (1, 1)


def bf(t):
    return t.float().bfloat16().double()


def step64(w_h, gates, c, c_out, gh, gc, rnd, want_dh):
    """One layer's R repeats in fp64: ([dz_r], dzx, dh_in, dc_in); rnd: dz and W_h through bf16 in the adjoint."""
    R = len(gates)
    dh = torch.zeros_like(c[0]) if gh is None else gh
    dc = torch.zeros_like(c[0]) if gc is None else gc
    dzs, dzx = [None] * R, 0
    for r in range(R - 1, -1, -1):
        i, f, o, g = gates[r].chunk(4, 1)
        tc = c_out[r].tanh()
        dct = dc + dh * o * (1 - tc * tc)
        dz = torch.cat([dct * g * (i * (1 - i)), dct * c[r] * (f * (1 - f)), dh * tc * (o * (1 - o)),
                        dct * i * (1 - g * g)], 1)
        dc = dct * f
        dzs[r], dzx = dz, dzx + dz
        if r > 0 or want_dh:
            dh = F.conv_transpose2d(bf(dz) if rnd else dz, bf(w_h) if rnd else w_h, padding=1)
    return dzs + [dzx, dh if want_dh else None, dc]


def entry(pack, ins, N, variant):
    """The entry on the first N rows, outputs between sentinels: per layer [dz_0 .. dz_{R-1}, dzx, dh_in, dc_in]."""
    gates, c, c_out, gh, gc = ins
    L, R, dev = len(gates), len(gates[0]), gates[0][0].device
    arena, A, I = Arena(dev), _native.ptr_array, _native.i64_array
    flat = lambda tss: [t[:N] for ts in tss for t in ts]
    dz = [arena.out((N, 128, 6, 6)) for _ in range(L * R)]
    dzx, dc_in = ([arena.out((N, ch, 6, 6)) for _ in range(L)] for ch in (128, 32))
    dh_in = [None if variant == 'no_dh_in' else arena.out((N, 32, 6, 6)) for _ in range(L)]
    gh = [None if variant == 'no_gh' else t[:N] for t in gh]
    gc = [None if variant == 'no_gc' else t[:N] for t in gc]
    strides = lambda ts: I([0 if t is None else t.stride(0) for t in ts])
    code = _native.load().hrl_drc_bf16_step_backward(
        _native.ptr(pack), pack.numel(), I(list(range(L))), L, R, 32, A(flat(gates)), A(flat(c)), A(flat(c_out)), A(gh),
        strides(gh), A(gc), strides(gc), N, A(dz), A(dzx), A(dh_in), A(dc_in), _native.stream_of(dev))
    assert code == _native.HRL_OK, code
    arena.check()
    return [dz[l * R:(l + 1) * R] + [dzx[l], dh_in[l], dc_in[l]] for l in range(L)]


@pytest.mark.parametrize('variant', ['all', 'no_gh', 'no_gc', 'no_dh_in'])
@pytest.mark.parametrize('L,R', CASES)
def test_step_backward_at_the_entry(cuda, L, R, variant):
    N = 2 * G + 1
    gen = torch.Generator().manual_seed(100 * L + R)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    ws = [(rnd(128, 64, 3, 3) * 0.08).to(cuda) for _ in range(L)]
    gates = [[torch.cat([torch.sigmoid(rnd(N, 96, 6, 6)), torch.tanh(rnd(N, 32, 6, 6))], 1).to(cuda)
              for _ in range(R)] for _ in range(L)]
    c, c_out = ([[rnd(N, 32, 6, 6).to(cuda) for _ in range(R)] for _ in range(L)] for _ in range(2))
    gh = [rnd(N, 40, 6, 6).to(cuda)[:, :32] for _ in range(L)]     # a row stride above the row
    gc = [rnd(N, 32, 6, 6).to(cuda) for _ in range(L)]
    ins = (gates, c, c_out, gh, gc)
    pack = hnn.drc_bf16_adjoint_pack(ws, 32)
    big = entry(pack, ins, N, variant)
    for n in (1, G - 1, G, G + 1):   # a row depends on nothing but the row
        for a, b in zip(entry(pack, ins, n, variant), big):
            assert all(x is None or torch.equal(bits(x), bits(y[:n])) for x, y in zip(a, b)), n
    if variant == 'no_dh_in':        # the r = 0 adjoint is skipped; nothing else moves
        for a, b in zip(big, entry(pack, ins, N, 'all')):
            assert all(torch.equal(bits(x), bits(y)) for k, (x, y) in enumerate(zip(a, b)) if k != R + 1)
    d = lambda t: None if t is None else t.detach().cpu().double()
    rel = lambda a, r: float((d(a) - r).norm() / r.norm())
    for l in range(L):
        a64 = (d(ws[l][:, 32:]), [d(t) for t in gates[l]], [d(t) for t in c[l]], [d(t) for t in c_out[l]],
               None if variant == 'no_gh' else d(gh[l]), None if variant == 'no_gc' else d(gc[l]))
        exact, emu = (step64(*a64, r, variant != 'no_dh_in') for r in (False, True))
        for k, (a, e, x) in enumerate(zip(big[l], emu, exact)):
            if x is None:
                continue
            e_new, e_emu = rel(a, x), rel(e, x)
            print('L %d R %d %s layer %d output %d: kernel %.3g, emulation %.3g' % (L, R, variant, l, k, e_new, e_emu))
            assert e_new <= 2 * e_emu + 1e-6, (l, k, e_new, e_emu)
        if R == 1:   # dz_0, dzx and dc_in see no bf16: beside the gate kernel the launch replaces
            old = [torch.empty(N, ch, 6, 6, device=cuda) for ch in (128, 128, 32)]   # dz, dzx, dc
            P = _native.ptr
            _native.check(_native.load().hrl_lstm_gates_backward_ex(
                P(gates[l][0]), P(c[l][0]), P(c_out[l][0]), None if variant == 'no_gh' else P(gh[l]), gh[l].stride(0), 1,
                32 * 36, None if variant == 'no_gc' else P(gc[l]), N, 32, 36, P(old[0]), P(old[2]), P(old[1]), 1,
                _native.stream_of(cuda)), 'hrl_lstm_gates_backward_ex')
            for k, o in zip((0, 1, 3), old):
                e_new, e_old = (float((d(t) - exact[k]).abs().max()) for t in (big[l][k], o))
                print('L 1 R 1 %s output %d: one launch %.3g, gate kernel %.3g' % (variant, k, e_new, e_old))
                assert e_new <= 4 * e_old + 1e-6, (k, e_new, e_old)


def cell64(zx, h, c, w_h):
    """The forward emulation: h and W_h through bf16, straight-through for autograd."""
    h, w_h = h + (bf(h) - h).detach(), w_h + (bf(w_h) - w_h).detach()
    i, f, o, g = (zx + F.conv2d(h, w_h, padding=1)).chunk(4, 1)
    c2 = f.sigmoid() * c + i.sigmoid() * g.tanh()
    return o.sigmoid() * c2.tanh(), c2


@pytest.mark.parametrize('L,R', CASES)
def test_drc_step_gradients(cuda, L, R):
    N = 2 * G + 1
    gen = torch.Generator().manual_seed(10 + L)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    ws = [(rnd(128, 64, 3, 3) * 0.08).to(cuda) for _ in range(L)]
    zx, hs, cs = ([t.to(cuda) for t in ts] for ts in ([rnd(N, 128, 6, 6) for _ in range(L)],
                                                       [torch.tanh(rnd(N, 32, 6, 6)) for _ in range(L)],
                                                       [rnd(N, 32, 6, 6) for _ in range(L)]))
    u, v = rnd(2, N, 32, 6, 6).to(cuda)
    leaves = [zx[-1], hs[-1], cs[-1], ws[-1]]
    for t in leaves:
        t.requires_grad_(True)
    with hnn.deferred_weight_grads() as dfr:
        h2, c2 = hnn.drc_step(zx, hs, cs, ws, SL, PAD, None, R, precision='bf16_drc_bwd')
        ((h2[-1] * u).sum() + (c2[-1] * v).sum()).backward()
        dfr.flush()
    l64 = [t.detach().cpu().double().requires_grad_(True) for t in leaves]
    h, c = l64[1], l64[2]
    for _ in range(R):
        h, c = cell64(l64[0], h, c, l64[3][:, 32:])
    ((h * u.cpu().double()).sum() + (c * v.cpu().double()).sum()).backward()
    for k, (a, r) in enumerate(zip(leaves, l64)):
        got, ref = (t.grad[:, 32:] if k == 3 else t.grad for t in (a, r))
        e = float((got.cpu().double() - ref).norm() / ref.norm())
        print('L %d R %d gradient %d (zx, h, c, W_h): relative L2 %.3g' % (L, R, k, e))
        assert e <= (2 * R + 1) * 2.0 ** -8, (k, e)


def _losses(cuda, graph):
    """Three LearnerStep updates of a seeded GeisterNet (B = 8, T = 4) under precision bf16_drc_bwd."""
    B, T = 8, 4
    torch.manual_seed(0)
    net = GeisterNet().to(cuda)
    batch = geister_batch(B, T, cuda, seed=5)
    hidden = tuple([t.to(cuda) for t in ts] for ts in net.init_hidden([B, 2]))
    step = LearnerStep(net, dict(default_args(T, B), precision='bf16_drc_bwd'), cuda, graph=graph)
    losses = [{k: v.detach().clone() for k, v in step.step(batch, hidden).items()} for _ in range(3)]
    return losses


def test_learner_step_eager_and_graph(cuda, monkeypatch):
    def refused(*args):   # a replay holds what its capture launched: the replaced entry cannot be in the graph
        raise AssertionError("the per-repeat gate backward was called under precision 'bf16_drc_bwd'")
    monkeypatch.setattr(_native.load(), 'hrl_lstm_gates_backward_ex', refused)
    for a, b in zip(_losses(cuda, False), _losses(cuda, True)):
        assert set(a) == set(b) and all(bool(torch.isfinite(x).all()) for x in a.values())
        assert all(torch.equal(bits(a[k]), bits(b[k])) for k in a)
