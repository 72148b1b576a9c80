"""The mixed-precision GeeseNet tower on the GPU (csrc/hrl_torus_bf16.hip; contract: include/hrl_nn.h), each launch
at its C entry with guard-band outputs (tests/guarded.py) against fp64 torch ops on the same values, then the tower
through nn.torus_tower(precision='bf16') and a captured learner step with train_args precision: bf16.

Integer data (every accumulator and stored value an integer below 256, alpha = 1, beta an integer) must be EQUAL to
the reference.  Random bf16-representable data: a stored bf16 value within one bf16 ulp of bf(reference); an fp32 /
fp64 sum within n 2^-24 sum|terms|, n the number of accumulated terms (forward / adjoint statistics: n = N H W per
channel; dW: n = N H W per element; db: the same).  A conv workgroup walks 8 samples and 512 of them a pass (stride
4096); a weight-gradient workgroup 4 samples, 256 of them a pass (stride 1024).

ONE_SIGN: the random operands of a sum that is stored in bf16 are of one sign.  A sum that cancels to near zero carries
an fp32 accumulation error of many ulps of the result in any summation order, so the one-ulp clause can only hold
where nothing cancels; signs are the integer cases' business, where the clause is equality.

The tower's gradients are compared as relative L2 errors, bound (L + 2) 2^-8; a conv bias gradient is zero in exact
arithmetic (the BatchNorm that follows removes it): db = sum DY is what the roundings of its terms leave, at most
2^-9 sum |dy| per stored rounding, so its error is taken relative to the sums of its absolute terms, sum |dy|.  Measured errors: DESIGN 4.28."""

import copy

import pytest
import torch
import torch.nn.functional as F

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.hungry_geese import GeeseNet
from tests.guarded import Arena, bits

pytestmark = pytest.mark.gpu
P = _native.ptr
SHAPES = [(7, 11, 1), (7, 11, 7), (7, 11, 9), (4, 5, 9), (1, 3, 9), (8, 10, 9)]
CONV_CASES = [c + (True,) for c in SHAPES + [(7, 11, 4095), (7, 11, 4097)]] + [(7, 11, 9, False)]
WGRAD_CASES = [c + (True,) for c in SHAPES + [(7, 11, 1023), (7, 11, 1025)]] + [(7, 11, 9, False)]


def to_cl(t):
    """(N, 32, H, W) -> the stored form (N, H W, 32) bf16."""
    return t.flatten(2).transpose(1, 2).contiguous().bfloat16()


def from_cl(t, H, W):
    return t.double().transpose(1, 2).reshape(t.shape[0], 32, H, W)


def conv64(x, w):
    return F.conv2d(F.pad(x.double(), (1, 1, 1, 1), mode='circular'), w.double())


def bf_out(arena, N, HW, name):
    return arena.out((N * HW * 16,), torch.int32, name=name).view(torch.bfloat16).view(N, HW, 32)


class Data:
    """Seeded operands on the CPU: integers (exact in bf16) or random bf16-representable values."""

    def __init__(self, seed, integer):
        self.g, self.integer = torch.Generator().manual_seed(seed), integer

    def __call__(self, shape, lo, hi, density=1.0):
        if self.integer:
            v = torch.randint(lo, hi + 1, shape, generator=self.g).float()
        else:
            v = (lo + (hi - lo) * torch.rand(shape, generator=self.g)).bfloat16().float()
        return v if density == 1.0 else v * (torch.rand(shape, generator=self.g) < density)


def packed(lib, cuda, weights, stem_cin=17):
    ws = [w.to(cuda).contiguous() for w in weights]
    pack = torch.empty(lib.hrl_torus_bf16_pack_bytes(len(ws)), dtype=torch.uint8, device=cuda)
    assert lib.hrl_torus_bf16_pack(_native.ptr_array(ws), len(ws), stem_cin, P(pack), pack.numel(),
                                   _native.stream_of(cuda)) == 0
    return pack


def close(got, ref, integer, terms=None, n=0):
    """Stored bf16 (terms None): equal / within one ulp of bf(ref).  Sums: equal / within n 2^-24 sum|terms|."""
    got = got.cpu().double()
    if integer:
        assert torch.equal(got, ref), float((got - ref).abs().max())
    elif terms is None:
        want = ref.float().bfloat16().double()
        ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want)[1] - 8)
        assert bool(((got - want).abs() <= ulp).all()), float(((got - want).abs() / ulp).max())
    else:
        assert bool(((got - ref).abs() <= n * 2.0 ** -24 * terms).all()), float(((got - ref).abs() / terms).max())


@pytest.mark.parametrize('H,W,N,integer', CONV_CASES)
@pytest.mark.parametrize('mode', ['stem', 'first', 'residual'])
def test_forward_launch(cuda, mode, H, W, N, integer):
    lib, d, HW = _native.load(), Data(H * W + N, integer), H * W
    cin = 17 if mode == 'stem' else 32
    w, b = (d((32, cin, 3, 3), -1, 1, 0.04), d((32,), -2, 2)) if integer else (d((32, cin, 3, 3), 0, 1), d((32,), 0, 2))
    if mode == 'stem':
        x = (torch.rand(N, 17, H, W, generator=d.g) < 0.2).float()
        h = x.double()
    else:
        yp, hp = d((N, 32, H, W), -3, 3), d((N, 32, H, W), 0, 2)
        al = torch.ones(32) if integer else d((32,), 0.5, 1.5)
        be = d((32,), -1, 1)
        o = yp * al.view(1, -1, 1, 1) + be.view(1, -1, 1, 1)   # fp32, the contract's operation order
        h = torch.relu(hp + o if mode == 'residual' else o).bfloat16().double()
    y = conv64(h, w) + b.double().view(1, -1, 1, 1)
    assert not integer or float(y.abs().max()) < 256
    arena = Arena(cuda)
    y_out = bf_out(arena, N, HW, 'y')
    part = arena.out((lib.hrl_torus_bf16_stats_blocks(N), 32, 2), torch.float64, name='part')
    pack = packed(lib, cuda, [w] if mode == 'stem' else [torch.zeros(32, 17, 3, 3), w])
    s = _native.stream_of(cuda)
    if mode == 'stem':
        keep = (x.to(cuda),)
        rc = lib.hrl_torus_bf16_unit_forward(P(keep[0]), None, None, None, None, None, N, H, W, P(pack), 0,
                                             P(b.to(cuda)), P(y_out), P(part), s)
    else:
        h_out = bf_out(arena, N, HW, 'h')
        keep = (to_cl(yp).to(cuda), to_cl(hp).to(cuda) if mode == 'residual' else None, al.to(cuda), be.to(cuda),
                b.to(cuda))
        rc = lib.hrl_torus_bf16_unit_forward(None, P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), P(h_out), N, H, W,
                                             P(pack), 1, P(keep[4]), P(y_out), P(part), s)
    assert rc == 0
    arena.check()
    if mode != 'stem':
        close(from_cl(h_out, H, W), h, True)   # h is bf(.) of the reference: equal on either kind of data
    close(from_cl(y_out, H, W), y, integer)
    terms = conv64(h.abs(), w.abs()) + b.abs().double().view(1, -1, 1, 1)
    sums = torch.stack([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))], 1)
    close(part.sum(0), sums, integer, torch.stack([terms.sum((0, 2, 3)), (terms * terms).sum((0, 2, 3))], 1),
          n=N * HW + 9 * cin)


@pytest.mark.parametrize('H,W,N,integer', CONV_CASES)
@pytest.mark.parametrize('g_fp32', [0, 1])
def test_adjoint_launch(cuda, g_fp32, H, W, N, integer):
    lib, d, HW = _native.load(), Data(3 * H * W + N, integer), H * W
    shape = (N, 32, H, W)
    lo = -1 if integer else 0                                   # random operands of one sign: ONE_SIGN above
    w = d((32, 32, 3, 3), lo, 1, 0.04 if integer else 1.0)
    dy, g, hn, hm, yp, mean = d(shape, 2 * lo, 2), d(shape, 3 * lo, 3), d(shape, -1, 1), d(shape, -1, 1), \
        d(shape, -3, 3), d((32,), -1, 1)
    hn, hm = torch.relu(hn), torch.relu(hm)
    gm = g * (hn > 0) if not g_fp32 else g
    xin = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    ref = torch.autograd.grad(conv64(xin, w), xin, dy.double())[0] + gm.double()
    assert not integer or float(ref.abs().max()) < 256
    arena = Arena(cuda)
    dh = bf_out(arena, N, HW, 'dh')
    part = arena.out((lib.hrl_torus_bf16_stats_blocks(N), 32, 2), torch.float64, name='part')
    pack = packed(lib, cuda, [torch.zeros(32, 17, 3, 3), w])
    g_dev = g.flatten(2).transpose(1, 2).contiguous().to(cuda) if g_fp32 else to_cl(g).to(cuda)
    keep = (to_cl(dy).to(cuda), to_cl(hn).to(cuda), to_cl(hm).to(cuda), to_cl(yp).to(cuda), mean.to(cuda))
    assert lib.hrl_torus_bf16_unit_input_grad(P(keep[0]), N, H, W, P(pack), 1, P(g_dev), g_fp32, P(keep[1]), P(dh),
                                              P(keep[2]), P(keep[3]), P(keep[4]), P(part),
                                              _native.stream_of(cuda)) == 0
    arena.check()
    got = from_cl(dh, H, W)
    close(got, ref, integer)
    v = got.cpu() * (hm > 0)                                    # the sums take the stored gradient
    c = yp.double() - mean.double().view(1, -1, 1, 1)
    close(part.sum(0), torch.stack([v.sum((0, 2, 3)), (v * c).sum((0, 2, 3))], 1), integer,
          torch.stack([v.abs().sum((0, 2, 3)), (v * c).abs().sum((0, 2, 3))], 1), n=N * HW)


@pytest.mark.parametrize('H,W,N,integer', WGRAD_CASES)
@pytest.mark.parametrize('mode', ['stem', 'plain', 'residual', 'last'])
def test_weight_gradient_launch(cuda, mode, H, W, N, integer):
    lib, d, HW = _native.load(), Data(5 * H * W + N, integer), H * W
    shape, cin, g_fp32 = (N, 32, H, W), 17 if mode == 'stem' else 32, int(mode == 'last')
    x = (torch.rand(N, 17, H, W, generator=d.g) < 0.2).float() if mode == 'stem' else torch.relu(d(shape, -1, 3))
    one = lambda lo, hi: d((32,), lo, hi)
    if integer:
        y, g, mean, gmean = d(shape, -2, 2), d(shape, -2, 2), one(-1, 1), one(-1, 1)
    else:                                                       # every term of dy of one sign: ONE_SIGN above
        y, g, mean, gmean = d(shape, -2, 0), d(shape, 0, 2), one(0, 1), one(-1, 0)
    al, be, k = (torch.ones(32) if integer else one(0.5, 1.5)), one(-1, 1), one(0, 1)
    invstd, gamma = (2.0 ** one(0, 1), 2.0 ** one(0, 1)) if integer else (one(0.5, 2), one(0.5, 2))
    col = lambda t: t.double().view(1, -1, 1, 1)
    o = y * al.view(1, -1, 1, 1) + be.view(1, -1, 1, 1)          # fp32, the forward's operation order
    o = x + o if mode in ('residual', 'last') else o
    gm = g.double() if g_fp32 else g.double() * (torch.relu(o).bfloat16() > 0)
    dy = (((gm - col(gmean)) - (y.double() - col(mean)) * col(k)) * col(invstd)) * col(gamma)
    dyb = dy.float().bfloat16().double()
    assert not integer or (float(dy.abs().max()) < 256 and torch.equal(dy, dyb))
    arena = Arena(cuda)
    dy_out = bf_out(arena, N, HW, 'dy')
    dw, db = arena.out((32, cin, 3, 3), name='dw'), arena.out((32,), name='db')
    ws = arena.ws(lib.hrl_torus_bf16_workspace_bytes(N), name='ws')
    g_dev = g.flatten(2).transpose(1, 2).contiguous().to(cuda) if g_fp32 else to_cl(g).to(cuda)
    keep = [t.to(cuda) for t in (al, be, gamma, mean, invstd, k, gmean)]
    x_dev = x.to(cuda) if mode == 'stem' else to_cl(x).to(cuda)
    y_dev = to_cl(y).to(cuda)
    assert lib.hrl_torus_bf16_wgrad_bn(P(x_dev) if mode == 'stem' else None, None if mode == 'stem' else P(x_dev), N, H,
                                       W, P(y_dev), P(g_dev), g_fp32, P(keep[0]), P(keep[1]),
                                       int(mode in ('residual', 'last')), P(keep[2]), P(keep[3]), P(keep[4]),
                                       P(keep[5]), P(keep[6]), P(dy_out), P(dw), P(db), P(ws), ws.numel(),
                                       _native.stream_of(cuda)) == 0
    arena.check()
    got = from_cl(dy_out, H, W).cpu()
    close(got, dy, integer)
    # dW and db from the stored DY, as the contract forms them
    wv = torch.zeros(32, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    ref_dw = torch.autograd.grad(conv64(x, wv), wv, got)[0]
    t_dw = torch.autograd.grad(conv64(x.abs(), wv), wv, got.abs())[0]
    close(dw, ref_dw, integer, t_dw, n=N * HW)
    close(db, got.sum((0, 2, 3)), integer, got.abs().sum((0, 2, 3)), n=N * HW)


# ------------------------------------------------------------------------------------------------ the tower
def tower_net(L, cuda, seed=7):
    torch.manual_seed(seed)
    net = GeeseNet(layers=L).train()
    with torch.no_grad():
        for u in [net.conv0, *net.blocks]:
            u.bn.weight.uniform_(0.5, 1.5)
            u.bn.bias.uniform_(-0.5, 0.5)
    return net, hnn.accelerate(copy.deepcopy(net).to(cuda)).train()


def units_of(net):
    return [net.conv0, *net.blocks]


def tower64(net, x, rounded):
    """The fp64 tower of `net` (a double copy, training mode) and the running statistics its BatchNorms end with;
    rounded: the contract's storage points as straight-through bf16 roundings (the emulation)."""
    r = (lambda t: t + (t.float().bfloat16().double() - t).detach()) if rounded else (lambda t: t)
    h, stats, ys, n = r(x), [], [], x.shape[0] * x.shape[2] * x.shape[3]
    for i, u in enumerate(units_of(net)):
        y = conv64(h, r(u.conv.weight)) + u.conv.bias.view(1, -1, 1, 1)
        ys.append(y)
        if y.requires_grad:
            y.retain_grad()
        mu, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        stats += [(0.9 * u.bn.running_mean + 0.1 * mu).detach(), (0.9 * u.bn.running_var + 0.1 * var * n / (n - 1)).detach()]
        al = u.bn.weight / torch.sqrt(var + u.bn.eps)
        o = r(y) * al.view(1, -1, 1, 1) + (u.bn.bias - mu * al).view(1, -1, 1, 1)
        full = torch.relu(o if i == 0 else h + o)
        h = r(full)
    return full, stats, ys


def tower_grads(net):
    return [p.grad.detach().cpu().double() for u in units_of(net) for p in (u.conv.weight, u.conv.bias, u.bn.weight,
                                                                           u.bn.bias)]


def run_tower(gpu, x, gout, precision):
    gpu.zero_grad()
    h = hnn.torus_tower(x, units_of(gpu), precision)
    h.backward(gout)
    return h.detach(), tower_grads(gpu)


@pytest.mark.parametrize('L', [1, 12])
def test_tower_forward_and_gradients(cuda, L):
    net, gpu = tower_net(L, cuda)
    g = torch.Generator().manual_seed(L)
    x = (torch.rand(9, 17, 7, 11, generator=g) < 0.2).float()
    gout = torch.randn(9, 32, 7, 11, generator=g)
    h, grads = run_tower(gpu, x.to(cuda), gout.to(cuda), 'bf16')
    exact, emu = copy.deepcopy(net).double(), copy.deepcopy(net).double()
    with torch.no_grad():
        h64, stats64, _ = tower64(exact, x.double(), False)
    he, stats_e, ys = tower64(emu, x.double(), True)
    he.backward(gout.double())
    e_k, e_e = float((h.cpu().double() - h64).abs().max()), float((he.detach() - h64).abs().max())
    print('L = %d forward max |error| against fp64: kernel %.3e, emulation %.3e' % (L, e_k, e_e))
    assert e_e > 0 and e_k <= 2 * e_e + 1e-6
    got_stats = [t.cpu().double() for u in units_of(gpu) for t in (u.bn.running_mean, u.bn.running_var)]
    s_k = max(float((a - b).abs().max()) for a, b in zip(got_stats, stats64))
    s_e = max(float((a - b).abs().max()) for a, b in zip(stats_e, stats64))
    print('L = %d running statistics max |error| against fp64: kernel %.3e, emulation %.3e' % (L, s_k, s_e))
    assert s_k <= 2 * s_e + 1e-6
    assert all(int(u.bn.num_batches_tracked) == 1 for u in units_of(gpu))
    ref_grads, bound = tower_grads(emu), (L + 2) * 2.0 ** -8
    for i, (got, want) in enumerate(zip(grads, ref_grads)):
        # conv bias: zero in exact arithmetic; relative to the sums of its absolute terms (the module docstring)
        scale = want.norm() if i % 4 != 1 else ys[i // 4].grad.abs().sum((0, 2, 3)).norm()
        rel = float((got - want).norm() / scale)
        print('L = %d unit %d %s: relative L2 error %.3e (bound %.3e)'
              % (L, i // 4, ('conv.weight', 'conv.bias', 'bn.weight', 'bn.bias')[i % 4], rel, bound))
        assert rel <= bound, (i, rel)


def test_determinism_rows_and_no_leak_into_fp32(cuda):
    net, gpu = tower_net(2, cuda)
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(9, 17, 7, 11, generator=g) < 0.2).float().to(cuda)
    gout = torch.randn(9, 32, 7, 11, generator=g).to(cuda)
    state = copy.deepcopy(gpu.state_dict())
    same = lambda a, b: all(torch.equal(bits(s), bits(t)) for s, t in zip(a, b))
    f_h, f_g = run_tower(gpu, x, gout, 'fp32')
    gpu.load_state_dict(state)
    b_h, b_g = run_tower(gpu, x, gout, 'bf16')
    gpu.load_state_dict(state)
    b_h2, b_g2 = run_tower(gpu, x, gout, 'bf16')
    gpu.load_state_dict(state)
    f_h2, f_g2 = run_tower(gpu, x, gout, 'fp32')
    assert torch.equal(bits(b_h), bits(b_h2)) and same(b_g, b_g2)              # deterministic
    assert torch.equal(bits(f_h), bits(f_h2)) and same(f_g, f_g2)              # the fp32 tower is untouched
    assert not torch.equal(f_h, b_h)                                           # and the option does something
    # a statistics-free launch (the stem's conv): rows of N = 9 equal the same rows of a batch past the stride
    lib, s = _native.load(), _native.stream_of(cuda)
    big = (torch.rand(4097, 17, 7, 11, generator=g) < 0.2).float().to(cuda)
    big[:9] = x
    pack = packed(lib, cuda, [gpu.conv0.conv.weight.detach()])
    outs = []
    for xs in (x, big):
        n = xs.shape[0]
        y = torch.empty(n, 77, 32, dtype=torch.bfloat16, device=cuda)
        part = torch.empty(lib.hrl_torus_bf16_stats_blocks(n) * 64, dtype=torch.float64, device=cuda)
        assert lib.hrl_torus_bf16_unit_forward(P(xs), None, None, None, None, None, n, 7, 11, P(pack), 0,
                                               P(gpu.conv0.conv.bias.detach()), P(y), P(part), s) == 0
        outs.append(y[:9].clone())
    assert torch.equal(bits(outs[0]), bits(outs[1]))


def test_learner_step_as_a_captured_graph(cuda):
    """train_args precision: bf16 through LearnerStep: the captured step replays with finite losses and moving
    weights, and launches as many torus kernels (conv, adjoint, weight gradient, reduce, pool) as the fp32 tower."""
    from torch.profiler import ProfilerActivity, profile
    from handyrl_amd.synthetic import geese_args, geese_batch
    from handyrl_amd.trainer import LearnerStep
    B, T, counts = 4, 4, {}
    batch = geese_batch(B, T, cuda, seed=3)
    for precision in ('fp32', 'bf16'):
        torch.manual_seed(3)
        step = LearnerStep(GeeseNet(layers=2), dict(geese_args(T, B), precision=precision), cuda, graph=True)
        assert step.precision == precision
        before = step.net.conv0.conv.weight.detach().clone()
        for _ in range(3):                                       # eager warm-up, capture, first replay
            step.step(batch)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            outs = [step.step(batch) for _ in range(3)]
            torch.cuda.synchronize()
        assert all(bool(torch.isfinite(torch.as_tensor(float(o['total'])))) for o in outs)
        assert not torch.equal(before, step.net.conv0.conv.weight.detach())
        names = [e.name for e in prof.events() if 'torus' in e.name and 'pack' not in e.name]
        counts[precision] = len(names)
        assert any('torus_bf16' in n for n in names) == (precision == 'bf16')
    print('torus launches in 3 replays:', counts)
    assert counts['bf16'] == counts['fp32'] > 0
