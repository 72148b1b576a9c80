"""One-launch bf16 GeisterNet inference on the GPU (csrc/hrl_geister_infer_bf16.hip), at the C entry with guard-band
outputs and through nn.GeisterInference(net, precision='bf16').

Reference: the plain cell-by-cell ``GeisterNet.forward`` in fp64 on the CPU.  Yardstick: the same forward in fp64
with ``.bfloat16().double()`` applied where include/hrl_nn.h's contract rounds (``emulate``).  Rule (the GeeseNet bf16
test's): the kernel's largest absolute error against fp64 is at most twice the emulation's on the same inputs, plus
1e-6, for each of policy, value, return, h and c; the emulation's own error is non-zero.

Launch shape: one workgroup per (T = 16-row tile, layer) item on a grid of at most 256, further items walked by the
same workgroups.  A workgroup first takes a second item when tiles * L exceeds 256: N2 = 16 * (256 // L) + 1 rows
(4097, 2049, 1361, 1025 for L = 1..4).  The sizes are 1, T - 1, T, T + 1, 2T + 1, N2 and N2 + 1."""

import copy

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from tests.guarded import Arena, bits
from tests.test_geister_infer_gpu import flat, forward64, inputs, leaves, make_net

pytestmark = pytest.mark.gpu

T = 16
CONFIGS = {'stock': (3, 3, 8, True), 'small': (1, 1, 4, True), 'deep': (4, 2, 2, True), 'nobias': (2, 2, 8, False)}
# make_net's seed per configuration: a net whose move, value and return heads all pass their ReLU somewhere in the batch
# (a head that is dead in fp64 is exactly 0 in every form, and "the emulation's error is non-zero" could not hold)
SEEDS = {'stock': 7, 'small': 11, 'deep': 14, 'nobias': 7}
KEYS = ('policy', 'value', 'return')


def bf(t):
    return t.bfloat16().double()


def emulate(net, obs, h, c):
    """The contract in fp64: 3x3 conv weights and every stored conv / head operand through bf16, the rest exact."""
    n = copy.deepcopy(net).cpu().double().eval()
    with torch.no_grad():
        for conv in [n.conv1, n.head_p_move.conv1] + [cell.conv for cell in n.body.blocks]:
            conv.weight.copy_(bf(conv.weight))
        board, scalar = obs['board'].cpu().double(), obs['scalar'].cpu().double()
        x = bf(torch.cat([scalar[..., None, None].expand(*scalar.shape, 6, 6), board], 1))
        h_e = bf(torch.relu(n.bn1(n.conv1(x))))
        hs, cs = leaves(h.cpu().double()), leaves(c.cpu().double())
        hb = [bf(t) for t in hs]
        for _ in range(n.num_repeats):
            for i, cell in enumerate(n.body.blocks):
                hs[i], cs[i] = cell(h_e, (hb[i], cs[i]))
                hb[i] = bf(hs[i])
        hh = torch.cat([h_e, hb[-1]], 1)
        policy = torch.cat([n.head_p_move(hh), n.head_p_set(scalar[:, :1])], -1)
        return [policy, torch.tanh(n.head_v(hh)), n.head_r(hh), torch.cat(hs, 1), torch.cat(cs, 1)]


def c_forward(w, obs, h, c, entry='hrl_geister_infer_bf16'):
    """The entry with every output between sentinels."""
    N, dev = h.shape[0], h.device
    arena = Arena(dev)
    outs = [arena.out(s, name=n) for n, s in (('policy', (N, 214)), ('value', (N, 1)), ('ret', (N, 1)),
                                               ('h_out', tuple(h.shape)), ('c_out', tuple(c.shape)))]
    code = getattr(_native.load(), entry)(
        _native.ptr(w.pack(dev)), w.layers, w.net.num_repeats, w.p_filters, _native.ptr(obs['board']),
        _native.ptr(obs['scalar']), _native.ptr(h), _native.ptr(c), N, *[_native.ptr(o) for o in outs],
        _native.stream_of(dev))
    assert code == _native.HRL_OK, code
    arena.check()
    return [o.clone().cpu() for o in outs]


def within_rule(got, emu, ref, what):
    for name, a, e, r in zip(KEYS + ('h', 'c'), got, emu, ref):
        e_new, e_emu = float((a.double() - r).abs().max()), float((e - r).abs().max())
        print('%s %s: kernel %.3g, emulation %.3g (|ref| up to %.3g)' % (what, name, e_new, e_emu, float(r.abs().max())))
        assert e_emu > 0 and e_new <= 2 * e_emu + 1e-6, (what, name, e_new, e_emu)


@pytest.fixture(scope='module')
def cases(cuda):
    """Per configuration: the GPU net, its bf16 wrapper, the largest batch's inputs, the fp64 result, the emulation's
    and the C entry's -- computed once and left unchanged."""
    made = {}

    def get(name):
        if name not in made:
            L, R, pf, bias = CONFIGS[name]
            n2 = T * (256 // L) + 1
            sizes = (1, T - 1, T, T + 1, 2 * T + 1, n2, n2 + 1)
            net = make_net(L, R, pf, bias, seed=SEEDS[name])
            obs, h, c = inputs(max(sizes), L, seed=3)
            r64, h64, c64 = forward64(net, obs, h, c)
            gnet = copy.deepcopy(net).to(cuda).eval()
            w = hnn.GeisterInference(gnet, precision='bf16')
            gobs, gh, gc = {k: v.to(cuda) for k, v in obs.items()}, h.to(cuda), c.to(cuda)
            with torch.no_grad(), w.inference_session():
                big = c_forward(w, gobs, gh, gc)
            made[name] = dict(net=net, gnet=gnet, w=w, obs=gobs, h=gh, c=gc, big=big, sizes=sizes,
                              ref=[r64[k] for k in KEYS] + [h64, c64], emu=emulate(net, obs, h, c))
        return made[name]
    return get


@pytest.mark.parametrize('name', list(CONFIGS))
def test_one_step_against_fp64(cases, name):
    """Every size: all five outputs between sentinels, bit-identical to the same rows of the largest batch (a row
    depends on nothing but the row), the wrapper equal to the C entry, and the largest batch within the rule (the
    rule compares two maxima of rounding noise: it is taken over the N2 + 1 rows that contain every smaller batch)."""
    k = cases(name)
    for N in k['sizes']:
        obs = {key: v[:N].contiguous() for key, v in k['obs'].items()}
        h, c = k['h'][:N].contiguous(), k['c'][:N].contiguous()
        with torch.no_grad(), k['w'].inference_session():
            got = c_forward(k['w'], obs, h, c)
            out = flat(k['w'](obs, (leaves(h), leaves(c))))
        assert all(torch.equal(bits(a), bits(b[:N])) for a, b in zip(got, k['big'])), N
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, out)), N
    within_rule(k['big'], k['emu'], k['ref'], name)


def test_recurrence_in_place(cases, cuda):
    """12 steps on N = 33 with fresh observations: the stacked state advanced in place equals the out-of-place run
    bit for bit at every step, and step 12 is within the rule against fp64 unrolled over the same inputs, the
    emulation unrolled too -- c included: a c that passed through bf16 anywhere is 2^-9 relative off, far outside."""
    k = cases('stock')
    N, L, steps = 33, 3, 12
    _, h0, c0 = inputs(N, L, seed=39)
    ref, emu = (h0.double(), c0.double()), (h0.double(), c0.double())
    fresh, hin, cin = (h0.to(cuda), c0.to(cuda)), h0.to(cuda).clone(), c0.to(cuda).clone()
    with torch.no_grad():
        for t in range(steps):
            obs = inputs(N, L, seed=40 + t)[0]
            gobs = {key: v.to(cuda) for key, v in obs.items()}
            r64, rh, rc = forward64(k['net'], obs, *ref)
            ref = (rh, rc)
            e = emulate(k['net'], obs, *emu)
            emu = (e[3], e[4])
            with k['w'].inference_session():
                o = k['w'](gobs, (leaves(fresh[0]), leaves(fresh[1])))
            fresh = (torch.cat(o['hidden'][0], 1), torch.cat(o['hidden'][1], 1))
            with k['w'].inference_session(inplace_state=True):
                i = k['w'](gobs, (leaves(hin), leaves(cin)))
            assert i['hidden'][0][0].data_ptr() == hin.data_ptr() and i['hidden'][1][0].data_ptr() == cin.data_ptr()
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(flat(i), flat(o)))
            assert torch.equal(bits(hin), bits(fresh[0])) and torch.equal(bits(cin), bits(fresh[1]))
    within_rule(flat(i), e, [r64[key] for key in KEYS] + [rh, rc], 'step 12')


def test_default_form_untouched(cases):
    """GeisterInference(net) and precision='fp32' are the exact entry, bit for bit, and not the bf16 one."""
    k = cases('stock')
    obs = {key: v[:33].contiguous() for key, v in k['obs'].items()}
    h, c = k['h'][:33].contiguous(), k['c'][:33].contiguous()
    a, b = hnn.GeisterInference(k['gnet']), hnn.GeisterInference(k['gnet'], precision='fp32')
    with torch.no_grad(), a.inference_session(), b.inference_session():
        direct = c_forward(a, obs, h, c, entry='hrl_geister_infer')
        outs = [flat(w(obs, (leaves(h), leaves(c)))) for w in (a, b)]
    for out in outs:
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(out, direct))
    assert not torch.equal(direct[0], k['big'][0][:33])


def test_captured_ply_follows_the_weights(cases, cuda):
    """A captured ply replayed after a second session with changed weights equals the eager forward with the new
    weights, bit for bit, on several replays: the pack keeps its address and is refreshed in place."""
    k = cases('stock')
    net = copy.deepcopy(k['gnet'])
    w = hnn.GeisterInference(net, precision='bf16')
    obs = {key: v[:33].contiguous() for key, v in k['obs'].items()}
    hidden = (leaves(k['h'][:33].contiguous()), leaves(k['c'][:33].contiguous()))
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad():
        with w.inference_session():
            address = w.pack(cuda).data_ptr()
            w(obs, hidden)
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                out = w(obs, hidden)
        for p in net.parameters():
            p.mul_(1.25)
        with w.inference_session():
            assert w.pack(cuda).data_ptr() == address
            eager = flat(w(obs, hidden))
            for _ in range(3):
                graph.replay()
                torch.cuda.synchronize()
                assert all(torch.equal(bits(a), bits(b)) for a, b in zip(flat(out), eager))
    assert not torch.equal(eager[0], k['big'][0][:33])
