"""One-launch recurrent GeisterNet inference on the GPU (csrc/hrl_geister_infer.hip), at the C entry with guard-band
outputs (tests/guarded.py) and through nn.GeisterInference.

Reference: the plain cell-by-cell ``GeisterNet.forward`` in fp64 on the CPU.  Yardstick: the GPU module path (the
``accelerate``d net in its own session).  Rule (the GeeseNet tower test's): the wrapper's largest absolute error may
be at most twice the module path's on the same inputs, plus 1e-6 -- the fold and the summation order differ.

Launch shape: one workgroup per (16-row tile, layer) item on a grid of at most 256, further items walked by the same
workgroups.  A workgroup first takes a second item when tiles * L exceeds 256, i.e. past N = 16 * (256 // L): 4096,
2048, 1360, 1024 for L = 1..4.  The sizes are 1, the tile +- 1 (15, 16, 17), two tiles + 1 (33) and that N and N + 1."""

import copy

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.envs.geister import GeisterBatch, GeisterNet
from tests.guarded import Arena, bits

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 33)
CONFIGS = {'stock': (3, 3, 8, True), 'small': (1, 1, 4, True), 'deep': (4, 2, 2, True), 'nobias': (2, 2, 8, False)}
KEYS = ('policy', 'value', 'return')


def make_net(layers, repeats, p_filters, bias, seed=7):
    """A net with non-trivial statistics: BN running mean / var random (var in [0.25, 4]), BN weights / biases and
    cell biases O(1)."""
    torch.manual_seed(seed)
    net = GeisterNet(layers=layers, p_filters=p_filters, num_repeats=repeats)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        if not bias:
            for cell in net.body.blocks:
                cell.conv.bias = None
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                m.running_mean.copy_(torch.randn(C, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(C, generator=g) * 3.75 + 0.25)
                m.weight.copy_(torch.rand(C, generator=g) + 0.5)
                m.bias.copy_(torch.randn(C, generator=g) * 0.5)
        for cell in net.body.blocks:
            if cell.conv.bias is not None:
                cell.conv.bias.copy_(torch.randn(128, generator=g) * 0.5)
    return net.eval()


def inputs(N, layers, seed):
    """Geister-like observations and an O(1) random state (stacked (N, L*32, 6, 6))."""
    g = torch.Generator().manual_seed(seed)
    obs = {'board': (torch.rand(N, 7, 6, 6, generator=g) < 0.2).float(),
           'scalar': torch.cat([(torch.rand(N, 1, generator=g) < 0.5).float(), torch.rand(N, 17, generator=g)], 1)}
    return obs, torch.randn(N, layers * 32, 6, 6, generator=g), torch.randn(N, layers * 32, 6, 6, generator=g)


def leaves(t):
    return list(t.split(32, 1))


def forward64(net, obs, h, c):
    n64 = copy.deepcopy(net).cpu().double().eval()
    with torch.no_grad():
        out = n64({k: v.cpu().double() for k, v in obs.items()}, (leaves(h.cpu().double()), leaves(c.cpu().double())))
    return out, torch.cat(out['hidden'][0], 1), torch.cat(out['hidden'][1], 1)


def flat(out):
    """policy, value, return and the stacked state of a forward's output, on the CPU."""
    return [out[k].cpu() for k in KEYS] + [torch.cat([t.cpu() for t in out['hidden'][i]], 1) for i in (0, 1)]


def c_forward(w, obs, h, c):
    """hrl_geister_infer with every output between sentinels."""
    N, dev = h.shape[0], h.device
    arena = Arena(dev)
    outs = [arena.out(s, name=n) for n, s in (('policy', (N, 214)), ('value', (N, 1)), ('ret', (N, 1)),
                                               ('h_out', tuple(h.shape)), ('c_out', tuple(c.shape)))]
    code = _native.load().hrl_geister_infer(
        _native.ptr(w.pack(dev)), w.layers, w.net.num_repeats, w.p_filters, _native.ptr(obs['board']),
        _native.ptr(obs['scalar']), _native.ptr(h), _native.ptr(c), N, *[_native.ptr(o) for o in outs],
        _native.stream_of(dev))
    assert code == _native.HRL_OK, code
    arena.check()
    return [o.clone().cpu() for o in outs]


@pytest.fixture(scope='module')
def cases(cuda):
    """Per configuration: the GPU net, its wrapper, the largest batch's inputs, the fp64 result, the module path's
    and the wrapper's (C entry) -- computed once and left unchanged."""
    made = {}

    def get(name):
        if name not in made:
            L, R, pf, bias = CONFIGS[name]
            sizes = SIZES + (16 * (256 // L), 16 * (256 // L) + 1)
            net = make_net(L, R, pf, bias)
            obs, h, c = inputs(max(sizes), L, seed=3)
            r64, h64, c64 = forward64(net, obs, h, c)
            ref = [r64[k] for k in KEYS] + [h64, c64]
            gnet = hnn.accelerate(copy.deepcopy(net).to(cuda)).eval()
            gobs, gh, gc = {k: v.to(cuda) for k, v in obs.items()}, h.to(cuda), c.to(cuda)
            w = hnn.GeisterInference(gnet)
            with torch.no_grad():
                with gnet.inference_session():
                    mod = flat(gnet(gobs, (leaves(gh), leaves(gc))))
                with w.inference_session():
                    big = c_forward(w, gobs, gh, gc)
            made[name] = dict(net=net, gnet=gnet, w=w, obs=gobs, h=gh, c=gc, ref=ref, mod=mod, big=big, sizes=sizes)
        return made[name]
    return get


def within_rule(got, mod, ref, what):
    for name, a, m, r in zip(KEYS + ('h', 'c'), got, mod, ref):
        e_new, e_mod = float((a.double() - r).abs().max()), float((m.double() - r).abs().max())
        print('%s %s: wrapper %.3g, module path %.3g (|ref| up to %.3g)' % (what, name, e_new, e_mod, float(r.abs().max())))
        assert e_new <= 2 * e_mod + 1e-6, (what, name, e_new, e_mod)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_one_step_against_fp64(cases, name):
    """Every size of the configuration: policy (all 214 columns), value, return and every h, c leaf under the 2x +
    1e-6 rule, wrapper and C entry bit-identical.  Measured on an MI355X, wrapper / module path: stock N = 1361 policy
    2.5e-07 / 2.3e-07, value 1.3e-07 / 7.8e-08, return 9.4e-08 / 9.0e-08, h 3.8e-07 / 2.4e-07, c 7.7e-07 / 5.8e-07;
    small N = 4097 policy 2.3e-07 / 2.5e-07, h 4.2e-07 / 3.8e-07, c 9.5e-07 / 8.5e-07; deep N = 1025 h 3.1e-07 / 2.3e-07,
    c 9.0e-07 / 6.2e-07; nobias N = 2049 policy 1.9e-07 / 1.9e-07, value 2.0e-07 / 1.7e-07, h 3.1e-07 / 2.0e-07, c
    9.2e-07 / 6.2e-07."""
    k = cases(name)
    for N in k['sizes']:
        obs = {key: v[:N].contiguous() for key, v in k['obs'].items()}
        h, c = k['h'][:N].contiguous(), k['c'][:N].contiguous()
        with torch.no_grad(), k['w'].inference_session():
            got = c_forward(k['w'], obs, h, c)
            out = flat(k['w'](obs, (leaves(h), leaves(c))))
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, out)), N
        within_rule(got, [m[:N] for m in k['mod']], [r[:N] for r in k['ref']], '%s N=%d' % (name, N))


@pytest.mark.parametrize('name', list(CONFIGS))
def test_rows_do_not_depend_on_the_batch(cases, name):
    """Rows 0..16 of the largest batch equal, bit for bit, the N = 17 batch: the 15 padding rows of its last tile
    and the other tiles influence nothing."""
    k = cases(name)
    obs = {key: v[:17].contiguous() for key, v in k['obs'].items()}
    with torch.no_grad(), k['w'].inference_session():
        small = c_forward(k['w'], obs, k['h'][:17].contiguous(), k['c'][:17].contiguous())
    for a, b in zip(small, k['big']):
        assert torch.equal(bits(a), bits(b[:17]))


def test_recurrence_in_place(cases, cuda):
    """12 steps on N = 17 with fresh observations: the stacked state advanced in place (inplace_state session) equals
    the out-of-place run bit for bit at every step (an h overwritten before it was read would differ), and the last
    step is within the rule against fp64 unrolled over the same inputs."""
    k = cases('stock')
    N, L, T = 17, 3, 12
    steps = [inputs(N, L, seed=40 + t)[0] for t in range(T)]
    _, h0, c0 = inputs(N, L, seed=39)
    ref, mod = (h0.double(), c0.double()), (h0.to(cuda), c0.to(cuda))
    fresh, hin, cin = (h0.to(cuda), c0.to(cuda)), h0.to(cuda).clone(), c0.to(cuda).clone()
    with torch.no_grad():
        for obs in steps:
            gobs = {key: v.to(cuda) for key, v in obs.items()}
            r64, rh, rc = forward64(k['net'], obs, *ref)
            ref = (rh, rc)
            with k['gnet'].inference_session():
                m = k['gnet'](gobs, (leaves(mod[0]), leaves(mod[1])))
            mod = (torch.cat(m['hidden'][0], 1), torch.cat(m['hidden'][1], 1))
            with k['w'].inference_session():
                o = k['w'](gobs, (leaves(fresh[0]), leaves(fresh[1])))
            fresh = (torch.cat(o['hidden'][0], 1), torch.cat(o['hidden'][1], 1))
            with k['w'].inference_session(inplace_state=True):
                i = k['w'](gobs, (leaves(hin), leaves(cin)))
            assert i['hidden'][0][0].data_ptr() == hin.data_ptr() and i['hidden'][1][0].data_ptr() == cin.data_ptr()
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(flat(i), flat(o)))
            assert torch.equal(bits(hin), bits(fresh[0])) and torch.equal(bits(cin), bits(fresh[1]))
    within_rule(flat(i), flat(m), [r64[key] for key in KEYS] + [rh, rc], 'step 12')


def test_through_the_env(cuda):
    """12 plies of GeisterBatch(32), the moves random legal ones from a seeded CPU generator (fixed for both paths: a
    near-tie cannot fork the games); the mover's observation through the wrapper and the module path, each advancing
    its own inference_hidden state: policies, values and returns agree to 1e-5 at every ply."""
    E = 32
    net = hnn.accelerate(make_net(3, 3, 8, True).to(cuda)).eval()
    w = hnn.GeisterInference(net)
    env = GeisterBatch(E, cuda)
    g = torch.Generator().manual_seed(5)
    st_w, st_m = w.inference_hidden(E, 2, cuda), net.inference_hidden(E, 2, cuda)
    with torch.no_grad(), w.inference_session(inplace_state=True), net.inference_session(inplace_state=True):
        for t in range(12):
            p = t % 2
            assert bool((env.turn() == p).all())
            obs = env.observation(env.turn())
            a = w(obs, tuple([leaf[p] for leaf in kind] for kind in st_w))
            b = net(obs, tuple([leaf[p] for leaf in kind] for kind in st_m))
            for key in KEYS:
                torch.testing.assert_close(a[key], b[key], rtol=0, atol=1e-5)
            legal = env.legal().cpu()
            env.step(torch.multinomial(legal.float() + 1e-12, 1, generator=g).view(-1).to(cuda),
                     torch.ones(E, dtype=torch.bool, device=cuda))


def test_captured_ply_follows_the_weights(cases, cuda):
    """A captured ply replayed after a second session with changed weights equals the eager forward with the new
    weights, bit for bit, on several replays: the pack keeps its address and is refreshed in place."""
    k = cases('stock')
    net = copy.deepcopy(k['gnet'])
    w = hnn.GeisterInference(net)
    obs = {key: v[:33].contiguous() for key, v in k['obs'].items()}
    h, c = k['h'][:33].contiguous(), k['c'][:33].contiguous()
    hidden = (leaves(h), leaves(c))
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad():
        with w.inference_session():
            w(obs, hidden)
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                out = w(obs, hidden)
        for p in net.parameters():
            p.mul_(1.25)
        with w.inference_session():
            eager = flat(w(obs, hidden))
            for _ in range(3):
                graph.replay()
                torch.cuda.synchronize()
                assert all(torch.equal(bits(a), bits(b)) for a, b in zip(flat(out), eager))
    assert not torch.equal(eager[0], k['big'][0][:33])
