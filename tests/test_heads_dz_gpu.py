"""The fused heads hand the chain's last block dz (N, 28) instead of dh (N, 288).

hrl_heads_backward_dz stops writing dh = W1^T dz and hrl_conv3x3_block_backward_dz rebuilds it per element with the
same float operations, so everything downstream is bit-identical to the materialised-dh path:
* the heads entry: weight gradients and BN sums equal to hrl_heads_backward's, dz's pad 0, rows past N untouched,
  and dh rebuilt on the CPU from the kernel's dz (separate fp32 multiplies and adds, m ascending) equal to the old
  entry's dh;
* the block entry: gin, dweight (or the workspace's partial rows) and the epilogue-2 sums equal to
  hrl_conv3x3_block_backward fed that dh;
* the argument checks of both entries;
* one learner step of the TicTacToe net with nn.HEADS_DZ on and off: losses and every parameter gradient equal,
  eager and under graph capture.
"""

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 3           # rows allocated after row N: must keep their fill
FILL = 12345.0

_HEADS = {}         # (N, bn) -> the two heads entries' results, computed once and left unchanged


def _heads_case(cuda, N, bn):
    """hrl_heads_backward (dh) and hrl_heads_backward_dz (dz) on the same seeded inputs."""
    key = (N, bn)
    if key in _HEADS:
        return _HEADS[key]
    from handyrl_amd import _native
    lib = _native.load()
    P = _native.ptr
    stream = _native.stream_of(cuda)
    g0 = torch.Generator(device=cuda).manual_seed(N + 7 * bn)
    rnd = lambda *s: torch.randn(*s, device=cuda, generator=g0)   # noqa: E731
    y = rnd(N, 288)
    w1p, w1v, wp, wv = rnd(2, 32), rnd(1, 32), rnd(9, 18), rnd(1, 9)
    a_p, a_v = rnd(N, 18), rnd(N, 9)
    dp, dv = rnd(N, 9), rnd(N, 1)
    vt = torch.tanh(rnd(N, 1))
    al, be, mu = (rnd(32).abs() + 0.5, rnd(32) * 0.3, rnd(32) * 0.1) if bn else (None, None, None)
    assert lib.hrl_heads_set_bwd_form(0) == 2
    ws_bytes = lib.hrl_heads_workspace_bytes(N)
    nparts = lib.hrl_heads_bn_parts(N)
    res = {'w1p': w1p, 'w1v': w1v}
    for name, entry, width in (('old', lib.hrl_heads_backward, 288), ('dz', lib.hrl_heads_backward_dz, 28)):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cuda)
        part = torch.zeros(nparts * 64, dtype=torch.float64, device=cuda)
        out = torch.full((N + GUARD, width), FILL, device=cuda)
        grads = [torch.empty(2, 32, device=cuda), torch.empty(2, device=cuda), torch.empty(1, 32, device=cuda),
                 torch.empty(1, device=cuda), torch.empty(9, 18, device=cuda), torch.empty(1, 9, device=cuda)]
        _native.check(entry(P(y), N, P(w1p), P(w1v), P(wp), P(wv), P(al), P(be), P(mu), P(part) if bn else None,
                            P(a_p), P(a_v), P(dp), P(dv), P(vt), P(out), *[P(o) for o in grads], P(ws), ws_bytes,
                            stream), 'heads_backward ' + name)
        torch.cuda.synchronize(cuda)
        res[name] = (out, grads, part)
    _HEADS[key] = res
    return res


@pytest.mark.parametrize('N', [1, 31, 32, 33, 37, 4099])
@pytest.mark.parametrize('bn', [False, True])
def test_heads_backward_dz_matches_dh_entry(cuda, N, bn):
    """N around the 32-row block (31, 32, 33), one row, a ragged block (37) and several workgroups (4099)."""
    res = _heads_case(cuda, N, bn)
    (dh, grads0, part0), (dz, grads1, part1) = res['old'], res['dz']
    for a, b in zip(grads1, grads0):
        assert torch.equal(a, b)
    assert torch.equal(part1, part0)
    assert bool((dz[:N, 27] == 0).all())
    assert bool((dz[N:] == FILL).all()) and bool((dh[N:] == FILL).all())
    # dh[c][q] = ((0 + W1[0][c] dz[0][q]) + W1[1][c] dz[1][q]) + W1[2][c] dz[2][q], fp32, one rounding per operation
    w1 = torch.cat([res['w1p'], res['w1v']]).cpu()          # (3, 32)
    d = dz[:N, :27].cpu().view(N, 3, 1, 9)
    t = torch.zeros(N, 32, 9)
    for m in range(3):
        prod = w1[m].view(1, 32, 1) * d[:, m]
        t = t + prod
    assert torch.equal(t.view(N, 288), dh[:N].cpu())


def _block_inputs(cuda, M, pro):
    from handyrl_amd import _native
    lib = _native.load()
    g0 = torch.Generator(device=cuda).manual_seed(M + 2)
    rnd = lambda *s: torch.randn(*s, device=cuda, generator=g0)   # noqa: E731
    y, x = rnd(M, 288), rnd(M, 288)
    w = rnd(32, 32, 3, 3) * 0.1
    gamma, beta = rnd(32).abs() + 0.5, rnd(32) * 0.2
    mean, invstd = rnd(32) * 0.1, rnd(32).abs() + 0.5
    kcoef, gmean = rnd(32) * 0.1, rnd(32) * 0.1
    a, b = rnd(32).abs() + 0.5, rnd(32) * 0.3
    alpha, bet = (a, b) if pro else (None, None)
    em, ea, eb = rnd(32) * 0.1, rnd(32).abs() + 0.5, rnd(32) * 0.3
    packed = torch.empty(1, 2, 9216, device=cuda)
    _native.check(lib.hrl_conv3x3_pack_n(_native.ptr_array([w]), 1, _native.ptr(packed), _native.stream_of(cuda)),
                  'pack')
    return dict(y=y, x=x, gamma=gamma, beta=beta, mean=mean, invstd=invstd, kcoef=kcoef, gmean=gmean, alpha=alpha,
                bet=bet, em=em, ea=ea, eb=eb, packed=packed)


def _block_call(cuda, M, c, g, w1, dweight, gin, epi, part, ws):
    """The old entry (w1 None, g = dh) or the dz entry (g = dz, w1 = (w1p, w1v)); returns the status code."""
    from handyrl_amd import _native
    lib = _native.load()
    P = _native.ptr
    tail = (P(c['y']), M, P(c['gamma']), P(c['beta']), P(c['mean']), P(c['invstd']), P(c['kcoef']), P(c['gmean']),
            P(c['x']), P(c['alpha']), P(c['bet']), P(c['packed'][0, 1]), P(dweight), P(gin), epi, P(c['em']),
            P(c['ea']), P(c['eb']), P(part), P(ws), ws.numel(), _native.stream_of(cuda))
    if w1 is None:
        return lib.hrl_conv3x3_block_backward(P(g), *tail)
    return lib.hrl_conv3x3_block_backward_dz(P(g), P(w1[0]), P(w1[1]), *tail)


@pytest.mark.parametrize('M', [1, 16, 17, 37, 117, 4099, 20000])
@pytest.mark.parametrize('pro', [False, True])
def test_block_backward_dz_matches_dh_entry(cuda, M, pro):
    """M = 1, 16, 17: one tile, full, and one row into the second; 37: one workgroup, 3 tiles, the last ragged;
    117: two workgroups of 4 iterations; 4099 and 20000: every workgroup several tiles."""
    from handyrl_amd import _native
    lib = _native.load()
    heads = _heads_case(cuda, M, True)
    dh, dz = heads['old'][0][:M], heads['dz'][0][:M]
    w1 = (heads['w1p'], heads['w1v'])
    c = _block_inputs(cuda, M, pro)
    assert lib.hrl_conv3x3_set_block_form(1) == 1
    ws_bytes = lib.hrl_conv3x3_workspace_bytes(M)
    nblk = lib.hrl_conv3x3_block_sum_blocks(M)
    off = ctypes.c_int64(0)
    nparts = lib.hrl_conv3x3_wgrad_partials(M, ctypes.byref(off))
    res = []
    for g, w in ((dh, None), (dz, w1)):
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=cuda)
        ws2 = torch.zeros(ws_bytes, dtype=torch.uint8, device=cuda)
        dw = torch.empty(32, 32, 3, 3, device=cuda)
        gin, part = torch.empty(M, 288, device=cuda), torch.zeros(nblk * 64, dtype=torch.float64, device=cuda)
        gin2, part2 = torch.empty_like(gin), torch.zeros_like(part)
        _native.check(_block_call(cuda, M, c, g, w, dw, gin, 2, part, ws), 'block')
        _native.check(_block_call(cuda, M, c, g, w, None, gin2, 2, part2, ws2), 'block (partials)')
        torch.cuda.synchronize(cuda)
        rows = ws2[off.value:].view(torch.float32)[:nparts * 9216].clone()
        res.append((gin, dw, part, gin2, part2, rows))
    for a, b in zip(res[1], res[0]):
        assert torch.equal(a, b)


def test_dz_entries_argument_checks(cuda):
    """HRL_EINVAL before any launch: the block entry for epilogues 0 and 3, no gin, and the per-wave block form; the
    heads entry under form 1.  The outputs keep their fill."""
    from handyrl_amd import _native
    lib = _native.load()
    P = _native.ptr
    M = 37
    heads = _heads_case(cuda, M, True)
    dz, w1 = heads['dz'][0][:M], (heads['w1p'], heads['w1v'])
    c = _block_inputs(cuda, M, True)
    ws = torch.zeros(lib.hrl_conv3x3_workspace_bytes(M), dtype=torch.uint8, device=cuda)
    dw = torch.full((32, 32, 3, 3), FILL, device=cuda)
    gin = torch.full((M, 288), FILL, device=cuda)
    part = torch.zeros(lib.hrl_conv3x3_block_sum_blocks(M) * 64, dtype=torch.float64, device=cuda)
    assert lib.hrl_conv3x3_set_block_form(1) == 1
    assert _block_call(cuda, M, c, dz, w1, dw, gin, 0, part, ws) == _native.HRL_EINVAL
    assert _block_call(cuda, M, c, dz, w1, dw, gin, 3, part, ws) == _native.HRL_EINVAL
    assert _block_call(cuda, M, c, dz, w1, dw, None, 2, part, ws) == _native.HRL_EINVAL
    prev = lib.hrl_conv3x3_set_block_form(0)
    try:
        assert _block_call(cuda, M, c, dz, w1, dw, gin, 2, part, ws) == _native.HRL_EINVAL
    finally:
        lib.hrl_conv3x3_set_block_form(prev)
    torch.cuda.synchronize(cuda)
    assert bool((dw == FILL).all()) and bool((gin == FILL).all()) and bool((part == 0).all())
    # the heads entry under the row-per-lane form
    N = 37
    rnd = lambda *s: torch.randn(*s, device=cuda)   # noqa: E731
    y, a_p, a_v, dp, dv = rnd(N, 288), rnd(N, 18), rnd(N, 9), rnd(N, 9), rnd(N, 1)
    w1p, w1v, wp, wv = rnd(2, 32), rnd(1, 32), rnd(9, 18), rnd(1, 9)
    out = torch.full((N, 28), FILL, device=cuda)
    grads = [torch.empty(2, 32, device=cuda), torch.empty(2, device=cuda), torch.empty(1, 32, device=cuda),
             torch.empty(1, device=cuda), torch.empty(9, 18, device=cuda), torch.empty(1, 9, device=cuda)]
    prev = lib.hrl_heads_set_bwd_form(1)
    try:
        ws_bytes = lib.hrl_heads_workspace_bytes(N)
        hws = torch.empty(ws_bytes, dtype=torch.uint8, device=cuda)
        rc = lib.hrl_heads_backward_dz(P(y), N, P(w1p), P(w1v), P(wp), P(wv), None, None, None, None, P(a_p), P(a_v),
                                       P(dp), P(dv), None, P(out), *[P(o) for o in grads], P(hws), ws_bytes,
                                       _native.stream_of(cuda))
    finally:
        lib.hrl_heads_set_bwd_form(prev)
    assert rc == _native.HRL_EINVAL
    torch.cuda.synchronize(cuda)
    assert bool((out == FILL).all())
    assert lib.hrl_heads_set_bwd_form(0) == 2 and lib.hrl_conv3x3_set_block_form(1) == 1


@pytest.mark.parametrize('rows,graph', [(37, False), (37, True), (4099, False)])
def test_learner_step_equal_with_and_without_dz(cuda, rows, graph):
    """One LearnerStep of the TicTacToe net at B*T = rows from identical state with nn.HEADS_DZ on and off: the
    losses and every parameter gradient are bit-identical, eager and captured."""
    from handyrl_amd import nn as hnn
    from handyrl_amd.envs.tictactoe import SimpleConv2dModel
    from handyrl_amd.synthetic import tictactoe_batch, default_args
    from handyrl_amd.trainer import LearnerStep
    B, T = rows, 1
    args = default_args(T, B)
    batch = tictactoe_batch(B, T, cuda, seed=rows)
    torch.manual_seed(2)
    state = {k: v.clone() for k, v in SimpleConv2dModel().state_dict().items()}
    prev = hnn.HEADS_DZ
    res = []
    try:
        for on in (True, False):
            hnn.HEADS_DZ = on
            net = SimpleConv2dModel()
            net.load_state_dict(state)
            step = LearnerStep(net, args, cuda, graph=graph)
            out = step.step(batch)
            torch.cuda.synchronize()
            res.append(({k: v.detach().clone() for k, v in out.items()},
                        {n: p.grad.detach().clone() for n, p in step.net.named_parameters()}))
    finally:
        hnn.HEADS_DZ = prev
    (out1, g1), (out0, g0) = res
    assert set(out1) == set(out0) and set(g1) == set(g0) and g1
    for k in out0:
        assert torch.equal(out1[k], out0[k]), k
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
