"""forward_prediction's per-step plumbing kernels on their own (reference train.py:155-183): the recurrent-state
kernels (csrc/hrl_hidden.hip), the ConvLSTM gate kernels (csrc/hrl_lstm.hip), self-play's state advance
(hrl_masked_rows_copy) and the output masking (hrl_output_mask_forward/backward).

Every operation has two plain references written here from the formulas (no project Function or kernel in them):

(a) fp64: the torch expression in float64, gradients by autograd through it;
(b) fp32 mirror: the same expression in float32 on the CPU in the kernels' stated operation order -- (1 - m)
    first, every product its own rounded tensor, the sum over players an explicit left-to-right loop over p, the
    adjoints written out (dH = g (1 - m); dnh = sum_p g m; an addend added as e + t).

The hidden, masked-rows and output-mask kernels must equal (b) bit for bit (the build has no fp contraction) and
lie within k * 2^-24 * sum|terms| of (a) elementwise, k = 2P + 2: no element's path has more float operations
than that (the longest, the fused update+gather, has 1 - m, two products' worth of depth, the add, the product
with the next mask and P - 1 adds: P + 3 roundings), and sum|terms| is (a) evaluated on the absolute values of its
inputs (every coefficient m, 1 - m is >= 0, so that is the sum of the terms' magnitudes).

The LSTM kernels run device expf/tanhf, so they are held to (a) by the error of the fp32 torch formulation of
the cell on the CPU on the same inputs: per output tensor, in max-abs norm,
err_kernel <= 4 * err_fp32_torch + 2^-23 * max|ref| (device transcendentals are allowed a couple of ulps where
host libm gives one or fewer, and the backward chains several).  Observed on the first MI355X run (max over the
cases of each test, err_kernel / err_fp32_torch):

    test                      tensor   err_kernel / err_fp32_torch
    hidden unroll (T = 3)     state    3.63e-07 / 3.63e-07     w.grad  1.20e-06 / 1.04e-06
    forward / backward        h        1.49e-07 / 1.49e-07     c       3.29e-07 / 3.29e-07
                              gates    8.62e-08 / 8.61e-08     dz      3.78e-07 / 3.78e-07
                              dc       5.17e-07 / 5.17e-07
    forward with bias         h        1.57e-07 / 1.57e-07     c       3.40e-07 / 3.40e-07
                              gates    1.46e-07 / 1.21e-07
    nn.lstm_gates             h        1.27e-07 / 1.21e-07     c       3.10e-07 / 3.10e-07
                              dz       3.81e-07 / 2.84e-07     dc      2.73e-07 / 2.73e-07
    forward_grouped           h        1.63e-07 / 1.45e-07     c       3.64e-07 / 3.64e-07
                              gates    9.26e-08 / 9.26e-08
    backward_ex               dz       5.47e-07 / 5.47e-07     dc      3.65e-07 / 3.65e-07
    grid-stride (N = 700000)  h        1.87e-07 / 1.87e-07     c       5.56e-07 / 5.56e-07
                              gates    8.71e-08 / 8.71e-08     dz      7.85e-07 / 5.96e-07
                              dc       6.08e-07 / 6.08e-07

The kernel's error never exceeded 0.29 of its bound: both are dominated by the fp32 rounding of the results.

Which case launches which template instantiation (<4>: every F, stride % 4 == 0 and pointer 16-byte aligned):

    hrl_hidden.hip, test_hidden_functions ids (every case runs all three Functions, forward and backward)
      gather_sum<4> / gather_keep<4>        *-sum-board-* / *-keep-board-*, *-vec4-*-pad4-*
      gather_sum<1> / gather_keep<1>        *-sum-odd-*, *-sum-mixed-* / *-keep-odd-*, *-keep-mixed-*, *-off
      gather_bwd, update, update_bwd,       <4>: *-board-*, *-vec4-*-pad4-*, *-rows4-*,
      update_gather, update_gather_bwd           test_hidden_adjoint_entry_points[True]
                                            <1>: *-odd-*, *-mixed-*, *-vec4-*-pad3-*, *-off, *-rows3-*, *-sixteen-*,
                                                 test_hidden_adjoint_entry_points[False]
      update_gather_bwd, g == NULL          <4>: *-vec4-*-pad4-* (leaf 2), *-board-*-r2; <1>: *-mixed-* (leaf 2)
    hrl_lstm.hip
      lstm_fwd<4> / lstm_bwd<4>             test_lstm_forward_backward_vs_fp64[36-slice], [36-none]
      lstm_fwd<1> / lstm_bwd<1>             [36-slice_odd_stride] (forward), [15-*], [1-*], test_lstm_grid_stride_loop
      lstm_fwd_grouped<4> / <1>             test_lstm_forward_grouped[*-36-8] / [*-36-3], [*-15-*]
      lstm_bwd_ex<4> / <1>                  test_lstm_backward_ex[*-36] / [*-15]
"""

import pytest
import torch

from handyrl_amd import _native

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


# ------------------------------------------------------------------ shared helpers

def _masks(gen, B, P, kind):
    """(B, P) masks: 'frac' real values in [0, 1] (only these can expose a fused or reordered operation: with 0/1
    every product is exact); 'bin' 0/1 with an all-zero first and an all-one last row."""
    if kind == 'frac':
        return torch.rand(B, P, generator=gen)
    m = (torch.rand(B, P, generator=gen) > 0.5).float()
    m[0] = 0.0
    m[-1] = 1.0 if B > 1 else m[-1]
    return m


def _bview(m, t):
    """(B, P) mask broadcastable against t (B, P, *shape)."""
    return m.view(*m.shape, *([1] * (t.dim() - 2)))


def _check(got, mirror, ref64, mag64, k, what):
    """got (device fp32) is the mirror bit for bit and within k 2^-24 sum|terms| of the fp64 reference."""
    got = got.detach().cpu()
    assert got.shape == mirror.shape, (what, got.shape, mirror.shape)
    assert torch.equal(got, mirror), (what, 'differs from the fp32 mirror', float((got - mirror).abs().max()))
    err = (got.double() - ref64).abs()
    assert bool((err <= k * EPS * mag64).all()), (what, 'outside the fp64 bound', float(err.max()))


def _grad64(fn, inputs, gouts):
    """outputs of fn on fp64 leaves and d(sum_i <out_i, gout_i>)/d(inputs) by autograd (None: no path)."""
    xs = [x.detach().clone().requires_grad_(True) for x in inputs]
    outs = fn(xs)
    roots = [(o, g) for o, g in zip(outs, gouts) if g is not None]
    grads = [None] * len(xs)
    if roots:
        grads = torch.autograd.grad([o for o, _ in roots], xs, [g for _, g in roots], allow_unused=True)
    return [o.detach() for o in outs], list(grads)


def _on(t, dev, offset=False):
    """t on the device; offset: contiguous but starting 4 bytes into its storage (not 16-byte aligned)."""
    if not offset:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


class _Wide:
    """An upstream gradient that reaches a Function's backward as a channel slice of a wider tensor: the output is
    concatenated with `pad` more channels before the loss, so autograd hands back a narrow view (row stride > F)."""

    def __init__(self, gen, shape, dim, pad):
        self.dim, self.C = dim, shape[dim]
        wide = list(shape)
        wide[dim] += pad
        self.wide = torch.randn(*wide, generator=gen)
        self.other = torch.randn(*shape[:dim], pad, *shape[dim + 1:], generator=gen)
        self.g = self.wide.narrow(dim, 0, self.C).contiguous()     # what the references see
        self.row_stride = int(torch.Size(wide[dim:]).numel())


def _backward_dev(outs, gouts, dev):
    """backward of the device outputs; a _Wide gradient goes through torch.cat so that it arrives strided.
    Returns the strides of the gradients as the Functions received them."""
    roots, gs, seen = [], [], {}
    for i, (o, g) in enumerate(zip(outs, gouts)):
        if g is None:
            continue
        if isinstance(g, _Wide):
            o.register_hook(lambda gr, i=i: seen.__setitem__(i, gr.stride()))
            roots.append(torch.cat([o, g.other.to(dev)], g.dim))
            gs.append(g.wide.to(dev))
        else:
            roots.append(o)
            gs.append(g.to(dev))
    if roots:
        torch.autograd.backward(roots, gs)
    for i, g in enumerate(gouts):
        if isinstance(g, _Wide):
            assert seen[i][g.dim - 1] == g.row_stride, 'the addend did not arrive as a slice of the wider tensor'
    return seen


def _plain(g):
    return g.g if isinstance(g, _Wide) else g


# ------------------------------------------------------------------ 1. hidden-state kernels: references

def ref_gather(H, m, summed):
    """h_in = sum_p h[:, p] m[:, p] (p ascending) or h m with one row per player (train.py:157-164)."""
    outs = []
    for h in H:
        mm = _bview(m, h)
        if summed:
            acc = h[:, 0] * mm[:, 0]
            for p in range(1, h.shape[1]):
                acc = acc + h[:, p] * mm[:, p]
            outs.append(acc)
        else:
            outs.append((h * mm).reshape(-1, *h.shape[2:]))
    return outs


def ref_update(H, NH, m, Pn):
    """h' = h (1 - m) + nh m, nh broadcast over the players when it has one row per game (train.py:167-174)."""
    outs = []
    for h, nh in zip(H, NH):
        mm = _bview(m, h)
        om = 1 - mm
        outs.append(h * om + nh.view(h.shape[0], Pn, *h.shape[2:]) * mm)
    return outs


def mir_gather_bwd(g, e, m, summed, shape):
    """dH = [e +] g m: g the gathered input's gradient ((B or B*P, *s), None: zero), e the state's other gradient."""
    if g is None:
        return e
    B, P = m.shape
    t = g.view(B, 1 if summed else P, *shape[2:]) * m.view(B, P, *([1] * (len(shape) - 2)))
    return t if e is None else e + t


def mir_update_bwd(go, f, m, Pn):
    """dH = go (1 - m); dnh = [f +] sum_p go m (p ascending; nh with one row per game) or [f +] go m."""
    mm = _bview(m, go)
    dH = go * (1 - mm)
    if Pn == 1:
        acc = go[:, 0] * mm[:, 0]
        for p in range(1, go.shape[1]):
            acc = acc + go[:, p] * mm[:, p]
    else:
        acc = (go * mm).reshape(-1, *go.shape[2:])
    return dH, (acc if f is None else f + acc)


SHAPES = {
    'board': [(8, 6, 6)],                                   # F = 288: float4
    'odd': [(3, 5)],                                        # F = 15: the scalar kernels
    'mixed': [(8, 6, 6), (3, 5), (4,), (300, 3, 3)],        # different F, scalar, F = 2700 > 256 * 4: gridDim.x > 1
    'vec4': [(8, 6, 6), (4,), (2, 2, 2), (300, 2, 2)],      # different F, all float4, gridDim.x > 1
    'rows4': [(2, 2)],                                      # small F for the row loop past the 4096-row cap
    'rows3': [(3,)],
    'sixteen': [(1 + (5 * i) % 7,) for i in range(16)],     # kMaxLeaves
}

# what reaches each leaf's backward: (gathered-input gradient, state / new-state gradient)
ROLES = {0: (True, True), 1: (True, False), 2: (False, True), 3: (False, False)}


def _hidden_cases():
    cases, i = [], 0
    for P in (1, 2, 3, 4):
        for pn_is_p in ((False,) if P == 1 else (False, True)):
            for summed in (True, False):
                for key in ('board', 'odd', 'mixed'):
                    kind = 'bin' if i % 3 == 2 else 'frac'
                    out_k = (-1, 0, len(SHAPES[key]) - 1)[i % 3]
                    cases.append(dict(P=P, Pn=P if pn_is_p else 1, summed=summed, key=key, B=5, kind=kind,
                                      pad=(4, 3)[i % 2], out_k=out_k))
                    i += 1
    extra = [
        dict(P=2, Pn=1, summed=True, key='vec4', B=5, kind='frac', pad=4, out_k=0),      # float4 with every role
        dict(P=3, Pn=3, summed=False, key='vec4', B=5, kind='frac', pad=4, out_k=2),
        dict(P=2, Pn=1, summed=True, key='vec4', B=5, kind='frac', pad=3, out_k=0),      # strides % 4 != 0: scalar
        dict(P=2, Pn=1, summed=True, key='board', B=5, kind='frac', pad=4, out_k=0, roles=[2]),   # g == NULL, float4
        dict(P=2, Pn=2, summed=False, key='board', B=5, kind='frac', pad=4, out_k=-1, roles=[1]),
        dict(P=2, Pn=1, summed=True, key='board', B=5, kind='frac', pad=4, out_k=0, offset=True),  # misaligned
        dict(P=3, Pn=3, summed=False, key='vec4', B=5, kind='frac', pad=4, out_k=1, offset=True),
        dict(P=2, Pn=1, summed=True, key='mixed', B=1, kind='frac', pad=4, out_k=0),
        dict(P=4, Pn=4, summed=False, key='board', B=1, kind='bin', pad=4, out_k=-1),
        dict(P=2, Pn=1, summed=True, key='rows4', B=4100, kind='frac', pad=4, out_k=0),   # rows > grid_of's cap
        dict(P=2, Pn=2, summed=False, key='rows4', B=4100, kind='frac', pad=4, out_k=-1),
        dict(P=2, Pn=1, summed=False, key='rows3', B=4100, kind='bin', pad=3, out_k=0),
        dict(P=3, Pn=1, summed=True, key='rows3', B=4100, kind='frac', pad=3, out_k=-1),
        dict(P=3, Pn=1, summed=True, key='sixteen', B=5, kind='frac', pad=3, out_k=15),
        dict(P=2, Pn=2, summed=False, key='sixteen', B=5, kind='bin', pad=4, out_k=4),
    ]
    return cases + extra


def _case_id(c):
    return 'P%d-Pn%d-%s-%s-B%d-%s-pad%d-k%d%s%s' % (
        c['P'], c['Pn'], 'sum' if c['summed'] else 'keep', c['key'], c['B'], c['kind'], c['pad'], c['out_k'],
        '-off' if c.get('offset') else '', '-r%s' % ''.join(map(str, c['roles'])) if 'roles' in c else '')


@pytest.mark.parametrize('case', _hidden_cases(), ids=_case_id)
def test_hidden_functions(cuda, case):
    """_HiddenGather, _HiddenUpdate and _HiddenUpdateGather, forward and every gradient (the pass-through alias
    outputs' included, as channel slices of wider tensors), against the mirror bit for bit and the fp64 bound;
    leaves without a gradient stay None; the fused Function equals update-then-gather bit for bit."""
    from handyrl_amd.nn import _HiddenGather, _HiddenUpdate, _HiddenUpdateGather
    P, Pn, summed, B, out_k = case['P'], case['Pn'], case['summed'], case['B'], case['out_k']
    shapes = SHAPES[case['key']]
    n = len(shapes)
    roles = case.get('roles', [l % 4 for l in range(n)])
    off = case.get('offset', False)
    k = 2 * P + 2
    gen = torch.Generator().manual_seed(1000 * P + 10 * n + B % 7)
    m, mn = _masks(gen, B, P, case['kind']), _masks(gen, B, P, case['kind'])
    H = [torch.randn(B, P, *s, generator=gen) for s in shapes]          # non-zero initial state
    NH = [torch.randn(B * Pn, *s, generator=gen) for s in shapes]
    rows = B if summed else B * P
    GG = [torch.randn(rows, *s, generator=gen) if ROLES[r][0] else None for s, r in zip(shapes, roles)]
    GS = [_Wide(gen, (B, P, *s), 2, case['pad']) if ROLES[r][1] else None for s, r in zip(shapes, roles)]
    GO = [torch.randn(B, P, *s, generator=gen) if ROLES[r][1] else None for s, r in zip(shapes, roles)]
    GK = _Wide(gen, (B * Pn, *shapes[out_k]), 1, case['pad']) if out_k >= 0 else None
    md, mnd = m.to(cuda), mn.to(cuda)
    d64 = lambda ts: [t.double() for t in ts]                                   # noqa: E731
    a64 = lambda ts: [None if t is None else _plain(t).double().abs() for t in ts]   # noqa: E731
    g64 = lambda ts: [None if t is None else _plain(t).double() for t in ts]    # noqa: E731

    def compare(what, fn, inputs, gouts, dev_outs, dev_inputs, mir_grads, m_list):
        """forward outputs and input gradients of one Function against the mirror and the fp64 bound"""
        with torch.no_grad():
            mir_outs = fn(inputs, *m_list)
        ref_outs, ref_grads = _grad64(lambda xs: fn(xs, *d64(m_list)), d64(inputs), g64(gouts))
        mag_outs, mag_grads = _grad64(lambda xs: fn(xs, *d64(m_list)), [x.double().abs() for x in inputs],
                                      a64(gouts))
        assert len(dev_outs) == len(mir_outs)
        for i, o in enumerate(dev_outs):
            _check(o, mir_outs[i], ref_outs[i], mag_outs[i], k, (what, 'output', i))
        for i, x in enumerate(dev_inputs):
            if mir_grads[i] is None:
                assert x.grad is None and ref_grads[i] is None, (what, 'a pruned leaf got a gradient', i)
            else:
                assert x.grad is not None, (what, 'gradient missing', i)
                _check(x.grad, mir_grads[i], ref_grads[i], mag_grads[i], k, (what, 'gradient', i))

    # ---- gather
    def f_gather(xs, mask):
        return ref_gather(xs, mask, summed) + [x.view_as(x) for x in xs]

    Hd = [_on(h, cuda, off).requires_grad_(True) for h in H]
    outs = _HiddenGather.apply(md, summed, B, P, *Hd)
    _backward_dev(outs, GG + GS, cuda)
    compare('gather', f_gather, H, GG + GS, outs, Hd,
            [mir_gather_bwd(GG[l], None if GS[l] is None else GS[l].g, m, summed, H[l].shape) for l in range(n)],
            [m])

    # ---- update
    def f_update(xs, mask):
        res = ref_update(xs[:n], xs[n:], mask, Pn)
        return res + ([xs[n + out_k].view_as(xs[n + out_k])] if out_k >= 0 else [])

    gouts = GO + ([GK] if out_k >= 0 else [])
    Hd = [_on(h, cuda, off).requires_grad_(True) for h in H]
    NHd = [_on(x, cuda, off).requires_grad_(True) for x in NH]
    outs = _HiddenUpdate.apply(md, B, P, Pn, n, out_k, *Hd, *NHd)
    _backward_dev(outs, gouts, cuda)
    mir = [(None, None) if GO[l] is None else
           mir_update_bwd(GO[l], GK.g if l == out_k else None, m, Pn) for l in range(n)]
    if out_k >= 0 and GO[out_k] is None:
        mir[out_k] = (None, GK.g)
    compare('update', f_update, H + NH, gouts, outs, Hd + NHd, [x[0] for x in mir] + [x[1] for x in mir], [m])

    # ---- update + gather fused, and the two Functions in sequence
    def f_fused(xs, mask, mask_next):
        st = ref_update(xs[:n], xs[n:], mask, Pn)
        return (ref_gather(st, mask_next, summed) + [s.view_as(s) for s in st]
                + ([xs[n + out_k].view_as(xs[n + out_k])] if out_k >= 0 else []))

    gouts = GG + GS + ([GK] if out_k >= 0 else [])
    Hd = [_on(h, cuda, off).requires_grad_(True) for h in H]
    NHd = [_on(x, cuda, off).requires_grad_(True) for x in NH]
    fused = _HiddenUpdateGather.apply(md, mnd, summed, B, P, Pn, n, out_k, *Hd, *NHd)
    _backward_dev(fused, gouts, cuda)
    mir = []
    for l in range(n):
        go = mir_gather_bwd(GG[l], None if GS[l] is None else GS[l].g, mn, summed, H[l].shape)
        if go is None:
            mir.append((None, GK.g if l == out_k else None))
        else:
            mir.append(mir_update_bwd(go, GK.g if l == out_k else None, m, Pn))
    compare('update_gather', f_fused, H + NH, gouts, fused, Hd + NHd, [x[0] for x in mir] + [x[1] for x in mir],
            [m, mn])

    H2 = [_on(h, cuda, off).requires_grad_(True) for h in H]
    NH2 = [_on(x, cuda, off).requires_grad_(True) for x in NH]
    u = _HiddenUpdate.apply(md, B, P, Pn, n, out_k, *H2, *NH2)
    g = _HiddenGather.apply(mnd, summed, B, P, *u[:n])
    two = tuple(g) + ((u[n],) if out_k >= 0 else ())
    _backward_dev(two, gouts, cuda)
    for i, (a, b) in enumerate(zip(fused, two)):
        assert torch.equal(a, b), ('fused vs update then gather: output', i)
    for i, (a, b) in enumerate(zip(Hd + NHd, H2 + NH2)):
        assert (a.grad is None) == (b.grad is None), ('fused vs update then gather: pruning', i)
        assert a.grad is None or torch.equal(a.grad, b.grad), ('fused vs update then gather: gradient', i)


@pytest.mark.parametrize('vec', [True, False])
def test_hidden_adjoint_entry_points(cuda, vec):
    """The C adjoints called directly: the plain wrappers (no addend) and the _add / fused forms with explicit
    addend row strides (a channel slice of a wider buffer; vec: strides % 4 == 0, else not) and, in the fused
    adjoint, a NULL gathered-input gradient next to a given one."""
    lib = _native.load()
    B, P, F = 6, 3, [8, 20]
    pad = 4 if vec else 3
    gen = torch.Generator().manual_seed(5 + vec)
    m, mn = torch.rand(B, P, generator=gen), torch.rand(B, P, generator=gen)
    k = 2 * P + 2
    s = _native.stream_of(cuda)
    ia, pa, p = _native.i64_array, _native.ptr_array, _native.ptr
    md, mnd = m.to(cuda), mn.to(cuda)
    for summed, Pn in ((True, 1), (False, P)):
        rows = B if summed else B * P
        g = [torch.randn(rows, f, generator=gen) for f in F]
        go = [torch.randn(B, P, f, generator=gen) for f in F]
        ew = [torch.randn(B * P, f + pad, generator=gen) for f in F]      # state-gradient addends, strided
        fw = [torch.randn(B * Pn, f + pad, generator=gen) for f in F]     # step-output addends, strided
        e = [w[:, :f].reshape(B, P, f) for w, f in zip(ew, F)]
        fa = [w[:, :f].contiguous() for w, f in zip(fw, F)]
        gd, god, ewd, fwd = ([t.to(cuda) for t in ts] for ts in (g, go, ew, fw))
        new = lambda r: [torch.full((r, f), float('nan'), device=cuda) for f in F]   # noqa: E731
        st = ia([f + pad for f in F])

        def bound(got, mirror, fn64, args, what):
            ref = fn64(*[None if a is None else a.double() for a in args])
            mag = fn64(*[None if a is None else a.double().abs() for a in args])
            _check(got.view(mirror.shape), mirror, ref, mag, k, what)

        # hrl_hidden_gather_backward (no addend) and _add with a stride
        d0, d1 = new(B * P), new(B * P)
        assert lib.hrl_hidden_gather_backward(pa(gd), p(md), B, P, 2, ia(F), int(summed), pa(d0), s) == 0
        assert lib.hrl_hidden_gather_backward_add(pa(gd), p(md), B, P, 2, ia(F), int(summed), pa(ewd), st, pa(d1),
                                                  s) == 0
        for l in range(2):
            shape = (B, P, F[l])
            bound(d0[l], mir_gather_bwd(g[l], None, m, summed, shape),
                  lambda a, mm: mir_gather_bwd(a, None, mm, summed, shape), (g[l], m), ('gather_backward', l))
            bound(d1[l], mir_gather_bwd(g[l], e[l], m, summed, shape),
                  lambda a, b, mm: mir_gather_bwd(a, b, mm, summed, shape), (g[l], e[l], m),
                  ('gather_backward_add', l))
        # hrl_hidden_update_backward and _add (only leaf 1 has an addend)
        a0, b0, a1, b1 = new(B * P), new(B * Pn), new(B * P), new(B * Pn)
        assert lib.hrl_hidden_update_backward(pa(god), p(md), B, P, Pn, 2, ia(F), pa(a0), pa(b0), s) == 0
        assert lib.hrl_hidden_update_backward_add(pa(god), p(md), B, P, Pn, 2, ia(F), pa([None, fwd[1]]), st,
                                                  pa(a1), pa(b1), s) == 0
        for l in range(2):
            for add, (da, db) in ((None, (a0, b0)), (fa[l] if l == 1 else None, (a1, b1))):
                mir = mir_update_bwd(go[l], add, m, Pn)
                for j, (got, name) in enumerate(((da[l], 'dH'), (db[l], 'dnh'))):
                    bound(got, mir[j], lambda a, b, mm, j=j: mir_update_bwd(a, b, mm, Pn)[j], (go[l], add, m),
                          ('update_backward', name, l))
        # hrl_hidden_update_gather_backward: leaf 0 has no gathered-input gradient (NULL), leaf 1 has both
        a2, b2 = new(B * P), new(B * Pn)
        assert lib.hrl_hidden_update_gather_backward(
            pa([None, gd[1]]), p(md), p(mnd), B, P, Pn, 2, ia(F), int(summed), pa(ewd), st, pa([fwd[0], None]), st,
            pa(a2), pa(b2), s) == 0
        for l in range(2):
            args = (None if l == 0 else g[l], e[l], fa[l] if l == 0 else None, m, mn)

            def chain(gg, ee, ff, mm, mmn, l=l):
                return mir_update_bwd(mir_gather_bwd(gg, ee, mmn, summed, (B, P, F[l])), ff, mm, Pn)
            mir = chain(*args)
            for j, (got, name) in enumerate(((a2[l], 'dH'), (b2[l], 'dnh'))):
                bound(got, mir[j], lambda *xs, j=j: chain(*xs)[j], args, ('update_gather_backward', name, l))


def _lstm_tolerance(name, got, ref64, t32, record=None):
    """err_kernel <= 4 err_fp32_torch + 2^-23 max|ref| in max-abs norm; prints both errors."""
    got = got.detach()
    assert bool(torch.isfinite(got).all()), (name, 'not finite')
    err_k = float((got.double() - ref64.to(got.device)).abs().max())
    err_t = float((t32.double() - ref64.to(t32.device)).abs().max())
    top = float(ref64.abs().max())
    print('LSTMERR %s err_kernel %.3e err_fp32_torch %.3e max|ref| %.3e' % (name, err_k, err_t, top))
    if record is not None:
        record.append((name, err_k, err_t, top))
        return
    assert err_k <= 4 * err_t + 2.0 ** -23 * top, (name, err_k, err_t, top)


@pytest.mark.parametrize('fuse', [False, True])
@pytest.mark.parametrize('summed', [True, False])
def test_hidden_unroll_t3(cuda, summed, fuse):
    """A T = 3 unroll as train._unroll_flat_hidden chains the Functions -- gather, a toy step nh = tanh(h_in w),
    update -- with and without the fused update+gather, against the torch formulation of train.py:155-174 in
    fp64: the final state and w.grad.  tanh is a transcendental, so the bound is the LSTM tests' (the fp32 torch
    formulation's own error on the CPU); w has one weight per state element, so no gradient is a long sum."""
    from handyrl_amd.nn import _HiddenGather, _HiddenUpdate, _HiddenUpdateGather
    B, P, T = 5, 3, 3
    shapes = [(8, 6, 6), (3, 5), (4,)]
    n = len(shapes)
    Pn = 1 if summed else P
    gen = torch.Generator().manual_seed(77)
    masks = torch.rand(T, B, P, generator=gen)
    masks[1] = (masks[1] > 0.5).float()
    H0 = [torch.randn(B, P, *s, generator=gen) for s in shapes]
    W = [torch.randn(B * Pn, *s, generator=gen) for s in shapes]
    R = [torch.randn(B, P, *s, generator=gen) for s in shapes]

    def torch_unroll(dt):
        hidden = [h.to(dt) for h in H0]
        w = [x.detach().clone().to(dt).requires_grad_(True) for x in W]
        for t in range(T):
            nxt = []
            for l, h in enumerate(hidden):
                om = _bview(masks[t].to(dt), h)
                h_in = h * om
                h_in = h_in.sum(1) if summed else h_in.reshape(-1, *h.shape[2:])
                nh = torch.tanh(h_in * w[l]).view(B, -1, *h.shape[2:])
                nxt.append(h * (1 - om) + nh * om)
            hidden = nxt
        torch.autograd.backward(hidden, [r.to(dt) for r in R])
        return [h.detach() for h in hidden], [x.grad for x in w]

    md = masks.to(cuda)
    w = [x.detach().clone().to(cuda).requires_grad_(True) for x in W]
    g = _HiddenGather.apply(md[0], summed, B, P, *[h.to(cuda) for h in H0])
    for t in range(T):
        nh = [torch.tanh(g[l] * w[l]) for l in range(n)]
        if fuse and t + 1 < T:
            g = _HiddenUpdateGather.apply(md[t], md[t + 1], summed, B, P, Pn, n, -1, *g[n:], *nh)[:2 * n]
            continue
        leaves = list(_HiddenUpdate.apply(md[t], B, P, Pn, n, -1, *g[n:], *nh))
        if t + 1 < T:
            g = _HiddenGather.apply(md[t + 1], summed, B, P, *leaves)
    torch.autograd.backward(leaves, [r.to(cuda) for r in R])

    (s64, g64), (s32, g32) = torch_unroll(torch.float64), torch_unroll(torch.float32)
    for l in range(n):
        _lstm_tolerance('unroll state %d' % l, leaves[l].cpu(), s64[l], s32[l])
        _lstm_tolerance('unroll w.grad %d' % l, w[l].grad.cpu(), g64[l], g32[l])


# ------------------------------------------------------------------ 2. LSTM gate kernels

def ref_cell(zx, zh, c, bias=None):
    """The ConvLSTM cell tail on (N, 4H, HW) pre-activations in gate order i, f, o, g: z = [(zx [+ bias]) +] zh;
    c' = sigmoid(f) c + sigmoid(i) tanh(g); h' = sigmoid(o) tanh(c').  bias: (N, 4H), each sample's row."""
    if zx is None:
        z = zh
    elif bias is None:
        z = zx + zh
    else:
        z = (zx + bias[:, :, None]) + zh
    i, f, o, g = z.chunk(4, 1)
    si, sf, so, tg = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
    c2 = sf * c + si * tg
    return so * torch.tanh(c2), c2, torch.cat([si, sf, so, tg], 1)


def ref_cell_grads(dt, zx, zh, c, bias, dh, dc_out, dev=None):
    """(h', c', gates, dz, dc) of ref_cell in dtype dt, gradients by autograd (dh / dc_out None: zero)."""
    cv = lambda t: None if t is None else t.detach().to(device=dev or t.device, dtype=dt)   # noqa: E731
    zh_, c_ = cv(zh).requires_grad_(True), cv(c).requires_grad_(True)
    h2, c2, gates = ref_cell(cv(zx), zh_, c_, cv(bias))
    roots = [(o, cv(g)) for o, g in ((h2, dh), (c2, dc_out)) if g is not None]
    dz = dc = None
    if roots:
        dz, dc = torch.autograd.grad([o for o, _ in roots], [zh_, c_], [g for _, g in roots])
    return h2.detach(), c2.detach(), gates.detach(), dz, dc


def _lstm_inputs(gen, N, H, HW, saturate=True):
    zh = torch.randn(N, 4 * H, HW, generator=gen)
    if saturate:    # some gates saturated: pre-activations at +-100
        hit = torch.rand(N, 4 * H, HW, generator=gen)
        zh = torch.where(hit < 0.03, torch.full_like(zh, 100.0), zh)
        zh = torch.where(hit > 0.97, torch.full_like(zh, -100.0), zh)
    return zh, torch.randn(N, H, HW, generator=gen)


def _slice_of_wider(t, dev, before, after, lead=1):
    """t on the device as columns [before, before + row) of a wider (rows, before + row + after) buffer: the same
    values, rows `before + row + after` floats apart."""
    rows = int(torch.Size(t.shape[:lead]).numel())
    row = t.numel() // rows
    buf = torch.randn(rows, before + row + after, device=dev)
    v = buf[:, before:before + row]
    v.copy_(t.reshape(rows, row))
    return v, before + row + after


def k_lstm_forward(zx, zx_stride, zh, c, bias=None, bias_rows=1, gates=True, c_out=None):
    lib, p = _native.load(), _native.ptr
    N, G, HW = zh.shape
    h = torch.full_like(c, float('nan'))
    c2 = torch.full_like(c, float('nan')) if c_out is None else c_out
    ga = torch.full_like(zh, float('nan')) if gates else None
    rc = lib.hrl_lstm_gates_forward(p(zx), zx_stride, p(zh), p(c), N, G // 4, HW, p(bias), bias_rows, p(h), p(c2),
                                    p(ga), _native.stream_of(zh.device))
    assert rc == 0, rc
    return h, c2, ga


def k_lstm_backward(gates, c, c_out, dh, dc_out):
    lib, p = _native.load(), _native.ptr
    N, G, HW = gates.shape
    dz, dc = torch.full_like(gates, float('nan')), torch.full_like(c, float('nan'))
    rc = lib.hrl_lstm_gates_backward(p(gates), p(c), p(c_out), p(dh), p(dc_out), N, G // 4, HW, p(dz), p(dc),
                                     _native.stream_of(gates.device))
    assert rc == 0, rc
    return dz, dc


@pytest.mark.parametrize('zx_form', ['slice', 'slice_odd_stride', 'none'])
@pytest.mark.parametrize('HW', [36, 15, 1])
def test_lstm_forward_backward_vs_fp64(cuda, HW, zx_form):
    """hrl_lstm_gates_forward with zx a channel slice (row stride % 4 == 0 or not) or NULL, the inference forms
    (bias rows 1 and 3 with N % 3 != 0, gates NULL, c_out aliasing c), and hrl_lstm_gates_backward from the saved
    gates with dh / dc_out given or NULL, against the fp64 cell."""
    N, H = 37, 8
    gen = torch.Generator().manual_seed(HW)
    zh, c = _lstm_inputs(gen, N, H, HW)
    zx = None if zx_form == 'none' else torch.randn(N, 4 * H, HW, generator=gen)
    zxd, stride = None, 0
    if zx is not None:
        zxd, stride = _slice_of_wider(zx, cuda, 8 * HW, 4 * HW if zx_form == 'slice' else 4 * HW + 3)
    zhd, cd = zh.to(cuda), c.to(cuda)
    dh, dc_out = torch.randn(N, H, HW, generator=gen), torch.randn(N, H, HW, generator=gen)
    tag = 'fwd/bwd HW%d %s' % (HW, zx_form)
    h2, c2, ga = k_lstm_forward(zxd, stride, zhd, cd)
    for use_dh, use_dc in ((True, True), (True, False), (False, True)):
        a, b = (dh if use_dh else None), (dc_out if use_dc else None)
        r64, r32 = ref_cell_grads(torch.float64, zx, zh, c, None, a, b), \
            ref_cell_grads(torch.float32, zx, zh, c, None, a, b)
        dz, dc = k_lstm_backward(ga, cd, c2, None if a is None else a.to(cuda), None if b is None else b.to(cuda))
        for name, got, i in (('h', h2, 0), ('c', c2, 1), ('gates', ga, 2), ('dz', dz, 3), ('dc', dc, 4)):
            _lstm_tolerance('%s %s dh%d dc%d' % (tag, name, use_dh, use_dc), got.cpu(), r64[i], r32[i])
    # inference forms
    h3, c3, none = k_lstm_forward(zxd, stride, zhd, cd, gates=False)
    assert none is None and torch.equal(h3, h2) and torch.equal(c3, c2)
    if zx is None:
        return
    for rows in (1, 3):
        bias = torch.randn(rows, 4 * H, generator=gen)
        per_sample = bias[torch.arange(N) % rows]
        r64 = ref_cell(zx.double(), zh.double(), c.double(), per_sample.double())
        r32 = ref_cell(zx, zh, c, per_sample)
        hb, cb, gb = k_lstm_forward(zxd, stride, zhd, cd, bias.to(cuda), rows, gates=True)
        for name, got, i in (('h', hb, 0), ('c', cb, 1), ('gates', gb, 2)):
            _lstm_tolerance('%s bias_rows%d %s' % (tag, rows, name), got.cpu(), r64[i], r32[i])
        alias = cd.clone()      # c_out is c itself: each element is read, then written
        ha, ca, _ = k_lstm_forward(zxd, stride, zhd, alias, bias.to(cuda), rows, gates=False, c_out=alias)
        assert ca is alias and torch.equal(ha, hb) and torch.equal(alias, cb)


def test_lstm_gates_function_forms(cuda):
    """nn.lstm_gates: zx None with autograd, and the inference forms bias (3 rows) and out=(h, c) with c_out being
    c, against the fp64 cell."""
    from handyrl_amd.nn import lstm_gates
    N, H, hw = 37, 8, (3, 5)
    HW = hw[0] * hw[1]
    gen = torch.Generator().manual_seed(3)
    zh, c = _lstm_inputs(gen, N, H, HW)
    zx = torch.randn(N, 4 * H, HW, generator=gen)
    dh, dc_out = torch.randn(N, H, HW, generator=gen), torch.randn(N, H, HW, generator=gen)
    v4 = lambda t: t.view(t.shape[0], t.shape[1], *hw)   # noqa: E731
    zhd, cd = v4(zh).to(cuda).requires_grad_(True), v4(c).to(cuda).requires_grad_(True)
    h2, c2 = lstm_gates(None, zhd, cd)
    torch.autograd.backward([h2, c2], [v4(dh).to(cuda), v4(dc_out).to(cuda)])
    r64 = ref_cell_grads(torch.float64, None, zh, c, None, dh, dc_out)
    r32 = ref_cell_grads(torch.float32, None, zh, c, None, dh, dc_out)
    for name, got, i in (('h', h2, 0), ('c', c2, 1), ('dz', zhd.grad, 3), ('dc', cd.grad, 4)):
        _lstm_tolerance('function zx=None %s' % name, got.detach().cpu().flatten(2), r64[i], r32[i])
    bias = torch.randn(3, 4 * H, generator=gen)
    per_sample = bias[torch.arange(N) % 3]
    r64 = ref_cell(zx.double(), zh.double(), c.double(), per_sample.double())
    r32 = ref_cell(zx, zh, c, per_sample)
    wide = torch.randn(N, 12 * H, *hw, device=cuda)
    wide[:, 4 * H:8 * H] = v4(zx).to(cuda)
    state = v4(c).to(cuda)
    h_buf = torch.empty_like(state)
    with torch.no_grad():
        h3, c3 = lstm_gates(wide[:, 4 * H:8 * H], v4(zh).to(cuda), state, bias=bias.to(cuda), bias_rows=3,
                            out=(h_buf, state))
    assert h3.data_ptr() == h_buf.data_ptr() and c3.data_ptr() == state.data_ptr()
    _lstm_tolerance('function bias out= h', h_buf.cpu().flatten(2), r64[0], r32[0])
    _lstm_tolerance('function bias out= c', state.cpu().flatten(2), r64[1], r32[1])
    with pytest.raises(ValueError):
        lstm_gates(None, zhd, cd, out=(h_buf, state))      # inference-only form with gradients enabled


@pytest.mark.parametrize('extra', [8, 3])
@pytest.mark.parametrize('HW', [36, 15])
@pytest.mark.parametrize('L', [1, 3, 4])
def test_lstm_forward_grouped(cuda, L, HW, extra):
    """hrl_lstm_gates_forward_grouped: zh a slice of a wider buffer (zh_stride > L 4H HW; extra = 3: not a
    multiple of 4, the scalar kernel at HW = 36 too), per-layer zx strides that differ, gates[l] NULL for one
    layer: equal to L separate hrl_lstm_gates_forward calls bit for bit, each layer within the fp64 bound."""
    lib, p, pa = _native.load(), _native.ptr, _native.ptr_array
    N, H = 11, 8
    G = 4 * H
    gen = torch.Generator().manual_seed(10 * L + HW)
    zh, c, zx = [], [], []
    for l in range(L):
        a, b = _lstm_inputs(gen, N, H, HW)
        zh.append(a)
        c.append(b)
        zx.append(torch.randn(N, G, HW, generator=gen))
    zh_all, zh_stride = _slice_of_wider(torch.cat(zh, 1), cuda, 4 * HW, extra)
    assert zh_stride > L * G * HW
    zxd = [_slice_of_wider(zx[l], cuda, 4 * HW * l, 4 * HW * (l + 1)) for l in range(L)]
    assert L == 1 or len({st for _, st in zxd}) == L
    cd = [x.to(cuda) for x in c]
    nan = lambda t: torch.full(t.shape, float('nan'), device=cuda)   # noqa: E731
    h_out, c_out = [nan(x) for x in c], [nan(x) for x in c]
    skip = 1 if L > 1 else -1           # this layer saves no gates
    gates = [None if l == skip else nan(zh[l]) for l in range(L)]
    rc = lib.hrl_lstm_gates_forward_grouped(L, p(zh_all), zh_stride, pa([v for v, _ in zxd]),
                                            _native.i64_array([st for _, st in zxd]), pa(cd), N, H, HW, pa(h_out),
                                            pa(c_out), pa(gates), _native.stream_of(cuda))
    assert rc == 0, rc
    for l in range(L):
        zh_l = zh_all[:, l * G * HW:(l + 1) * G * HW].contiguous().view(N, G, HW)
        h1, c1, g1 = k_lstm_forward(zxd[l][0], zxd[l][1], zh_l, cd[l])
        assert torch.equal(h_out[l], h1) and torch.equal(c_out[l], c1), l
        assert gates[l] is None or torch.equal(gates[l], g1), l
        r64 = ref_cell(zx[l].double(), zh[l].double(), c[l].double())
        r32 = ref_cell(zx[l], zh[l], c[l])
        for name, got, i in (('h', h_out[l], 0), ('c', c_out[l], 1), ('gates', gates[l], 2)):
            if got is not None:
                _lstm_tolerance('grouped L%d HW%d extra%d layer%d %s' % (L, HW, extra, l, name), got.cpu(), r64[i],
                                r32[i])


@pytest.mark.parametrize('HW', [36, 15])
@pytest.mark.parametrize('S', [1, 4])
def test_lstm_backward_ex(cuda, S, HW):
    """hrl_lstm_gates_backward_ex: dh the sum of S partials (dh_stride = S H HW, dh_part_stride = H HW), dh or
    dc_out NULL, dzx initialised by the first call and accumulated by two more: dz and dc equal
    hrl_lstm_gates_backward on the dh summed left to right in fp32 bit for bit and pass the fp64 bound; dzx is
    (dz1 + dz2) + dz3 bit for bit."""
    lib, p = _native.load(), _native.ptr
    N, H = 13, 8
    gen = torch.Generator().manual_seed(S * 100 + HW)
    zh, c = _lstm_inputs(gen, N, H, HW)
    zhd, cd = zh.to(cuda), c.to(cuda)
    _, c2, ga = k_lstm_forward(None, 0, zhd, cd)
    dzx = torch.full_like(ga, float('nan'))
    dzs = []
    for call, (use_dh, use_dc) in enumerate(((True, True), (False, True), (True, False))):
        parts = torch.randn(N, S, H, HW, generator=gen)
        dc_out = torch.randn(N, H, HW, generator=gen)
        dh = parts[:, 0].clone()
        for sp in range(1, S):
            dh = dh + parts[:, sp]
        dh, dc_out = (dh if use_dh else None), (dc_out if use_dc else None)
        pd = parts.to(cuda)
        dhd, dcd = (None if t is None else t.to(cuda) for t in (dh, dc_out))
        dz, dc = torch.full_like(ga, float('nan')), torch.full_like(cd, float('nan'))
        rc = lib.hrl_lstm_gates_backward_ex(p(ga), p(cd), p(c2), p(pd) if use_dh else None, S * H * HW, S, H * HW,
                                            p(dcd), N, H, HW, p(dz), p(dc), p(dzx), int(call == 0),
                                            _native.stream_of(cuda))
        assert rc == 0, rc
        dz0, dc0 = k_lstm_backward(ga, cd, c2, dhd, dcd)
        assert torch.equal(dz, dz0) and torch.equal(dc, dc0), (call, 'differs from hrl_lstm_gates_backward')
        r64 = ref_cell_grads(torch.float64, None, zh, c, None, dh, dc_out)
        r32 = ref_cell_grads(torch.float32, None, zh, c, None, dh, dc_out)
        _lstm_tolerance('backward_ex S%d HW%d call%d dz' % (S, HW, call), dz.cpu(), r64[3], r32[3])
        _lstm_tolerance('backward_ex S%d HW%d call%d dc' % (S, HW, call), dc.cpu(), r64[4], r32[4])
        dzs.append(dz.clone())
    assert torch.equal(dzx, (dzs[0] + dzs[1]) + dzs[2])


def test_lstm_grid_stride_loop(cuda):
    """N = 700000, H = 8, HW = 3: 16.8 M work items on the scalar kernels, more than the 65536 x 256 threads of
    the largest grid, so the grid-stride loops of hrl_lstm_gates_forward / _backward take a second trip.  The
    fp64 cell runs on the device, the fp32 torch formulation on the CPU, both in chunks of samples."""
    N, H, HW, chunk = 700000, 8, 3, 100000
    assert N * H * HW > 65536 * 256
    gen = torch.Generator(device=cuda).manual_seed(9)
    zh = torch.randn(N, 4 * H, HW, device=cuda, generator=gen)
    hit = torch.rand(N, 4 * H, HW, device=cuda, generator=gen)
    zh = torch.where(hit < 0.03, torch.full_like(zh, 100.0), zh)
    zh = torch.where(hit > 0.97, torch.full_like(zh, -100.0), zh)
    del hit
    c = torch.randn(N, H, HW, device=cuda, generator=gen)
    dh = torch.randn(N, H, HW, device=cuda, generator=gen)
    dc_out = torch.randn(N, H, HW, device=cuda, generator=gen)
    h2, c2, ga = k_lstm_forward(None, 0, zh, c)
    dz, dc = k_lstm_backward(ga, c, c2, dh, dc_out)
    names = ('h', 'c', 'gates', 'dz', 'dc')
    worst = {k: [0.0, 0.0, 0.0] for k in names}
    for a in range(0, N, chunk):
        sl = slice(a, a + chunk)
        r64 = ref_cell_grads(torch.float64, None, zh[sl], c[sl], None, dh[sl], dc_out[sl])
        r32 = ref_cell_grads(torch.float32, None, zh[sl].cpu(), c[sl].cpu(), None, dh[sl].cpu(), dc_out[sl].cpu())
        for i, (name, got) in enumerate(zip(names, (h2, c2, ga, dz, dc))):
            rec = []
            _lstm_tolerance('big %s [%d:]' % (name, a), got[sl], r64[i], r32[i].to(cuda), record=rec)
            worst[name] = [max(x, y) for x, y in zip(worst[name], rec[0][1:])]
    for name, (err_k, err_t, top) in worst.items():
        print('LSTMERR big %s total err_kernel %.3e err_fp32_torch %.3e max|ref| %.3e' % (name, err_k, err_t, top))
        assert err_k <= 4 * err_t + 2.0 ** -23 * top, (name, err_k, err_t, top)


# ------------------------------------------------------------------ 3. masked_rows_copy_

def _row_masks(gen, E):
    return {'none': torch.zeros(E, dtype=torch.bool), 'all': torch.ones(E, dtype=torch.bool),
            'random': torch.rand(E, generator=gen) > 0.5}


def _masked_rows_case(cuda, E, Fs, gen):
    """dst the mover's slice h[:, p] of an (E, P, F) state, src a channel slice of a stacked (E, 3, F) tensor
    (both row strides > F); every float of both storages outside the selected rows must be unchanged."""
    from handyrl_amd.nn import masked_rows_copy_
    P = 2
    for kind, mask in _row_masks(gen, E).items():
        states = [torch.randn(E, P, F, generator=gen).to(cuda) for F in Fs]
        stacked = [torch.randn(E, 3, F, generator=gen).to(cuda) for F in Fs]
        dst = [s[:, l % P] for l, s in enumerate(states)]
        src = [s[:, 1 + l % 2] for l, s in enumerate(stacked)]
        md = mask.to(cuda)
        want = []
        for l, s in enumerate(states):
            w = s.clone()
            w[:, l % P] = torch.where(md[:, None], src[l], dst[l])
            want.append(w)
        src_before = [s.clone() for s in stacked]
        masked_rows_copy_(dst, src, md)
        for l in range(len(Fs)):
            assert torch.equal(states[l], want[l]), (kind, E, Fs[l], 'state')
            assert torch.equal(stacked[l], src_before[l]), (kind, E, Fs[l], 'source changed')


@pytest.mark.parametrize('F', [1, 36, 1152, 1153])
@pytest.mark.parametrize('E', [1, 7, 3000])
def test_masked_rows_copy(cuda, E, F):
    """torch.where(mask[:, None], src, dst), exactly: one leaf; F = 1152 / 1153: several trips of the per-thread
    loop with and without an odd tail."""
    _masked_rows_case(cuda, E, [F], torch.Generator().manual_seed(E + F))


def test_masked_rows_copy_sixteen_leaves(cuda):
    _masked_rows_case(cuda, 7, [1, 36, 1152, 1153, 2, 3, 5, 255, 256, 257, 511, 513, 7, 64, 100, 1000],
                      torch.Generator().manual_seed(16))


# ------------------------------------------------------------------ 4. output-mask kernels

def ref_output_mask(opol, oval, tmask, omask, amask):
    """policy = sum_p o_pol[p or 0] tmask[p] - amask, summed from 0 in p order; value = o_val[p or 0] omask[p]
    (train.py:176-183).  opol (B, T, Pq, A), oval (B, T, Pq, 1), masks (B, T, P, 1), amask (B, T, 1, A)."""
    P, Pq = tmask.shape[2], opol.shape[2]
    acc = torch.zeros_like(amask)
    for p in range(P):
        q = 0 if Pq == 1 else p
        acc = acc + opol[:, :, q:q + 1] * tmask[:, :, p:p + 1]
    val = None if oval is None else (oval if Pq == P else oval.expand(-1, -1, P, -1)) * omask
    return acc - amask, val


def mir_output_mask_bwd(gpol, gval, tmask, omask, Pq):
    """gopol[q] = sum_p gpol tmask[p] from 0 (Pq = 1) or gpol tmask[q]; goval likewise from gval omask."""
    P = tmask.shape[2]
    if Pq == 1:
        gopol = torch.zeros_like(gpol)
        for p in range(P):
            gopol = gopol + gpol * tmask[:, :, p:p + 1]
    else:
        gopol = gpol * tmask
    goval = None
    if gval is not None:
        if Pq == 1:
            goval = torch.zeros_like(gval[:, :, :1])
            for p in range(P):
                goval = goval + gval[:, :, p:p + 1] * omask[:, :, p:p + 1]
        else:
            goval = gval * omask
    return gopol, goval


@pytest.mark.parametrize('kind', ['frac', 'bin'])
@pytest.mark.parametrize('A', [1, 9, 214])
@pytest.mark.parametrize('P,Pq', [(4, 4), (4, 1), (3, 3), (1, 1)])
def test_output_mask(cuda, P, Pq, A, kind):
    """_OutputMask at the Geese geometry (P = 4) and others, B T = 35 (a partial last block at every A), and the
    C entries with oval NULL (forward) and gval NULL (backward)."""
    from handyrl_amd.train import _OutputMask
    lib, p = _native.load(), _native.ptr
    B, T = 7, 5
    k = 2 * P + 2
    gen = torch.Generator().manual_seed(100 * P + 10 * Pq + A)
    opol = torch.randn(B, T, Pq, A, generator=gen)
    oval = torch.randn(B, T, Pq, 1, generator=gen)
    tmask = _masks(gen, B * T, P, kind).view(B, T, P, 1)
    omask = _masks(gen, B * T, P, kind).view(B, T, P, 1)
    amask = (torch.rand(B, T, 1, A, generator=gen) > 0.7).float() * 1e32
    gpol, gval = torch.randn(B, T, 1, A, generator=gen), torch.randn(B, T, P, 1, generator=gen)
    ins = [opol, oval, tmask, omask, amask]
    fn = lambda xs, tm, om, am: list(ref_output_mask(xs[0], xs[1], tm, om, am))   # noqa: E731
    with torch.no_grad():
        mir_outs = fn(ins[:2], *ins[2:])
    mir_grads = mir_output_mask_bwd(gpol, gval, tmask, omask, Pq)
    d = lambda ts: [t.double() for t in ts]   # noqa: E731
    ref_outs, ref_grads = _grad64(lambda xs: fn(xs, *d(ins[2:])), d(ins[:2]), d([gpol, gval]))
    # sum|terms|: the action mask is subtracted, so its magnitude enters with the other sign
    mag_outs, mag_grads = _grad64(lambda xs: fn(xs, *d([tmask, omask, -amask])), [x.abs() for x in d(ins[:2])],
                                  [x.abs() for x in d([gpol, gval])])
    dev = [t.to(cuda) for t in ins]
    dev[0].requires_grad_(True)
    dev[1].requires_grad_(True)
    outs = _OutputMask.apply(*dev)
    torch.autograd.backward(outs, [gpol.to(cuda), gval.to(cuda)])
    for i in range(2):
        _check(outs[i], mir_outs[i], ref_outs[i], mag_outs[i], k, ('output', i))
        _check(dev[i].grad, mir_grads[i], ref_grads[i], mag_grads[i], k, ('gradient', i))
    # oval NULL: only the policy is written; gval NULL: only the policy's gradient
    pol = torch.full((B, T, 1, A), float('nan'), device=cuda)
    val = torch.full((B, T, P, 1), 7.0, device=cuda)
    rc = lib.hrl_output_mask_forward(p(dev[0]), None, p(dev[2]), p(dev[3]), p(dev[4]), B * T, P, Pq, A, p(pol),
                                     p(val), _native.stream_of(cuda))
    assert rc == 0 and torch.equal(pol.cpu(), mir_outs[0]) and bool((val == 7.0).all())
    gopol = torch.full((B, T, Pq, A), float('nan'), device=cuda)
    goval = torch.full((B, T, Pq, 1), 7.0, device=cuda)
    gpd = gpol.to(cuda)
    rc = lib.hrl_output_mask_backward(p(gpd), None, p(dev[2]), p(dev[3]), B * T, P, Pq, A, p(gopol),
                                      p(goval), _native.stream_of(cuda))
    assert rc == 0 and torch.equal(gopol.cpu(), mir_grads[0]) and bool((goval == 7.0).all())

