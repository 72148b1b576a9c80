"""hrl_league_finish and hrl_rows_permute against their torch formulation (handyrl_amd.evaluation), bit for bit, on
guard-band buffers (tests/guarded.py): a store outside a buffer, into a row that is not addressed or into a slot that
must store nothing fails the run.  The result buffers have exactly Q * G rows for the kernel (the torch ops use one
spare row for the slots that store nothing).  And hrl_match_act as the league calls it: both logit pointers equal."""

import numpy as np
import pytest
import torch

from handyrl_amd import evaluation as ev
from tests.guarded import Arena, bits
from tests.test_eval_kernels_gpu import _legal, _logits, _slots

pytestmark = pytest.mark.gpu

P = 2


def _same(a, b, what):
    assert torch.equal(bits(a), bits(b)), what


def _run_finish(cuda, Q, S, G, Tm, seed):
    """Every block: distinct game numbers, so no two slots store to one row; numbers >= G (up to 2**40, on active
    slots too: they store nothing and retire).  Slots: active (terminal or not, at ply Tm - 1 or below), inactive with
    and without `pending`, retired (game == G)."""
    E = Q * S
    rng = np.random.default_rng([Q, S, G, Tm, seed])
    game = np.concatenate([rng.permutation(max(G, S) + 2)[:S] for _ in range(Q)]).astype(np.int64)
    far = (game >= G) & (rng.random(E) < 0.5)
    game[far] = rng.integers(1 << 32, 1 << 40, int(far.sum())) if far.any() else 0
    active = rng.random(E) < 0.75
    retired = (~active) & (rng.random(E) < 0.5)
    game[retired] = G
    pending = (~active) & (~retired) & (rng.random(E) < 0.6)
    ply = rng.integers(0, Tm, E)
    ply[rng.random(E) < 0.3] = Tm - 1                  # ends by its length
    terminal = rng.random(E) < 0.4
    if seed == 0:
        active[:] = True                               # every slot done at once
        terminal[:] = True
    if seed == 1:
        terminal[:] = False
        ply[:] = 0                                     # nothing done (unless Tm == 1)
    st = {'Tm': Tm, 'P': P, 'S': S, 'game': torch.from_numpy(game), 'ply': torch.from_numpy(ply),
          'active': torch.from_numpy(active), 'pending': torch.from_numpy(pending), 'state': torch.tensor([11])}
    st = {k: v.to(cuda) if isinstance(v, torch.Tensor) else v for k, v in st.items()}
    terminal = torch.from_numpy(terminal).to(cuda)
    outcome = torch.from_numpy(rng.integers(-1, 2, (E, P)).astype(np.float32)).to(cuda)
    keys = ('game', 'ply', 'active', 'pending', 'state')
    ref = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
    ref_out = torch.full((Q * G + 1, P), 9.0, device=cuda)
    ref_len = torch.full((Q * G + 1,), -9, dtype=torch.long, device=cuda)
    ev.league_finish_torch(ref, terminal, outcome, G, ref_out, ref_len)
    arena = Arena(cuda)
    hip = dict(st)
    for k in keys:
        hip[k] = arena.inout(st[k], name=k)
    out = arena.inout(torch.full((Q * G, P), 9.0, device=cuda), name='outcome_out')
    ln = arena.inout(torch.full((Q * G,), -9, dtype=torch.long, device=cuda), name='length_out')
    ev.league_finish_hip(hip, arena.inout(terminal, name='terminal'), arena.inout(outcome, name='outcome'), G, out, ln)
    arena.check()
    what = (Q, S, G, Tm, seed)
    for k in keys:
        _same(hip[k], ref[k], (k,) + what)
    _same(out, ref_out[:Q * G], ('outcome_out',) + what)
    _same(ln, ref_len[:Q * G], ('length_out',) + what)
    # the rule itself, on the host
    done = st['active'] & (terminal | (st['ply'] + 1 >= Tm))
    assert int(hip['state'][0]) == 11 + int(done.sum())
    nxt = st['game'] + S
    assert torch.equal(hip['game'][done], torch.where(nxt < G, nxt, G)[done])
    assert torch.equal(hip['pending'][done], (nxt < G)[done]) and not bool(hip['active'][done].any())
    assert not bool(hip['ply'][done].any())
    assert torch.equal(hip['ply'][~done], (st['ply'] + st['active'].long())[~done])
    return int(done.sum()), int((done & (nxt >= G)).sum())


@pytest.mark.parametrize('Q,S', [(1, 2), (3, 2), (3, 6), (10, 8)])
def test_league_finish_equals_torch_formulation(cuda, Q, S):
    done = retired = 0
    for G in (1, 2, 7):
        for Tm in (1, 9):
            for seed in range(4):
                d, r = _run_finish(cuda, Q, S, G, Tm, seed)
                done += d
                retired += r
    assert retired > 0 and (S > 2 or done > retired)   # slots retired and, where game + S < G happens, restarted


LEAF_F = (1, 3, 4, 37, 1152)
PADS = (0, 1, 4, 3)


def _leaves(arena, rng, nleaves, rows, tag):
    """nleaves (rows, F) views of (rows, F + pad) buffers: row strides larger than F on most; F % 4 == 0 with an
    aligned stride takes the float4 path, an odd stride the scalar one."""
    whole, views = [], []
    for l in range(nleaves):
        F = LEAF_F[l % len(LEAF_F)]
        stride = F + PADS[(l // len(LEAF_F) + l) % len(PADS)]
        t = arena.inout(torch.from_numpy(rng.standard_normal((rows, stride)).astype(np.float32)),
                        name='%s%d' % (tag, l))
        whole.append(t)
        views.append(t[:, :F])
    return whole, views


@pytest.mark.parametrize('n', (1, 5, 64, 67))
@pytest.mark.parametrize('nleaves', (1, 3, 16))
def test_rows_permute_equals_index_ops(cuda, nleaves, n):
    """Gather only, scatter only and both; every index in range, the dst rows distinct; rows that are not addressed
    and the columns between F and the row stride keep their bits."""
    for mode in ('gather', 'scatter', 'both'):
        rng = np.random.default_rng([nleaves, n, len(mode)])
        arena = Arena(cuda)
        src_rows, dst_rows = n + 3, n + 2
        src_whole, src = _leaves(arena, rng, nleaves, src_rows, 'src')
        dst_whole, dst = _leaves(arena, rng, nleaves, dst_rows, 'dst')
        src_index = dst_index = None
        if mode in ('gather', 'both'):
            src_index = arena.inout(torch.from_numpy(rng.integers(0, src_rows, n)), name='src_index')
        if mode in ('scatter', 'both'):
            dst_index = arena.inout(torch.from_numpy(rng.permutation(dst_rows)[:n].astype(np.int64)),
                                    name='dst_index')
        want_whole = [t.clone() for t in dst_whole]
        want = [t[:, :v.shape[1]] for t, v in zip(want_whole, dst)]
        before = [t.clone() for t in src_whole]
        ev.rows_permute_torch(want, src, src_index, dst_index, n)
        ev.rows_permute_hip(dst, src, src_index, dst_index, n)
        arena.check()
        for l in range(nleaves):
            _same(dst_whole[l], want_whole[l], (mode, nleaves, n, l))
            _same(src_whole[l], before[l], ('src', mode, nleaves, n, l))
            si = torch.arange(n, device=cuda) if src_index is None else src_index
            di = torch.arange(n, device=cuda) if dst_index is None else dst_index
            _same(dst[l][di], src[l][si], ('rows', mode, nleaves, n, l))


def test_rows_permute_without_rows_launches_nothing(cuda):
    rng = np.random.default_rng(0)
    arena = Arena(cuda)
    _, src = _leaves(arena, rng, 3, 4, 'src')
    _, dst = _leaves(arena, rng, 3, 4, 'dst')
    index = arena.inout(torch.zeros(4, dtype=torch.long), name='index')
    ev.rows_permute_hip(dst, src, index, index, 0)
    ev.rows_permute_hip(dst, src, None, None, 0)
    arena.check_untouched()


def test_stacked_state_leaves_and_the_evaluators_shapes(cuda):
    """The shapes the league routes: Geister's observation leaves (7 * 36 and 18 floats) for E = 67 rows into
    net-major order by a permutation, its logits (214) back by the inverse; channel slices of a stacked tensor."""
    rng = np.random.default_rng(5)
    arena = Arena(cuda)
    E = 67
    board = arena.inout(torch.from_numpy(rng.standard_normal((E, 7, 6, 6)).astype(np.float32)), name='board')
    scalar = arena.inout(torch.from_numpy(rng.standard_normal((E, 18)).astype(np.float32)), name='scalar')
    out_b, out_s = arena.out((E, 7, 6, 6), name='out_board'), arena.out((E, 18), name='out_scalar')
    order = torch.from_numpy(rng.permutation(E).astype(np.int64)).to(cuda)
    ev.rows_permute_hip([out_b, out_s], [board, scalar], order, None)
    arena.check()
    _same(out_b, board[order], 'board')
    _same(out_s, scalar[order], 'scalar')
    back = torch.empty_like(order)
    back[order] = torch.arange(E, device=cuda)
    logits = arena.inout(torch.from_numpy(rng.standard_normal((E, 214)).astype(np.float32)), name='logits')
    slot = arena.out((E, 214), name='slot_logits')
    ev.rows_permute_hip([slot], [logits], back, None)
    arena.check()
    _same(slot[order], logits, 'logits')
    stacked = arena.inout(torch.from_numpy(rng.standard_normal((E, 3 * 8, 6, 6)).astype(np.float32)), name='stacked')
    keep = stacked.clone()
    fresh = arena.out((E, 8, 6, 6), name='fresh')
    ev.rows_permute_hip([fresh], [stacked[:, 8:16]], order, None)
    arena.check()
    _same(fresh, keep[order][:, 8:16], 'slice')
    _same(stacked, keep, 'stacked')


@pytest.mark.parametrize('E,A', [(5, 9), (67, 9), (64, 214)])
def test_match_act_with_both_logit_pointers_equal(cuda, E, A):
    """The league's decision: hrl_match_act as it stands, home and opponent logits in ONE slot-ordered buffer and one
    temperature; every output equals the call with two buffers that hold the same rows."""
    for n, (temperature, opening) in enumerate(((0.0, 0), (0.0, 2), (0.5, 0), (0.5, 1))):
        rng = np.random.default_rng([E, A, n])
        G = E + 3
        st = _slots(rng, E, G, 'rule', n % 2, cuda)
        logits = _logits(rng, E, A, 'random', A + 3).to(cuda)
        legal = _legal(rng, E, A, 'mixed').to(cuda)
        arena = Arena(cuda)
        one = arena.inout(logits, name='logits')
        got = ev.match_act_hip(st, one, one, arena.inout(legal, name='legal'), n % 2, 12345, temperature, temperature,
                               opening, G)
        arena.check()
        want = ev.match_act_hip(st, logits, logits.clone(), legal, n % 2, 12345, temperature, temperature, opening, G)
        _same(got, want, (E, A, temperature, opening))
        _same(got, ev.match_act_torch(st, logits, logits.clone(), legal, n % 2, 12345, temperature, temperature,
                                      opening, G), ('torch', E, A, temperature, opening))
        _same(one, logits, 'logits untouched')
