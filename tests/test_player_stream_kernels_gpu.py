"""The per-player streaming generator's three entries against their formulations, bit for bit, on guard-band buffers
(tests/guarded.py): hrl_geese_observe_at against the CPU batch's ``observation_of`` loop,
hrl_selfplay_sample_record_players_stream against ``rollout.sample_record_players_stream_torch`` and
hrl_selfplay_harvest_players against ``rollout.harvest_players_torch``.  Every record is prefilled, and what the
contract leaves alone must keep its prefill."""

import pytest
import torch

from tests.guarded import Arena, Plain, bits
from handyrl_amd import rollout
from handyrl_amd.envs import geese
from handyrl_amd.envs.geese import HungryGeeseBatch
from handyrl_amd.rollout import PlayerReplay

pytestmark = pytest.mark.gpu


def _eq(a, b, what):
    assert torch.equal(bits(a), bits(b)), what


# ---- hrl_geese_observe_at

def _geese_states():
    """Three games: one with a dead goose and long bodies, one a few steps in, one fresh."""
    a = geese.new_game(3, 0)
    a['geese'][0] = [5, 6, 7, 18, 29]
    a['geese'][2] = []                       # dead: its slot must end up zero
    a['prev'] = [4, 30, -1, 60]
    b = geese.new_game(3, 1)
    for actions in ((0, 1, 2, 3), (0, 1, 2, 3), (2, 2, 0, 0)):
        geese.step_game(b, actions, 3)
    return [a, b, geese.new_game(3, 2)]


@pytest.mark.parametrize('active', [(1, 1, 1), (1, 0, 1), (0, 1, 0)])
def test_observe_at_matches_the_cpu_batch(cuda, active):
    E, Tm = 3, 4
    ply = torch.tensor([0, 3, 4])            # the last one is out of range: no store
    active = torch.tensor(active, dtype=torch.bool)
    states = _geese_states()
    recs, views = [], []
    for dev, maker in (('cpu', None), (cuda, Arena(cuda)), (cuda, Plain(cuda))):
        env = HungryGeeseBatch(E, dev, seed=3)
        env.load_games(states, range(E))
        infer = env.turns_mask() & active.to(dev).view(E, 1)
        assert infer[0].tolist() == [bool(active[0]), bool(active[0]), False, bool(active[0])]
        fill = torch.full((E, Tm, 4, 17, 7, 11), 0xAB, dtype=torch.uint8)
        rec = fill if maker is None else maker.inout(fill)
        v = env.observe_players_record_at(rec, ply.to(dev), infer, active.to(dev))
        if maker is not None:
            maker.check()
        recs.append(rec.cpu())
        views.append(v.cpu())
    for rec, v in zip(recs[1:], views[1:]):
        _eq(v, views[0], 'views')
        _eq(rec, recs[0], 'record')
    rec = recs[1]
    # the addressed slots hold planes or zeros, every other byte its prefill
    untouched = torch.ones(E, Tm, dtype=torch.bool)
    for e, t in ((0, 0), (1, 3)):
        if active[e]:
            untouched[e, t] = False
            assert bool((rec[e, t] <= 1).all()) and bool(rec[e, t].any())
    assert bool((rec[untouched] == 0xAB).all())
    if active[0]:
        assert not bool(rec[0, 0, 2].any())                     # the dead goose's slot: zeros, not the prefill
        assert torch.equal(rec[0, 0, 1].float(), torch.from_numpy(geese.observation_of(states[0], 1)))


# ---- hrl_selfplay_sample_record_players_stream

@pytest.mark.parametrize('per_player_legal', [False, True])
@pytest.mark.parametrize('E,P,A', [(5, 4, 4), (7, 2, 9)])
def test_tail_matches_torch(cuda, E, P, A, per_player_legal):
    Tm = 5
    g = torch.Generator().manual_seed(100 * E + A + per_player_legal)
    big = torch.randn(P * E, A + 3, generator=g).to(cuda)
    logits = big[:, :A]                                          # rows of stride A + 3
    assert logits.stride(0) == A + 3
    value = torch.randn(P * E, 1, generator=g).to(cuda)
    legal = torch.rand(*((E, P, A) if per_player_legal else (E, A)), generator=g) < 0.6
    legal[1] = False
    legal[1][..., A - 2] = True                                  # rows with one legal label
    legal[2] = False                                             # and with none
    turns = torch.rand(E, P, generator=g) < 0.7
    turns[0] = True
    turns[2, 0] = False                                          # a player without a turn in a played game
    infer = turns | (torch.rand(E, P, generator=g) < 0.3)
    active = torch.ones(E, dtype=torch.bool)
    active[3] = False                                            # an inactive game
    ply = torch.tensor([0, 4, 2, 1, Tm, 3, 0][:E])               # game 4: active at ply == Tm, treated as inactive
    game = torch.tensor([3, 0, (1 << 40) + 5, 17, 4, 1000003, 6][:E])
    turns[3] = True                                              # turns of an inactive game: no action all the same
    rec = {'policy': torch.randn(E, Tm, P, A, generator=g), 'amask': torch.randn(E, Tm, P, A, generator=g),
           'action': torch.randint(0, A, (E, Tm, P), generator=g), 'value': torch.randn(E, Tm, P, generator=g),
           'tmask': torch.rand(E, Tm, P, generator=g) < 0.5, 'omask': torch.rand(E, Tm, P, generator=g) < 0.5}
    seed = 0x9e3779b97f4a7c15
    results = []
    for maker in (None, Arena(cuda), Plain(cuda)):
        keep = (lambda t: t.clone().to(cuda)) if maker is None else maker.inout
        st = {k: keep(v) for k, v in rec.items()}
        st.update(ply=ply.to(cuda), game=game.to(cuda), rows=torch.arange(E, device=cuda))
        fn = (rollout.sample_record_players_stream_torch if maker is None
              else rollout.sample_record_players_stream_hip)
        a, usel = fn(st, seed, logits, legal.to(cuda), value, turns.to(cuda), infer.to(cuda), active.to(cuda))
        if maker is not None:
            maker.check()
        results.append((a, usel, st))
    a0, u0, s0 = results[0]
    assert not bool(a0[3].any()) and not bool(a0[4].any()) and not bool(a0[~turns.to(cuda)].any())
    _eq(u0.cpu(), torch.from_numpy(rollout.stream_select_uniform(seed, game.numpy(), ply.numpy())), 'usel rule')
    for a, usel, st in results[1:]:
        _eq(a, a0, 'action')
        _eq(usel, u0, 'usel')
        for k in rec:
            _eq(st[k], s0[k], k)
    st = results[1][2]
    for k, v in rec.items():                     # games that are not played store nothing; played ones one ply
        for e in (3, 4):
            _eq(st[k][e], v[e].to(cuda), (k, e))
        _eq(st[k][0, 1:], v[0, 1:].to(cuda), (k, 'other plies'))
    # the one legal label is the sample; a player without a turn holds the reset values in a played game
    label = torch.full((P,), A - 2, device=cuda)
    assert torch.equal(a0[1][turns[1].to(cuda)], label[turns[1].to(cuda)])
    e, p, t = 2, 0, int(ply[2])
    assert not bool(st['policy'][e, t, p].any()) and bool((st['amask'][e, t, p] == 1e32).all())
    assert int(st['action'][e, t, p]) == 0 and not bool(st['tmask'][e, t, p])
    assert bool(st['omask'][e, t, p]) == bool(infer[e, p])


# ---- hrl_selfplay_harvest_players

E, TM = 7, 5
SHAPE = {'planes': (17, 7, 11), 'board': (27,), 'scalar': (5,), 'one': (1,), 'line': (16,)}


def _harvest_case(P, N, ring_ptr, slot_dtype, ring_dtype):
    g = torch.Generator().manual_seed(31 * P + N)
    A = 4 if P == 4 else 9
    rec = {'obs': {k: torch.randint(0, 2, (E, TM, P) + s, generator=g).to(slot_dtype) for k, s in SHAPE.items()},
           'policy': torch.randn(E, TM, P, A, generator=g), 'amask': torch.randn(E, TM, P, A, generator=g),
           'action': torch.randint(0, A, (E, TM, P), generator=g), 'value': torch.randn(E, TM, P, generator=g),
           'tmask': torch.rand(E, TM, P, generator=g) < 0.5, 'omask': torch.rand(E, TM, P, generator=g) < 0.5,
           'reward': torch.randn(E, TM, P, generator=g, dtype=torch.float64)}
    done = torch.tensor([1, 1, 0, 1, 1, 1, 0], dtype=torch.bool)       # c = 5
    ply = torch.tensor([0, 1, 3, TM - 1, TM, 2, 1])                    # lengths 0, 1, Tm - 1, Tm among the done slots
    replay = PlayerReplay(N, TM, SHAPE, A, P, 'cpu', obs_dtype=ring_dtype)
    ring = {k: torch.randn(getattr(replay, k).shape, generator=g) for k in ('policy', 'amask', 'value', 'reward',
                                                                             'ret', 'outcome')}
    ring.update({k: torch.randint(0, 5, getattr(replay, k).shape, generator=g) for k in ('action', 'length')})
    ring.update({k: torch.rand(getattr(replay, k).shape, generator=g) < 0.5 for k in ('tmask', 'omask')})
    ring['obs'] = {k: torch.randint(0, 2, v.shape, generator=g).to(ring_dtype) for k, v in replay.obs.items()}
    return dict(rec=rec, done=done, ply=ply, state=torch.tensor([ring_ptr, 100, 1000]), game=torch.arange(E) * 3 + 50,
                pending=torch.tensor([0, 0, 0, 0, 0, 0, 1], dtype=torch.bool), outcome=torch.randn(E, P, generator=g),
                ring=ring, ring_game=torch.randint(0, 40, (N,), generator=g), A=A, P=P, N=N)


def _run_harvest(case, dev, maker, fn, ring_dtype, reward):
    keep = (lambda t: t.clone().to(dev)) if maker is None else maker.inout
    st = {k: v.to(dev) for k, v in case['rec'].items() if k != 'obs'}
    st['obs'] = {k: v.to(dev) for k, v in case['rec']['obs'].items()}
    st.update(ply=keep(case['ply']), game=keep(case['game']), pending=keep(case['pending']),
              state=keep(case['state']), rows=torch.arange(E, device=dev))
    replay = PlayerReplay(case['N'], TM, SHAPE, case['A'], case['P'], dev, obs_dtype=ring_dtype)
    for k, v in case['ring'].items():
        if k == 'obs':
            replay.obs = {kk: keep(vv) for kk, vv in v.items()}
        else:
            setattr(replay, k, keep(v))
    ring_game = keep(case['ring_game'])
    fn(st, case['done'].to(dev), case['outcome'].to(dev), 0.8, replay, ring_game, reward)
    if maker is not None:
        maker.check()
    out = {k: getattr(replay, k) for k in case['ring'] if k != 'obs'}
    out.update({'obs.' + k: v for k, v in replay.obs.items()})
    out.update(ring_game=ring_game, ply=st['ply'], game=st['game'], pending=st['pending'], state=st['state'])
    return out


@pytest.mark.parametrize('reward', [False, True])
@pytest.mark.parametrize('slot_dtype,ring_dtype', [(torch.uint8, torch.uint8), (torch.uint8, torch.float32),
                                                   (torch.float32, torch.uint8), (torch.float32, torch.float32)])
@pytest.mark.parametrize('P,N,ring_ptr', [(4, 3, 2), (2, 8, 6)])
def test_harvest_matches_torch(cuda, P, N, ring_ptr, slot_dtype, ring_dtype, reward):
    """P = 4: the Geese leaf takes the 4-byte unit and 'line' the 16-byte one; P = 2: widths 27, 5 and 1 give records
    of 270, 50 and 10 elements per slot, the element-by-element path.  N = 3 < c = 5: rows are claimed twice.  N = 8
    from row 6: the rows wrap, lengths 0 and 1 land in rows of their own, rows 3-5 keep their prefill."""
    case = _harvest_case(P, N, ring_ptr, slot_dtype, ring_dtype)
    want = _run_harvest(case, cuda, None, rollout.harvest_players_torch, ring_dtype, reward)
    for maker in (Arena(cuda), Plain(cuda)):
        got = _run_harvest(case, cuda, maker, rollout.harvest_players_hip, ring_dtype, reward)
        for k in want:
            _eq(got[k], want[k], k)
    assert want['state'].tolist() == [(ring_ptr + 5) % N, 105, 1005]
    assert want['game'].tolist() == [1000, 1001, 56, 1002, 1003, 1004, 68] and want['ply'][2] == 3
    assert want['pending'].tolist() == [True, True, False, True, True, True, True]
    if N == 8:
        assert want['length'][[6, 7, 0, 1, 2]].tolist() == [0, 1, TM - 1, TM, 2]
        for k, v in case['ring'].items():
            for kk, vv in (v.items() if k == 'obs' else [(None, v)]):
                _eq(want[k if kk is None else 'obs.' + kk][3:6], vv[3:6].to(cuda), (k, kk, 'untouched rows'))
        _eq(want['ring_game'][3:6], case['ring_game'][3:6].to(cuda), 'ring_game')
        assert bool((want['amask'][6] == 1e32).all()) and not bool(want['obs.planes'][6].any())
    else:
        assert want['ring_game'].tolist() == [65, 59, 62]       # slots 5, 3, 4: the highest claim of each row
    if reward:
        rew = case['rec']['reward'][4].double()
        acc, ret = torch.zeros(P, dtype=torch.float64), torch.zeros(TM, P)
        for t in range(TM - 1, -1, -1):
            acc = rew[t] + 0.8 * acc
            ret[t] = acc.float()
        row = 2 if N == 3 else 1
        _eq(want['ret'][row].cpu(), ret, 'ret of the full-length game')
    else:
        assert not bool(want['ret'][2 if N == 3 else 1].any())
