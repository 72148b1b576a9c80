"""The pieces the device generators and evaluators share: the one decision (``act_torch`` is ``match_act_torch``
without an opponent), ``rollout.params_key`` and the training mode that every driver puts back when a forward raises.
CPU only."""

import copy
import os

import numpy as np
import pytest
import torch
from torch import nn

from handyrl_amd import evaluation as ev
from handyrl_amd.evaluation import DeviceEvaluator, LeagueEvaluator
from handyrl_amd import rollout
from handyrl_amd.rollout import (DeviceGenerator, DeviceReplay, ParallelTicTacToeBatch, PlayerReplay,
                                 PlayerStreamGenerator, StreamGenerator, TicTacToeBatch, params_key)

E, A, P, TM, G, SEED = 7, 5, 3, 6, 5, 0x1234567887654321


def _state():
    """Seven slots: live ones on every seat, an inactive one, a ply and two game numbers out of range."""
    return {'Tm': TM, 'P': P,
            'game': torch.tensor([0, 1, 2, 3, 4, G, -1]), 'ply': torch.tensor([0, 5, 2, TM, 1, 0, 3]),
            'seat': torch.tensor([0, 1, 2, 0, 1, 2, 0]),
            'active': torch.tensor([True, True, True, True, False, True, True])}


def _trace():
    return {'action': torch.full((G + 1, TM), -1), 'picked': torch.full((G + 1, TM), -1),
            'policy': torch.zeros(G + 1, TM, A), 'model_ply': torch.zeros(G + 1, TM, dtype=torch.bool)}


@pytest.mark.parametrize('temperature', [0.0, 0.5])
@pytest.mark.parametrize('mover', range(P))
def test_act_torch_is_the_match_decision_without_an_opponent(temperature, mover):
    g = torch.Generator().manual_seed(3 * mover + int(temperature > 0))
    logits = torch.randn(E, A + 2, generator=g)
    legal = torch.rand(E, A, generator=g) < 0.6
    legal[:, 1] = True
    legal[2] = False                                   # a row with no legal label
    forced = torch.full((G + 1, TM), -1)
    forced[1, 5] = 4
    st, tr_a, tr_m = _state(), _trace(), _trace()
    a = ev.act_torch(st, logits, legal, mover, SEED, temperature, G, forced, tr_a)
    m = ev.match_act_torch(st, logits, None, legal, mover, SEED, temperature, 0.0, 0, G, forced, tr_m)
    assert torch.equal(a, m)
    for k in tr_a:
        assert torch.equal(tr_a[k][:G], tr_m[k][:G]), k
    # and the decision is the public rule: 0 for a slot that does not play, a forced move as given, eval_pick on a
    # random seat, the argmax of the masked logits on the model's seat at temperature 0
    ok = [0, 1, 2]
    assert a[3:].tolist() == [0, 0, 0, 0]
    for e in ok:
        game, ply, model = int(st['game'][e]), int(st['ply'][e]), int(st['seat'][e]) == mover
        assert bool(tr_a['model_ply'][game, ply]) == model
        if (game, ply) == (1, 5):
            assert int(a[e]) == 4
        elif not model and bool(legal[e].any()):
            assert int(a[e]) == ev.eval_pick(SEED, game, ply, legal[e].tolist())
        elif model and temperature == 0:
            assert int(a[e]) == int(torch.argmax(logits[e, :A] - torch.where(legal[e], 0.0, 1e32)))


class Raises(nn.Module):
    """A net whose forward fails."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))

    def forward(self, x, hidden=None):
        raise RuntimeError('the forward failed')


def _generator():
    net = Raises()
    return [net], DeviceGenerator(TicTacToeBatch(4, 'cpu'), net).generate


def _stream():
    cls, net = TicTacToeBatch, Raises()
    replay = DeviceReplay(8, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P, 'cpu')
    gen = StreamGenerator(cls(4, 'cpu'), net, replay)
    return [net], lambda: gen.generate(2)


def _evaluator():
    nets = [Raises(), Raises()]
    evaluator = DeviceEvaluator(TicTacToeBatch(4, 'cpu'), nets[0], opponent=nets[1], opening_plies=1)
    return nets, lambda: evaluator.evaluate(4)


def _league():
    nets = [Raises(), Raises()]
    league = LeagueEvaluator(TicTacToeBatch(4, 'cpu'), nets)
    return nets, lambda: league.evaluate(2)


@pytest.mark.parametrize('make', [_generator, _stream, _evaluator, _league])
@pytest.mark.parametrize('training', [True, False])
def test_a_failing_forward_leaves_the_training_mode(make, training):
    nets, call = make()
    modes = [training] + [not training] * (len(nets) - 1)      # a second net in the other mode
    for n, mode in zip(nets, modes):
        n.train(mode)
    with pytest.raises(RuntimeError, match='the forward failed'):
        call()
    assert [n.training for n in nets] == modes


def test_params_key_follows_the_tensors_not_their_values():
    net, other = nn.Linear(3, 2), nn.BatchNorm1d(2)
    key = params_key(net, other)
    assert key == tuple(t.data_ptr() for n in (net, other) for t in list(n.parameters()) + list(n.buffers()))
    assert len(key) == 2 + 2 + 3
    src = copy.deepcopy(net)
    with torch.no_grad():
        src.weight.add_(1.0)
    net.load_state_dict(src.state_dict())              # in place: the tensors stay where they are
    assert torch.equal(net.weight, src.weight) and params_key(net, other) == key
    net.weight = nn.Parameter(torch.zeros(2, 3))       # a parameter tensor replaced
    assert params_key(net, other) != key
    assert params_key(net, other)[1:] == key[1:]


def test_the_stream_generators_share_one_driver():
    cls = TicTacToeBatch
    gen = StreamGenerator(cls(4, 'cpu'), nn.Identity(),
                          DeviceReplay(8, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P, 'cpu'))
    cls = ParallelTicTacToeBatch
    players = PlayerStreamGenerator(cls(4, 'cpu'), nn.Identity(),
                                    PlayerReplay(8, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P, 'cpu'))
    for g in (gen, players):
        assert isinstance(g, rollout._StreamDriver)
        assert type(g).generate is rollout._StreamDriver.generate
        assert type(g)._capture is rollout._StreamDriver._capture


def _harvest_state(players):
    """A hand-made harvest of E = 4 slots, Tm = 3, into a ring of N = 5 from ring_ptr = 4: slots 0, 2 and 3 are done
    with lengths 2, 3 (= Tm) and 0, so rows 4, 0 and 1 are written (the write wraps) and rows 2 and 3 keep their
    prefill.  The mover layout narrows fp32 observations into a uint8 ring, the per-player one widens uint8
    observations into an fp32 ring."""
    n, Tm, N, P, A = 4, 3, 5, 2, 2
    g = torch.Generator().manual_seed(5 + players)
    lead = (n, Tm, P) if players else (n, Tm)
    obs = torch.randint(0, 256, lead + (2,), generator=g)
    st = {'obs': obs.to(torch.uint8) if players else obs.float(),
          'policy': torch.randn(lead + (A,), generator=g), 'amask': torch.randn(lead + (A,), generator=g),
          'action': torch.randint(0, A, lead, generator=g), 'value': torch.randn(lead, generator=g),
          'reward': torch.randn(n, Tm, P, generator=g, dtype=torch.float64),
          'ply': torch.tensor([2, 1, 3, 0]), 'game': torch.tensor([7, 8, 9, 10]),
          'pending': torch.tensor([False, True, False, False]), 'state': torch.tensor([4, 20, 30]),
          'rows': torch.arange(n)}
    if players:
        st['tmask'], st['omask'] = torch.rand(lead, generator=g) < 0.5, torch.rand(lead, generator=g) < 0.5
        replay = PlayerReplay(N, Tm, (2,), A, P, 'cpu', obs_dtype=torch.float32)
    else:
        st['turn'] = torch.randint(0, P, lead, generator=g)
        replay = DeviceReplay(N, Tm, (2,), A, P, 'cpu', obs_dtype=torch.uint8)
    keys = ('policy', 'amask', 'action', 'value', 'reward', 'ret', 'length', 'outcome') + \
        (('tmask', 'omask') if players else ('turn',))
    for k in keys + ('obs',):                # a prefill that no record's reset value equals
        t = getattr(replay, k)
        t.copy_(torch.randint(2, 9, t.shape, generator=g).to(t.dtype))
    done = torch.tensor([True, False, True, True])
    outcome = torch.randn(n, P, generator=g)
    ring_game = torch.tensor([-1, 3, 4, 5, 6])
    return st, done, outcome, replay, ring_game, keys


@pytest.mark.parametrize('players', [False, True])
def test_both_harvest_formulations_are_the_shared_one(players):
    """``harvest_torch`` and ``harvest_players_torch`` give the ring bytes they gave as two separate functions
    (tests/golden/stream_harvest.npz).  The fixture is ``_harvest_state`` run through the two functions of the commit
    before they became one, every ring and slot tensor saved under ``mover.`` / ``players.`` + its name: check that
    commit out, call either function on ``_harvest_state(players)`` with gamma 0.8 and a reward, and the arrays
    compared below are the file's."""
    st, done, outcome, replay, ring_game, keys = _harvest_state(players)
    calls = []
    shared = rollout._harvest_torch
    try:
        rollout._harvest_torch = lambda *a: (calls.append(a[0]), shared(*a))
        (rollout.harvest_players_torch if players else rollout.harvest_torch)(
            st, done, outcome, 0.8, replay, ring_game, True)
    finally:
        rollout._harvest_torch = shared
    assert calls == [('action', 'value', 'tmask', 'omask') if players else ('action', 'value', 'turn')]
    got = {k: getattr(replay, k) for k in keys + ('obs',)}
    got.update(ring_game=ring_game, ply=st['ply'], game=st['game'], pending=st['pending'], state=st['state'])
    golden = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'stream_harvest.npz'))
    prefix = 'players.' if players else 'mover.'
    assert sorted(k[len(prefix):] for k in golden.files if k.startswith(prefix)) == sorted(got)
    for k, v in got.items():
        want = golden[prefix + k]
        assert v.numpy().dtype == want.dtype and v.numpy().tobytes() == want.tobytes(), k
    assert got['length'][[4, 0, 1]].tolist() == [2, 3, 0] and got['ring_game'].tolist() == [9, 10, 4, 5, 7]
    assert got['state'].tolist() == [2, 23, 33] and got['game'].tolist() == [30, 8, 31, 32]
