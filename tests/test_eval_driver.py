"""The pieces the device generators and evaluators share: the one decision (``act_torch`` is ``match_act_torch``
without an opponent), ``rollout.params_key`` and the training mode that every driver puts back when a forward raises.
CPU only."""

import copy

import pytest
import torch
from torch import nn

from handyrl_amd import evaluation as ev
from handyrl_amd.evaluation import DeviceEvaluator, LeagueEvaluator
from handyrl_amd.rollout import DeviceGenerator, DeviceReplay, StreamGenerator, TicTacToeBatch, params_key

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
