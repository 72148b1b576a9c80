"""evaluation.PlayerEvaluator on the GPU: the launches against the torch formulation and the captured graph against
eager plies give identical result dicts; a second call reuses the graph; the pure-Python referee of
tests/test_player_eval_rollout.py accepts what the GPU reports; moving the net's tensors recaptures."""

import pytest
import torch

from handyrl_amd import evaluation
from handyrl_amd.envs.geese import HungryGeeseBatch
from handyrl_amd.evaluation import PlayerEvaluator
from handyrl_amd.rollout import ParallelTicTacToeBatch
from tests.test_player_eval_rollout import SEED, IntNet, cpu, referee_geese, referee_ptt, same

pytestmark = pytest.mark.gpu

CASES = {'geese': (HungryGeeseBatch, 6, 17), 'ptt': (ParallelTicTacToeBatch, 8, 30)}


def _batch(cls, E, dev):
    b = cls(E, dev)
    if hasattr(b, 'seed'):
        b.seed(SEED)
    return b


def _evaluator(name, dev, match, graph, temperature=0.0):
    cls, E, _ = CASES[name]
    net = IntNet(cls).to(dev)
    kw = {'opponent': IntNet(cls, gen=23).to(dev), 'opening_plies': 2} if match else {}
    return PlayerEvaluator(_batch(cls, E, dev), net, temperature=temperature, seed=SEED, graph=graph, **kw), net, kw


@pytest.fixture
def torch_ops(monkeypatch):
    def switch(on):
        monkeypatch.setattr(evaluation, 'FUSED_PLAYER_EVAL', not on)
    return switch


@pytest.mark.parametrize('match', [False, True])
@pytest.mark.parametrize('name', ['geese', 'ptt'])
def test_fused_graph_eager_and_torch_ops_agree_and_are_refereed(cuda, torch_ops, name, match):
    G = CASES[name][2]
    ev, net, kw = _evaluator(name, cuda, match, graph=True)
    graph = ev.evaluate(G, trace=True)
    graphs = ev._run['graphs']
    assert graphs is not None and len(graphs) == 1                    # one graph: the ply has no mover
    same(ev.evaluate(G, trace=True), graph)                           # a second call starts afresh ...
    assert ev._run['graphs'] is graphs                                # ... and reuses the graph
    eager = _evaluator(name, cuda, match, graph=False)[0].evaluate(G, trace=True)
    same(eager, graph)
    torch_ops(True)
    same(_evaluator(name, cuda, match, graph=False)[0].evaluate(G, trace=True), graph)
    torch_ops(False)
    referee = referee_geese if name == 'geese' else referee_ptt
    cpu_net = IntNet(CASES[name][0])
    opp = IntNet(CASES[name][0], gen=23) if match else None
    referee(graph, G, cpu_net, opponent=opp, opening=2 if match else 0)
    # and the CPU evaluator plays the same games
    cls, E, _ = CASES[name]
    cpu_kw = {'opponent': opp, 'opening_plies': 2} if match else {}
    same(PlayerEvaluator(_batch(cls, E, 'cpu'), cpu_net, seed=SEED, **cpu_kw).evaluate(G, trace=True), graph)


def test_temperature_fused_equals_torch_ops(cuda, torch_ops):
    fused = _evaluator('geese', cuda, True, graph=True, temperature=0.8)[0].evaluate(17, trace=True)
    torch_ops(True)
    same(_evaluator('geese', cuda, True, graph=False, temperature=0.8)[0].evaluate(17, trace=True), fused)


def test_moving_the_nets_tensors_recaptures(cuda):
    ev, net, _ = _evaluator('geese', cuda, False, graph=True)
    first = ev.evaluate(17)
    graphs = ev._run['graphs']
    net.w = net.w.clone() * 2 + 1                                     # another tensor at another address
    second = ev.evaluate(17)
    assert ev._run['graphs'] is not graphs
    want = PlayerEvaluator(_batch(HungryGeeseBatch, 6, cuda), net, seed=SEED, graph=False).evaluate(17)
    same(second, want)
    assert cpu(first)['games'] == 17


def test_real_net_on_the_gpu_is_refereed(cuda):
    from handyrl_amd.envs.geese import GeeseNet
    from handyrl_amd.nn import accelerate
    torch.manual_seed(11)
    ref = GeeseNet()
    ref.eval()
    net = accelerate(GeeseNet().to(cuda))
    net.load_state_dict(ref.state_dict())
    res = PlayerEvaluator(_batch(HungryGeeseBatch, 6, cuda), net, seed=SEED).evaluate(17, trace=True)
    # the margin between the two largest logits decides whether a 1e-5 difference may flip a pick: the referee
    # takes the argmax of the TRACED policy and compares the policy itself with the CPU forward
    referee_geese(res, 17, ref, tol=1e-5)
