"""nn.GeeseInference where the project plays Hungry Geese, on the CPU: the wrapper runs the net's own forward, so the
evaluator's result and the per-player generator's episodes equal the plain run's exactly."""

import pytest
import torch

from handyrl_amd import nn as hnn
from handyrl_amd.envs.geese import HungryGeeseBatch
from handyrl_amd.envs.hungry_geese import GeeseNet
from handyrl_amd.evaluation import PlayerEvaluator
from handyrl_amd.rollout import DeviceGenerator

from .test_board_infer_rollout import _equal_tree
from .test_player_eval_rollout import SEED, same


def _net(layers=2, seed=3):
    torch.manual_seed(seed)
    return GeeseNet(layers=layers).eval()


@pytest.mark.parametrize('kw', [{}, {'opponent': 'rule'}])
def test_cpu_evaluator_with_the_wrapper_equals_plain(kw):
    net = _net()
    res = []
    for n in (net, hnn.GeeseInference(net)):
        b = HungryGeeseBatch(4, 'cpu')
        b.seed(SEED)
        res.append(PlayerEvaluator(b, n, seed=SEED, **kw).evaluate(6, trace=True))
    same(res[0], res[1])
    assert res[0]['games'] == 6


def test_cpu_generator_with_the_wrapper_equals_plain():
    net = _net()
    eps = []
    for n in (net, hnn.GeeseInference(net)):
        gen = DeviceGenerator(HungryGeeseBatch(4, 'cpu', seed=3), n, gamma=0.8)
        assert gen.per_player
        eps.append(gen.generate(generator=torch.Generator().manual_seed(3)))
    _equal_tree(eps[0], eps[1])
    assert int(eps[0]['length'].max()) > 1


def test_cpu_evaluator_in_training_mode_is_put_back():
    """The evaluator plays in eval mode and puts the training mode back; the wrapper itself refuses it."""
    net = _net(1)
    w = hnn.GeeseInference(net).train()
    with pytest.raises(RuntimeError):
        w(torch.zeros(1, 17, 7, 11))
    b = HungryGeeseBatch(2, 'cpu')
    b.seed(SEED)
    res = PlayerEvaluator(b, w, seed=SEED).evaluate(2)
    assert res['games'] == 2 and net.training
