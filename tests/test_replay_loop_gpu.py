"""The training loops on the fused replay gather: the same weights as the torch gather, and no batch copy into
the learner graph's static inputs from the second step on.
"""

import os

import pytest
import torch

from handyrl_amd import rollout
from handyrl_amd.trainer import LearnerStep

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def load_batch_calls(monkeypatch):
    """The step index (0 = the capturing step) of every LearnerStep.load_batch call."""
    calls = []
    real_load, real_step = LearnerStep.load_batch, LearnerStep.step
    steps = [0]

    def load_batch(self, batch):
        calls.append(steps[0])
        return real_load(self, batch)

    def step(self, batch, hidden=None):
        out = real_step(self, batch, hidden)
        steps[0] += 1
        return out
    monkeypatch.setattr(LearnerStep, 'load_batch', load_batch)
    monkeypatch.setattr(LearnerStep, 'step', step)
    return calls, steps


def _adam_state(learner):
    """Adam's moments and step counts: the step tail's flat buffers, or torch.optim.Adam's state."""
    if learner.tail is not None:
        return {'m': learner.tail.m, 'v': learner.tail.v, 'step': learner.tail.step_t}
    state = learner.optimizer.state_dict()['state']
    return {'%s.%s' % (k, n): torch.as_tensor(v) for k, s in state.items() for n, v in s.items()}


def _run(cuda, fused, monkeypatch):
    from handyrl_amd.envs.tictactoe import SimpleConv2dModel
    from handyrl_amd.loop import SelfPlayTrainer
    from handyrl_amd.synthetic import default_args
    monkeypatch.setattr(rollout, 'FUSED_GATHER', fused)
    torch.manual_seed(0)
    net = SimpleConv2dModel().to(cuda)
    args = default_args(4, 64)
    tr = SelfPlayTrainer(net, args, cuda, games_per_round=128, capacity=256, graph=True, seed=3)
    tr.run(1, 3)
    torch.cuda.synchronize()
    assert tr.steps == 3
    return net, tr.learner


def test_selfplay_trainer_weights_are_exact_and_no_batch_is_copied(cuda, monkeypatch, load_batch_calls):
    calls, steps = load_batch_calls
    net_a, learner_a = _run(cuda, False, monkeypatch)
    del calls[:]
    steps[0] = 0
    net_b, learner_b = _run(cuda, True, monkeypatch)
    assert steps[0] == 3 and calls == [], calls        # fused run: no load_batch at all (the batch is the static input)
    for (ka, a), (kb, b) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    sa, sb = _adam_state(learner_a), _adam_state(learner_b)
    assert sa.keys() == sb.keys() and len(sa) > 0
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert any(bool((v != 0).any()) for v in sa.values())


def test_train_main_copies_no_batch(cuda, tmp_path, load_batch_calls):
    from handyrl_amd.main import load_config, train_main
    calls, steps = load_batch_calls
    args = load_config(os.path.join(ROOT, 'config.yaml'))
    args['env_args']['env'] = 'TicTacToe'
    args['train_args'].update(update_episodes=16, minimum_episodes=32, maximum_episodes=64, batch_size=8,
                              forward_steps=6, epochs=2, window_draw='inverse')
    assert rollout.FUSED_GATHER
    train_main(args, device=cuda, model_dir=str(tmp_path), log=lambda *_: None)
    assert steps[0] >= 2
    assert [c for c in calls if c >= 1] == [], calls
    assert os.path.exists(tmp_path / '2.pth')
