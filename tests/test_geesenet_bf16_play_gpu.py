"""nn.GeeseInference(precision='bf16') where the project plays Hungry Geese on the GPU: the evaluators finish their
games, the stream generator records the policy it sampled from (the behaviour policy V-trace corrects for), and
``main --eval`` takes ``inference: fused_bf16``."""

import pytest
import torch

from handyrl_amd import nn as hnn
from handyrl_amd.envs.geese import GeeseNet, HungryGeeseBatch
from handyrl_amd.evaluation import PlayerEvaluator, eval_main
from handyrl_amd.rollout import PlayerReplay, PlayerStreamGenerator
from tests.test_player_eval_entry import _args
from tests.test_player_eval_rollout import SEED
from tests.test_player_stream_rollout import ring_rows

pytestmark = pytest.mark.gpu

E, G = 8, 24


def _wrapper(cuda, seed=11):
    torch.manual_seed(seed)
    return hnn.GeeseInference(hnn.accelerate(GeeseNet().to(cuda)).eval(), precision='bf16')


@pytest.mark.parametrize('kw', [{}, {'opponent': 'rule'}], ids=['random', 'rule'])
def test_evaluator_plays_its_games(cuda, kw):
    b = HungryGeeseBatch(E, cuda)
    b.seed(SEED)
    res = PlayerEvaluator(b, _wrapper(cuda), seed=SEED, **kw).evaluate(G)
    assert res['games'] == G and sum(res['results'].values()) == G
    assert int(res['length'].max()) > 1


def test_stream_generator_records_the_policy_it_sampled_from(cuda):
    w = _wrapper(cuda)
    N = 16
    env = HungryGeeseBatch(E, cuda, seed=5)
    replay = PlayerReplay(N, env.MAX_PLIES, env.OBS_SHAPE, env.A, env.P, cuda, obs_dtype=torch.uint8)
    gen = PlayerStreamGenerator(env, w, replay, gamma=0.8, seed=5)
    gen.generate(N)
    rec = ring_rows(replay, gen, list(range(N)))
    turn = rec['tmask']                                         # (N, T, P): the plies a player moved at
    assert int(turn.sum()) > N
    obs = rec['obs'][turn].float().to(cuda)
    with torch.no_grad(), w.inference_session():
        logits = w(obs)['policy'].cpu()
    again = torch.softmax(logits - rec['amask'][turn], -1)
    recorded = torch.softmax(rec['policy'][turn], -1)
    a = rec['action'][turn].view(-1, 1)
    torch.testing.assert_close(recorded.gather(1, a), again.gather(1, a), rtol=0, atol=1e-6)


def test_eval_entry_takes_fused_bf16(cuda, tmp_path):
    torch.manual_seed(4)
    torch.save(GeeseNet().state_dict(), tmp_path / 'a.pth')
    logs = []
    res = eval_main(_args(inference='fused_bf16'), [str(tmp_path / 'a.pth'), str(G), str(E)], device=cuda,
                    log=logs.append)
    assert res['games'] == G and logs[-1].startswith('total ')
