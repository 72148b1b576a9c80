"""rollout.PlayerStreamGenerator on the GPU: the launches against their torch formulation inside the generator, the
captured step against the eager one, a recapture that keeps the games, the Geese referee of
tests/test_player_stream_rollout.py on GPU rows, and ``main.train_main`` with ``self_play: stream``."""

import os

import pytest
import torch

from handyrl_amd import rollout
from tests.test_player_stream_rollout import GeeseGame, bookkeeping, make, referee, ring_rows, same

pytestmark = pytest.mark.gpu

CASES = [('geese', 6, 16, 8), ('ptt', 7, 64, 32)]


def _run(name, cuda, E, N, n, move=False, **kw):
    """Two calls of a fresh generator; ``move``: the net's tensors move in between (same values)."""
    gen, replay, _ = make(name, cuda, E, N, seed=5, **kw)
    outs = [gen.generate(n)]
    graphs = gen._graphs
    if move:
        for p in list(gen.net.parameters()) + list(gen.net.buffers()):
            p.data = p.data.clone()
    outs.append(gen.generate(n))
    emitted = bookkeeping(gen, replay, outs)
    return gen, graphs, emitted, ring_rows(replay, gen, list(range(N)))


@pytest.mark.parametrize('name,E,N,n', CASES)
def test_fused_stream_equals_torch_formulation(cuda, monkeypatch, name, E, N, n):
    recs = []
    for fused in (True, False):
        monkeypatch.setattr(rollout, 'FUSED_STREAM', fused)
        gen, graphs, emitted, rows = _run(name, cuda, E, N, n)
        assert gen._graphs is graphs and graphs is not None      # the second call replays the first one's capture
        assert gen._state()['obs'].dtype == (torch.uint8 if name == 'geese' else torch.float32)
        recs.append((emitted, rows))
    assert recs[0][0] == recs[1][0] >= 2 * n
    same(recs[0][1], recs[1][1])         # every row, the unwritten ones included


@pytest.mark.parametrize('name,E,N,n', CASES)
def test_graph_equals_eager_and_recapture_keeps_the_games(cuda, name, E, N, n):
    gen, graphs, emitted, want = _run(name, cuda, E, N, n)
    assert graphs is not None and gen._graphs is graphs
    gen, graphs, eager_emitted, eager = _run(name, cuda, E, N, n, graph=False)
    assert graphs is None and gen._graphs is None
    assert eager_emitted == emitted
    same(want, eager)                    # capture and warm-up left no trace
    gen, graphs, moved_emitted, moved = _run(name, cuda, E, N, n, move=True)
    assert gen._graphs is not graphs     # captured again, and the games in flight went on
    assert moved_emitted == emitted
    same(want, moved)


def test_geese_rows_are_refereed(cuda):
    gen, replay, cpu = make('geese', cuda, 6, 64, seed=3)
    out = gen.generate(24)
    emitted = bookkeeping(gen, replay, [out])
    assert 24 <= emitted <= 64
    lengths = referee(GeeseGame, gen, replay, cpu, list(range(emitted)))
    assert out['env_steps'] == sum(lengths)


def test_train_main_streams_geese(cuda, tmp_path):
    from handyrl_amd.main import train_main
    args = {'env_args': {'env': 'Geese'},
            'train_args': {'turn_based_training': False, 'observation': False, 'update_episodes': 8,
                           'minimum_episodes': 8, 'maximum_episodes': 32, 'batch_size': 4, 'forward_steps': 4,
                           'epochs': 1, 'seed': 4, 'self_play': 'stream'}}
    logs = []
    train_main(args, device=cuda, model_dir=str(tmp_path), log=logs.append)
    assert os.path.isfile(os.path.join(str(tmp_path), '1.pth')) and len(logs) == 1
    # an alternating env with observation is still the lockstep generator's
    bad = {'env_args': {'env': 'TicTacToe'},
           'train_args': {**args['train_args'], 'turn_based_training': True, 'observation': True}}
    with pytest.raises(ValueError, match='self_play'):
        train_main(bad, device=cuda, model_dir=str(tmp_path / 'bad'), log=logs.append)
