"""``main --eval-league``: a directory of checkpoints played as a round robin from the entry point (CPU device)."""

import os
import re

import pytest
import torch
import yaml

import handyrl_amd.evaluation as he
import handyrl_amd.main as hm
from handyrl_amd.evaluation import LeagueEvaluator, eval_league_main, league_paths, load_net
from handyrl_amd.main import load_config
from handyrl_amd.rollout import TicTacToeBatch
from tests.test_eval_entry import _small

CPU = torch.device('cpu')


def _checkpoints(tmp_path):
    from handyrl_amd.envs.tictactoe import SimpleConv2dModel
    models = tmp_path / 'models'
    models.mkdir()
    for name, seed in (('2.pth', 4), ('10.pth', 5), ('1.pth', 6)):
        torch.manual_seed(seed)
        torch.save(SimpleConv2dModel().state_dict(), models / name)
    (models / 'latest.txt').write_text('not a checkpoint')
    (models / 'best.pth').write_bytes(b'')            # not <integer>.pth: left out
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(_small(seed=3)))
    return models


def test_a_directory_expands_in_epoch_order(tmp_path):
    models = _checkpoints(tmp_path)
    want = [str(models / ('%d.pth' % e)) for e in (1, 2, 10)]
    assert league_paths([str(models)]) == want
    assert league_paths([want[2], str(models)]) == [want[2]] + want


def test_eval_league_cli_on_a_directory(tmp_path, monkeypatch, capsys):
    models = _checkpoints(tmp_path)
    monkeypatch.chdir(tmp_path)
    args = load_config('config.yaml')
    logs = []
    res = eval_league_main(args, ['models', '6', '12'], device=CPU, log=logs.append)
    assert logs[0] == '3 agents, 3 pairings, 12 slots, 6 games per pairing'
    paths = [os.path.join('models', '%d.pth' % e) for e in (1, 2, 10)]
    for k, path in enumerate(paths):
        m = re.fullmatch(r'agent %d (\S+) rating ([+-]\d+\.\d) win rate (\d\.\d{3}) games (\d+)' % k, logs[1 + k])
        assert m and m.group(1) == path, logs[1 + k]
        assert abs(float(m.group(2)) - float(res['rating'][k])) <= 0.05 + 1e-9
        assert abs(float(m.group(3)) - float(res['win_rate'][k])) <= 0.0005 + 1e-9
        assert int(m.group(4)) == 12
    # the cross table: a header, then row i with i's win rate against j
    assert logs[4].startswith('cross table')
    assert logs[5].split() == ['0', '1', '2']
    for i in range(3):
        cells = logs[6 + i].split()
        assert cells[0] == str(i) and cells[1 + i] == '-'
        for j in range(3):
            if i != j:
                assert abs(float(cells[1 + j]) - float(res['score'][i, j]) / 6) <= 0.0005 + 1e-9
    assert len(logs) == 9
    # the returned dict is a direct run's: the same nets, arguments from train_args, 12 slots
    from handyrl_amd.environment import make_env, prepare_env
    prepare_env(args['env_args'])
    env = make_env(args['env_args'])
    nets = [load_net(env, p, CPU) for p in paths]
    direct = LeagueEvaluator(TicTacToeBatch(12, CPU), nets, observation=False, temperature=0.0, opening_plies=2,
                             seed=3).evaluate(6)
    assert sorted(direct) == sorted(res)
    assert sorted(res) == ['env_steps', 'games', 'length', 'outcome', 'pairings', 'plies', 'rating', 'score',
                           'win_rate']
    for k in direct:
        if isinstance(direct[k], torch.Tensor):
            assert torch.equal(direct[k], res[k]), k
        else:
            assert direct[k] == res[k], k
    assert res['pairings'] == [(0, 1), (0, 2), (1, 2)] and res['outcome'].shape == (3, 6, 2)


def test_trailing_integers_are_games_and_slots(tmp_path, monkeypatch):
    models = _checkpoints(tmp_path)
    monkeypatch.chdir(tmp_path)
    args = load_config('config.yaml')
    a, b = str(models / '1.pth'), str(models / '2.pth')
    logs = []
    res = eval_league_main(args, [a, b, '5'], device=CPU, log=logs.append)          # NUM_GAMES alone
    assert logs[0] == '2 agents, 1 pairings, 6 slots, 5 games per pairing'            # S capped at 5 rounded up to even
    assert res['outcome'].shape == (1, 5, 2)
    logs = []
    eval_league_main(args, [a, b, '8', '7'], device=CPU, log=logs.append)            # 7 rounds down to 6 = 3 * 2Q
    assert logs[0] == '2 agents, 1 pairings, 6 slots, 8 games per pairing'
    logs = []
    eval_league_main(args, ['models', '4', '1'], device=CPU, log=logs.append)        # at least 2Q = 6
    assert logs[0] == '3 agents, 3 pairings, 6 slots, 4 games per pairing'
    # a file whose name is a number is a path, not a count
    torch.save(torch.load(a, weights_only=True), tmp_path / '7')
    logs = []
    res = eval_league_main(args, [a, '7', '2'], device=CPU, log=logs.append)
    assert logs[0] == '2 agents, 1 pairings, 2 slots, 2 games per pairing' and logs[2].split()[2] == '7'
    with pytest.raises(ValueError, match='two checkpoints'):
        eval_league_main(args, [a, '5'], device=CPU)


def test_main_runs_the_mode(tmp_path, monkeypatch, capsys):
    _checkpoints(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(he, 'eval_league_main', lambda args, argv: eval_league_main(args, argv, device=CPU))
    assert hm.main(['--eval-league', 'models', '4', '6']) == 0
    out = capsys.readouterr().out
    assert '3 agents, 3 pairings, 6 slots, 4 games per pairing' in out and 'cross table' in out
    assert all(os.path.join('models', '%d.pth' % e) in out for e in (1, 2, 10))
    assert hm.main([]) == 1
    assert '--eval-league MODEL_OR_DIR' in capsys.readouterr().out
    assert '--eval-league MODEL_OR_DIR' in hm.__doc__


def test_a_missing_path_raises_before_any_game(tmp_path, monkeypatch):
    models = _checkpoints(tmp_path)
    monkeypatch.chdir(tmp_path)

    def never(*a, **k):
        raise AssertionError('a net was loaded or a game played')
    monkeypatch.setattr(he, 'load_net', never)
    monkeypatch.setattr(he.LeagueEvaluator, 'evaluate', never)
    with pytest.raises(FileNotFoundError, match='none.pth'):
        eval_league_main(load_config('config.yaml'), [str(models), 'none.pth', '4'], device=CPU)
    with pytest.raises(ValueError, match='simultaneous'):
        eval_league_main(_small('ParallelTicTacToe'), [str(models)], device=CPU)
