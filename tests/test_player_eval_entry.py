"""Hungry Geese from the entry points: ``main --eval`` and ``main --eval-match`` on saved GeeseNet checkpoints and the
per-epoch win rate of ``train_main`` with ``env: Geese`` and ``eval_simultaneous`` (against random agents and ``vs
previous``), which must leave training exactly as it is.  Without that key ``eval_rate`` on Geese raises as it always
has, and ``--eval-league`` on Geese stays refused."""

import ast
import re

import pytest
import torch
import yaml

import handyrl_amd.evaluation as he
import handyrl_amd.main as hm
from handyrl_amd.envs.geese import GeeseNet
from handyrl_amd.evaluation import PlayerEvaluator, eval_games, eval_league_main, eval_main, eval_match_main, wp_func
from handyrl_amd.main import TRAIN_DEFAULTS, train_main
from tests.test_eval_entry import _oracle_loss, _same_training

CPU = torch.device('cpu')
THIRDS = {float(torch.tensor(k / 3, dtype=torch.float32)) for k in range(-3, 4)}


def _args(**kw):
    """The smallest settings that train: solo training as in the README's Geese config."""
    targs = {**TRAIN_DEFAULTS, 'turn_based_training': False, 'observation': False, 'update_episodes': 4,
             'minimum_episodes': 4, 'maximum_episodes': 8, 'batch_size': 2, 'forward_steps': 4, 'epochs': 2, 'seed': 2}
    targs.update(kw)
    return {'env_args': {'env': 'Geese'}, 'train_args': targs}


def _checkpoints(tmp_path):
    for name, seed in (('a.pth', 4), ('b.pth', 5)):
        torch.manual_seed(seed)
        torch.save(GeeseNet().state_dict(), tmp_path / name)


def _table(line, tag):
    m = re.fullmatch(r'%s (\{.*\}) (\S+)' % tag, line)
    assert m, line
    table = ast.literal_eval(m.group(1))
    assert list(table) == sorted(table, reverse=True) and set(table) <= THIRDS, line
    assert float(m.group(2)) == wp_func(table), line
    return table


def test_eval_cli_on_a_saved_geese_checkpoint(tmp_path, monkeypatch, capsys):
    _checkpoints(tmp_path)
    logs = []
    res = eval_main(_args(), [str(tmp_path / 'a.pth'), '7', '3'], device=CPU, log=logs.append)
    assert logs[0] == '3 slots, 7 games'
    assert res['games'] == 7 and res['outcome'].shape == (7, 4) and 'opponent_results' not in res
    assert _table(logs[-1], 'total') == res['results'] and sum(res['results'].values()) == 7
    # the games are Geese games 0 .. 6 under train_args' seed, whatever the slot count
    again = eval_main(_args(), [str(tmp_path / 'a.pth'), '7', '2'], device=CPU, log=lambda *_: None)
    assert torch.equal(again['outcome'], res['outcome']) and torch.equal(again['length'], res['length'])
    other = eval_main(_args(seed=3), [str(tmp_path / 'a.pth'), '7', '3'], device=CPU, log=lambda *_: None)
    assert not torch.equal(other['length'], res['length']) or not torch.equal(other['outcome'], res['outcome'])
    # through main(): config.yaml of the working directory, the same line on stdout
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(_args()))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(he, 'eval_main', lambda args, argv: eval_main(args, argv, device=CPU))
    assert hm.main(['--eval', 'a.pth', '7', '3']) == 0
    assert logs[-1] in capsys.readouterr().out


def test_eval_match_cli_on_two_geese_checkpoints(tmp_path):
    """Agent 0 on seat g mod 4, agent 1 on the three other seats; per agent one ``default`` line and the ``total``
    line of the reference's evaluate_mp (no -F / -S patterns: it has those for two-player games only)."""
    _checkpoints(tmp_path)
    logs = []
    res = eval_match_main(_args(), [str(tmp_path / 'a.pth'), str(tmp_path / 'b.pth'), '6', '4'], device=CPU,
                          log=logs.append)
    assert logs[0] == '4 slots, 6 games'
    assert [l.split(' ')[0] for l in logs[1:]] == ['---agent', 'default', 'total'] * 2
    assert logs[1] == '---agent 0---' and logs[4] == '---agent 1---'
    assert _table(logs[2], 'default') == _table(logs[3], 'total') == res['results']
    assert _table(logs[5], 'default') == _table(logs[6], 'total') == res['opponent_results']
    assert sum(res['results'].values()) == 6 and sum(res['opponent_results'].values()) == 18
    assert res['seat'].tolist() == [0, 1, 2, 3, 0, 1]
    with pytest.raises(ValueError, match='two checkpoints'):
        eval_match_main(_args(), [str(tmp_path / 'a.pth')], device=CPU)


def test_eval_league_on_geese_stays_refused(tmp_path):
    _checkpoints(tmp_path)
    with pytest.raises(ValueError, match='simultaneous'):
        eval_league_main(_args(), [str(tmp_path / 'a.pth'), str(tmp_path / 'b.pth')], device=CPU)


def test_eval_rate_without_the_opt_in_raises_as_before(tmp_path):
    """``eval_rate`` alone on a simultaneous-move env keeps its start-up error; the error names the key."""
    for kw in ({}, {'eval_simultaneous': False}, {'eval_opponent': 'previous'}):
        with pytest.raises(ValueError, match='alternating-move envs.*eval_simultaneous'):
            train_main(_args(eval_rate=0.5, **kw), device=CPU, loss_fn=_oracle_loss, model_dir=str(tmp_path / 'x'),
                       log=lambda *_: None)
    assert not (tmp_path / 'x').exists()                 # before any epoch
    args = _args(eval_rate=0.5, eval_simultaneous=True)
    args['env_args']['env'] = 'ParallelTicTacToe'        # the key opens nothing for an env PlayerEvaluator is not for
    with pytest.raises(ValueError, match='simultaneous'):
        train_main(args, device=CPU, loss_fn=_oracle_loss, model_dir=str(tmp_path / 'y'), log=lambda *_: None)


def _train(tmp_path, tag, spy_eval=None, **kw):
    logs, state = [], {}
    real = hm.Trainer

    def spy(*a, **k):
        state['trainer'] = real(*a, **k)
        return state['trainer']
    hm.Trainer = spy
    real_eval = PlayerEvaluator.evaluate
    if spy_eval is not None:
        def evaluate(self, games, *a, **k):
            spy_eval(self)
            return real_eval(self, games, *a, **k)
        PlayerEvaluator.evaluate = evaluate
    try:
        model = train_main(_args(**kw), device=CPU, loss_fn=_oracle_loss, model_dir=str(tmp_path / tag),
                           log=logs.append)
    finally:
        hm.Trainer = real
        PlayerEvaluator.evaluate = real_eval
    return logs, model, state['trainer']


def _check_lines(plain, lines, n, vs=None):
    assert len(plain) == len(lines) == 2
    tail = r'' if vs is None else r' vs (\S+)'
    for a, b in zip(plain, lines):
        assert 'win rate' not in a
        m = re.fullmatch(r'(epoch .*\)), win rate (\d\.\d{3}) \((\d+\.\d) / (\d+)\)' + tail, b)
        assert m and int(m.group(4)) == n and abs(float(m.group(3)) - float(m.group(2)) * n) <= 0.06, b
        assert vs is None or m.group(5) == vs
        assert re.sub(r'\(\d+\.\ds\)', '', m.group(1)) == re.sub(r'\(\d+\.\ds\)', '', a)


def test_train_main_logs_the_win_rate_and_trains_the_same(tmp_path):
    """``env: Geese`` with ``eval_rate`` and ``eval_simultaneous``: every epoch line ends in the win rate; with
    ``eval_opponent: previous`` in ``vs previous``; weights, Adam state and BatchNorm statistics equal the run without
    the keys bit for bit."""
    n = eval_games(0.5, 4)
    plain = _train(tmp_path, 'plain')
    seen = []
    rated = _train(tmp_path, 'rated', eval_rate=0.5, eval_simultaneous=True, eval_slots=2,
                   spy_eval=lambda ev: seen.append((ev.env.E, ev.env._seed, ev.seed, ev.opponent)))
    _check_lines(plain[0], rated[0], n)
    _same_training(plain, rated)
    assert seen == [(2, 2, 2, None)] * 2                  # eval_slots slots, env and evaluator under the rank's seed
    seen = []
    prev = _train(tmp_path, 'previous', eval_rate=0.5, eval_simultaneous=True, eval_slots=2, eval_opponent='previous',
                  eval_opening_plies=1,
                  spy_eval=lambda ev: seen.append((ev.opening_plies,
                                                   {k: v.clone() for k, v in ev.opponent.state_dict().items()})))
    _check_lines(plain[0], prev[0], n, vs='previous')
    _same_training(plain, prev)
    torch.manual_seed(2)
    start = GeeseNet().state_dict()
    first = torch.load(tmp_path / 'previous' / '1.pth', weights_only=True)
    assert [o for o, _ in seen] == [1, 1]
    for got, want in ((seen[0][1], start), (seen[1][1], first)):
        assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)


@pytest.mark.gpu
def test_train_main_gpu_logs_the_win_rate_and_trains_the_same(tmp_path, cuda):
    """The HIP learner step and the accelerated nets: ``previous`` changes neither weights, Adam state nor BatchNorm
    statistics, and every epoch line names the opponent."""
    runs = []
    for tag, kw in (('plain', {}),
                    ('previous', {'eval_rate': 0.5, 'eval_simultaneous': True, 'eval_opponent': 'previous'})):
        logs, state = [], {}
        real = hm.Trainer

        def spy(*a, **k):
            state['trainer'] = real(*a, **k)
            return state['trainer']
        hm.Trainer = spy
        try:
            model = train_main(_args(update_episodes=8, minimum_episodes=8, maximum_episodes=16, **kw), device=cuda,
                               model_dir=str(tmp_path / tag), log=logs.append)
        finally:
            hm.Trainer = real
        runs.append((logs, model, state['trainer']))
    _check_lines(runs[0][0], runs[1][0], eval_games(0.5, 8), vs='previous')
    _same_training(runs[0], runs[1])
