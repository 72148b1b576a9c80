"""The rule-based Geese opponent from the entry points: ``main --eval-rulebase`` on a saved GeeseNet checkpoint and the
per-epoch win rate of ``train_main`` with ``eval_opponent: rulebase``, which must leave training exactly as it is;
an env without a rule-based agent raises at start-up."""

import pytest
import torch
import yaml

import handyrl_amd.evaluation as he
import handyrl_amd.main as hm
from handyrl_amd.evaluation import eval_games, eval_main, eval_rulebase_main
from handyrl_amd.main import TRAIN_DEFAULTS, train_main
from tests.test_eval_entry import _oracle_loss, _same_training
from tests.test_player_eval_entry import _args, _check_lines, _checkpoints, _table, _train

CPU = torch.device('cpu')


def test_eval_rulebase_cli_on_a_saved_geese_checkpoint(tmp_path, monkeypatch, capsys):
    """Agent 0 = the model on seat g mod 4, agent 1 = the rule's three seats; ``--eval-match``'s lines on Geese."""
    _checkpoints(tmp_path)
    logs = []
    res = eval_rulebase_main(_args(), [str(tmp_path / 'a.pth'), '6', '4'], device=CPU, log=logs.append)
    assert logs[0] == '4 slots, 6 games'
    assert [l.split(' ')[0] for l in logs[1:]] == ['---agent', 'default', 'total'] * 2
    assert logs[1] == '---agent 0---' and logs[4] == '---agent 1---'
    assert _table(logs[2], 'default') == _table(logs[3], 'total') == res['results']
    assert _table(logs[5], 'default') == _table(logs[6], 'total') == res['opponent_results']
    assert sum(res['results'].values()) == 6 and sum(res['opponent_results'].values()) == 18
    assert res['seat'].tolist() == [0, 1, 2, 3, 0, 1]
    # the same games whatever the slot count; other games than against random agents
    again = eval_rulebase_main(_args(), [str(tmp_path / 'a.pth'), '6', '2'], device=CPU, log=lambda *_: None)
    assert torch.equal(again['outcome'], res['outcome']) and torch.equal(again['length'], res['length'])
    rand = eval_main(_args(), [str(tmp_path / 'a.pth'), '6', '4'], device=CPU, log=lambda *_: None)
    assert int(res['length'].sum()) > int(rand['length'].sum())          # greedy geese last longer
    with pytest.raises(ValueError, match='checkpoint'):
        eval_rulebase_main(_args(), [], device=CPU)
    # through main(): config.yaml of the working directory, the same lines on stdout
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(_args()))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(he, 'eval_rulebase_main', lambda args, argv: eval_rulebase_main(args, argv, device=CPU))
    assert hm.main(['--eval-rulebase', 'a.pth', '6', '4']) == 0
    out = capsys.readouterr().out
    assert all(line in out for line in logs)
    assert hm.main(['--no-such-flag']) == 1
    assert '--eval-rulebase MODEL_PATH [NUM_GAMES] [SLOTS]' in capsys.readouterr().out


def test_eval_rulebase_needs_an_env_with_a_rule(tmp_path):
    args = _args()
    args['env_args']['env'] = 'TicTacToe'
    with pytest.raises(ValueError, match='TicTacToe'):
        eval_rulebase_main(args, [str(tmp_path / 'a.pth')], device=CPU)


def test_train_main_logs_vs_rulebase_and_trains_the_same(tmp_path):
    """``eval_opponent: rulebase`` beside ``eval_rate`` and ``eval_simultaneous``: every epoch line ends ``vs
    rulebase``; weights, Adam state and BatchNorm statistics equal the run without the keys bit for bit; no net is
    constructed for the opponent."""
    n = eval_games(0.5, 4)
    plain = _train(tmp_path, 'plain')
    seen = []
    rule = _train(tmp_path, 'rule', eval_rate=0.5, eval_simultaneous=True, eval_slots=2, eval_opponent='rulebase',
                  spy_eval=lambda ev: seen.append((ev.env.E, ev.env._seed, ev.seed, ev.opponent, ev.rule,
                                                   ev.opening_plies)))
    _check_lines(plain[0], rule[0], n, vs='rulebase')
    _same_training(plain, rule)
    assert seen == [(2, 2, 2, None, 'greedy_players', 0)] * 2


def test_rulebase_on_an_env_without_a_rule_raises_at_start_up(tmp_path):
    targs = {**TRAIN_DEFAULTS, 'update_episodes': 4, 'minimum_episodes': 4, 'maximum_episodes': 8, 'batch_size': 2,
             'forward_steps': 4, 'epochs': 1, 'eval_rate': 0.5, 'eval_opponent': 'rulebase'}
    with pytest.raises(ValueError, match='TicTacToe'):
        train_main({'env_args': {'env': 'TicTacToe'}, 'train_args': targs}, device=CPU, loss_fn=_oracle_loss,
                   model_dir=str(tmp_path / 'x'), log=lambda *_: None)
    assert not (tmp_path / 'x').exists()                 # before any epoch


@pytest.mark.gpu
def test_train_main_gpu_logs_vs_rulebase_and_trains_the_same(tmp_path, cuda):
    """The HIP learner step, the accelerated net and the captured evaluation graph with hrl_geese_greedy in it."""
    runs = []
    for tag, kw in (('plain', {}),
                    ('rule', {'eval_rate': 0.5, 'eval_simultaneous': True, 'eval_opponent': 'rulebase'})):
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
    _check_lines(runs[0][0], runs[1][0], eval_games(0.5, 8), vs='rulebase')
    _same_training(runs[0], runs[1])
