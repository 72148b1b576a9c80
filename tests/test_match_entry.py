"""Matches from the entry points: ``main --eval-match A B`` on two checkpoints and ``eval_opponent`` in train_args
(a fixed anchor, or the previous epoch's model), which must leave training exactly as it is."""

import ast
import os
import re

import pytest
import torch
import yaml

import handyrl_amd.evaluation as he
import handyrl_amd.main as hm
from handyrl_amd.evaluation import eval_games, eval_match_main, wp_func
from handyrl_amd.main import load_config, train_main
from tests.test_eval_entry import _oracle_loss, _same_training, _small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _checkpoints(tmp_path):
    from handyrl_amd.envs.tictactoe import SimpleConv2dModel
    for name, seed in (('a.pth', 4), ('b.pth', 5)):
        torch.manual_seed(seed)
        torch.save(SimpleConv2dModel().state_dict(), tmp_path / name)


def test_repo_config_documents_the_keys_and_leaves_them_off():
    targs = load_config(os.path.join(ROOT, 'config.yaml'))['train_args']
    text = open(os.path.join(ROOT, 'config.yaml')).read()
    for k in ('eval_opponent', 'eval_opening_plies'):
        assert k not in targs and re.search(r'#\s*%s:' % k, text), k


def test_eval_match_cli_on_two_checkpoints(tmp_path, monkeypatch, capsys):
    """The reference's evaluate_mp tables: per agent ``default-F`` (agent 0 moves first: the even game numbers,
    (N + 1) // 2 of them), ``default-S`` and ``total``, each a sorted {outcome: count} table and its win rate."""
    _checkpoints(tmp_path)
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(_small()))
    monkeypatch.chdir(tmp_path)
    logs = []
    res = eval_match_main(load_config('config.yaml'), ['a.pth', 'b.pth', '21', '6'], device=torch.device('cpu'),
                          log=logs.append)
    assert logs[0] == '6 slots, 21 games'
    assert res['games'] == 21 and sum(res['results'].values()) == 21 == sum(res['opponent_results'].values())
    assert [l.split(' ')[0] for l in logs[1:]] == ['---agent', 'default-F', 'default-S', 'total'] * 2
    assert logs[1] == '---agent 0---' and logs[5] == '---agent 1---'
    tables = []
    for line in logs[2:5] + logs[6:9]:
        m = re.fullmatch(r'(default-F|default-S|total) (\{.*\}) (\S+)', line)
        table = ast.literal_eval(m.group(2))
        assert list(table) == sorted(table, reverse=True) and float(m.group(3)) == wp_func(table), line
        tables.append(table)
    assert [sum(t.values()) for t in tables] == [11, 10, 21, 11, 10, 21]
    assert tables[2] == res['results'] and tables[5] == res['opponent_results']
    assert float(logs[4].split(' ')[-1]) == res['win_rate'] and float(logs[8].split(' ')[-1]) == res['opponent_win_rate']
    for mine, theirs in zip(tables[:3], tables[3:]):               # zero-sum, table by table
        assert {-k + 0.0: v for k, v in mine.items()} == theirs
    # the first-mover tables are those of the even game numbers
    first = {}
    for g in range(0, 21, 2):
        o = float(res['outcome'][g, 0]) + 0.0
        first[o] = first.get(o, 0) + 1
    assert first == tables[0]
    # a checkpoint against itself, the default game count's argument left to NUM_GAMES alone
    res = eval_match_main(load_config('config.yaml'), ['a.pth', 'a.pth', '8'], device=torch.device('cpu'),
                          log=logs.append)
    assert sum(res['results'].values()) == 8
    # through main(): the same lines on stdout
    monkeypatch.setattr(he, 'eval_match_main',
                        lambda args, argv: eval_match_main(args, argv, device=torch.device('cpu')))
    assert hm.main(['--eval-match', 'a.pth', 'b.pth', '21', '6']) == 0
    out = capsys.readouterr().out
    assert all(line in out for line in logs[1:9])
    with pytest.raises(ValueError, match='two checkpoints'):
        eval_match_main(load_config('config.yaml'), ['a.pth'], device=torch.device('cpu'))


def _train(tmp_path, tag, device=torch.device('cpu'), loss_fn=_oracle_loss, spy_eval=None, **kw):
    args = _small(**kw)
    logs, state = [], {}
    real = hm.Trainer

    def spy(*a, **k):
        state['trainer'] = real(*a, **k)
        return state['trainer']
    hm.Trainer = spy
    real_eval = he.DeviceEvaluator.evaluate
    if spy_eval is not None:
        def evaluate(self, games, *a, **k):
            spy_eval(self)
            return real_eval(self, games, *a, **k)
        he.DeviceEvaluator.evaluate = evaluate
    try:
        model = train_main(args, device=device, loss_fn=loss_fn, model_dir=str(tmp_path / tag), log=logs.append)
    finally:
        hm.Trainer = real
        he.DeviceEvaluator.evaluate = real_eval
    return logs, model, state['trainer']


LINE = r'(epoch .*\)), win rate (\d\.\d{3}) \((\d+\.\d) / (\d+)\) vs (\S+)'


def _check_lines(plain, lines, vs, n):
    assert len(plain) == len(lines) == 2
    for a, b in zip(plain, lines):
        m = re.fullmatch(LINE, b)
        assert m and int(m.group(4)) == n and abs(float(m.group(3)) - float(m.group(2)) * n) <= 0.06, b
        assert m.group(5) == vs
        assert re.sub(r'\(\d+\.\ds\)', '', m.group(1)) == re.sub(r'\(\d+\.\ds\)', '', a)


def test_eval_opponent_anchor_and_previous_train_the_same(tmp_path):
    """Two epochs without evaluation, against a checkpoint and against ``previous``: the epoch lines end in
    ``vs <path>`` / ``vs previous``; weights, Adam state and BatchNorm statistics are bit-identical in all three; the
    anchor keeps its weights; ``previous`` holds the starting weights at epoch 1, models/1.pth at epoch 2 and
    models/2.pth afterwards."""
    _checkpoints(tmp_path)
    anchor = str(tmp_path / 'a.pth')
    n = eval_games(0.5, 16)
    plain = _train(tmp_path, 'plain')
    seen = []
    fixed = _train(tmp_path, 'anchor', eval_rate=0.5, eval_slots=3, eval_opponent=anchor,
                   spy_eval=lambda ev: seen.append((ev.opening_plies, {k: v.clone() for k, v in
                                                                       ev.opponent.state_dict().items()})))
    _check_lines(plain[0], fixed[0], anchor, n)
    _same_training(plain, fixed)
    want = torch.load(anchor, weights_only=True)
    assert len(seen) == 2
    for opening, state in seen:
        assert opening == 2 and all(torch.equal(state[k], want[k]) for k in want)
    seen = []
    evaluators = []
    prev = _train(tmp_path, 'previous', eval_rate=0.5, eval_slots=3, eval_opponent='previous', eval_opening_plies=1,
                  spy_eval=lambda ev: (evaluators.append(ev), seen.append(
                      (ev.opening_plies, {k: v.clone() for k, v in ev.opponent.state_dict().items()}))))
    _check_lines(plain[0], prev[0], 'previous', n)
    _same_training(plain, prev)
    torch.manual_seed(_small()['train_args']['seed'])
    from handyrl_amd.envs.tictactoe import SimpleConv2dModel
    start = SimpleConv2dModel().state_dict()
    first = torch.load(tmp_path / 'previous' / '1.pth', weights_only=True)
    last = torch.load(tmp_path / 'previous' / '2.pth', weights_only=True)
    assert [o for o, _ in seen] == [1, 1]
    for got, state in ((seen[0][1], start), (seen[1][1], first), (evaluators[-1].opponent.state_dict(), last)):
        assert set(got) == set(state) and all(torch.equal(got[k].cpu(), state[k]) for k in state)
    assert any(not torch.equal(first[k], last[k]) for k in first)
    # random: nothing new is constructed
    rnd = _train(tmp_path, 'random', eval_rate=0.5, eval_slots=3, eval_opponent='random',
                 spy_eval=lambda ev: evaluators.append(ev))
    assert evaluators[-1].opponent is None and all(re.search(r'/ %d\)$' % n, line) for line in rnd[0])


def test_previous_after_a_restart_is_the_loaded_checkpoint(tmp_path):
    _train(tmp_path, 'run', epochs=1)
    seen = []
    _train(tmp_path, 'run', epochs=1, restart_epoch=1, eval_rate=0.5, eval_slots=3, eval_opponent='previous',
           spy_eval=lambda ev: seen.append({k: v.clone() for k, v in ev.opponent.state_dict().items()}))
    want = torch.load(tmp_path / 'run' / '1.pth', weights_only=True)
    assert len(seen) == 1 and all(torch.equal(seen[0][k], want[k]) for k in want)


def test_bad_opponents_raise_at_start_up(tmp_path):
    with pytest.raises(FileNotFoundError, match='eval_opponent'):
        _train(tmp_path, 'x', eval_rate=0.5, eval_opponent=str(tmp_path / 'none.pth'))
    assert not (tmp_path / 'x').exists()                 # before any epoch
    args = _small('ParallelTicTacToe', eval_rate=0.5, eval_opponent='previous')
    with pytest.raises(ValueError, match='simultaneous'):
        train_main(args, device=torch.device('cpu'), loss_fn=_oracle_loss, model_dir=str(tmp_path / 'y'),
                   log=lambda *_: None)
    with pytest.raises(ValueError, match='simultaneous'):
        eval_match_main(_small('ParallelTicTacToe'), ['a.pth', 'b.pth'], device=torch.device('cpu'))
    # without eval_rate the key is not looked at: no new code runs
    _train(tmp_path, 'z', epochs=1, eval_opponent=str(tmp_path / 'none.pth'))


@pytest.mark.gpu
def test_train_main_gpu_with_and_without_an_opponent(tmp_path, cuda):
    """The HIP loss and learner step, the accelerated opponent: ``previous`` changes neither weights, Adam state nor
    BatchNorm statistics, and every epoch line names the opponent."""
    plain = _train(tmp_path, 'plain', device=cuda, loss_fn=None)
    prev = _train(tmp_path, 'previous', device=cuda, loss_fn=None, eval_rate=0.5, eval_opponent='previous')
    _check_lines(plain[0], prev[0], 'previous', eval_games(0.5, 16))
    _same_training(plain, prev)
