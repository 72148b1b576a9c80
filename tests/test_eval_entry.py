"""Evaluation from the entry points: ``main --eval`` on a checkpoint and the per-epoch win rate of ``train_main``,
which must leave training exactly as it is."""

import os
import re

import pytest
import torch
import yaml

import handyrl_amd.main as hm
from handyrl_amd.evaluation import eval_games, eval_main
from handyrl_amd.main import load_config, train_main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_loss(outputs, batch, args):
    from oracle.learner import loss_from_outputs
    losses, dcnt = loss_from_outputs(outputs, batch, args)
    return losses, torch.tensor(dcnt)


def _small(env='TicTacToe', **kw):
    args = load_config(os.path.join(ROOT, 'config.yaml'))
    args['env_args']['env'] = env
    args['train_args'].update(update_episodes=16, minimum_episodes=32, maximum_episodes=64, batch_size=8,
                              forward_steps=6, epochs=2)
    args['train_args'].update(kw)
    return args


def test_repo_config_leaves_evaluation_off():
    targs = load_config(os.path.join(ROOT, 'config.yaml'))['train_args']
    assert not any(k in targs for k in ('eval_rate', 'eval_temperature', 'eval_slots'))
    text = open(os.path.join(ROOT, 'config.yaml')).read()
    for k in ('eval_rate', 'eval_temperature', 'eval_slots'):
        assert re.search(r'#\s*%s:' % k, text), k


def test_eval_cli_on_a_saved_checkpoint(tmp_path, monkeypatch, capsys):
    """``main --eval MODEL N SLOTS`` reads config.yaml from the working directory, loads the checkpoint into
    env.net() and prints the result table and the win rate in the reference's ``total`` form."""
    from handyrl_amd.envs.tictactoe import SimpleConv2dModel
    torch.manual_seed(4)
    torch.save(SimpleConv2dModel().state_dict(), tmp_path / 'm.pth')
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(_small()))
    monkeypatch.chdir(tmp_path)
    logs = []
    res = eval_main(load_config('config.yaml'), ['m.pth', '20', '6'], device=torch.device('cpu'), log=logs.append)
    assert res['games'] == 20 and sum(res['results'].values()) == 20 and 0.0 <= res['win_rate'] <= 1.0
    assert logs[-1] == 'total %s %s' % (res['results'], res['win_rate'])
    assert list(res['results']) == sorted(res['results'], reverse=True)
    # through main(): the same numbers on stdout
    import handyrl_amd.evaluation as he
    monkeypatch.setattr(he, 'eval_main', lambda args, argv: eval_main(args, argv, device=torch.device('cpu')))
    assert hm.main(['--eval', 'm.pth', '20', '6']) == 0
    assert logs[-1] in capsys.readouterr().out
    assert hm.main([]) == 1


def test_train_main_logs_the_win_rate_and_trains_the_same(tmp_path, env='TicTacToe'):
    """With eval_rate set every epoch line ends in the win rate and there are still exactly ``epochs`` lines; the
    final weights, Adam state and BatchNorm statistics equal a run without evaluation bit for bit (oracle loss)."""
    kw = {}
    runs = {}
    for rate in (None, 0.5):
        args = _small(env, **kw)
        if rate is not None:
            args['train_args'].update(eval_rate=rate, eval_slots=3)
        logs, state = [], {}
        real = hm.Trainer

        def spy(*a, **k):
            state['trainer'] = real(*a, **k)
            return state['trainer']
        hm.Trainer = spy
        try:
            model = train_main(args, device=torch.device('cpu'), loss_fn=_oracle_loss,
                               model_dir=str(tmp_path / str(rate)), log=logs.append)
        finally:
            hm.Trainer = real
        runs[rate] = (logs, model, state['trainer'])
    epochs = _small(env, **kw)['train_args']['epochs']
    plain, evald = runs[None][0], runs[0.5][0]
    assert len(plain) == len(evald) == epochs
    n = eval_games(0.5, _small(env, **kw)['train_args']['update_episodes'])
    for a, b in zip(plain, evald):
        assert 'win rate' not in a
        m = re.fullmatch(r'(epoch .*\)), win rate (\d\.\d{3}) \((\d+\.\d) / (\d+)\)', b)
        assert m and int(m.group(4)) == n and abs(float(m.group(3)) - float(m.group(2)) * n) <= 0.06, b
        assert re.sub(r'\(\d+\.\ds\)', '', m.group(1)) == re.sub(r'\(\d+\.\ds\)', '', a)
    _same_training(runs[None], runs[0.5])


def _same_training(a, b):
    sa, sb = a[1].state_dict(), b[1].state_dict()
    assert set(sa) == set(sb)
    for k in sa:                                    # weights and BatchNorm running statistics
        assert torch.equal(sa[k], sb[k]), k
    oa, ob = _optimizer_tensors(a[2]), _optimizer_tensors(b[2])
    assert len(oa) == len(ob) and len(oa) > 0
    for x, y in zip(oa, ob):
        assert torch.equal(x.cpu(), y.cpu())


def _optimizer_tensors(trainer):
    """Every tensor of the learner's Adam state (torch.optim.Adam on the CPU, the fused tail on the GPU)."""
    return list(trainer.learner._opt_state())


def test_simultaneous_env_with_eval_rate_raises(tmp_path):
    args = _small('ParallelTicTacToe', eval_rate=0.5)
    with pytest.raises(ValueError, match='simultaneous'):
        train_main(args, device=torch.device('cpu'), loss_fn=_oracle_loss, model_dir=str(tmp_path),
                   log=lambda *_: None)
    # without the key the same configuration trains as before
    args = _small('ParallelTicTacToe', epochs=1)
    train_main(args, device=torch.device('cpu'), loss_fn=_oracle_loss, model_dir=str(tmp_path), log=lambda *_: None)
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(_small('ParallelTicTacToe')))
    with pytest.raises(ValueError, match='simultaneous'):
        eval_main(_small('ParallelTicTacToe'), ['none.pth'], device=torch.device('cpu'))


@pytest.mark.gpu
def test_train_main_gpu_with_and_without_evaluation(tmp_path, cuda):
    """The HIP loss and learner step: evaluation after each epoch changes neither weights, Adam state nor BatchNorm
    statistics, and every epoch line carries the win rate."""
    runs = {}
    for rate in (None, 0.5):
        args = _small()
        if rate is not None:
            args['train_args'].update(eval_rate=rate)
        logs, state = [], {}
        real = hm.Trainer

        def spy(*a, **k):
            state['trainer'] = real(*a, **k)
            return state['trainer']
        hm.Trainer = spy
        try:
            model = train_main(args, device=cuda, model_dir=str(tmp_path / str(rate)), log=logs.append)
        finally:
            hm.Trainer = real
        runs[rate] = (logs, model, state['trainer'])
    assert len(runs[None][0]) == len(runs[0.5][0]) == 2
    assert all('win rate' in line for line in runs[0.5][0]) and not any('win rate' in line for line in runs[None][0])
    _same_training(runs[None], runs[0.5])
