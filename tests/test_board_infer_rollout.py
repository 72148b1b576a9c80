"""nn.BoardInference where the project plays TicTacToe: the generators, the evaluators, the league and main.py.

CPU: a wrapper on a CPU env runs the net's own forward, so every record equals the plain run's exactly.
GPU (E = 64 slots): every ring row of a streamed run is refereed on its own (rules on a one-game CPU env, the
Gumbel-max of the recorded policy, the recorded policy / value against the fp64 forward at 1e-5, returns exact -- the
referee of test_stream_rollout.py with the fp64 net); graph episodes equal eager ones; the lockstep and per-player
generators; the evaluator's greedy choice against the fp64 logits; the grouped league against the same wrappers
ungrouped (bit for bit) and its launch count independent of K; main.train_main with ``inference: fused``.
"""

import contextlib
import copy
import os

import pytest
import torch

from handyrl_amd import nn as hnn
from handyrl_amd.evaluation import DeviceEvaluator, LeagueEvaluator
from handyrl_amd.rollout import DeviceGenerator, DeviceReplay, StreamGenerator, TicTacToeBatch

from . import board_infer_util as util
from .test_main_entry import _oracle_loss, _small
from .test_stream_rollout import GAMMA, _bookkeeping, _rows, _same, _written_rows, referee

E = 64


class Net64:
    """The fp64 torch-CPU forward of a deep copy of ``net`` in eval mode, called like a net."""

    def __init__(self, net):
        self.net = copy.deepcopy(net).cpu().double().eval()

    @torch.no_grad()
    def __call__(self, obs, hidden=None):
        out = self.net(obs.double(), None)
        return {'policy': out['policy'], 'value': out['value']}


def _net(dev, seed=0, layers=3):
    return copy.deepcopy(util.seeded_net(layers, seed=seed)).to(dev).eval()


def _equal_tree(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            _equal_tree(a[k], b[k])
        elif isinstance(a[k], torch.Tensor):
            x, y = a[k].cpu(), b[k].cpu()
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), k
        else:
            assert a[k] == b[k], k


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('per_player', [False, True])
def test_cpu_generator_with_the_wrapper_equals_plain(per_player):
    cpu = torch.device('cpu')
    net = _net(cpu)
    eps = []
    for n in (net, hnn.BoardInference(net)):
        gen = DeviceGenerator(TicTacToeBatch(16, cpu), n, gamma=GAMMA, observation=per_player,
                              per_player=per_player)
        eps.append(gen.generate(generator=torch.Generator().manual_seed(3)))
    _equal_tree(eps[0], eps[1])


def test_cpu_evaluator_with_the_wrapper_equals_plain():
    cpu = torch.device('cpu')
    net, opp = _net(cpu), _net(cpu, seed=1)
    res = []
    for wrap in (lambda n: n, hnn.BoardInference):
        ev = DeviceEvaluator(TicTacToeBatch(6, cpu), wrap(net), seed=7, opponent=wrap(opp), opening_plies=2)
        res.append(ev.evaluate(20, trace=True))
    _equal_tree(res[0], res[1])


def test_cpu_league_group_takes_the_loop():
    """On the CPU (and with observation) the grouped branch is not taken: the result is the plain nets'."""
    cpu = torch.device('cpu')
    nets = [_net(cpu, seed=s) for s in range(3)]
    res = []
    for ns in (nets, hnn.board_inference_group(nets)):
        ev = LeagueEvaluator(TicTacToeBatch(12, cpu), ns, opening_plies=2, seed=5)
        res.append(ev.evaluate(6))
        assert ev._st['group'] is None
    assert torch.equal(res[0]['outcome'], res[1]['outcome']) and torch.equal(res[0]['score'], res[1]['score'])


def test_fused_key_raises_by_name_off_the_gpu(tmp_path):
    args = _small()
    args['train_args'].update(inference='fused', epochs=1)
    with pytest.raises(ValueError, match='inference'):
        hnn.configured_inference('fused', [_net('cpu')], torch.device('cpu'))
    with pytest.raises(ValueError, match='inference'):
        hnn.configured_inference('quick', [_net('cpu')], torch.device('cpu'))
    from handyrl_amd.main import train_main
    with pytest.raises(ValueError, match='inference'):
        train_main(args, device=torch.device('cpu'), loss_fn=_oracle_loss, model_dir=str(tmp_path),
                   log=lambda *_: None)
    nets = [_net('cpu')]
    assert hnn.configured_inference(None, nets, torch.device('cpu')) is nets


# ------------------------------------------------------------------------------------------------ GPU
def _stream(cuda, N, seed, **kw):
    net = _net(cuda)
    replay = DeviceReplay(N, TicTacToeBatch.MAX_PLIES, TicTacToeBatch.OBS_SHAPE, TicTacToeBatch.A, TicTacToeBatch.P,
                          cuda, obs_dtype=torch.uint8)
    gen = StreamGenerator(TicTacToeBatch(E, cuda), hnn.BoardInference(net), replay, gamma=GAMMA, seed=seed, **kw)
    return gen, replay, net


@pytest.mark.gpu
def test_stream_with_the_wrapper_is_refereed(cuda):
    gen, replay, net = _stream(cuda, 160, seed=5)
    out = gen.generate(200)
    emitted = _bookkeeping(gen, replay, [out])
    assert emitted >= 3 * E                                   # the slots restarted; the ring wrapped
    lengths = referee('tictactoe', gen, replay, Net64(net), _written_rows(replay))
    assert len(lengths) == 160 and all(5 <= n <= 9 for n in lengths)


@pytest.mark.gpu
def test_stream_graph_equals_eager_with_the_wrapper(cuda):
    recs = []
    for graph in (True, False):
        gen, replay, _ = _stream(cuda, 256, seed=5, graph=graph)
        outs = [gen.generate(96), gen.generate(96)]
        assert (gen._graphs is not None) == graph
        emitted = _bookkeeping(gen, replay, outs)
        recs.append((emitted, _rows(replay, gen, list(range(256)))))
    assert recs[0][0] == recs[1][0]
    _same(recs[0][1], recs[1][1])


def _check_values(net, obs, value, mask):
    """Recorded values against the fp64 forward on the recorded observations, where ``mask``."""
    rows = mask.reshape(-1).nonzero().reshape(-1)
    o = obs.reshape(-1, 3, 3, 3).float().cpu()[rows.cpu()]
    _, v64 = util.forward64(net, o)
    err = (value.reshape(-1).cpu()[rows.cpu()].double() - v64.reshape(-1)).abs().max().item()
    assert err <= 1e-5, err
    return rows.numel()


@pytest.mark.gpu
def test_lockstep_generator_with_the_wrapper(cuda):
    net = _net(cuda)
    gen = DeviceGenerator(TicTacToeBatch(E, cuda), hnn.BoardInference(net), gamma=GAMMA)
    for _ in range(2):                                       # the second call replays the captured ply
        ep = gen.generate(generator=torch.Generator(device=cuda).manual_seed(1))
        assert ep['length'].shape == (E,) and bool(((ep['length'] >= 5) & (ep['length'] <= 9)).all())
        Tm = TicTacToeBatch.MAX_PLIES
        live = torch.arange(Tm, device=cuda).view(1, Tm) < ep['length'].view(E, 1)
        n = _check_values(net, ep['observation'], ep['value'], live)
        assert n == int(ep['length'].sum())


@pytest.mark.gpu
def test_per_player_generator_with_the_wrapper(cuda):
    net = _net(cuda)
    w = hnn.BoardInference(net)
    gen = DeviceGenerator(TicTacToeBatch(E, cuda), w, gamma=GAMMA, observation=True, per_player=True)
    ep = gen.generate(generator=torch.Generator(device=cuda).manual_seed(2))
    assert ep['value'].shape[:3] == (E, TicTacToeBatch.MAX_PLIES, 2)
    n = _check_values(net, ep['observation'], ep['value'], ep['omask'])
    assert n == 2 * int(ep['length'].sum())                   # every player infers at every ply
    assert w._live == 0                                       # the session was entered, and left


@pytest.mark.gpu
def test_evaluator_is_greedy_up_to_the_tolerance(cuda):
    """At every traced ply of the model the fp64 logit of the chosen move is within 2e-5 of the best legal one
    (1e-5 on each side)."""
    G = 96
    net = _net(cuda)
    ev = DeviceEvaluator(TicTacToeBatch(E, cuda), hnn.BoardInference(net), seed=11)
    res = ev.evaluate(G, trace=True)
    assert sum(res['results'].values()) == G
    tr = {k: v.cpu() for k, v in res['trace'].items()}
    length = res['length'].cpu().tolist()
    obs, legal, chosen = [], [], []
    one = torch.ones(1, dtype=torch.bool)
    for g in range(G):
        b = TicTacToeBatch(1, 'cpu')
        for t in range(length[g]):
            a = int(tr['action'][g, t])
            if bool(tr['model_ply'][g, t]):
                assert int(tr['picked'][g, t]) == a
                obs.append(b.observation(b.turn())[0])
                legal.append(b.legal()[0])
                chosen.append(a)
            b.step(torch.tensor([a]), one)
        assert bool(b.terminal())
    assert len(chosen) >= 2 * G
    p64, _ = util.forward64(net, torch.stack(obs))
    best = torch.where(torch.stack(legal), p64, float('-inf')).max(-1).values
    gap = (best - p64[torch.arange(len(chosen)), torch.tensor(chosen)]).max().item()
    assert 0 <= gap <= 2e-5, gap


def _league(cuda, nets, slots, **kw):
    return LeagueEvaluator(TicTacToeBatch(slots, cuda), nets, opening_plies=2, seed=5, **kw)


@pytest.mark.gpu
def test_league_group_equals_the_wrappers_ungrouped(cuda):
    nets = [_net(cuda, seed=s) for s in range(3)]
    grouped = _league(cuda, hnn.board_inference_group(nets), 12)
    a = grouped.evaluate(10)
    assert grouped._st['group'] is not None
    loose = _league(cuda, [hnn.BoardInference(n) for n in nets], 12)
    b = loose.evaluate(10)
    assert loose._st['group'] is None
    for k in ('outcome', 'length', 'score', 'games'):
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    assert int(a['games'].sum()) == 2 * 3 * 10


def _ply_launches(cuda, K):
    """(kernel launches, group.forward calls) of one eager grouped league ply on E = 24 slots."""
    from torch.profiler import ProfilerActivity, profile
    nets = [_net(cuda, seed=s) for s in range(K)]
    group = hnn.board_inference_group(nets)
    ev = _league(cuda, group, 24, graph=False)
    calls = []
    real = group.forward
    group.forward = lambda obs, span: (calls.append(len(span)), real(obs, span))[1]
    with torch.no_grad(), contextlib.ExitStack() as stack:
        for m in group:
            stack.enter_context(m.inference_session())
        st = ev._state()
        assert st['group'] is group
        run = ev._prepare(st, 4)
        ev._begin(st, run)
        ev._ply(st, run, 0)
        ev._ply(st, run, 1)                                  # warm: every lazy initialisation is done
        torch.cuda.synchronize(cuda)
        del calls[:]
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            ev._ply(st, run, 0)
            torch.cuda.synchronize(cuda)
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(kernels), calls


@pytest.mark.gpu
def test_grouped_ply_launch_count_does_not_depend_on_K(cuda):
    n3, calls3 = _ply_launches(cuda, 3)
    n4, calls4 = _ply_launches(cuda, 4)
    print('grouped league ply: %d launches at K = 3, %d at K = 4' % (n3, n4))
    assert calls3 == [4] and calls4 == [5]                   # one grouped forward per ply, over K + 1 offsets
    assert n3 == n4 and n3 > 0


@pytest.mark.gpu
def test_train_main_with_fused_inference(tmp_path, cuda, monkeypatch):
    from handyrl_amd.main import train_main
    args = _small()
    args['train_args'].update(inference='fused', epochs=1, eval_rate=0.5, eval_opponent='previous')
    made = []
    real = hnn.BoardInference.__init__
    monkeypatch.setattr(hnn.BoardInference, '__init__', lambda self, net: (made.append(1), real(self, net))[1])
    logs = []
    model = train_main(args, device=cuda, model_dir=str(tmp_path / 'fused'), log=logs.append)
    assert os.path.exists(tmp_path / 'fused' / '1.pth') and len(made) == 2       # the net and its opponent
    assert len(logs) == 1 and 'win rate' in logs[0] and 'vs previous' in logs[0]
    saved = torch.load(tmp_path / 'fused' / '1.pth', weights_only=True)
    assert set(saved) == set(model.state_dict())
    assert all(torch.isfinite(v.float()).all() for v in saved.values())
    # the key absent (or None): nothing of the feature runs, and the run is the one it always was
    del made[:]
    runs = []
    for name, value in (('absent', 'pop'), ('none', None)):
        a = _small()
        a['train_args'].update(epochs=1)
        if value is None:
            a['train_args']['inference'] = None
        else:
            a['train_args'].pop('inference', None)
        train_main(a, device=cuda, model_dir=str(tmp_path / name), log=lambda *_: None)
        runs.append(torch.load(tmp_path / name / '1.pth', weights_only=True))
    assert not made
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
