"""evaluation.DeviceEvaluator: every game it reports is refereed on its own; the reference is not involved.

A game's moves depend on (seed, game number, ply) and the model only, so game g can be checked without knowing in
which slot or when it was played: the traced actions are replayed through a fresh one-game CPU batch (rules, legal
sets, outcome, length), the random seat's moves are redone with ``eval_pick`` (exact), the model's ``picked`` is the
argmax of its own traced policy (lowest label on ties) and the traced policy is compared with a CPU eval forward on
the replayed observations (1e-5 absolute, the project's self-play bound; exact for the test-local integer nets).
"""

import pytest
import torch
from torch import nn

from handyrl_amd import evaluation
from handyrl_amd.evaluation import DeviceEvaluator, eval_pick, wp_func
from handyrl_amd.rollout import TicTacToeBatch

DEVICES = ['cpu', pytest.param('cuda', marks=pytest.mark.gpu)]
SEED = 0x5eed0123456789


@pytest.fixture(params=DEVICES)
def dev(request):
    if request.param == 'cuda':
        return request.getfixturevalue('cuda')
    return torch.device('cpu')


def _batch_cls(name):
    if name == 'tictactoe':
        return TicTacToeBatch
    from handyrl_amd.envs.geister import GeisterBatch
    return GeisterBatch


def _flat(x):
    xs = [x[k] for k in sorted(x)] if isinstance(x, dict) else [x]
    return torch.cat([t.flatten(1).float() for t in xs], 1)


class IntNet(nn.Module):
    """Logits that are small integers whatever the summation order: binary observations times integer weights."""

    def __init__(self, cls, recurrent=False, H=5):
        super().__init__()
        import numpy as np
        n = sum(int(np.prod(s)) for s in (cls.OBS_SHAPE.values() if isinstance(cls.OBS_SHAPE, dict)
                                           else [cls.OBS_SHAPE]))
        g = torch.Generator().manual_seed(17)
        self.register_buffer('w', torch.randint(-3, 4, (n, cls.A), generator=g).float())
        self.H = H if recurrent else 0
        if recurrent:
            self.register_buffer('wh', torch.randint(0, 3, (n, H), generator=g).float())
            self.register_buffer('wo', torch.randint(-2, 3, (H, cls.A), generator=g).float())
            self.init_hidden = lambda batch_size: torch.zeros(*batch_size, H)

    def forward(self, x, hidden=None):
        f = _flat(x)
        out = {'policy': f @ self.w, 'value': torch.zeros(f.shape[0], 1, device=f.device)}
        if self.H:
            h = torch.remainder(hidden + f @ self.wh + 1, 7)     # never zero again once it has moved
            out['policy'] = out['policy'] + h @ self.wo
            out['hidden'] = h
        return out


def _real_nets(name, dev):
    if name == 'tictactoe':
        from handyrl_amd.envs.tictactoe import SimpleConv2dModel as Net
    else:
        from handyrl_amd.envs.geister import GeisterNet as Net
    torch.manual_seed(11)
    cpu = Net()
    cpu.eval()
    if dev.type == 'cpu':
        return cpu, cpu
    net = Net().to(dev)
    if name == 'geister':
        from handyrl_amd.nn import accelerate
        net = accelerate(net)
    net.load_state_dict(cpu.state_dict())
    return net, cpu


def _cpu(res):
    out = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in res.items() if k != 'trace'}
    out['trace'] = {k: v.cpu() for k, v in res['trace'].items()}
    return out


def referee(name, res, cpu_net, G, observation=False, tol=1e-5):
    cls = _batch_cls(name)
    Tm, P = cls.MAX_PLIES, cls.P
    res = _cpu(res)
    tr = res['trace']
    assert res['games'] == G and res['outcome'].shape == (G, P) and res['length'].shape == (G,)
    assert res['seat'].tolist() == [g % P for g in range(G)]
    assert res['env_steps'] == int(res['length'].sum())
    one = torch.ones(1, dtype=torch.bool)
    views = {}                                   # (g, t) -> the model's observation, for the net check
    with torch.no_grad():
        for g in range(G):
            L, seat = int(res['length'][g]), g % P
            assert 1 <= L <= Tm, (g, L)                                # played exactly once: a result is there
            b = cls(1, 'cpu')
            for t in range(L):
                assert not bool(b.terminal()) and int(b.turn()) == t % P, (g, t)
                legal = b.legal()[0]
                a, picked = int(tr['action'][g, t]), int(tr['picked'][g, t])
                model = t % P == seat
                assert bool(tr['model_ply'][g, t]) == model, (g, t)
                if model or observation:
                    views[(g, t)] = b.observation(torch.tensor([seat]))
                if model:
                    p = tr['policy'][g, t]
                    assert torch.equal(p == p.clamp(min=-1e31), legal), (g, t)      # masked exactly off the legal set
                    assert picked == int(torch.argmax(p)), (g, t)
                    assert picked == min(i for i in range(cls.A) if p[i] == p.max()), (g, t)
                else:
                    assert picked == eval_pick(SEED, g, t, legal.tolist()), (g, t)
                    assert not bool(tr['policy'][g, t].any()), (g, t)
                assert a == picked and bool(legal[a]), (g, t)
                b.step(torch.tensor([a]), one)
            assert bool(b.terminal()) or L == Tm, g
            assert torch.equal(res['outcome'][g], b.outcome()[0].float()), g
            assert bool((tr['action'][g, L:] == -1).all()) and bool((tr['picked'][g, L:] == -1).all()), g
            assert not bool(tr['model_ply'][g, L:].any()) and not bool(tr['policy'][g, L:].any()), g
        # the traced policy against a CPU forward, games advancing together; one state per game from zeros, moved
        # at the model's plies and (observation) at the opponent's too
        recurrent = hasattr(cpu_net, 'init_hidden')
        hidden = cpu_net.init_hidden([G]) if recurrent else None
        lengths = res['length'].tolist()
        for t in range(max(lengths) if G else 0):
            idx = [g for g in range(G) if (g, t) in views]
            if not idx:
                continue
            ix = torch.tensor(idx)
            obs = [views[(g, t)] for g in idx]
            obs = ({k: torch.cat([o[k] for o in obs]) for k in obs[0]} if isinstance(obs[0], dict) else torch.cat(obs))
            h = None
            if recurrent:
                h = _map(hidden, lambda x: x[ix])
            out = cpu_net(obs, h)
            if recurrent:
                _bimap(hidden, out['hidden'], lambda x, nx: x.index_copy_(0, ix, nx))
            for j, g in enumerate(idx):
                if t % P != g % P:
                    continue
                p = tr['policy'][g, t]
                legal = p > -1e31
                d = float(torch.where(legal, (p - out['policy'][j].float()).abs(), torch.zeros(())).max())
                assert d <= tol, (g, t, d)
    results = {}
    for g in range(G):
        o = float(res['outcome'][g, g % P]) + 0.0
        results[o] = results.get(o, 0) + 1
    assert results == res['results'] and sum(results.values()) == G
    assert res['win_rate'] == wp_func(results)
    return res


def _map(x, f):
    return type(x)(_map(y, f) for y in x) if isinstance(x, (list, tuple)) else f(x)


def _bimap(x, y, f):
    if isinstance(x, (list, tuple)):
        for a, b in zip(x, y):
            _bimap(a, b, f)
    else:
        f(x, y)


def _evaluate(name, dev, E, G, net, **kw):
    ev = DeviceEvaluator(_batch_cls(name)(E, dev), net, seed=SEED, **kw)
    return ev.evaluate(G, trace=True)


def test_tictactoe_games_are_refereed(dev):
    """G = 48 on E = 7 (not a multiple of the kernel's 4 slots per workgroup): slots restart six times over."""
    net, cpu = _real_nets('tictactoe', dev)
    res = referee('tictactoe', _evaluate('tictactoe', dev, 7, 48, net), cpu, 48)
    assert res['plies'] >= int(res['length'].max()) and sum(res['results'].values()) == 48


def test_geister_games_are_refereed(dev):
    """G = 6 on E = 4, the recurrent GeisterNet: two slots restart, two retire."""
    net, cpu = _real_nets('geister', dev)
    referee('geister', _evaluate('geister', dev, 4, 6, net), cpu, 6)


@pytest.mark.parametrize('E,G', [(9, 4), (5, 0), (3, 1), (1, 5)])
def test_edges_of_the_game_count(dev, E, G):
    """More slots than games (the spare slots never play), no game at all, one game, one slot."""
    net, cpu = _real_nets('tictactoe', dev)
    res = referee('tictactoe', _evaluate('tictactoe', dev, E, G, net), cpu, G)
    if G == 0:
        assert res['plies'] == 0 and res['results'] == {} and res['win_rate'] == 0.0 and res['env_steps'] == 0


def _same(a, b):
    for k in ('outcome', 'length', 'seat'):
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    for k in a['trace']:
        ta, tb = a['trace'][k].cpu(), b['trace'][k].cpu()
        if ta.dtype == torch.float32:
            ta, tb = ta.view(torch.int32), tb.view(torch.int32)
        assert torch.equal(ta, tb), k
    assert a['results'] == b['results'] and a['win_rate'] == b['win_rate']


@pytest.mark.parametrize('recurrent,observation', [(False, False), (True, False), (True, True)])
def test_games_do_not_depend_on_the_slots(dev, recurrent, observation):
    """Integer nets (exact in fp32 in any summation order): the same 48 games on 7 and on 48 slots, refereed
    exactly.  The recurrent net's policy depends on its state, so a restarted slot's state is zero and, without
    ``observation``, does not move on the opponent's ply -- or the referee's own state would disagree."""
    net = IntNet(TicTacToeBatch, recurrent).to(dev)
    cpu = IntNet(TicTacToeBatch, recurrent)
    a = _evaluate('tictactoe', dev, 7, 48, net, observation=observation)
    b = _evaluate('tictactoe', dev, 48, 48, net, observation=observation)
    _same(a, b)
    referee('tictactoe', a, cpu, 48, observation=observation, tol=0.0)
    if recurrent:       # the two modes do differ: the state is really used
        c = _evaluate('tictactoe', dev, 7, 48, net, observation=not observation)
        assert not torch.equal(a['trace']['policy'].cpu(), c['trace']['policy'].cpu())


def test_geister_integer_net_on_few_and_many_slots(dev):
    from handyrl_amd.envs.geister import GeisterBatch
    net = IntNet(GeisterBatch, True).to(dev)
    a = _evaluate('geister', dev, 2, 3, net)
    _same(a, _evaluate('geister', dev, 3, 3, net))
    referee('geister', a, IntNet(GeisterBatch, True), 3, tol=0.0)


def test_temperature_and_forced(dev):
    """Temperature > 0: the model's picked is the Gumbel-max of the traced policy with the game's own uniforms.
    Forced moves are played whichever seat moves, and ``picked`` stays the evaluator's own decision."""
    from handyrl_amd.rollout import stream_uniforms
    net = IntNet(TicTacToeBatch).to(dev)
    ev = DeviceEvaluator(TicTacToeBatch(5, dev), net, temperature=0.5, seed=SEED)
    res = _cpu(ev.evaluate(12, trace=True))
    tr = res['trace']
    n = 0
    for g in range(12):
        for t in range(int(res['length'][g])):
            if t % 2 == g % 2:
                u = torch.from_numpy(stream_uniforms(SEED, g, t, 9)).to(dev)       # the logs on the device played on
                v = tr['policy'][g, t].to(dev) * 2.0 - torch.log(-torch.log(u))
                assert int(tr['picked'][g, t]) == int(torch.argmax(v)), (g, t)
                n += 1
    assert n > 30
    forced = tr['action'].clone()
    greedy = DeviceEvaluator(TicTacToeBatch(5, dev), net, seed=SEED)
    again = _cpu(greedy.evaluate(12, forced=forced, trace=True))
    assert torch.equal(again['trace']['action'], tr['action']) and torch.equal(again['outcome'], res['outcome'])
    assert torch.equal(again['length'], res['length'])
    free = _cpu(greedy.evaluate(12, trace=True))
    rand = ~tr['model_ply'] & (tr['action'] >= 0)
    assert torch.equal(again['trace']['picked'][rand], tr['picked'][rand])          # the same game, ply, legal set
    assert not torch.equal(again['trace']['picked'], again['trace']['action'])      # greedy differs from sampled
    assert torch.equal(free['trace']['picked'], free['trace']['action'])


def test_out_of_scope_envs_name_the_reason():
    from handyrl_amd.rollout import ParallelTicTacToeBatch
    with pytest.raises(ValueError, match='simultaneous'):
        DeviceEvaluator(ParallelTicTacToeBatch(4, 'cpu'), IntNet(TicTacToeBatch))
    with pytest.raises(ValueError, match='batched'):
        evaluation.batched_env('tests.plugin_env')


def test_training_mode_is_put_back_and_no_generator_is_drawn(dev):
    net, _ = _real_nets('tictactoe', dev)
    net.train()
    state = torch.get_rng_state()
    before = [b.clone() for b in net.buffers()]
    DeviceEvaluator(TicTacToeBatch(4, dev), net, seed=SEED).evaluate(6)
    assert net.training and torch.equal(torch.get_rng_state(), state)
    for b, old in zip(net.buffers(), before):       # BatchNorm running statistics untouched
        assert torch.equal(b, old)


# ---- GPU only: graph against eager, the kernels against the torch formulation, whole games

@pytest.mark.gpu
@pytest.mark.parametrize('name,E,G', [('tictactoe', 7, 48), ('geister', 4, 6)])
def test_integer_net_graph_eager_fused_agree(cuda, monkeypatch, name, E, G):
    """Identical per game: graph against eager, FUSED_EVAL on against off, and the CPU."""
    cls = _batch_cls(name)
    net = IntNet(cls, True).to(cuda)
    base = _evaluate(name, cuda, E, G, net, graph=True)
    _same(base, _evaluate(name, cuda, E, G, net, graph=False))
    monkeypatch.setattr(evaluation, 'FUSED_EVAL', False)
    _same(base, _evaluate(name, cuda, E, G, net, graph=False))
    _same(base, _evaluate(name, cuda, E, G, net, graph=True))
    _same(base, _evaluate(name, torch.device('cpu'), E, G, IntNet(cls, True)))


@pytest.mark.gpu
@pytest.mark.parametrize('name,E,G', [('tictactoe', 7, 48), ('geister', 4, 6)])
def test_real_net_graph_equals_eager(cuda, name, E, G):
    net, _ = _real_nets(name, cuda)
    _same(_evaluate(name, cuda, E, G, net, graph=True), _evaluate(name, cuda, E, G, net, graph=False))


@pytest.mark.gpu
def test_a_second_call_reuses_the_graphs_and_starts_afresh(cuda):
    net, _ = _real_nets('tictactoe', cuda)
    ev = DeviceEvaluator(TicTacToeBatch(7, cuda), net, seed=SEED)
    a = ev.evaluate(48, trace=True)
    graphs = ev._run['graphs']
    b = ev.evaluate(48, trace=True)
    assert graphs is not None and ev._run['graphs'] is graphs
    _same(a, b)


@pytest.mark.gpu
def test_geister_64_games_results_add_up(cuda):
    """Seeded-init GeisterNet, 64 games on 24 slots, no trace."""
    net, _ = _real_nets('geister', cuda)
    res = DeviceEvaluator(_batch_cls('geister')(24, cuda), net, seed=SEED).evaluate(64)
    assert 'trace' not in res and sum(res['results'].values()) == 64
    mine = res['outcome'][torch.arange(64), res['seat']].tolist()
    table = {}
    for o in mine:
        table[o + 0.0] = table.get(o + 0.0, 0) + 1
    assert table == res['results'] and res['win_rate'] == wp_func(table)
    assert bool((res['length'] >= 2).all()) and bool((res['length'] <= 202).all())
    assert torch.equal(res['outcome'][:, 0], -res['outcome'][:, 1])
