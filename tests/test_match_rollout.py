"""evaluation.DeviceEvaluator with an opponent net: every game of a match is refereed on its own.

A game's moves depend on (seed, game number, ply) and the two nets only.  The traced actions are replayed through a
fresh one-game CPU batch (rules, legal sets, outcome, length); an opening ply's ``picked`` is redone with
``eval_pick``; every other ply's ``picked`` is the argmax of the policy of the net whose seat moves, recomputed on
the CPU from the refereed position and that net's own recurrent state (exact for the integer nets, 1e-5 absolute --
the project's self-play bound -- for the real ones).  The two integer nets differ (the opponent's policy weights are
negated), so a ply decided by the wrong net, from the wrong view or with the wrong state fails.
"""

import copy

import pytest
import torch

from handyrl_amd import evaluation
from handyrl_amd.evaluation import DeviceEvaluator, act_torch, eval_pick, finish_torch, wp_func
from handyrl_amd.rollout import TicTacToeBatch
from tests.test_eval_rollout import IntNet, _batch_cls, _bimap, _map, _real_nets

DEVICES = ['cpu', pytest.param('cuda', marks=pytest.mark.gpu)]
SEED = 0x5eed0123456789


@pytest.fixture(params=DEVICES)
def dev(request):
    if request.param == 'cuda':
        return request.getfixturevalue('cuda')
    return torch.device('cpu')


def _int_nets(cls, dev, recurrent=False):
    """(home, opponent) on ``dev`` and their CPU twins; the opponent's policy weights are the home's negated."""
    nets = []
    for d in (dev, torch.device('cpu')):
        home, opp = IntNet(cls, recurrent), IntNet(cls, recurrent)
        opp.w.neg_()
        nets += [home.to(d), opp.to(d)]
    return nets


def _cpu(res):
    out = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in res.items() if k != 'trace'}
    out['trace'] = {k: v.cpu() for k, v in res['trace'].items()}
    return out


def _table(values):
    t = {}
    for o in values:
        t[o + 0.0] = t.get(o + 0.0, 0) + 1
    return {k: t[k] for k in sorted(t, reverse=True)}


def referee(name, res, cpu_home, cpu_opp, G, opening, observation=False, tol=0.0):
    cls = _batch_cls(name)
    Tm, P, A = cls.MAX_PLIES, cls.P, cls.A
    assert P == 2
    res = _cpu(res)
    tr = res['trace']
    assert res['games'] == G and res['outcome'].shape == (G, P) and res['length'].shape == (G,)
    assert res['seat'].tolist() == [g % P for g in range(G)]
    assert res['env_steps'] == int(res['length'].sum())
    one = torch.ones(1, dtype=torch.bool)
    views, legals = {}, {}                       # (g, t, home net?) -> that net's observation
    with torch.no_grad():
        for g in range(G):
            L, seat = int(res['length'][g]), g % P
            assert 1 <= L <= Tm, (g, L)
            b = cls(1, 'cpu')
            for t in range(L):
                assert not bool(b.terminal()) and int(b.turn()) == t % P, (g, t)
                legal = b.legal()[0]
                legals[(g, t)] = legal
                a, picked = int(tr['action'][g, t]), int(tr['picked'][g, t])
                assert bool(tr['model_ply'][g, t]) == (t % P == seat), (g, t)     # still the HOME seat's plies
                views[(g, t, True)] = b.observation(torch.tensor([seat]))
                views[(g, t, False)] = b.observation(torch.tensor([(seat + 1) % P]))
                p = tr['policy'][g, t]
                assert torch.equal(p == p.clamp(min=-1e31), legal), (g, t)        # masked exactly off the legal set
                if t < opening:
                    assert picked == eval_pick(SEED, g, t, legal.tolist()), (g, t)
                else:
                    assert picked == min(i for i in range(A) if p[i] == p.max()), (g, t)
                assert a == picked and bool(legal[a]), (g, t)
                b.step(torch.tensor([a]), one)
            assert bool(b.terminal()) or L == Tm, g
            assert torch.equal(res['outcome'][g], b.outcome()[0].float()), g
            assert bool((tr['action'][g, L:] == -1).all()) and bool((tr['picked'][g, L:] == -1).all()), g
            assert not bool(tr['model_ply'][g, L:].any()) and not bool(tr['policy'][g, L:].any()), g
        # each net on its own: one state per game from zeros, moved at that net's plies and (observation) at the
        # other's too; its policy at its own plies is the traced one and, past the opening, decides the move
        lengths = res['length'].tolist()
        checked = 0
        for net, is_home in ((cpu_home, True), (cpu_opp, False)):
            recurrent = hasattr(net, 'init_hidden')
            hidden = net.init_hidden([G]) if recurrent else None
            for t in range(max(lengths) if G else 0):
                idx = [g for g in range(G) if t < lengths[g] and (observation or (t % P == g % P) == is_home)]
                if not idx:
                    continue
                ix = torch.tensor(idx)
                obs = [views[(g, t, is_home)] for g in idx]
                obs = ({k: torch.cat([o[k] for o in obs]) for k in obs[0]} if isinstance(obs[0], dict)
                       else torch.cat(obs))
                out = net(obs, _map(hidden, lambda x: x[ix]) if recurrent else None)
                if recurrent:
                    _bimap(hidden, out['hidden'], lambda x, nx: x.index_copy_(0, ix, nx))
                for j, g in enumerate(idx):
                    if (t % P == g % P) != is_home:
                        continue
                    p, legal = tr['policy'][g, t], legals[(g, t)]
                    mine = out['policy'][j].float()
                    d = float(torch.where(legal, (p - mine).abs(), torch.zeros(())).max())
                    assert d <= tol, (g, t, is_home, d)
                    if tol == 0.0 and t >= opening:
                        masked = mine - torch.where(legal, 0.0, 1e32)
                        assert int(tr['picked'][g, t]) == int(torch.argmax(masked)), (g, t, is_home)
                    checked += 1
        assert checked == sum(lengths)
    mine = [float(res['outcome'][g, g % P]) for g in range(G)]
    theirs = [float(res['outcome'][g, (g + 1) % P]) for g in range(G)]
    assert res['results'] == _table(mine) and sum(res['results'].values()) == G
    assert res['opponent_results'] == _table(theirs) and list(res['opponent_results']) == sorted(
        res['opponent_results'], reverse=True)
    assert res['win_rate'] == wp_func(res['results']) and res['opponent_win_rate'] == wp_func(res['opponent_results'])
    return res


def _match(name, dev, E, G, home, opp, opening=2, **kw):
    ev = DeviceEvaluator(_batch_cls(name)(E, dev), home, seed=SEED, opponent=opp, opening_plies=opening, **kw)
    return ev.evaluate(G, trace=True)


def _same(a, b):
    for k in ('outcome', 'length', 'seat'):
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    for k in a['trace']:
        ta, tb = a['trace'][k].cpu(), b['trace'][k].cpu()
        if ta.dtype == torch.float32:
            ta, tb = ta.view(torch.int32), tb.view(torch.int32)
        assert torch.equal(ta, tb), k
    for k in ('results', 'win_rate', 'opponent_results', 'opponent_win_rate'):
        assert a.get(k) == b.get(k), k


@pytest.mark.parametrize('recurrent,observation', [(False, False), (True, False), (True, True)])
def test_tictactoe_match_is_refereed_on_few_and_many_slots(dev, recurrent, observation):
    """64 games on 7 slots (not a multiple of the kernel's 4 slots per workgroup: slots restart nine times over) and
    on 64, identical per game and refereed exactly.  The recurrent nets' policies depend on their state: a restarted
    slot has both states zero, and without ``observation`` the opponent's state moves at its own plies only, with
    it on every ply -- or the referee's states would disagree.  Zero-sum: the two win rates add up to 1 exactly (64
    games: every division is by a power of two)."""
    home, opp, cpu_home, cpu_opp = _int_nets(TicTacToeBatch, dev, recurrent)
    a = _match('tictactoe', dev, 7, 64, home, opp, observation=observation)
    _same(a, _match('tictactoe', dev, 64, 64, home, opp, observation=observation))
    res = referee('tictactoe', a, cpu_home, cpu_opp, 64, 2, observation=observation)
    assert res['win_rate'] + res['opponent_win_rate'] == 1.0
    assert res['opponent_results'] == _table([-k for k, v in res['results'].items() for _ in range(v)])
    if recurrent:       # the two modes do differ: the states are really used
        c = _match('tictactoe', dev, 7, 64, home, opp, observation=not observation)
        assert not torch.equal(a['trace']['policy'].cpu(), c['trace']['policy'].cpu())
    # the opponent decides: against the home net's own weights the games differ
    twin = copy.deepcopy(home)
    b = _match('tictactoe', dev, 7, 64, home, twin, observation=observation)
    assert not torch.equal(a['trace']['action'].cpu(), b['trace']['action'].cpu())


@pytest.mark.parametrize('observation', [False, True])
def test_geister_match_with_recurrent_integer_nets(dev, observation):
    """4 games on 3 slots (one restarts) and on 4, three opening plies (an odd count: the first net ply is the
    second mover's)."""
    from handyrl_amd.envs.geister import GeisterBatch
    home, opp, cpu_home, cpu_opp = _int_nets(GeisterBatch, dev, True)
    a = _match('geister', dev, 3, 4, home, opp, opening=3, observation=observation)
    _same(a, _match('geister', dev, 4, 4, home, opp, opening=3, observation=observation))
    res = referee('geister', a, cpu_home, cpu_opp, 4, 3, observation=observation)
    assert res['win_rate'] + res['opponent_win_rate'] == 1.0


def test_real_nets_match_is_refereed(dev):
    """Two seeded-init SimpleConv2dModels: the traced policies against CPU forwards of the right net, 1e-5."""
    home, cpu_home = _real_nets('tictactoe', dev)
    torch.manual_seed(12)
    cpu_opp = type(cpu_home)()
    cpu_opp.eval()
    opp = copy.deepcopy(cpu_opp).to(dev)
    referee('tictactoe', _match('tictactoe', dev, 7, 24, home, opp), cpu_home, cpu_opp, 24, 2, tol=1e-5)


def test_a_net_against_a_copy_of_itself(dev):
    """Without opening plies two greedy agents replay ONE game whoever sits where, so the home table and the
    opponent's are each other's mirror; with opening plies every game is decided by the same weights on both seats
    (the referee recomputes both from the one CPU net) and the tables mirror each other game by game."""
    home, _, cpu_home, _ = _int_nets(TicTacToeBatch, dev)
    twin = copy.deepcopy(home)
    res = _cpu(_match('tictactoe', dev, 5, 16, home, twin, opening=0))
    assert bool((res['trace']['action'] == res['trace']['action'][0]).all())
    assert bool((res['outcome'] == res['outcome'][0]).all())
    first = float(res['outcome'][0, 0]) + 0.0
    assert res['results'] == _table([first] * 8 + [-first] * 8) == res['opponent_results']
    res = referee('tictactoe', _match('tictactoe', dev, 5, 16, home, twin), cpu_home, cpu_home, 16, 2)
    for g in range(16):
        assert float(res['outcome'][g, g % 2]) == -float(res['outcome'][g, (g + 1) % 2])
    assert len(set(map(tuple, res['trace']['action'].tolist()))) > 2      # the openings do spread the games


def test_opening_plies_and_temperatures(dev):
    """Opening plies without an opponent (the random seats stay eval_pick, the model's first plies too), and one
    temperature per agent: each net's ``picked`` is the Gumbel-max of its own policy at its own temperature over the
    game's one stream."""
    from handyrl_amd.rollout import stream_uniforms
    home, opp, cpu_home, cpu_opp = _int_nets(TicTacToeBatch, dev)
    res = _cpu(DeviceEvaluator(TicTacToeBatch(5, dev), home, seed=SEED, opening_plies=3).evaluate(12, trace=True))
    assert 'opponent_results' not in res
    tr = res['trace']
    b0 = TicTacToeBatch(1, 'cpu')
    for g in range(12):
        assert int(tr['picked'][g, 0]) == eval_pick(SEED, g, 0, b0.legal()[0].tolist())
        for t in range(int(res['length'][g])):
            model = t % 2 == g % 2
            assert bool((tr['policy'][g, t] < -1e31).any()) == (model and t > 0)   # traced at opening plies too
            if model and t >= 3:
                assert int(tr['picked'][g, t]) == int(torch.argmax(tr['policy'][g, t]))
    ev = DeviceEvaluator(TicTacToeBatch(5, dev), home, seed=SEED, temperature=0.5, opponent=opp,
                         opponent_temperature=0.25, opening_plies=1)
    res = _cpu(ev.evaluate(12, trace=True))
    tr, n = res['trace'], 0
    for g in range(12):
        for t in range(1, int(res['length'][g])):
            r = 2.0 if t % 2 == g % 2 else 4.0
            u = torch.from_numpy(stream_uniforms(SEED, g, t, 9)).to(dev)        # the logs on the device played on
            v = tr['policy'][g, t].to(dev) * r - torch.log(-torch.log(u))
            assert int(tr['picked'][g, t]) == int(torch.argmax(v)), (g, t)
            n += 1
    assert n > 40
    same = DeviceEvaluator(TicTacToeBatch(5, dev), home, seed=SEED, temperature=0.5, opponent=opp, opening_plies=1)
    assert same.opponent_temperature == 0.5                                   # None: the home temperature


def _by_hand(cls, net, E, G, observation):
    """The evaluator's ply against random agents spelled out with ``act_torch`` and ``finish_torch`` on the CPU."""
    env = cls(E, 'cpu')
    Tm, P, A = cls.MAX_PLIES, cls.P, cls.A
    rows = torch.arange(E)
    st = {'Tm': Tm, 'P': P, 'game': torch.clamp(rows, max=G), 'ply': torch.zeros(E, dtype=torch.long),
          'seat': torch.where(rows < G, rows % P, 0), 'active': rows < G,
          'pending': torch.zeros(E, dtype=torch.bool), 'state': torch.tensor([0, min(E, G)])}
    hidden = net.init_hidden([E]) if hasattr(net, 'init_hidden') else None
    outcome, length = torch.zeros(G + 1, P), torch.zeros(G + 1, dtype=torch.long)
    trace = {'action': torch.full((G + 1, Tm), -1), 'picked': torch.full((G + 1, Tm), -1),
             'policy': torch.zeros(G + 1, Tm, A), 'model_ply': torch.zeros(G + 1, Tm, dtype=torch.bool)}
    env.reset()
    s = 0
    with torch.no_grad():
        while int(st['state'][0]) < G:
            mover = s % P
            if mover == 0:
                env.reset_where(st['pending'])
                if hidden is not None:
                    hidden.masked_fill_(st['pending'].view(-1, 1), 0)
                st['active'].logical_or_(st['pending'])
                st['pending'].zero_()
            out = net(env.observation(st['seat']), hidden)
            a = act_torch(st, out['policy'], env.legal(), mover, SEED, 0.0, G, None, trace)
            if hidden is not None:
                adv = st['active'].clone() if observation else st['active'] & (st['seat'] == mover)
                hidden.copy_(torch.where(adv.view(-1, 1), out['hidden'], hidden))
            env.step(a, st['active'])
            finish_torch(st, env.terminal(), env.outcome(), G, outcome, length)
            s += 1
    return {'outcome': outcome[:G], 'length': length[:G], 'trace': {k: v[:G] for k, v in trace.items()}}


@pytest.mark.parametrize('recurrent,observation', [(False, False), (True, False), (True, True)])
def test_default_arguments_play_the_random_agents_as_before(dev, monkeypatch, recurrent, observation):
    """No opponent, no opening plies: the games are those of act_torch / finish_torch driven by hand, the result has
    no new key and the one decision (match_act_*) only ever runs in its no-opponent form: no second net's logits, no
    opening plies."""
    calls = []

    def no_opponent(decide):
        def spy(st, logits_home, logits_opp, legal, mover, seed, temperature_home, temperature_opp, opening, *a, **k):
            assert logits_opp is None and opening == 0, 'the decision saw an opponent or opening plies'
            calls.append(decide.__name__)
            return decide(st, logits_home, logits_opp, legal, mover, seed, temperature_home, temperature_opp, opening,
                          *a, **k)
        return spy
    monkeypatch.setattr(evaluation, 'match_act_torch', no_opponent(evaluation.match_act_torch))
    monkeypatch.setattr(evaluation, 'match_act_hip', no_opponent(evaluation.match_act_hip))
    net = IntNet(TicTacToeBatch, recurrent).to(dev)
    res = DeviceEvaluator(TicTacToeBatch(7, dev), net, observation=observation, seed=SEED).evaluate(48, trace=True)
    assert calls
    assert sorted(res) == ['env_steps', 'games', 'length', 'outcome', 'plies', 'results', 'seat', 'trace', 'win_rate']
    want = _by_hand(TicTacToeBatch, IntNet(TicTacToeBatch, recurrent), 7, 48, observation)
    assert torch.equal(res['outcome'].cpu(), want['outcome']) and torch.equal(res['length'].cpu(), want['length'])
    for k, v in want['trace'].items():
        assert torch.equal(res['trace'][k].cpu(), v), k
    assert res['results'] == _table([float(want['outcome'][g, g % 2]) for g in range(48)])


def test_modes_are_put_back_and_no_generator_is_drawn(dev):
    home, _ = _real_nets('tictactoe', dev)
    opp = copy.deepcopy(home)
    home.train()
    opp.eval()
    state = torch.get_rng_state()
    dstate = torch.cuda.get_rng_state(dev) if dev.type == 'cuda' else None
    before = [b.clone() for n in (home, opp) for b in n.buffers()]
    ev = DeviceEvaluator(TicTacToeBatch(4, dev), home, seed=SEED, opponent=opp, opening_plies=2)
    ev.evaluate(6)
    assert home.training and not opp.training
    opp.train()
    ev.evaluate(6)
    assert home.training and opp.training
    assert torch.equal(torch.get_rng_state(), state)
    if dstate is not None:
        assert torch.equal(torch.cuda.get_rng_state(dev), dstate)
    for b, old in zip([b for n in (home, opp) for b in n.buffers()], before):     # BatchNorm statistics untouched
        assert torch.equal(b, old)


def test_arguments_are_checked():
    net = IntNet(TicTacToeBatch)
    env = TicTacToeBatch(4, 'cpu')
    with pytest.raises(ValueError, match='opponent_temperature'):
        DeviceEvaluator(env, net, opponent=IntNet(TicTacToeBatch), opponent_temperature=-1.0)
    with pytest.raises(ValueError, match='opening_plies'):
        DeviceEvaluator(env, net, opening_plies=-1)
    with pytest.raises(ValueError, match='copy'):
        DeviceEvaluator(env, net, opponent=net)


def test_set_opponent_state_copies_in_place(dev):
    """The opponent's tensors keep their addresses (captured graphs address them) and the next call plays the new
    weights: with the home net's weights the match is the self-match."""
    home, opp, _, _ = _int_nets(TicTacToeBatch, dev)
    ev = DeviceEvaluator(TicTacToeBatch(7, dev), home, seed=SEED, opponent=opp, opening_plies=2)
    a = ev.evaluate(24, trace=True)
    run, ptrs = ev._run, [b.data_ptr() for b in opp.buffers()]
    ev.set_opponent_state(home.state_dict())
    b = ev.evaluate(24, trace=True)
    assert ev._run is run and ptrs == [b.data_ptr() for b in opp.buffers()]
    assert torch.equal(opp.w, home.w)
    assert not torch.equal(a['trace']['action'], b['trace']['action'])
    _same(b, _match('tictactoe', dev, 7, 24, home, copy.deepcopy(home)))


# ---- GPU only: graph against eager, the kernel against the torch formulation, whole games

@pytest.mark.gpu
@pytest.mark.parametrize('name,E,G,opening', [('tictactoe', 7, 48, 2), ('geister', 3, 4, 3)])
def test_integer_nets_graph_eager_fused_agree(cuda, monkeypatch, name, E, G, opening):
    """Identical per game: graph against eager, FUSED_EVAL on against off, and the CPU."""
    cls = _batch_cls(name)
    home, opp, cpu_home, cpu_opp = _int_nets(cls, cuda, True)
    base = _match(name, cuda, E, G, home, opp, opening, graph=True)
    _same(base, _match(name, cuda, E, G, home, opp, opening, graph=False))
    monkeypatch.setattr(evaluation, 'FUSED_EVAL', False)
    _same(base, _match(name, cuda, E, G, home, opp, opening, graph=False))
    _same(base, _match(name, cuda, E, G, home, opp, opening, graph=True))
    _same(base, _match(name, torch.device('cpu'), E, G, cpu_home, cpu_opp, opening))


@pytest.mark.gpu
@pytest.mark.parametrize('name,E,G', [('tictactoe', 7, 48), ('geister', 4, 6)])
def test_real_nets_graph_equals_eager(cuda, name, E, G):
    """The accelerated nets in two inference sessions at once; a second call reuses the graphs."""
    home, _ = _real_nets(name, cuda)
    opp = copy.deepcopy(home)
    with torch.no_grad():
        for p in opp.parameters():
            p.mul_(-0.5)
    ev = DeviceEvaluator(_batch_cls(name)(E, cuda), home, seed=SEED, opponent=opp, opening_plies=2, graph=True)
    a = ev.evaluate(G, trace=True)
    graphs = ev._run['graphs']
    b = ev.evaluate(G, trace=True)
    assert graphs is not None and ev._run['graphs'] is graphs
    _same(a, b)
    _same(a, _match(name, cuda, E, G, home, opp, graph=False))
    assert sum(a['opponent_results'].values()) == G
