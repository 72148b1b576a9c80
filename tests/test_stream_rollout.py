"""rollout.StreamGenerator: every episode it puts into the ring is refereed on its own.

A game's uniforms depend on (seed, game number, ply, label) only, so a ring row with game number n can be checked
without knowing in which slot or when it was played: the recorded actions are replayed through a fresh one-game CPU
batch (rules, observations, masks, outcome), the sampling is redone from ``stream_uniforms`` (exact), the net's
outputs are compared with an eval forward on the recorded observations (1e-5 absolute, the project's self-play bound
of test_gpu_selfplay_2048_games_matches_per_game_loop) and the returns with the fp64 discounted sum (exact).
"""

import numpy as np
import pytest
import torch

from handyrl_amd import rollout
from handyrl_amd.rollout import DeviceReplay, StreamGenerator, TicTacToeBatch, stream_uniforms

DEVICES = ['cpu', pytest.param('cuda', marks=pytest.mark.gpu)]
GAMMA = 0.8


@pytest.fixture(params=DEVICES)
def dev(request):
    if request.param == 'cuda':
        return request.getfixturevalue('cuda')
    return torch.device('cpu')


def _nets(name, dev):
    """(the net the generator plays with on ``dev``, its CPU twin with the same weights)."""
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


def _batch_cls(name):
    if name == 'tictactoe':
        return TicTacToeBatch
    from handyrl_amd.envs.geister import GeisterBatch
    return GeisterBatch


def _make(name, dev, E, N, seed, **kw):
    cls = _batch_cls(name)
    net, cpu = _nets(name, dev)
    replay = DeviceReplay(N, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P, dev, obs_dtype=torch.uint8)
    gen = StreamGenerator(cls(E, dev), net, replay, gamma=GAMMA, seed=seed, **kw)
    return gen, replay, cpu


def _rows(replay, gen, rows):
    """The ring rows ``rows`` as CPU tensors."""
    idx = torch.as_tensor(rows, device=replay.policy.device)
    out = {k: getattr(replay, k)[idx].cpu() for k in ('policy', 'amask', 'action', 'value', 'turn', 'reward', 'ret',
                                                       'length', 'outcome')}
    obs = replay.obs if isinstance(replay.obs, dict) else {'': replay.obs}
    out['obs'] = {k: v[idx].cpu() for k, v in obs.items()}
    out['game'] = gen.ring_game[idx].cpu()
    return out


def _same(a, b):
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        else:
            assert torch.equal(rollout_bits(a[k]), rollout_bits(b[k])), k


def rollout_bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _net_check(cpu_net, rec, P):
    """3. policy (at the legal labels) and value against the CPU net's eval forward on the recorded observations
    (equal to the env's, checked before), the hidden state carried per game and player from zeros.  The games
    advance together, one forward per ply and mover over the games that are still running."""
    lengths = rec['length'].tolist()
    R = len(lengths)
    recurrent = hasattr(cpu_net, 'init_hidden')
    hidden = {p: [[h.clone() for h in hs] for hs in cpu_net.init_hidden([R])] for p in range(P)} if recurrent else None
    for t in range(max(lengths)):
        for p in range(P):
            idx = [i for i in range(R) if lengths[i] > t and int(rec['turn'][i, t]) == p]
            if not idx:
                continue
            ix = torch.tensor(idx)
            obs = {k: v[ix, t].float() for k, v in rec['obs'].items()}
            h = [[x[ix] for x in hs] for hs in hidden[p]] if recurrent else None
            out = cpu_net(obs if '' not in obs else obs[''], h)
            if recurrent:
                for hs, new in zip(hidden[p], out['hidden']):
                    for x, nx in zip(hs, new):
                        x[ix] = nx
            legal = rec['amask'][ix, t] == 0
            dp = torch.where(legal, (rec['policy'][ix, t] - out['policy'].float()).abs(), 0.0).max()
            dv = (rec['value'][ix, t] - out['value'].float().reshape(-1)).abs().max()
            assert float(dp) <= 1e-5 and float(dv) <= 1e-5, (t, p, float(dp), float(dv))


def referee(name, gen, replay, cpu_net, rows):
    """Checks 1-5 of the module doc for the ring rows ``rows``; returns their lengths."""
    cls = _batch_cls(name)
    Tm, A, P = cls.MAX_PLIES, cls.A, cls.P
    rec = _rows(replay, gen, rows)
    one = torch.ones(1, dtype=torch.bool)
    sample_game, sample_ply, sample_row = [], [], []
    has_reward = hasattr(cls, 'reward')
    with torch.no_grad():
        for i, row in enumerate(rows):
            n, L = int(rec['game'][i]), int(rec['length'][i])
            assert 0 <= n < gen.games_started and 1 <= L <= Tm, (row, n, L)
            b = cls(1, 'cpu')
            rewards = np.zeros((L, P), dtype=np.float64)
            for t in range(L):
                assert not bool(b.terminal()), (row, t)
                turn = b.turn()
                assert int(rec['turn'][i, t]) == int(turn), (row, t)
                obs = b.observation(turn)
                obs_d = obs if isinstance(obs, dict) else {'': obs}
                for k, v in obs_d.items():       # exact: the ring holds the binary planes as uint8
                    assert torch.equal(rec['obs'][k][i, t].float(), v[0]), (row, t, k)
                legal = b.legal()[0]
                assert torch.equal(rec['amask'][i, t], torch.where(legal, 0.0, 1e32)), (row, t)
                a = int(rec['action'][i, t])
                assert bool(legal[a]), (row, t, a)
                b.step(torch.tensor([a]), one)
                if has_reward:
                    rewards[t] = b.reward()[0].double().numpy()
                sample_game.append(n)
                sample_ply.append(t)
                sample_row.append((i, t))
            assert bool(b.terminal()), (row, L)
            assert torch.equal(rec['outcome'][i], b.outcome()[0].float()), row
            # 4. returns: fp32 of the fp64 discounted sum; the reward: fp32 of the env's
            ret = np.zeros((L, P), dtype=np.float64)
            acc = np.zeros(P, dtype=np.float64)
            for t in range(L - 1, -1, -1):
                acc = rewards[t] + GAMMA * acc
                ret[t] = acc
            assert np.array_equal(rec['ret'][i, :L].numpy(), ret.astype(np.float32)), row
            assert np.array_equal(rec['reward'][i, :L].numpy(), rewards.astype(np.float32)), row
            # 5. the reset values past the end
            for k, v in rec['obs'].items():
                assert not bool(v[i, L:].any()), (row, k)
            assert not bool(rec['policy'][i, L:].any()) and bool((rec['amask'][i, L:] == 1e32).all()), row
            for k in ('action', 'value', 'turn', 'reward', 'ret'):
                assert not bool(rec[k][i, L:].any()), (row, k)
        _net_check(cpu_net, rec, P)
    # 2. sampling, on the device the generator ran on, exact
    dev = replay.policy.device
    u = torch.from_numpy(stream_uniforms(gen.seed, np.array(sample_game), np.array(sample_ply), A)).to(dev)
    ii = torch.tensor([s[0] for s in sample_row])
    tt = torch.tensor([s[1] for s in sample_row])
    pol = rec['policy'][ii, tt].to(dev)
    act = torch.argmax(pol - torch.log(-torch.log(u)), dim=-1).cpu()
    assert torch.equal(act, rec['action'][ii, tt])
    return rec['length'].tolist()


def _written_rows(replay):
    return list(range(replay.count))


def _bookkeeping(gen, replay, outs, ptr0=0):
    emitted = sum(o['episodes'] for o in outs)
    st = gen._state()
    ring_ptr, dev_emitted, next_game = st['state'].tolist()
    assert dev_emitted == emitted and replay.ptr == ring_ptr == (ptr0 + emitted) % replay.N
    assert replay.count == min(emitted, replay.N)
    assert gen.games_started == next_game == gen.env.E + emitted
    games = gen.ring_game[:replay.count].tolist()
    assert len(set(games)) == len(games) and all(0 <= g < gen.games_started for g in games)
    assert bool((gen.ring_game[replay.count:] == -1).all())
    return emitted


def test_tictactoe_stream_is_refereed(dev):
    """E = 7 (not a multiple of the tail's 4 games per workgroup), N = 40, 64 episodes: the ring wraps."""
    gen, replay, cpu = _make('tictactoe', dev, 7, 40, seed=5)
    out = gen.generate(64)
    assert out['episodes'] >= 64 and out['plies'] % 16 == 0
    emitted = _bookkeeping(gen, replay, [out])
    assert emitted >= 3 * 7                 # more games than slots three times over: the slots restarted
    lengths = referee('tictactoe', gen, replay, cpu, _written_rows(replay))
    assert all(5 <= n <= 9 for n in lengths)
    # the ring holds the newest 40 games, the oldest of them at the ring pointer
    assert int(gen.ring_game.min()) == int(gen.ring_game[replay.ptr])


def test_geister_stream_is_refereed(dev):
    gen, replay, cpu = _make('geister', dev, 6, 8, seed=9)
    out = gen.generate(10)
    assert out['episodes'] >= 10
    _bookkeeping(gen, replay, [out])
    lengths = referee('geister', gen, replay, cpu, _written_rows(replay))
    assert all(3 <= n <= 202 for n in lengths)


def _emission_order(gen, replay, count):
    """With a ring that has not wrapped (row k = the k-th emitted game): each row's slot and the step its game
    ended at, rebuilt from the restart rule alone -- initial game n sits in slot n and starts at step 0; the game
    started by the k-th emission has number E + k, takes that game's slot and starts at the next even step."""
    E, P = gen.env.E, gen.env.P
    games = gen.ring_game[:count].tolist()
    lengths = replay.length[:count].tolist()
    slot, start = {n: n for n in range(E)}, {n: 0 for n in range(E)}
    rows = []
    for k, (n, L) in enumerate(zip(games, lengths)):
        assert n in slot, 'row %d holds game %d, which no earlier emission started' % (k, n)
        end = start[n] + L
        rows.append((end, slot[n]))
        slot[E + k], start[E + k] = slot[n], -(-end // P) * P
    return rows


def test_tictactoe_stream_is_deterministic_and_ordered(dev):
    """The same seed and E: one generate(64), four generate(16) and check_every = 1 emit the same first 64
    episodes, bit for bit; rows appear in step order and, within a step, in slot order."""
    runs = []
    for calls, kw in (((64,), {}), ((16, 16, 16, 16), {}), ((64,), {'check_every': 1})):
        gen, replay, _ = _make('tictactoe', dev, 7, 128, seed=5, **kw)
        outs = [gen.generate(n) for n in calls]
        emitted = _bookkeeping(gen, replay, outs)
        assert 64 <= emitted <= 128
        if kw:
            assert all(o['plies'] >= 1 for o in outs) and emitted < 64 + 7
        assert sum(o['env_steps'] for o in outs) == int(replay.length[:emitted].sum())
        runs.append((gen, replay, emitted, _rows(replay, gen, list(range(64)))))
    for other in runs[1:]:
        _same(runs[0][3], other[3])
    gen, replay, emitted, rec = runs[0]
    rows = _emission_order(gen, replay, emitted)
    assert rows == sorted(rows), 'rows are not in (step, slot) order'
    per_slot = {}
    for _, s in rows:
        per_slot[s] = per_slot.get(s, 0) + 1
    assert max(per_slot.values()) >= 3
    lengths = rec['length'].tolist()
    odd = sum(n % 2 for n in lengths)
    assert odd >= 10 and 64 - odd >= 10, (odd, 64 - odd)     # one-ply waits and none, both well represented
    # the N = 40 run of the referee test plays the same games: its ring holds this run's episodes 25..64
    assert len({(e, s) for e, s in rows}) == len(rows)


@pytest.mark.gpu
def test_graph_mode_equals_eager_mode(cuda):
    recs = []
    for graph in (True, False):
        gen, replay, _ = _make('tictactoe', cuda, 7, 128, seed=5, graph=graph)
        outs = [gen.generate(32), gen.generate(32)]
        assert (gen._graphs is not None) == graph
        emitted = _bookkeeping(gen, replay, outs)
        recs.append((emitted, _rows(replay, gen, list(range(128)))))
    assert recs[0][0] == recs[1][0]
    _same(recs[0][1], recs[1][1])       # every row, the unwritten ones included: capture left no trace


@pytest.mark.gpu
def test_recapture_keeps_the_games(cuda):
    """The net's tensors move between two calls (same values): the plies are captured again and the games in
    flight go on, so the ring equals that of a run whose tensors stayed."""
    recs = []
    for move in (False, True):
        gen, replay, _ = _make('tictactoe', cuda, 7, 128, seed=5)
        outs = [gen.generate(32)]
        graphs = gen._graphs
        if move:
            for p in list(gen.net.parameters()) + list(gen.net.buffers()):
                p.data = p.data.clone()
        outs.append(gen.generate(32))
        assert (gen._graphs is not graphs) == move
        emitted = _bookkeeping(gen, replay, outs)
        recs.append((emitted, _rows(replay, gen, list(range(128)))))
    assert recs[0][0] == recs[1][0]
    _same(recs[0][1], recs[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize('name,E,N,n', [('tictactoe', 7, 128, 32), ('geister', 6, 16, 4)])
def test_fused_stream_equals_torch_formulation(cuda, monkeypatch, name, E, N, n):
    """FUSED_STREAM on and off give the same ring, bit for bit, over two calls; the second replays the graphs the
    first captured."""
    recs = []
    for fused in (True, False):
        monkeypatch.setattr(rollout, 'FUSED_STREAM', fused)
        gen, replay, _ = _make(name, cuda, E, N, seed=5)
        outs = [gen.generate(n)]
        graphs = gen._graphs
        outs.append(gen.generate(n))
        assert gen._graphs is graphs and graphs is not None
        emitted = _bookkeeping(gen, replay, outs)
        assert emitted <= N
        recs.append((emitted, _rows(replay, gen, list(range(N)))))
    assert recs[0][0] == recs[1][0]
    _same(recs[0][1], recs[1][1])


def test_out_of_scope_requests_name_the_lockstep_generator():
    from handyrl_amd.envs.tictactoe import SimpleConv2dModel
    from handyrl_amd.rollout import ParallelTicTacToeBatch, PlayerReplay
    net = SimpleConv2dModel()
    cls = TicTacToeBatch
    replay = DeviceReplay(8, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P, 'cpu')
    preplay = PlayerReplay(8, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P, 'cpu')
    for env, rep, kw in ((ParallelTicTacToeBatch(4, 'cpu'), replay, {}), (cls(4, 'cpu'), preplay, {}),
                         (cls(4, 'cpu'), replay, {'observation': True}),
                         (cls(4, 'cpu'), replay, {'per_player': True})):
        with pytest.raises(ValueError, match='DeviceGenerator'):
            StreamGenerator(env, net, rep, **kw)
