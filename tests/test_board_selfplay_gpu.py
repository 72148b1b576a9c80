"""Whole TicTacToe self-play games in one launch on the GPU (csrc/hrl_boardplay.hip).

The entry against the path it replaces (the eager lockstep generator with ``nn.BoardInference``), bit for bit, on
guard-band buffers; split calls against one call; ``DeviceGenerator(fused_game=True)`` against the same generator
without the option over two calls with the weights changed in between; a referee that does not use the unfused GPU
path (the rules on a one-game CPU env, the Gumbel-max of the recorded policy, policy / value against the fp64 forward
at 1e-5: the fp32 forward's own distance from fp64 is below 1e-6, tests/test_board_infer_abi.py); what is launched;
training through ``loop.SelfPlayTrainer`` and ``main.train_main``.
"""

import copy
import os

import pytest
import torch

from handyrl_amd import _native
from handyrl_amd import nn as hnn
from handyrl_amd.rollout import DeviceGenerator, TicTacToeBatch

from . import board_infer_util as util
from .guarded import Arena, bits
from .test_board_infer_rollout import _equal_tree
from .test_main_entry import _small

pytestmark = pytest.mark.gpu

Tm = TicTacToeBatch.MAX_PLIES
RECORDS = (('observation', (27,), torch.float32), ('policy', (9,), torch.float32),
           ('action_mask', (9,), torch.float32), ('action', (), torch.long), ('value', (), torch.float32),
           ('turn', (), torch.long))


def _net(dev, layers=3, seed=0):
    return copy.deepcopy(util.seeded_net(layers, seed=seed)).to(dev).eval()


def _G(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _uniforms(dev, E, seed):
    return torch.rand((Tm, E, 9), generator=_G(dev, seed), device=dev).clamp_(1e-20, 1.0)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(bits(a).cpu(), bits(b).cpu()), what


def _entry(wrapped, E, U, splits):
    """hrl_board_selfplay over the ply ranges ``splits`` on fresh guard-band buffers and a fresh game state, inside
    the wrapper's session; returns the records and the final state (the arena is checked)."""
    dev = U.device
    arena = Arena(dev)
    rec = {k: arena.out((E, Tm) + tail, dtype, name=k) for k, tail, dtype in RECORDS}
    env = TicTacToeBatch(E, dev)
    state = {k: arena.inout(getattr(env, k), name=k) for k in ('board', 'color', 'nmoves', 'winner')}
    with torch.no_grad(), wrapped.inference_session():
        for t0, t1 in splits:
            _native.check(_native.load().hrl_board_selfplay(
                _native.ptr(wrapped.pack(dev)), wrapped.layers, E, Tm, t0, t1, _native.ptr(U),
                _native.ptr(state['board']), _native.ptr(state['color']), _native.ptr(state['nmoves']),
                _native.ptr(state['winner']), _native.ptr(rec['observation']), _native.ptr(rec['policy']),
                _native.ptr(rec['action_mask']), _native.ptr(rec['action']), _native.ptr(rec['value']),
                _native.ptr(rec['turn']), _native.stream_of(dev)), 'hrl_board_selfplay')
    arena.check()
    return {k: v.clone() for k, v in rec.items()}, {k: v.clone() for k, v in state.items()}


@pytest.mark.parametrize('layers', [1, 3])
@pytest.mark.parametrize('E', [1, 15, 16, 17, 33])
def test_entry_equals_the_eager_generator(cuda, E, layers):
    seed = 100 + E
    wrapped = hnn.BoardInference(_net(cuda, layers))
    ref = DeviceGenerator(TicTacToeBatch(E, cuda), wrapped, graph=False).generate(generator=_G(cuda, seed))
    rec, state = _entry(wrapped, E, _uniforms(cuda, E, seed), [(0, Tm)])
    for k, tail, _ in RECORDS:
        _same_bits(rec[k], ref[k].reshape((E, Tm) + tail), k)
    assert torch.equal(state['nmoves'].long(), ref['length'])
    assert torch.equal(state['winner'].float(), ref['outcome'][:, 0])
    assert bool(((ref['length'] >= 5) & (ref['length'] <= 9)).all())


def test_split_calls_equal_one_call(cuda):
    E = 17
    wrapped = hnn.BoardInference(_net(cuda))
    U = _uniforms(cuda, E, 7)
    whole = _entry(wrapped, E, U, [(0, Tm)])
    for splits in ([(0, 4), (4, Tm)], [(t, t + 1) for t in range(Tm)]):
        part = _entry(wrapped, E, U, splits)
        for a, b in zip(whole, part):
            for k in a:
                _same_bits(a[k], b[k], (k, splits))
    assert int(whole[1]['nmoves'].min()) >= 5


def _perturb(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.add_((0.01 * torch.randn(m.weight.shape, generator=g)).to(m.weight.device))


@pytest.mark.parametrize('graph', [None, False])
@pytest.mark.parametrize('E', [1, 17, 64])
def test_generator_option_equals_the_ply_loop(cuda, E, graph):
    runs = []
    for fused in (False, True):
        net = _net(cuda)
        gen = DeviceGenerator(TicTacToeBatch(E, cuda), hnn.BoardInference(net), graph=graph, fused_game=fused)
        g = _G(cuda, 11)
        eps = [gen.generate(generator=g)]
        _perturb(net, 5)                                     # the second call must play the repacked weights
        eps.append(gen.generate(generator=g))
        assert (gen._st['graphs'] is None) == (fused or graph is False)
        runs.append(eps)
    for a, b in zip(*runs):
        _equal_tree(a, b)
        assert {'return', 'reward'} <= set(b)
        assert b['length'].shape == (E,) and b['length'].dtype == torch.long
        assert b['outcome'].shape == (E, 2) and b['outcome'].dtype == torch.float32
        assert b['action'].shape == (E, Tm) and b['action'].dtype == torch.long
    assert not torch.equal(bits(runs[1][0]['policy']).cpu(), bits(runs[1][1]['policy']).cpu())


def test_fused_games_are_refereed(cuda):
    E = 64
    net = _net(cuda)
    gen = DeviceGenerator(TicTacToeBatch(E, cuda), hnn.BoardInference(net), fused_game=True)
    ep = gen.generate(generator=_G(cuda, 1))
    U = gen._st['U']
    # the argmax as sample_record_torch forms it, on the device, from the recorded policy and the call's uniforms
    picked = torch.argmax(ep['policy'] - torch.log(-torch.log(U.permute(1, 0, 2))), dim=-1).cpu()
    ep = {k: v.cpu() for k, v in ep.items()}
    one = torch.ones(1, dtype=torch.bool)
    lengths, outcomes, obs, legal, rows = [], set(), [], [], []
    for e in range(E):
        b = TicTacToeBatch(1, 'cpu')
        L = int(ep['length'][e])
        assert 5 <= L <= 9
        for t in range(L):
            assert not bool(b.terminal())
            o = b.observation(b.turn())[0]
            assert torch.equal(ep['observation'][e, t], o)
            assert int(ep['turn'][e, t]) == t % 2
            lg = b.legal()[0]
            assert torch.equal(ep['action_mask'][e, t], torch.where(lg, 0.0, 1e32).float())
            a = int(ep['action'][e, t])
            assert bool(lg[a]) and a == int(picked[e, t])
            obs.append(o)
            legal.append(lg)
            rows.append((e, t))
            b.step(torch.tensor([a]), one)
        assert bool(b.terminal())
        assert torch.equal(ep['outcome'][e], b.outcome()[0])
        # every slot at or after the end holds the reset values
        assert not ep['observation'][e, L:].any() and not ep['policy'][e, L:].any()
        assert bool((ep['action_mask'][e, L:] == 1e32).all())
        assert not ep['action'][e, L:].any() and not ep['value'][e, L:].any() and not ep['turn'][e, L:].any()
        lengths.append(L)
        outcomes.add(float(ep['outcome'][e, 0]))
    assert not ep['return'].any() and not ep['reward'].any()
    assert len(lengths) == E and min(lengths) < 9 and max(lengths) == 9
    p64, v64 = util.forward64(net, torch.stack(obs))
    es, ts = torch.tensor(rows).t()
    verr = (ep['value'][es, ts].double() - v64.reshape(-1)).abs().max().item()
    lg = torch.stack(legal)
    perr = ((ep['policy'][es, ts].double() - p64).abs() * lg).max().item()
    print('fused game referee: %d plies, lengths %s, outcomes %s, value err %.3g, policy err %.3g'
          % (len(rows), sorted(set(lengths)), sorted(outcomes), verr, perr))
    assert verr <= 1e-5 and perr <= 1e-5


def _kernel_names(cuda, gen):
    from torch.profiler import ProfilerActivity, profile
    for _ in range(2):                                      # warm: every lazy initialisation is done
        gen.generate(generator=_G(cuda, 2))
    torch.cuda.synchronize(cuda)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        gen.generate(generator=_G(cuda, 2))
        torch.cuda.synchronize(cuda)
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_what_runs(cuda):
    """The plain call is profiled eager (graph=False): its launches are then counted one by one."""
    E = 64
    net = _net(cuda)
    fused = _kernel_names(cuda, DeviceGenerator(TicTacToeBatch(E, cuda), hnn.BoardInference(net), fused_game=True))
    plain = _kernel_names(cuda, DeviceGenerator(TicTacToeBatch(E, cuda), hnn.BoardInference(net), graph=False))
    print('generate() at E = 64: %d kernels with fused_game, %d without' % (len(fused), len(plain)))

    def count(names, part):
        return sum(part in n for n in names)
    assert count(fused, 'board_selfplay_kernel') == 1
    assert count(fused, 'board_infer_pack_kernel') == 1
    assert count(fused, 'board_infer_kernel') == 0 and count(fused, 'sample_record_kernel') == 0
    assert count(plain, 'board_selfplay_kernel') == 0 and count(plain, 'board_infer_kernel') == Tm
    assert 0 < len(fused) < len(plain)


def test_trainer_with_the_option_trains_the_same(cuda):
    from handyrl_amd.loop import SelfPlayTrainer
    args = _small()['train_args']
    args.update(batch_size=16, forward_steps=4)
    trainers = []
    for fused in (False, True):
        net = _net(cuda)
        net.train()
        tr = SelfPlayTrainer(net, dict(args), cuda, games_per_round=64, capacity=256, seed=3, fused_inference=True,
                             fused_game=fused)
        assert tr.gen.fused_game == fused
        for _ in range(2):
            tr.generate()
            tr.train_steps(2)
        trainers.append(tr)
    a, b = trainers
    sa, sb = a.play_net.state_dict(), b.play_net.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        _same_bits(sa[k], sb[k], k)
    for k in ('obs', 'policy', 'amask', 'action', 'value', 'turn', 'reward', 'ret', 'length', 'outcome'):
        _same_bits(getattr(a.replay, k), getattr(b.replay, k), k)
    assert a.replay.count == b.replay.count == 128 and a.steps == b.steps == 4


def test_train_main_with_the_fused_game(tmp_path, cuda, monkeypatch):
    from handyrl_amd import rollout
    from handyrl_amd.main import train_main
    calls = []
    real = rollout.DeviceGenerator._generate_fused
    monkeypatch.setattr(rollout.DeviceGenerator, '_generate_fused',
                        lambda self, st, g: (calls.append(1), real(self, st, g))[1])
    args = _small()
    args['train_args'].update(inference='fused', self_play='fused', epochs=1)
    model = train_main(args, device=cuda, model_dir=str(tmp_path), log=lambda *_: None)
    assert calls                                            # the games were played by the one-launch path
    saved = torch.load(os.path.join(str(tmp_path), '1.pth'), weights_only=True)
    assert set(saved) == set(model.state_dict())
    assert all(torch.isfinite(v.float()).all() for v in saved.values())
    # without the inference key the self_play key raises by name, before anything is played
    del calls[:]
    bad = _small()
    bad['train_args'].update(self_play='fused', epochs=1)
    with pytest.raises(ValueError, match='self_play'):
        train_main(bad, device=cuda, model_dir=str(tmp_path / 'bad'), log=lambda *_: None)
    assert not calls
