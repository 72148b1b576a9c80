"""Device self-play of Hungry Geese (envs/geese.py): rates, the ply's split and the observe kernel's A/B.

    python tools/geese_selfplay_bench.py [--out profiles/geese_selfplay.txt] [--games 256 2048] [--reps 6]

On one GPU, in one call:
  * env-steps/s of ``DeviceGenerator`` over ``HungryGeeseBatch`` with a seeded-init GeeseNet, graph on, per E
    (``--reps`` calls each: their spread is the noise floor);
  * the baseline a user has without the device twin: ``HostBatchGenerator`` over the host ``Environment``;
  * the eager ply split into observe / forward / sample+record / step with HIP events (the graph replays the same
    launches without the host gaps, so the graph's ms per ply is printed beside it);
  * ``hrl_geese_observe`` with its record against the torch formulation of the same stores.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from handyrl_amd.environment import make_env  # noqa: E402
from handyrl_amd.envs.geese import GeeseNet, HungryGeeseBatch  # noqa: E402
from handyrl_amd.hostgen import HostBatchGenerator  # noqa: E402
from handyrl_amd.nn import accelerate  # noqa: E402
from handyrl_amd.rollout import DeviceGenerator, eval_mode  # noqa: E402


def device_rate(net, dev, E, reps, graph=True):
    gen = DeviceGenerator(HungryGeeseBatch(E, dev, seed=1), net, graph=graph)
    g = torch.Generator(device=dev).manual_seed(0)
    gen.generate(generator=g)
    runs = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ep = gen.generate(generator=g)
        steps, loops = int(ep['length'].sum()), int(ep['length'].max())
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        runs.append((steps / dt, dt * 1e3, loops))
    del ep
    # the parts of a call: the reset of every buffer, one replayed ply (all games live), the copy of the episode
    st = gen._st

    def timed(fn, n=1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        torch.cuda.synchronize(dev)
        del out
        return (time.perf_counter() - t0) / n * 1e3
    parts = {'reset': timed(lambda: gen._reset(st, g), 5), 'ply': timed(st['graphs'][None].replay, 100),
             'copy of the observations': timed(st['obs'].clone, 5)}
    return runs, parts


def host_rate(net, E, games):
    args = {'turn_based_training': False, 'observation': False, 'gamma': 0.8, 'compress_steps': 4}
    gen = HostBatchGenerator(lambda: make_env({'env': 'Geese'}), net, args, E=E, seed=1)
    gen.generate(E)
    t0 = time.perf_counter()
    eps = gen.generate(games)
    dt = time.perf_counter() - t0
    return sum(ep['steps'] for ep in eps) / dt


class Stamps:
    """HIP events around the pieces of one eager ply: the env's observe and step calls and the net's forward."""

    def __init__(self):
        self.marks = {}

    def mark(self, name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.marks[name] = ev

    def wrap(self, fn, name):
        def call(*a, **k):
            self.mark(name + '0')
            out = fn(*a, **k)
            self.mark(name + '1')
            return out
        return call

    def ms(self, a, b):
        return self.marks[a].elapsed_time(self.marks[b])


def ply_split(net, dev, E, plies=22):
    env = HungryGeeseBatch(E, dev, seed=1)
    gen = DeviceGenerator(env, net, graph=False)
    st = gen._state()
    gen._reset(st, torch.Generator(device=dev).manual_seed(0))
    s = Stamps()
    env.observe_players_record = s.wrap(env.observe_players_record, 'observe')
    env.step_players = s.wrap(env.step_players, 'step')
    hooks = [net.register_forward_pre_hook(lambda *_: s.mark('forward0')),
             net.register_forward_hook(lambda *_: s.mark('forward1'))]
    rows = []
    with torch.no_grad(), eval_mode(net):
        for _ in range(plies):
            s.mark('ply0')
            gen._ply(st, None)
            s.mark('ply1')
            torch.cuda.synchronize(dev)
            rows.append({'masks': s.ms('ply0', 'observe0'), 'observe': s.ms('observe0', 'observe1'),
                         'forward': s.ms('forward0', 'forward1'), 'sample+record': s.ms('forward1', 'step0'),
                         'step': s.ms('step0', 'step1'), 'ply': s.ms('ply0', 'ply1')})
    for h in hooks:
        h.remove()
    rows = rows[2:]                      # the first plies warm the allocator
    return {k: sum(r[k] for r in rows) / len(rows) for k in rows[0]}


def observe_ab(dev, E, iters={'kernel': 5000, 'torch': 500}):
    env = HungryGeeseBatch(E, dev, seed=1)
    Tm = env.MAX_PLIES
    rec = torch.zeros(E, Tm, 4, *env.OBS_SHAPE, device=dev)
    t = torch.full((1,), 5, dtype=torch.long, device=dev)
    infer = env.turns_mask()

    def kernel():
        return env.observe_players_record(rec, t, infer)

    def torch_ops():
        views = env.views_torch()
        keep = infer.view(E, 4, 1, 1, 1)
        rec.index_copy_(1, t, torch.where(keep, views.transpose(0, 1), 0).unsqueeze(1))
        return views.view(4 * E, *env.OBS_SHAPE)
    assert torch.equal(kernel(), torch_ops())
    out = {'kernel': [], 'torch': []}
    for _ in range(2):                   # the two forms alternate; each window is a tenth of a second or more
        for name, fn in (('kernel', kernel), ('torch', torch_ops)):
            for _ in range(3):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters[name]):
                fn()
            b.record()
            torch.cuda.synchronize(dev)
            out[name].append(a.elapsed_time(b) / iters[name] * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/geese_selfplay.txt')
    ap.add_argument('--games', type=int, nargs='+', default=[256, 2048])
    ap.add_argument('--reps', type=int, default=6)
    ap.add_argument('--host-games', type=int, default=256)
    opts = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    net = accelerate(GeeseNet().to(dev))
    lines = ['Hungry Geese device self-play, seeded-init GeeseNet, %s' % torch.cuda.get_device_name(dev)]

    def say(line):
        lines.append(line)
        print(line, flush=True)
    for E in opts.games:
        runs, parts = device_rate(net, dev, E, opts.reps)
        for steps_s, ms, loops in runs:
            say('device  E=%-5d graph: %10.0f env-steps/s  %.1f ms per call  (longest game %d plies)'
                % (E, steps_s, ms, loops))
        say('parts   E=%-5d ms: %s;  %d games x 1 ply / ply time = %.0f env-steps/s while every game is live'
            % (E, '  '.join('%s %.3f' % kv for kv in parts.items()), E, E / parts['ply'] * 1e3))
    rate = host_rate(net, min(256, opts.host_games), opts.host_games)
    say('host    E=%-5d HostBatchGenerator over the host Environment, forward on the GPU: %10.0f env-steps/s'
        % (min(256, opts.host_games), rate))
    for E in opts.games:
        split = ply_split(net, dev, E)
        say('split   E=%-5d eager ply, HIP events, ms: %s' % (E, '  '.join('%s %.3f' % kv for kv in split.items())))
    for E in opts.games:
        ab = observe_ab(dev, E)
        say('observe E=%-5d views + record, us per call, two runs: hrl_geese_observe %s   torch ops %s'
            % (E, ' '.join('%.1f' % x for x in ab['kernel']), ' '.join('%.1f' % x for x in ab['torch'])))
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
