"""Device self-play of Hungry Geese (envs/geese.py): rates, the ply's split and the observe kernel's A/B.

    python tools/geese_selfplay_bench.py [--out profiles/geese_selfplay.txt] [--games 256 2048] [--reps 6]

On one GPU, in one call:
  * env-steps/s of ``DeviceGenerator`` over ``HungryGeeseBatch`` with a seeded-init GeeseNet, graph on, per E
    (``--reps`` calls each: their spread is the noise floor);
  * the baseline a user has without the device twin: ``HostBatchGenerator`` over the host ``Environment``;
  * the eager ply split into observe / forward / sample+record / step with HIP events (the graph replays the same
    launches without the host gaps, so the graph's ms per ply is printed beside it);
  * ``hrl_geese_observe`` with its record against the torch formulation of the same stores.

    python tools/geese_selfplay_bench.py --stream [--out profiles/geese_stream.txt] [--games 2048 256] [--reps 6]

The streaming generator against the lockstep one, in one process and in alternating order, per E:
  * lockstep ``generate()`` + ``replay.add`` and ``PlayerStreamGenerator.generate(E)``: env-steps/s, ms per global
    step and the share of the forward's rows that belong to live games, ``--reps`` (at least six) calls each;
  * the stream step's harvest and observe launches on their own (device events behind a spinning kernel, so the host's
    preparation of a call is not in the window).
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
from handyrl_amd import rollout  # noqa: E402
from handyrl_amd.rollout import DeviceGenerator, PlayerReplay, PlayerStreamGenerator, eval_mode  # noqa: E402


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


def _event_us(fn, iters, before=None):
    """Device time of ``fn`` alone, one pair of events per call: (median, min, max) in us over ``iters`` calls;
    ``before`` runs ahead of each call outside the events (it puts back what ``fn`` consumes)."""
    times = []
    for _ in range(iters):
        if before is not None:
            before()
        torch.cuda._sleep(2000000)       # the device is busy while the host enqueues: the window holds no host time
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def stream_ab(net, dev, E, reps, say):
    """Lockstep ``generate() + replay.add`` against stream ``generate(E)`` in alternating order, the same net, seed,
    E and ring size in one process; then the stream step's harvest and observe launches on their own."""
    def replay():
        return PlayerReplay(E, HungryGeeseBatch.MAX_PLIES, HungryGeeseBatch.OBS_SHAPE, 4, 4, dev,
                            obs_dtype=torch.uint8, solo=True)
    Tm = HungryGeeseBatch.MAX_PLIES
    lock, lock_replay = DeviceGenerator(HungryGeeseBatch(E, dev, seed=1), net), replay()
    stream = PlayerStreamGenerator(HungryGeeseBatch(E, dev, seed=1), net, replay(), seed=1)
    g = torch.Generator(device=dev).manual_seed(0)
    lock_replay.add(lock.generate(generator=g))          # both capture their graphs and warm every shape
    stream.generate(E)
    st = stream._state()
    rows = {'lockstep': [], 'stream': []}
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ep = lock.generate(generator=g)
        lock_replay.add(ep)
        steps, longest = int(ep['length'].sum()), int(ep['length'].max())
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        del ep
        plies = min(Tm, -(-longest // lock.check_every) * lock.check_every)     # the loop looks every check_every plies
        rows['lockstep'].append((steps / dt, dt * 1e3, plies, dt * 1e3 / plies, steps / (plies * E), E))
        live0 = int(st['played'].sum())
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = stream.generate(E)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        live = int(st['played'].sum()) - live0
        rows['stream'].append((out['env_steps'] / dt, dt * 1e3, out['plies'], dt * 1e3 / out['plies'],
                               live / (out['plies'] * E), out['episodes']))
    for name in ('lockstep', 'stream'):
        for rate, ms, plies, per, share, eps in rows[name]:
            say('%-8s E=%-5d %10.0f env-steps/s  %8.1f ms per call  %3d global steps  %.3f ms per step  '
                'live rows %.3f  %d episodes' % (name, E, rate, ms, plies, per, share, eps))
    med = {k: sorted(r[0] for r in v)[len(v) // 2] for k, v in rows.items()}
    per_step = sorted(r[3] for r in rows['stream'])[reps // 2]
    say('ratio    E=%-5d stream / lockstep, medians of %d alternating calls: %.2f   (stream %.0f, lockstep %.0f '
        'env-steps/s; a step of all-live rows would give E / ms per step = %.0f env-steps/s)'
        % (E, reps, med['stream'] / med['lockstep'], med['stream'], med['lockstep'], E / per_step * 1e3))
    # the harvest on its own: as many done slots as a step of the runs above ends on average, spread over the slots,
    # each a game of the runs' mean length; the slots' state is put back before every call
    ended = max(1, round(sum(r[5] for r in rows['stream']) / sum(r[2] for r in rows['stream'])))
    length = max(1, round(sum(r[0] * r[1] for r in rows['stream']) / 1e3 / sum(r[5] for r in rows['stream'])))
    done = torch.zeros(E, dtype=torch.bool, device=dev)
    done[torch.linspace(0, E - 1, ended, device=dev).long()] = True
    keep = {k: st[k].clone() for k in ('ply', 'game', 'pending', 'state')}
    outcome = stream.env.outcome()

    def put_back():
        for k, v in keep.items():
            st[k].copy_(v)
        st['ply'].fill_(length)
    us = _event_us(lambda: rollout.harvest_players_hip(st, done, outcome, 0.8, stream.replay, stream.ring_game),
                   50, put_back)
    for k, v in keep.items():
        st[k].copy_(v)
    row_bytes = sum(getattr(stream.replay, k)[0].numel() * getattr(stream.replay, k).element_size()
                    for k in ('policy', 'amask', 'action', 'value', 'tmask', 'omask', 'reward', 'ret'))
    row_bytes += stream.replay.obs[0].numel()
    say('harvest  E=%-5d hrl_selfplay_harvest_players, %d done slots of %d plies, both launches, us: median %.1f  '
        'min %.1f  max %.1f   (%.1f MB of ring rows stored: %.0f GB/s)'
        % (E, ended, length, *us, ended * row_bytes / 1e6, ended * row_bytes / us[0] / 1e3))
    env = stream.env
    active = env.active().clone()
    infer = env.turns_mask()
    ply = torch.full((E,), 5, dtype=torch.long, device=dev)
    us = _event_us(lambda: env.observe_players_record_at(st['obs'], ply, infer, active), 200)
    rec32 = torch.zeros(E, 8, 4, *env.OBS_SHAPE, device=dev)
    t = torch.full((1,), 5, dtype=torch.long, device=dev)
    us32 = _event_us(lambda: env.observe_players_record(rec32, t, infer), 200)
    say('observe  E=%-5d views + record, us: hrl_geese_observe_at (uint8 record) median %.1f  min %.1f  max %.1f;  '
        'hrl_geese_observe (fp32 record) median %.1f  min %.1f  max %.1f' % (E, *us, *us32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--games', type=int, nargs='+', default=[256, 2048])
    ap.add_argument('--reps', type=int, default=6)
    ap.add_argument('--host-games', type=int, default=256)
    ap.add_argument('--stream', action='store_true',
                    help='lockstep against rollout.PlayerStreamGenerator in alternating order (default --out '
                         'profiles/geese_stream.txt) instead of the lockstep report')
    opts = ap.parse_args()
    opts.out = opts.out or ('profiles/geese_stream.txt' if opts.stream else 'profiles/geese_selfplay.txt')
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    net = accelerate(GeeseNet().to(dev))
    lines = ['Hungry Geese device self-play, seeded-init GeeseNet, %s' % torch.cuda.get_device_name(dev)]

    def say(line):
        lines.append(line)
        print(line, flush=True)
    if opts.stream:
        say('lockstep: DeviceGenerator.generate() + PlayerReplay.add;  stream: PlayerStreamGenerator.generate(E);  '
            'graphs on, alternating calls, wall clock around a device synchronise')
        for E in opts.games:
            stream_ab(net, dev, E, max(6, opts.reps), say)
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
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
