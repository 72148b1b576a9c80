"""Whole TicTacToe self-play games in one launch (``DeviceGenerator(fused_game=True)``) against the lockstep ply loop.

    python tools/board_selfplay_bench.py --part generator|launch|all [--seconds 3] [--repeats 3] [--out FILE]

The protocol of tools/board_infer_bench.py: run each part as a process of its own; both forms are built from the same
seeded net (``accelerate``d, eval mode, wrapped in ``nn.BoardInference``), warmed up, and their legs alternate in one
call; per form the median and the spread (min .. max) over ``--repeats`` legs, one JSON line per measurement.  The
yardstick is the lockstep generator of the same call (``fused_game=False``: the ply loop and its captured graphs,
untouched by the option), never the new code against itself.

  generator  ``DeviceGenerator`` at E = 4096 and 16384 without and with ``fused_game``: env-steps/s, ms per
             ``generate()`` call, and the kernels of one call (torch.profiler, outside the timed legs; the reset, the
             session's pack launch and the clones are counted in).
  launch     ``hrl_board_selfplay`` alone (nine plies, fresh games, the call's own buffers) between two device events
             around every single launch; the env's reset is outside the pair.  us per launch over 50 launches a leg.
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.board_infer_bench import _kernels, _net, _stats   # noqa: E402


def _generator(dev, E, fused):
    import torch
    from handyrl_amd.nn import BoardInference
    from handyrl_amd.rollout import DeviceGenerator, TicTacToeBatch
    gen = DeviceGenerator(TicTacToeBatch(E, dev), BoardInference(_net(dev)), gamma=0.8, fused_game=fused)
    rng = torch.Generator(device=dev).manual_seed(1)
    return gen, (lambda: gen.generate(generator=rng)['length'].sum())


def generator(dev, seconds, repeats, emit):
    import torch
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731
    for E in (4096, 16384):
        calls = {'lockstep': _generator(dev, E, False)[1], 'fused_game': _generator(dev, E, True)[1]}
        for _ in range(3):
            for c in calls.values():
                c()
        sync()
        launches = {name: _kernels(c, dev) for name, c in calls.items()}
        legs = {k: [] for k in calls}
        for _ in range(repeats):
            for name, c in calls.items():
                sync()
                t0 = time.perf_counter()
                steps = []
                while time.perf_counter() - t0 < seconds:
                    steps.append(c())
                sync()
                dt = time.perf_counter() - t0
                legs[name].append({'env_steps_per_s': sum(float(s) for s in steps) / dt,
                                   'ms_per_call': 1e3 * dt / len(steps)})
        out = {'part': 'generator', 'E': E, 'seconds_per_leg': seconds, 'repeats': repeats}
        for name, ls in legs.items():
            out[name] = {'env_steps_per_s': _stats([l['env_steps_per_s'] for l in ls]),
                         'ms_per_call': _stats([l['ms_per_call'] for l in ls]), 'launches_per_call': launches[name]}
        out['fused_over_lockstep_env_steps'] = (out['fused_game']['env_steps_per_s']['median']
                                                / out['lockstep']['env_steps_per_s']['median'])
        emit(out)


def launch(dev, repeats, emit):
    import torch
    from handyrl_amd import _native
    per_leg = 50
    for E in (4096, 16384):
        gen, call = _generator(dev, E, True)
        call()
        st, env, net = gen._st, gen.env, gen.net
        Tm = env.MAX_PLIES
        legs = []
        with torch.no_grad(), net.inference_session():
            for _ in range(repeats + 1):                    # the first leg warms up
                us = []
                for _ in range(per_leg):
                    env.reset()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _native.check(_native.load().hrl_board_selfplay(
                        _native.ptr(net.pack(dev)), net.layers, E, Tm, 0, Tm, _native.ptr(st['U']),
                        _native.ptr(env.board), _native.ptr(env.color), _native.ptr(env.nmoves),
                        _native.ptr(env.winner), _native.ptr(st['obs']), _native.ptr(st['policy']),
                        _native.ptr(st['amask']), _native.ptr(st['action']), _native.ptr(st['value']),
                        _native.ptr(st['turn']), _native.stream_of(dev)), 'hrl_board_selfplay')
                    e1.record()
                    e1.synchronize()
                    us.append(1e3 * e0.elapsed_time(e1))
                legs.append(statistics.median(us))
        steps = float(env.plies().sum())
        emit({'part': 'launch', 'E': E, 'launches_per_leg': per_leg, 'repeats': repeats, 'env_steps_per_launch': steps,
              'us_per_launch': _stats(legs[1:]), 'us_per_ply': statistics.median(legs[1:]) / Tm})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['generator', 'launch', 'all'])
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('board_selfplay_bench measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    if a.part in ('generator', 'all'):
        generator(dev, a.seconds, a.repeats, emit)
    if a.part in ('launch', 'all'):
        launch(dev, a.repeats, emit)


if __name__ == '__main__':
    main()
