"""Lockstep against streaming device self-play on one GPU, in one call.

    python tools/stream_rollout_bench.py [--config tictactoe|geister|all] [--seconds 4] [--repeats 3] [--out FILE]
    python tools/stream_rollout_bench.py --profile lockstep|stream --config geister --calls 3
                                     (the program of a separate `rocprofv3 --kernel-trace --stats -- python ...` run:
                                      a fixed number of calls after warm-up, no timing; prints the plies it ran)

Both forms play the same env with the same net (seeded random init, eval mode) at the same slot count E:

  lockstep  ``DeviceGenerator.generate()`` + ``DeviceReplay.add()``: E games per call, every slot waits for the
            longest game of the batch
  stream    ``StreamGenerator.generate(E)``: a finished game is written into the ring by one launch and its slot
            restarts; the call returns once E more games are in the ring

A leg is ``--seconds`` of calls after warm-up (two calls of each form: graph capture, library workspaces), timed by
a host clock around a device synchronise at both ends; the legs alternate lockstep, stream, lockstep, ... for
``--repeats`` rounds.  Reported per leg: env-steps/s (the lengths of the episodes that reached the replay, over the
leg's time) and global steps (plies) per second; per form the median and the spread (min .. max) over the repeats,
and the ratio of the medians.  One JSON line per config.
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {'tictactoe': 4096, 'geister': 2048}   # env: slots E


def build(env, E, dev):
    import torch
    from handyrl_amd.rollout import DeviceGenerator, DeviceReplay, StreamGenerator, TicTacToeBatch
    torch.manual_seed(0)
    from handyrl_amd.nn import accelerate
    if env == 'tictactoe':
        from handyrl_amd.envs.tictactoe import SimpleConv2dModel
        cls, net = TicTacToeBatch, accelerate(SimpleConv2dModel().to(dev))   # the nets of bench.py's rollouts
    else:
        from handyrl_amd.envs.geister import GeisterBatch, GeisterNet
        cls, net = GeisterBatch, accelerate(GeisterNet().to(dev))
    net.eval()

    def replay():
        return DeviceReplay(4 * E, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P, dev, obs_dtype=torch.uint8)
    lock_replay, stream_replay = replay(), replay()
    lock = DeviceGenerator(cls(E, dev), net, gamma=0.8)
    stream = StreamGenerator(cls(E, dev), net, stream_replay, gamma=0.8, seed=1)
    rng = torch.Generator(device=dev).manual_seed(1)

    def lockstep_call():
        ep = lock.generate(generator=rng)
        lock_replay.add(ep)
        return ep['length'].sum(), lock._st['t'].clone()   # device scalars (the call's env-steps and plies), read
                                                           # after the leg's synchronise

    def stream_call():
        out = stream.generate(E)
        return out['env_steps'], out['plies']
    return {'lockstep': lockstep_call, 'stream': stream_call}, cls, lock


def leg(call, seconds, sync):
    sync()
    t0 = time.perf_counter()
    steps, plies = [], []
    while time.perf_counter() - t0 < seconds:
        s, p = call()
        steps.append(s)
        plies.append(p)
    sync()
    dt = time.perf_counter() - t0
    return {'env_steps_per_s': sum(float(s) for s in steps) / dt, 'calls': len(steps), 'seconds': dt,
            'plies_per_s': sum(float(p) for p in plies) / dt}


def measure(env, seconds, repeats):
    import torch
    dev = torch.device('cuda', 0)
    calls, cls, _ = build(env, CONFIGS[env], dev)
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731
    for _ in range(2):
        for c in calls.values():
            c()
    legs = {k: [] for k in calls}
    for _ in range(repeats):
        for k, c in calls.items():
            legs[k].append(leg(c, seconds, sync))
    out = {'config': env, 'E': CONFIGS[env], 'seconds_per_leg': seconds, 'repeats': repeats}
    for k, ls in legs.items():
        rates = [l['env_steps_per_s'] for l in ls]
        out[k] = {'env_steps_per_s_median': statistics.median(rates), 'env_steps_per_s_min': min(rates),
                  'env_steps_per_s_max': max(rates), 'calls': [l['calls'] for l in ls],
                  'plies_per_s': [round(l['plies_per_s'], 1) for l in ls]}
    out['stream_over_lockstep'] = (out['stream']['env_steps_per_s_median']
                                   / out['lockstep']['env_steps_per_s_median'])
    return out


def profile(env, form, n):
    import torch
    dev = torch.device('cuda', 0)
    calls, _, lock = build(env, CONFIGS[env], dev)
    for _ in range(2):
        calls[form]()
    torch.cuda.synchronize(dev)
    steps = plies = 0
    for _ in range(n):
        s, p = calls[form]()
        steps += float(s)
        plies += int(p)
    torch.cuda.synchronize(dev)
    print(json.dumps({'profile': form, 'config': env, 'calls': n, 'env_steps': steps, 'plies': plies}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='all', choices=list(CONFIGS) + ['all'])
    ap.add_argument('--seconds', type=float, default=4.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--profile', choices=['lockstep', 'stream'])
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('stream_rollout_bench measures on the GPU; none is visible')
    configs = list(CONFIGS) if a.config == 'all' else [a.config]
    if a.profile:
        for env in configs:
            profile(env, a.profile, a.calls)
        return
    for env in configs:
        line = json.dumps(measure(env, a.seconds, a.repeats))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
