"""The device evaluator against the parent's code of the same env on one GPU, in one call.

    python tools/eval_bench.py [--config tictactoe|geister|all] [--seconds 3] [--repeats 3] [--out FILE]
    python tools/eval_bench.py --profile --config geister --calls 2
                  (the program of a separate `rocprofv3 --kernel-trace --stats -- python ...` run: a fixed number of
                   evaluate() calls after warm-up, no timing; prints the plies it ran)
    python tools/eval_bench.py --match [--config ...] [--seconds 3] [--repeats 3] [--out FILE]
                  (a match of the net against a copy of itself with two opening plies, the unchanged evaluator against
                   random agents and one eval-mode forward of the net at E rows, alternating in one call; --profile
                   --match is the match's kernel-trace program)
    python tools/eval_bench.py --reference PATH [--games 20]
                  (context, on the CPU: the rate of the reference's one-process exec_match, greedy Agent against
                   RandomAgent, from the HandyRL tree at PATH)

  eval      ``DeviceEvaluator(E slots).evaluate(G)``: TicTacToe E = 4096, G = 16384; Geister E = 2048, G = 4096
  match     ``DeviceEvaluator(E slots, opponent=copy of the net, opening_plies=2).evaluate(G)``, same E and G; its
            yardstick is the ``eval`` ply plus one ``forward`` (the match adds the opponent's forward and, for a
            recurrent net, one state advance); ``forward`` reports ms per forward as its ms per ply
  baseline  TicTacToe: ``loop.evaluate_vs_random(games=4096)`` (the lockstep torch loop, nine plies per call);
            Geister: the lockstep ``DeviceGenerator.generate()`` ply at E = 2048, which runs the same forward

The net is the env's seeded random init in eval mode.  A leg is ``--seconds`` of calls after warm-up (two calls:
graph capture, library workspaces), timed by a host clock around a device synchronise at both ends; the legs
alternate eval, baseline, ... for ``--repeats`` rounds; the median and the spread (min .. max) are reported:
games/s and ms per ply (a global step over all slots).  One JSON line per config.  Kernel launches per ply come from
the ``--profile`` run's kernel trace: every kernel's call count over the plies of all its calls (warm-up included).
"""

import argparse
import contextlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {'tictactoe': (4096, 16384), 'geister': (2048, 4096)}   # env: slots E, games G


def build(env, dev, match=False):
    import copy
    import torch
    from handyrl_amd.evaluation import DeviceEvaluator
    from handyrl_amd.nn import accelerate
    from handyrl_amd.rollout import DeviceGenerator, TicTacToeBatch
    E, G = CONFIGS[env]
    torch.manual_seed(0)
    if env == 'tictactoe':
        from handyrl_amd.envs.tictactoe import SimpleConv2dModel
        from handyrl_amd.loop import evaluate_vs_random
        cls, net = TicTacToeBatch, accelerate(SimpleConv2dModel().to(dev))

        def baseline():
            evaluate_vs_random(net, dev, games=4096)
            return 4096, TicTacToeBatch.MAX_PLIES
    else:
        from handyrl_amd.envs.geister import GeisterBatch, GeisterNet
        cls, net = GeisterBatch, accelerate(GeisterNet().to(dev))
        lock = DeviceGenerator(cls(E, dev), net, gamma=0.8)
        rng = torch.Generator(device=dev).manual_seed(1)

        def baseline():
            lock.generate(generator=rng)
            return E, lock._st['t'].clone()      # a device scalar, read after the leg's synchronise
    net.eval()
    ev = DeviceEvaluator(cls(E, dev), net, seed=1)

    def evaluate():
        res = ev.evaluate(G)
        return G, res['plies']
    if not match:
        return {'eval': evaluate, 'baseline': baseline}, cls, net
    mv = DeviceEvaluator(cls(E, dev), net, seed=1, opponent=copy.deepcopy(net), opening_plies=2)

    def play_match():
        res = mv.evaluate(G)
        return G, res['plies']
    board = cls(E, dev)
    board.reset()
    obs = board.observation(torch.arange(E, device=dev) % cls.P)
    hidden = None
    if hasattr(net, 'inference_hidden'):
        hidden = tuple([x[0] for x in leaf] for leaf in net.inference_hidden(E, 1, dev))
    elif hasattr(net, 'init_hidden'):
        hidden = net.init_hidden([E])

    def forward(n=64):
        with torch.no_grad(), net.inference_session() if hasattr(net, 'inference_session') \
                else contextlib.nullcontext():
            for _ in range(n):
                net(obs, hidden)
        return 0, n
    return {'match': play_match, 'eval': evaluate, 'forward': forward}, cls, net


def leg(call, seconds, sync):
    sync()
    t0 = time.perf_counter()
    games, plies = [], []
    while time.perf_counter() - t0 < seconds:
        g, p = call()
        games.append(g)
        plies.append(p)
    sync()
    dt = time.perf_counter() - t0
    plies = sum(float(p) for p in plies)
    return {'games_per_s': sum(games) / dt, 'ms_per_ply': 1e3 * dt / plies, 'calls': len(games), 'seconds': dt}


def measure(env, seconds, repeats, match=False):
    import torch
    dev = torch.device('cuda', 0)
    calls, cls, net = build(env, dev, match)
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731
    for _ in range(2):
        for c in calls.values():
            c()
    legs = {k: [] for k in calls}
    for _ in range(repeats):
        for k, c in calls.items():
            legs[k].append(leg(c, seconds, sync))
    E, G = CONFIGS[env]
    out = {'config': env, 'E': E, 'G': G, 'seconds_per_leg': seconds, 'repeats': repeats}
    for k, ls in legs.items():
        out[k] = {}
        for q in ('games_per_s', 'ms_per_ply'):
            v = [l[q] for l in ls]
            out[k][q] = {'median': statistics.median(v), 'min': min(v), 'max': max(v)}
        out[k]['calls'] = [l['calls'] for l in ls]
    if match:
        yard = out['eval']['ms_per_ply']['median'] + out['forward']['ms_per_ply']['median']
        out['yardstick_ms_per_ply'] = yard
        out['ply_match_over_yardstick'] = out['match']['ms_per_ply']['median'] / yard
    else:
        out['ply_eval_over_baseline'] = out['eval']['ms_per_ply']['median'] / out['baseline']['ms_per_ply']['median']
    return out


def profile_run(env, n, match=False):
    import torch
    dev = torch.device('cuda', 0)
    calls, _, _ = build(env, dev, match)
    which = 'match' if match else 'eval'
    for _ in range(2):
        calls[which]()
    torch.cuda.synchronize(dev)
    plies = 0
    for _ in range(n):
        plies += calls[which]()[1]
    torch.cuda.synchronize(dev)
    print(json.dumps({'profile': which, 'config': env, 'calls': n, 'plies': plies}))


def reference(path, games):
    """The reference's exec_match, greedy Agent against RandomAgent, one process on the CPU."""
    import random
    sys.path.insert(0, path)
    import torch
    from handyrl.agent import Agent, RandomAgent
    from handyrl.environment import make_env
    from handyrl.evaluation import exec_match
    from handyrl.model import ModelWrapper
    for name in ('TicTacToe', 'Geister'):
        env = make_env({'env': name})
        torch.manual_seed(0)
        net = env.net()()
        net.eval()
        model = ModelWrapper(net)
        random.seed(0)
        t0 = time.perf_counter()
        for g in range(games):
            exec_match(env, {g % 2: Agent(model), 1 - g % 2: RandomAgent()}, None)
        dt = time.perf_counter() - t0
        print(json.dumps({'reference_exec_match': name, 'games': games, 'games_per_s': games / dt}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='all', choices=list(CONFIGS) + ['all'])
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--match', action='store_true')
    ap.add_argument('--calls', type=int, default=2)
    ap.add_argument('--reference')
    ap.add_argument('--games', type=int, default=20)
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.reference:
        reference(a.reference, a.games)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('eval_bench measures on the GPU; none is visible')
    configs = list(CONFIGS) if a.config == 'all' else [a.config]
    for env in configs:
        if a.profile:
            profile_run(env, a.calls, a.match)
            continue
        line = json.dumps(measure(env, a.seconds, a.repeats, a.match))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
