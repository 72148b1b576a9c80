"""A league of checkpoints on the device against what a user had before it: one match run per pairing.

    python tools/league_bench.py [--config tictactoe|geister|all] [--rounds 3] [--out FILE]
    python tools/league_bench.py --profile league|sequential|k2_league|k2_match --config geister
                  (the program of a separate `rocprofv3 --kernel-trace --stats -- python ...` run: the leg's warm-up
                   call and one more, no timing; prints the plies it ran, warm-up included)
    python tools/league_bench.py --launches KERNEL_TRACE.csv --plies N
                  (kernel launches per ply of such a trace)

Seeded random-init nets in eval mode, one GPU, all legs in one call:

  league      ``LeagueEvaluator(K nets, E slots).evaluate(G)``: Geister K = 4 (Q = 6), E = 2,040, G = 680 per pairing;
              TicTacToe K = 8 (Q = 28), E = 4,088, G = 4,096
  sequential  the same pairings as Q runs, one after another, of the unchanged ``DeviceEvaluator(opponent=)`` with the
              same E, G, opening plies and seed: the yardstick
  seq_cli     the same Q runs with the slot count ``--eval-match`` picks, min(E, G) (it differs for Geister only)
  k2_league   a league of two nets at the same E, G = 2 E
  k2_match    the one ``DeviceEvaluator`` match that league plays

A leg is one call that plays all its games, after one warm-up call (graph capture, library workspaces), timed by a
host clock around a device synchronise at both ends.  The legs alternate for ``--rounds`` rounds; the median and the
spread (min .. max) of the wall time, of games per second and of ms per ply (a global step over all slots; for the
sequential legs the plies of the Q runs added up) are reported, one JSON line per config, with the share of the
league's games whose outcome equals the sequential leg's (tests/test_league_rollout.py holds the exact comparison, on
nets that are exact in any batch size).
"""

import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {'tictactoe': (8, 4088, 4096), 'geister': (4, 2040, 680)}   # env: agents K, slots E, games per pairing G
OPENING, SEED = 2, 1


def build(env, dev, only=None):
    import torch
    from handyrl_amd.evaluation import DeviceEvaluator, LeagueEvaluator
    from handyrl_amd.nn import accelerate
    from handyrl_amd.rollout import TicTacToeBatch
    K, E, G = CONFIGS[env]
    if env == 'tictactoe':
        from handyrl_amd.envs.tictactoe import SimpleConv2dModel as Net
        cls = TicTacToeBatch
    else:
        from handyrl_amd.envs.geister import GeisterBatch as cls, GeisterNet as Net
    nets = []
    for k in range(K):
        torch.manual_seed(k)
        nets.append(accelerate(Net().to(dev)).eval())
    pairs = [(i, j) for i in range(K) for j in range(i + 1, K)]
    legs, made = {}, {}

    def lazily(name, make):
        def call():
            if name not in made:
                made[name] = make()
            return made[name]()
        if only is None or name == only:
            legs[name] = call

    def league(agents, games):
        def make():
            ev = LeagueEvaluator(cls(E, dev), agents, opening_plies=OPENING, seed=SEED)
            q = len(agents) * (len(agents) - 1) // 2

            def run():
                res = ev.evaluate(games)
                return q * games, res['plies'], res['outcome']
            return run
        return make

    def matches(which, slots, games):
        def make():
            evs = [DeviceEvaluator(cls(slots, dev), nets[i], opponent=nets[j], opening_plies=OPENING, seed=SEED)
                   for i, j in which]

            def run():
                res = [ev.evaluate(games) for ev in evs]
                return len(evs) * games, sum(r['plies'] for r in res), torch.stack([r['outcome'] for r in res])
            return run
        return make
    lazily('league', league(nets, G))
    lazily('sequential', matches(pairs, E, G))
    if min(E, G) != E:
        lazily('seq_cli', matches(pairs, min(E, G), G))
    lazily('k2_league', league(nets[:2], 2 * E))
    lazily('k2_match', matches(pairs[:1], E, 2 * E))
    return legs


def measure(env, rounds):
    import torch
    dev = torch.device('cuda', 0)
    legs = build(env, dev)
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731
    first = {k: c() for k, c in legs.items()}    # warm-up; and the results, compared below
    # the accelerated nets are not exact across batch sizes (the league forwards other row counts than a match), so
    # a near-tie may be decided otherwise: the share of games with the same outcome is reported, not asserted
    def share(a, b):
        return float((first[a][2] == first[b][2]).all(-1).float().mean())
    same = {'league_games_as_sequential': share('league', 'sequential'),
            'k2_league_games_as_match': share('k2_league', 'k2_match')}
    runs = {k: [] for k in legs}
    for _ in range(rounds):
        for k, c in legs.items():
            sync()
            t0 = time.perf_counter()
            games, plies, _ = c()
            sync()
            dt = time.perf_counter() - t0
            runs[k].append({'seconds': dt, 'games_per_s': games / dt, 'ms_per_ply': 1e3 * dt / plies, 'plies': plies})
    K, E, G = CONFIGS[env]
    out = {'config': env, 'K': K, 'Q': K * (K - 1) // 2, 'E': E, 'G': G, 'rounds': rounds, **same}
    for k, rs in runs.items():
        out[k] = {'plies': rs[0]['plies']}
        for q in ('seconds', 'games_per_s', 'ms_per_ply'):
            v = [r[q] for r in rs]
            out[k][q] = {'median': statistics.median(v), 'min': min(v), 'max': max(v)}
    out['league_over_sequential_seconds'] = out['league']['seconds']['median'] / out['sequential']['seconds']['median']
    out['k2_league_over_match_seconds'] = out['k2_league']['seconds']['median'] / out['k2_match']['seconds']['median']
    return out


def profile_run(env, leg):
    import torch
    dev = torch.device('cuda', 0)
    call = build(env, dev, only=leg)[leg]
    plies = 0
    for _ in range(2):
        plies += call()[1]
    torch.cuda.synchronize(dev)
    print(json.dumps({'profile': leg, 'config': env, 'calls': 2, 'plies': plies}))


def launches(path, plies):
    """Kernel launches per ply of a rocprofv3 kernel trace, and the kernels that make them up."""
    count, total = {}, {}
    for r in csv.DictReader(open(path)):
        n = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0][:90]
        count[n] = count.get(n, 0) + 1
        total[n] = total.get(n, 0) + int(r['End_Timestamp']) - int(r['Start_Timestamp'])
    print('%.2f launches per ply (%d launches, %d plies), %.3f ms kernel time per ply'
          % (sum(count.values()) / plies, sum(count.values()), plies, sum(total.values()) / 1e6 / plies))
    for n in sorted(total, key=total.get, reverse=True)[:25]:
        print('  %7.2f per ply  %8.2f us each  %6.1f us per ply  %s'
              % (count[n] / plies, total[n] / 1e3 / count[n], total[n] / 1e3 / plies, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='all', choices=list(CONFIGS) + ['all'])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--profile', choices=['league', 'sequential', 'seq_cli', 'k2_league', 'k2_match'])
    ap.add_argument('--launches')
    ap.add_argument('--plies', type=int)
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.launches:
        launches(a.launches, a.plies)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('league_bench measures on the GPU; none is visible')
    for env in (list(CONFIGS) if a.config == 'all' else [a.config]):
        if a.profile:
            profile_run(env, a.profile)
            continue
        line = json.dumps(measure(env, a.rounds))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
