"""GeeseNet's eval forward: the exact tower (nn.GeeseInference) against the bf16 one-launch form (precision='bf16').

    python tools/geese_infer_bf16_bench.py [--out profiles/geese_infer_bf16.txt] [--rows 256 1024 2048 8192] [--reps 7]
                                           [--iters 50] [--slots 2048]

tools/geese_infer_bench.py's method: one process holds both forms, each captured in a graph; within every repetition
the two alternate (device events around ``--iters`` replays); the spread is the minimum and maximum over the
repetitions.  Then ``PlayerEvaluator`` (4 E games per call) and ``PlayerStreamGenerator.generate(E)`` with both
wrappers, wall clock around a device synchronise, ms per global step."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from handyrl_amd.envs.geese import HungryGeeseBatch  # noqa: E402
from handyrl_amd.evaluation import PlayerEvaluator  # noqa: E402
from handyrl_amd.nn import GeeseInference  # noqa: E402
from handyrl_amd.rollout import PlayerReplay, PlayerStreamGenerator  # noqa: E402
from tools.geese_infer_bench import SEED, captured, events_ms, fmt, observations, seeded_net  # noqa: E402

FORMS = (('tower', 'fp32'), ('bf16', 'bf16'))


def forward_ab(dev, rows, reps, iters, say):
    net = seeded_net(dev)
    ws = {name: GeeseInference(net, precision=p) for name, p in FORMS}
    for N in rows:
        x = observations(N, dev)
        with torch.no_grad(), ws['tower'].inference_session(), ws['bf16'].inference_session():
            outs = {k: w(x) for k, w in ws.items()}
            err = {k: float((outs['tower'][k] - outs['bf16'][k]).abs().max()) for k in ('policy', 'value')}
            graphs = {k: captured(lambda w=w: w(x), dev) for k, w in ws.items()}
            for f in graphs.values():
                events_ms(f, 3)
            runs = {k: [] for k in graphs}
            for _ in range(reps):
                for k, f in graphs.items():
                    runs[k].append(events_ms(f, iters))
        for k in runs:
            say('forward N=%-5d graph  %-6s ms per forward %s' % (N, k, fmt(runs[k])))
        t, b = statistics.median(runs['tower']), statistics.median(runs['bf16'])
        spread = max(max(r) - min(r) for r in runs.values())
        say('forward N=%-5d tower - bf16 medians %.4f ms (tower / bf16 %.2f), the larger spread %.4f ms: %s; '
            '|tower - bf16| policy %.3e value %.3e'
            % (N, t - b, t / b, spread, 'bf16 wins' if t - b > spread else 'NO WIN', err['policy'], err['value']))


def players_ab(dev, slots, reps, say):
    net = seeded_net(dev)
    for E in slots:
        steps = {}
        for name, p in FORMS:
            b = HungryGeeseBatch(E, dev)
            b.seed(SEED)
            ev = PlayerEvaluator(b, GeeseInference(net, precision=p), seed=SEED)
            env = HungryGeeseBatch(E, dev, seed=SEED)
            replay = PlayerReplay(E, env.MAX_PLIES, env.OBS_SHAPE, 4, 4, dev, obs_dtype=torch.uint8, solo=True)
            gen = PlayerStreamGenerator(env, GeeseInference(net, precision=p), replay, seed=SEED)
            steps['evaluator ' + name] = lambda ev=ev: ev.evaluate(4 * E)['plies']
            steps['stream    ' + name] = lambda gen=gen: gen.generate(E)['plies']
        for f in steps.values():
            f()                                                   # capture and warm-up
        runs = {k: [] for k in steps}
        for _ in range(reps):
            for k, f in steps.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                plies = f()
                torch.cuda.synchronize(dev)
                runs[k].append((time.perf_counter() - t0) * 1e3 / plies)
        for k in runs:
            say('%s E=%-5d ms per global step %s' % (k, E, fmt(runs[k])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'geese_infer_bf16.txt'))
    ap.add_argument('--rows', type=int, nargs='+', default=[256, 1024, 2048, 8192])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--slots', type=int, nargs='*', default=[2048])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('geese_infer_bf16_bench measures on the GPU; no GPU is visible')
    dev = torch.device('cuda', 0)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('GeeseNet eval forward, %s, seeded-init GeeseNet (12 blocks), board 7x11; tower = nn.GeeseInference (exact), '
        'bf16 = nn.GeeseInference(precision=\'bf16\'), one launch' % torch.cuda.get_device_name(dev))
    forward_ab(dev, args.rows, max(3, args.reps), args.iters, say)
    players_ab(dev, args.slots, max(3, args.reps), say)
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
