"""GeeseNet's eval forward: the module-by-module path against nn.GeeseInference (csrc/hrl_geesenet.hip).

    python tools/geese_infer_bench.py [--out profiles/geese_infer.txt] [--rows 256 1024 1536 2048 8192] [--reps 7]
                                      [--iters 50] [--slots 256 2048] [--stream-slots 2048] [--no-trace]

On one GPU with a seeded-init GeeseNet, everything in one process, the forms ALTERNATING within every repetition:
  forward   per batch size: the accelerated net's own eval forward (``net(x)``) and the wrapper inside a session
            (``w(x)``), eager (device events around ``--iters`` back-to-back forwards) and as a captured graph (events
            around ``--iters`` replays: what the generators and evaluators run); the wrapper also with each launch
            shape forced (hrl_geesenet_infer_set_form 1 / 2).  Outputs are compared first (1e-5).  The spread is the
            minimum and maximum over ``--reps`` repetitions of the same code.
  players   ``PlayerEvaluator`` (G = 4 E games per call) per slot count and ``PlayerStreamGenerator.generate(E)``, with
            the plain net and with the wrapper: wall clock around a device synchronise, ms per global step.
  launches  kernel launches per forward of both forms from ``rocprofv3 --kernel-trace --stats`` runs of this file's
            ``--trace-child K`` program (a fresh process each; K and 2 K forwards of both forms, the difference of
            the call counts over K; nothing else is collected in those runs).
"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from handyrl_amd import _native  # noqa: E402
from handyrl_amd.envs.geese import GeeseNet, HungryGeeseBatch  # noqa: E402
from handyrl_amd.evaluation import PlayerEvaluator  # noqa: E402
from handyrl_amd.nn import GeeseInference, accelerate  # noqa: E402
from handyrl_amd.rollout import PlayerReplay, PlayerStreamGenerator  # noqa: E402

SEED = 1
UNIT = 'geese_unit_kernel'


def seeded_net(dev, seed=7):
    torch.manual_seed(seed)
    return accelerate(GeeseNet().to(dev)).eval()


def observations(N, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, 17, 7, 11, generator=g) < 0.1).float()
    return x.to(dev)


def fmt(xs, unit='ms'):
    return '%.4f-%.4f, median %.4f %s' % (min(xs), max(xs), statistics.median(xs), unit)


def events_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def captured(fn, dev):
    """``fn`` captured in a graph after a warm-up on a side stream; returns the replay callable (and keeps the graph)."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def forward_ab(dev, rows, reps, iters, say):
    lib = _native.load()
    net = seeded_net(dev)
    w = GeeseInference(net)
    for N in rows:
        x = observations(N, dev)
        with torch.no_grad(), w.inference_session():
            ref, got = net(x), w(x)
            for k in ('policy', 'value'):
                err = float((ref[k] - got[k]).abs().max())
                assert err <= 1e-5, (k, err)
            forms = {'module': lambda: net(x), 'wrapper': lambda: w(x)}
            graphs = {k: captured(f, dev) for k, f in forms.items()}
            for form in (1, 2):                                   # the launch shape is fixed at capture
                prev = lib.hrl_geesenet_infer_set_form(form)
                graphs['wrapper, %d-wave shape' % (8 if form == 1 else 2)] = captured(forms['wrapper'], dev)
                lib.hrl_geesenet_infer_set_form(prev)
            for f in list(forms.values()) + list(graphs.values()):   # warm every timed callable
                events_ms(f, 3)
            eager = {k: [] for k in forms}
            graph = {k: [] for k in graphs}
            for _ in range(reps):
                for k, f in forms.items():
                    eager[k].append(events_ms(f, iters))
                for k, f in graphs.items():
                    graph[k].append(events_ms(f, iters))
        for k in forms:
            say('forward N=%-5d eager  %-28s ms per forward %s' % (N, k, fmt(eager[k])))
        for k in graphs:
            say('forward N=%-5d graph  %-28s ms per forward %s' % (N, k, fmt(graph[k])))
        m, g = statistics.median(graph['module']), statistics.median(graph['wrapper'])
        say('forward N=%-5d graph  module / wrapper, medians of %d alternating repetitions of %d forwards: %.2f  '
            '(the slowest wrapper repetition %.4f ms against the fastest module repetition %.4f ms)'
            % (N, reps, iters, m / g, max(graph['wrapper']), min(graph['module'])))


def players_ab(dev, slots, stream_slots, reps, say):
    net = seeded_net(dev)
    for E in slots:
        G = 4 * E
        evs = {}
        for name, n in (('module', net), ('wrapper', GeeseInference(net))):
            b = HungryGeeseBatch(E, dev)
            b.seed(SEED)
            evs[name] = PlayerEvaluator(b, n, seed=SEED)
        first = {k: ev.evaluate(G) for k, ev in evs.items()}          # capture and warm-up
        agree = bool(torch.equal(first['module']['outcome'], first['wrapper']['outcome']))
        runs = {k: [] for k in evs}
        for _ in range(reps):
            for k, ev in evs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                res = ev.evaluate(G)
                torch.cuda.synchronize(dev)
                runs[k].append((time.perf_counter() - t0) * 1e3 / res['plies'])
        for k in evs:
            say('evaluator E=%-5d %-8s G=%d games per call, ms per global step %s' % (E, k, G, fmt(runs[k])))
        say('evaluator E=%-5d module / wrapper, medians: %.2f; the same outcomes in the first call: %s'
            % (E, statistics.median(runs['module']) / statistics.median(runs['wrapper']), agree))
        del evs
    for E in stream_slots:
        gens = {}
        for name, n in (('module', net), ('wrapper', GeeseInference(net))):
            env = HungryGeeseBatch(E, dev, seed=SEED)
            replay = PlayerReplay(E, env.MAX_PLIES, env.OBS_SHAPE, 4, 4, dev, obs_dtype=torch.uint8, solo=True)
            gens[name] = PlayerStreamGenerator(env, n, replay, seed=SEED)
            gens[name].generate(E)                                    # capture and warm-up
        runs = {k: [] for k in gens}
        for _ in range(reps):
            for k, gen in gens.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                out = gen.generate(E)
                torch.cuda.synchronize(dev)
                runs[k].append((time.perf_counter() - t0) * 1e3 / out['plies'])
        for k in gens:
            say('stream    E=%-5d %-8s generate(E), ms per global step %s' % (E, k, fmt(runs[k])))
        say('stream    E=%-5d module / wrapper, medians: %.2f'
            % (E, statistics.median(runs['module']) / statistics.median(runs['wrapper'])))
        del gens


def trace_child(K, N):
    """The program of a kernel-trace run: K eager forwards of each form at N rows (one session)."""
    dev = torch.device('cuda', 0)
    net = seeded_net(dev)
    w = GeeseInference(net)
    x = observations(N, dev)
    with torch.no_grad(), w.inference_session():
        for _ in range(K):
            net(x)
            w(x)
    torch.cuda.synchronize(dev)


def traced_calls(K, N):
    """{kernel name: calls} of a ``rocprofv3 --kernel-trace --stats`` run of ``--trace-child K``."""
    prof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    out = tempfile.mkdtemp(prefix='geese_infer_trace_')
    try:
        cmd = [prof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'run', '--', sys.executable,
               os.path.abspath(__file__), '--trace-child', str(K), '--trace-rows', str(N)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        if res.returncode != 0:
            raise RuntimeError('rocprofv3 failed (%d):\n%s' % (res.returncode, res.stderr[-2000:]))
        files = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
        if not files:
            raise RuntimeError('rocprofv3 wrote no kernel_stats.csv under %s' % out)
        calls = {}
        for path in files:
            with open(path, newline='') as f:
                for row in csv.DictReader(f):
                    calls[row['Name']] = calls.get(row['Name'], 0) + int(row['Calls'])
        return calls
    finally:
        shutil.rmtree(out, ignore_errors=True)


def launches(N, say, K=8):
    one, two = traced_calls(K, N), traced_calls(2 * K, N)
    per = {n: (two.get(n, 0) - one.get(n, 0)) / K for n in two}
    wrapper = sum(v for n, v in per.items() if UNIT in n)
    module = {n: v for n, v in per.items() if UNIT not in n and v}
    say('launches  N=%-5d per forward, rocprofv3 --kernel-trace --stats, calls(%d forwards) - calls(%d) over %d: '
        'wrapper %g (%s only; the pack launch once per session), module path %g'
        % (N, 2 * K, K, K, wrapper, UNIT, sum(module.values())))
    for n, v in sorted(module.items(), key=lambda kv: -kv[1]):
        say('launches            module path %5g x %s' % (v, n[:100]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'geese_infer.txt'))
    ap.add_argument('--rows', type=int, nargs='+', default=[256, 1024, 1536, 2048, 8192])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--slots', type=int, nargs='*', default=[256, 2048])
    ap.add_argument('--stream-slots', type=int, nargs='*', default=[2048])
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-child', type=int, default=0)
    ap.add_argument('--trace-rows', type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('geese_infer_bench measures on the GPU; no GPU is visible')
    if args.trace_child:
        return trace_child(args.trace_child, args.trace_rows)
    dev = torch.device('cuda', 0)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('GeeseNet eval forward, %s, seeded-init GeeseNet (12 blocks), board 7x11; module = the accelerated net\'s own '
        'forward, wrapper = nn.GeeseInference' % torch.cuda.get_device_name(dev))
    if not args.no_trace:
        launches(args.trace_rows, say)                # before this process opens the device's queues for timing
    forward_ab(dev, args.rows, max(3, args.reps), args.iters, say)
    players_ab(dev, args.slots, args.stream_slots, max(3, args.reps), say)
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
