"""What batch assembly costs the training loop: replay.sample and sample -> learner.step on one GPU.

    python tools/replay_gather_bench.py --config ttt9                one tree (this one), one JSON line
    python tools/replay_gather_bench.py --compare PARENT_TREE        parent, this tree, parent again, per config,
                                                                     each run a fresh process; prints the table of
                                                                     profiles/replay_gather.txt

The replay is filled by the device generator, the loop is ``loop.SelfPlayTrainer.train_steps`` as the tree under
test has it (graph=True), so the same script measures a tree without the fused gather.  Per configuration:

  (a) us per ``replay.sample`` call, as ``train_steps`` issues it (``out=`` where the tree has ``alloc_batch``)
  (b) ms per loop iteration sample -> learner.step
  (c) (b) minus the step alone (the graph replay on the static batch)

Each is the median of ``--calls`` calls (default 300) after ``--warmup`` calls, wall clock with a device
synchronisation at both ends of every call.  ``b_pipe`` / ``c_pipe`` are the same from blocks of 20 iterations
with one synchronisation per block (the loop as it runs, host and device overlapped).
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {   # name: (env, B, T, games per round, rounds)
    'ttt9': ('tictactoe', 4096, 9, 4096, 4),
    'ttt32': ('tictactoe', 4096, 32, 4096, 4),
    'geister16': ('geister', 256, 16, 256, 2),
}


def _median_ms(fn, calls, warmup, sync, block=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(calls):
        sync()
        t0 = time.perf_counter()
        for _ in range(block):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / block)
    return statistics.median(out)


def measure(tree, config, calls, warmup, draw):
    sys.path.insert(0, tree)
    import torch
    from handyrl_amd.loop import SelfPlayTrainer
    from handyrl_amd.synthetic import default_args
    env, B, T, games, rounds = CONFIGS[config]
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    if env == 'tictactoe':
        from handyrl_amd.envs.tictactoe import SimpleConv2dModel as Net
        from handyrl_amd.rollout import TicTacToeBatch as env_cls
    else:
        from handyrl_amd.envs.geister import GeisterNet as Net, GeisterBatch as env_cls
    args = default_args(T, B)
    tr = SelfPlayTrainer(Net().to(dev), args, dev, games_per_round=games, capacity=games * rounds, graph=True,
                         env_cls=env_cls)
    if draw != 'multinomial':
        tr.replay.draw = draw
    for _ in range(rounds):
        tr.generate()
    sync = lambda: torch.cuda.synchronize(dev)
    tr.train_steps(3)    # capture
    fused = hasattr(tr.replay, 'alloc_batch')
    batch = getattr(tr, '_batch', None)

    def sample():
        if fused:
            tr.replay.sample(B, T, generator=tr.rng, out=batch)
        else:
            tr.replay.sample(B, T, generator=tr.rng)

    static = tr.learner._static
    res = {'config': config, 'tree': os.path.basename(os.path.abspath(tree)), 'fused': fused, 'draw': draw,
           'B': B, 'T': T, 'episodes': int(tr.replay.count)}
    res['a_us'] = 1e3 * _median_ms(sample, calls, warmup, sync)
    res['b_ms'] = _median_ms(lambda: tr.train_steps(1), calls, warmup, sync)
    res['step_ms'] = _median_ms(lambda: tr.learner.step(static, tr.hidden), calls, warmup, sync)
    res['c_ms'] = res['b_ms'] - res['step_ms']
    blocks = max(10, calls // 20)
    res['b_pipe_ms'] = _median_ms(lambda: tr.train_steps(1), blocks, 2, sync, block=20)
    res['step_pipe_ms'] = _median_ms(lambda: tr.learner.step(static, tr.hidden), blocks, 2, sync, block=20)
    res['c_pipe_ms'] = res['b_pipe_ms'] - res['step_pipe_ms']
    return res


def compare(parent, opts):
    rows = []
    for config in opts.configs.split(','):
        for tree in (parent, ROOT, parent):
            cmd = [sys.executable, os.path.abspath(__file__), '--tree', tree, '--config', config, '--calls',
                   str(opts.calls), '--warmup', str(opts.warmup)]
            if tree == ROOT:
                cmd += ['--draw', opts.draw]
            env = dict(os.environ, PYTHONPATH='')
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=opts.timeout, env=env)
            if res.returncode != 0:
                sys.stderr.write(res.stdout + res.stderr)
                raise SystemExit('run failed (%d): %s' % (res.returncode, ' '.join(cmd)))
            row = json.loads(res.stdout.strip().splitlines()[-1])
            row['role'] = 'this tree' if tree == ROOT else 'parent'
            rows.append(row)
            print(json.dumps(row), flush=True)
    print()
    head = ('config', 'run', 'a us/sample', 'b ms/iter', 'step ms', 'c ms', 'b pipelined', 'c pipelined')
    print('%-10s %-10s %12s %10s %9s %8s %12s %12s' % head)
    for r in rows:
        print('%-10s %-10s %12.1f %10.3f %9.3f %8.3f %12.3f %12.3f' % (
            r['config'], r['role'], r['a_us'], r['b_ms'], r['step_ms'], r['c_ms'], r['b_pipe_ms'], r['c_pipe_ms']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=ROOT, help='repository root whose handyrl_amd is measured')
    ap.add_argument('--config', default='ttt9', choices=sorted(CONFIGS))
    ap.add_argument('--configs', default='ttt9,ttt32,geister16')
    ap.add_argument('--compare', metavar='PARENT_TREE', help='a built checkout of the parent commit')
    ap.add_argument('--calls', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--draw', default='multinomial', choices=('multinomial', 'inverse'))
    ap.add_argument('--timeout', type=int, default=400)
    opts = ap.parse_args()
    if opts.compare:
        compare(os.path.abspath(opts.compare), opts)
    else:
        print(json.dumps(measure(os.path.abspath(opts.tree), opts.config, opts.calls, opts.warmup, opts.draw)))


if __name__ == '__main__':
    main()
