"""GeisterNet's eval forward two ways on one GPU, in one process, alternating: the module path (the ``accelerate``d
net in its inference session, about 14 launches) and nn.GeisterInference (hrl_geister_infer, one launch).

Per batch size each form's ply (forward + in-place state advance on a live random state) is captured as a HIP graph;
a repetition replays A then B ``--iters`` times each under events, and the table gives the median and the spread
(min .. max) over ``--reps`` repetitions.  Then the lockstep self-play generation (rollout.DeviceGenerator on
GeisterBatch, E games from the first ply to the last) both ways, alternating, wall time per generation.

    python tools/geister_infer_bench.py [--sizes 256 2048 4096] [--games 2048] [--out profiles/geister_infer.txt]
"""

import argparse
import copy
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from handyrl_amd import nn as hnn                                    # noqa: E402
from handyrl_amd.envs.geister import GeisterBatch, GeisterNet        # noqa: E402
from handyrl_amd.rollout import DeviceGenerator                      # noqa: E402


def captured_ply(model, N, dev, seed):
    """(graph, keepalive) of one forward on N rows advancing its own stacked state in place; the model's in-place
    session must be open."""
    g = torch.Generator().manual_seed(seed)
    obs = {'board': (torch.rand(N, 7, 6, 6, generator=g) < 0.2).float().to(dev),
           'scalar': torch.rand(N, 18, generator=g).to(dev)}
    hidden = model.inference_hidden(N, 1, dev)
    for kind in hidden:
        for leaf in kind:
            leaf.copy_(torch.randn(leaf.shape, generator=g))
    state = tuple([leaf[0] for leaf in kind] for kind in hidden)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        for _ in range(3):
            model(obs, state)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model(obs, state)
    return graph, (obs, hidden, out)


def timed(graph, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3   # us per ply


def row(name, xs, unit):
    return '%-34s median %9.1f %s   min %9.1f   max %9.1f' % (name, statistics.median(xs), unit, min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[256, 2048, 4096])
    ap.add_argument('--games', type=int, default=2048)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--generations', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    torch.manual_seed(1)
    net = hnn.accelerate(GeisterNet().to(dev)).eval()
    wrapper = hnn.GeisterInference(net)
    lines = ['%s, torch %s' % (torch.cuda.get_device_name(dev), torch.__version__),
             'GeisterNet eval forward, us per ply: captured graphs, A/B alternating, %d replays x %d repetitions'
             % (args.iters, args.reps)]
    with torch.no_grad():
        for N in args.sizes:
            with net.inference_session(inplace_state=True), wrapper.inference_session(inplace_state=True):
                ga, keep_a = captured_ply(net, N, dev, seed=N)
                gb, keep_b = captured_ply(wrapper, N, dev, seed=N)
                for g in (ga, gb):
                    timed(g, 10)
                ta, tb = [], []
                for _ in range(args.reps):
                    ta.append(timed(ga, args.iters))
                    tb.append(timed(gb, args.iters))
            lines.append(row('N = %5d  module path' % N, ta, 'us'))
            lines.append(row('N = %5d  hrl_geister_infer' % N, tb, 'us'))
        if args.games:
            lines.append('lockstep self-play, E = %d games, ms per generation (first ply to last), alternating'
                         % args.games)
            gens = {'module path': DeviceGenerator(GeisterBatch(args.games, dev), net, gamma=0.8),
                    'GeisterInference': DeviceGenerator(GeisterBatch(args.games, dev), wrapper, gamma=0.8)}
            times = {k: [] for k in gens}
            for rep in range(args.generations + 1):
                for k, gen in gens.items():
                    rng = torch.Generator(device=dev).manual_seed(3)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    gen.generate(generator=rng)
                    torch.cuda.synchronize()
                    if rep:   # the first generation captures its graphs
                        times[k].append((time.perf_counter() - t0) * 1e3)
            for k, xs in times.items():
                lines.append(row(k, xs, 'ms'))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
