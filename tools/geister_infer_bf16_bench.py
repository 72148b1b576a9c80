"""GeisterNet's eval forward three ways on one GPU, in one process, alternating: the module path (the ``accelerate``d
net in its inference session), nn.GeisterInference (hrl_geister_infer, exact) and nn.GeisterInference(precision=
'bf16') (hrl_geister_infer_bf16).  tools/geister_infer_bench.py's method with a third arm:

* the forward: per batch size each form's ply (forward + in-place state advance) captured as a HIP graph, the forms
  alternating within each of ``--reps`` repetitions of ``--iters`` replays under device events; median, min, max;
* one lockstep self-play generation (rollout.DeviceGenerator, E games from the first ply to the last), wall time;
* the streaming ply (rollout.StreamGenerator, E slots), wall time of a generate(E) call over its global steps;
* the drift: one 200-ply run of 256 games whose moves the exact form samples; the bf16 form sees the same
  observations and carries its own state: max |h - h_exact|, max |c - c_exact| over the mover's state and the largest
  total-variation distance between the two move policies (softmax over the legal actions), at plies 1, 10, 50, 100, 200.

    python tools/geister_infer_bf16_bench.py [--sizes 256 2048 4096] [--games 2048] [--out profiles/geister_infer_bf16.txt]
"""

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geister_infer_bench import captured_ply, row, timed             # noqa: E402
from handyrl_amd import nn as hnn                                    # noqa: E402
from handyrl_amd.envs.geister import GeisterBatch, GeisterNet        # noqa: E402
from handyrl_amd.rollout import DeviceGenerator, DeviceReplay, StreamGenerator   # noqa: E402


def drift(exact, bf16, dev, E=256, plies=200, marks=(1, 10, 50, 100, 200)):
    env = GeisterBatch(E, dev)
    rng = torch.Generator(device=dev).manual_seed(11)
    st_a, st_b = exact.inference_hidden(E, 2, dev), bf16.inference_hidden(E, 2, dev)
    lines = []
    with exact.inference_session(inplace_state=True), bf16.inference_session(inplace_state=True):
        for t in range(1, plies + 1):
            live = env.active().clone()
            if not bool(live.any()):
                break
            p = (t - 1) % 2
            obs, legal = env.observation(env.turn()), env.legal()
            a = exact(obs, tuple([leaf[p] for leaf in kind] for kind in st_a))
            b = bf16(obs, tuple([leaf[p] for leaf in kind] for kind in st_b))
            pa, pb = (torch.softmax(o['policy'].masked_fill(~legal, -1e30), -1) for o in (a, b))
            if t in marks:
                dh, dc = (max(float((x[p] - y[p])[live].abs().max()) for x, y in zip(st_a[i], st_b[i])) for i in (0, 1))
                tv = float((0.5 * (pa - pb).abs().sum(-1))[live].max())
                lines.append('ply %3d  live %3d  max|h - h_exact| %.3e  max|c - c_exact| %.3e  max TV(policy) %.3e'
                             % (t, int(live.sum()), dh, dc, tv))
            env.step(torch.multinomial(pa, 1, generator=rng).view(-1), live)
    return lines


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
    forms = {'module path': net, 'hrl_geister_infer': hnn.GeisterInference(net),
             'hrl_geister_infer_bf16': hnn.GeisterInference(net, precision='bf16')}
    lines = ['%s, torch %s' % (torch.cuda.get_device_name(dev), torch.__version__),
             'GeisterNet eval forward, us per ply: captured graphs, the three forms alternating, %d replays x %d '
             'repetitions' % (args.iters, args.reps)]
    with torch.no_grad():
        for N in args.sizes:
            with net.inference_session(inplace_state=True), forms['hrl_geister_infer'].inference_session(True), \
                    forms['hrl_geister_infer_bf16'].inference_session(True):
                caps = {k: captured_ply(m, N, dev, seed=N) for k, m in forms.items()}
                times = {k: [] for k in forms}
                for g, _ in caps.values():
                    timed(g, 10)
                for _ in range(args.reps):
                    for k, (g, _) in caps.items():
                        times[k].append(timed(g, args.iters))
            lines += [row('N = %5d  %s' % (N, k), xs, 'us') for k, xs in times.items()]
        if args.games:
            E = args.games
            lines.append('lockstep self-play, E = %d games, ms per generation (first ply to last), alternating' % E)
            gens = {k: DeviceGenerator(GeisterBatch(E, dev), m, gamma=0.8) for k, m in forms.items()}
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
            lines += [row(k, xs, 'ms') for k, xs in times.items()]
            lines.append('streaming self-play, %d slots, us per global step (a generate(E) call over its plies), '
                         'alternating' % E)
            cls = GeisterBatch
            gens = {k: StreamGenerator(cls(E, dev), m, DeviceReplay(4 * E, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P,
                                                                    dev, obs_dtype=torch.uint8), gamma=0.8, seed=1)
                    for k, m in forms.items()}
            times = {k: [] for k in gens}
            for rep in range(args.generations + 1):
                for k, gen in gens.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = gen.generate(E)
                    torch.cuda.synchronize()
                    if rep:
                        times[k].append((time.perf_counter() - t0) * 1e6 / out['plies'])
            lines += [row(k, xs, 'us') for k, xs in times.items()]
        lines.append('drift, 256 games, 200 plies, the exact form samples the moves (seeded-init net)')
        lines += drift(forms['hrl_geister_infer'], forms['hrl_geister_infer_bf16'], dev)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
