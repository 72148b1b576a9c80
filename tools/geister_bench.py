"""Time the recurrent (GeisterNet, config C3) learner step on the GPU.

    python tools/geister_bench.py --B 256 1024 --T 16 --graph 0 1
    python tools/geister_bench.py --B 256 --graph 1 --precision fp32 bf16_drc bf16_drc_bwd --rounds 9

With more than one ``--precision`` (train_args' key) the forms run in ONE process, one learner each, alternating
round by round; every form reports the median and min-max of its rounds' mean step time.

One step = forward_prediction unrolled over T (3 ConvLSTM cells x 3 repeats
per step) + compute_loss + backward + clip + Adam on a synthetic Geister
batch (handyrl_amd.synthetic.geister_batch), hidden state zero at the window
start (train.py:375).
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from handyrl_amd.envs.geister import GeisterNet  # noqa: E402
from handyrl_amd.synthetic import geister_batch, default_args  # noqa: E402
from handyrl_amd.trainer import LearnerStep  # noqa: E402


def to_dev(h, device):
    return ([x.to(device) for x in h[0]], [x.to(device) for x in h[1]])


def run_forms(B, T, graph, steps, warmup, device, precisions, rounds):
    """One learner per precision on the same seeded net and batch; ``rounds`` timed windows each, alternating."""
    batch = geister_batch(B, T, device, seed=5)
    forms = []
    for p in precisions:
        torch.manual_seed(0)
        net = GeisterNet().to(device)
        hidden = to_dev(net.init_hidden([B, 2]), device)
        learner = LearnerStep(net, dict(default_args(T, B), precision=p), device, graph=bool(graph))
        for _ in range(warmup):
            learner.step(batch, hidden)
        forms.append((p, learner, hidden, []))
    for _ in range(rounds):
        for _, learner, hidden, times in forms:
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(steps):
                learner.step(batch, hidden)
            torch.cuda.synchronize(device)
            times.append((time.perf_counter() - t0) / steps * 1e3)
    for p, learner, _, times in forms:
        sums, n = learner.pop_stats()
        yield {'B': B, 'T': T, 'graph': graph, 'precision': p, 'rounds': rounds, 'steps_per_round': steps,
               'ms_per_step_median': round(sorted(times)[len(times) // 2], 4), 'ms_per_step_min': round(min(times), 4),
               'ms_per_step_max': round(max(times), 4), 'loss_total_mean': sums.get('total', 0.0) / max(n, 1)}


def run(B, T, graph, steps, warmup, device):
    args = default_args(T, B)
    torch.manual_seed(0)
    net = GeisterNet().to(device)
    batch = geister_batch(B, T, device, seed=5)
    hidden = to_dev(net.init_hidden([B, 2]), device)
    learner = LearnerStep(net, args, device, graph=bool(graph))
    for _ in range(warmup):
        learner.step(batch, hidden)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        learner.step(batch, hidden)
    torch.cuda.synchronize(device)
    dt = (time.perf_counter() - t0) / steps
    sums, n = learner.pop_stats()
    return {'B': B, 'T': T, 'graph': graph, 'ms_per_step': round(dt * 1e3, 3),
            'env_steps_per_s': round(B * T / dt, 1), 'loss_total_mean': sums.get('total', 0.0) / max(n, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--T', type=int, nargs='+', default=[16])
    ap.add_argument('--graph', type=int, nargs='+', default=[0, 1])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--flat', type=int, nargs='+', default=[1], help='train.FLAT_HIDDEN values to compare')
    ap.add_argument('--precision', nargs='+', default=None, help="train_args' precision values to alternate")
    ap.add_argument('--rounds', type=int, default=9, help='timed windows per precision (with --precision)')
    opts = ap.parse_args()
    device = torch.device('cuda', 0)
    if 'HRL_GBOARD_WHOLE' in os.environ:   # hrl_gboard's whole-k-step ring on (default) / off
        from handyrl_amd import _native
        _native.load().hrl_gboard_set_whole_ring(int(os.environ['HRL_GBOARD_WHOLE']))
    import handyrl_amd.train as train_mod
    for flat in opts.flat:
        train_mod.FLAT_HIDDEN = bool(flat)
        for T in opts.T:
            for B in opts.B:
                for g in opts.graph:
                    if opts.precision:
                        for r in run_forms(B, T, g, opts.steps, opts.warmup, device, opts.precision, opts.rounds):
                            print(json.dumps(r), flush=True)
                        continue
                    r = run(B, T, g, opts.steps, opts.warmup, device)
                    r['flat_hidden'] = flat
                    print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
