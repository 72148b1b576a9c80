"""Time the GeeseNet learner step with the mixed-precision tower (train_args precision: bf16) and with its fused tail
(precision: bf16_heads) in ONE process, as captured graphs on the same synthetic batch, alternating the two forms
within every repetition.

    python tools/geese_learner_bf16_heads_bench.py --B 2048 --T 64 --reps 7 --steps 5 \\
        > profiles/geese_learner_bf16_heads.txt

Prints, per form, the minimum, median and maximum ms per step over the repetitions and the peak memory of its
warm-up (torch.cuda.max_memory_allocated, reset before each form is built), then the verdict: the fused tail is
faster only if the medians differ by more than the larger of the two spreads (max - min), and it is `not_slower` if
its median is not above bf16's by more than that spread.  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/geese_learner_bf16_heads_bench.py --reps 1 --only FORM` run.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from handyrl_amd.envs.hungry_geese import GeeseNet  # noqa: E402
from handyrl_amd.synthetic import geese_args, geese_batch  # noqa: E402
from handyrl_amd.trainer import LearnerStep  # noqa: E402

FORMS = ('bf16', 'bf16_heads')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=2048)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', choices=FORMS, default=None, help='one form alone (a profiler run)')
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('geese_learner_bf16_heads_bench: no GPU; a timing needs one')
    dev = torch.device('cuda', 0)
    batch = geese_batch(o.B, o.T, dev, seed=5)
    learners, peak = {}, {}
    for precision in (FORMS if o.only is None else (o.only,)):
        torch.manual_seed(0)
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        learners[precision] = LearnerStep(GeeseNet(), dict(geese_args(o.T, o.B), precision=precision), dev, graph=True)
        for _ in range(o.warmup):   # eager step, capture and warm replays
            learners[precision].step(batch)
        torch.cuda.synchronize(dev)
        peak[precision] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 30   # above what was held before it
    ms = {p: [] for p in learners}
    for _ in range(o.reps):
        for precision, learner in learners.items():
            t0 = time.perf_counter()
            for _ in range(o.steps):
                learner.step(batch)
            torch.cuda.synchronize(dev)
            ms[precision].append((time.perf_counter() - t0) / o.steps * 1e3)
    res = {'B': o.B, 'T': o.T, 'reps': o.reps, 'steps_per_rep': o.steps}
    for p, v in ms.items():
        res[p] = {'min_ms': round(min(v), 3), 'median_ms': round(statistics.median(v), 3), 'max_ms': round(max(v), 3),
                  'peak_GiB_above_start': round(peak[p], 3)}
    if o.only is None:
        spread = max(max(v) - min(v) for v in ms.values())
        gain = statistics.median(ms['bf16']) - statistics.median(ms['bf16_heads'])
        res['median_gain_ms'], res['larger_spread_ms'] = round(gain, 3), round(spread, 3)
        res['bf16_heads_faster_beyond_spread'] = bool(gain > spread)
        res['bf16_heads_not_slower'] = bool(-gain <= spread)
        res['peak_GiB_saved'] = round(peak['bf16'] - peak['bf16_heads'], 3)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
