"""Time the GeeseNet learner step with the fp32 tower and with the mixed-precision tower (train_args precision:
bf16) in ONE process, as captured graphs on the same synthetic batch, alternating the two forms within every
repetition.

    python tools/geese_learner_bf16_bench.py --B 2048 --T 64 --reps 7 --steps 10 > profiles/geese_learner_bf16.txt

Prints, per form, the minimum, median and maximum ms per step over the repetitions, and the verdict: bf16 is faster
only if the medians differ by more than the larger of the two spreads (max - min).  Per-kernel medians come from a
separate `rocprofv3 --kernel-trace --stats -- python tools/geese_learner_bf16_bench.py --reps 1` run.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=2048)
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('geese_learner_bf16_bench: no GPU; a timing needs one')
    dev = torch.device('cuda', 0)
    batch = geese_batch(o.B, o.T, dev, seed=5)
    learners = {}
    for precision in ('fp32', 'bf16'):
        torch.manual_seed(0)
        learners[precision] = LearnerStep(GeeseNet(), dict(geese_args(o.T, o.B), precision=precision), dev, graph=True)
        for _ in range(o.warmup):   # eager step, capture and warm replays
            learners[precision].step(batch)
    torch.cuda.synchronize(dev)
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
        res[p] = {'min_ms': round(min(v), 3), 'median_ms': round(statistics.median(v), 3), 'max_ms': round(max(v), 3)}
    spread = max(max(v) - min(v) for v in ms.values())
    gain = statistics.median(ms['fp32']) - statistics.median(ms['bf16'])
    res['bf16_faster_beyond_spread'] = bool(gain > spread)
    res['median_gain_ms'], res['larger_spread_ms'] = round(gain, 3), round(spread, 3)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
