"""The fused value-head scan (VTRACE target + UPGO advantages) on contiguous, windowed, time-major and broadcast
operands: HIP events around graph-captured back-to-back launches, as tools/scan_sweep.py takes them.

It calls the public operator only, so the same file run in a checkout of an earlier commit measures what that
commit does for the same inputs (there: one copy kernel per non-contiguous operand, then the contiguous scan).

    python tools/scan_strided_bench.py [--out profiles/scan_strided.txt] [--repeat 2] [--quick] [--patterns a,b]

Bytes are the algorithmic ones of the scan itself (every distinct input element once, both outputs once), so the
GB/s of a run that copies first is the useful rate, not the traffic.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import HBM_PEAK_GBS  # noqa: E402

P, K = 2, 1


def make_set(pattern, B, T, dev, g):
    """(values, returns, rhos, cs) of logical shapes (B,T,P,K), (B,1,P,K), (B,T,P,K)|(B,T,1,1), (B,T,1,1)."""
    def rnd(*shape):
        return torch.rand(*shape, device=dev, generator=g)
    if pattern == 'contiguous':
        return rnd(B, T, P, K), rnd(B, 1, P, K), rnd(B, T, 1, 1), rnd(B, T, 1, 1)
    if pattern == 'window':        # pattern 1: [:, 3:3+T] of a buffer of T+5 steps
        w = slice(3, 3 + T)
        return rnd(B, T + 5, P, K)[:, w], rnd(B, 1, P, K), rnd(B, T + 5, 1, 1)[:, w], rnd(B, T + 5, 1, 1)[:, w]
    if pattern == 'window16':      # the same with 16-byte friendly extents: [:, 4:4+T] of a buffer of T+8 steps
        w = slice(4, 4 + T)
        return rnd(B, T + 8, P, K)[:, w], rnd(B, 1, P, K), rnd(B, T + 8, 1, 1)[:, w], rnd(B, T + 8, 1, 1)[:, w]
    if pattern == 'time_major':    # pattern 3: (T, B, ...) storage seen as (B, T, ...)
        tm = lambda *s: rnd(*s).permute(1, 0, 2, 3)   # noqa: E731
        return tm(T, B, P, K), rnd(B, 1, P, K), tm(T, B, 1, 1), tm(T, B, 1, 1)
    if pattern == 'broadcast':     # pattern 5: the outcome over players, rhos over players as a value-shaped view
        return rnd(B, T, P, K), rnd(B, 1, 1, 1).expand(B, 1, P, K), rnd(B, T, 1, 1).expand(B, T, P, K), rnd(B, T, 1, 1)
    raise ValueError(pattern)


def scan_bytes(pattern, B, T):
    inputs = B * T * P * K + B * (1 if pattern == 'broadcast' else P * K) + 2 * B * T
    return 4 * (inputs + 2 * B * T * P * K)


def time_one(pattern, B, T, dev, iters, cold):
    from handyrl_amd.losses import compute_targets_fused
    g = torch.Generator(device=dev).manual_seed(7)
    nbytes = scan_bytes(pattern, B, T)
    # cold: rotate through enough input sets that every launch misses the 256 MiB Infinity Cache
    n_sets = max(2, int(3 * 256 * 2 ** 20 // nbytes) + 1) if cold else 1
    sets = [make_set(pattern, B, T, dev, g) for _ in range(n_sets)]

    def launch(i):
        v, ret, rho, cs = sets[i % n_sets]
        compute_targets_fused('VTRACE', 'UPGO', v, ret, None, 0.7, 1, rho, cs)
    for i in range(2):
        launch(i)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        launch(0)
    torch.cuda.current_stream(dev).wait_stream(side)
    with torch.cuda.graph(graph):
        for i in range(iters):
            launch(i)
    stream = torch.cuda.current_stream(dev)
    graph.replay()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record(stream)
    graph.replay()
    end.record(stream)
    end.synchronize()
    us = start.elapsed_time(end) * 1e3 / iters
    del graph, sets
    torch.cuda.empty_cache()
    return us, nbytes / (us * 1e-6) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--repeat', type=int, default=2, help='runs per configuration (the spread is the noise floor)')
    ap.add_argument('--patterns', default='contiguous,window,window16,time_major,broadcast')
    ap.add_argument('--quick', action='store_true', help='leave out B = 2^20')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sizes = [(4096, 32, False), (1 << 18, 32, True), (1 << 18, 9, True)]
    if not args.quick:
        sizes += [(1 << 20, 32, True), (1 << 20, 9, True)]
    lines = ['%-11s %8s %3s %-4s %s   GB/s of best (%% of HBM peak)' % (
        'operands', 'B', 'T', '', '  '.join('run%d us' % (i + 1) for i in range(args.repeat)))]
    print(lines[0], flush=True)
    for pattern in args.patterns.split(','):
        for B, T, cold in sizes:
            iters = 200 if not cold else (50 if B <= (1 << 18) else 20)
            runs = [time_one(pattern, B, T, dev, iters, cold) for _ in range(args.repeat)]
            best = max(r[1] for r in runs)
            line = '%-11s %8d %3d %-4s %s   %8.1f (%4.1f%%)' % (
                pattern, B, T, 'cold' if cold else 'hot', '  '.join('%9.2f' % r[0] for r in runs), best,
                100 * best / HBM_PEAK_GBS)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
