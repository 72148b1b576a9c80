"""The TicTacToe net's eval forward: the net's own launches (plain) against nn.BoardInference (fused), one GPU.

    python tools/board_infer_bench.py --part forward|selfplay|league|all [--seconds 3] [--repeats 3] [--out FILE]

Every part builds both forms from the same seeded nets (``accelerate``d, eval mode: the nets of the device
generators), warms both up, then alternates their legs in one call; per form the median and the spread (min .. max)
over ``--repeats`` legs are reported, one JSON line per measurement.  The plain legs of the same call are the
baseline.

  forward   one forward at N = 4096 and 16384 rows: plain = ``net(x)`` (weights re-prepared per call), fused =
            ``BoardInference(net)(x)`` inside a session.  Each form is captured in a graph; a leg is 200 replays
            between two device events.  Launches per forward: the kernels of one eager call (torch.profiler).
  selfplay  ``DeviceGenerator`` lockstep at E = 4096, per-player (observation) at E = 16384, ``StreamGenerator`` at
            E = 4096, each with the plain net and with the wrapper: env-steps/s, ms per ply (a leg's time over its
            global steps) and the kernels of one call over its plies (torch.profiler, outside the timed legs; a call's
            reset, session and clones are counted in).
  league    K = 8 nets, E = 4088 slots, G = 4096 games per pairing (tools/league_bench.py's league): the plain nets,
            the wrappers ungrouped, and one ``board_inference_group``; also the sequential yardstick of that tool (one
            ``DeviceEvaluator`` match per pairing, plain nets), so that league / sequential can be read off.
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _net(dev, seed=0):
    import torch
    from handyrl_amd.envs.tictactoe import SimpleConv2dModel
    from handyrl_amd.nn import accelerate
    torch.manual_seed(seed)
    return accelerate(SimpleConv2dModel().to(dev)).eval()


def _kernels(fn, dev):
    """The number of GPU kernels ``fn()`` launches (None where the profiler gives no device events)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize(dev)
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return n or None
    except Exception as exc:   # measurement aid only: say so and go on
        print('launch count not measured: %r' % (exc,), file=sys.stderr)
        return None


def _stats(values):
    return {'median': statistics.median(values), 'min': min(values), 'max': max(values)}


def forward(dev, repeats, emit):
    import torch
    from handyrl_amd.nn import BoardInference
    net = _net(dev)
    fused = BoardInference(net)
    replays = 200
    for N in (4096, 16384):
        x = torch.randint(0, 2, (N, 3, 3, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(N)).float()
        with torch.no_grad(), fused.inference_session():
            forms = {'plain': lambda: net(x, None), 'fused': lambda: fused(x, None)}
            graphs, counts = {}, {}
            for name, fn in forms.items():
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(3):
                        fn()
                torch.cuda.current_stream(dev).wait_stream(side)
                counts[name] = _kernels(fn, dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                for _ in range(20):
                    g.replay()
                graphs[name] = g
            a, b = net(x, None), fused(x, None)
            diff = {k: float((a[k] - b[k]).abs().max()) for k in ('policy', 'value')}
            times = {k: [] for k in graphs}
            for _ in range(repeats):
                for name, g in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(replays):
                        g.replay()
                    e1.record()
                    e1.synchronize()
                    times[name].append(1e3 * e0.elapsed_time(e1) / replays)        # us per forward
        out = {'part': 'forward', 'N': N, 'replays_per_leg': replays, 'repeats': repeats,
               'max_abs_diff_plain_vs_fused': diff}
        for name in graphs:
            out[name] = {'us_per_forward': _stats(times[name]), 'launches': counts[name]}
        out['plain_over_fused'] = out['plain']['us_per_forward']['median'] / out['fused']['us_per_forward']['median']
        emit(out)


def _leg(call, seconds, sync):
    sync()
    t0 = time.perf_counter()
    steps, plies = [], []
    while time.perf_counter() - t0 < seconds:
        s, p = call()
        steps.append(s)
        plies.append(p)
    sync()
    dt = time.perf_counter() - t0
    nplies = sum(float(p) for p in plies)
    return {'env_steps_per_s': sum(float(s) for s in steps) / dt, 'ms_per_ply': 1e3 * dt / max(nplies, 1.0)}


def selfplay(dev, seconds, repeats, emit):
    import torch
    from handyrl_amd.nn import BoardInference
    from handyrl_amd.rollout import DeviceGenerator, DeviceReplay, StreamGenerator, TicTacToeBatch as cls
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731

    def lockstep(E, wrap, per_player):
        net = wrap(_net(dev))
        gen = DeviceGenerator(cls(E, dev), net, gamma=0.8, observation=per_player, per_player=per_player)
        rng = torch.Generator(device=dev).manual_seed(1)

        def call():
            ep = gen.generate(generator=rng)
            return ep['length'].sum(), gen._st['t'].clone()
        return call

    def stream(E, wrap):
        replay = DeviceReplay(4 * E, cls.MAX_PLIES, cls.OBS_SHAPE, cls.A, cls.P, dev, obs_dtype=torch.uint8)
        gen = StreamGenerator(cls(E, dev), wrap(_net(dev)), replay, gamma=0.8, seed=1)

        def call():
            out = gen.generate(E)
            return out['env_steps'], out['plies']
        return call
    modes = (('lockstep', 4096, lambda E, w: lockstep(E, w, False)),
             ('per_player', 16384, lambda E, w: lockstep(E, w, True)),
             ('stream', 4096, stream))
    for mode, E, make in modes:
        calls = {'plain': make(E, lambda n: n), 'fused': make(E, BoardInference)}
        for _ in range(2):
            for c in calls.values():
                c()
        sync()
        per_ply = {}
        for name, c in calls.items():
            got = []
            n = _kernels(lambda: got.append(c()), dev)
            per_ply[name] = None if n is None else n / max(float(got[0][1]), 1.0)
        legs = {k: [] for k in calls}
        for _ in range(repeats):
            for name, c in calls.items():
                legs[name].append(_leg(c, seconds, sync))
        out = {'part': 'selfplay', 'mode': mode, 'E': E, 'seconds_per_leg': seconds, 'repeats': repeats}
        for name, ls in legs.items():
            out[name] = {'env_steps_per_s': _stats([l['env_steps_per_s'] for l in ls]),
                         'ms_per_ply': _stats([l['ms_per_ply'] for l in ls]), 'launches_per_ply': per_ply[name]}
        out['fused_over_plain_env_steps'] = (out['fused']['env_steps_per_s']['median']
                                             / out['plain']['env_steps_per_s']['median'])
        emit(out)


def league(dev, repeats, emit):
    import torch
    from handyrl_amd.evaluation import DeviceEvaluator, LeagueEvaluator
    from handyrl_amd.nn import BoardInference, board_inference_group
    from handyrl_amd.rollout import TicTacToeBatch as cls
    K, E, G, OPENING, SEED = 8, 4088, 4096, 2, 1
    nets = [_net(dev, seed=k) for k in range(K)]
    pairs = [(i, j) for i in range(K) for j in range(i + 1, K)]
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731

    def league_of(agents):
        ev = LeagueEvaluator(cls(E, dev), agents, opening_plies=OPENING, seed=SEED)
        return lambda: ev.evaluate(G)['plies']

    def sequential():
        evs = [DeviceEvaluator(cls(E, dev), nets[i], opponent=nets[j], opening_plies=OPENING, seed=SEED)
               for i, j in pairs]
        return lambda: sum(ev.evaluate(G)['plies'] for ev in evs)
    legs = {'sequential_plain': sequential(), 'league_plain': league_of(nets),
            'league_fused_ungrouped': league_of([BoardInference(n) for n in nets]),
            'league_fused_grouped': league_of(board_inference_group(nets))}
    for c in legs.values():
        c()
    runs = {k: [] for k in legs}
    for _ in range(repeats):
        for name, c in legs.items():
            sync()
            t0 = time.perf_counter()
            plies = c()
            sync()
            dt = time.perf_counter() - t0
            runs[name].append({'seconds': dt, 'ms_per_ply': 1e3 * dt / plies, 'plies': plies})
    out = {'part': 'league', 'K': K, 'E': E, 'G': G, 'repeats': repeats}
    for name, rs in runs.items():
        out[name] = {'plies': rs[0]['plies'], 'seconds': _stats([r['seconds'] for r in rs]),
                     'ms_per_ply': _stats([r['ms_per_ply'] for r in rs])}
    base = out['sequential_plain']['seconds']['median']
    for name in ('league_plain', 'league_fused_ungrouped', 'league_fused_grouped'):
        out[name + '_over_sequential'] = out[name]['seconds']['median'] / base
    emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['forward', 'selfplay', 'league', 'all'])
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('board_infer_bench measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    if a.part in ('forward', 'all'):
        forward(dev, a.repeats, emit)
    if a.part in ('selfplay', 'all'):
        selfplay(dev, a.seconds, a.repeats, emit)
    if a.part in ('league', 'all'):
        league(dev, a.repeats, emit)


if __name__ == '__main__':
    main()
