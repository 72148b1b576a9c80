"""Device evaluation of Hungry Geese (evaluation.PlayerEvaluator): what the relative-seat rows buy, and the baseline.

    python tools/geese_eval_bench.py [--out profiles/geese_eval.txt] [--slots 256 2048] [--reps 6] [--host-games 64]

On one GPU with seeded-init GeeseNets, graphs on, in one process and in ALTERNATING order, ``--reps`` (at least six)
calls each of G = 4 E games per call, wall clock around a device synchronise:
  (a) ``PlayerEvaluator`` against random agents: ``observe_seats(seat, 1)``, an E-row forward;
  (b) the same games with a 4 E-row forward -- all four views of every game (``observe_players_record``-style rows,
      player-major), the home seat's logits gathered by seat: what reusing the self-play ply would cost.  Its
      outcomes must equal (a)'s;
  (c) a match: ``observe_seats(seat, 4)``, the home net over rows[:E] and a second net over rows[E:];
and (d) the baseline without the device evaluator: one process stepping the host ``Environment`` game by game, the net
on batch-1 CPU inference for its seat and ``random.choice`` for the others, as the reference's ``exec_match`` loop does.

    python tools/geese_eval_bench.py --rule [--out profiles/geese_greedy.txt] [--slots 256 2048] [--reps 6]

measures the rule-based opponent instead: forms (a) and
  (r) ``PlayerEvaluator(opponent='rule')``: the same E-row forward as (a), one more launch (hrl_geese_greedy) and the
      decision through hrl_players_act_rule,
alternating in one process by the same scheme.  What compares is the ms per GLOBAL STEP; games against greedy geese are
about ten times longer than against random agents, so (r)'s games per second are far lower than (a)'s at the same cost
per step.
"""
import argparse
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from handyrl_amd.environment import make_env  # noqa: E402
from handyrl_amd.envs.geese import GEESE, GeeseNet, HungryGeeseBatch  # noqa: E402
from handyrl_amd.evaluation import PlayerEvaluator  # noqa: E402
from handyrl_amd.nn import accelerate  # noqa: E402

SEED = 1


class AllViews(PlayerEvaluator):
    """(b): every player's view is built and forwarded (4 E rows), and the home seat's logits are gathered."""

    def _rows(self, st, K):
        assert K == 1
        return self.env._views().view(GEESE * self.env.E, *self.env.OBS_SHAPE)


class _GatherHome(torch.nn.Module):
    """The net over the 4 E player-major rows; the policy rows of the home seats, in slot order."""

    def __init__(self, net, seat):
        super().__init__()
        self.net, self.seat = net, seat

    def forward(self, x, hidden=None):
        out = self.net(x, hidden)
        E = self.seat.shape[0]
        rows = torch.arange(E, device=x.device)
        return {'policy': out['policy'].view(GEESE, E, -1)[self.seat, rows]}


def evaluators(dev, E, rule=False):
    nets = []
    for seed in (7, 8):
        torch.manual_seed(seed)
        nets.append(accelerate(GeeseNet().to(dev)))

    def env():
        return HungryGeeseBatch(E, dev, seed=SEED)
    a = PlayerEvaluator(env(), nets[0], seed=SEED)
    if rule:
        return {'a': a, 'r': PlayerEvaluator(env(), nets[0], seed=SEED, opponent='rule')}
    b = AllViews(env(), nets[0], seed=SEED)
    b.net = _GatherHome(nets[0], b._state()['seat'])
    c = PlayerEvaluator(env(), nets[0], seed=SEED, opponent=nets[1], opening_plies=2)
    return {'a': a, 'b': b, 'c': c}


def host_rate(games):
    """(d): games per second of the one-process loop over the host env, batch-1 CPU inference on the home seat."""
    torch.manual_seed(7)
    net = GeeseNet()
    net.eval()
    env = make_env({'env': 'Geese', 'seed': SEED})
    random.seed(0)
    plies = 0
    t0 = time.perf_counter()
    with torch.no_grad():
        for g in range(games):
            env.games = g
            env.reset()
            seat = g % GEESE
            while not env.terminal():
                actions = {}
                for p in env.turns():
                    if p == seat:
                        x = torch.from_numpy(env.observation(p)).unsqueeze(0)
                        actions[p] = int(net(x, None)['policy'][0].argmax())
                    else:
                        actions[p] = random.choice(env.legal_actions(p))
                env.step(actions)
                plies += 1
    dt = time.perf_counter() - t0
    return games / dt, plies / games


def spread(xs):
    return '%.1f-%.1f, median %.1f' % (min(xs), max(xs), statistics.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rule', action='store_true', help='forms (a) and (r): the rule-based opponent')
    ap.add_argument('--out', default=None)
    ap.add_argument('--slots', type=int, nargs='+', default=[256, 2048])
    ap.add_argument('--reps', type=int, default=6)
    ap.add_argument('--host-games', type=int, default=64)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join('profiles', 'geese_greedy.txt' if args.rule else 'geese_eval.txt')
    if not torch.cuda.is_available():
        raise SystemExit('geese_eval_bench measures on the GPU; no GPU is visible')
    dev = torch.device('cuda', 0)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('Hungry Geese device evaluation, %s, seeded-init GeeseNet, graphs on, G = 4 E games per call, %d calls each in '
        'alternating order' % (torch.cuda.get_device_name(dev), max(6, args.reps)))
    for E in args.slots:
        G = 4 * E
        evs = evaluators(dev, E, args.rule)
        first = {k: ev.evaluate(G) for k, ev in evs.items()}        # capture and warm-up
        if not args.rule:
            assert torch.equal(first['a']['outcome'], first['b']['outcome']), 'the two forms must play the same games'
            assert torch.equal(first['a']['length'], first['b']['length'])
        runs = {k: [] for k in evs}
        for _ in range(max(6, args.reps)):
            for k, ev in evs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                res = ev.evaluate(G)
                torch.cuda.synchronize(dev)
                runs[k].append((time.perf_counter() - t0, res['plies'], res['env_steps']))
        names = {'a': '(a) vs random, E-row forward (K = 1)', 'b': '(b) vs random, 4E-row forward, gathered',
                 'c': '(c) match, K = 4 (E + 3E rows)', 'r': '(r) vs rule (greedy geese), E-row forward (K = 1)'}
        for k in evs:
            ms = [dt * 1e3 for dt, _, _ in runs[k]]
            per = [dt * 1e3 / plies for dt, plies, _ in runs[k]]
            rate = [G / dt for dt, _, _ in runs[k]]
            say('E = %d  %s: ms per call %s; ms per global step %s; games/s %s; global steps %d, mean game %.1f plies'
                % (E, names[k], spread(ms), '%.3f-%.3f, median %.3f' % (min(per), max(per), statistics.median(per)),
                   '%.0f-%.0f, median %.0f' % (min(rate), max(rate), statistics.median(rate)), runs[k][0][1],
                   runs[k][0][2] / G))
        if args.rule:
            pa, pr = (statistics.median(dt * 1e3 / plies for dt, plies, _ in runs[k]) for k in ('a', 'r'))
            say('E = %d  (r) - (a) ms per global step, medians: %+.3f (ratio %.3f); the games are %.1f times as long, '
                'so games/s are lower at the same cost per step; win rate of the seeded-init net vs random %.3f, vs '
                'rule %.3f' % (E, pr - pa, pr / pa, runs['r'][0][2] / runs['a'][0][2], first['a']['win_rate'],
                               first['r']['win_rate']))
            del evs
            continue
        ma, mb = (statistics.median(dt for dt, _, _ in runs[k]) for k in ('a', 'b'))
        say('E = %d  (a) / (b) time per call, medians: %.3f; win rate of the seeded-init net vs random %.3f'
            % (E, ma / mb, first['a']['win_rate']))
        del evs
    if not args.rule:
        rate, mean = host_rate(args.host_games)
        say('(d) host loop, one process, batch-1 CPU inference, %d games: %.1f games/s, mean game %.1f plies'
            % (args.host_games, rate, mean))
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
