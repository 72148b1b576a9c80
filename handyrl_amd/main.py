"""Config-driven learner entry point: the reference's ``main.py --train`` on one GPU node.

    python -m handyrl_amd.main --train [config.yaml]
    python -m handyrl_amd.main --eval MODEL_PATH [NUM_GAMES] [SLOTS]
    python -m handyrl_amd.main --eval-match MODEL_A MODEL_B [NUM_GAMES] [SLOTS]
    python -m handyrl_amd.main --eval-rulebase MODEL_PATH [NUM_GAMES] [SLOTS]
    python -m handyrl_amd.main --eval-league MODEL_OR_DIR [MODEL_OR_DIR ...] [NUM_GAMES] [SLOTS]
    python -m torch.distributed.run --nproc-per-node N -m handyrl_amd.main --train [config.yaml]

Reads the reference's ``config.yaml`` (main.py:13-15; config.yaml:1-35;
docs/parameters.md) -- ``env_args`` and ``train_args`` -- and runs the
reference's training cycle (train.py:425-560: workers generate episodes,
the trainer steps on recency-weighted windows, every ``update_episodes``
episodes an epoch ends, the lr is rescheduled and ``models/<epoch>.pth`` is
written) with the actors and the learner on the GPU:

* ``prepare_env`` / ``make_env`` resolve the env by name or module path
  (environment.py:18-39) and ``env.net()`` gives the model class;
* generation: an env module with a batched (device) twin (TicTacToe,
  ParallelTicTacToe, Geister, CIGeister, Geese) is played by
  ``rollout.DeviceGenerator``: in the stock layout of an alternating env
  (turn_based_training, no opponent observation) the mover-only ply into
  ``rollout.DeviceReplay``; with ``observation: True``, solo training or a
  simultaneous-move env the per-player ply (every player's view, records
  with a player axis) into ``rollout.PlayerReplay``.  ANY other env -- a
  user's module, the reference's own plugins named by module path -- is
  played through the plugin API by ``hostgen.HostBatchGenerator`` (host
  envs, one batched GPU forward per ply, generation.py's semantics) into
  ``hostgen.MomentReplay``; ``generator: host`` in train_args forces that
  path for every env;
* ``self_play: stream`` in train_args (default ``lockstep``) plays the stock mode of an alternating env with
  ``rollout.StreamGenerator`` instead: ``stream_slots`` game slots (default: the rank's ``update_episodes``), a
  finished game written into the ``DeviceReplay`` ring by one launch and its slot restarted at once, so no slot
  waits for the longest game of a batch.  Every call plays until ``update_episodes`` more games are in the ring
  (it may overshoot by less than one check interval) and the episode counts follow what was actually emitted;
  a simultaneous-move env (Hungry Geese, ParallelTicTacToe) with ``observation`` or solo training
  (``turn_based_training: False``) streams its per-player ply with ``rollout.PlayerStreamGenerator`` into a
  ``PlayerReplay`` the same way, a finished slot restarting on the very next step; any other mode with ``stream``
  (an alternating env with ``observation`` or solo training, a simultaneous env in the stock mode) raises at start-up;
* ``self_play: fused`` is the lockstep generator with ``fused_game=True``: every ``generate`` call is one launch that
  plays all the games to the end (TicTacToe's stock mode on a CUDA device with ``inference: fused``; else it raises);
* ``update_episodes`` games per epoch with the current weights (the
  reference's workers hold the latest published model), recency-weighted
  replay of ``maximum_episodes``; training starts once ``minimum_episodes``
  are stored.  The three counts are global, as in the reference: under
  torchrun each rank generates and keeps 1/world of them.  The device
  replays assemble every batch in one launch into one reused batch;
  ``window_draw: inverse`` in train_args also draws the windows in one
  launch (default ``multinomial``: the seeded ``sample_windows`` stream);
* ``trainer.Trainer`` runs the epoch (its lr / data-count EMA schedule is the
  reference's, train.py:394-401) for ``steps_per_epoch`` steps (default: the
  epoch's new env-steps of ALL ranks over the global batch world*B*T, at
  least 1 -- every rank runs the same count, so their collectives pair up);
* data parallel under torchrun: every rank generates and trains its own
  shard, the gradients are SUMmed over RCCL (distributed.py), rank 0 saves.

* evaluation: ``eval_rate`` > 0 in train_args makes rank 0 play the reference's per-epoch evaluation after each
  epoch's training -- the greedy model against random agents on the device (``evaluation.DeviceEvaluator``,
  ``eval_slots`` slots, ``eval_temperature``) -- and append its win rate to the epoch's log line;
  ``--eval MODEL_PATH [NUM_GAMES] [SLOTS]`` evaluates a checkpoint (evaluation.py:291-312).  ``env: Geese`` is
  evaluated by ``evaluation.PlayerEvaluator`` (every goose moves every ply: the net on seat ``g mod 4``, random
  agents or the ``eval_opponent`` net on the three others; ``--eval-match`` seats MODEL_B there and prints one
  ``default`` table per agent); for the per-epoch evaluation that takes ``eval_simultaneous: true`` beside
  ``eval_rate`` -- ``eval_rate`` alone on a simultaneous-move env raises at start-up as it always has;
  ParallelTicTacToe and ``--eval-league`` on Geese stay refused;
* matches: the win rate against random agents saturates within a few epochs, so ``eval_opponent`` in train_args
  seats a second net on the other seats of the per-epoch evaluation instead (the reference's match of one ``Agent``
  per model, evaluation.py:64-116): a path to a ``.pth`` is a fixed anchor loaded once, ``previous`` is the model
  as it was at the end of the previous epoch (at the first epoch: as training started), absent or ``random`` is the
  evaluation above.  The first ``eval_opening_plies`` plies (default 2) of every game are uniform random moves on
  both seats: two greedy agents on a deterministic env play the same game every time, so 0 with
  ``eval_temperature`` 0 replays two games, one per seating.  The epoch line then ends ``vs previous`` or
  ``vs <path>``.  ``--eval-match MODEL_A MODEL_B [NUM_GAMES] [SLOTS]`` plays two checkpoints against each other
  and prints the reference's per-agent tables (evaluation.py:233-248).  Training is bit-identical with and
  without the key.
* a rule-based opponent: ``eval_opponent: rulebase`` (``env: Geese`` with ``eval_simultaneous: true``) seats the env's
  rule-based agent on the three other seats -- this project's greedy goose, ``envs.geese.greedy_action_of``, modelled
  on the published behaviour of Kaggle's GreedyAgent, not that agent move for move -- and the epoch line ends
  ``vs rulebase``; no net is constructed and ``eval_opening_plies`` defaults to 0 (the games differ by game number).
  ``--eval-rulebase MODEL_PATH [NUM_GAMES] [SLOTS]`` evaluates a checkpoint that way and prints ``--eval-match``'s
  per-agent tables (agent 1: the rule's three seats).  An env without a rule-based agent raises at start-up.
* leagues: ``--eval-league MODEL_OR_DIR [MODEL_OR_DIR ...] [NUM_GAMES] [SLOTS]`` plays a round robin of checkpoints
  (a directory expands to its ``<epoch>.pth`` files in epoch order) in one run on the device
  (``evaluation.LeagueEvaluator``): NUM_GAMES games per pairing, each game the one ``--eval-match`` would play, every
  net forwarded only over the rows where it moves.  It prints one line per agent with its Bradley-Terry rating (Elo,
  mean 0), win rate and game count, and the cross table of win rates.

The worker/server network plane, the network match server and client (their match itself is ``--eval-match``) and
the other CLI modes are not rebuilt.
"""

import math
import os
import sys
import time

import torch
import yaml

from . import distributed as hdist
from .environment import make_env, prepare_env
from .hostgen import HostBatchGenerator, MomentReplay
from .rollout import (DeviceGenerator, DeviceReplay, ParallelTicTacToeBatch, PlayerReplay, PlayerStreamGenerator,
                      StreamGenerator, TicTacToeBatch)
from .trainer import Trainer


def _batched_envs():
    from .envs.geister import GeisterBatch
    from .envs.ci_geister import CIGeisterBatch
    from .envs.geese import HungryGeeseBatch
    return {'handyrl_amd.envs.tictactoe': TicTacToeBatch, 'handyrl_amd.envs.geister': GeisterBatch,
            'handyrl_amd.envs.ci_geister': CIGeisterBatch, 'handyrl_amd.envs.geese': HungryGeeseBatch,
            'handyrl_amd.envs.parallel_tictactoe': ParallelTicTacToeBatch}


TRAIN_DEFAULTS = {   # config.yaml:9-31
    'turn_based_training': True, 'observation': False, 'gamma': 0.8, 'forward_steps': 16,
    'compress_steps': 4, 'entropy_regularization': 1.0e-1, 'entropy_regularization_decay': 0.1,
    'update_episodes': 200, 'batch_size': 256, 'minimum_episodes': 400, 'maximum_episodes': 100000,
    'epochs': -1, 'lambda': 0.7, 'policy_target': 'UPGO', 'value_target': 'VTRACE', 'seed': 0,
    'restart_epoch': 0,
}


def load_config(path='config.yaml'):
    with open(path) as f:
        args = yaml.safe_load(f)
    args['train_args'] = {**TRAIN_DEFAULTS, **(args.get('train_args') or {})}
    return args


class ReplayBatcher:
    """``batch()`` for Trainer: one window batch gathered on the device from the replay (train.py:284-309)."""

    def __init__(self, replay, args, generator):
        self.replay, self.args, self.g = replay, args, generator
        self._out = None

    def batch(self):
        B, T = self.args['batch_size'], self.args['forward_steps']
        if not hasattr(self.replay, 'alloc_batch'):   # the host replay assembles a fresh batch
            return self.replay.sample(B, T, generator=self.g)
        # One batch for every step, gathered in place (a graph learner keeps it as its static input).  Reuse is
        # safe by stream order: the gather runs on the stream of the step that last read these tensors.
        if self._out is None:
            self._out = self.replay.alloc_batch(B, T)
        return self.replay.sample(B, T, generator=self.g, out=self._out)


def _per_rank(n, world):
    return max(1, -(-int(n) // world))


def _eval_opponent(env, net, spec, device):
    """The opponent module of ``eval_opponent``: ``env.net()()`` holding ``net``'s weights (``previous``) or the
    checkpoint ``spec``.  Constructing a net draws initial weights, so the torch RNG state is put back: training
    draws what it draws without the key."""
    cpu_state = torch.get_rng_state()
    dev_state = torch.cuda.get_rng_state(device) if device.type == 'cuda' else None
    try:
        opponent = env.net()()
    finally:
        torch.set_rng_state(cpu_state)
        if dev_state is not None:
            torch.cuda.set_rng_state(dev_state, device)
    opponent.load_state_dict(net.state_dict() if spec == 'previous'
                             else torch.load(spec, map_location='cpu', weights_only=True))
    opponent = opponent.to(device)
    if device.type == 'cuda':
        from .nn import accelerate
        accelerate(opponent)
    return opponent


def train_main(args, device=None, loss_fn=None, model_dir='models', log=print):
    """The learner cycle of train.py:425-560 on the device; returns the trained model (CPU copy)."""
    env_args, targs = args['env_args'], {**TRAIN_DEFAULTS, **args['train_args']}
    rank, world, local = hdist.init_process_group('cuda' if device is None else device.type)
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError('handyrl_amd.main trains on the GPU (HIP kernels); no GPU is visible')
        device = torch.device('cuda', local)
        torch.cuda.set_device(device)
    prepare_env(env_args)
    env = make_env(env_args)
    module = type(env).__module__
    batched = _batched_envs().get(module)
    mode = targs.get('generator', 'auto')
    if mode not in ('auto', 'device', 'host'):
        raise ValueError("train_args['generator'] must be auto, device or host, not %r" % (mode,))
    # the mover-only ply for the stock mode of an alternating env, the per-player ply (every player's view,
    # records with a player axis) with observation, for simultaneous envs and for solo training
    tbt, observe = targs['turn_based_training'], targs['observation']
    per_player = observe or not tbt or getattr(batched, 'SIMULTANEOUS', False)
    if mode == 'device' and batched is None:
        raise ValueError('no batched (device) form of env %r' % module)
    use_device = batched is not None and mode != 'host'
    seed = int(targs['seed']) + rank
    torch.manual_seed(targs['seed'])            # the same initial weights on every rank
    net = env.net()()
    restart = int(targs['restart_epoch'])
    if restart > 0:
        net.load_state_dict(torch.load(os.path.join(model_dir, '%d.pth' % restart), map_location='cpu',
                                       weights_only=True))
    net = net.to(device)
    # train_args['inference']: fused -- self-play and the per-epoch evaluation run the net's one-launch eval forward
    # (nn.BoardInference, which refers to `net`); the learner trains `net` itself.  Absent: `net` plays as it is
    from .nn import configured_inference
    infer_mode = targs.get('inference')
    play_net = configured_inference(infer_mode, [net], device)[0]
    # the episode counts are global (train.py:480-503, 549-552): each rank plays and keeps 1/world of them
    games = _per_rank(targs['update_episodes'], world)
    minimum = _per_rank(targs['minimum_episodes'], world)
    maximum = _per_rank(targs['maximum_episodes'], world)
    rng = torch.Generator(device=device).manual_seed(seed)
    self_play = targs.get('self_play', 'lockstep')
    if self_play not in ('lockstep', 'stream', 'fused'):
        raise ValueError("train_args['self_play'] must be lockstep, stream or fused, not %r" % (self_play,))
    if self_play == 'fused' and (device.type != 'cuda' or not use_device or per_player or batched is not TicTacToeBatch
                                 or infer_mode != 'fused'):
        raise ValueError("train_args['self_play']: 'fused' plays whole TicTacToe games in one launch: it needs a CUDA "
                         "device, the stock mode (turn_based_training without observation) of the TicTacToe batched "
                         "env and inference: fused; this configuration is played by self_play: lockstep")
    # a simultaneous-move env under a per-player configuration (observation or solo training) streams its per-player
    # ply (PlayerStreamGenerator), an alternating env in the stock mode its mover-only ply
    stream_players = use_device and getattr(batched, 'SIMULTANEOUS', False) and (observe or not tbt)
    if self_play == 'stream' and not stream_players and (not use_device or per_player
                                                        or not getattr(batched, 'ALTERNATING', False)):
        raise ValueError("train_args['self_play']: 'stream' plays the mover-only ply of an alternating env with a "
                         "batched (device) form (turn_based_training without observation); this configuration is "
                         "played by the lockstep generator (self_play: lockstep)")
    evaluator = None
    eval_vs = targs.get('eval_opponent')
    if float(targs.get('eval_rate') or 0) > 0:
        # the reference's per-epoch evaluation (train.py:519-526); an env it cannot play raises here, at start-up
        from .evaluation import (DeviceEvaluator, PlayerEvaluator, batched_env, eval_games, opening_plies,
                                 player_eval_env, rule_eval_env)
        # Hungry Geese (every player moves every ply) is evaluated by PlayerEvaluator once `eval_simultaneous` says so;
        # without that key a simultaneous-move env raises here as it always has
        eval_players = player_eval_env(module) if targs.get('eval_simultaneous') else None
        eval_cls = eval_players or batched_env(module)
        eval_n = eval_games(targs['eval_rate'], targs['update_episodes'])
        # `rulebase`: the env's rule-based agent on the other seats (Hungry Geese's greedy goose); an env without one
        # raises here.  No net is constructed and no generator drawn from
        if eval_vs == 'rulebase':
            rule_eval_env(module)
        # a second net on the other seats: a checkpoint (a fixed anchor) or `previous`; a bad path raises here
        elif eval_vs not in (None, 'random', 'previous') and not os.path.isfile(str(eval_vs)):
            raise FileNotFoundError("train_args['eval_opponent'] is random, previous, rulebase or a checkpoint: no "
                                    "file %r" % (eval_vs,))
        if rank == 0:
            eval_slots = max(1, min(int(targs.get('eval_slots') or eval_n), eval_n))
            match = {}
            if eval_vs == 'rulebase':
                match = {'opponent': 'rule', 'opening_plies': int(targs.get('eval_opening_plies') or 0)}
            elif eval_vs not in (None, 'random'):
                opponent = _eval_opponent(env, net, eval_vs, device)
                match = {'opponent': configured_inference(infer_mode, [opponent], device)[0],
                         'opening_plies': opening_plies(targs)}
            if eval_players is not None:
                eval_batch = eval_cls(eval_slots, device)
                eval_batch.seed(seed)               # game g of an evaluation is Geese game number g under this seed
                evaluator = PlayerEvaluator(eval_batch, play_net,
                                            temperature=float(targs.get('eval_temperature', 0.0)), seed=seed, **match)
            else:
                evaluator = DeviceEvaluator(eval_cls(eval_slots, device), play_net, observation=observe,
                                            temperature=float(targs.get('eval_temperature', 0.0)), seed=seed, **match)
    played = None   # a generator that reports what it emitted (stream): episodes of the last play()
    if use_device and self_play == 'stream' and stream_players:
        slots = int(targs.get('stream_slots') or games)
        env_batch = batched(slots, device)
        if hasattr(env_batch, 'seed'):     # an env with randomness of its own (Geese's food): per rank, like `rng`
            env_batch.seed(seed)
        replay = PlayerReplay(maximum, batched.MAX_PLIES, batched.OBS_SHAPE, batched.A, batched.P, device,
                              maximum_episodes=maximum, obs_dtype=torch.uint8, solo=not tbt,
                              mover=tbt and not observe, draw=targs.get('window_draw', 'multinomial'))
        gen = PlayerStreamGenerator(env_batch, play_net, replay, gamma=targs['gamma'], seed=seed, observation=observe)
        played = [0]

        def play():
            out = gen.generate(games)       # at least `games` more episodes, straight into the ring
            played[0] = out['episodes']
            return float(out['env_steps'])
    elif use_device and self_play == 'stream':
        slots = int(targs.get('stream_slots') or games)
        replay = DeviceReplay(maximum, batched.MAX_PLIES, batched.OBS_SHAPE, batched.A, batched.P, device,
                              maximum_episodes=maximum, obs_dtype=torch.uint8,
                              draw=targs.get('window_draw', 'multinomial'))
        gen = StreamGenerator(batched(slots, device), play_net, replay, gamma=targs['gamma'], seed=seed)
        played = [0]

        def play():
            out = gen.generate(games)       # at least `games` more episodes, straight into the ring
            played[0] = out['episodes']
            return float(out['env_steps'])
    elif use_device:
        env_batch = batched(games, device)
        if hasattr(env_batch, 'seed'):     # an env with randomness of its own (Geese's food): per rank, like `rng`
            env_batch.seed(seed)
        gen = DeviceGenerator(env_batch, play_net, gamma=targs['gamma'], observation=observe,
                              per_player=per_player, fused_game=self_play == 'fused')
        # binary observation planes live in HBM as uint8 (widened by the gather)
        if per_player:
            replay = PlayerReplay(maximum, batched.MAX_PLIES, batched.OBS_SHAPE, batched.A, batched.P, device,
                                  maximum_episodes=maximum, obs_dtype=torch.uint8, solo=not tbt,
                                  mover=tbt and not observe, draw=targs.get('window_draw', 'multinomial'))
        else:
            replay = DeviceReplay(maximum, batched.MAX_PLIES, batched.OBS_SHAPE, batched.A, batched.P, device,
                                  maximum_episodes=maximum, obs_dtype=torch.uint8,
                                  draw=targs.get('window_draw', 'multinomial'))

        def play():
            ep = gen.generate(generator=rng)
            replay.add(ep)
            return float(ep['length'].float().sum())
    else:
        slots = min(games, int(targs.get('host_envs', 256)))
        made = [0]

        def host_env():
            # an env that numbers its games per instance under a seed from its args (SEEDED: Geese) gets a seed per
            # slot and rank unless env_args name one: otherwise every slot would play the same games
            if 'seed' in env_args or not getattr(type(env), 'SEEDED', False):
                return make_env(env_args)
            made[0] += 1
            return make_env({**env_args, 'seed': (seed << 20) + made[0]})
        gen = HostBatchGenerator(host_env, play_net, targs, E=slots, seed=seed)
        replay = MomentReplay({**targs, 'maximum_episodes': maximum}, device, maximum_episodes=maximum)

        def play():
            eps = gen.generate(games)
            replay.add(eps)
            return float(sum(ep['steps'] for ep in eps))
    trainer = Trainer(targs, net, ReplayBatcher(replay, targs, rng), device=device, world_size=world,
                      loss_fn=loss_fn)
    episodes = 0
    t0 = time.perf_counter()

    def generate():
        nonlocal episodes
        steps = play()
        episodes += games if played is None else played[0]
        return steps

    def global_steps(n):
        """Every rank's new env-steps summed: all ranks derive the same step count from it."""
        if world == 1:
            return n
        t = torch.tensor([n], dtype=torch.float64, device=device if device.type == 'cuda' else 'cpu')
        return float(hdist.all_reduce_sum_([t])[0].item())

    new_steps = 0.0
    while episodes < minimum:
        new_steps += generate()
    epoch = restart
    model = None
    while targs['epochs'] < 0 or epoch < restart + targs['epochs']:
        new_steps += generate()
        steps = targs.get('steps_per_epoch') or max(1, math.ceil(
            global_steps(new_steps) / (world * targs['batch_size'] * targs['forward_steps'])))
        new_steps = 0.0
        model = trainer.train(max_steps=int(steps))
        epoch += 1
        if rank == 0:
            os.makedirs(model_dir, exist_ok=True)
            torch.save(model.state_dict(), os.path.join(model_dir, '%d.pth' % epoch))
            line = 'epoch %d: episodes %d, steps %d, lr %.3e (%.1fs)' % (epoch, episodes * world, trainer.steps,
                                                                         trainer.lr, time.perf_counter() - t0)
            if evaluator is not None:
                res = evaluator.evaluate(eval_n)
                line += ', win rate %.3f (%.1f / %d)' % (res['win_rate'], res['win_rate'] * eval_n, eval_n)
                if evaluator.opponent is not None or eval_vs == 'rulebase':
                    line += ' vs %s' % (eval_vs,)
                    if eval_vs == 'previous':     # the next epoch's opponent: the model as it is now, in place
                        evaluator.set_opponent_state(model.state_dict())
            log(line)
    return model


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if argv and argv[0] in ('--eval', '-e'):
        from .evaluation import eval_main
        args = load_config('config.yaml')
        print(args)
        eval_main(args, argv[1:])
        return 0
    if argv and argv[0] == '--eval-match':
        from .evaluation import eval_match_main
        args = load_config('config.yaml')
        print(args)
        eval_match_main(args, argv[1:])
        return 0
    if argv and argv[0] == '--eval-rulebase':
        from .evaluation import eval_rulebase_main
        args = load_config('config.yaml')
        print(args)
        eval_rulebase_main(args, argv[1:])
        return 0
    if argv and argv[0] == '--eval-league':
        from .evaluation import eval_league_main
        args = load_config('config.yaml')
        print(args)
        eval_league_main(args, argv[1:])
        return 0
    if not argv or argv[0] not in ('--train', '-t'):
        print('usage: python -m handyrl_amd.main --train [config.yaml] | --eval MODEL_PATH [NUM_GAMES] [SLOTS] | '
              '--eval-match MODEL_A MODEL_B [NUM_GAMES] [SLOTS] | '
              '--eval-rulebase MODEL_PATH [NUM_GAMES] [SLOTS] | '
              '--eval-league MODEL_OR_DIR [MODEL_OR_DIR ...] [NUM_GAMES] [SLOTS]')
        return 1
    args = load_config(argv[1] if len(argv) > 1 else 'config.yaml')
    print(args)
    train_main(args)
    return 0


if __name__ == '__main__':
    sys.exit(main())
