"""Device-resident batched self-play and replay for the learner.

The reference plays one game per worker process, one batch-1 CPU inference
per player per ply (generation.py:20-88, model.py:43-53), ships each episode
as bz2(pickle) blocks over TCP/pipes (generation.py:79-86, worker.py), and a
batcher process rebuilds padded training windows on the CPU (train.py:33-133,
284-302).  Here thousands of games advance together on the GPU:

* ``TicTacToeBatch``  E concurrent games as tensors, rules of
  handyrl/envs/tictactoe.py:103-172 (black moves first, 8 winning lines,
  outcome +-1 / 0, 3-plane observation relative to the viewing player);
* ``DeviceGenerator`` one batched forward of the env network per ply for
  every live game, the reference's legal-action masking (-1e32,
  generation.py:49-52) and categorical sampling over the legal actions by
  Gumbel-max (the same distribution as ``random.choices(legal,
  weights=softmax(p[legal]))``, generation.py:53), episode returns as the
  reference's discounted sum (generation.py:73-77);
* ``DeviceReplay``    a ring buffer of episodes in HBM; ``sample`` draws
  windows with the reference Batcher's recency-weighted episode choice and
  uniform window start (train.py:284-293) and gathers them straight into the
  make_batch layout (train.py:109-133) the learner consumes -- no host copy,
  no pickling.

Training modes.  With turn_based_training=True and observation=False (the
stock configuration) only the player to move runs inference each ply and the
episode records one mover per ply.  With ``observation=True`` (every player
infers every ply, generation.py:35-46) or a simultaneous-move env
(``SIMULTANEOUS``, e.g. ``ParallelTicTacToeBatch``: every player moves every
ply, parallel_tictactoe.py:20-24) ``DeviceGenerator`` runs the per-player
ply instead: one forward over all P x E (player, game) views, per-player
recurrent state in HBM advanced for the players that inferred, the turn
players sampled, per-player records with the turn and observation masks;
``PlayerReplay`` gathers those into make_batch's per-player layout
(train.py:63-67), one random player per window for solo training
(turn_based_training=False, train.py:55-56).
"""

import contextlib
import ctypes
import functools

import numpy as np
import torch

from .util import map_r, bimap_r

__all__ = ['TicTacToeBatch', 'ParallelTicTacToeBatch', 'DeviceGenerator', 'DeviceReplay', 'PlayerReplay',
           'episodes_to_wire', 'player_episodes_to_wire', 'reference_uniforms', 'StreamGenerator', 'stream_uniforms',
           'philox4x32', 'PlayerStreamGenerator', 'stream_player_uniforms', 'stream_select_uniform']


class TicTacToeBatch:
    """E TicTacToe games on one device (handyrl/envs/tictactoe.py:72-172)."""

    A = 9
    P = 2
    MAX_PLIES = 9
    ALTERNATING = True   # the mover is ply % 2 in every live game
    OBS_SHAPE = (3, 3, 3)
    LINES = ((0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6))

    def __init__(self, E, device):
        self.E, self.device = E, device
        self.lines = torch.tensor(self.LINES, device=device)
        self.reset()

    def reset(self):
        """State tensors are allocated once and then reset and advanced in place, so a HIP graph captured
        over a ply (DeviceGenerator) keeps addressing them."""
        E, dev = self.E, self.device
        if not hasattr(self, 'board'):
            self.board = torch.zeros(E, 9, dtype=torch.int8, device=dev)     # +1 black, -1 white
            self.color = torch.ones(E, dtype=torch.int8, device=dev)          # side to move
            self.nmoves = torch.zeros(E, dtype=torch.int32, device=dev)
            self.winner = torch.zeros(E, dtype=torch.int8, device=dev)
        self.board.zero_()
        self.color.fill_(1)
        self.nmoves.zero_()
        self.winner.zero_()

    def turn(self):
        """Index of the player to move: 0 (black) on even plies."""
        return (self.nmoves % 2).long()

    def plies(self):
        return self.nmoves

    def terminal(self):
        return (self.winner != 0) | (self.nmoves >= 9)

    def legal(self):
        return self.board == 0

    def observation(self, player):
        """(E,3,3,3): [turn-view indicator, own stones, opponent stones] for `player` (E,) (tictactoe.py:157-168)."""
        turn_view = player == self.turn()
        me = torch.where(turn_view, self.color, -self.color).view(-1, 1)
        b = self.board
        planes = torch.stack([turn_view.view(-1, 1).expand(-1, 9), b == me, b == -me], dim=1)
        return planes.float().view(-1, 3, 3, 3)

    def step(self, action, active):
        """Play `action` (E,) for the side to move in every `active` game (tictactoe.py:103-118)."""
        rows = torch.arange(self.E, device=self.device)
        act = torch.where(active, action, torch.zeros_like(action))
        new = torch.where(active, self.color, self.board[rows, act])
        self.board[rows, act] = new
        sums = self.board.long()[:, self.lines].sum(-1)                   # (E, 8)
        won = active & (sums == 3 * self.color.long().view(-1, 1)).any(-1)
        self.winner.copy_(torch.where(won, self.color, self.winner))
        self.color.copy_(torch.where(active, -self.color, self.color))
        self.nmoves.add_(active.int())

    def outcome(self):
        """(E, 2) float: +1/-1 for the winner/loser, 0/0 for a draw (tictactoe.py:140-147)."""
        w = self.winner.float()
        return torch.stack([w, -w], dim=1)

    def turns_mask(self):
        """(E, P) bool: the players to move (turns(), environment.py:107-113): the side to move."""
        return torch.nn.functional.one_hot(self.turn(), self.P).bool()

    def state_tensors(self):
        """Every tensor of the game state (StreamGenerator saves and restores them around a graph capture)."""
        return [self.board, self.color, self.nmoves, self.winner]

    def reset_where(self, mask):
        """reset() for the games of ``mask`` (E,) bool only, in place (StreamGenerator: finished games restart)."""
        self.board.masked_fill_(mask.view(-1, 1), 0)
        self.color.masked_fill_(mask, 1)
        self.nmoves.masked_fill_(mask, 0)
        self.winner.masked_fill_(mask, 0)


class ParallelTicTacToeBatch(TicTacToeBatch):
    """E Parallel Tic-Tac-Toe games (handyrl/envs/parallel_tictactoe.py:13-61): both players choose a move every
    ply (turns() = both) and one of them, picked uniformly, is played with its own colour.  The reference's turn()
    returns an exception object, so observation(p) is the non-turn view for both p, and its colour never changes
    from black: both players see [zeros, white stones, black stones] (tictactoe.py:157-168)."""

    ALTERNATING = False
    SIMULTANEOUS = True

    def turns_mask(self):
        return torch.ones(self.E, self.P, dtype=torch.bool, device=self.device)

    def turn(self):
        return torch.zeros(self.E, dtype=torch.long, device=self.device)

    def observation(self, player):
        b = self.board
        planes = torch.stack([torch.zeros_like(b, dtype=torch.bool), b == -1, b == 1], dim=1)
        return planes.float().view(-1, 3, 3, 3)

    def step_players(self, actions, turns, active, u):
        """The played player: floor(u * P) of the E uniforms u (random.choice over the action dict's P keys,
        parallel_tictactoe.py:21); its action with its colour, player 0 black (parallel_tictactoe.py:25-35)."""
        rows = torch.arange(self.E, device=self.device)
        sel = torch.clamp((u * self.P).long(), max=self.P - 1)
        act = torch.where(active, actions[rows, sel], torch.zeros_like(sel))
        colour = torch.where(sel == 0, 1, -1).to(self.board.dtype)
        self.board[rows, act] = torch.where(active, colour, self.board[rows, act])
        sums = self.board.long()[:, self.lines].sum(-1)                   # (E, 8)
        won = active & (sums == 3 * colour.long().view(-1, 1)).any(-1)
        self.winner.copy_(torch.where(won, colour, self.winner))
        self.nmoves.add_(active.int())


def _leaves(x):
    """The tensors of a nested list / tuple / dict, in order."""
    out = []
    map_r(x, out.append)
    return out


def _alloc(spec, lead, device, dtype=torch.float32):
    """Zero tensors (*lead, *shape) for an observation spec: a shape tuple or {name: shape}."""
    if isinstance(spec, dict):
        return {k: torch.zeros(*lead, *v, device=device, dtype=dtype) for k, v in spec.items()}
    return torch.zeros(*lead, *spec, device=device, dtype=dtype)


def _stack_views(views, batch_first=False):
    """P views (each a tensor (E, ...) or {name: (E, ...)}) -> (P * E, ...) player-major, or (E, P, ...)."""
    def stack(xs):
        return torch.stack(xs, 1) if batch_first else torch.cat(xs, 0)
    if isinstance(views[0], dict):
        return {k: stack([v[k] for v in views]) for k in views[0]}
    return stack(views)


def reference_uniforms(seeds, Tm, P, simultaneous=False):
    """The random-stream values seeded reference games draw (generation.py:53, parallel_tictactoe.py:21): for
    game k, ``random.seed(seeds[k])`` then per ply each turn player's ``random.choices`` takes one ``random()``
    (players in order: the mover, ply % P, or every player of a simultaneous env) and a simultaneous env's step
    one ``random.choice`` over the P players.  Returns u (E, Tm, P) float64 and sel (E, Tm) int64 (None for
    alternating envs), for ``DeviceGenerator.generate(reference=...)``.  Draws past a game's end are unused."""
    import random as _random
    E = len(seeds)
    u = np.zeros((E, Tm, P), dtype=np.float64)
    sel = np.zeros((E, Tm), dtype=np.int64) if simultaneous else None
    for e, seed in enumerate(seeds):
        r = _random.Random(seed)
        for t in range(Tm):
            for p in (range(P) if simultaneous else (t % P,)):
                u[e, t, p] = r.random()
            if simultaneous:
                sel[e, t] = r.choice(list(range(P)))
    return u, sel


def sample_record_torch(st, logits, legal, value, active, player, reward):
    """The ply's sampling and recording tail as torch ops (generation.py:43-62): illegal logits masked by
    -1e32, Gumbel-max over the ply's uniforms st['U'][t] (the distribution of random.choices over the softmax
    of the legal logits), and slot t of the policy / action mask / action / value / turn / reward records
    (reset values for finished games).  Returns the sampled action per game."""
    E, t = logits.shape[0], st['t']
    m = torch.where(legal, 0.0, 1e32)                                  # generation.py:50-51
    p = logits - m
    u = st['U'].index_select(0, t).view(E, -1)
    a = torch.argmax(p - torch.log(-torch.log(u)), dim=-1)              # Gumbel-max = softmax over legal

    def record(buf, x, fill=0):
        live = active.view(-1, *([1] * (x.dim() - 1)))
        buf.index_copy_(1, t, torch.where(live, x, fill).to(buf.dtype).unsqueeze(1))
    record(st['policy'], p)
    record(st['amask'], m, 1e32)
    record(st['action'], a)
    record(st['value'], value.reshape(-1))
    record(st['turn'], player)
    if reward is not None:
        record(st['reward'], reward)
    return a


def sample_record_hip(st, logits, legal, value, active, player, reward):
    """sample_record_torch as ONE launch (csrc/hrl_selfplay.hip, one wave per game): the same fp32 operations,
    torch.argmax's tie order, the same records."""
    from . import _native
    E, A = logits.shape
    Tm = st['action'].shape[1]
    P = st['reward'].shape[2]
    logits = logits.float()
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    value = value.reshape(E).float().contiguous()
    legal, active = legal.contiguous(), active.contiguous()
    player = player.to(torch.long).contiguous()
    assert legal.shape == (E, A) and legal.dtype == torch.bool and active.shape == (E,) and player.shape == (E,)
    assert st['policy'].shape == (E, Tm, A) and st['U'].shape == (Tm, E, A)
    if reward is not None:
        reward = reward.to(torch.float64).contiguous()
        assert reward.shape == (E, P)
    a = torch.empty(E, dtype=torch.long, device=logits.device)
    _native.check(_native.load().hrl_selfplay_sample_record(
        _native.ptr(logits), logits.stride(0), _native.ptr(legal), _native.ptr(st['U']), _native.ptr(st['t']),
        _native.ptr(value), _native.ptr(active), _native.ptr(player), _native.ptr(reward), E, A, Tm, P,
        _native.ptr(a), _native.ptr(st['policy']), _native.ptr(st['amask']), _native.ptr(st['action']),
        _native.ptr(st['value']), _native.ptr(st['turn']), None if reward is None else _native.ptr(st['reward']),
        _native.stream_of(logits.device)), 'hrl_selfplay_sample_record')
    return a


def params_key(*nets):
    """The addresses of the nets' parameters and buffers.  A captured ply reads them where they live: the generators
    and evaluators recapture when this key changes (an in-place ``load_state_dict`` keeps it)."""
    return tuple(t.data_ptr() for n in nets for t in list(n.parameters()) + list(n.buffers()))


@contextlib.contextmanager
def eval_mode(*nets):
    """The nets in eval mode; their training modes are put back on the way out, also when the body raises."""
    was_training = [n.training for n in nets]
    try:
        for n in nets:
            n.eval()
        yield
    finally:
        for n, mode in zip(nets, was_training):
            n.train(mode)


def graph_wanted(device, graph):
    """``graph=None`` (default) or true on a CUDA device: the ply is replayed from captured graphs."""
    return torch.device(device).type == 'cuda' and (graph is None or bool(graph))


def capture_graphs(device, bodies, warm=None):
    """{key: CUDAGraph} of the ordered {key: callable} ``bodies``, captured in that order out of one shared pool.
    ``warm`` (default: every body once) runs first on a side stream, so that library workspaces exist before the
    capture.  What warm-up and capture did to the caller's buffers is the caller's to put back."""
    dev = torch.device(device)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        if warm is not None:
            warm()
        else:
            for body in bodies.values():
                body()
    torch.cuda.current_stream(dev).wait_stream(side)
    graphs, pool = {}, None
    for key, body in bodies.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=pool):
            body()
        pool = g.pool()
        graphs[key] = g
    return graphs


class DeviceGenerator:
    """Batched self-play of E games with one env-network forward per ply (generation.py:20-88).

    Recurrent nets (``init_hidden``, e.g. GeisterNet) keep one hidden state
    per game and player in HBM, starting from ``init_hidden`` zeros; each ply
    only the mover's state advances (generation.py:23-25, 38-41).  Rewards
    (``env.reward()``, e.g. Geister's -0.01 per ply) are recorded for both
    players every ply and turned into discounted returns in fp64 exactly as
    the reference's Python-float loop (generation.py:73-77).

    Every buffer of a call (episode tensors, hidden state, the ply's uniforms,
    the ply index as a device scalar) is allocated once and reset in place, and
    the ply body addresses the current ply through that device scalar.  So on
    a GPU the ply is captured ONCE per mover parity as a HIP graph (``graph``;
    default: on for CUDA envs whose mover is ply % P) and each ply is one
    graph replay instead of ≈100 small launches; the discounted-return loop is
    a third graph.  Eager and graph mode run the same ply function on the same
    uniforms (one (Tm, E, A) draw per call), so they give the same episodes.

    ``observation=True`` or a ``SIMULTANEOUS`` env selects the per-player ply
    (module doc; ``_ply_players``): the episode's records gain a player axis
    (E, Tm, P, ...) with ``tmask`` / ``omask``; its ply is one graph for every
    ply.  ``generate(reference=(u, sel))`` samples by the reference's inverse
    CDF instead of Gumbel-max: u (E, Tm, P) are the ``random()`` values each
    turn player's ``random.choices`` draws and sel (E, Tm) the simultaneous
    env's played-player uniforms (``reference_uniforms``), so seeded reference
    games replay move for move.

    ``fused_game=True`` (opt-in; TicTacToe with a ``nn.BoardInference`` net): on a CUDA env a call is ONE
    ``hrl_board_selfplay`` launch (csrc/hrl_boardplay.hip) for all nine plies of all E games -- observation,
    forward, sampling, records and rules, the games resident in LDS -- on the same buffers, the env's own state
    tensors and the same uniforms instead of the ply loop; no graph is captured and the episodes are the ply loop's
    bit for bit.  The env must be exactly a ``TicTacToeBatch`` in the mover-only mode and the net a
    ``BoardInference``; a member of a ``board_inference_group`` is accepted and plays from its row of the group's
    buffer.  Anything else raises ``ValueError`` here.  On a CPU env the option runs the ordinary ply loop.
    """

    def __init__(self, env_batch, net, gamma=0.8, check_every=16, graph=None, observation=False, per_player=None,
                 fused_game=False):
        self.env = env_batch
        self.net = net
        self.gamma = gamma
        self.check_every = check_every
        self.graph = graph
        self.observation = bool(observation)
        # per_player=True also for a mover-only alternating game whose batches need per-player records (solo)
        self.per_player = (self.observation or getattr(env_batch, 'SIMULTANEOUS', False) if per_player is None
                           else bool(per_player) or self.observation or getattr(env_batch, 'SIMULTANEOUS', False))
        self.fused_game = bool(fused_game)
        if self.fused_game:
            from .nn import BoardInference
            if type(env_batch) is not TicTacToeBatch:
                raise ValueError('fused_game: the one-launch game plays the rules of TicTacToeBatch itself, not %s'
                                 % type(env_batch).__name__)
            if self.per_player:
                raise ValueError('fused_game: the one-launch game is the mover-only ply (no observation, no '
                                 'per-player records)')
            if not isinstance(net, BoardInference):
                raise ValueError('fused_game: the one-launch game runs the forward of nn.BoardInference, not %s'
                                 % type(net).__name__)
        self._st = None

    def _use_graph(self):
        dev = torch.device(self.env.device)
        if self.graph is None:
            return dev.type == 'cuda' and (self.per_player or getattr(self.env, 'ALTERNATING', False))
        return bool(self.graph) and dev.type == 'cuda'

    def _state(self):
        """The call's buffers, allocated once per (generator, net)."""
        # a captured ply reads the net's parameters and buffers where they live: recapture if any moved
        key = params_key(self.net)
        if self._st is not None and self._st['net'] is self.net and self._st['key'] == key:
            return self._st
        env, E, dev = self.env, self.env.E, self.env.device
        Tm, A, P = env.MAX_PLIES, env.A, env.P
        st = {'net': self.net, 'key': key, 'graphs': None,
              'obs': _alloc(env.OBS_SHAPE, (E, Tm), dev),
              'policy': torch.zeros(E, Tm, A, device=dev),
              'amask': torch.full((E, Tm, A), 1e32, device=dev),
              'action': torch.zeros(E, Tm, dtype=torch.long, device=dev),
              'value': torch.zeros(E, Tm, device=dev),
              'turn': torch.zeros(E, Tm, dtype=torch.long, device=dev),
              'reward': torch.zeros(E, Tm, P, device=dev, dtype=torch.float64),  # Python floats in the reference
              'ret': torch.zeros(E, Tm, P, device=dev),
              'U': torch.empty(Tm, E, A, device=dev),
              't': torch.zeros(1, dtype=torch.long, device=dev),
              'rows': torch.arange(E, device=dev),
              'hidden': None, 'obs_dev': torch.device(dev).type}
        if self.per_player:
            # records with a player axis; the uniforms (Tm, E, P, A) for Gumbel-max, (E, Tm, P) / (E, Tm) for the
            # reference sampler; the state (P, E, ...): the (player, game) rows of one forward are its view
            st.update(obs=_alloc(env.OBS_SHAPE, (E, Tm, P), dev),
                      policy=torch.zeros(E, Tm, P, A, device=dev),
                      amask=torch.full((E, Tm, P, A), 1e32, device=dev),
                      action=torch.zeros(E, Tm, P, dtype=torch.long, device=dev),
                      value=torch.zeros(E, Tm, P, device=dev),
                      tmask=torch.zeros(E, Tm, P, dtype=torch.bool, device=dev),
                      omask=torch.zeros(E, Tm, P, dtype=torch.bool, device=dev),
                      U=torch.empty(Tm, E, P, A, device=dev),
                      Uref=torch.zeros(E, Tm, P, dtype=torch.float64, device=dev),
                      Usel=torch.empty(Tm, E, device=dev),
                      ref_mode=False, rank=False,
                      players=torch.arange(P, device=dev).view(P, 1).expand(P, E).contiguous(), pmajor=True)
            st['flat_state'] = False
            if (self.observation and hasattr(self.net, 'inference_hidden') and hasattr(self.net, 'inference_session')
                    and torch.device(dev).type == 'cuda'):
                # every player infers every ply: the net's own stacked layout over the P*E rows, advanced in place
                # inside its inference session (GeisterNet), leaves (P*E, ...) player-major
                st['hidden'] = map_r(self.net.inference_hidden(P * E, 1, dev), lambda h: h[0])
                st['flat_state'] = True
            elif hasattr(self.net, 'init_hidden'):
                st['hidden'] = map_r(self.net.init_hidden([P, E]), lambda h: h.to(dev).contiguous())
            self._st = st
            return st
        st['pmajor'] = False   # state leaves (E, P, ...) as init_hidden gives them
        if hasattr(self.net, 'inference_hidden') and torch.device(dev).type == 'cuda':
            st['hidden'] = self.net.inference_hidden(E, P, dev)   # leaves (P, E, ...), the net's own layout
            st['pmajor'] = True
        elif hasattr(self.net, 'init_hidden'):
            st['hidden'] = map_r(self.net.init_hidden([E, P]), lambda h: h.to(dev).contiguous())
        self._st = st
        return st

    def _reset(self, st, generator, draw=True):
        self.env.reset()
        map_r(st['obs'], lambda b: b.zero_())
        for k in ('policy', 'action', 'value', 'turn', 'reward', 'ret') + (('tmask', 'omask') if self.per_player
                                                                           else ()):
            st[k].zero_()
        st['amask'].fill_(1e32)
        if st['hidden'] is not None:
            map_r(st['hidden'], lambda h: h.zero_())
        if draw:
            torch.rand(st['U'].shape, out=st['U'], generator=generator, device=st['U'].device)
            st['U'].clamp_(1e-20, 1.0)
            if self.per_player:
                torch.rand(st['Usel'].shape, out=st['Usel'], generator=generator, device=st['Usel'].device)
        st['t'].zero_()

    def _ply_players(self, st):
        """The per-player ply (generation.py:35-62 with observation, or every player a turn player): every
        (player, game) view in one forward -- the players that infer are the turn players, or all with
        ``observation`` --, their values / observations recorded and their state advanced, the turn players'
        policies masked and sampled, then the env steps on the turn players' actions."""
        env, E, P, A = self.env, self.env.E, self.env.P, self.env.A
        t = st['t']
        hidden = st['hidden']
        # a snapshot: an env's active() may be state its step updates in place (GeisterBatch.live), and the
        # reward after the step is recorded for the games that were live before it
        active = (env.active() if hasattr(env, 'active') else ~env.terminal()).clone()
        live = active.view(E, 1)
        turns = (env.turns_mask() if hasattr(env, 'turns_mask') else
                 torch.nn.functional.one_hot(env.turn().long(), P).bool()) & live          # (E, P)
        infer = live.expand(E, P) if self.observation else turns
        views = None
        if hasattr(env, 'observe_players_record'):
            # the env builds every view and records slot t of the (game, player) pairs of `infer` in one launch
            o = env.observe_players_record(st['obs'], t, infer)                           # (P * E, ...)
        else:
            views = [env.observation(st['players'][p]) for p in range(P)]
            o = _stack_views(views)                                                       # (P * E, ...)
        h_in = (None if hidden is None else hidden if st['flat_state'] else
                map_r(hidden, lambda h: h.view(P * E, *h.shape[2:])))
        out = self.net(o, h_in)
        logits = out['policy'].float().view(P, E, A).transpose(0, 1)                   # (E, P, A)
        value = out['value'].float().reshape(P, E).t()                                  # (E, P)
        legal = (env.legal_players() if hasattr(env, 'legal_players') else
                 env.legal().view(E, 1, A).expand(E, P, A))
        m = torch.where(legal, 0.0, 1e32)                                                 # generation.py:50-51
        p = logits - m
        # Gumbel-max over the legal logits (softmax sampling), or the reference's inverse CDF of random.choices:
        # bisect(cumsum(softmax(p[legal])), u * total), fp64 here (the reference's fp32 sums decide otherwise only
        # when u falls within their rounding of a boundary)
        if not st['ref_mode']:
            g = st['U'].index_select(0, t).view(E, P, A)
            a = torch.argmax(p - torch.log(-torch.log(g)), dim=-1)
        else:
            # the reference's legal_actions order: ascending labels, or the env's own (legal_rank: Geister's pieces)
            base = (env.legal_rank().view(E, 1, A) if st['rank'] else
                    torch.arange(A, device=p.device).view(1, 1, A)).expand(E, P, A)
            order = torch.argsort(torch.where(legal, base, 1 << 30), dim=-1, stable=True)    # legal ones first
            lo = torch.gather(legal, -1, order)
            pd = torch.where(lo, torch.gather(p, -1, order).double(), float('-inf'))
            w = torch.exp(pd - pd.max(-1, keepdim=True).values)
            cum = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
            x = st['Uref'].index_select(1, t).view(E, P, 1) * cum[..., -1:]
            k = ((cum <= x) & lo).sum(-1, keepdim=True)                                  # bisect_right over legal
            k = torch.minimum(k, lo.sum(-1, keepdim=True) - 1).clamp(min=0)
            a = torch.gather(order, -1, k).squeeze(-1)                                   # legal entries lead

        def record(buf, x, mask, fill=0):
            keep = mask.view(*mask.shape, *([1] * (x.dim() - mask.dim())))
            buf.index_copy_(1, t, torch.where(keep, x, fill).to(buf.dtype).unsqueeze(1))
        if views is not None:
            views_e = _stack_views(views, batch_first=True)                               # (E, P, ...)
            bimap_r(st['obs'], views_e, lambda b, v: record(b, v, infer))
        record(st['value'], value, infer)
        record(st['policy'], p, turns)
        record(st['amask'], m, turns, 1e32)
        record(st['action'], a, turns)
        record(st['tmask'], turns, turns)
        record(st['omask'], infer, infer)
        if hidden is not None and st['flat_state']:
            # the session advanced every (player, game) row in place -- all of them inferred (observation); a
            # finished game's rows moved too, but nothing reads them again.  Without the in-place form: a copy
            dst, src = _leaves(hidden), _leaves(out['hidden'])
            if not all(d.data_ptr() == x.data_ptr() and d.stride() == x.stride() for d, x in zip(dst, src)):
                for d, x in zip(dst, src):
                    d.copy_(x)
        elif hidden is not None:                                   # only the players that inferred advance
            keep = infer.t().contiguous()                          # (P, E)

            def advance(h, nh):
                nh = nh.view(h.shape)
                h.copy_(torch.where(keep.view(P, E, *([1] * (h.dim() - 2))), nh, h))
            bimap_r(hidden, out['hidden'], advance)
        if getattr(env, 'SIMULTANEOUS', False):
            env.step_players(a, turns, active, st['Usel'].index_select(0, t).view(E))
        else:
            rows = torch.arange(E, device=a.device)
            env.step(a[rows, env.turn().long()], active)
        if hasattr(env, 'reward'):
            r = env.reward().to(st['reward'].dtype)
            st['reward'].index_copy_(1, t, torch.where(live, r, 0).unsqueeze(1))
        t.add_(1)

    def _ply(self, st, mover):
        """One ply for every game at ply index st['t'] (a device scalar, advanced here); ``mover``: the
        player index every live game moves with (ALTERNATING envs), or None."""
        if self.per_player:
            return self._ply_players(st)
        env, E = self.env, self.env.E
        t = st['t']
        hidden = st['hidden']
        active = env.active() if hasattr(env, 'active') else ~env.terminal()
        player = env.turn()
        # envs with a GPU observation kernel record the view into slot t in the same launch
        obs_recorded = st['obs_dev'] == 'cuda' and hasattr(env, 'observation_record')
        o = env.observation_record(player, st['obs'], t, active) if obs_recorded else env.observation(player)
        # envs whose mover is ply % P in every live game (TicTacToe, Geister): the mover's state is a view
        if hidden is None:
            h_in = None
        elif mover is not None:
            h_in = map_r(hidden, (lambda h: h[mover]) if st['pmajor'] else (lambda h: h[:, mover]))
        elif st['pmajor']:
            h_in = map_r(hidden, lambda h: h[player, st['rows']])
        else:
            h_in = map_r(hidden, lambda h: h[st['rows'], player])
        out = self.net(o, h_in)
        # the reference reads the reward after env.step (generation.py:59-65); an env whose reward does not
        # depend on the state (REWARD_STATELESS, e.g. Geister's -0.01 per ply) has it recorded by the
        # sampling launch, any other env's after its step below
        has_reward = hasattr(env, 'reward')
        early = has_reward and getattr(env, 'REWARD_STATELESS', False)
        reward = env.reward() if early else None
        # slot t of every record is written once per call, so a finished game keeps the reset value
        def record(buf, x, fill=0):
            live = active.view(-1, *([1] * (x.dim() - 1)))
            buf.index_copy_(1, t, torch.where(live, x, fill).to(buf.dtype).unsqueeze(1))
        if not obs_recorded:
            bimap_r(st['obs'], o, record)
        sample = sample_record_hip if st['obs_dev'] == 'cuda' else sample_record_torch
        a = sample(st, out['policy'], env.legal(), out['value'], active, player, reward)
        if hidden is not None and mover is not None and st['obs_dev'] == 'cuda':
            dst = [h[mover] if st['pmajor'] else h[:, mover] for h in _leaves(hidden)]
            src = _leaves(out['hidden'])
            # a net that advanced its stacked state in place (GeisterNet in an in-place session) left nothing to
            # copy: finished games' states moved too, but nothing reads them again (their records are reset
            # values); otherwise one HIP launch for every state tensor instead of a where + copy per tensor
            if not all(d.data_ptr() == x.data_ptr() and d.stride() == x.stride() for d, x in zip(dst, src)):
                from .nn import masked_rows_copy_
                masked_rows_copy_(dst, src, active.contiguous())
        elif hidden is not None:
            def advance(h, nh):
                live = active.view(-1, *([1] * (nh.dim() - 1)))
                if st['pmajor']:
                    h[player, st['rows']] = torch.where(live, nh, h[player, st['rows']])
                elif mover is not None:
                    h[:, mover].copy_(torch.where(live, nh, h[:, mover]))
                else:
                    h[st['rows'], player] = torch.where(live, nh, h[st['rows'], player])
            bimap_r(hidden, out['hidden'], advance)
        env.step(a, active)
        if has_reward and not early:
            r = env.reward().to(st['reward'].dtype)
            st['reward'].index_copy_(1, t, torch.where(active.view(-1, 1), r, 0).unsqueeze(1))
        t.add_(1)

    def _returns(self, st):
        """Discounted returns per player, fp64 like the reference's Python floats (generation.py:73-77)."""
        reward, ret = st['reward'], st['ret']
        acc = torch.zeros_like(reward[:, 0])
        for t in range(reward.shape[1] - 1, -1, -1):
            acc = reward[:, t] + self.gamma * acc
            ret[:, t].copy_(acc)

    def _capture(self, st, keys):
        """Graphs of the ply (one per mover key) and of the return loop; warm-up plies run first on a side
        stream (library workspaces), then the state is reset."""
        bodies = {k: functools.partial(self._ply, st, k) for k in keys}
        bodies['returns'] = functools.partial(self._returns, st)
        st['graphs'] = capture_graphs(self.env.device, bodies)
        self._reset(st, None, draw=False)   # the call's uniforms stay as drawn

    @torch.no_grad()
    def generate(self, generator=None, reference=None):
        """One batch of E games; ``reference`` (per-player mode): (u, sel) from ``reference_uniforms``."""
        alternating = getattr(self.env, 'ALTERNATING', False) and not self.per_player
        st = self._state()
        if reference is not None and not self.per_player:
            raise ValueError('the reference sampler is the per-player ply\'s (observation or simultaneous envs)')
        # per-call weight preparation (GeisterNet); its own stacked state is advanced in place by the net (the
        # per-player ply too when every player infers; otherwise it runs the net's ordinary forward).  A wrapper
        # without state (nn.BoardInference) is entered in every mode
        session = (getattr(self.net, 'inference_session', None)
                   if (not self.per_player or st.get('flat_state') or getattr(self.net, 'stateless_session', False))
                   else None)
        with eval_mode(self.net), \
                session(inplace_state=st['pmajor']) if session is not None else contextlib.nullcontext():
            if self.fused_game and st['obs_dev'] == 'cuda':
                return self._generate_fused(st, generator)
            return self._generate(st, generator, alternating, reference)

    def _generate_fused(self, st, generator):
        """``_generate`` with the ply loop as one launch (``fused_game``), inside the net's inference session.  The
        kernel stores every slot of every record, so of ``_reset`` only the env's and the draw of the uniforms run
        (reward / ret stay the zeros they were allocated as: TicTacToe has no per-ply reward)."""
        from . import _native
        env, net = self.env, self.net
        E, Tm = env.E, env.MAX_PLIES
        env.reset()
        torch.rand(st['U'].shape, out=st['U'], generator=generator, device=st['U'].device)
        st['U'].clamp_(1e-20, 1.0)
        dev = st['U'].device
        for x in env.state_tensors() + [st['obs'], st['policy'], st['amask'], st['action'], st['value'], st['turn']]:
            assert x.is_contiguous() and x.device == dev
        assert (env.board.dtype, env.color.dtype, env.nmoves.dtype, env.winner.dtype) == \
            (torch.int8, torch.int8, torch.int32, torch.int8) and env.board.shape == (E, 9)
        _native.check(_native.load().hrl_board_selfplay(
            _native.ptr(net.pack(dev)), net.layers, E, Tm, 0, Tm, _native.ptr(st['U']), _native.ptr(env.board),
            _native.ptr(env.color), _native.ptr(env.nmoves), _native.ptr(env.winner), _native.ptr(st['obs']),
            _native.ptr(st['policy']), _native.ptr(st['amask']), _native.ptr(st['action']), _native.ptr(st['value']),
            _native.ptr(st['turn']), _native.stream_of(dev)), 'hrl_board_selfplay')
        out = {'observation': st['obs'].clone()}
        for key, k in (('policy', 'policy'), ('action_mask', 'amask'), ('action', 'action'), ('value', 'value'),
                       ('turn', 'turn'), ('return', 'ret')):
            out[key] = st[k].clone()
        out.update(length=env.plies().long(), outcome=env.outcome(), reward=st['reward'].float())
        return out

    def _generate(self, st, generator, alternating, reference=None):
        env = self.env
        Tm, P = env.MAX_PLIES, env.P
        if self.per_player:
            # the sampler is part of the captured ply: a change of sampler recaptures it; an env whose
            # legal_actions order is not ascending keeps what gives it (Geister: piece indices)
            ref_mode = reference is not None
            if ref_mode != st['ref_mode']:
                st['ref_mode'], st['graphs'] = ref_mode, None
            st['rank'] = ref_mode and hasattr(env, 'legal_rank')
            if st['rank'] and getattr(env, 'pidx', None) is None:
                env.piece_order(True)
                st['graphs'] = None
        self._reset(st, generator)
        if self.per_player:
            if reference is not None:
                u, sel = reference
                st['Uref'].copy_(torch.as_tensor(u, dtype=torch.float64))
                if sel is not None:   # the played player p is floor(Usel * P): the middle of its interval
                    st['Usel'].copy_(((torch.as_tensor(sel, dtype=torch.float64) + 0.5) / P).t().float())
        graphs = None
        if self._use_graph():
            if st['graphs'] is None:
                self._capture(st, list(range(P)) if alternating else [None])
            graphs = st['graphs']
        for t in range(Tm):
            if t and self.check_every and t % self.check_every == 0 and bool(env.terminal().all()):
                break
            mover = t % P if alternating else None
            if graphs is not None:
                graphs[mover].replay()
            else:
                self._ply(st, mover)
        if hasattr(env, 'reward'):
            if graphs is not None:
                graphs['returns'].replay()
            else:
                self._returns(st)
        out = {'observation': map_r(st['obs'], lambda b: b.clone())}
        for key, k in (('policy', 'policy'), ('action_mask', 'amask'), ('action', 'action'), ('value', 'value'),
                       ('turn', 'turn'), ('return', 'ret')) + ((('tmask', 'tmask'), ('omask', 'omask'))
                                                            if self.per_player else ()):
            out[key] = st[k].clone()
        out.update(length=env.plies().long(), outcome=env.outcome(), reward=st['reward'].float())
        return out


# ---- streaming self-play: every slot at its own ply, finished games restart in place (StreamGenerator) ----

# True: on a GPU the streaming ply's tail and harvest are the launches of hrl_selfplay_sample_record_stream,
# hrl_geister_observation_record_at and hrl_selfplay_harvest (include/hrl_env.h) instead of the torch ops below,
# which stay as the CPU path and as the formulation the kernels are tested against (bit-identical).
FUSED_STREAM = True

_M32 = 0xffffffff
_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) in host integer arithmetic: ``counter`` four and ``key`` two 32-bit
    words (ints or broadcastable integer arrays); returns the four output words as uint64 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(_M32) for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & np.uint64(_M32) for x in key]
    m0, m1 = (np.uint64(m) for m in _PHILOX_M)
    w0, w1 = (np.uint64(w) for w in _PHILOX_W)
    mask, s32 = np.uint64(_M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + w0) & mask, (k[1] + w1) & mask]
    return c


def stream_uniforms(seed, game, ply, A):
    """The uniforms game number ``game`` samples its ply ``ply`` with, one per action label: (A,) float32 (``game``
    / ``ply`` may be integer arrays: (..., A)).  The public sampling rule of the streaming generator, which
    hrl_selfplay_sample_record_stream reproduces bit for bit: Philox4x32-10 with key (seed & 0xffffffff,
    seed >> 32) and counter (game & 0xffffffff, game >> 32, ply, a // 4); label a takes output word a % 4, and
    u = ((x >> 9) + 0.5) * 2**-23, exact in fp32 and inside [2**-24, 1 - 2**-24] (no 0, no 1, no clamp).  A game's
    uniforms depend on (seed, game, ply, label) only -- not on the slot or the moment it is played."""
    seed = int(seed) & 0xffffffffffffffff
    game = np.asarray(game, dtype=np.int64).astype(np.uint64)[..., None]
    ply = np.asarray(ply, dtype=np.int64).astype(np.uint64)[..., None]
    a = np.arange(A, dtype=np.uint64)
    out = philox4x32((game, game >> np.uint64(32), ply, a >> np.uint64(2)), (seed & _M32, seed >> 32))
    word = np.broadcast_to(a & np.uint64(3), np.broadcast_shapes(out[0].shape, a.shape))
    x = np.select([word == 0, word == 1, word == 2], out[:3], out[3])
    return ((x >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def stream_uniforms_torch(seed, game, ply, A):
    """``stream_uniforms`` for E games as torch ops: game, ply (E,) int64 -> (E, A) float32.  32-bit words held in
    int64; a 32 x 32 product wraps in int64 to the right 64 bits."""
    seed = int(seed) & 0xffffffffffffffff
    E = game.shape[0]
    a = torch.arange(A, device=game.device)
    c0 = (game & _M32).view(E, 1).expand(E, A)
    c1 = ((game >> 32) & _M32).view(E, 1).expand(E, A)
    c2 = (ply & _M32).view(E, 1).expand(E, A)
    c3 = (a >> 2).view(1, A).expand(E, A)
    k0, k1 = seed & _M32, seed >> 32
    for _ in range(10):
        p0, p1 = c0 * _PHILOX_M[0], c2 * _PHILOX_M[1]
        c0, c1, c2, c3 = ((p1 >> 32) & _M32) ^ c1 ^ k0, p1 & _M32, ((p0 >> 32) & _M32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W[0]) & _M32, (k1 + _PHILOX_W[1]) & _M32
    w = (a & 3).view(1, A)
    x = torch.where(w == 0, c0, torch.where(w == 1, c1, torch.where(w == 2, c2, c3)))
    return ((x >> 9).float() + 0.5) * (2.0 ** -23)


PLAYER_W3, SELECT_W3 = 0x40000000, 0x80000000


def _player_blocks(P, A):
    """ceil(A / 4), the Philox calls per player; the players' range of the last counter word must end below
    ``SELECT_W3 - PLAYER_W3``."""
    blocks = (int(A) + 3) // 4
    if int(P) * blocks >= 0x40000000:
        raise ValueError('P * ceil(A / 4) = %d leaves the counter range of the player uniforms (< 0x40000000)'
                         % (int(P) * blocks))
    return blocks


def _words_to_uniform(out, word):
    x = np.select([word == 0, word == 1, word == 2], out[:3], out[3])
    return ((x >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def stream_player_uniforms(seed, game, ply, P, A):
    """The uniforms the players of game number ``game`` sample ply ``ply`` with in a simultaneous-move env: (P, A)
    float32 (``game`` / ``ply`` integer arrays: (..., P, A)).  The public rule of ``PlayerStreamGenerator``, which
    hrl_selfplay_sample_record_players_stream reproduces bit for bit: ``stream_uniforms``' generator, key and float
    mapping with the counter (game & 0xffffffff, game >> 32, ply, w3), w3 = 0x40000000 + p * ceil(A / 4) + a // 4
    for player p and label a, output word a % 4.

    The last counter word w3 keeps apart what one (seed, game, ply) draws -- ``main`` gives the env and the generator
    the same seed: the mover rule (``stream_uniforms``) takes a // 4, below 0x40000000; the Hungry Geese picks
    (``geese.geese_picks``) 0 and 1; these player uniforms [0x40000000, 0x80000000); ``stream_select_uniform``
    0x80000000; ``evaluation.eval_pick`` 0xffffffff.  Without the offset a game's food placement and its geese's action
    noise would be the same random words.  ``ValueError`` when P * ceil(A / 4) >= 0x40000000."""
    blocks = _player_blocks(P, A)
    seed = int(seed) & 0xffffffffffffffff
    game = np.asarray(game, dtype=np.int64).astype(np.uint64)[..., None, None]
    ply = np.asarray(ply, dtype=np.int64).astype(np.uint64)[..., None, None]
    a = np.arange(A, dtype=np.uint64).reshape(1, A)
    p = np.arange(P, dtype=np.uint64).reshape(P, 1)
    w3 = np.uint64(PLAYER_W3) + p * np.uint64(blocks) + (a >> np.uint64(2))
    out = philox4x32((game, game >> np.uint64(32), ply, w3), (seed & _M32, seed >> 32))
    return _words_to_uniform(out, np.broadcast_to(a & np.uint64(3), out[0].shape))


def stream_select_uniform(seed, game, ply):
    """The uniform ``u`` a simultaneous env's ``step_players`` takes at ply ``ply`` of game number ``game`` (float32
    scalar; arrays: the broadcast shape): the rule of ``stream_player_uniforms`` with w3 = 0x80000000 and output word
    0.  ParallelTicTacToe plays player floor(u * P); Hungry Geese ignores it."""
    seed = int(seed) & 0xffffffffffffffff
    game = np.asarray(game, dtype=np.int64).astype(np.uint64)
    ply = np.asarray(ply, dtype=np.int64).astype(np.uint64)
    out = philox4x32((game, game >> np.uint64(32), ply, SELECT_W3), (seed & _M32, seed >> 32))
    return ((out[0] >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def _philox_torch(seed, c0, c1, c2, c3):
    """Philox4x32-10 on int64 tensors holding 32-bit words (a 32 x 32 product wraps in int64 to the right 64 bits)."""
    k0, k1 = seed & _M32, seed >> 32
    for _ in range(10):
        p0, p1 = c0 * _PHILOX_M[0], c2 * _PHILOX_M[1]
        c0, c1, c2, c3 = ((p1 >> 32) & _M32) ^ c1 ^ k0, p1 & _M32, ((p0 >> 32) & _M32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W[0]) & _M32, (k1 + _PHILOX_W[1]) & _M32
    return c0, c1, c2, c3


def stream_player_uniforms_torch(seed, game, ply, P, A):
    """``stream_player_uniforms`` for E games as torch ops: game, ply (E,) int64 -> (E, P, A) float32."""
    blocks = _player_blocks(P, A)
    seed = int(seed) & 0xffffffffffffffff
    E, dev = game.shape[0], game.device
    a = torch.arange(A, device=dev).view(1, 1, A)
    p = torch.arange(P, device=dev).view(1, P, 1)
    shape = (E, P, A)
    c = _philox_torch(seed, (game & _M32).view(E, 1, 1).expand(shape), ((game >> 32) & _M32).view(E, 1, 1).expand(shape),
                      (ply & _M32).view(E, 1, 1).expand(shape), (PLAYER_W3 + p * blocks + (a >> 2)).expand(shape))
    w = a & 3
    x = torch.where(w == 0, c[0], torch.where(w == 1, c[1], torch.where(w == 2, c[2], c[3])))
    return ((x >> 9).float() + 0.5) * (2.0 ** -23)


def stream_select_uniform_torch(seed, game, ply):
    """``stream_select_uniform`` for E games as torch ops: game, ply (E,) int64 -> (E,) float32."""
    seed = int(seed) & 0xffffffffffffffff
    c = _philox_torch(seed, game & _M32, (game >> 32) & _M32, ply & _M32, torch.full_like(game, SELECT_W3))
    return ((c[0] >> 9).float() + 0.5) * (2.0 ** -23)


def _record_at(buf, rows, ply, x, active):
    """Slot (e, ply[e]) of ``buf`` (E, Tm, ...) becomes x[e] where active[e]; an inactive game stores nothing (its
    ply may equal Tm: the index is clamped and the old value written back)."""
    idx = ply.clamp(0, buf.shape[1] - 1)
    live = active.view(-1, *([1] * (x.dim() - 1)))
    buf[rows, idx] = torch.where(live, x.to(buf.dtype), buf[rows, idx])


def sample_record_stream_torch(st, seed, logits, legal, value, active, player, reward):
    """The streaming ply's sampling and recording tail as torch ops: ``sample_record_torch`` with the uniforms of
    ``stream_uniforms`` for (st['game'][e], st['ply'][e]) and the records at slot (e, st['ply'][e]); an inactive
    game gets action 0 and no record store."""
    rows, ply = st['rows'], st['ply']
    m = torch.where(legal, 0.0, 1e32)
    p = logits.float() - m
    u = stream_uniforms_torch(seed, st['game'], ply, logits.shape[1])
    a = torch.argmax(p - torch.log(-torch.log(u)), dim=-1)
    a = torch.where(active, a, torch.zeros_like(a))
    _record_at(st['policy'], rows, ply, p, active)
    _record_at(st['amask'], rows, ply, m, active)
    _record_at(st['action'], rows, ply, a, active)
    _record_at(st['value'], rows, ply, value.reshape(-1).float(), active)
    _record_at(st['turn'], rows, ply, player, active)
    if reward is not None:
        _record_at(st['reward'], rows, ply, reward, active)
    return a


def sample_record_stream_hip(st, seed, logits, legal, value, active, player, reward):
    """sample_record_stream_torch as ONE launch (hrl_selfplay_sample_record_stream, one wave per game)."""
    from . import _native
    E, A = logits.shape
    Tm = st['action'].shape[1]
    P = st['reward'].shape[2]
    logits = logits.float()
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    value = value.reshape(E).float().contiguous()
    legal, active = legal.contiguous(), active.contiguous()
    player = player.to(torch.long).contiguous()
    assert legal.shape == (E, A) and legal.dtype == torch.bool and active.shape == (E,) and player.shape == (E,)
    assert active.dtype == torch.bool and st['policy'].shape == (E, Tm, A)
    for k in ('game', 'ply'):
        assert st[k].shape == (E,) and st[k].dtype == torch.long and st[k].is_contiguous()
    if reward is not None:
        reward = reward.to(torch.float64).contiguous()
        assert reward.shape == (E, P)
    a = torch.empty(E, dtype=torch.long, device=logits.device)
    _native.check(_native.load().hrl_selfplay_sample_record_stream(
        _native.ptr(logits), logits.stride(0), _native.ptr(legal), int(seed) & 0xffffffffffffffff,
        _native.ptr(st['game']), _native.ptr(st['ply']), _native.ptr(value), _native.ptr(active), _native.ptr(player),
        _native.ptr(reward), E, A, Tm, P, _native.ptr(a), _native.ptr(st['policy']), _native.ptr(st['amask']),
        _native.ptr(st['action']), _native.ptr(st['value']), _native.ptr(st['turn']),
        None if reward is None else _native.ptr(st['reward']), _native.stream_of(logits.device)),
        'hrl_selfplay_sample_record_stream')
    return a


def _harvest_torch(keys, st, done, outcome, gamma, replay, ring_game, has_reward):
    """The streaming generators' harvest as torch ops, without a host read (graph-capturable): the episodes of the
    ``done`` slots go to the ring rows (ring_ptr + r) mod N, r = the number of done slots below, and their slots
    restart.  Formed over the W = min(E, N) rows the call can write: row k of them is written when k < c (the done
    count), by the last done slot that claims it.  ``keys``: the per-ply records besides obs, policy and amask;
    an observation leaf is converted as ``src.to(dst.dtype)``."""
    E, N, Tm = done.shape[0], replay.N, replay.Tm
    dev = done.device
    if dev.type == 'cpu' and not bool(done.any()):
        return      # nothing changes; on the CPU the look costs nothing (a GPU call must not read the device)
    state, ply, game = st['state'], st['ply'], st['game']
    W = min(E, N)
    d = done.long()
    r = torch.cumsum(d, 0) - d
    c = d.sum()
    e_idx = st['rows']
    order = torch.empty_like(e_idx).scatter_(0, torch.where(done, r, c + (e_idx - r)), e_idx)   # done slots first
    k = torch.arange(W, device=dev)
    written = k < c
    last = k + N * torch.div(torch.clamp(c - 1 - k, min=0), N, rounding_mode='floor')
    slot = order[torch.where(written, last, k)]
    rows = (state[0] + k) % N
    L = ply[slot].clamp(0, Tm)
    valid = torch.arange(Tm, device=dev).view(1, Tm) < L.view(W, 1)

    def put(dst, new):
        w = written.view(W, *([1] * (new.dim() - 1)))
        dst.index_copy_(0, rows, torch.where(w, new.to(dst.dtype), dst.index_select(0, rows)))

    def plies(src, fill=0):
        v = valid.view(W, Tm, *([1] * (src.dim() - 2)))
        return torch.where(v, src.index_select(0, slot), fill)
    bimap_r(replay.obs, st['obs'], lambda dst, src: put(dst, plies(src)))
    put(replay.policy, plies(st['policy']))
    put(replay.amask, plies(st['amask'], 1e32))
    for key in keys:
        put(getattr(replay, key), plies(st[key]))
    rew = plies(st['reward']) if has_reward else torch.zeros(W, Tm, replay.P, dtype=torch.float64, device=dev)
    put(replay.reward, rew.float())
    ret = torch.zeros(W, Tm, replay.P, device=dev)
    acc = torch.zeros_like(rew[:, 0])
    for t in range(Tm - 1, -1, -1):       # DeviceGenerator._returns: fp64 from the top
        acc = rew[:, t] + gamma * acc
        ret[:, t].copy_(acc)
    put(replay.ret, ret)
    put(replay.length, L)
    put(replay.outcome, outcome.index_select(0, slot))
    put(ring_game, game.index_select(0, slot))
    game.copy_(torch.where(done, state[2] + r, game))
    ply.masked_fill_(done, 0)
    st['pending'].logical_or_(done)
    state[0:1].copy_(((state[0] + c) % N).view(1))
    state[1:3].add_(c)


def harvest_torch(st, done, outcome, gamma, replay, ring_game, has_reward=True):
    """``_harvest_torch`` for the mover records into a ``DeviceReplay`` (the contract of hrl_selfplay_harvest,
    include/hrl_env.h, which equals this bit for bit).  ``st``: the slot records and 'ply', 'game', 'pending',
    'state', 'rows'."""
    _harvest_torch(('action', 'value', 'turn'), st, done, outcome, gamma, replay, ring_game, has_reward)


def harvest_players_torch(st, done, outcome, gamma, replay, ring_game, has_reward=False):
    """``_harvest_torch`` for per-player records into a ``PlayerReplay`` (the contract of
    hrl_selfplay_harvest_players, which equals this bit for bit): the records carry a player axis and ``tmask`` /
    ``omask`` take the place of ``turn``."""
    _harvest_torch(('action', 'value', 'tmask', 'omask'), st, done, outcome, gamma, replay, ring_game, has_reward)


def _obs_type(t):
    from . import _native
    if t.dtype not in (torch.uint8, torch.float32):
        raise ValueError('observation records are uint8 or float32, not %s' % t.dtype)
    return _native.REPLAY_F32 if t.dtype == torch.float32 else _native.REPLAY_U8


def _obs_leaves(struct, obs, lead, typed=True):
    """The observation fields of a slots or ring struct from the leaves of ``obs``, each ``lead`` + its own shape;
    ``typed``: the struct names each leaf's type, else every leaf is fp32.  Returns the leaves."""
    from . import _native
    src = _leaves(obs)
    if len(src) > _native.REPLAY_MAX_LEAVES:
        raise ValueError('at most %d observation leaves' % _native.REPLAY_MAX_LEAVES)
    struct.nleaves = len(src)
    for l, o in enumerate(src):
        assert o.is_contiguous() and o.shape[:len(lead)] == lead
        struct.obs[l] = o.data_ptr()
        struct.obs_width[l] = int(np.prod(o.shape[len(lead):], dtype=np.int64))
        if typed:
            struct.obs_type[l] = _obs_type(o)
        else:
            assert o.dtype == torch.float32
    return src


def _ring_struct(replay):
    """struct hrl_replay_ring of a DeviceReplay / PlayerReplay (the struct keeps no tensor alive)."""
    from . import _native
    ring = _native.ReplayRing()
    ring.N, ring.Tm, ring.P, ring.A = replay.N, replay.Tm, replay.P, replay.policy.shape[-1]
    _obs_leaves(ring, replay.obs, tuple(replay.policy.shape[:replay._lead]))
    for k in ('policy', 'amask', 'action', 'value', 'reward', 'ret', 'length', 'outcome'):
        setattr(ring, k, getattr(replay, k).data_ptr())
    if replay._lead == 3:      # PlayerReplay: the PLAYERS layouts
        ring.tmask, ring.omask = replay.tmask.data_ptr(), replay.omask.data_ptr()
    else:
        ring.turn = replay.turn.data_ptr()
    return ring


def _harvest_hip(entry, slots, lead, typed, keys, st, done, outcome, gamma, replay, ring_game, has_reward):
    """The two launches of ``entry`` (hrl_selfplay_harvest / hrl_selfplay_harvest_players) on the slot records
    ``keys`` of ``st``; ``slots``: the entry's struct with E, Tm, P, A set; ``lead``: the records' leading dims;
    ``typed``: the struct names each observation leaf's type (else every leaf is fp32)."""
    from . import _native
    E = slots.E
    _obs_leaves(slots, st['obs'], lead, typed)
    for k in ('policy', 'amask') + keys:
        assert st[k].is_contiguous()
        setattr(slots, k, st[k].data_ptr())
    slots.reward = st['reward'].data_ptr() if has_reward else None
    done, outcome = done.contiguous(), outcome.float().contiguous()
    assert done.shape == (E,) and done.dtype == torch.bool and outcome.shape == (E, replay.P)
    assert st['pending'].dtype == torch.bool and st['state'].shape == (3,) and st['state'].dtype == torch.long
    assert ring_game.shape == (replay.N,) and ring_game.dtype == torch.long and ring_game.is_contiguous()
    ring = _ring_struct(replay)
    _native.check(getattr(_native.load(), entry)(
        _native.ptr(done), ctypes.byref(slots), _native.ptr(st['ply']), _native.ptr(outcome), float(gamma),
        ctypes.byref(ring), _native.ptr(ring_game), _native.ptr(st['game']), _native.ptr(st['pending']),
        _native.ptr(st['state']), _native.stream_of(done.device)), entry)


def harvest_hip(st, done, outcome, gamma, replay, ring_game, has_reward=True):
    """harvest_torch as the two launches of hrl_selfplay_harvest."""
    from . import _native
    slots = _native.SelfplaySlots()
    slots.E, slots.Tm, slots.A = st['policy'].shape
    slots.P = st['reward'].shape[2]
    _harvest_hip('hrl_selfplay_harvest', slots, (slots.E, slots.Tm), False, ('action', 'value', 'turn'), st, done,
                 outcome, gamma, replay, ring_game, has_reward)


def harvest_players_hip(st, done, outcome, gamma, replay, ring_game, has_reward=False):
    """harvest_players_torch as the two launches of hrl_selfplay_harvest_players."""
    from . import _native
    slots = _native.SelfplayPlayerSlots()
    slots.E, slots.Tm, slots.P, slots.A = st['policy'].shape
    assert st['tmask'].dtype == st['omask'].dtype == torch.bool and st['action'].dtype == torch.long
    _harvest_hip('hrl_selfplay_harvest_players', slots, (slots.E, slots.Tm, slots.P), True,
                 ('action', 'value', 'tmask', 'omask'), st, done, outcome, gamma, replay, ring_game, has_reward)


class _StreamDriver:
    """What ``StreamGenerator`` and ``PlayerStreamGenerator`` share: the bookkeeping of a stream of games, the
    capture of the step's graphs with the games put back afterwards, and the loop that replays them until enough
    episodes are in the ring, with one host read of the device ring state per ``check_every`` steps.  A subclass
    checks its scope before it calls ``__init__`` and has ``_state()``, ``_persistent(st)`` (everything a step
    changes besides the slot records and the ring), ``_bodies(st, dry=False)`` (the ordered {m: callable} of one
    global step each, step s running body s % len; ``dry``: nothing is harvested) and ``_session(st)`` (the context a
    call runs in: the net's inference session, if it has one)."""

    def __init__(self, env_batch, net, replay, gamma, seed, check_every, graph, shape_error):
        if (replay.Tm, replay.P, replay.policy.shape[-1]) != (env_batch.MAX_PLIES, env_batch.P, env_batch.A):
            raise ValueError(shape_error)
        self.env, self.net, self.replay = env_batch, net, replay
        self.gamma, self.seed = float(gamma), int(seed) & 0xffffffffffffffff
        self.check_every = max(1, int(check_every or 1))
        self.graph = graph
        self.s = 0                         # global steps run
        self.games_started = env_batch.E
        self._emitted = 0
        self._steps = 0                    # env-steps of the emitted episodes
        self._st = None
        self._graphs = None
        self.ring_game = torch.full((replay.N,), -1, dtype=torch.long, device=env_batch.device)

    def _use_graph(self):
        return graph_wanted(self.env.device, self.graph)

    def _capture(self, st):
        """One graph per body.  Dry steps run first on a side stream (library workspaces) and harvest nothing; the
        games, the ring state and the recurrent state are then put back, so that warm-up and capture leave no trace
        (a slot record the warm-up wrote is written again by the ply that owns it)."""
        keep = [t.clone() for t in self._persistent(st)]
        dry = self._bodies(st, dry=True)

        def warm():
            for body in dry.values():
                body()
        graphs = capture_graphs(self.env.device, self._bodies(st), warm)
        for t, k in zip(self._persistent(st), keep):
            t.copy_(k)
        return graphs

    @torch.no_grad()
    def generate(self, episodes):
        """Run global steps until ``episodes`` more games have been emitted into the ring (checked every
        ``check_every`` steps, so a call may overshoot).  Returns {'episodes': emitted by this call, 'env_steps':
        the sum of their lengths, 'plies': global steps run}."""
        st = self._state()
        with eval_mode(self.net), self._session(st):
            return self._generate(st, int(episodes))

    def _generate(self, st, episodes):
        N = self.replay.N
        bodies = self._bodies(st)
        if self._use_graph():
            # a captured step reads the net's parameters and buffers where they live: recapture if any moved (the
            # games stay); the switch between the kernels and their torch formulation is part of the capture too
            key = (FUSED_STREAM,) + params_key(self.net)
            if self._graphs is None or self._graphs[0] != key:
                self._graphs = (key, self._capture(st))
            bodies = {m: g.replay for m, g in self._graphs[1].items()}
        emitted0, steps0, s0 = self._emitted, self._steps, self.s
        target = emitted0 + episodes
        emitted = emitted0
        M = len(bodies)
        while emitted < target:
            for _ in range(self.check_every):
                bodies[self.s % M]()
                self.s += 1
            emitted = int(st['state'][1])
        ring_ptr, emitted, next_game = (int(v) for v in st['state'].tolist())
        self._steps = int(st['played'].sum()) - int(st['ply'].sum())   # all plies played less the games in flight
        self.replay.ptr = ring_ptr
        self.replay.count = min(self.replay.count + emitted - emitted0, N)
        self._emitted, self.games_started = emitted, next_game
        return {'episodes': emitted - emitted0, 'env_steps': self._steps - steps0, 'plies': self.s - s0}


class StreamGenerator(_StreamDriver):
    """Continuous batched self-play: E slots, each at its own ply; a finished game goes straight into the replay
    ring and its slot starts a new game (the reference's workers start an episode the moment one ends,
    generation.py:20-88, worker.py:58-77).  ``DeviceGenerator`` plays its E games in lockstep instead, and a
    finished game's slot idles until the longest game of the batch ends.

    Scope: the mover-only ply of ALTERNATING envs (TicTacToe, Geister, CIGeister in the stock mode) into a
    ``DeviceReplay``; per-player records, ``observation`` and ``SIMULTANEOUS`` envs stay with the lockstep
    ``DeviceGenerator``.

    A global step counter s fixes the mover m = s % P of every live game, as in lockstep (so the P captured ply
    graphs, ``h[mover]`` as a view and GeisterNet's in-place session all carry over); to keep that invariant a
    finished slot restarts only at a step with s % P == 0 -- a game of odd length waits one ply.  Each slot
    carries its ply index and its game number; game n samples ply t with ``stream_uniforms(seed, n, t, A)``
    whatever slot it is played in and whenever, so every episode can be checked on its own (``ring_game`` names
    the game in each ring row) and no (Tm, E, A) uniform buffer exists.  The harvest
    (hrl_selfplay_harvest) writes the finished games' records, returns, lengths and outcomes into the ring in slot
    order and keeps the ring state {ring_ptr, emitted, next_game} in device memory; ``DeviceReplay.add`` is not
    used.  ``generate`` mirrors that state into ``replay.ptr`` / ``replay.count`` on return, so ``replay.sample``,
    ``draw_windows`` and the gather work unchanged.

    Weights: every call enters the net's ``inference_session``, which refreshes the inference weights in place;
    games in flight continue under the new weights.  That is sound for IMPALA-style off-policy learning (V-trace /
    UPGO with importance ratios) because every ply records the policy it was sampled from.

    State persists across calls: ``generate(64)`` and four ``generate(16)`` emit the same first 64 episodes.
    ``games_started``: game numbers handed out so far (the next new game's number).
    """

    def __init__(self, env_batch, net, replay, gamma=0.8, seed=0, check_every=16, graph=None, observation=False,
                 per_player=False):
        if (observation or per_player or getattr(env_batch, 'SIMULTANEOUS', False)
                or not getattr(env_batch, 'ALTERNATING', False) or getattr(replay, '_lead', 2) != 2):
            raise ValueError('StreamGenerator plays the mover-only ply of an alternating env into a DeviceReplay; '
                             'per-player records, observation=True and simultaneous envs are played by the lockstep '
                             'generator (rollout.DeviceGenerator)')
        super().__init__(env_batch, net, replay, gamma, seed, check_every, graph,
                         'the replay does not have the env\'s MAX_PLIES, P and A')

    def _state(self):
        """The slots' buffers, allocated once: the games live in them across calls."""
        if self._st is not None:
            return self._st
        env, E, dev = self.env, self.env.E, self.env.device
        Tm, A, P = env.MAX_PLIES, env.A, env.P
        st = {'obs': _alloc(env.OBS_SHAPE, (E, Tm), dev),
              'policy': torch.zeros(E, Tm, A, device=dev),
              'amask': torch.full((E, Tm, A), 1e32, device=dev),
              'action': torch.zeros(E, Tm, dtype=torch.long, device=dev),
              'value': torch.zeros(E, Tm, device=dev),
              'turn': torch.zeros(E, Tm, dtype=torch.long, device=dev),
              'reward': torch.zeros(E, Tm, P, device=dev, dtype=torch.float64),
              'ply': torch.zeros(E, dtype=torch.long, device=dev),
              'game': torch.arange(E, dtype=torch.long, device=dev),
              'pending': torch.zeros(E, dtype=torch.bool, device=dev),
              'played': torch.zeros(E, dtype=torch.long, device=dev),     # plies played by the slot, all games
              'state': torch.tensor([self.replay.ptr, 0, E], dtype=torch.long, device=dev),
              'rows': torch.arange(E, device=dev),
              'hidden': None, 'pmajor': False, 'obs_dev': torch.device(dev).type}
        if hasattr(self.net, 'inference_hidden') and st['obs_dev'] == 'cuda':
            st['hidden'] = self.net.inference_hidden(E, P, dev)   # leaves (P, E, ...), the net's own layout
            st['pmajor'] = True
        elif hasattr(self.net, 'init_hidden'):
            st['hidden'] = map_r(self.net.init_hidden([E, P]), lambda h: h.to(dev).contiguous())
        env.reset()
        self._st = st
        return st

    def _persistent(self, st):
        """Everything a ply changes besides the slot records and the ring."""
        hidden = [] if st['hidden'] is None else _leaves(st['hidden'])
        return self.env.state_tensors() + hidden + [st[k] for k in ('ply', 'game', 'pending', 'played', 'state')]

    def _ply(self, st, mover, dry=False):
        """One global step with mover ``mover`` = s % P; ``dry``: nothing is harvested (capture warm-up)."""
        env, E, Tm = self.env, self.env.E, self.env.MAX_PLIES
        fused = FUSED_STREAM and st['obs_dev'] == 'cuda'
        ply, rows, hidden = st['ply'], st['rows'], st['hidden']
        if mover == 0:
            # finished games restart here only, so that s % P is the mover of every live game
            pending = st['pending']
            env.reset_where(pending)
            if hidden is not None:
                def clear(h):
                    shape = (1, E) if st['pmajor'] else (E, 1)
                    h.masked_fill_(pending.view(*shape, *([1] * (h.dim() - 2))), 0)
                map_r(hidden, clear)
            pending.zero_()
        # a snapshot: GeisterBatch.active() is state its step updates in place
        active = env.active().clone() if hasattr(env, 'active') else ~env.terminal()
        player = env.turn()
        obs_recorded = fused and hasattr(env, 'observation_record_at')
        o = env.observation_record_at(player, st['obs'], ply, active) if obs_recorded else env.observation(player)
        if hidden is None:
            h_in = None
        else:
            h_in = map_r(hidden, (lambda h: h[mover]) if st['pmajor'] else (lambda h: h[:, mover]))
        out = self.net(o, h_in)
        has_reward = hasattr(env, 'reward')
        early = has_reward and getattr(env, 'REWARD_STATELESS', False)
        reward = env.reward() if early else None
        if not obs_recorded:
            bimap_r(st['obs'], o, lambda b, x: _record_at(b, rows, ply, x, active))
        sample = sample_record_stream_hip if fused else sample_record_stream_torch
        a = sample(st, self.seed, out['policy'], env.legal(), out['value'], active, player, reward)
        if hidden is not None and st['obs_dev'] == 'cuda':
            dst = [h[mover] if st['pmajor'] else h[:, mover] for h in _leaves(hidden)]
            src = _leaves(out['hidden'])
            # a net that advanced its stacked state in place left nothing to copy (DeviceGenerator._ply); a
            # finished game's state moves too, and is zeroed when its slot restarts
            if not all(d.data_ptr() == x.data_ptr() and d.stride() == x.stride() for d, x in zip(dst, src)):
                from .nn import masked_rows_copy_
                masked_rows_copy_(dst, src, active.contiguous())
        elif hidden is not None:
            def advance(h, nh):
                live = active.view(-1, *([1] * (nh.dim() - 1)))
                h[:, mover].copy_(torch.where(live, nh, h[:, mover]))
            bimap_r(hidden, out['hidden'], advance)
        env.step(a, active)
        if has_reward and not early:
            _record_at(st['reward'], rows, ply, env.reward().to(st['reward'].dtype), active)
        ply.add_(active)
        st['played'].add_(active)
        done = active & (env.terminal() | (ply >= Tm))
        if dry:
            done = torch.zeros_like(done)
        harvest = harvest_hip if fused else harvest_torch
        harvest(st, done, env.outcome(), self.gamma, self.replay, self.ring_game, has_reward)

    def _bodies(self, st, dry=False):
        """One body per mover: step s runs the ply of mover s % P."""
        return {m: functools.partial(self._ply, st, m, dry) for m in range(self.env.P)}

    def _session(self, st):
        session = getattr(self.net, 'inference_session', None)
        return session(inplace_state=st['pmajor']) if session is not None else contextlib.nullcontext()


# ---- streaming self-play of simultaneous-move envs: per-player records (PlayerStreamGenerator) ----

def sample_record_players_stream_torch(st, seed, logits, legal, value, turns, infer, active):
    """The per-player streaming ply's sampling and recording tail as torch ops (the contract of
    hrl_selfplay_sample_record_players_stream, include/hrl_env.h, which equals this bit for bit).  ``logits``
    (P * E, >= A) and ``value`` (P * E, ...) are the forward's rows, player-major; ``legal`` (E, A) or (E, P, A);
    ``turns`` / ``infer`` (E, P) and ``active`` (E,) bool.  A game is played when it is active and its ply lies in
    [0, Tm); a played game stores slot (e, ply[e]) of EVERY player: the live values where ``turns`` (policy, action
    mask, action, turn mask) or ``infer`` (value, observation mask) is set and the reset values elsewhere.  Returns
    the actions (E, P) (0 where not played or no turn) and the select uniforms (E,)."""
    rows, ply, game = st['rows'], st['ply'], st['game']
    E, P = turns.shape
    Tm, A = st['policy'].shape[1], st['policy'].shape[3]
    played = active & (ply >= 0) & (ply < Tm)
    lg = logits.float().view(P, E, -1)[:, :, :A].transpose(0, 1)                  # (E, P, A)
    val = value.float().reshape(P, E).t()                                         # (E, P)
    if legal.dim() == 2:
        legal = legal.view(E, 1, A).expand(E, P, A)
    m = torch.where(legal, 0.0, 1e32)
    p = lg - m
    u = stream_player_uniforms_torch(seed, game, ply, P, A)
    a = torch.argmax(p - torch.log(-torch.log(u)), dim=-1)
    sampled = turns & played.view(E, 1)
    a = torch.where(sampled, a, torch.zeros_like(a))
    t3 = turns.view(E, P, 1)
    _record_at(st['policy'], rows, ply, torch.where(t3, p, 0.0), played)
    _record_at(st['amask'], rows, ply, torch.where(t3, m, 1e32), played)
    _record_at(st['action'], rows, ply, a, played)
    _record_at(st['tmask'], rows, ply, turns, played)
    _record_at(st['value'], rows, ply, torch.where(infer, val, 0.0), played)
    _record_at(st['omask'], rows, ply, infer, played)
    return a, stream_select_uniform_torch(seed, game, ply)


def sample_record_players_stream_hip(st, seed, logits, legal, value, turns, infer, active):
    """sample_record_players_stream_torch as ONE launch, one wave per (game, player)."""
    from . import _native
    E, P = turns.shape
    Tm, A = st['policy'].shape[1], st['policy'].shape[3]
    _player_blocks(P, A)
    logits = logits.float()
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    value = value.reshape(P * E).float().contiguous()
    legal, turns, infer, active = legal.contiguous(), turns.contiguous(), infer.contiguous(), active.contiguous()
    assert logits.shape[0] == P * E and logits.shape[1] >= A
    assert legal.dtype == torch.bool and legal.shape in ((E, A), (E, P, A))
    assert infer.shape == (E, P) and active.shape == (E,)
    assert turns.dtype == infer.dtype == active.dtype == torch.bool
    assert st['policy'].shape == st['amask'].shape == (E, Tm, P, A)
    for k, dt in (('policy', torch.float32), ('amask', torch.float32), ('action', torch.long),
                  ('value', torch.float32), ('tmask', torch.bool), ('omask', torch.bool)):
        assert st[k].dtype == dt and st[k].is_contiguous() and st[k].shape[:3] == (E, Tm, P), k
    for k in ('game', 'ply'):
        assert st[k].shape == (E,) and st[k].dtype == torch.long and st[k].is_contiguous()
    a = torch.empty(E, P, dtype=torch.long, device=logits.device)
    usel = torch.empty(E, device=logits.device)
    _native.check(_native.load().hrl_selfplay_sample_record_players_stream(
        _native.ptr(logits), logits.stride(0), _native.ptr(value), _native.ptr(legal), A if legal.dim() == 3 else 0,
        _native.ptr(turns), _native.ptr(infer), _native.ptr(active), int(seed) & 0xffffffffffffffff,
        _native.ptr(st['game']), _native.ptr(st['ply']), E, P, A, Tm, _native.ptr(a), _native.ptr(usel),
        _native.ptr(st['policy']), _native.ptr(st['amask']), _native.ptr(st['action']), _native.ptr(st['value']),
        _native.ptr(st['tmask']), _native.ptr(st['omask']), _native.stream_of(logits.device)),
        'hrl_selfplay_sample_record_players_stream')
    return a, usel


class PlayerStreamGenerator(_StreamDriver):
    """``StreamGenerator`` for simultaneous-move envs (``SIMULTANEOUS``: Hungry Geese, ParallelTicTacToe): E slots,
    each at its own ply, every player moving every ply; a finished game goes straight into a ``PlayerReplay`` ring
    and its slot starts the next game on the very next step (a simultaneous env has no mover parity to wait for).
    The lockstep ``DeviceGenerator`` runs every ply until the last of its E games ends; with games of a few plies
    most of its forward rows belong to finished games.

    One global step: the ``pending`` slots restart (``env.restart_games(mask, games)`` where the env numbers its
    games itself, else ``reset_where``); ``active`` / ``turns`` / ``infer`` are snapshot; every view is built and
    recorded at (e, ply[e]) (``env.observe_players_record_at``: uint8 slot records, one launch; else torch ops on
    fp32 ones); one forward over the P * E rows; the sampling and recording tail
    (hrl_selfplay_sample_record_players_stream); ``env.step_players``; ``ply += active``; the harvest of the games
    that ended (hrl_selfplay_harvest_players).  The step is one captured graph.

    Game number n samples ply t with ``stream_player_uniforms(seed, n, t, P, A)`` and steps with
    ``stream_select_uniform(seed, n, t)`` whatever slot it is played in and whenever, so every ring row can be
    refereed on its own (``ring_game`` names its game).  State persists across calls: ``generate(64)`` and four
    ``generate(16)`` emit the same first 64 episodes.  ``generate`` mirrors the device ring state into
    ``replay.ptr`` / ``replay.count``, ``games_started`` and ``env.next_game``.

    Scope: a ``SIMULTANEOUS`` env, a net without recurrent state and a ``PlayerReplay`` of the env's (Tm, P, A);
    ``observation=True`` records every live player's view (for these envs every live player is a turn player
    anyway).  Everything else is played by the lockstep ``DeviceGenerator`` and raises ``ValueError`` here."""

    def __init__(self, env_batch, net, replay, gamma=0.8, seed=0, check_every=16, graph=None, observation=False):
        if (not getattr(env_batch, 'SIMULTANEOUS', False) or hasattr(net, 'init_hidden')
                or getattr(replay, '_lead', 2) != 3):
            raise ValueError('PlayerStreamGenerator plays a simultaneous-move env with a net without recurrent state '
                             'into a PlayerReplay; alternating envs stream through rollout.StreamGenerator, and '
                             'everything else is played by the lockstep generator (rollout.DeviceGenerator)')
        super().__init__(env_batch, net, replay, gamma, seed, check_every, graph,
                         'the replay does not have the env\'s MAX_PLIES, P and A; the lockstep generator '
                         '(rollout.DeviceGenerator) returns episodes of any replay\'s shape')
        _player_blocks(env_batch.P, env_batch.A)
        self.observation = bool(observation)

    def _state(self):
        """The slots' buffers, allocated once: the games live in them across calls.  Every slot starts ``pending``
        with its own index as game number, so the first step starts games 0 .. E-1 like any later restart."""
        if self._st is not None:
            return self._st
        env, E, dev = self.env, self.env.E, self.env.device
        Tm, A, P = env.MAX_PLIES, env.A, env.P
        u8 = hasattr(env, 'observe_players_record_at')
        st = {'obs': _alloc(env.OBS_SHAPE, (E, Tm, P), dev, torch.uint8 if u8 else torch.float32),
              'policy': torch.zeros(E, Tm, P, A, device=dev),
              'amask': torch.full((E, Tm, P, A), 1e32, device=dev),
              'action': torch.zeros(E, Tm, P, dtype=torch.long, device=dev),
              'value': torch.zeros(E, Tm, P, device=dev),
              'tmask': torch.zeros(E, Tm, P, dtype=torch.bool, device=dev),
              'omask': torch.zeros(E, Tm, P, dtype=torch.bool, device=dev),
              'ply': torch.zeros(E, dtype=torch.long, device=dev),
              'game': torch.arange(E, dtype=torch.long, device=dev),
              'pending': torch.ones(E, dtype=torch.bool, device=dev),
              'played': torch.zeros(E, dtype=torch.long, device=dev),     # plies played by the slot, all games
              'state': torch.tensor([self.replay.ptr, 0, E], dtype=torch.long, device=dev),
              'rows': torch.arange(E, device=dev),
              'players': torch.arange(P, device=dev).view(P, 1).expand(P, E).contiguous(),
              'obs_dev': torch.device(dev).type}
        if hasattr(env, 'reward'):
            st['reward'] = torch.zeros(E, Tm, P, device=dev, dtype=torch.float64)
        self._st = st
        return st

    def _persistent(self, st):
        """Everything a step changes besides the slot records and the ring."""
        return self.env.state_tensors() + [st[k] for k in ('ply', 'game', 'pending', 'played', 'state')]

    def _ply(self, st, dry=False):
        """One global step; ``dry``: nothing is harvested (capture warm-up)."""
        env, E, P, Tm = self.env, self.env.E, self.env.P, self.env.MAX_PLIES
        fused = FUSED_STREAM and st['obs_dev'] == 'cuda'
        ply, rows, pending = st['ply'], st['rows'], st['pending']
        if hasattr(env, 'restart_games'):
            env.restart_games(pending, st['game'])
        else:
            env.reset_where(pending)
        pending.zero_()
        # snapshots: an env's active() may be state its step updates in place
        active = (env.active() if hasattr(env, 'active') else ~env.terminal()).clone()
        turns = (env.turns_mask() & active.view(E, 1)).contiguous()
        infer = active.view(E, 1).expand(E, P).contiguous() if self.observation else turns
        if hasattr(env, 'observe_players_record_at'):
            o = env.observe_players_record_at(st['obs'], ply, infer, active)                  # (P * E, ...)
        else:
            views = [env.observation(st['players'][p]) for p in range(P)]
            o = _stack_views(views)
            played = active & (ply < Tm)

            def record(buf, v):
                keep = infer.view(E, P, *([1] * (v.dim() - 2)))
                _record_at(buf, rows, ply, torch.where(keep, v, 0.0), played)
            bimap_r(st['obs'], _stack_views(views, batch_first=True), record)
        out = self.net(o, None)
        legal = env.legal_players() if hasattr(env, 'legal_players') else env.legal()
        sample = sample_record_players_stream_hip if fused else sample_record_players_stream_torch
        a, usel = sample(st, self.seed, out['policy'], legal, out['value'], turns, infer, active)
        env.step_players(a, turns, active, usel)
        has_reward = 'reward' in st
        if has_reward:
            _record_at(st['reward'], rows, ply, env.reward().to(st['reward'].dtype), active & (ply < Tm))
        ply.add_(active)
        st['played'].add_(active)
        done = active & (env.terminal() | (ply >= Tm))
        if dry:
            done = torch.zeros_like(done)
        harvest = harvest_players_hip if fused else harvest_players_torch
        harvest(st, done, env.outcome(), self.gamma, self.replay, self.ring_game, has_reward)

    def _bodies(self, st, dry=False):
        """Every player moves every ply: one body."""
        return {0: functools.partial(self._ply, st, dry)}

    def _session(self, st):
        stateless = getattr(self.net, 'stateless_session', False)
        session = getattr(self.net, 'inference_session', None) if stateless else None
        return session() if session is not None else contextlib.nullcontext()

    def _generate(self, st, episodes):
        out = super()._generate(st, episodes)
        if hasattr(self.env, 'next_game'):
            self.env.next_game = self.games_started
        return out


# True: on a GPU ``gather`` is the one launch of hrl_replay_gather (include/hrl_replay.h) instead of the torch ops
# below, which stay as the CPU path and as the formulation the kernel is tested against (bit-identical).
FUSED_GATHER = True

_DRAWS = ('multinomial', 'inverse')


class DeviceReplay:
    """Ring buffer of episodes in HBM; windows gathered into the make_batch layout.

    ``obs_shape`` is a shape or {name: shape}; ``obs_dtype`` lets binary
    observation planes (TicTacToe, Geister) live in HBM as uint8, a quarter
    of the bytes, widened to fp32 by the gather.  ``draw``: how ``sample``
    picks its windows, ``'multinomial'`` (``sample_windows``) or ``'inverse'``
    (``draw_windows``: one uniform draw and one launch).
    """

    solo = mover = False
    _lead = 2    # leading axes of a record, (N, Tm); PlayerReplay: (N, Tm, P)

    def __init__(self, capacity, max_plies, obs_shape, A, P, device, maximum_episodes=None,
                 obs_dtype=torch.float32, draw='multinomial'):
        if draw not in _DRAWS:
            raise ValueError('draw must be one of %s, not %r' % (_DRAWS, draw))
        self.draw = draw
        self.N, self.Tm, self.P, self.device = capacity, max_plies, P, device
        self.maximum_episodes = maximum_episodes or capacity
        f = dict(device=device)
        self.obs = _alloc(obs_shape, (capacity, max_plies), device, obs_dtype)
        self.policy = torch.zeros(capacity, max_plies, A, **f)
        self.amask = torch.full((capacity, max_plies, A), 1e32, **f)
        self.action = torch.zeros(capacity, max_plies, dtype=torch.long, **f)
        self.value = torch.zeros(capacity, max_plies, **f)
        self.turn = torch.zeros(capacity, max_plies, dtype=torch.long, **f)
        self.reward = torch.zeros(capacity, max_plies, P, **f)
        self.ret = torch.zeros(capacity, max_plies, P, **f)
        self.length = torch.ones(capacity, dtype=torch.long, **f)
        self.outcome = torch.zeros(capacity, P, **f)
        self.ptr = 0      # next slot
        self.count = 0    # stored episodes (<= capacity)

    def add(self, ep):
        E = ep['length'].shape[0]
        slots = (self.ptr + torch.arange(E, device=self.device)) % self.N
        bimap_r(self.obs, ep['observation'], lambda dst, src: dst.index_copy_(0, slots, src.to(dst.dtype)))
        for dst, key in ((self.policy, 'policy'), (self.amask, 'action_mask'),
                         (self.action, 'action'), (self.value, 'value'), (self.turn, 'turn'),
                         (self.reward, 'reward'), (self.ret, 'return'), (self.length, 'length'),
                         (self.outcome, 'outcome')):
            dst.index_copy_(0, slots, ep[key])
        self.ptr = (self.ptr + E) % self.N
        self.count = min(self.count + E, self.N)

    def _age_order(self):
        """Slot of the i-th oldest stored episode (i = 0 oldest)."""
        start = (self.ptr - self.count) % self.N
        return (start + torch.arange(self.count, device=self.device)) % self.N

    def sample_windows(self, B, T, generator=None):
        """(slot, start) of B windows, as Batcher.select_episode draws them (train.py:284-293).

        Episode i of the n newest (i = n-1 newest) is accepted with probability
        1 - (n-1-i)/maximum_episodes; drawing from that weighting directly is
        the distribution of the reference's rejection loop.
        """
        n = min(self.count, self.maximum_episodes)
        i = torch.arange(n, device=self.device, dtype=torch.float64)
        w = 1.0 - (n - 1 - i) / self.maximum_episodes
        pick = torch.multinomial(w.float(), B, replacement=True, generator=generator)
        slots = self._age_order()[self.count - n:][pick]
        steps = self.length[slots]
        cand = 1 + torch.clamp(steps - T, min=0)
        u = torch.rand(B, device=self.device, generator=generator)
        start = torch.minimum((u * cand).long(), cand - 1)
        return slots, start

    def draw_windows(self, B, T, generator=None, u=None):
        """(slot, start, player) of B windows from ``u`` (3, B) uniforms in [0, 1) (drawn here when None), by the
        integer rule of hrl_replay_draw (include/hrl_replay.h): the inverse of the cumulative integer weights
        M - (n-1-i) of ``sample_windows``' distribution.  On a GPU one ``torch.rand`` and one launch; elsewhere the
        torch formulation of the same rule, which the kernel equals exactly."""
        if self.count < 1:
            raise ValueError('draw_windows on an empty replay')
        if u is None:
            u = torch.rand(3, B, device=self.device, generator=generator)
        if u.shape != (3, B) or u.dtype != torch.float32:
            raise ValueError('u must be (3, %d) float32' % B)
        M, P = int(self.maximum_episodes), self.P
        if u.is_cuda:
            from . import _native
            idx = torch.empty(3, B, dtype=torch.long, device=u.device)
            u = u.contiguous()
            w = B * 8
            _native.check(_native.load().hrl_replay_draw(
                _native.ptr(u), B, self.ptr, self.count, self.N, M, _native.ptr(self.length), T, P,
                idx.data_ptr(), idx.data_ptr() + w, idx.data_ptr() + 2 * w, _native.stream_of(u.device)),
                'hrl_replay_draw')
            return idx[0], idx[1], idx[2]
        n = min(self.count, M)
        i = torch.arange(n, device=u.device)
        cum = (i + 1) * (M - n + 1) + i * (i + 1) // 2
        total = n * (M - n + 1) + (n - 1) * n // 2
        x = torch.floor(u[0].double() * float(total)).long()
        pick = torch.searchsorted(cum, x, right=True).clamp_(max=n - 1)
        slots = (self.ptr - n + pick) % self.N
        cand = 1 + torch.clamp(self.length[slots] - T, min=0)
        start = torch.minimum((u[1] * cand).long(), cand - 1)
        players = torch.clamp((u[2] * float(P)).long(), max=P - 1)
        return slots, start, players

    def _player_axes(self, solo, mover):
        """(Pm, Pn): the player axis of observation / policy / action_mask / action, and of the other fields."""
        return 1, self.P

    def _batch_spec(self, B, T, Pm, Pn):
        """{key: shape} of a batch; 'observation': the shapes of its leaves, in ``_leaves`` order."""
        A = self.policy.shape[-1]
        return {'observation': [(B, T, Pm) + tuple(o.shape[self._lead:]) for o in _leaves(self.obs)],
                'policy': (B, T, Pm, A), 'value': (B, T, Pn, 1), 'action': (B, T, Pm, 1),
                'outcome': (B, 1, Pn, 1), 'reward': (B, T, Pn, 1), 'return': (B, T, Pn, 1),
                'episode_mask': (B, T, 1, 1), 'turn_mask': (B, T, Pn, 1), 'observation_mask': (B, T, Pn, 1),
                'action_mask': (B, T, Pm, A), 'progress': (B, T, 1)}

    def _alloc_spec(self, spec):
        f = dict(device=self.policy.device)
        out = {k: torch.empty(s, dtype=torch.long if k == 'action' else torch.float32, **f)
               for k, s in spec.items() if k != 'observation'}
        shapes = iter(spec['observation'])
        out['observation'] = map_r(self.obs, lambda o: torch.empty(next(shapes), **f))
        return out

    def alloc_batch(self, B, T):
        """A batch dict for ``gather(..., out=)`` / ``sample(..., out=)`` that the caller keeps and reuses."""
        return self._alloc_spec(self._batch_spec(B, T, *self._player_axes(self.solo, self.mover)))

    def _gather_native(self, slots, start, T, players, mover, out):
        """hrl_replay_gather: one launch fills ``out`` (allocated here when None); no torch op on the batch."""
        from . import _native
        B = slots.shape[0]
        per_player = self._lead == 3
        Pm, Pn = self._player_axes(players is not None, mover)
        spec = self._batch_spec(B, T, Pm, Pn)
        if out is None:
            out = self._alloc_spec(spec)
        src, dst, shapes = _leaves(self.obs), _leaves(out['observation']), spec['observation']
        if len(src) > _native.REPLAY_MAX_LEAVES:
            raise ValueError('hrl_replay_gather takes at most %d observation leaves' % _native.REPLAY_MAX_LEAVES)
        if len(dst) != len(src):
            raise ValueError("out['observation'] does not have the replay's leaves")
        for name, t, shape, dtype in ([(k, out[k], spec[k], torch.long if k == 'action' else torch.float32)
                                       for k in spec if k != 'observation']
                                      + [('observation', t, s, torch.float32) for t, s in zip(dst, shapes)]):
            if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda:
                raise ValueError('out[%r]: expected a contiguous %s GPU tensor of shape %s, got %s %s'
                                 % (name, dtype, tuple(shape), t.dtype, tuple(t.shape)))
        for name, t in (('slots', slots), ('start', start), ('players', players)):
            if t is not None and (t.dtype != torch.long or t.shape != (B,) or not t.is_contiguous() or not t.is_cuda):
                raise ValueError('%s must be a contiguous (B,) int64 GPU tensor' % name)
        ring = _native.ReplayRing()
        ring.N, ring.Tm, ring.P, ring.A, ring.nleaves = self.N, self.Tm, self.P, self.policy.shape[-1], len(src)
        for l, o in enumerate(src):
            if o.dtype not in (torch.uint8, torch.bool, torch.float32):
                raise ValueError('observation records are uint8, bool or float32, not %s' % o.dtype)
            ring.obs[l] = o.data_ptr()
            ring.obs_type[l] = _native.REPLAY_F32 if o.dtype == torch.float32 else _native.REPLAY_U8
            ring.obs_width[l] = int(np.prod(o.shape[self._lead:], dtype=np.int64))
        for k in ('policy', 'amask', 'action', 'value', 'reward', 'ret', 'length', 'outcome'):
            setattr(ring, k, getattr(self, k).data_ptr())
        if per_player:
            ring.tmask, ring.omask = self.tmask.data_ptr(), self.omask.data_ptr()
            layout = 'players_mover' if mover else ('players_all' if players is None else 'players_solo')
        else:
            ring.turn = self.turn.data_ptr()
            layout = 'mover_records'
        batch = _native.ReplayBatch()
        for l, t in enumerate(dst):
            batch.obs[l] = t.data_ptr()
        for k, key in (('policy', 'policy'), ('amask', 'action_mask'), ('action', 'action'), ('value', 'value'),
                       ('outcome', 'outcome'), ('reward', 'reward'), ('ret', 'return'),
                       ('episode_mask', 'episode_mask'), ('turn_mask', 'turn_mask'),
                       ('observation_mask', 'observation_mask'), ('progress', 'progress')):
            setattr(batch, k, out[key].data_ptr())
        _native.check(_native.load().hrl_replay_gather(
            _native.REPLAY_LAYOUT[layout], ctypes.byref(ring), _native.ptr(slots), _native.ptr(start),
            _native.ptr(players), B, T, ctypes.byref(batch), _native.stream_of(slots.device)), 'hrl_replay_gather')
        return out

    @staticmethod
    def _fill(out, batch):
        """The CPU / torch path of ``out=``: copy the formulation's result into the caller's tensors."""
        if out is None:
            return batch
        for k, v in batch.items():
            bimap_r(out[k], v, lambda dst, s: dst.copy_(s))
        return out

    def gather(self, slots, start, T, out=None):
        """make_batch-layout batch of the windows [start, start+T) of episodes `slots` (train.py:33-133).
        ``out``: a batch dict (``alloc_batch``) that is filled and returned."""
        if FUSED_GATHER and self.policy.is_cuda:
            return self._gather_native(slots, start, T, None, False, out)
        return self._fill(out, self._gather_torch(slots, start, T))

    def _gather_torch(self, slots, start, T):
        B, P, dev = slots.shape[0], self.P, self.device
        t = start.view(-1, 1) + torch.arange(T, device=dev).view(1, -1)      # (B, T)
        length = self.length[slots].view(-1, 1)
        valid = t < length
        tc = torch.minimum(t, length - 1)
        e = slots.view(-1, 1)
        vf = valid.float()
        obs = map_r(self.obs, lambda o: (o[e, tc].float() * vf.view(B, T, *([1] * (o.dim() - 2)))).unsqueeze(2))
        pol = self.policy[e, tc] * vf.unsqueeze(-1)
        amask = torch.where(valid.unsqueeze(-1), self.amask[e, tc], torch.full_like(pol, 1e32))
        act = self.action[e, tc] * valid.long()
        onehot = torch.nn.functional.one_hot(self.turn[e, tc], P).float() * vf.unsqueeze(-1)   # (B,T,P)
        oc = self.outcome[slots].view(B, 1, P, 1)
        val = (onehot * self.value[e, tc].unsqueeze(-1)).unsqueeze(-1)
        val = torch.where(valid.view(B, T, 1, 1), val, oc.expand(B, T, P, 1))
        rew = self.reward[e, tc] * vf.unsqueeze(-1)
        ret = self.ret[e, tc] * vf.unsqueeze(-1)
        progress = torch.where(valid, t.float() / length.float(), torch.ones_like(vf))
        return {
            'observation': obs,
            'policy': pol.unsqueeze(2).contiguous(),
            'value': val.contiguous(),
            'action': act.view(B, T, 1, 1).contiguous(),
            'outcome': oc.contiguous(),
            'reward': rew.unsqueeze(-1).contiguous(),
            'return': ret.unsqueeze(-1).contiguous(),
            'episode_mask': vf.view(B, T, 1, 1).contiguous(),
            'turn_mask': onehot.unsqueeze(-1).contiguous(),
            'observation_mask': onehot.unsqueeze(-1).clone(),
            'action_mask': amask.unsqueeze(2).contiguous(),
            'progress': progress.unsqueeze(-1).contiguous(),
        }

    def sample(self, B, T, generator=None, out=None):
        if self.draw == 'inverse':
            slots, start, _ = self.draw_windows(B, T, generator)
        else:
            slots, start = self.sample_windows(B, T, generator)
        return self.gather(slots, start, T, out=out)


class PlayerReplay(DeviceReplay):
    """DeviceReplay for the per-player episodes (``DeviceGenerator`` with ``observation`` or a simultaneous env):
    records (N, Tm, P, ...) with the turn and observation masks; ``gather`` forms make_batch's per-player layout
    (train.py:63-67, 76-83): every player, or one player per window (``players``, solo training, train.py:55-56),
    zeros / 1e32 / the outcome where a player did not infer or move and past the episode's end.  ``solo``
    (turn_based_training=False) samples one player per window; ``mover`` (turn_based_training without
    observation, e.g. a simultaneous env under the stock configuration) takes observation, policy, action and
    action mask from each ply's first turn player and the rest per player, as make_batch's first branch does
    (train.py:62-66)."""

    _lead = 3

    def __init__(self, capacity, max_plies, obs_shape, A, P, device, maximum_episodes=None,
                 obs_dtype=torch.float32, solo=False, mover=False, draw='multinomial'):
        if draw not in _DRAWS:
            raise ValueError('draw must be one of %s, not %r' % (_DRAWS, draw))
        self.draw = draw
        self.solo, self.mover = bool(solo), bool(mover)
        self.N, self.Tm, self.P, self.device = capacity, max_plies, P, device
        self.maximum_episodes = maximum_episodes or capacity
        f = dict(device=device)
        self.obs = _alloc(obs_shape, (capacity, max_plies, P), device, obs_dtype)
        self.policy = torch.zeros(capacity, max_plies, P, A, **f)
        self.amask = torch.full((capacity, max_plies, P, A), 1e32, **f)
        self.action = torch.zeros(capacity, max_plies, P, dtype=torch.long, **f)
        self.value = torch.zeros(capacity, max_plies, P, **f)
        self.tmask = torch.zeros(capacity, max_plies, P, dtype=torch.bool, **f)
        self.omask = torch.zeros(capacity, max_plies, P, dtype=torch.bool, **f)
        self.reward = torch.zeros(capacity, max_plies, P, **f)
        self.ret = torch.zeros(capacity, max_plies, P, **f)
        self.length = torch.ones(capacity, dtype=torch.long, **f)
        self.outcome = torch.zeros(capacity, P, **f)
        self.ptr = 0
        self.count = 0

    def add(self, ep):
        E = ep['length'].shape[0]
        slots = (self.ptr + torch.arange(E, device=self.device)) % self.N
        bimap_r(self.obs, ep['observation'], lambda dst, src: dst.index_copy_(0, slots, src.to(dst.dtype)))
        for dst, key in ((self.policy, 'policy'), (self.amask, 'action_mask'), (self.action, 'action'),
                         (self.value, 'value'), (self.tmask, 'tmask'), (self.omask, 'omask'),
                         (self.reward, 'reward'), (self.ret, 'return'), (self.length, 'length'),
                         (self.outcome, 'outcome')):
            dst.index_copy_(0, slots, ep[key].to(dst.dtype))
        self.ptr = (self.ptr + E) % self.N
        self.count = min(self.count + E, self.N)

    def _player_axes(self, solo, mover):
        Pn = 1 if solo else self.P
        return (1 if mover else Pn), Pn

    def gather(self, slots, start, T, players=None, mover=None, out=None):
        """make_batch of the windows [start, start+T) of episodes ``slots`` over every player, or over one
        player per window (``players`` (B,) long); ``mover`` (default: the replay's): observation, policy, action
        and action mask of each ply's first turn player.  ``out``: a batch dict (``alloc_batch``) that is filled
        and returned."""
        mover = self.mover if mover is None else mover
        if FUSED_GATHER and self.policy.is_cuda:
            return self._gather_native(slots, start, T, players, bool(mover), out)
        return self._fill(out, self._gather_torch(slots, start, T, players, mover))

    def _gather_torch(self, slots, start, T, players, mover):
        B, dev = slots.shape[0], self.device
        t = start.view(-1, 1) + torch.arange(T, device=dev).view(1, -1)      # (B, T)
        length = self.length[slots].view(-1, 1)
        valid = t < length
        tc = torch.minimum(t, length - 1)
        e = slots.view(-1, 1)
        pidx = (torch.arange(self.P, device=dev).view(1, 1, -1).expand(B, T, self.P) if players is None
                else players.view(B, 1, 1).expand(B, T, 1))
        # make_batch's first branch: m['turn'][0], the lowest-index turn player of the ply
        midx = torch.argmax(self.tmask[e, tc].long(), dim=-1, keepdim=True) if mover else pidx

        def take(x, ix=pidx):   # (N, Tm, P, ...) -> (B, T, Pn, ...)
            y = x[e, tc]
            Pn = ix.shape[2]
            idx = ix.reshape(B, T, Pn, *([1] * (y.dim() - 3))).expand(B, T, Pn, *y.shape[3:])
            return torch.gather(y, 2, idx)
        Pn = pidx.shape[2]
        vf = valid.float()
        vp = vf.view(B, T, 1)
        obs = map_r(self.obs, lambda o: take(o, midx).float() * vp.view(B, T, 1, *([1] * (o.dim() - 3))))
        pol = take(self.policy, midx) * vp.unsqueeze(-1)
        amask = torch.where(valid.view(B, T, 1, 1), take(self.amask, midx), torch.full_like(pol, 1e32))
        act = take(self.action, midx) * valid.long().view(B, T, 1)
        oc = torch.gather(self.outcome[slots], 1, pidx[:, 0]).view(B, 1, Pn, 1)
        val = torch.where(valid.view(B, T, 1, 1), take(self.value).unsqueeze(-1), oc.expand(B, T, Pn, 1))
        rew = take(self.reward) * vp
        ret = take(self.ret) * vp
        tm = take(self.tmask).float() * vp
        om = take(self.omask).float() * vp
        progress = torch.where(valid, t.float() / length.float(), torch.ones_like(vf))
        return {
            'observation': obs,
            'policy': pol.contiguous(),
            'value': val.contiguous(),
            'action': act.unsqueeze(-1).contiguous(),
            'outcome': oc.contiguous(),
            'reward': rew.unsqueeze(-1).contiguous(),
            'return': ret.unsqueeze(-1).contiguous(),
            'episode_mask': vf.view(B, T, 1, 1).contiguous(),
            'turn_mask': tm.unsqueeze(-1).contiguous(),
            'observation_mask': om.unsqueeze(-1).contiguous(),
            'action_mask': amask.contiguous(),
            'progress': progress.unsqueeze(-1).contiguous(),
        }

    def sample(self, B, T, generator=None, out=None):
        """B windows; solo replays: one uniformly chosen player per window (train.py:55-56)."""
        if self.draw == 'inverse':
            slots, start, players = self.draw_windows(B, T, generator)
            players = players if self.solo else None
        else:
            slots, start = self.sample_windows(B, T, generator)
            players = torch.randint(self.P, (B,), device=self.device, generator=generator) if self.solo else None
        return self.gather(slots, start, T, players, out=out)


def player_episodes_to_wire(ep, compress_steps=4):
    """Per-player device episodes -> the reference episode format (generation.py:29-86): a player's observation
    and value where it inferred, its policy / action mask / action where it moved, None elsewhere."""
    import bz2
    import pickle
    cpu = map_r(ep, lambda v: v.cpu().numpy())
    P = cpu['tmask'].shape[2]
    has_reward = bool((cpu['reward'] != 0).any())
    out = []
    for e in range(cpu['length'].shape[0]):
        L = int(cpu['length'][e])
        moments = []
        for t in range(L):
            m = {k: {p: None for p in range(P)} for k in ('observation', 'policy', 'action_mask', 'action',
                                                          'value', 'reward', 'return')}
            for p in range(P):
                if cpu['omask'][e, t, p]:
                    m['observation'][p] = map_r(cpu['observation'], lambda o: o[e, t, p].astype(np.float32))
                    m['value'][p] = np.array([cpu['value'][e, t, p]], dtype=np.float32)
                if cpu['tmask'][e, t, p]:
                    m['policy'][p] = cpu['policy'][e, t, p].astype(np.float32)
                    m['action_mask'][p] = cpu['action_mask'][e, t, p].astype(np.float32)
                    m['action'][p] = int(cpu['action'][e, t, p])
                if has_reward:
                    m['reward'][p] = float(cpu['reward'][e, t, p])
                m['return'][p] = float(cpu['return'][e, t, p])
            m['turn'] = [p for p in range(P) if cpu['tmask'][e, t, p]]
            moments.append(m)
        out.append({'args': {}, 'steps': L, 'outcome': {p: float(cpu['outcome'][e, p]) for p in range(P)},
                    'moment': [bz2.compress(pickle.dumps(moments[i:i + compress_steps]))
                               for i in range(0, L, compress_steps)]})
    return out


def episodes_to_wire(ep, compress_steps=4):
    """Device episodes -> the reference episode format (generation.py:79-86), for parity checks."""
    import bz2
    import pickle
    cpu = map_r(ep, lambda v: v.cpu().numpy())
    has_reward = bool((cpu['reward'] != 0).any())
    out = []
    for e in range(cpu['length'].shape[0]):
        L = int(cpu['length'][e])
        moments = []
        for t in range(L):
            p = int(cpu['turn'][e, t])
            m = {k: {0: None, 1: None} for k in ('observation', 'policy', 'action_mask', 'action', 'value',
                                                    'reward', 'return')}
            m['observation'][p] = map_r(cpu['observation'], lambda o: o[e, t].astype(np.float32))
            m['policy'][p] = cpu['policy'][e, t].astype(np.float32)
            m['action_mask'][p] = cpu['action_mask'][e, t].astype(np.float32)
            m['action'][p] = int(cpu['action'][e, t])
            m['value'][p] = np.array([cpu['value'][e, t]], dtype=np.float32)
            for q in (0, 1):
                if has_reward:
                    m['reward'][q] = float(cpu['reward'][e, t, q])
                m['return'][q] = float(cpu['return'][e, t, q])
            m['turn'] = [p]
            moments.append(m)
        out.append({'args': {}, 'steps': L, 'outcome': {0: float(cpu['outcome'][e, 0]), 1: float(cpu['outcome'][e, 1])},
                    'moment': [bz2.compress(pickle.dumps(moments[i:i + compress_steps]))
                               for i in range(0, L, compress_steps)]})
    return out
