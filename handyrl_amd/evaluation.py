"""Device evaluation: the greedy model against random agents, the reference's win rate.

The reference evaluates every epoch with its greedy ``Agent`` on one seat and ``RandomAgent`` on the others
(train.py:519-526, evaluation.py:119-136, agent.py:13-19, 55-110) and has ``main.py --eval MODEL N``
(evaluation.py:291-312); each game is one process stepping one env with batch-1 CPU inference.  Here
``DeviceEvaluator`` plays exactly G such games on E slots of a batched env: one forward per global step for every
slot, finished games restart in place, and only the result of a game is kept.

The rules are public (include/hrl_env.h spells them out; the kernels reproduce them bit for bit):

* games are counted by NUMBER: 0 .. G-1 are each played once; slot e starts game e, a finished slot takes
  ``next_game + r`` (r = done slots below it in slot order) and a slot whose number would be >= G is retired.
  Counting the first G games to finish instead would bias the sample toward short games;
* ``seat(g) = g mod P`` is the model's seat in game g (balanced like evaluation.py:179-187 and train.py:583);
* the mover of global step s is ``s mod P`` in every live game, so a slot restarts only at a step with
  ``s mod P == 0`` (as in ``rollout.StreamGenerator``) and one captured graph per mover serves every step;
* the random seats play ``eval_pick(seed, game, ply, legal)``;
* the model seat plays the argmax of its masked logits (ties to the lowest label) or, at a temperature, Gumbel-max
  over ``p / temperature`` with ``rollout.stream_uniforms(seed, game, ply, A)``.

A match of two nets (``DeviceEvaluator(..., opponent=)``, ``main.py --eval-match A B``, ``eval_opponent`` in
train_args) seats a second net on the other seats, as the reference's ``exec_match`` seats one ``Agent`` per model
(evaluation.py:64-116); the vs-random win rate saturates within a few epochs, a match against a checkpoint does not.
Each agent has its own temperature, and the first ``opening_plies`` plies of a game are ``eval_pick`` on every seat.

``FUSED_EVAL``: on a GPU the ply's decision and bookkeeping are the launches of hrl_eval_act (hrl_match_act in a
match), hrl_eval_finish and hrl_masked_rows_fill (csrc/hrl_eval.hip); the torch formulation below is the CPU path and
the form the kernels are tested against.
"""

import contextlib
import math
import os

import numpy as np
import torch

from .rollout import _M32, _PHILOX_M, _PHILOX_W, _leaves, philox4x32, stream_uniforms_torch
from .util import map_r

__all__ = ['DeviceEvaluator', 'eval_pick', 'eval_pick_torch', 'eval_main', 'eval_match_main', 'wp_func', 'eval_games',
           'batched_env']

# True: on a GPU the three steps are HIP launches; False (or a CPU env): the torch ops below, bit-identical.
FUSED_EVAL = True

_PICK_WORD = 0xffffffff   # the counter's last word: disjoint from stream_uniforms' a // 4 (A <= 2**20)


def eval_pick(seed, game, ply, legal):
    """The random seat's move at ply ``ply`` of game number ``game``: ``legal`` is a sequence of A flags; with n
    legal labels, x = word 0 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (game &
    0xffffffff, game >> 32, ply, 0xffffffff), w = x >> 9 and k = (w * n) >> 23 in integer arithmetic (0 <= k < n
    always; an fp32 floor(u * n) can round up to n), the move is the k-th legal label in ascending order."""
    seed = int(seed) & 0xffffffffffffffff
    game = int(game) & 0xffffffffffffffff
    labels = [a for a, ok in enumerate(legal) if ok]
    x = int(philox4x32((game & _M32, game >> 32, int(ply) & _M32, _PICK_WORD), (seed & _M32, seed >> 32))[0])
    return labels[((x >> 9) * len(labels)) >> 23]


def _pick_words_torch(seed, game, ply):
    """w = x >> 9 of ``eval_pick`` for E slots: 32-bit words held in int64 (``rollout.stream_uniforms_torch``)."""
    seed = int(seed) & 0xffffffffffffffff
    c0, c1, c2 = game & _M32, (game >> 32) & _M32, ply & _M32
    c3 = torch.full_like(c0, _PICK_WORD)
    k0, k1 = seed & _M32, seed >> 32
    for _ in range(10):
        p0, p1 = c0 * _PHILOX_M[0], c2 * _PHILOX_M[1]
        c0, c1, c2, c3 = ((p1 >> 32) & _M32) ^ c1 ^ k0, p1 & _M32, ((p0 >> 32) & _M32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W[0]) & _M32, (k1 + _PHILOX_W[1]) & _M32
    return c0 >> 9


def eval_pick_torch(seed, game, ply, legal):
    """``eval_pick`` for E slots as torch ops: game, ply (E,) int64, legal (E, A) bool -> (E,) int64 (0 for a row
    without a legal label)."""
    n = legal.sum(-1)
    k = (_pick_words_torch(seed, game, ply) * n) >> 23
    hit = legal & (torch.cumsum(legal.long(), -1) == (k + 1).view(-1, 1))
    return hit.long().argmax(-1)


def wp_func(results):
    """The reference's win rate of a {outcome: count} table (evaluation.py:139-144): sum (o + 1) / 2 over games."""
    games = sum(v for k, v in results.items() if k is not None)
    win = sum((k + 1) / 2 * v for k, v in results.items() if k is not None)
    return 0.0 if games == 0 else win / games


def eval_games(eval_rate, update_episodes):
    """Games of one epoch's evaluation (train.py:429-430, 564: the share of episodes the reference's workers spend
    on evaluation, at least update_episodes ** 0.85 of them)."""
    n = int(update_episodes)
    return int(math.ceil(max(float(eval_rate), n ** 0.85 / n) * n))


def batched_env(module):
    """The batched twin the evaluator can play for the env module ``module`` (a ValueError names what is missing)."""
    from .main import _batched_envs
    cls = _batched_envs().get(module)
    _check_env(cls, module)
    return cls


def _check_env(cls, name=None):
    if cls is None:
        raise ValueError('device evaluation needs a batched (device) form of the env; %r has none' % (name,))
    if getattr(cls, 'SIMULTANEOUS', False) or not getattr(cls, 'ALTERNATING', False):
        raise ValueError('device evaluation plays alternating-move envs (TicTacToe, Geister, CIGeister): %s is a '
                         'simultaneous-move env, where every player moves at every ply'
                         % (getattr(cls, '__name__', None) or type(cls).__name__))


# ---- the three steps as torch ops (the CPU path; the kernels equal them bit for bit) ----
# Buffers indexed by game number have G + 1 rows: row G takes the stores of the slots that store nothing, so every
# index is in range without a host read (graph-capturable) and no live row is written twice.

def act_torch(st, logits, legal, mover, seed, temperature, G, forced=None, trace=None):
    """hrl_eval_act: the action of every slot, 0 for an inactive one; ``trace`` (dict or None) gets the records."""
    game, ply, active, seat = st['game'], st['ply'], st['active'], st['seat']
    E, A = legal.shape
    Tm = st['Tm']
    ok = active & (ply >= 0) & (ply < Tm) & (game >= 0) & (game < G)
    m = torch.where(legal, 0.0, 1e32)
    p = logits[:, :A].float() - m
    v = p
    if temperature > 0:
        u = stream_uniforms_torch(seed, game, ply, A)
        v = p * float(np.float32(1.0 / temperature)) - torch.log(-torch.log(u))
    model = seat == mover
    pick = torch.where(model, torch.argmax(v, dim=-1), eval_pick_torch(seed, game, ply, legal))
    g = torch.where(ok, game, G)
    t = torch.where(ok, ply, 0)
    a = pick
    if forced is not None:
        f = forced[g, t]
        a = torch.where(f >= 0, f, pick)
    a = torch.where(ok, a, 0)
    if trace is not None:
        trace['action'][g, t] = a
        trace['picked'][g, t] = pick
        trace['model_ply'][g, t] = model
        trace['policy'][torch.where(model, g, G), t] = p
    return a


def act_hip(st, logits, legal, mover, seed, temperature, G, forced=None, trace=None):
    """act_torch as ONE launch (hrl_eval_act, one wave per slot)."""
    from . import _native
    E, A = legal.shape
    logits = logits.float()
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    legal = legal.contiguous()
    assert logits.shape[0] == E and logits.shape[1] >= A and legal.dtype == torch.bool
    for k in ('game', 'ply', 'seat'):
        assert st[k].shape == (E,) and st[k].dtype == torch.long and st[k].is_contiguous()
    assert st['active'].shape == (E,) and st['active'].dtype == torch.bool
    Tm = st['Tm']
    if forced is not None:
        assert forced.dtype == torch.long and forced.is_contiguous() and forced.shape[0] >= G
        assert forced.shape[1] == Tm
    tr = [None] * 4
    if trace is not None:
        tr = [trace[k] for k in ('action', 'picked', 'policy', 'model_ply')]
        assert all(x.is_contiguous() and x.shape[0] >= G and x.shape[1] == Tm for x in tr)
        assert tr[0].dtype == tr[1].dtype == torch.long and tr[2].dtype == torch.float32 and tr[2].shape[2] == A
        assert tr[3].dtype == torch.bool
    a = torch.empty(E, dtype=torch.long, device=legal.device)
    _native.check(_native.load().hrl_eval_act(
        _native.ptr(logits), logits.stride(0), _native.ptr(legal), int(seed) & 0xffffffffffffffff,
        float(temperature), _native.ptr(st['game']), _native.ptr(st['ply']), _native.ptr(st['active']),
        _native.ptr(st['seat']), int(mover), _native.ptr(forced), E, A, Tm, st['P'], G, _native.ptr(a),
        *[_native.ptr(x) for x in tr], _native.stream_of(legal.device)), 'hrl_eval_act')
    return a


def match_act_torch(st, logits_home, logits_opp, legal, mover, seed, temperature_home, temperature_opp, opening, G,
                    forced=None, trace=None):
    """hrl_match_act: ``act_torch`` with a second net on the other seats (``logits_opp`` None: they play
    ``eval_pick``) and ``opening`` random plies on every seat.  With ``logits_opp`` None and ``opening`` 0 these are
    ``act_torch``'s operations."""
    game, ply, active, seat = st['game'], st['ply'], st['active'], st['seat']
    E, A = legal.shape
    Tm = st['Tm']
    ok = active & (ply >= 0) & (ply < Tm) & (game >= 0) & (game < G)
    m = torch.where(legal, 0.0, 1e32)
    u = None
    if temperature_home > 0 or (logits_opp is not None and temperature_opp > 0):
        u = stream_uniforms_torch(seed, game, ply, A)   # one agent moves at (game, ply): one stream for both

    def net(logits, temperature):
        p = logits[:, :A].float() - m
        v = p
        if temperature > 0:
            v = p * float(np.float32(1.0 / temperature)) - torch.log(-torch.log(u))
        return p, torch.argmax(v, dim=-1)

    home = seat == mover
    rand = eval_pick_torch(seed, game, ply, legal)
    p, pick = net(logits_home, temperature_home)
    has_net = home
    if logits_opp is not None:
        po, ao = net(logits_opp, temperature_opp)
        p, pick = torch.where(home.view(-1, 1), p, po), torch.where(home, pick, ao)
        has_net = torch.ones_like(home)
    pick = torch.where(has_net & (ply >= opening), pick, rand)
    g = torch.where(ok, game, G)
    t = torch.where(ok, ply, 0)
    a = pick
    if forced is not None:
        f = forced[g, t]
        a = torch.where(f >= 0, f, pick)
    a = torch.where(ok, a, 0)
    if trace is not None:
        trace['action'][g, t] = a
        trace['picked'][g, t] = pick
        trace['model_ply'][g, t] = home
        trace['policy'][torch.where(has_net, g, G), t] = p
    return a


def match_act_hip(st, logits_home, logits_opp, legal, mover, seed, temperature_home, temperature_opp, opening, G,
                  forced=None, trace=None):
    """match_act_torch as ONE launch (hrl_match_act, one wave per slot)."""
    from . import _native
    E, A = legal.shape
    legal = legal.contiguous()
    assert legal.dtype == torch.bool
    rows = []
    for logits in (logits_home, logits_opp):
        if logits is not None:
            logits = logits.float()
            if logits.stride(1) != 1:
                logits = logits.contiguous()
            assert logits.shape[0] == E and logits.shape[1] >= A
        rows.append(logits)
    for k in ('game', 'ply', 'seat'):
        assert st[k].shape == (E,) and st[k].dtype == torch.long and st[k].is_contiguous()
    assert st['active'].shape == (E,) and st['active'].dtype == torch.bool
    Tm = st['Tm']
    if forced is not None:
        assert forced.dtype == torch.long and forced.is_contiguous() and forced.shape[0] >= G
        assert forced.shape[1] == Tm
    tr = [None] * 4
    if trace is not None:
        tr = [trace[k] for k in ('action', 'picked', 'policy', 'model_ply')]
        assert all(x.is_contiguous() and x.shape[0] >= G and x.shape[1] == Tm for x in tr)
        assert tr[0].dtype == tr[1].dtype == torch.long and tr[2].dtype == torch.float32 and tr[2].shape[2] == A
        assert tr[3].dtype == torch.bool
    a = torch.empty(E, dtype=torch.long, device=legal.device)
    _native.check(_native.load().hrl_match_act(
        _native.ptr(rows[0]), rows[0].stride(0), _native.ptr(rows[1]), 0 if rows[1] is None else rows[1].stride(0),
        _native.ptr(legal), int(seed) & 0xffffffffffffffff, float(temperature_home), float(temperature_opp),
        int(opening), _native.ptr(st['game']), _native.ptr(st['ply']), _native.ptr(st['active']),
        _native.ptr(st['seat']), int(mover), _native.ptr(forced), E, A, Tm, st['P'], G, _native.ptr(a),
        *[_native.ptr(x) for x in tr], _native.stream_of(legal.device)), 'hrl_match_act')
    return a


def finish_torch(st, terminal, outcome, G, outcome_out, length_out):
    """hrl_eval_finish: plies counted, finished games' results stored by game number, slots restarted or retired."""
    game, ply, active, seat, pending, state = (st[k] for k in ('game', 'ply', 'active', 'seat', 'pending', 'state'))
    Tm, P = st['Tm'], st['P']
    ply.add_(active)
    done = active & (terminal | (ply >= Tm))
    d = done.long()
    r = torch.cumsum(d, 0) - d
    c = d.sum()
    idx = torch.where(done & (game >= 0) & (game < G), game, G)
    outcome_out[idx] = outcome.float()
    length_out[idx] = ply
    n = state[1] + r
    again = done & (n < G)
    game.copy_(torch.where(done, torch.where(again, n, G), game))
    seat.copy_(torch.where(done, torch.where(again, n % P, 0), seat))
    ply.masked_fill_(done, 0)
    pending.copy_(torch.where(done, again, pending))
    active.logical_and_(~done)
    state[0:1].add_(c)
    state[1:2].copy_(torch.clamp(state[1] + c, max=G).view(1))


def finish_hip(st, terminal, outcome, G, outcome_out, length_out):
    """finish_torch as ONE launch of one workgroup (hrl_eval_finish)."""
    from . import _native
    E, P = st['game'].shape[0], st['P']
    terminal, outcome = terminal.contiguous(), outcome.float().contiguous()
    assert terminal.shape == (E,) and terminal.dtype == torch.bool and outcome.shape == (E, P)
    assert outcome_out.shape[0] >= G and outcome_out.shape[1] == P and outcome_out.dtype == torch.float32
    assert length_out.shape[0] >= G and length_out.dtype == torch.long
    assert outcome_out.is_contiguous() and length_out.is_contiguous()
    assert st['pending'].dtype == torch.bool and st['state'].shape == (2,) and st['state'].dtype == torch.long
    _native.check(_native.load().hrl_eval_finish(
        _native.ptr(terminal), _native.ptr(outcome), E, st['Tm'], P, G, _native.ptr(st['active']),
        _native.ptr(st['ply']), _native.ptr(st['game']), _native.ptr(st['seat']), _native.ptr(st['pending']),
        _native.ptr(st['state']), _native.ptr(outcome_out), _native.ptr(length_out),
        _native.stream_of(terminal.device)), 'hrl_eval_finish')


def rows_fill_torch(leaves, mask):
    """Rows e with mask[e] of every leaf (E, ...) become 0."""
    for h in leaves:
        h.masked_fill_(mask.view(-1, *([1] * (h.dim() - 1))), 0)


def rows_fill_hip(leaves, mask):
    """rows_fill_torch in ONE launch over the masked rows only (hrl_masked_rows_fill); leaves (E, *shape) fp32 with
    contiguous rows and any row stride."""
    from . import _native
    E = mask.shape[0]
    assert mask.dtype == torch.bool and mask.is_contiguous()
    for h in leaves:
        assert h.is_cuda and h.dtype == torch.float32 and h.shape[0] == E and (E == 0 or h[0].is_contiguous())
    _native.check(_native.load().hrl_masked_rows_fill(
        len(leaves), _native.ptr_array(leaves), _native.i64_array([h.stride(0) for h in leaves]),
        _native.i64_array([h[0].numel() if E else 1 for h in leaves]), _native.ptr(mask), E,
        _native.stream_of(mask.device)), 'hrl_masked_rows_fill')


class DeviceEvaluator:
    """Plays ``games`` games of ``net`` (``Agent(model, observation, temperature)``, agent.py:55-110) against
    uniform random agents (``RandomAgent``) on the E slots of ``env_batch`` (TicTacToeBatch, GeisterBatch,
    CIGeisterBatch) by the module's public rules.

    Every ply views the board from the model's seat.  A recurrent net keeps ONE state per slot: it advances on the
    rows where the model moves and, with ``observation=True``, also where it watches the opponent move
    (agent.py:102-105); the forward's other rows are computed and discarded.  A restarting slot's state is zeroed.
    On a GPU each mover's ply is a captured HIP graph (``graph=False``: eager), run inside the net's
    ``inference_session`` in eval mode; the training mode is put back.  No torch generator is drawn from and no
    training state is touched.  The host reads the two-word device state every ``check_every`` steps; that read is
    the only synchronisation.

    A match (``exec_match`` with one ``Agent`` per model, evaluation.py:64-116): ``opponent`` is a second net (another
    module object than ``net``) that plays every other seat greedily or at ``opponent_temperature`` (None: the same
    as ``temperature``), and the first ``opening_plies`` plies of every game are ``eval_pick`` moves on every seat:
    two greedy agents on a deterministic env would otherwise play the same two games over and over.  Each ply then
    runs both nets over the E slots (the home net views the board from ``seat``, the opponent from the other seat;
    include/hrl_env.h has the rule for P > 2) and ONE launch of hrl_match_act decides.  There is one recurrent state
    per net per slot; the opponent's advances where the home seat does not move, or with ``observation`` on every
    active row.  The result gains ``opponent_results`` (the {outcome: count} table over every non-home seat) and
    ``opponent_win_rate``.  With the three arguments at their defaults nothing changes.
    """

    def __init__(self, env_batch, net, observation=False, temperature=0.0, seed=0, check_every=16, graph=None,
                 opponent=None, opponent_temperature=None, opening_plies=0):
        _check_env(type(env_batch))
        if not temperature >= 0:
            raise ValueError('temperature must be >= 0, not %r' % (temperature,))
        if opponent_temperature is None:
            opponent_temperature = temperature
        if not opponent_temperature >= 0:
            raise ValueError('opponent_temperature must be >= 0, not %r' % (opponent_temperature,))
        if int(opening_plies) < 0:
            raise ValueError('opening_plies must be >= 0, not %r' % (opening_plies,))
        if opponent is net:
            raise ValueError('the opponent must be a module of its own (a copy of the net plays a self-match)')
        self.env, self.net = env_batch, net
        self.opponent, self.opponent_temperature = opponent, float(opponent_temperature)
        self.opening_plies = int(opening_plies)
        self.observation, self.temperature = bool(observation), float(temperature)
        self.seed = int(seed) & 0xffffffffffffffff
        self.check_every = max(1, int(check_every or 1))
        self.graph = graph
        self._st = None
        self._run = None      # (key, per-G buffers, graphs) of the last evaluate()

    def _use_graph(self):
        dev = torch.device(self.env.device)
        return dev.type == 'cuda' and (self.graph is None or bool(self.graph))

    def _state(self):
        if self._st is not None:
            return self._st
        env, E, dev = self.env, self.env.E, self.env.device
        st = {'Tm': env.MAX_PLIES, 'P': env.P, 'cuda': torch.device(dev).type == 'cuda',
              'game': torch.zeros(E, dtype=torch.long, device=dev), 'ply': torch.zeros(E, dtype=torch.long, device=dev),
              'seat': torch.zeros(E, dtype=torch.long, device=dev),
              'active': torch.zeros(E, dtype=torch.bool, device=dev),
              'pending': torch.zeros(E, dtype=torch.bool, device=dev),
              'state': torch.zeros(2, dtype=torch.long, device=dev), 'rows': torch.arange(E, device=dev),
              'hidden': None, 'hidden_opp': None}
        for key, net in (('hidden', self.net), ('hidden_opp', self.opponent)):
            if hasattr(net, 'inference_hidden') and st['cuda']:
                # the net's stacked layout for one "player": leaf (1, E, ...) -> the slot-major view (E, ...)
                st[key] = map_r(net.inference_hidden(E, 1, dev), lambda h: h[0])
            elif hasattr(net, 'init_hidden'):
                st[key] = map_r(net.init_hidden([E]), lambda h: h.to(dev).contiguous())
        self._st = st
        return st

    def _begin(self, st, run):
        """Every buffer as at the start of a call: slot e plays game e (e < G) or is retired."""
        E, G, P = self.env.E, run['G'], st['P']
        self.env.reset()
        rows = st['rows']
        st['game'].copy_(torch.clamp(rows, max=G))
        st['seat'].copy_(torch.where(rows < G, rows % P, 0))
        st['active'].copy_(rows < G)
        st['ply'].zero_()
        st['pending'].zero_()
        st['state'].copy_(torch.tensor([0, min(E, G)], dtype=torch.long))
        for key in ('hidden', 'hidden_opp'):
            if st[key] is not None:
                map_r(st[key], lambda h: h.zero_())
        run['outcome'].zero_()
        run['length'].zero_()
        if run['trace'] is not None:
            run['trace']['action'].fill_(-1)
            run['trace']['picked'].fill_(-1)
            run['trace']['policy'].zero_()
            run['trace']['model_ply'].zero_()

    def _ply(self, st, run, mover):
        """One global step with mover ``mover`` = s % P."""
        env, hidden, hidden_opp = self.env, st['hidden'], st['hidden_opp']
        fused = FUSED_EVAL and st['cuda']
        active, seat, pending = st['active'], st['seat'], st['pending']
        if mover == 0:
            # finished games restart here only, so that s % P is the mover of every live game
            env.reset_where(pending)
            for h in (hidden, hidden_opp):
                if h is not None:
                    (rows_fill_hip if fused else rows_fill_torch)(_leaves(h), pending)
            active.logical_or_(pending)
            pending.zero_()
        out = self.net(env.observation(seat), hidden)
        out_opp = None
        if self.opponent is not None:
            # the opponent's view: the mover's seat where it moves, else the seat after the home seat
            other = (seat + 1) % st['P']
            opp_seat = other if st['P'] == 2 else torch.where(seat != mover, torch.full_like(seat, mover), other)
            out_opp = self.opponent(env.observation(opp_seat), hidden_opp)
        if out_opp is None and self.opening_plies == 0:
            act = act_hip if fused else act_torch
            a = act(st, out['policy'], env.legal(), mover, self.seed, self.temperature, run['G'], run['forced'],
                    run['trace'])
        else:
            act = match_act_hip if fused else match_act_torch
            a = act(st, out['policy'], None if out_opp is None else out_opp['policy'], env.legal(), mover, self.seed,
                    self.temperature, self.opponent_temperature, self.opening_plies, run['G'], run['forced'],
                    run['trace'])
        # a net's state moves where it played, or (observation) wherever a game is running
        for h, o, mine in ((hidden, out, True), (hidden_opp, out_opp, False)):
            if h is None:
                continue
            adv = active.clone() if self.observation else active & ((seat == mover) == mine)
            dst, src = _leaves(h), _leaves(o['hidden'])
            if fused:
                from .nn import masked_rows_copy_
                masked_rows_copy_(dst, src, adv)
            else:
                for x, nx in zip(dst, src):
                    x.copy_(torch.where(adv.view(-1, *([1] * (nx.dim() - 1))), nx, x))
        env.step(a, active)
        finish = finish_hip if fused else finish_torch
        finish(st, env.terminal(), env.outcome(), run['G'], run['outcome'], run['length'])

    def _capture(self, st, run):
        """One graph per mover; warm-up plies run first on a side stream (library workspaces).  ``_begin`` then
        starts the call afresh, so warm-up and capture leave no trace."""
        dev = torch.device(self.env.device)
        P = st['P']
        self._begin(st, run)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for m in range(P):
                self._ply(st, run, m)
        torch.cuda.current_stream(dev).wait_stream(side)
        graphs, pool = {}, None
        for m in range(P):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                self._ply(st, run, m)
            pool = g.pool()
            graphs[m] = g
        return graphs

    def _prepare(self, st, G, forced, trace):
        """The buffers that depend on G (a captured ply addresses them) and the graphs, kept for the next call with
        the same G, forced / trace choice and parameter addresses."""
        dev = self.env.device
        nets = [self.net] + ([] if self.opponent is None else [self.opponent])
        key = (G, forced is not None, bool(trace), FUSED_EVAL, self._use_graph(), self.opponent is not None,
               self.opening_plies) + tuple(t.data_ptr() for n in nets for t in list(n.parameters()) + list(n.buffers()))
        if self._run is None or self._run['key'] != key:
            Tm, P, A = st['Tm'], st['P'], self.env.A
            run = {'key': key, 'G': G, 'graphs': None, 'forced': None, 'trace': None,
                   'outcome': torch.zeros(G + 1, P, device=dev),
                   'length': torch.zeros(G + 1, dtype=torch.long, device=dev)}
            if forced is not None:
                run['forced'] = torch.full((G + 1, Tm), -1, dtype=torch.long, device=dev)
            if trace:
                run['trace'] = {'action': torch.empty(G + 1, Tm, dtype=torch.long, device=dev),
                                'picked': torch.empty(G + 1, Tm, dtype=torch.long, device=dev),
                                'policy': torch.empty(G + 1, Tm, A, device=dev),
                                'model_ply': torch.empty(G + 1, Tm, dtype=torch.bool, device=dev)}
            self._run = run
            if self._use_graph() and G > 0:
                run['graphs'] = self._capture(st, run)
        run = self._run
        if forced is not None:
            forced = torch.as_tensor(forced, dtype=torch.long)
            if forced.dim() != 2 or forced.shape[0] != G or forced.shape[1] > st['Tm']:
                raise ValueError('forced is (games, <= MAX_PLIES) int64, not %s' % (tuple(forced.shape),))
            run['forced'].fill_(-1)
            run['forced'][:G, :forced.shape[1]].copy_(forced)
        return run

    @torch.no_grad()
    def evaluate(self, games, forced=None, trace=False):
        """Play game numbers 0 .. games-1.  Returns {'outcome' (G, P) fp32, 'length' (G,), 'seat' (G,): per game;
        'results': {the model's outcome: count}, 'win_rate': ``wp_func`` of it, 'games', 'plies' (global steps run),
        'env_steps' (the sum of the lengths)}, and with ``trace`` the four records of include/hrl_env.h under
        'trace'.  ``forced`` (G, Tm) int64: moves >= 0 are played as given, -1 leaves the decision here."""
        G = int(games)
        if G < 0:
            raise ValueError('games must be >= 0')
        st = self._state()
        nets = [self.net] + ([] if self.opponent is None else [self.opponent])
        was_training = [n.training for n in nets]
        try:
            with contextlib.ExitStack() as stack:
                for n in nets:
                    n.eval()
                    if hasattr(n, 'inference_session'):
                        stack.enter_context(n.inference_session())
                run = self._prepare(st, G, forced, trace)
                plies = self._play(st, run)
        finally:
            for n, mode in zip(nets, was_training):
                n.train(mode)
        dev = self.env.device
        P = st['P']
        outcome, length = run['outcome'][:G].clone(), run['length'][:G].clone()
        seat = torch.arange(G, device=dev) % P
        mine = outcome[torch.arange(G, device=dev), seat].tolist() if G else []
        results = {}
        for o in mine:
            o = o + 0.0   # a draw's -0.0 counts as 0.0
            results[o] = results.get(o, 0) + 1
        results = {k: results[k] for k in sorted(results, reverse=True)}
        res = {'outcome': outcome, 'length': length, 'seat': seat, 'results': results, 'win_rate': wp_func(results),
               'games': G, 'plies': plies, 'env_steps': int(length.sum())}
        if self.opponent is not None:
            others = outcome[(torch.arange(P, device=dev) != seat.view(-1, 1))].tolist() if G else []
            table = {}
            for o in others:
                table[o + 0.0] = table.get(o + 0.0, 0) + 1
            res['opponent_results'] = {k: table[k] for k in sorted(table, reverse=True)}
            res['opponent_win_rate'] = wp_func(res['opponent_results'])
        if run['trace'] is not None:
            res['trace'] = {k: v[:G].clone() for k, v in run['trace'].items()}
        return res

    @torch.no_grad()
    def set_opponent_state(self, state_dict):
        """Copy weights and buffers into the opponent IN PLACE (no tensor is replaced), so the captured graphs, which
        address them, stay valid."""
        self.opponent.load_state_dict(state_dict)

    def _play(self, st, run):
        G, P = run['G'], st['P']
        if G == 0:
            return 0
        self._begin(st, run)
        graphs = run['graphs']
        s = 0
        limit = (-(-G // max(1, min(self.env.E, G))) + 1) * (st['Tm'] + P) + self.check_every
        while True:
            for _ in range(self.check_every):
                if graphs is not None:
                    graphs[s % P].replay()
                else:
                    self._ply(st, run, s % P)
                s += 1
            if int(st['state'][0]) >= G:
                return s
            if s > limit:
                raise RuntimeError('evaluation did not finish %d games in %d steps' % (G, s))


def eval_main(args, argv, device=None, log=print):
    """``main.py --eval MODEL_PATH [NUM_GAMES=100] [SLOTS]`` (evaluation.py:291-312): the checkpoint in ``env.net()``
    against random agents; logs the result table and win rate in the reference's ``total`` form and returns the
    evaluator's result."""
    from .environment import make_env, prepare_env
    env_args = args['env_args']
    prepare_env(env_args)
    env = make_env(env_args)
    cls = batched_env(type(env).__module__)
    targs = args.get('train_args') or {}
    model_path = argv[0] if len(argv) >= 1 else os.path.join('models', 'latest.pth')
    games = int(argv[1]) if len(argv) >= 2 else 100
    slots = int(argv[2]) if len(argv) >= 3 else int(targs.get('eval_slots') or 1024)
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError('handyrl_amd.main evaluates on the GPU (HIP kernels); no GPU is visible')
        device = torch.device('cuda', 0)
    net = load_net(env, model_path, device)
    E = max(1, min(slots, games))
    log('%d slots, %d games' % (E, games))
    ev = DeviceEvaluator(cls(E, device), net, observation=bool(targs.get('observation', False)),
                         temperature=float(targs.get('eval_temperature', 0.0)), seed=int(targs.get('seed', 0)))
    res = ev.evaluate(games)
    log('total %s %s' % (res['results'], res['win_rate']))
    return res


def load_net(env, model_path, device):
    """The checkpoint ``model_path`` in ``env.net()()`` on ``device``, HIP-backed on a GPU."""
    net = env.net()()
    net.load_state_dict(torch.load(model_path, map_location='cpu', weights_only=True))
    net = net.to(device)
    if device.type == 'cuda':
        from .nn import accelerate
        accelerate(net)
    return net


def opening_plies(targs):
    """``eval_opening_plies`` of a match (default 2).  Two greedy agents on a deterministic env play the same game
    every time: 0 with ``eval_temperature`` 0 replays two games, one per seating."""
    n = targs.get('eval_opening_plies')
    return 2 if n is None else int(n)


def eval_match_main(args, argv, device=None, log=print):
    """``main.py --eval-match MODEL_A MODEL_B [NUM_GAMES=100] [SLOTS]``: two checkpoints in ``env.net()`` against
    each other (the reference's match of one ``Agent`` per model, evaluation.py:64-116), agent 0 = MODEL_A on seat
    ``g mod 2`` of game g.  train_args gives ``observation``, ``eval_temperature`` (both agents), ``eval_opening_plies``
    and ``seed``.  Logs the reference's ``evaluate_mp`` tables (evaluation.py:233-248) -- per agent the games where
    agent 0 moves first (``default-F``: the even game numbers, (NUM_GAMES + 1) // 2 of them), those where it moves
    second (``default-S``) and the total, each with its win rate -- and returns the evaluator's result."""
    from .environment import make_env, prepare_env
    env_args = args['env_args']
    prepare_env(env_args)
    env = make_env(env_args)
    cls = batched_env(type(env).__module__)
    if cls.P != 2:
        raise ValueError('--eval-match seats two models: %s has %d players' % (cls.__name__, cls.P))
    targs = args.get('train_args') or {}
    if len(argv) < 2:
        raise ValueError('--eval-match needs two checkpoints: MODEL_A MODEL_B [NUM_GAMES] [SLOTS]')
    games = int(argv[2]) if len(argv) >= 3 else 100
    slots = int(argv[3]) if len(argv) >= 4 else int(targs.get('eval_slots') or 1024)
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError('handyrl_amd.main evaluates on the GPU (HIP kernels); no GPU is visible')
        device = torch.device('cuda', 0)
    nets = [load_net(env, path, device) for path in argv[:2]]
    E = max(1, min(slots, games))
    log('%d slots, %d games' % (E, games))
    ev = DeviceEvaluator(cls(E, device), nets[0], observation=bool(targs.get('observation', False)),
                         temperature=float(targs.get('eval_temperature', 0.0)), seed=int(targs.get('seed', 0)),
                         opponent=nets[1], opening_plies=opening_plies(targs))
    res = ev.evaluate(games)
    outcome, seat = res['outcome'].tolist(), res['seat'].tolist()
    for agent in (0, 1):
        log('---agent %d---' % agent)
        total = {}
        for tag, first in (('default-F', 0), ('default-S', 1)):     # agent 0 moves first / second
            table = {}
            for g in range(games):
                if seat[g] == first:
                    o = outcome[g][seat[g] if agent == 0 else 1 - seat[g]] + 0.0
                    table[o] = table.get(o, 0) + 1
                    total[o] = total.get(o, 0) + 1
            if table:
                log('%s %s %s' % (tag, {k: table[k] for k in sorted(table, reverse=True)}, wp_func(table)))
        log('total %s %s' % ({k: total[k] for k in sorted(total, reverse=True)}, wp_func(total)))
    return res
