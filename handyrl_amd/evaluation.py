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

A league (``LeagueEvaluator``, ``main.py --eval-league``) plays a round robin of K nets, every pairing's games being
those of the match above, with each net forwarded only over the rows where it moves, and rates the agents with
``bradley_terry``; include/hrl_env.h has its rules.

A simultaneous-move env (Hungry Geese; ParallelTicTacToe at class level) has no mover: ``PlayerEvaluator`` seats the
home net on ``g mod P`` and random agents (``eval_pick_player``) or a second net on ALL other seats, decides for every
player in one launch (hrl_players_act) and restarts a finished slot on the very next step; include/hrl_env.h has its
rules.  ``PlayerEvaluator(..., opponent='rule')``, ``eval_opponent: rulebase`` and ``main.py --eval-rulebase`` seat the
env's rule-based agent on the other seats instead (Hungry Geese: this project's greedy goose,
``envs.geese.greedy_action_of`` -- one more launch per step, hrl_geese_greedy, and the decision through
hrl_players_act_rule): the vs-random win rate on Geese is saturated before training starts.

``FUSED_EVAL``: on a GPU the ply's decision and bookkeeping are the launches of hrl_match_act (the one decision
kernel; hrl_eval_act is its form without an opponent and opening plies), hrl_eval_finish and hrl_masked_rows_fill
(csrc/hrl_eval.hip); the torch formulation below is the CPU path and the form the kernels are tested against.
"""

import contextlib
import functools
import math
import os

import numpy as np
import torch

from .rollout import (_M32, _PHILOX_M, _PHILOX_W, _leaves, _philox_torch, _player_blocks, _stack_views,
                      capture_graphs, eval_mode, graph_wanted, params_key, philox4x32, stream_player_uniforms_torch,
                      stream_select_uniform_torch, stream_uniforms_torch)
from .util import map_r

__all__ = ['DeviceEvaluator', 'eval_pick', 'eval_pick_torch', 'eval_main', 'eval_match_main', 'wp_func', 'eval_games',
           'batched_env', 'LeagueEvaluator', 'bradley_terry', 'eval_league_main', 'PlayerEvaluator', 'eval_pick_player',
           'eval_pick_player_torch', 'player_eval_env', 'rule_eval_env', 'eval_rulebase_main']

# True: on a GPU the three steps are HIP launches; False (or a CPU env): the torch ops below, bit-identical.
FUSED_EVAL = True
# PlayerEvaluator's decision (hrl_players_act; the finish is hrl_eval_finish): True: HIP launches on a GPU; False (or a
# CPU env): players_act_torch and finish_torch.
FUSED_PLAYER_EVAL = True
# The league's own two steps (hrl_league_finish, hrl_rows_permute; csrc/hrl_league.hip) and its use of hrl_match_act
# and hrl_masked_rows_fill: True: HIP launches on a GPU; False (or a CPU env): league_finish_torch, rows_permute_torch.
FUSED_LEAGUE = True

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


def eval_pick_player(seed, game, ply, player, legal):
    """The random agent's move for ``player`` at ply ``ply`` of game number ``game`` in a simultaneous-move env, where
    every player needs a word of its own at one (game, ply): ``eval_pick``'s integer rule on output word
    ``player & 3`` of the Philox call with last counter word ``0xffffffff - (player >> 2)``.  Player 0 is ``eval_pick``
    itself; the words stay apart from the Geese picks (0, 1), ``rollout.stream_player_uniforms`` [0x40000000,
    0x80000000) and ``rollout.stream_select_uniform`` (0x80000000)."""
    seed = int(seed) & 0xffffffffffffffff
    game = int(game) & 0xffffffffffffffff
    player = int(player)
    labels = [a for a, ok in enumerate(legal) if ok]
    x = int(philox4x32((game & _M32, game >> 32, int(ply) & _M32, _PICK_WORD - (player >> 2)),
                       (seed & _M32, seed >> 32))[player & 3])
    return labels[((x >> 9) * len(labels)) >> 23]


def eval_pick_player_torch(seed, game, ply, P, legal):
    """``eval_pick_player`` for E slots and P players as torch ops: game, ply (E,) int64, legal (E, A) or (E, P, A)
    bool -> (E, P) int64 (0 for a row without a legal label)."""
    seed = int(seed) & 0xffffffffffffffff
    E, A = game.shape[0], legal.shape[-1]
    p = torch.arange(P, device=game.device).view(1, P)
    shape = (E, P)
    c = _philox_torch(seed, (game & _M32).view(E, 1).expand(shape), ((game >> 32) & _M32).view(E, 1).expand(shape),
                      (ply & _M32).view(E, 1).expand(shape), (_PICK_WORD - (p >> 2)).expand(shape))
    w = p & 3
    x = torch.where(w == 0, c[0], torch.where(w == 1, c[1], torch.where(w == 2, c[2], c[3])))
    if legal.dim() == 2:
        legal = legal.view(E, 1, A).expand(E, P, A)
    n = legal.sum(-1)
    k = ((x >> 9) * n) >> 23
    hit = legal & (torch.cumsum(legal.long(), -1) == (k + 1).unsqueeze(-1))
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


def player_eval_env(module):
    """The batched twin ``PlayerEvaluator`` plays at the entry points (``eval_rate``, ``--eval``, ``--eval-match``)
    for the env module ``module``: the class marked ``PLAYER_EVAL`` (Hungry Geese), or None -- every other env goes
    through ``batched_env`` and the alternating evaluators."""
    from .main import _batched_envs
    cls = _batched_envs().get(module)
    return cls if getattr(cls, 'PLAYER_EVAL', False) else None


def _check_env(cls, name=None):
    if cls is None:
        raise ValueError('device evaluation needs a batched (device) form of the env; %r has none' % (name,))
    if getattr(cls, 'SIMULTANEOUS', False) or not getattr(cls, 'ALTERNATING', False):
        raise ValueError('device evaluation plays alternating-move envs (TicTacToe, Geister, CIGeister): %s is a '
                         'simultaneous-move env, where every player moves at every ply%s'
                         % (getattr(cls, '__name__', None) or type(cls).__name__,
                            ' (PlayerEvaluator plays it: eval_simultaneous: true in train_args, --eval, --eval-match)'
                            if getattr(cls, 'PLAYER_EVAL', False) else ''))


# ---- the three steps as torch ops (the CPU path; the kernels equal them bit for bit) ----
# Buffers indexed by game number have G + 1 rows: row G takes the stores of the slots that store nothing, so every
# index is in range without a host read (graph-capturable) and no live row is written twice.

def act_torch(st, logits, legal, mover, seed, temperature, G, forced=None, trace=None):
    """hrl_eval_act: the action of every slot, 0 for an inactive one; ``trace`` (dict or None) gets the records."""
    return match_act_torch(st, logits, None, legal, mover, seed, temperature, 0.0, 0, G, forced, trace)


def _act_operands(st, rows, legal, mover, G, forced, trace):
    """What hrl_eval_act and hrl_match_act both take, checked: the logits of ``rows`` (None stays None) as fp32 with
    unit inner stride, ``legal`` contiguous, the action buffer, and the entries' common arguments from ``game`` on."""
    from . import _native
    E, A = legal.shape
    legal = legal.contiguous()
    assert legal.dtype == torch.bool
    rows = list(rows)
    for i, logits in enumerate(rows):
        if logits is not None:
            logits = logits.float()
            if logits.stride(1) != 1:
                logits = logits.contiguous()
            assert logits.shape[0] == E and logits.shape[1] >= A
            rows[i] = logits
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
    tail = [_native.ptr(st['game']), _native.ptr(st['ply']), _native.ptr(st['active']), _native.ptr(st['seat']),
            int(mover), _native.ptr(forced), E, A, Tm, st['P'], G, _native.ptr(a), *[_native.ptr(x) for x in tr],
            _native.stream_of(legal.device)]
    return rows, legal, a, tail


def act_hip(st, logits, legal, mover, seed, temperature, G, forced=None, trace=None):
    """act_torch as ONE launch (the hrl_eval_act entry, one wave per slot)."""
    from . import _native
    (logits,), legal, a, tail = _act_operands(st, [logits], legal, mover, G, forced, trace)
    _native.check(_native.load().hrl_eval_act(
        _native.ptr(logits), logits.stride(0), _native.ptr(legal), int(seed) & 0xffffffffffffffff,
        float(temperature), *tail), 'hrl_eval_act')
    return a


def match_act_torch(st, logits_home, logits_opp, legal, mover, seed, temperature_home, temperature_opp, opening, G,
                    forced=None, trace=None):
    """hrl_match_act, the one decision of every evaluator: the home net where ``seat == mover``, a second net on the
    other seats (``logits_opp`` None: they play ``eval_pick``) and ``opening`` random plies on every seat.  The action
    of every slot, 0 for an inactive one; ``trace`` (dict or None) gets the records."""
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
    (home, opp), legal, a, tail = _act_operands(st, [logits_home, logits_opp], legal, mover, G, forced, trace)
    _native.check(_native.load().hrl_match_act(
        _native.ptr(home), home.stride(0), _native.ptr(opp), 0 if opp is None else opp.stride(0), _native.ptr(legal),
        int(seed) & 0xffffffffffffffff, float(temperature_home), float(temperature_opp), int(opening), *tail),
        'hrl_match_act')
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


def _finish_operands(st, terminal, outcome, rows, outcome_out, length_out):
    """The env's ``terminal`` and ``outcome`` as the finish kernels read them, and the checks both share on them and
    on the two result buffers of at least ``rows`` rows."""
    E, P = st['game'].shape[0], st['P']
    terminal, outcome = terminal.contiguous(), outcome.float().contiguous()
    assert terminal.shape == (E,) and terminal.dtype == torch.bool and outcome.shape == (E, P)
    assert outcome_out.shape[0] >= rows and outcome_out.shape[1] == P and outcome_out.dtype == torch.float32
    assert length_out.shape[0] >= rows and length_out.dtype == torch.long
    assert outcome_out.is_contiguous() and length_out.is_contiguous()
    return terminal, outcome


def finish_hip(st, terminal, outcome, G, outcome_out, length_out):
    """finish_torch as ONE launch of one workgroup (hrl_eval_finish)."""
    from . import _native
    E, P = st['game'].shape[0], st['P']
    terminal, outcome = _finish_operands(st, terminal, outcome, G, outcome_out, length_out)
    assert st['pending'].dtype == torch.bool and st['state'].shape == (2,) and st['state'].dtype == torch.long
    _native.check(_native.load().hrl_eval_finish(
        _native.ptr(terminal), _native.ptr(outcome), E, st['Tm'], P, G, _native.ptr(st['active']),
        _native.ptr(st['ply']), _native.ptr(st['game']), _native.ptr(st['seat']), _native.ptr(st['pending']),
        _native.ptr(st['state']), _native.ptr(outcome_out), _native.ptr(length_out),
        _native.stream_of(terminal.device)), 'hrl_eval_finish')


def players_act_torch(st, logits_home, logits_opp, legal, turns, seed, temperature_home, temperature_opp, opening, G,
                      forced=None, trace=None, rule=None):
    """hrl_players_act, the decision of ``PlayerEvaluator``: every player of every slot in one go.  ``logits_home``
    (E, >= A) and ``logits_opp`` ((P - 1) * E, >= A) or None are relative-seat-major: row (k - 1) * E + e of the
    opponent belongs to player (seat[e] + k) mod P; ``legal`` (E, A) or (E, P, A); ``turns`` (E, P) bool.  Returns the
    actions (E, P) (0 for an inactive slot and for a player that does not move) and the select uniforms (E,);
    ``trace`` (dict or None) gets the records.  ``rule`` (E, P) int64 or None (hrl_players_act_rule; not together with
    ``logits_opp``): a player without a net at ``ply >= opening`` picks rule[e, p] where that is a legal label in
    [0, A), else the random pick as without a rule."""
    game, ply, active, seat = st['game'], st['ply'], st['active'], st['seat']
    E, P = turns.shape
    A, Tm, dev = legal.shape[-1], st['Tm'], turns.device
    if rule is not None and logits_opp is not None:
        raise ValueError('players_act: a rule and a second net are not seated together')
    ok = active & (ply >= 0) & (ply < Tm) & (game >= 0) & (game < G)
    if legal.dim() == 2:
        legal = legal.view(E, 1, A).expand(E, P, A)
    m = torch.where(legal, 0.0, 1e32)
    players = torch.arange(P, device=dev).view(1, P).expand(E, P)
    k = (players - seat.view(E, 1)) % P                                      # the relative seat, >= 0
    home = k == 0
    lg = logits_home[:, :A].float().view(E, 1, A).expand(E, P, A)
    has_net = home
    if logits_opp is not None:
        opp = logits_opp[:, :A].float().reshape(P - 1, E, A)
        rows = torch.arange(E, device=dev).view(E, 1).expand(E, P)
        lg = torch.where(home.unsqueeze(-1), lg, opp[(k - 1).clamp(min=0), rows])
        has_net = torch.ones_like(home)
    p = lg - m
    u = None
    if temperature_home > 0 or (logits_opp is not None and temperature_opp > 0):
        u = stream_player_uniforms_torch(seed, game, ply, P, A)

    def net(temperature):
        v = p
        if temperature > 0:
            v = p * float(np.float32(1.0 / temperature)) - torch.log(-torch.log(u))
        return torch.argmax(v, dim=-1)

    pick = net(temperature_home)
    if logits_opp is not None and temperature_opp != temperature_home:
        pick = torch.where(home, pick, net(temperature_opp))
    rand = eval_pick_player_torch(seed, game, ply, P, legal)
    pick = torch.where(has_net & (ply >= opening).view(E, 1), pick, rand)
    if rule is not None:
        in_range = (rule >= 0) & (rule < A)
        r = torch.where(in_range, rule, 0)
        use = in_range & legal.gather(-1, r.unsqueeze(-1)).squeeze(-1) & ~has_net & (ply >= opening).view(E, 1)
        pick = torch.where(use, r, pick)
    moves = turns & ok.view(E, 1)
    g = torch.where(ok, game, G)
    t = torch.where(ok, ply, 0)
    a = pick
    if forced is not None:
        f = forced[g, t]
        a = torch.where(f >= 0, f, pick)
    a = torch.where(moves, a, 0)
    if trace is not None:
        trace['action'][g, t] = torch.where(moves, a, -1)
        trace['picked'][g, t] = torch.where(moves, pick, -1)
        trace['alive'][g, t] = moves
        trace['policy'][torch.where(moves & has_net, g.view(E, 1), G), t.view(E, 1).expand(E, P), players] = p
    return a, stream_select_uniform_torch(seed, game, ply)


def players_act_hip(st, logits_home, logits_opp, legal, turns, seed, temperature_home, temperature_opp, opening, G,
                    forced=None, trace=None, rule=None, rule_entry=False):
    """players_act_torch as ONE launch (hrl_players_act, one wave per (slot, player); with ``rule``, or with
    ``rule_entry`` and a NULL rule, the same kernel through hrl_players_act_rule)."""
    from . import _native
    E, P = turns.shape
    A, Tm = legal.shape[-1], st['Tm']
    _player_blocks(P, A)
    legal, turns = legal.contiguous(), turns.contiguous()
    assert legal.dtype == torch.bool and legal.shape in ((E, A), (E, P, A)) and turns.dtype == torch.bool
    rows = [logits_home, logits_opp]
    for i, (logits, n) in enumerate(zip(rows, (E, (P - 1) * E))):
        if logits is not None:
            logits = logits.float()
            if logits.stride(1) != 1:
                logits = logits.contiguous()
            assert logits.shape[0] == n and logits.shape[1] >= A
            rows[i] = logits
    for key in ('game', 'ply', 'seat'):
        assert st[key].shape == (E,) and st[key].dtype == torch.long and st[key].is_contiguous()
    assert st['active'].shape == (E,) and st['active'].dtype == torch.bool and st['P'] == P
    if forced is not None:
        assert forced.dtype == torch.long and forced.is_contiguous() and forced.shape[0] >= G
        assert forced.shape[1:] == (Tm, P)
    tr = [None] * 4
    if trace is not None:
        tr = [trace[key] for key in ('action', 'picked', 'policy', 'alive')]
        assert all(x.is_contiguous() and x.shape[0] >= G and x.shape[1:3] == (Tm, P) for x in tr)
        assert tr[0].dtype == tr[1].dtype == torch.long and tr[2].dtype == torch.float32 and tr[2].shape[3] == A
        assert tr[3].dtype == torch.bool
    home, opp = rows
    entry, extra = ('hrl_players_act_rule', [None]) if rule_entry else ('hrl_players_act', [])
    if rule is not None:
        assert rule.shape == (E, P) and rule.dtype == torch.long and rule.is_contiguous()
        assert rule.device == legal.device
        entry, extra = 'hrl_players_act_rule', [_native.ptr(rule)]
    a = torch.empty(E, P, dtype=torch.long, device=legal.device)
    usel = torch.empty(E, device=legal.device)
    _native.check(getattr(_native.load(), entry)(
        _native.ptr(home), home.stride(0), _native.ptr(opp), 0 if opp is None else opp.stride(0), _native.ptr(legal),
        A if legal.dim() == 3 else 0, _native.ptr(turns), int(seed) & 0xffffffffffffffff, float(temperature_home),
        float(temperature_opp), int(opening), _native.ptr(st['game']), _native.ptr(st['ply']),
        _native.ptr(st['active']), _native.ptr(st['seat']), _native.ptr(forced), *extra, E, P, A, Tm, G,
        _native.ptr(a), _native.ptr(usel), *[_native.ptr(x) for x in tr], _native.stream_of(legal.device)), entry)
    return a, usel


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


def league_finish_torch(st, terminal, outcome, G, outcome_out, length_out):
    """hrl_league_finish: ``finish_torch`` with the block rule.  Slot e belongs to block e // S and its next game is
    game + S; the seat is not touched.  ``outcome_out`` (Q * G + 1, P) and ``length_out`` (Q * G + 1,) are indexed by
    block * G + game; the last row takes the stores of the slots that store nothing."""
    game, ply, active, pending, state = (st[k] for k in ('game', 'ply', 'active', 'pending', 'state'))
    Tm, S = st['Tm'], st['S']
    E = game.shape[0]
    ply.add_(active)
    done = active & (terminal | (ply >= Tm))
    block = torch.arange(E, device=game.device) // S
    idx = torch.where(done & (game >= 0) & (game < G), block * G + game, (E // S) * G)
    outcome_out[idx] = outcome.float()
    length_out[idx] = ply
    n = game + S
    again = done & (n < G)
    game.copy_(torch.where(done, torch.where(again, n, G), game))
    ply.masked_fill_(done, 0)
    pending.copy_(torch.where(done, again, pending))
    active.logical_and_(~done)
    state[0:1].add_(done.sum())


def league_finish_hip(st, terminal, outcome, G, outcome_out, length_out):
    """league_finish_torch as ONE launch of one workgroup (hrl_league_finish); the kernel needs no spare row."""
    from . import _native
    E, P, S = st['game'].shape[0], st['P'], st['S']
    assert S >= 2 and S % 2 == 0 and E % S == 0
    terminal, outcome = _finish_operands(st, terminal, outcome, (E // S) * G, outcome_out, length_out)
    for k in ('game', 'ply'):
        assert st[k].shape == (E,) and st[k].dtype == torch.long and st[k].is_contiguous()
    for k in ('active', 'pending'):
        assert st[k].shape == (E,) and st[k].dtype == torch.bool
    assert st['state'].shape == (1,) and st['state'].dtype == torch.long
    _native.check(_native.load().hrl_league_finish(
        _native.ptr(terminal), _native.ptr(outcome), E, S, st['Tm'], P, G, _native.ptr(st['active']),
        _native.ptr(st['ply']), _native.ptr(st['game']), _native.ptr(st['pending']), _native.ptr(st['state']),
        _native.ptr(outcome_out), _native.ptr(length_out), _native.stream_of(terminal.device)), 'hrl_league_finish')


def rows_permute_torch(dst, src, src_index=None, dst_index=None, n=None):
    """Row dst_index[r] of dst[l] = row src_index[r] of src[l], r < n, for every leaf pair; a None index is the
    identity.  ``n`` defaults to the index length."""
    if n is None:
        n = (src_index if src_index is not None else dst_index).shape[0]
    for d, s in zip(dst, src):
        x = s[:n] if src_index is None else s.index_select(0, src_index[:n])
        if dst_index is None:
            d[:n].copy_(x)
        else:
            d.index_copy_(0, dst_index[:n], x)


def rows_permute_hip(dst, src, src_index=None, dst_index=None, n=None):
    """rows_permute_torch in ONE launch for up to 16 fp32 leaves (hrl_rows_permute); leaves (rows, *shape) with
    contiguous rows and any row stride.  The indices are not read here: the caller keeps them in range."""
    from . import _native
    if n is None:
        n = (src_index if src_index is not None else dst_index).shape[0]
    assert len(dst) == len(src)
    for ix in (src_index, dst_index):
        assert ix is None or (ix.dtype == torch.long and ix.is_contiguous() and ix.dim() == 1 and ix.shape[0] >= n)
    F = []
    for d, s in zip(dst, src):
        assert d.is_cuda and d.dtype == torch.float32 and s.dtype == torch.float32 and d.shape[1:] == s.shape[1:]
        assert (src_index is not None or s.shape[0] >= n) and (dst_index is not None or d.shape[0] >= n)
        assert n == 0 or (d[0].is_contiguous() and s[0].is_contiguous())
        F.append(max(1, d[0].numel()) if d.shape[0] else 1)
    _native.check(_native.load().hrl_rows_permute(
        len(dst), _native.ptr_array(dst), _native.i64_array([max(d.stride(0), f) for d, f in zip(dst, F)]),
        _native.ptr_array(src), _native.i64_array([max(s.stride(0), f) for s, f in zip(src, F)]),
        _native.i64_array(F), _native.ptr(src_index), _native.ptr(dst_index), int(n),
        _native.stream_of(dst[0].device)), 'hrl_rows_permute')


def _tally(outcomes):
    """The {outcome: count} table of a list of outcomes, the best outcome first; a draw's -0.0 counts as 0.0."""
    table = {}
    for o in outcomes:
        table[o + 0.0] = table.get(o + 0.0, 0) + 1
    return {k: table[k] for k in sorted(table, reverse=True)}


class _PlyEvaluator:
    """What ``DeviceEvaluator`` and ``LeagueEvaluator`` share: the common arguments, one captured graph per mover
    (``rollout.capture_graphs``), the replay loop that reads the device state every ``check_every`` steps, and the
    nets' eval mode and inference sessions around a call.  A subclass has ``_state()``, ``_begin(st, run)`` (every
    buffer as at the start of a call) and ``_ply(st, run, mover)`` (one global step), and keeps its run in
    ``_run``: {'key', 'G', 'graphs', ...}.  ``_movers(st)`` is the period of the mover (P; 1 where every player moves
    every ply: one graph) and ``_check_env_batch`` what the class can play."""

    _check_env_batch = staticmethod(lambda env_batch: _check_env(type(env_batch)))

    @staticmethod
    def _movers(st):
        return st['P']

    def __init__(self, env_batch, observation, temperature, opening_plies, seed, check_every, graph):
        self._check_env_batch(env_batch)
        if not temperature >= 0:
            raise ValueError('temperature must be >= 0, not %r' % (temperature,))
        if int(opening_plies) < 0:
            raise ValueError('opening_plies must be >= 0, not %r' % (opening_plies,))
        self.env = env_batch
        self.observation, self.temperature = bool(observation), float(temperature)
        self.opening_plies = int(opening_plies)
        self.seed = int(seed) & 0xffffffffffffffff
        self.check_every = max(1, int(check_every or 1))
        self.graph = graph
        self._st = None
        self._run = None      # (key, per-G buffers, graphs) of the last evaluate()

    def _use_graph(self):
        return graph_wanted(self.env.device, self.graph)

    def _capture(self, st, run):
        """One graph per mover, everything of a ply one after another on the capturing stream (no parallel
        branches); warm-up plies run first on a side stream.  ``_play`` starts the call afresh with ``_begin``, so
        warm-up and capture leave no trace."""
        self._begin(st, run)
        return capture_graphs(self.env.device,
                              {m: functools.partial(self._ply, st, run, m) for m in range(self._movers(st))})

    def _play(self, st, run, slots, target, unfinished):
        """Global steps until ``target`` games are finished; ``slots``: the slots one stream of game numbers 0 .. G-1
        is played on; ``unfinished``: the error's text for (target, steps)."""
        G, P, M = run['G'], st['P'], self._movers(st)
        if G == 0:
            return 0
        self._begin(st, run)
        graphs = run['graphs']
        s = 0
        limit = (-(-G // max(1, min(slots, G))) + 1) * (st['Tm'] + P) + self.check_every
        while True:
            for _ in range(self.check_every):
                if graphs is not None:
                    graphs[s % M].replay()
                else:
                    self._ply(st, run, s % M)
                s += 1
            if int(st['state'][0]) >= target:
                return s
            if s > limit:
                raise RuntimeError(unfinished % (target, s))

    @staticmethod
    @contextlib.contextmanager
    def _sessions(nets, inplace):
        """The nets in eval mode and inside their inference sessions (``inplace``, per net: the session advances the
        recurrent state in place); the training modes are put back."""
        with eval_mode(*nets), contextlib.ExitStack() as stack:
            for n, own in zip(nets, inplace):
                if hasattr(n, 'inference_session'):
                    stack.enter_context(n.inference_session(inplace_state=True) if own else n.inference_session())
            yield


class DeviceEvaluator(_PlyEvaluator):
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
        super().__init__(env_batch, observation, temperature, opening_plies, seed, check_every, graph)
        if opponent_temperature is None:
            opponent_temperature = temperature
        if not opponent_temperature >= 0:
            raise ValueError('opponent_temperature must be >= 0, not %r' % (opponent_temperature,))
        if opponent is net:
            raise ValueError('the opponent must be a module of its own (a copy of the net plays a self-match)')
        self.net, self.opponent, self.opponent_temperature = net, opponent, float(opponent_temperature)

    def _nets(self):
        return [self.net] + ([] if self.opponent is None else [self.opponent])

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
        act = match_act_hip if fused else match_act_torch
        a = act(st, out['policy'], None if out_opp is None else out_opp['policy'], env.legal(), mover, self.seed,
                self.temperature, self.opponent_temperature, self.opening_plies, run['G'], run['forced'], run['trace'])
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

    def _prepare(self, st, G, forced, trace):
        """The buffers that depend on G (a captured ply addresses them) and the graphs, kept for the next call with
        the same G, forced / trace choice and parameter addresses."""
        dev = self.env.device
        key = (G, forced is not None, bool(trace), FUSED_EVAL, self._use_graph(), self.opponent is not None,
               self.opening_plies) + params_key(*self._nets())
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
        nets = self._nets()
        with self._sessions(nets, [False] * len(nets)):
            run = self._prepare(st, G, forced, trace)
            plies = self._play(st, run, self.env.E, G, 'evaluation did not finish %d games in %d steps')
        dev = self.env.device
        P = st['P']
        outcome, length = run['outcome'][:G].clone(), run['length'][:G].clone()
        seat = torch.arange(G, device=dev) % P
        mine = outcome[torch.arange(G, device=dev), seat].tolist() if G else []
        results = _tally(mine)
        res = {'outcome': outcome, 'length': length, 'seat': seat, 'results': results, 'win_rate': wp_func(results),
               'games': G, 'plies': plies, 'env_steps': int(length.sum())}
        if self.opponent is not None:
            others = outcome[(torch.arange(P, device=dev) != seat.view(-1, 1))].tolist() if G else []
            res['opponent_results'] = _tally(others)
            res['opponent_win_rate'] = wp_func(res['opponent_results'])
        if run['trace'] is not None:
            res['trace'] = {k: v[:G].clone() for k, v in run['trace'].items()}
        return res

    @torch.no_grad()
    def set_opponent_state(self, state_dict):
        """Copy weights and buffers into the opponent IN PLACE (no tensor is replaced), so the captured graphs, which
        address them, stay valid."""
        self.opponent.load_state_dict(state_dict)


def _check_player_env(env_batch):
    if not getattr(env_batch, 'SIMULTANEOUS', False):
        raise ValueError('PlayerEvaluator plays simultaneous-move envs (Hungry Geese, ParallelTicTacToe), where every '
                         'player moves at every ply: %s is played by DeviceEvaluator' % type(env_batch).__name__)


class PlayerEvaluator(_PlyEvaluator):
    """``DeviceEvaluator`` for simultaneous-move envs (``SIMULTANEOUS``: HungryGeeseBatch, ParallelTicTacToeBatch):
    plays game numbers 0 .. ``games`` - 1, each exactly once, on the E slots of ``env_batch`` by the public rules of
    include/hrl_env.h.  The home net sits on ``seat(g) = g mod P``; every other seat is a uniform random agent
    (``eval_pick_player``; the reference's ``Evaluator.execute`` with ``RandomAgent`` as the default agent,
    evaluation.py:119-136) or, with ``opponent``, a second net (``exec_match`` with one ``Agent`` per seat,
    evaluation.py:64-87) at ``opponent_temperature``; the first ``opening_plies`` plies are random picks on every seat.
    ``opponent='rule'`` seats the env's rule-based agent there instead (``RULE_AGENT``: Hungry Geese's greedy goose,
    ``geese.greedy_action_of``; the reference's ``Evaluator.default_agent`` names a RuleBasedAgent as the other choice):
    only the home seat is forwarded, as against random agents, ``env.greedy_players()`` is one more launch and the
    decision (hrl_players_act_rule) plays its label, or the random agent's pick where the rule has none;
    ``opponent_temperature`` is ignored and an env without ``RULE_AGENT`` raises ``ValueError``.

    What differs from ``DeviceEvaluator``: every player moves every ply, so the ply has no mover and is ONE captured
    graph; a finished slot restarts on the very next step -- through ``env.restart_games(pending, game)`` where the env
    has it (game g IS Geese game number g under the env's seed, so a game depends on (seed, g, actions) only, never on
    the slot), else ``reset_where``; a game runs until the env is terminal, also after the home player is out, and the
    outcome is the env's (Geese: a rank over the final rewards).  One launch (hrl_players_act) decides for every
    player from relative-seat-major logits.  The forward's rows are in relative-seat order too
    (``env.observe_seats(seat, K)``, else ``env.observation`` per relative seat): against random agents K = 1 and only
    the home seat is forwarded (E rows); in a match K = P, rows[:E] feed the home net and rows[E:] the opponent.
    The finish is hrl_eval_finish unchanged.

    A net with recurrent state raises ``ValueError`` (the scope of ``rollout.PlayerStreamGenerator``); there is no
    ``observation`` argument: for a net without state the reference's ``Agent.observe`` does nothing.  Eval mode and
    training modes are put back; no torch generator is drawn from; the host reads the two-word device state every
    ``check_every`` steps and nothing else."""

    _check_env_batch = staticmethod(_check_player_env)

    @staticmethod
    def _movers(st):
        return 1

    def __init__(self, env_batch, net, temperature=0.0, seed=0, check_every=16, graph=None, opponent=None,
                 opponent_temperature=None, opening_plies=0):
        super().__init__(env_batch, False, temperature, opening_plies, seed, check_every, graph)
        if opponent_temperature is None:
            opponent_temperature = temperature
        if not opponent_temperature >= 0:
            raise ValueError('opponent_temperature must be >= 0, not %r' % (opponent_temperature,))
        self.rule = None
        if isinstance(opponent, str):
            # a rule-based agent of the env's own on the other seats (Hungry Geese: the greedy goose)
            if opponent != 'rule':
                raise ValueError("opponent is a module, None or 'rule', not %r" % (opponent,))
            self.rule = getattr(env_batch, 'RULE_AGENT', None)
            if self.rule is None:
                raise ValueError("opponent='rule' needs an env with a rule-based agent (RULE_AGENT: Hungry Geese's "
                                 "greedy goose); %s has none" % type(env_batch).__name__)
            opponent = None
        if opponent is net:
            raise ValueError('the opponent must be a module of its own (a copy of the net plays a self-match)')
        for n in (net, opponent):
            if hasattr(n, 'init_hidden'):
                raise ValueError('PlayerEvaluator plays nets without recurrent state; %s has init_hidden'
                                 % type(n).__name__)
        _player_blocks(env_batch.P, env_batch.A)
        self.net, self.opponent, self.opponent_temperature = net, opponent, float(opponent_temperature)

    def _nets(self):
        return [self.net] + ([] if self.opponent is None else [self.opponent])

    def _state(self):
        if self._st is not None:
            return self._st
        env, E, dev = self.env, self.env.E, self.env.device
        self._st = {'Tm': env.MAX_PLIES, 'P': env.P, 'cuda': torch.device(dev).type == 'cuda',
                    'game': torch.zeros(E, dtype=torch.long, device=dev),
                    'ply': torch.zeros(E, dtype=torch.long, device=dev),
                    'seat': torch.zeros(E, dtype=torch.long, device=dev),
                    'active': torch.zeros(E, dtype=torch.bool, device=dev),
                    'pending': torch.zeros(E, dtype=torch.bool, device=dev),
                    'state': torch.zeros(2, dtype=torch.long, device=dev), 'rows': torch.arange(E, device=dev)}
        return self._st

    def _begin(self, st, run):
        """Every buffer as at the start of a call: slot e waits to start game e (e < G) or is retired; the first step
        starts the games like any later restart."""
        E, G, P = self.env.E, run['G'], st['P']
        rows = st['rows']
        st['game'].copy_(torch.clamp(rows, max=G))
        st['seat'].copy_(torch.where(rows < G, rows % P, 0))
        st['active'].zero_()
        st['pending'].copy_(rows < G)
        st['ply'].zero_()
        st['state'].copy_(torch.tensor([0, min(E, G)], dtype=torch.long))
        run['outcome'].zero_()
        run['length'].zero_()
        if run['trace'] is not None:
            run['trace']['action'].fill_(-1)
            run['trace']['picked'].fill_(-1)
            run['trace']['policy'].zero_()
            run['trace']['alive'].zero_()

    def _rows(self, st, K):
        """The forward's input rows (K * E, ...), relative-seat-major: row k * E + e is the view of player
        (seat[e] + k) mod P."""
        env = self.env
        if hasattr(env, 'observe_seats'):
            return env.observe_seats(st['seat'], K)
        return _stack_views([env.observation((st['seat'] + k) % st['P']) for k in range(K)])

    def _ply(self, st, run, mover=0):
        """One global step: every player of every active slot moves."""
        env, E, P = self.env, self.env.E, st['P']
        fused = FUSED_PLAYER_EVAL and st['cuda']
        active, pending = st['active'], st['pending']
        if hasattr(env, 'restart_games'):
            env.restart_games(pending, st['game'])
        else:
            env.reset_where(pending)
        active.logical_or_(pending)
        pending.zero_()
        turns = (env.turns_mask() & active.view(E, 1)).contiguous()
        out_opp = None
        if self.opponent is None:
            out = self.net(self._rows(st, 1), None)
        else:
            rows = self._rows(st, P)
            out = self.net(map_r(rows, lambda x: x[:E]), None)
            out_opp = self.opponent(map_r(rows, lambda x: x[E:]), None)
        legal = env.legal_players() if hasattr(env, 'legal_players') else env.legal()
        act = players_act_hip if fused else players_act_torch
        # a rule-based opponent: the env's label for every player, one launch; the decision seats it where no net sits
        rule = {} if self.rule is None else {'rule': getattr(env, self.rule)()}
        a, usel = act(st, out['policy'], None if out_opp is None else out_opp['policy'], legal, turns, self.seed,
                      self.temperature, self.opponent_temperature, self.opening_plies, run['G'], run['forced'],
                      run['trace'], **rule)
        env.step_players(a, turns, active, usel)
        finish = finish_hip if fused else finish_torch
        finish(st, env.terminal(), env.outcome(), run['G'], run['outcome'], run['length'])

    def _prepare(self, st, G, forced, trace):
        """The buffers that depend on G (the captured ply addresses them) and the graph, kept for the next call with
        the same G, forced / trace choice and parameter addresses."""
        dev = self.env.device
        key = (G, forced is not None, bool(trace), FUSED_PLAYER_EVAL, self._use_graph(),
               'rule' if self.rule is not None else self.opponent is not None,
               self.opening_plies) + params_key(*self._nets())
        if self._run is None or self._run['key'] != key:
            Tm, P, A = st['Tm'], st['P'], self.env.A
            run = {'key': key, 'G': G, 'graphs': None, 'forced': None, 'trace': None,
                   'outcome': torch.zeros(G + 1, P, device=dev),
                   'length': torch.zeros(G + 1, dtype=torch.long, device=dev)}
            if forced is not None:
                run['forced'] = torch.full((G + 1, Tm, P), -1, dtype=torch.long, device=dev)
            if trace:
                run['trace'] = {'action': torch.empty(G + 1, Tm, P, dtype=torch.long, device=dev),
                                'picked': torch.empty(G + 1, Tm, P, dtype=torch.long, device=dev),
                                'policy': torch.empty(G + 1, Tm, P, A, device=dev),
                                'alive': torch.empty(G + 1, Tm, P, dtype=torch.bool, device=dev)}
            self._run = run
            if self._use_graph() and G > 0:
                run['graphs'] = self._capture(st, run)
        run = self._run
        if forced is not None:
            forced = torch.as_tensor(forced, dtype=torch.long)
            if (forced.dim() != 3 or forced.shape[0] != G or forced.shape[1] > st['Tm']
                    or forced.shape[2] != st['P']):
                raise ValueError('forced is (games, <= MAX_PLIES, players) int64, not %s' % (tuple(forced.shape),))
            run['forced'].fill_(-1)
            run['forced'][:G, :forced.shape[1]].copy_(forced)
        return run

    @torch.no_grad()
    def evaluate(self, games, forced=None, trace=False):
        """Play game numbers 0 .. games-1.  Returns ``DeviceEvaluator.evaluate``'s dict: 'outcome' (G, P) fp32,
        'length' (G,), 'seat' (G,), 'results' ({the home seat's outcome: count}), 'win_rate', 'games', 'plies' (global
        steps run), 'env_steps'; with an opponent 'opponent_results' / 'opponent_win_rate' over all P - 1 other seats
        of every game; with ``trace`` the records of include/hrl_env.h under 'trace' ('action', 'picked' (G, Tm, P),
        'policy' (G, Tm, P, A), 'alive' (G, Tm, P)).  ``forced`` (G, <= Tm, P) int64: moves >= 0 are played as given,
        -1 leaves the decision here."""
        G = int(games)
        if G < 0:
            raise ValueError('games must be >= 0')
        st = self._state()
        nets = self._nets()
        with self._sessions(nets, [False] * len(nets)):
            run = self._prepare(st, G, forced, trace)
            plies = self._play(st, run, self.env.E, G, 'evaluation did not finish %d games in %d steps')
        dev = self.env.device
        P = st['P']
        outcome, length = run['outcome'][:G].clone(), run['length'][:G].clone()
        seat = torch.arange(G, device=dev) % P
        mine = outcome[torch.arange(G, device=dev), seat].tolist() if G else []
        results = _tally(mine)
        res = {'outcome': outcome, 'length': length, 'seat': seat, 'results': results, 'win_rate': wp_func(results),
               'games': G, 'plies': plies, 'env_steps': int(length.sum())}
        if self.opponent is not None or self.rule is not None:
            others = outcome[(torch.arange(P, device=dev) != seat.view(-1, 1))].tolist() if G else []
            res['opponent_results'] = _tally(others)
            res['opponent_win_rate'] = wp_func(res['opponent_results'])
        if run['trace'] is not None:
            res['trace'] = {k: v[:G].clone() for k, v in run['trace'].items()}
        return res

    @torch.no_grad()
    def set_opponent_state(self, state_dict):
        """Copy weights and buffers into the opponent IN PLACE (no tensor is replaced), so the captured graph, which
        addresses them, stays valid.  A rule-based opponent has no state: ValueError."""
        if self.opponent is None:
            raise ValueError('set_opponent_state needs a net on the other seats; this evaluator seats %s there'
                             % ('the env\'s rule-based agent' if self.rule is not None else 'random agents'))
        self.opponent.load_state_dict(state_dict)


def _connected(K, pairs):
    """Every agent reaches every other over the played pairs."""
    seen, todo = {0}, [0]
    while todo:
        a = todo.pop()
        for i, j in pairs:
            for x, y in ((i, j), (j, i)):
                if x == a and y not in seen:
                    seen.add(y)
                    todo.append(y)
    return len(seen) == K


def bradley_terry(score, games):
    """Ratings of K agents from a cross table, as Elo (400 log10 gamma, mean 0), (K,) fp64.

    ``score[i][j]`` is i's score in its ``games[i][j]`` games against j (a win 1, a draw 1/2).  Every played pair gets
    one virtual drawn game (0.5 to both scores, 1 to the count), so an agent that won or lost everything keeps a finite
    rating.  The Bradley-Terry strengths are fitted on the host in fp64 by the MM iteration
    gamma_i <- W_i / sum_j n_ij / (gamma_i + gamma_j), W_i the agent's total score, every agent updated from the
    previous sweep's strengths, renormalised to geometric mean 1 after each sweep, until the largest relative change
    is below 1e-12 (or 10,000 sweeps).  A pairing graph that is not connected has no common scale: ValueError."""
    s = torch.as_tensor(score, dtype=torch.float64).cpu().clone()
    n = torch.as_tensor(games, dtype=torch.float64).cpu().clone()
    K = s.shape[0]
    if s.shape != (K, K) or n.shape != (K, K):
        raise ValueError('score and games are (K, K) tables, not %s and %s' % (tuple(s.shape), tuple(n.shape)))
    n.fill_diagonal_(0)
    s.fill_diagonal_(0)
    n = torch.maximum(n, n.t())
    played = n > 0
    pairs = [(i, j) for i in range(K) for j in range(i + 1, K) if bool(played[i, j])]
    if K < 1 or not _connected(K, pairs):
        raise ValueError('the pairings do not connect every agent to every other: the ratings have no common scale')
    s = s + 0.5 * played
    n = n + played
    W = s.sum(1)
    gamma = torch.ones(K, dtype=torch.float64)
    for _ in range(10000):
        new = W / (n / (gamma.view(-1, 1) + gamma.view(1, -1))).sum(1) if K > 1 else gamma.clone()
        new = new / torch.exp(torch.log(new).mean())
        change = float(((new - gamma).abs() / gamma).max())
        gamma = new
        if change < 1e-12:
            break
    elo = 400.0 * torch.log10(gamma)
    return elo - elo.mean()


class LeagueEvaluator(_PlyEvaluator):
    """A round robin of K nets on the E slots of ``env_batch`` (an alternating env with two players): every pairing
    (i, j) plays ``games`` games, and game g of the pairing is the game g that
    ``DeviceEvaluator(env, nets[i], opponent=nets[j], observation=, temperature=, opening_plies=, seed=)`` plays.

    ``pairings``: None is every (i, j) with i < j in lexicographic order, or a list of pairs (i != j, each unordered
    pair once); the first agent of a pair is its home agent, on seat g mod 2 of game g.  Pairing q owns the S = E / Q
    slots from q * S; S is even, so slot t of a block always seats the home agent on t mod 2 and plays the game numbers
    t, t + S, ... below G.  The rows where a net moves at a mover parity are therefore fixed for the run: each ply the
    observation leaves go into net-major order in one launch (hrl_rows_permute), each net runs once over its own
    rows only (E rows in all; with ``observation=True`` every net runs over every slot it sits in, from its own seat:
    2 E rows), the logits return to slot order in one launch and hrl_match_act decides as in a match, both logit
    pointers at the one buffer.  A net keeps one recurrent-state row per slot it sits in, its rows of one seat
    contiguous: the rows it moves on are a view that the net advances (GeisterNet in place inside its session), the
    rows of a restarting slot are zeroed.  On a GPU each mover's ply is one captured graph, the K forwards one after
    another on one stream.  Eval mode, inference sessions and training modes are put back; no torch generator is drawn
    from; the host reads the one-word device state every ``check_every`` steps and nothing else.
    """

    def __init__(self, env_batch, nets, pairings=None, observation=False, temperature=0.0, opening_plies=0, seed=0,
                 check_every=16, graph=None):
        super().__init__(env_batch, observation, temperature, opening_plies, seed, check_every, graph)
        if env_batch.P != 2:
            raise ValueError('a league seats two nets per game: %s has %d players'
                             % (type(env_batch).__name__, env_batch.P))
        nets = list(nets)
        K = len(nets)
        if K < 2:
            raise ValueError('a league needs at least two nets, not %d' % K)
        if len({id(n) for n in nets}) != K:
            raise ValueError('every agent must be a module of its own (a copy of a net plays against it)')
        if pairings is None:
            pairings = [(i, j) for i in range(K) for j in range(i + 1, K)]
        pairings = [(int(i), int(j)) for i, j in pairings]
        for i, j in pairings:
            if not (0 <= i < K and 0 <= j < K) or i == j:
                raise ValueError('a pairing is (i, j) with i != j, both agents in 0 .. %d, not %r' % (K - 1, (i, j)))
        if len({frozenset(p) for p in pairings}) != len(pairings) or not pairings:
            raise ValueError('each unordered pair of agents may appear once in the pairings, and one at least')
        if not _connected(K, pairings):
            raise ValueError('the pairings do not connect every agent to every other: the ratings have no common '
                             'scale')
        Q = len(pairings)
        if env_batch.E <= 0 or env_batch.E % (2 * Q) != 0:
            raise ValueError('env_batch.E must be a positive multiple of 2Q = %d (Q = %d pairings, an even number of '
                             'slots each), not %d' % (2 * Q, Q, env_batch.E))
        self.nets, self.pairings = nets, pairings
        self.K, self.Q, self.S = K, Q, env_batch.E // Q

    def _layout(self):
        """The fixed routes.  rows[k][s]: the slots where agent k sits on seat s, ascending.  Net-major order is agent
        by agent; without observation, at mover m, agent k's rows are rows[k][m]; with it, rows[k][0] then rows[k][1]
        at both movers (the state's own layout)."""
        K, S, E = self.K, self.S, self.env.E
        rows = [([], []) for _ in range(K)]
        for e in range(E):
            (i, j), t = self.pairings[e // S], e % S
            rows[i][t % 2].append(e)
            rows[j][1 - t % 2].append(e)
        lay = {'rows': rows, 'count': [len(r[0]) + len(r[1]) for r in rows], 'total': E}
        # the movers' rows at mover m, agent by agent (the order of the logits, in both modes), and its inverse
        lay['span'], lay['order'], lay['back'] = [[], []], [[], []], [[0] * E, [0] * E]
        for m in (0, 1):
            off = 0
            for k in range(K):
                lay['span'][m].append((off, off + len(rows[k][m])))
                for e in rows[k][m]:
                    lay['order'][m].append(e)
                    lay['back'][m][e] = off
                    off += 1
            assert off == E
        if self.observation:
            # one order for both movers: agent k's block is [its seat-0 slots, its seat-1 slots] (its state's layout)
            lay['span'] = [[], []]
            lay['seat_src'], lay['seat_dst'] = [[], []], [[], []]
            off = 0
            for k in range(K):
                for m in (0, 1):
                    lay['span'][m].append((off, off + lay['count'][k]))
                for s in (0, 1):
                    for e in rows[k][s]:
                        lay['seat_src'][s].append(e)
                        lay['seat_dst'][s].append(off)
                        off += 1
            lay['total'] = off
        return lay

    def _state(self):
        if self._st is not None:
            return self._st
        env, E, dev, S = self.env, self.env.E, self.env.device, self.S
        cuda = torch.device(dev).type == 'cuda'
        lay = self._layout()

        def index(values, rows):
            assert all(0 <= v < rows for v in values)     # hrl_rows_permute does not read its indices: checked here
            return torch.tensor(values, dtype=torch.long, device=dev)
        t = torch.arange(E, device=dev) % S
        st = {'Tm': env.MAX_PLIES, 'P': 2, 'S': S, 'cuda': cuda, 'lay': lay, 'slot': t,
              'game': torch.zeros(E, dtype=torch.long, device=dev), 'ply': torch.zeros(E, dtype=torch.long, device=dev),
              'seat': (t % 2).contiguous(), 'active': torch.zeros(E, dtype=torch.bool, device=dev),
              'pending': torch.zeros(E, dtype=torch.bool, device=dev),
              'state': torch.zeros(1, dtype=torch.long, device=dev),
              'views': [torch.full((E,), s, dtype=torch.long, device=dev) for s in (0, 1)],
              'back': [index(b, E) for b in lay['back']],
              'logits': torch.zeros(E, env.A, device=dev)}
        if self.observation:
            st['seat_src'] = [index(x, E) for x in lay['seat_src']]
            st['seat_dst'] = [index(x, lay['total']) for x in lay['seat_dst']]
        else:
            st['order'] = [index(x, E) for x in lay['order']]
        # the observation leaves in net-major order, written by the route every ply
        probe = env.observation(st['views'][0])
        st['obs'] = map_r(probe, lambda x: torch.zeros(lay['total'], *x.shape[1:], dtype=x.dtype, device=dev))
        # one state row per net per slot it sits in: [its seat-0 slots, its seat-1 slots]
        st['hidden'], st['inplace'] = [], []
        for k, net in enumerate(self.nets):
            n = lay['count'][k]              # >= S: the pairings connect every agent
            h, inplace = None, False
            if hasattr(net, 'inference_hidden') and cuda:
                h = map_r(net.inference_hidden(n, 1, dev), lambda x: x[0])
                inplace = hasattr(net, 'inference_session')
            elif hasattr(net, 'init_hidden'):
                h = map_r(net.init_hidden([n]), lambda x: x.to(dev).contiguous())
            st['hidden'].append(h)
            st['inplace'].append(inplace)
        # nets that are the members of one nn.board_inference_group, in its order, without observation: one grouped
        # forward per ply over the spans of the movers' rows (anything else: the loop over the nets)
        group = getattr(self.nets[0], '_group', None)
        st['group'] = None
        if (group is not None and cuda and not self.observation and len(group) == self.K
                and all(n is m for n, m in zip(self.nets, group)) and env.A == 9
                and not isinstance(st['obs'], (dict, list, tuple))):
            st['group'] = group
            st['group_span'] = [[0] + [hi for _, hi in lay['span'][m]] for m in (0, 1)]
        # the slot of every state row, all nets one after another: a restarting slot's rows by one index op
        st['row_slot'] = index([e for k in range(self.K) for s in (0, 1) for e in lay['rows'][k][s]], E)
        self._st = st
        return st

    def _begin(self, st, run):
        """Every buffer as at the start of a call: slot t of every block plays game t (t < G) or is retired."""
        G = run['G']
        self.env.reset()
        st['game'].copy_(torch.clamp(st['slot'], max=G))
        st['active'].copy_(st['slot'] < G)
        st['ply'].zero_()
        st['pending'].zero_()
        st['state'].zero_()
        for h in st['hidden']:
            if h is not None:
                map_r(h, lambda x: x.zero_())
        run['outcome'].zero_()
        run['length'].zero_()

    def _ply(self, st, run, mover):
        """One global step with mover ``mover`` = s % 2."""
        env, lay = self.env, st['lay']
        fused = FUSED_LEAGUE and st['cuda']
        permute = rows_permute_hip if fused else rows_permute_torch
        active, pending = st['active'], st['pending']
        if mover == 0:
            # finished games restart here only, so that s % 2 is the mover of every live game
            env.reset_where(pending)
            if any(h is not None for h in st['hidden']):
                gone, off = pending.index_select(0, st['row_slot']), 0
                for k, h in enumerate(st['hidden']):
                    if h is not None:
                        (rows_fill_hip if fused else rows_fill_torch)(_leaves(h), gone[off:off + lay['count'][k]])
                    off += lay['count'][k]
            active.logical_or_(pending)
            pending.zero_()
        # the route in: the observation leaves into net-major order
        dst = _leaves(st['obs'])
        if self.observation:
            for s in (0, 1):
                permute(dst, _leaves(env.observation(st['views'][s])), st['seat_src'][s], st['seat_dst'][s])
        else:
            permute(dst, _leaves(env.observation(st['views'][mover])), st['order'][mover], None)
        group = st['group']
        if group is not None:
            # every net a member of one board_inference_group: the K forwards as one launch over the net-major rows,
            # its logits straight into the route out
            out = group.forward(st['obs'], st['group_span'][mover])
            permute([st['logits']], [out['policy']], st['back'][mover], None)
        # every net once, over its own rows; its state rows are a view, which it advances
        policies = []
        for k, net in enumerate(self.nets if group is None else ()):
            lo, hi = lay['span'][mover][k]
            h = st['hidden'][k]
            if h is not None and not self.observation:
                half = lay['count'][k] // 2
                h = map_r(h, lambda x: x[mover * half:(mover + 1) * half])
            out = net(map_r(st['obs'], lambda x: x[lo:hi]), h)
            if h is not None:
                for d, x in zip(_leaves(h), _leaves(out['hidden'])):
                    if not (d.data_ptr() == x.data_ptr() and d.stride() == x.stride()):
                        d.copy_(x)
            p = out['policy'][:, :env.A].float()
            if self.observation:      # the rows it moves on: its seat-`mover` half
                half = lay['count'][k] // 2
                p = p[mover * half:(mover + 1) * half]
            policies.append(p)
        # the route out: the movers' logits, agent by agent, back into slot order
        if group is None:
            permute([st['logits']], [torch.cat(policies)], st['back'][mover], None)
        act = match_act_hip if fused else match_act_torch
        a = act(st, st['logits'], st['logits'], env.legal(), mover, self.seed, self.temperature, self.temperature,
                self.opening_plies, run['G'])
        env.step(a, active)
        finish = league_finish_hip if fused else league_finish_torch
        finish(st, env.terminal(), env.outcome(), run['G'], run['outcome'], run['length'])

    def _prepare(self, st, G):
        dev = self.env.device
        key = (G, FUSED_LEAGUE, self._use_graph()) + params_key(*self.nets)
        if self._run is None or self._run['key'] != key:
            rows = self.Q * G + 1
            run = {'key': key, 'G': G, 'graphs': None, 'outcome': torch.zeros(rows, 2, device=dev),
                   'length': torch.zeros(rows, dtype=torch.long, device=dev)}
            self._run = run
            if self._use_graph() and G > 0:
                run['graphs'] = self._capture(st, run)
        return self._run

    @torch.no_grad()
    def evaluate(self, games):
        """Play game numbers 0 .. games-1 of every pairing.  Returns {'pairings': the pairs played; 'outcome'
        (Q, G, 2) fp32 and 'length' (Q, G): per pairing and game; 'score' (K, K) fp64: score[i][j] = the sum of
        (outcome_i + 1) / 2 over i's games against j; 'games' (K, K) counts; 'win_rate' (K,): ``wp_func`` over
        everything the agent played; 'rating' (K,): ``bradley_terry(score, games)``; 'plies' (global steps run),
        'env_steps' (the sum of the lengths)}."""
        G = int(games)
        if G < 0:
            raise ValueError('games must be >= 0')
        st = self._state()
        with self._sessions(self.nets, st['inplace']):
            run = self._prepare(st, G)
            plies = self._play(st, run, self.S, self.Q * G, 'the league did not finish %d games in %d steps')
        K, Q = self.K, self.Q
        outcome = run['outcome'][:Q * G].view(Q, G, 2).clone()
        length = run['length'][:Q * G].view(Q, G).clone()
        o = outcome.cpu().double()
        home = torch.arange(G) % 2
        score = torch.zeros(K, K, dtype=torch.float64)
        count = torch.zeros(K, K, dtype=torch.long)
        played = [[] for _ in range(K)]
        for q, (i, j) in enumerate(self.pairings):
            mine = o[q].gather(1, home.view(-1, 1)).view(-1)
            theirs = o[q].gather(1, (1 - home).view(-1, 1)).view(-1)
            score[i, j] += ((mine + 1) / 2).sum()
            score[j, i] += ((theirs + 1) / 2).sum()
            count[i, j] += G
            count[j, i] += G
            played[i] += mine.tolist()
            played[j] += theirs.tolist()
        win_rate = torch.tensor([wp_func(_tally(o)) for o in played], dtype=torch.float64)
        rating = bradley_terry(score, count) if G > 0 else torch.zeros(K, dtype=torch.float64)
        return {'pairings': list(self.pairings), 'outcome': outcome, 'length': length, 'score': score, 'games': count,
                'win_rate': win_rate, 'rating': rating, 'plies': plies, 'env_steps': int(length.sum())}


def league_paths(argv):
    """The checkpoints of ``--eval-league``: a directory expands to its ``<integer>.pth`` files in ascending epoch
    order, a file is itself; anything else raises FileNotFoundError."""
    paths = []
    for p in argv:
        if os.path.isdir(p):
            epochs = sorted(int(f[:-4]) for f in os.listdir(p) if f.endswith('.pth') and f[:-4].isdigit())
            paths += [os.path.join(p, '%d.pth' % e) for e in epochs if os.path.isfile(os.path.join(p, '%d.pth' % e))]
        elif os.path.isfile(p):
            paths.append(p)
        else:
            raise FileNotFoundError('--eval-league takes checkpoints and directories of <epoch>.pth files: no file %r'
                                    % (p,))
    return paths


def eval_league_main(args, argv, device=None, log=print):
    """``main.py --eval-league MODEL_OR_DIR [MODEL_OR_DIR ...] [NUM_GAMES=100] [SLOTS]``: a round robin of the
    checkpoints in ``env.net()`` (the reference's author answers "which checkpoint is strongest" by hand, looping
    evaluate_best_player.py over saved models one CPU game at a time).  Trailing arguments that are decimal integers
    and not existing paths are NUM_GAMES (per pairing) and SLOTS (in all; default ``eval_slots`` or 1024, rounded down
    to a multiple of 2Q and at least 2Q; a pairing gets no more slots than NUM_GAMES rounded up to even).  train_args
    gives ``observation``, ``eval_temperature``, ``eval_opening_plies`` and ``seed`` as for ``--eval-match``.  Logs one
    line per agent (path, rating, win rate, games) and the cross table (row i, column j: i's win rate against j) and
    returns the evaluator's result."""
    from .environment import make_env, prepare_env
    env_args = args['env_args']
    prepare_env(env_args)
    env = make_env(env_args)
    cls = batched_env(type(env).__module__)
    if cls.P != 2:
        raise ValueError('--eval-league seats two models per game: %s has %d players' % (cls.__name__, cls.P))
    targs = args.get('train_args') or {}
    argv, tail = list(argv), []
    while argv and len(tail) < 2 and argv[-1].isdigit() and not os.path.exists(argv[-1]):
        tail.insert(0, int(argv.pop()))
    paths = league_paths(argv)
    K = len(paths)
    if K < 2:
        raise ValueError('--eval-league needs two checkpoints at least: MODEL_OR_DIR [MODEL_OR_DIR ...] [NUM_GAMES] '
                         '[SLOTS]')
    games = tail[0] if len(tail) >= 1 else 100
    slots = tail[1] if len(tail) >= 2 else int(targs.get('eval_slots') or 1024)
    Q = K * (K - 1) // 2
    S = max(2, min(slots // (2 * Q) * 2, games + games % 2))
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError('handyrl_amd.main evaluates on the GPU (HIP kernels); no GPU is visible')
        device = torch.device('cuda', 0)
    from .nn import configured_inference
    # train_args['inference']: fused -- the nets as one board_inference_group (one launch per ply for all of them)
    nets = configured_inference(targs.get('inference'), [load_net(env, path, device) for path in paths], device)
    log('%d agents, %d pairings, %d slots, %d games per pairing' % (K, Q, Q * S, games))
    ev = LeagueEvaluator(cls(Q * S, device), nets, observation=bool(targs.get('observation', False)),
                         temperature=float(targs.get('eval_temperature', 0.0)), opening_plies=opening_plies(targs),
                         seed=int(targs.get('seed', 0)))
    res = ev.evaluate(games)
    played = res['games'].sum(1).tolist()
    for k, path in enumerate(paths):
        log('agent %d %s rating %+.1f win rate %.3f games %d'
            % (k, path, float(res['rating'][k]), float(res['win_rate'][k]), played[k]))
    log('cross table: row i, column j = the win rate of agent i against agent j')
    log('      ' + ' '.join('%5d' % j for j in range(K)))
    for i in range(K):
        cells = ['    -' if i == j or int(res['games'][i, j]) == 0
                 else '%5.3f' % (float(res['score'][i, j]) / int(res['games'][i, j])) for j in range(K)]
        log('%5d ' % i + ' '.join(cells))
    return res


def eval_main(args, argv, device=None, log=print):
    """``main.py --eval MODEL_PATH [NUM_GAMES=100] [SLOTS]`` (evaluation.py:291-312): the checkpoint in ``env.net()``
    against random agents; logs the result table and win rate in the reference's ``total`` form and returns the
    evaluator's result.  ``env: Geese`` is played by ``PlayerEvaluator`` (the net on seat g mod 4, three random
    agents), env and evaluator under train_args' ``seed``."""
    from .environment import make_env, prepare_env
    env_args = args['env_args']
    prepare_env(env_args)
    env = make_env(env_args)
    players_cls = player_eval_env(type(env).__module__)       # Hungry Geese: every player moves every ply
    cls = players_cls or batched_env(type(env).__module__)
    targs = args.get('train_args') or {}
    model_path = argv[0] if len(argv) >= 1 else os.path.join('models', 'latest.pth')
    games = int(argv[1]) if len(argv) >= 2 else 100
    slots = int(argv[2]) if len(argv) >= 3 else int(targs.get('eval_slots') or 1024)
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError('handyrl_amd.main evaluates on the GPU (HIP kernels); no GPU is visible')
        device = torch.device('cuda', 0)
    from .nn import configured_inference
    net = configured_inference(targs.get('inference'), [load_net(env, model_path, device)], device)[0]
    E = max(1, min(slots, games))
    log('%d slots, %d games' % (E, games))
    if players_cls is not None:
        ev = _player_evaluator(cls, E, device, net, targs)
    else:
        ev = DeviceEvaluator(cls(E, device), net, observation=bool(targs.get('observation', False)),
                             temperature=float(targs.get('eval_temperature', 0.0)), seed=int(targs.get('seed', 0)))
    res = ev.evaluate(games)
    log('total %s %s' % (res['results'], res['win_rate']))
    return res


def _player_evaluator(cls, E, device, net, targs, **match):
    """``PlayerEvaluator`` over ``cls(E, device)`` as the command-line entry points build it: the env's own picks
    (Geese's food) and the evaluator's under train_args' ``seed``, ``eval_temperature`` for every net."""
    seed = int(targs.get('seed', 0))
    env_batch = cls(E, device)
    if hasattr(env_batch, 'seed'):
        env_batch.seed(seed)
    return PlayerEvaluator(env_batch, net, temperature=float(targs.get('eval_temperature', 0.0)), seed=seed, **match)


def rule_eval_env(module):
    """The batched twin ``PlayerEvaluator(opponent='rule')`` plays for the env module ``module`` (``eval_opponent:
    rulebase``, ``--eval-rulebase``): the ``PLAYER_EVAL`` class with a ``RULE_AGENT`` (Hungry Geese).  An env without
    a rule-based agent raises ValueError, naming it."""
    from .main import _batched_envs
    cls = _batched_envs().get(module)
    if not getattr(cls, 'PLAYER_EVAL', False) or getattr(cls, 'RULE_AGENT', None) is None:
        raise ValueError('a rule-based opponent (eval_opponent: rulebase, --eval-rulebase) needs an env with a '
                         'rule-based agent on the device (RULE_AGENT: Hungry Geese, env: Geese); %s has none'
                         % (getattr(cls, '__name__', None) or module,))
    return cls


def eval_rulebase_main(args, argv, device=None, log=print):
    """``main.py --eval-rulebase MODEL_PATH [NUM_GAMES=100] [SLOTS]``: the checkpoint in ``env.net()`` on seat
    ``g mod 4`` against the env's rule-based agent on the three other seats (Hungry Geese: this project's greedy
    goose, ``geese.greedy_action_of`` -- not Kaggle's GreedyAgent move for move).  Logs ``--eval-match``'s tables on
    Geese: per agent ``---agent N---``, a ``default`` line and the ``total`` line; agent 0 is the model, agent 1 the
    rule's three seats.  train_args gives ``eval_temperature``, ``eval_opening_plies`` (default 0 here: the games
    already differ by game number) and ``seed``.  Returns the evaluator's result."""
    from .environment import make_env, prepare_env
    env_args = args['env_args']
    prepare_env(env_args)
    env = make_env(env_args)
    cls = rule_eval_env(type(env).__module__)
    targs = args.get('train_args') or {}
    if len(argv) < 1:
        raise ValueError('--eval-rulebase needs a checkpoint: MODEL_PATH [NUM_GAMES] [SLOTS]')
    games = int(argv[1]) if len(argv) >= 2 else 100
    slots = int(argv[2]) if len(argv) >= 3 else int(targs.get('eval_slots') or 1024)
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError('handyrl_amd.main evaluates on the GPU (HIP kernels); no GPU is visible')
        device = torch.device('cuda', 0)
    from .nn import configured_inference
    net = configured_inference(targs.get('inference'), [load_net(env, argv[0], device)], device)[0]
    E = max(1, min(slots, games))
    log('%d slots, %d games' % (E, games))
    res = _player_evaluator(cls, E, device, net, targs, opponent='rule',
                            opening_plies=int(targs.get('eval_opening_plies') or 0)).evaluate(games)
    for agent, key in enumerate(('results', 'opponent_results')):
        log('---agent %d---' % agent)
        log('default %s %s' % (res[key], wp_func(res[key])))
        log('total %s %s' % (res[key], wp_func(res[key])))
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
    second (``default-S``) and the total, each with its win rate -- and returns the evaluator's result.  ``env: Geese``
    (``PlayerEvaluator``): agent 0 sits on seat ``g mod 4`` and agent 1 on the three other seats; per agent one
    ``default`` line and the ``total`` line (the reference splits -F / -S for two-player games only)."""
    from .environment import make_env, prepare_env
    env_args = args['env_args']
    prepare_env(env_args)
    env = make_env(env_args)
    players_cls = player_eval_env(type(env).__module__)       # Hungry Geese: agent 1 sits on the three other seats
    cls = players_cls or batched_env(type(env).__module__)
    if players_cls is None and cls.P != 2:
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
    from .nn import configured_inference
    # train_args['inference']: fused -- each agent its one-launch forward (the members of a group, used one by one)
    nets = list(configured_inference(targs.get('inference'), [load_net(env, path, device) for path in argv[:2]],
                                     device))
    E = max(1, min(slots, games))
    log('%d slots, %d games' % (E, games))
    if players_cls is not None:
        # more than two players: one `default` pattern per agent, no -F / -S split (evaluation.py:188-192)
        res = _player_evaluator(cls, E, device, nets[0], targs, opponent=nets[1],
                                opening_plies=opening_plies(targs)).evaluate(games)
        for agent, key in enumerate(('results', 'opponent_results')):
            log('---agent %d---' % agent)
            log('default %s %s' % (res[key], wp_func(res[key])))
            log('total %s %s' % (res[key], wp_func(res[key])))
        return res
    ev = DeviceEvaluator(cls(E, device), nets[0], observation=bool(targs.get('observation', False)),
                         temperature=float(targs.get('eval_temperature', 0.0)), seed=int(targs.get('seed', 0)),
                         opponent=nets[1], opening_plies=opening_plies(targs))
    res = ev.evaluate(games)
    outcome, seat = res['outcome'].tolist(), res['seat'].tolist()
    for agent in (0, 1):
        log('---agent %d---' % agent)
        total = []
        for tag, first in (('default-F', 0), ('default-S', 1)):     # agent 0 moves first / second
            mine = [outcome[g][seat[g] if agent == 0 else 1 - seat[g]] for g in range(games) if seat[g] == first]
            total += mine
            if mine:
                log('%s %s %s' % (tag, _tally(mine), wp_func(_tally(mine))))
        log('total %s %s' % (_tally(total), wp_func(_tally(total))))
    return res
