"""Hungry Geese with rules of this package's own: host plugin env and batched device twin for GeeseNet.

Four geese on a 7 x 11 torus (cell = row * 11 + col); every goose moves every step (NORTH, SOUTH, WEST, EAST,
all wrapping), eats food to grow, loses a cell every 40 steps and dies when it reverses, runs into itself or
shares its head cell with any goose.  The last goose alive, or the longest after 199 steps, wins.

Provenance.  The reference plugin (handyrl/envs/kaggle/hungry_geese.py) holds no rules: it wraps the
``kaggle_environments`` interpreter, which is not available to this project and was not consulted.  ``step_game``
below is this project's restatement of one interpreter step and is the specification of everything else here (the
CPU batch, csrc/hrl_geese.hip, the tests).  What the reference plugin does hold -- ``observation()``,
``outcome()``, ``turns()``, ``terminal()``, ``legal_actions()`` (hungry_geese.py:162-240) -- is pinned to it by
tests/golden/geese_env.*.  Where the restatement decides something itself:

* the interpreter's ``max_length = 99`` trim can never fire on 77 cells and is left out;
* ``last`` is recorded for the geese that were alive when the step began (a dead goose's is never read again);
* food is placed by a public counter-based rule (``geese_picks``) instead of ``random.sample``, so a game depends
  on (seed, game number, actions) only -- never on the slot or the moment it is played.

A game state is a dict: ``geese`` four lists of cells, head first (empty = dead); ``food`` two slots (-1 = none);
``last`` / ``prev`` per goose the last action and the head cell in the previous state (-1 = none); ``reward`` per
goose; ``step``; ``game`` (the game number); ``live``.

``greedy_action_of`` is a rule-based goose of this project's own (modelled on the published behaviour of Kaggle's
``GreedyAgent``, which was not consulted either: no move-for-move parity is claimed), the evaluator's rule-based
opponent; ``rule_based_action``, which names Kaggle's agent, keeps raising.

``envs/hungry_geese.py`` keeps GeeseNet and its ``Environment`` that points to the reference plugin.
"""

import copy
import random

import numpy as np
import torch

from ..environment import BaseEnvironment
from .hungry_geese import GeeseNet

ROWS, COLS = 7, 11
CELLS = ROWS * COLS
GEESE = 4
PLANES = 4 * GEESE + 1
ACTION = ['NORTH', 'SOUTH', 'WEST', 'EAST']
OPPOSITE = (1, 0, 3, 2)
HUNGER = 40
MAX_PLIES = 199     # episodeSteps = 200 states
RING = 80

_M32 = 0xffffffff


def translate(cell, action):
    r, c = divmod(cell, COLS)
    if action == 0:
        r = (r - 1) % ROWS
    elif action == 1:
        r = (r + 1) % ROWS
    elif action == 2:
        c = (c - 1) % COLS
    else:
        c = (c + 1) % COLS
    return r * COLS + c


def _philox(counter, key):
    """Philox4x32-10 on Python ints (rollout.philox4x32 is the array form, csrc/hrl_pick.h the device form)."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def geese_picks(seed, game, step, words=8):
    """The 32-bit words game number ``game`` draws its picks of step ``step`` from: word j is output word j & 3 of
    Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (game & 0xffffffff, game >> 32, step, j >> 2).
    Reset (step 0) places the heads with words 0-3 and the food with words 4-5; a later step respawns food with
    words 0 and 1.  A pick among n free cells is ``pick_index(word, n)``."""
    seed, game = int(seed) & 0xffffffffffffffff, int(game) & 0xffffffffffffffff
    key = (seed & _M32, seed >> 32)
    out = []
    for block in range((words + 3) // 4):
        out += _philox((game & _M32, game >> 32, int(step) & _M32, block), key)
    return out[:words]


def pick_index(word, n):
    """The index among n free cells (ascending) a word picks: (word * n) >> 32, exact in integers."""
    return (word * n) >> 32


def _pick(occupied, word):
    free = [c for c in range(CELLS) if c not in occupied]
    cell = free[pick_index(word, len(free))]
    occupied.add(cell)
    return cell


def new_game(seed, game):
    w = geese_picks(seed, game, 0)
    occupied = set()
    geese = [[_pick(occupied, w[i])] for i in range(GEESE)]
    food = [_pick(occupied, w[4]), _pick(occupied, w[5])]
    return {'geese': geese, 'food': food, 'last': [-1] * GEESE, 'prev': [-1] * GEESE, 'reward': [0] * GEESE,
            'step': 0, 'game': int(game), 'live': True}


def step_game(state, actions, seed=0):
    """One step of one game, in place; ``actions`` one label per goose (a dead goose's is ignored).  Returns the
    events of the step as counts (``ate``, ``reversal``, ``self``, ``hunger``, ``starved``, ``collision``)."""
    ev = dict.fromkeys(('ate', 'reversal', 'self', 'hunger', 'starved', 'collision'), 0)
    s = state['step'] + 1
    geese, food = state['geese'], state['food']
    for i, goose in enumerate(geese):
        if not goose:
            state['prev'][i] = -1
            continue
        state['prev'][i] = goose[0]
        a = int(actions[i]) & 3
        last, state['last'][i] = state['last'][i], a
        if s > 1 and last >= 0 and a == OPPOSITE[last]:
            ev['reversal'] += 1
            goose.clear()
            continue
        h = translate(goose[0], a)
        if h in food:
            food[food.index(h)] = -1
            ev['ate'] += 1
        else:
            goose.pop()
        if h in goose:
            ev['self'] += 1
            goose.clear()
            continue
        goose.insert(0, h)
        if s % HUNGER == 0:
            goose.pop()
            ev['hunger'] += 1
            if not goose:
                ev['starved'] += 1
    count = {}
    for goose in geese:
        for c in goose:
            count[c] = count.get(c, 0) + 1
    for goose in [g for g in geese if g and count[g[0]] > 1]:
        ev['collision'] += 1
        goose.clear()
    occupied = {c for goose in geese for c in goose} | {f for f in food if f >= 0}
    if -1 in food:
        w = geese_picks(seed, state['game'], s, 4)
        j = 0
        for k in range(2):
            if food[k] < 0 and len(occupied) < CELLS:
                food[k] = _pick(occupied, w[j])
                j += 1
    alive = 0
    for i, goose in enumerate(geese):
        if goose:
            state['reward'][i] = s * 100 + len(goose)
            alive += 1
    state['step'] = s
    state['live'] = alive >= 2 and s < MAX_PLIES
    return ev


def observation_of(state, player=0):
    """(17, 7, 11) float32 seen by ``player``: goose i on plane (i - player) % 4 of heads 0-3, tails 4-7, bodies
    8-11 and previous heads 12-15; food on 16 (hungry_geese.py:211-240)."""
    b = np.zeros((PLANES, CELLS), dtype=np.float32)
    for i, goose in enumerate(state['geese']):
        q = (i - player) % GEESE
        if goose:
            b[q, goose[0]] = 1
            b[4 + q, goose[-1]] = 1
            b[8 + q, goose] = 1
        if state['prev'][i] >= 0:
            b[12 + q, state['prev'][i]] = 1
    for f in state['food']:
        if f >= 0:
            b[16, f] = 1
    return b.reshape(PLANES, ROWS, COLS)


def outcome_of(state):
    """Per goose, +1/3 for every goose with a smaller final reward and -1/3 for every one with a larger
    (hungry_geese.py:173-185)."""
    r = state['reward']
    out = [0] * GEESE
    for p in range(GEESE):
        for q in range(GEESE):
            if p != q and r[p] > r[q]:
                out[p] += 1 / (GEESE - 1)
            elif p != q and r[p] < r[q]:
                out[p] -= 1 / (GEESE - 1)
    return out


def turns_of(state):
    return [i for i, goose in enumerate(state['geese']) if goose] if state['live'] else []


GREEDY_ORDER = (0, 3, 1, 2)     # NORTH, EAST, SOUTH, WEST


def greedy_action_of(state, player):
    """The greedy rule-based goose: the label ``player`` plays in ``state``, or -1 (no candidate, or the goose is
    dead; the caller then plays a uniform random label).

    Provenance.  This is THIS PROJECT'S statement of a greedy goose, modelled on the published behaviour of Kaggle's
    ``GreedyAgent`` (what the reference plugin's ``rule_based_action`` calls); ``kaggle_environments`` is not available
    to this project and was not consulted, no move-for-move parity with it is claimed and none can be tested.  The
    function is the specification of ``HungryGeeseBatch.greedy_players`` and of hrl_geese_greedy (csrc/hrl_geese.hip).

    * Blocked cells: every cell of every goose (own cells and tails included) and the four torus neighbours of the
      head of every OTHER living goose.
    * Candidates: the labels in the order NORTH, EAST, SOUTH, WEST (0, 3, 1, 2) whose cell ``translate(head, a)`` is
      not blocked and, once the goose has moved (``last >= 0``), that do not reverse its last action.
    * ``d(a)``: the smallest ``|row - row| + |col - col|`` from that cell to a food cell -- the plain distance on the
      7 x 11 grid, not the torus distance; 0 with no food on the board.
    * The candidate of smallest d, ties to the earliest in the order."""
    geese = state['geese']
    if not geese[player]:
        return -1
    head, last = geese[player][0], state['last'][player]
    blocked = {c for goose in geese for c in goose}
    for i, goose in enumerate(geese):
        if i != player and goose:
            blocked.update(translate(goose[0], a) for a in range(4))
    food = [f for f in state['food'] if f >= 0]
    best, best_d = -1, None
    for a in GREEDY_ORDER:
        c = translate(head, a)
        if c in blocked or (last >= 0 and a == OPPOSITE[last]):
            continue
        d = min((abs(c // COLS - f // COLS) + abs(c % COLS - f % COLS) for f in food), default=0)
        if best_d is None or d < best_d:
            best, best_d = a, d
    return best


class Environment(BaseEnvironment):
    """The host plugin env over ``step_game``.  ``Environment(args)`` takes ``args.get('seed', 0)`` and numbers its
    games 0, 1, ... per instance; there is no ``reward()`` (the base class's empty dict, as in the reference)."""

    SEEDED = True     # main's host generator gives every slot a seed of its own

    def __init__(self, args=None):
        super().__init__()
        self.seed = int((args or {}).get('seed', 0))
        self.games = 0
        self.reset()

    def reset(self, args=None):
        self.state = new_game(self.seed, self.games)
        self.games += 1

    def step(self, actions):
        step_game(self.state, [actions.get(p) or 0 for p in self.players()], self.seed)

    def update(self, info, reset):
        self.state = copy.deepcopy(info)

    def diff_info(self, player=None):
        return copy.deepcopy(self.state)

    def turns(self):
        return turns_of(self.state)

    def terminal(self):
        return not self.state['live']

    def outcome(self):
        return dict(enumerate(outcome_of(self.state)))

    def legal_actions(self, player=None):
        return list(range(len(ACTION)))

    def action_length(self):
        return len(ACTION)

    def players(self):
        return list(range(GEESE))

    def observation(self, player=None):
        return observation_of(self.state, player or 0)

    def action2str(self, a, player=None):
        return ACTION[a]

    def str2action(self, s, player=None):
        return ACTION.index(s)

    def rule_based_action(self, player):
        raise NotImplementedError('the rule-based Hungry Geese agent is GreedyAgent of kaggle_environments '
                                  '(kaggle_environments.envs.hungry_geese), which this package does not have')

    def greedy_action(self, player):
        """This project's greedy goose (``greedy_action_of``; not Kaggle's GreedyAgent move for move): the rule's
        label, or a uniform random legal label where the rule has no candidate."""
        a = greedy_action_of(self.state, player)
        return a if a >= 0 else random.choice(self.legal_actions(player))

    def net(self):
        return GeeseNet

    def __str__(self):
        cells = ['.'] * CELLS
        for f in self.state['food']:
            if f >= 0:
                cells[f] = 'f'
        for i, goose in enumerate(self.state['geese']):
            for c in goose:
                cells[c] = 'abcd'[i]
            if goose:
                cells[goose[0]] = 'ABCD'[i]
        rows = [''.join(cells[r * COLS:(r + 1) * COLS]) for r in range(ROWS)]
        sizes = ' '.join(str(len(goose) or '-') for goose in self.state['geese'])
        return 'step %d\n%s\n%s' % (self.state['step'], '\n'.join(rows), sizes)


_STATE = (('body', np.uint8, (GEESE, RING)), ('head', np.uint8, (GEESE,)), ('length', np.uint8, (GEESE,)),
          ('food', np.int8, (2,)), ('last', np.int8, (GEESE,)), ('prev', np.int8, (GEESE,)),
          ('score', np.int32, (GEESE,)), ('nstep', np.int32, ()), ('game', np.int64, ()), ('live', np.bool_, ()))


def _encode(a, e, state):
    """Game ``state`` into row e of the arrays in the canonical form: ring heads at 0, unused ring bytes 0."""
    a['body'][e] = 0
    for i, goose in enumerate(state['geese']):
        a['body'][e, i, :len(goose)] = goose
        a['head'][e, i] = 0
        a['length'][e, i] = len(goose)
    a['food'][e] = state['food']
    a['last'][e] = state['last']
    a['prev'][e] = state['prev']
    a['score'][e] = state['reward']
    a['nstep'][e], a['game'][e], a['live'][e] = state['step'], state['game'], state['live']


def _decode(a, e):
    geese = []
    for i in range(GEESE):
        h, n = int(a['head'][e, i]), int(a['length'][e, i])
        geese.append([int(a['body'][e, i, (h + k) % RING]) for k in range(n)])
    return {'geese': geese, 'food': [int(x) for x in a['food'][e]], 'last': [int(x) for x in a['last'][e]],
            'prev': [int(x) for x in a['prev'][e]], 'reward': [int(x) for x in a['score'][e]],
            'step': int(a['nstep'][e]), 'game': int(a['game'][e]), 'live': bool(a['live'][e])}


class HungryGeeseBatch:
    """E Hungry Geese games on one device, the env ``DeviceGenerator``'s per-player ply consumes.

    State (allocated once, advanced in place; include/hrl_geese.h): ``body`` (E, 4, 80) uint8 rings with ``head``
    (E, 4) and ``length`` (E, 4) (0 = dead), ``food`` (E, 2) int8, ``last`` / ``prev`` (E, 4) int8, ``score`` (E, 4)
    int32 (the rules' reward), ``nstep`` (E,) int32, ``game`` (E,) int64, ``live`` (E,) bool.  A step writes a ring
    once: a surviving goose's head index steps back by one and the new head is stored there; a dead goose only gets
    length 0.

    On a CPU device every method loops over the games with ``step_game`` / ``observation_of`` (not meant to be fast:
    it is the formulation the kernels are tested against); on a CUDA device reset, step and the four views are one
    launch each of csrc/hrl_geese.hip.  ``reset()`` gives slot e the game number ``next_game + e`` and advances
    ``next_game`` by E; ``seed(s)`` sets the key of the pick rule."""

    A = 4
    P = GEESE
    MAX_PLIES = MAX_PLIES
    OBS_SHAPE = (PLANES, ROWS, COLS)
    SIMULTANEOUS = True
    ALTERNATING = False
    PLAYER_EVAL = True     # evaluation.player_eval_env: the entry points evaluate it with PlayerEvaluator
    RULE_AGENT = 'greedy_players'     # PlayerEvaluator(opponent='rule'): the method that gives every player's label

    def __init__(self, E, device, seed=0):
        self.E, self.device = E, device
        self.next_game = 0
        self.seed(seed)
        self._np = {name: np.zeros((E, *shape), dtype=dt) for name, dt, shape in _STATE}   # host staging / CPU state
        on_cpu = torch.device(device).type == 'cpu'
        for name, _, _ in _STATE:
            t = torch.from_numpy(self._np[name])                   # a CPU batch's tensors ARE the arrays
            setattr(self, name, t if on_cpu else t.to(device))
        self._games = [None] * E                                   # CPU: the games as Python states
        # the reference's sums of +-1/3 over three opponents, by (smaller - larger): exact multiples up to 2/3, then 1
        self._outcomes = torch.tensor([k * (1 / 3) if abs(k) < 3 else k / 3 for k in range(-3, 4)],
                                      dtype=torch.float32, device=device)
        self.reset()

    def seed(self, s):
        self._seed = int(s) & 0xffffffffffffffff

    def _hip(self):
        return self.body.is_cuda

    def state_tensors(self):
        return [getattr(self, name) for name, _, _ in _STATE]

    def _native(self, entry, *args):
        from .._native import load, check, ptr, stream_of
        args = [ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
        check(getattr(load(), entry)(*args, stream_of(self.body.device)), entry)

    def _state_ok(self):
        for (name, dt, shape), t in zip(_STATE, self.state_tensors()):
            assert t.shape == (self.E, *shape) and t.is_contiguous() and t.device == self.body.device, name

    # -- reset / injection
    def reset(self):
        self._reset(None, None, self.E)

    def reset_where(self, mask):
        """reset() for the games of ``mask`` (E,) bool: they get the next game numbers in slot order.  The count
        of new games is read back, so this is not for a captured graph."""
        mask = mask.to(torch.bool).contiguous()
        assert mask.shape == (self.E,)
        self._reset(mask, (torch.cumsum(mask, 0) - 1).contiguous(), int(mask.sum()))

    def _reset(self, mask, rank, count):
        if self._hip():
            self._state_ok()
            self._native('hrl_geese_reset', self.body, self.head, self.length, self.food, self.last, self.prev,
                         self.score, self.nstep, self.game, self.live, mask, rank, self.next_game, self._seed,
                         self.E, self.P)
        else:
            for e in range(self.E):
                if mask is None or bool(mask[e]):
                    self._games[e] = new_game(self._seed, self.next_game + (e if rank is None else int(rank[e])))
                    _encode(self._np, e, self._games[e])
        self.next_game += count

    def restart_games(self, mask, games):
        """Slot e with mask[e] set becomes game number games[e] (both (E,) device tensors: nothing is read on the
        host, so a captured graph may hold this).  ``next_game`` is not touched: the caller numbers the games
        (``rollout.PlayerStreamGenerator``)."""
        mask = mask.to(torch.bool).contiguous()
        games = games.to(torch.long).contiguous()
        assert mask.shape == (self.E,) and games.shape == (self.E,)
        if self._hip():
            self._state_ok()
            self._native('hrl_geese_reset', self.body, self.head, self.length, self.food, self.last, self.prev,
                         self.score, self.nstep, self.game, self.live, mask, games, 0, self._seed, self.E, self.P)
            return
        for e in np.flatnonzero(mask.numpy()):
            self._games[e] = new_game(self._seed, int(games[e]))
            _encode(self._np, e, self._games[e])

    def load_games(self, states, slots):
        """Python game states into the given slots (canonical ring form)."""
        slots = [int(e) for e in slots]
        if self._hip():
            for name, t in zip(self._np, self.state_tensors()):
                self._np[name][...] = t.cpu().numpy()
        for state, e in zip(states, slots):
            _encode(self._np, e, state)
            self._games[e] = copy.deepcopy(state)
        if self._hip():
            for name, t in zip(self._np, self.state_tensors()):
                t.copy_(torch.from_numpy(self._np[name]))

    def dump_games(self):
        """Every slot's game as a Python state, decoded from the tensors."""
        a = {name: t.cpu().numpy() for (name, _, _), t in zip(_STATE, self.state_tensors())}
        return [_decode(a, e) for e in range(self.E)]

    # -- what the ply reads
    def active(self):
        return self.live

    def terminal(self):
        return ~self.live

    def plies(self):
        return self.nstep

    def turn(self):
        return torch.zeros(self.E, dtype=torch.long, device=self.device)

    def turns_mask(self):
        return (self.length > 0) & self.live.view(-1, 1)

    def legal(self):
        return torch.ones(self.E, self.A, dtype=torch.bool, device=self.device)

    def outcome(self):
        """(E, 4) float32: (geese with a smaller reward - geese with a larger) / 3, as the reference sums it."""
        s = self.score
        k = (s.view(-1, GEESE, 1) > s.view(-1, 1, GEESE)).sum(-1) - (s.view(-1, GEESE, 1) < s.view(-1, 1, GEESE)).sum(-1)
        return self._outcomes[k + 3]

    def _views(self, rec=None, t=None, infer=None):
        """(4, E, 17, 7, 11) views, player-major; with ``rec`` (E, Tm, 4, 17, 7, 11) view p of game e also goes to
        slot (e, t, p) where infer[e, p] (t a device scalar)."""
        E = self.E
        if rec is not None:
            infer = infer.to(torch.bool).contiguous()
            assert rec.shape[0] == E and rec.shape[2:] == (GEESE, *self.OBS_SHAPE) and rec.is_contiguous()
            assert rec.dtype == torch.float32 and infer.shape == (E, GEESE) and t.dtype == torch.long
        if self._hip():
            self._state_ok()
            views = torch.empty(GEESE, E, *self.OBS_SHAPE, device=self.device)
            self._native('hrl_geese_observe', self.body, self.head, self.length, self.food, self.prev, views, rec,
                         t, infer, E, self.P, 1 if rec is None else rec.shape[1])
            return views
        views = torch.from_numpy(np.stack([np.stack([observation_of(g, p) for g in self._games])
                                           for p in range(GEESE)]))
        if rec is not None:
            tt = int(t)
            if 0 <= tt < rec.shape[1]:
                keep = infer.view(E, GEESE, 1, 1, 1)
                rec[:, tt] = torch.where(keep, views.transpose(0, 1), rec[:, tt])
        return views

    def observation(self, player):
        """(E, 17, 7, 11): game e seen by goose player[e]."""
        return self._views()[player.long(), torch.arange(self.E, device=self.device)]

    def observe_seats(self, seat, K):
        """The evaluator's forward rows (K * E, 17, 7, 11), relative-seat-major: row k * E + e is game e seen by goose
        (seat[e] + k) mod 4, k < K (``evaluation.PlayerEvaluator``: K = 1 forwards the home seat only, K = 4 feeds
        rows[:E] to the home net and rows[E:] to the opponent).  One launch, nothing recorded."""
        E, K = self.E, int(K)
        seat = seat.to(torch.long).contiguous()
        assert seat.shape == (E,) and 1 <= K <= GEESE
        if self._hip():
            self._state_ok()
            rows = torch.empty(K, E, *self.OBS_SHAPE, device=self.device)
            self._native('hrl_geese_observe_seats', self.body, self.head, self.length, self.food, self.prev, seat,
                         rows, E, self.P, K)
            return rows.view(K * E, *self.OBS_SHAPE)
        rows = np.stack([np.stack([observation_of(g, (int(s) + k) % GEESE) for g, s in zip(self._games, seat.tolist())])
                         for k in range(K)]) if E else np.zeros((K, 0, *self.OBS_SHAPE), dtype=np.float32)
        return torch.from_numpy(rows).view(K * E, *self.OBS_SHAPE)

    def greedy_players(self):
        """(E, 4) int64: ``greedy_action_of`` for every goose of every slot (-1: no candidate, or the goose is dead);
        the evaluator's rule-based opponent (``RULE_AGENT``).  One launch of hrl_geese_greedy on a CUDA batch."""
        if self._hip():
            self._state_ok()
            rule = torch.empty(self.E, GEESE, dtype=torch.long, device=self.device)
            self._native('hrl_geese_greedy', self.body, self.head, self.length, self.food, self.last, rule, self.E,
                         self.P)
            return rule
        return torch.tensor([[greedy_action_of(g, p) for p in range(GEESE)] for g in self._games],
                            dtype=torch.long).view(self.E, GEESE)

    def observe_players_record(self, rec, t, infer):
        """All four views of every game as the forward's (4 * E, 17, 7, 11) input rows, player-major, and in the
        same launch the observation record of slot t for the (game, player) pairs of ``infer``."""
        return self._views(rec, t, infer).view(GEESE * self.E, *self.OBS_SHAPE)

    def observe_players_record_at(self, rec, ply, infer, active):
        """``observe_players_record`` for the streaming generator: game e records at its own ply index ply[e] into
        the UINT8 record ``rec`` (E, Tm, 4, 17, 7, 11).  An ``active`` game with ply[e] in [0, Tm) gets view p in
        slot (e, ply[e], p) where infer[e, p] and zeros where not (the slot buffers outlive a game: a dead goose's
        slot must not keep an earlier game's planes); any other game stores nothing.  Returns the forward's
        (4 * E, 17, 7, 11) fp32 input rows, player-major, for every game."""
        E = self.E
        infer, active = infer.to(torch.bool).contiguous(), active.to(torch.bool).contiguous()
        assert rec.shape[0] == E and rec.shape[2:] == (GEESE, *self.OBS_SHAPE) and rec.is_contiguous()
        assert rec.dtype == torch.uint8 and infer.shape == (E, GEESE) and active.shape == (E,)
        assert ply.shape == (E,) and ply.dtype == torch.long and ply.is_contiguous()
        if self._hip():
            self._state_ok()
            views = torch.empty(GEESE, E, *self.OBS_SHAPE, device=self.device)
            self._native('hrl_geese_observe_at', self.body, self.head, self.length, self.food, self.prev, views, rec,
                         ply, infer, active, E, self.P, rec.shape[1])
            return views.view(GEESE * E, *self.OBS_SHAPE)
        views = self._views()
        for e in np.flatnonzero(active.numpy()):
            t = int(ply[e])
            if 0 <= t < rec.shape[1]:
                for p in range(GEESE):
                    rec[e, t, p] = views[p, e].to(torch.uint8) if bool(infer[e, p]) else 0
        return views.view(GEESE * E, *self.OBS_SHAPE)

    def views_torch(self):
        """``_views()`` as batched torch ops on the state tensors: the formulation tools/geese_selfplay_bench.py
        times the observe kernel against."""
        E, dev = self.E, self.body.device
        k = torch.arange(RING, device=dev)
        cells = torch.gather(self.body.long(), 2, (self.head.long().unsqueeze(-1) + k) % RING)      # head first
        valid = k < self.length.long().unsqueeze(-1)
        whole = torch.zeros(E, GEESE, CELLS, device=dev).scatter_add_(2, cells, valid.float()).clamp_(max=1)
        alive = (self.length > 0).float().unsqueeze(-1)
        one = torch.nn.functional.one_hot
        heads = one(cells[:, :, 0], CELLS).float() * alive
        tail = torch.gather(cells, 2, (self.length.long() - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1)
        tails = one(tail, CELLS).float() * alive
        prev = one(self.prev.long().clamp(min=0), CELLS).float() * (self.prev >= 0).float().unsqueeze(-1)
        food = (one(self.food.long().clamp(min=0), CELLS).float() * (self.food >= 0).float().unsqueeze(-1)).sum(1)
        groups = torch.stack([heads, tails, whole, prev], 1)                                      # (E, 4, goose, 77)
        views = [torch.cat([torch.roll(groups, -p, 2).reshape(E, 4 * GEESE, CELLS), food.view(E, 1, CELLS)], 1)
                 for p in range(GEESE)]
        return torch.stack(views).view(GEESE, E, *self.OBS_SHAPE)

    # -- the step
    def step_players(self, actions, turns, active, u):
        """One step of every ``active`` game on actions (E, 4); ``turns`` and ``u`` are not needed (a dead goose's
        action is ignored, food comes from the pick rule)."""
        E = self.E
        actions = actions.to(torch.long).contiguous()
        active = active.to(torch.bool).contiguous()
        assert actions.shape == (E, GEESE) and active.shape == (E,)
        if self._hip():
            self._state_ok()
            self._native('hrl_geese_step', self.body, self.head, self.length, self.food, self.last, self.prev,
                         self.score, self.nstep, self.game, self.live, actions, active, self._seed, E, self.P, self.A)
            return
        a = self._np
        for e in np.flatnonzero(active.numpy()):
            g = self._games[e]
            step_game(g, actions[e].tolist(), self._seed)
            for i, goose in enumerate(g['geese']):          # the ring as the kernel writes it
                if goose:
                    h = (int(a['head'][e, i]) - 1) % RING
                    a['body'][e, i, h], a['head'][e, i] = goose[0], h
                a['length'][e, i] = len(goose)
            a['food'][e], a['last'][e], a['prev'][e], a['score'][e] = g['food'], g['last'], g['prev'], g['reward']
            a['nstep'][e], a['live'][e] = g['step'], g['live']
