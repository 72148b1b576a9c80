/*
 * hrl_env.h — C ABI of the batched Geister rules, of the self-play ply tail, of the streaming
 * generator's harvest and of the device evaluator's ply (libhrl.so).
 *
 * Replaces the per-game rules of handyrl/envs/geister.py (Environment.legal_actions :460-487,
 * Environment.observation :495-535, Environment.play :359-394), which generation.py:20-88 calls
 * once per ply per worker process, by three launches over E games held in HBM in the layout of
 * handyrl_amd.envs.geister.GeisterBatch:
 *   board (E,36) int8: -1 empty, colour*2 + type (0 blue, 1 red), absolute cell x*6 + y;
 *   color, turn_count, win (E,) int64; cnt (E,4) int64 pieces per (colour, type).
 * Action labels are the reference's: 0..143 = direction*36 + cell in the mover's frame (white's
 * frame is the board rotated 180 degrees), 144 + k = initial layout k of combinations(range(8), 4).
 * All pointers are device pointers; bool tensors are one byte per element.  Asynchronous on
 * `stream`, no allocation, no synchronisation (graph-capturable).
 * Returns 0, HRL_EINVAL or HRL_ELAUNCH_BASE - hipError_t (hrl_targets.h).
 */
#ifndef HRL_ENV_H
#define HRL_ENV_H

#include <stdint.h>

#include "hrl_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

/* legal (E, 214) bytes: 1 where the side to move may play the label (geister.py:460-487). */
int hrl_geister_legal(const int8_t *board, const int64_t *color, const int64_t *turn_count, int64_t E,
                      uint8_t *legal, void *stream);

/* The view of `player` (E,): planes (E,7,6,6) fp32 [ones, own, opponent, own blue, own red, opponent
 * blue, opponent red] rotated for white, scalar (E,18) fp32 [me is black, turn view, one-hot 1..4 of
 * the four piece counts]; `full` != 0 shows the opponent's colours (observation(None), CIGeister)
 * (geister.py:495-535). */
int hrl_geister_observation(const int8_t *board, const int64_t *color, const int64_t *cnt, const int64_t *player,
                            int64_t E, int full, float *planes, float *scalar, void *stream);

/* hrl_geister_observation that also records the view for DeviceGenerator's episode: slot t (read from
 * device memory) of rec_planes (E,Tm,7,6,6) / rec_scalar (E,Tm,18) gets the view where active[e], zeros
 * elsewhere (the record of generation.py:55-62 with its reset value for finished games); rec_planes NULL:
 * no record. */
int hrl_geister_observation_record(const int8_t *board, const int64_t *color, const int64_t *cnt,
                                   const int64_t *player, int64_t E, int full, float *planes, float *scalar,
                                   const uint8_t *active, const int64_t *t, int64_t Tm, float *rec_planes,
                                   float *rec_scalar, void *stream);

/* hrl_geister_observation_record for the streaming generator (rollout.StreamGenerator): every game records
 * at its own ply index ply[e] (device memory) instead of one shared slot t.  An active game (active[e] != 0,
 * 0 <= ply[e] < Tm) gets its view in slot (e, ply[e]) of rec_planes / rec_scalar; an inactive game stores
 * NOTHING into the record (its ply[e] may equal Tm).  planes / scalar are written for every game.  All
 * pointers required; HRL_EINVAL (before any HIP call) for a NULL one, E < 0 or Tm < 1; E == 0: HRL_OK. */
int hrl_geister_observation_record_at(const int8_t *board, const int64_t *color, const int64_t *cnt,
                                      const int64_t *player, int64_t E, int full, float *planes, float *scalar,
                                      const uint8_t *active, const int64_t *ply, int64_t Tm, float *rec_planes,
                                      float *rec_scalar, void *stream);

/* Play action (E,) in every game whose active byte is set (geister.py:359-394): layouts, moves,
 * captures, escapes, piece counts, winner, the 200-move draw; the side to move flips.
 * layout_type (70,8) int8 piece type per initial slot, opos (2,8) int64 initial cells per colour.
 * live (E,) bytes or NULL: set to (win < 0) for every played game (the next ply's active mask; may be
 * the same array as `active`). */
int hrl_geister_step(int8_t *board, int64_t *color, int64_t *turn_count, int64_t *win, int64_t *cnt,
                     const int64_t *action, const uint8_t *active, const int8_t *layout_type, const int64_t *opos,
                     int64_t E, uint8_t *live, void *stream);

/* The sampling and recording tail of a self-play ply (generation.py:43-62), one wave per game:
 * m = legal ? 0 : 1e32, p = logits - m, action = argmax(p - log(-log(U[t]))) (torch.argmax's tie order);
 * slot t (read from device memory) of policy_buf / amask_buf (E,Tm,A), action_buf / value_buf / turn_buf
 * (E,Tm) and reward_buf (E,Tm,P) fp64 gets the game's p, m, action, value, player, reward when `active`,
 * else 0, 1e32, 0, 0, 0, 0.  logits (E, >=A) rows of stride logit_stride; U (Tm,E,A) uniforms in (0,1];
 * reward / reward_buf both NULL when the env has no per-ply reward.  action (E,) gets the sample. */
int hrl_selfplay_sample_record(const float *logits, int64_t logit_stride, const uint8_t *legal, const float *U,
                               const int64_t *t, const float *value, const uint8_t *active, const int64_t *player,
                               const double *reward, int64_t E, int64_t A, int64_t Tm, int64_t P, int64_t *action,
                               float *policy_buf, float *amask_buf, int64_t *action_buf, float *value_buf,
                               int64_t *turn_buf, double *reward_buf, void *stream);

/* hrl_selfplay_sample_record for the streaming generator: no uniform buffer and no shared ply index.  Game e
 * is game number game[e] at ply ply[e] (both (E,) int64 device arrays); the wave computes its uniforms itself
 * by the public rule of rollout.stream_uniforms, bit for bit:
 *   Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten rounds),
 *   key (seed & 0xffffffff, seed >> 32), counter (game & 0xffffffff, game >> 32, ply, a / 4),
 *   label a takes output word x = out[a % 4],  u = ((float)(x >> 9) + 0.5f) * 2^-23  (exact, in (0, 1)).
 * Otherwise the fp32 operations, the tie order and the records of hrl_selfplay_sample_record, written to slot
 * (e, ply[e]).  An inactive game gets action[e] = 0 and NO record store at all (its ply[e] may equal Tm); an
 * active game's ply[e] must lie in [0, Tm) (a game outside it is treated as inactive).
 * HRL_EINVAL (before any HIP call) for a NULL required pointer, E < 0, A < 1, Tm < 1, P < 1, logit_stride < A,
 * reward / reward_buf given one without the other; E == 0: HRL_OK, no launch. */
int hrl_selfplay_sample_record_stream(const float *logits, int64_t logit_stride, const uint8_t *legal, uint64_t seed,
                                      const int64_t *game, const int64_t *ply, const float *value,
                                      const uint8_t *active, const int64_t *player, const double *reward, int64_t E,
                                      int64_t A, int64_t Tm, int64_t P, int64_t *action, float *policy_buf,
                                      float *amask_buf, int64_t *action_buf, float *value_buf, int64_t *turn_buf,
                                      double *reward_buf, void *stream);

/* Whole TicTacToe self-play games in ONE launch (csrc/hrl_boardplay.hip): plies t0 <= t < t1 <= Tm <= 9 of
 * rollout.DeviceGenerator's mover-only ply on a TicTacToeBatch with a nn.BoardInference net, for E games, 16 per
 * workgroup.  pack: one hrl_board_infer_pack pack (include/hrl_nn.h; 16-byte aligned) of a net of `layers` blocks.
 * U (Tm, E, 9) uniforms in (0, 1].  board (E, 9) int8, color (E,) int8, nmoves (E,) int32, winner (E,) int8: the
 * env's state, advanced in place.  Per game and ply, in DeviceGenerator._ply's order: active = winner == 0 &&
 * nmoves < 9, player = nmoves % 2; the mover's view [1, board == color, board == -color]; hrl_board_infer's forward
 * (the same device code: the same bits); hrl_selfplay_sample_record's sampling (m = legal ? 0 : 1e32, p = logit - m,
 * argmax(p - log(-log(u))), torch.argmax's tie order); slot (e, t) of obs (E, Tm, 27), policy / amask (E, Tm, 9)
 * fp32 and action / value / turn (E, Tm) int64 / fp32 / int64 gets the live value of an active game, else 0, 0, 1e32,
 * 0, 0, 0 -- every slot of plies [t0, t1) is written for every game, whatever the buffers held; then
 * TicTacToeBatch.step for the active games (the cell takes color; winner = color on a line of three; color flips;
 * nmoves + 1).  Calls over [t0, tm) and [tm, t1) equal one over [t0, t1).  Asynchronous, allocates nothing,
 * capturable.  HRL_EINVAL (before any HIP call) for a NULL pointer, layers outside 1..8, a pack that is not 16-byte
 * aligned, E < 0 (or E > 2^31 - 17), Tm outside 1..9, t0 < 0, t1 > Tm, t0 > t1; E == 0 or t0 == t1: HRL_OK, no
 * launch. */
int hrl_board_selfplay(const void *pack, int64_t layers, int64_t E, int64_t Tm, int64_t t0, int64_t t1, const float *U,
                       int8_t *board, int8_t *color, int32_t *nmoves, int8_t *winner, float *obs, float *policy,
                       float *amask, int64_t *action, float *value, int64_t *turn, void *stream);

/* The slot records of the streaming generator (DeviceGenerator's mover-only layout), DEVICE pointers to
 * C-contiguous fp32 / int64 / fp64 tensors; the struct itself is HOST memory read before the call returns:
 *   obs[l] (E, Tm, obs_width[l]) fp32, l < nleaves <= 8      policy, amask (E, Tm, A) fp32
 *   action, turn (E, Tm) int64    value (E, Tm) fp32           reward (E, Tm, P) fp64 or NULL (no reward) */
typedef struct hrl_selfplay_slots {
    int64_t E, Tm, P, A;
    int32_t nleaves;
    int64_t obs_width[HRL_REPLAY_MAX_LEAVES];
    const float *obs[HRL_REPLAY_MAX_LEAVES];
    const float *policy, *amask;
    const int64_t *action;
    const float *value;
    const int64_t *turn;
    const double *reward;
} hrl_selfplay_slots;

/* Finished games leave their slots for the replay ring (rollout.StreamGenerator calls this once per ply, after
 * the env step).  done (E,) bytes marks them; ply[e] is a finished game's length L (0 <= L <= Tm; clamped).
 * With c the number of done slots and r(e) the number of done slots below e (slot order: deterministic, no
 * atomics), base = state[0]:
 *   ring row (base + r) mod N receives the whole episode of slot e, over the ring's WRITABLE records
 *   (`ring` as in hrl_replay_gather, layout HRL_REPLAY_MOVER_RECORDS; its tmask / omask are ignored):
 *     plies t < L   the slot's records; an observation leaf converted as src.to(dst.dtype) does (HRL_REPLAY_U8:
 *                   (uint8)x, x in [0, 255]), the reward narrowed to fp32,
 *                   ret[t] = reward[t] + gamma * ret[t+1] per player in fp64 from t = L-1 down (ret[L] = 0),
 *                   stored as fp32 (DeviceGenerator._returns; the library is built with -ffp-contract=off);
 *     plies t >= L  the reset values: obs 0, policy 0, amask 1e32, action, value, turn, reward, ret 0;
 *     length = L, outcome = outcome[e] ((E, P) fp32), ring_game[row] = game[e]  (ring_game (N,) int64).
 *   When c > N a row is claimed more than once in the call; the highest slot wins, as if the slots were emitted
 *   one after another.
 * A second launch of one workgroup, ordered after the first by the stream, then restarts the slots and advances
 * the state with plain stores: game[e] = state[2] + r, ply[e] = 0, pending[e] = 1 for the done slots, and
 * state = {ring_ptr, emitted, next_game} (3 int64) becomes {(base + c) mod N, emitted + c, next_game + c}.
 * A call with no done slot changes nothing.  slots->reward NULL: the ring's reward and ret get zeros.
 * HRL_EINVAL (before any HIP call) for: a NULL done / slots / ply / outcome / ring / ring_game / game / pending /
 * state; E < 0; Tm, P, A or N < 1; ring Tm, P, A or leaf count / widths other than the slots'; nleaves not in
 * [1, 8]; an obs_type other than HRL_REPLAY_U8 / HRL_REPLAY_F32; an obs_width < 1; a NULL required record (all but
 * slots->reward, ring->tmask, ring->omask); a record of 2^31 elements or more per slot.  E == 0 passes the same
 * validation, returns HRL_OK and launches nothing.  Ring offsets are formed in 64 bits. */
int hrl_selfplay_harvest(const uint8_t *done, const hrl_selfplay_slots *slots, int64_t *ply, const float *outcome,
                         double gamma, const hrl_replay_ring *ring, int64_t *ring_game, int64_t *game,
                         uint8_t *pending, int64_t *state, void *stream);

/* ---- The streaming generator for simultaneous-move envs (rollout.PlayerStreamGenerator): per-player records.
 *
 * Public sampling rules (pure-Python and torch twins in handyrl_amd/rollout.py), both Philox4x32-10 with key
 * (seed & 0xffffffff, seed >> 32), counter (game & 0xffffffff, game >> 32, ply, w3) and the float mapping above,
 * u = ((float)(x >> 9) + 0.5f) * 2^-23:
 *   stream_player_uniforms: player p, label a uses w3 = 0x40000000 + p * ceil(A / 4) + a / 4, output word a % 4;
 *   stream_select_uniform:  w3 = 0x80000000, output word 0 (the u that step_players takes).
 * The last counter word keeps the streams of one (seed, game, ply) apart: the mover rule above takes a / 4
 * (< 0x40000000), the Hungry Geese picks 0 and 1 (include/hrl_geese.h), eval_pick 0xffffffff, the player uniforms
 * [0x40000000, 0x80000000) and the select uniform 0x80000000.  P * ceil(A / 4) must stay below 0x40000000. */

/* The sampling and recording tail of the per-player ply in ONE launch, one wave per (game, player).
 * logits (P * E, >= A) fp32 rows of stride logit_stride, player-major: row p * E + e; value (P * E,) fp32 likewise.
 * legal: bytes, legal_player_stride == 0: (E, A), the same for every player; == A: (E, P, A).
 * turns, infer (E, P) bytes; active (E,) bytes; game, ply (E,) int64.
 *   m = legal ? 0 : 1e32;  p = logit - m;  a = argmax_a(p - log(-log(u)))  with u of stream_player_uniforms, the fp32
 *   operations of hrl_selfplay_sample_record_stream and torch.argmax's tie order (NaN first, then the lowest label).
 * A game is PLAYED when active[e] != 0 and 0 <= ply[e] < Tm.
 *   action (E, P) int64: the sample where the game is played and turns is set, else 0; written for every (e, p).
 *   usel (E,) fp32 = stream_select_uniform(seed, game[e], ply[e]); written for every game.
 *   A played game stores slot (e, ply[e], p) of EVERY player p (the slot buffers outlive a game):
 *     policy_buf, amask_buf (E, Tm, P, A) fp32, action_buf (E, Tm, P) int64, tmask_buf (E, Tm, P) bytes:
 *       p, m, a, 1 where turns is set, else 0, 1e32, 0, 0;
 *     value_buf (E, Tm, P) fp32, omask_buf (E, Tm, P) bytes: value, 1 where infer is set, else 0, 0.
 *   A game that is not played stores nothing into the records.
 * HRL_EINVAL (before any HIP call) for a NULL pointer, E < 0, P < 1, A < 1, A > 2^20, Tm < 1, logit_stride < A,
 * legal_player_stride other than 0 or A, P * E or P * ceil(A / 4) of 0x40000000 or more; E == 0: HRL_OK, no launch. */
int hrl_selfplay_sample_record_players_stream(const float *logits, int64_t logit_stride, const float *value,
                                              const uint8_t *legal, int64_t legal_player_stride, const uint8_t *turns,
                                              const uint8_t *infer, const uint8_t *active, uint64_t seed,
                                              const int64_t *game, const int64_t *ply, int64_t E, int64_t P, int64_t A,
                                              int64_t Tm, int64_t *action, float *usel, float *policy_buf,
                                              float *amask_buf, int64_t *action_buf, float *value_buf,
                                              uint8_t *tmask_buf, uint8_t *omask_buf, void *stream);

/* The slot records of the per-player streaming generator, DEVICE pointers to C-contiguous tensors; the struct itself
 * is HOST memory read before the call returns:
 *   obs[l] (E, Tm, P, obs_width[l]) uint8 or fp32 per obs_type[l] (HRL_REPLAY_U8 / HRL_REPLAY_F32), l < nleaves <= 8
 *   policy, amask (E, Tm, P, A) fp32     action (E, Tm, P) int64     value (E, Tm, P) fp32
 *   tmask, omask (E, Tm, P) bytes 0/1    reward (E, Tm, P) fp64 or NULL (no reward) */
typedef struct hrl_selfplay_player_slots {
    int64_t E, Tm, P, A;
    int32_t nleaves;
    int32_t obs_type[HRL_REPLAY_MAX_LEAVES];
    int64_t obs_width[HRL_REPLAY_MAX_LEAVES];
    const void *obs[HRL_REPLAY_MAX_LEAVES];
    const float *policy, *amask;
    const int64_t *action;
    const float *value;
    const uint8_t *tmask, *omask;
    const double *reward;
} hrl_selfplay_player_slots;

/* hrl_selfplay_harvest for per-player records: `ring` is a rollout.PlayerReplay (the PLAYERS layouts of
 * hrl_replay.h: records (N, Tm, P, ...), tmask / omask required, turn ignored).  The contract is that entry's: done
 * (E,) bytes, ply[e] the length L (clamped to [0, Tm]), c done slots, r(e) done slots below e, base = state[0]:
 *   ring row (base + r) mod N receives the whole episode of slot e, in slot order, without atomics; when c > N the
 *   highest slot that claims a row wins;
 *     plies t < L   the slot's records; an observation leaf converted as src.to(dst.dtype) does for each of the four
 *                   U8 / F32 pairs ((uint8)x for x in [0, 255], (float)b), the reward narrowed to fp32, ret[t] =
 *                   reward[t] + gamma * ret[t+1] per player in fp64 from t = L-1 down, stored as fp32;
 *     plies t >= L  the reset values: obs 0, policy 0, amask 1e32, action, value, tmask, omask, reward, ret 0;
 *     length = L, outcome = outcome[e] ((E, P) fp32), ring_game[row] = game[e]  (ring_game (N,) int64);
 *   the slot records are READ for t < L only (a Hungry Geese slot is 1 MB and the mean game a few plies), the
 *   rest of the row is stores of the reset values.
 * The second launch (one workgroup) is hrl_selfplay_harvest's: game[e] = state[2] + r, ply[e] = 0, pending[e] = 1
 * for the done slots, state = {ring_ptr, emitted, next_game} becomes {(base + c) mod N, emitted + c, next_game + c}.
 * A call with no done slot changes nothing.  slots->reward NULL: the ring's reward and ret get zeros.
 * 16-byte accesses are used only where the record's size per slot and both bases make them aligned for every slot
 * and row (then 4-byte ones under the same rule, else single elements); the reset values of a row are stored 16 bytes
 * at a time between the row's unaligned edges.  Offsets are formed in 64 bits.
 * HRL_EINVAL (before any HIP call) for: a NULL done / slots / ply / outcome / ring / ring_game / game / pending /
 * state; E < 0; Tm, P, A or N < 1; ring Tm, P, A or leaf count / widths other than the slots'; nleaves not in [1, 8];
 * an obs_type (slots or ring) other than HRL_REPLAY_U8 / HRL_REPLAY_F32; an obs_width < 1; a NULL required record
 * (all but slots->reward and ring->turn); a record of 2^31 elements or more per slot.  E == 0 passes the same
 * validation, returns HRL_OK and launches nothing. */
int hrl_selfplay_harvest_players(const uint8_t *done, const hrl_selfplay_player_slots *slots, int64_t *ply,
                                 const float *outcome, double gamma, const hrl_replay_ring *ring, int64_t *ring_game,
                                 int64_t *game, uint8_t *pending, int64_t *state, void *stream);

/* Masked row copy for the movers' recurrent state (generation.py:38-41: only the mover's hidden state
 * advances): for each of nleaves (<= 16) fp32 tensors, row e of dst[l] (E rows of F[l] contiguous floats,
 * row stride dst_stride[l] elements) becomes row e of src[l] where mask[e] != 0; other rows are untouched.
 * One launch for every state tensor, exactly torch.where(mask, src, dst). */
int hrl_masked_rows_copy(int nleaves, float *const *dst, const int64_t *dst_stride, const float *const *src,
                         const int64_t *src_stride, const int64_t *F, const uint8_t *mask, int64_t E, void *stream);

/* ---- The device evaluator (evaluation.DeviceEvaluator): the model on one seat, uniform random agents on the others
 * (handyrl/evaluation.py:64-87, agent.py:13-19, 55-110).  E slots play exactly G games and restart in place.
 *
 * Public rules (pure-Python twins in handyrl_amd/evaluation.py):
 *   Games are counted by NUMBER, never by finishing order: numbers 0 .. G-1 are each played exactly once.  Slot e
 *     starts game e when e < G and is retired otherwise; a finished slot takes next_game + r, r = the number of done
 *     slots below it in slot order (no atomics, tickets or spin-waits); a slot whose new number would be >= G is
 *     retired and stays inactive.  (Counting the first G games to FINISH would favour short games.)
 *   Seat: the model plays seat(g) = g mod P, the other seats are random agents.
 *   Mover: the mover of global step s is s mod P in every live game, so a slot restarts only at a step with
 *     s mod P == 0 (`pending` marks a slot that waits for it).
 *   Random seat, eval_pick(seed, game, ply, legal): n = the number of legal labels, x = output word 0 of
 *     Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (game & 0xffffffff, game >> 32, ply,
 *     0xffffffff) -- the last word is disjoint from the sampling rule's a / 4 above --, w = x >> 9,
 *     k = (w * n) >> 23 in integer arithmetic, so 0 <= k < n always (an fp32 floor(u * n) can round up to n); the
 *     action is the k-th legal label in ascending order.
 *   Model seat, temperature == 0 (agent.py:92-96): p = logits - (legal ? 0 : 1e32), action = argmax p, ties to the
 *     lowest label, NaN first (torch.argmax's order).  The one difference from the reference: it breaks an exact tie
 *     by legal_actions() order, which for Geister is by piece, not by label.
 *   Model seat, temperature > 0 (agent.py:97-100 as Gumbel-max): argmax of p * r - log(-log(u)) in fp32 with
 *     r = (float)(1.0 / temperature) and u of the streaming rule above for (seed, game, ply, label).
 *   Forced moves: forced (G, Tm) int64 or NULL; forced[g][t] >= 0 is played at ply t of game g whichever seat moves,
 *     -1 leaves the decision to the evaluator.
 *   Trace (tests; all four buffers or none): action, picked (G, Tm) int64, policy (G, Tm, A) fp32, model_ply (G, Tm)
 *     bytes.  At ply t of game g: action = the move played, picked = the evaluator's own decision even where a move
 *     was forced, model_ply = 1 and policy = p at a model ply (policy is not stored at a random-seat ply).
 *
 * All entries are asynchronous on `stream`, allocate nothing, read nothing on the host (graph-capturable) and
 * validate before any HIP call: HRL_EINVAL for a NULL required pointer, E < 0, A < 1, Tm < 1, P < 1, G < 0,
 * logit_stride < A (and: mover outside [0, P), temperature < 0 or NaN, some but not all trace buffers); E == 0:
 * HRL_OK, no launch. */

/* One launch per ply, one wave per slot, lanes over the A labels.  A slot with active[e] == 0 (retired or waiting
 * to restart; also one whose ply[e] is outside [0, Tm) or game[e] outside [0, G)) gets action[e] = 0 and NO other
 * store.  An active slot plays the model's move where seat[e] == mover and the random agent's elsewhere.
 * logits (E, >= A) rows of stride logit_stride, legal (E, A) bytes, game / ply / seat (E,) int64, active (E,) bytes;
 * action (E,) int64 is written for every slot and nothing else outside the trace.
 * There is one decision kernel: this entry is hrl_match_act (below) with logits_opp = NULL, stride_opp = 0,
 * temperature_opp = 0 and opening = 0, and its argument checks are that entry's. */
int hrl_eval_act(const float *logits, int64_t logit_stride, const uint8_t *legal, uint64_t seed, double temperature,
                 const int64_t *game, const int64_t *ply, const uint8_t *active, const int64_t *seat, int64_t mover,
                 const int64_t *forced, int64_t E, int64_t A, int64_t Tm, int64_t P, int64_t G, int64_t *action,
                 int64_t *trace_action, int64_t *trace_picked, float *trace_policy, uint8_t *trace_model_ply,
                 void *stream);

/* hrl_eval_act for a match of two nets (evaluation.DeviceEvaluator with an opponent; the reference seats one Agent per
 * model in exec_match, handyrl/evaluation.py:64-116).  One launch per ply of the same form; logits_home / logits_opp
 * (E, >= A) fp32 rows of stride stride_home / stride_opp.  For an active slot with game g and ply t in range:
 *   The mover's net is home where seat[e] == mover, otherwise opp, or no net when logits_opp is NULL.
 *   Where t < opening, or where the mover has no net, pick = eval_pick(seed, g, t, legal): the rule above, bit for bit.
 *   Otherwise pick comes from that net's own row and that net's own temperature: at temperature 0 the argmax of
 *     p = logits - (legal ? 0 : 1e32), ties to the lowest label, NaN first; at temperature > 0 the argmax of
 *     p * (float)(1.0 / temperature) - log(-log(u)) with u of the streaming rule for (seed, g, t, label).  Only one
 *     agent moves at a given (g, t), so both agents share the one stream.
 *   forced[g][t] >= 0 overrides the move played, not `picked`.
 *   Trace: policy[g][t] = p whenever the mover has a net, opening plies included; model_ply[g][t] = (seat == mover);
 *     action and picked as for hrl_eval_act.
 *   Which rows the evaluator feeds: the home net sees the board from `seat`; the opponent sees it from the mover's seat
 *     where the mover is not home and from seat (seat + 1) mod P otherwise (for P == 2: always the other seat).
 * An inactive, retired or out-of-range slot gets action[e] = 0 and no other store.  With logits_opp == NULL and
 * opening == 0 this is hrl_eval_act (the same launch).  HRL_EINVAL as for hrl_eval_act, and for
 * stride_home < A, stride_opp < A when logits_opp is given, either temperature < 0 or NaN, opening < 0. */
int hrl_match_act(const float *logits_home, int64_t stride_home, const float *logits_opp, int64_t stride_opp,
                  const uint8_t *legal, uint64_t seed, double temperature_home, double temperature_opp,
                  int64_t opening, const int64_t *game, const int64_t *ply, const uint8_t *active,
                  const int64_t *seat, int64_t mover, const int64_t *forced, int64_t E, int64_t A, int64_t Tm,
                  int64_t P, int64_t G, int64_t *action, int64_t *trace_action, int64_t *trace_picked,
                  float *trace_policy, uint8_t *trace_model_ply, void *stream);

/* After the env's step, one launch of one workgroup.  For every active slot: ply += 1 and
 * done = terminal[e] != 0 || ply >= Tm.  A done slot stores outcome_out[game] = outcome[e] ((G, P) and (E, P) fp32)
 * and length_out[game] = ply ((G,) int64), indexed by game number, then restarts or retires by the rule above with
 * {finished, next_game} = state (2 int64 in device memory, plain stores):
 *   n = next_game + r;  n < G: game = n, seat = n mod P, ply = 0, pending = 1;  else game = G, seat = 0, ply = 0,
 *   pending = 0;  active = 0 either way (the evaluator sets active where pending at the next step with mover 0);
 *   state = {finished + c, min(next_game + c, G)}, c = the number of done slots.
 * Slots that are not active are not touched. */
int hrl_eval_finish(const uint8_t *terminal, const float *outcome, int64_t E, int64_t Tm, int64_t P, int64_t G,
                    uint8_t *active, int64_t *ply, int64_t *game, int64_t *seat, uint8_t *pending, int64_t *state,
                    float *outcome_out, int64_t *length_out, void *stream);

/* The zeroing twin of hrl_masked_rows_copy: rows e with mask[e] != 0 of nleaves (<= 16) fp32 tensors (E rows of F[l]
 * contiguous floats, row stride dst_stride[l] elements) become 0; other rows are untouched.  One launch (a restarting
 * slot's recurrent state, by row). */
int hrl_masked_rows_fill(int nleaves, float *const *dst, const int64_t *dst_stride, const int64_t *F,
                         const uint8_t *mask, int64_t E, void *stream);

/* ---- The evaluator of simultaneous-move envs (evaluation.PlayerEvaluator: Hungry Geese; ParallelTicTacToe at class
 * level): the home net on one seat, uniform random agents -- or a second net -- on all the others, every player
 * moving every ply (handyrl/evaluation.py:64-87, 119-136).
 *
 * Public rules (pure-Python and torch twins in handyrl_amd/evaluation.py).  Games are counted by number and seated as
 * above (seat(g) = g mod P); the finish is hrl_eval_finish unchanged.  There is no mover: one launch per ply decides
 * for every player, and a finished slot restarts on the very next step as game number `game[e]` (for Hungry Geese:
 * Geese game number g under the env's seed, so a game depends on (seed, g, actions) only, never on the slot).  A game
 * runs until the env is terminal, also after the home player is out.  For an active slot with game g in [0, G), ply t
 * in [0, Tm) and a player p with turns[e][p] set:
 *   Relative seat: k = (p - seat[e]) mod P.  k == 0 is the home net; k >= 1 the opponent net when one is given, else
 *     no net.
 *   Random pick, eval_pick_player(seed, g, t, p, legal): eval_pick's integer rule on output word p & 3 of the Philox
 *     call with last counter word 0xffffffff - (p >> 2).  Player 0 is eval_pick itself.  These words stay apart from
 *     the Geese picks (0, 1), the player uniforms [0x40000000, 0x80000000) and the select uniform 0x80000000.
 *   Where t < opening or the player has no net, pick = the random pick.  Otherwise pick comes from the player's own
 *     logits row at its agent's temperature: at 0 the argmax of p = logits - (legal ? 0 : 1e32), ties to the lowest
 *     label, NaN first; above 0 the argmax of p * (float)(1.0 / temperature) - log(-log(u)) in fp32 with
 *     u = stream_player_uniforms(seed, g, t, P, A)[p].
 *   forced (G, Tm, P) int64 or NULL: forced[g][t][p] >= 0 overrides the move played, not `picked`.
 *   usel[e] = stream_select_uniform(seed, game[e], ply[e]) (ParallelTicTacToe's step_players takes it, Geese does not).
 *   Trace (all four buffers or none): action, picked (G, Tm, P) int64, policy (G, Tm, P, A) fp32, alive (G, Tm, P)
 *     bytes.  Every player of such a slot stores alive = turns; a player that moves stores action = the move played and
 *     picked = its own decision, one that does not stores -1 in both; policy = p is stored where the player moves and
 *     has a net, opening plies included.
 *
 * The decision in ONE launch, one wave per (slot, player), lanes striding over the A labels (A may exceed 64).
 * Logits are relative-seat-major: logits_home (E, >= A) fp32 rows of stride stride_home; logits_opp ((P - 1) * E, >= A)
 * rows of stride stride_opp, or NULL: row (k - 1) * E + e belongs to player (seat[e] + k) mod P.  legal: bytes,
 * legal_player_stride == 0: (E, A), the same for every player; == A: (E, P, A).  turns (E, P) bytes; game, ply, seat
 * (E,) int64; active (E,) bytes.
 * action (E, P) int64 and usel (E,) fp32 are written for EVERY slot: they are the step's inputs.  An inactive, retired
 * or out-of-range slot (active[e] == 0, ply outside [0, Tm), game outside [0, G)) gets action[e][:] = 0 and no other
 * store; a player of an active slot that does not move gets action 0.
 * Asynchronous on `stream`, allocates nothing, reads nothing on the host (graph-capturable).  HRL_EINVAL (before any
 * HIP call) for a NULL required pointer (all but logits_opp, forced and the trace), E < 0, P, A or Tm < 1, A > 2^20,
 * G < 0, stride_home < A, stride_opp < A when logits_opp is given, legal_player_stride other than 0 or A, a temperature
 * < 0 or NaN, opening < 0, some but not all trace buffers, P * E or P * ceil(A / 4) of 0x40000000 or more; E == 0:
 * HRL_OK, no launch. */
int hrl_players_act(const float *logits_home, int64_t stride_home, const float *logits_opp, int64_t stride_opp,
                    const uint8_t *legal, int64_t legal_player_stride, const uint8_t *turns, uint64_t seed,
                    double temperature_home, double temperature_opp, int64_t opening, const int64_t *game,
                    const int64_t *ply, const uint8_t *active, const int64_t *seat, const int64_t *forced, int64_t E,
                    int64_t P, int64_t A, int64_t Tm, int64_t G, int64_t *action, float *usel,
                    int64_t *trace_action, int64_t *trace_picked, float *trace_policy, uint8_t *trace_alive,
                    void *stream);

/* hrl_players_act with a rule-based agent on the seats without a net (PlayerEvaluator(opponent='rule'): Hungry Geese's
 * greedy goose, hrl_geese.h).  rule (E, P) int64 in device memory, or NULL.  A player of an active slot that moves,
 * has NO net (k >= 1; logits_opp must be NULL) and is at t >= opening picks rule[e][p] when that is in [0, A) and a
 * legal label for the player, and otherwise the random pick, unchanged (eval_pick_player(seed, g, t, p, legal): no
 * new counter word).  `picked` records that decision, `forced` still overrides the move played and no policy is
 * stored for such a player.  Everything else is hrl_players_act's rule word for word -- it is the same kernel with
 * one more pointer -- and with rule == NULL every output equals hrl_players_act's bit for bit.  HRL_EINVAL when both
 * rule and logits_opp are given (one meaning per call), and for every reason hrl_players_act has. */
int hrl_players_act_rule(const float *logits_home, int64_t stride_home, const float *logits_opp, int64_t stride_opp,
                         const uint8_t *legal, int64_t legal_player_stride, const uint8_t *turns, uint64_t seed,
                         double temperature_home, double temperature_opp, int64_t opening, const int64_t *game,
                         const int64_t *ply, const uint8_t *active, const int64_t *seat, const int64_t *forced,
                         const int64_t *rule, int64_t E, int64_t P, int64_t A, int64_t Tm, int64_t G, int64_t *action,
                         float *usel, int64_t *trace_action, int64_t *trace_picked, float *trace_policy,
                         uint8_t *trace_alive, void *stream);

/* ---- The league evaluator (evaluation.LeagueEvaluator): a round robin of K >= 2 nets on the device.
 *
 * Public rules (torch twins in handyrl_amd/evaluation.py):
 *   Agents: K nets, agents 0 .. K-1, each a module object of its own, on an alternating env with P == 2.
 *   Pairings: by default every (i, j) with i < j in lexicographic order, Q = K (K - 1) / 2 of them; or an explicit
 *     list of pairs with i != j in which each unordered pair appears at most once.  The first agent of a pair is its
 *     HOME agent.  A ladder of the newest agent against all others is [(K-1, 0), ..., (K-1, K-2)].
 *   Games: every pairing plays G games, numbers 0 .. G-1; in game g the home agent sits on seat g mod 2.
 *   Contract: every ply is decided by the match rules above, unchanged -- the mover's own net at the one shared
 *     temperature, eval_pick on the first `opening` plies, Philox keyed by (seed, g, ply) -- so game g of pairing
 *     (i, j) IS game g of the match of net i (home) against net j with the same arguments.
 *   Slots: E = Q * S; pairing q owns slots q * S .. q * S + S - 1; S is even and >= 2.  Slot t of a block plays games
 *     t, t + S, t + 2 S, ... while the number is below G, then retires.  A slot restarts only at a step with
 *     s mod 2 == 0.  Because S is even a slot's seating never changes (seat = t mod 2 for the whole run), so the set of
 *     rows on which a given net moves at a given mover parity is fixed: shapes are static and one captured graph per
 *     mover serves the run.  This is NOT hrl_eval_finish's next_game + r rule; every game number is still played
 *     exactly once, whichever game finishes first, so short games are not favoured.
 *   Forwards: without `observation` each net runs once per ply over the rows where it is the mover (the view is the
 *     mover's seat): E rows over all nets.  With it each net runs over every slot it sits in, from its own seat: 2 E.
 *   Recurrent state: one row per net per slot it sits in, zero when a game starts, advanced where the net moved (with
 *     `observation`: on every row); a net's rows of one seat are contiguous.
 * Both entries are asynchronous on `stream`, allocate nothing, read nothing on the host (graph-capturable) and
 * validate before any HIP call. */

/* hrl_eval_finish with the block rule; after the env's step, one launch of one workgroup.  For every active slot:
 * ply += 1 and done = terminal[e] != 0 || ply >= Tm.  A done slot e of block q = e / S with game number g:
 *   0 <= g < G: outcome_out[q][g] = outcome[e] and length_out[q][g] = ply  (outcome_out (Q, G, P) fp32, length_out
 *   (Q, G) int64, Q = E / S; outcome (E, P) fp32);
 *   n = g + S;  n < G: game = n, ply = 0, pending = 1;  else (retired) game = G, ply = 0, pending = 0;
 *   active = 0 either way.  The seat is not touched.
 * state[0] (one int64 in device memory, `finished`) grows by the number of done slots; the host stops at Q * G.
 * Plain stores only: no atomics, tickets or spin-waits.  Slots that are not active are not touched.
 * HRL_EINVAL for a NULL pointer, E < 0, S < 2 or odd, E not a multiple of S, Tm < 1, P < 1, G < 0; E == 0: HRL_OK, no
 * launch. */
int hrl_league_finish(const uint8_t *terminal, const float *outcome, int64_t E, int64_t S, int64_t Tm, int64_t P,
                      int64_t G, uint8_t *active, int64_t *ply, int64_t *game, uint8_t *pending, int64_t *state,
                      float *outcome_out, int64_t *length_out, void *stream);

/* The ply's route: for each of nleaves (<= 16) fp32 tensors in ONE launch, row dst_index[r] of dst[l] becomes row
 * src_index[r] of src[l] for r < n (rows of F[l] contiguous floats, row strides dst_stride[l] / src_stride[l] elements
 * as in hrl_masked_rows_copy).  src_index / dst_index (n,) int64 device arrays; NULL is the identity.  Every index
 * must be a row of its tensor, and the dst rows distinct; other rows of dst are untouched.  The observation leaves go
 * into net-major order in one launch and the nets' logits return to slot order in one launch, whatever K is.
 * HRL_EINVAL for nleaves outside [1, 16], a NULL array or leaf, F < 1, a stride < F, n < 0; n == 0: HRL_OK, no launch. */
int hrl_rows_permute(int nleaves, float *const *dst, const int64_t *dst_stride, const float *const *src,
                     const int64_t *src_stride, const int64_t *F, const int64_t *src_index, const int64_t *dst_index,
                     int64_t n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* HRL_ENV_H */
