/* hrl_geese.h -- batched Hungry Geese for device self-play (handyrl_amd.envs.geese.HungryGeeseBatch).
 *
 * Four geese on a 7 x 11 torus, cell = row * 11 + col, actions 0 NORTH 1 SOUTH 2 WEST 3 EAST.  The step rules are
 * this project's restatement of the Hungry Geese interpreter (handyrl_amd/envs/geese.py:step_game is the
 * specification); observation and outcome follow handyrl/envs/kaggle/hungry_geese.py:173-240.
 *
 * State of E games, allocated once by the caller and advanced in place (a captured graph keeps addressing it):
 *   body   (E, 4, 80) uint8   ring of cells per goose: cell k of the goose, head first, is body[(hd + k) % 80]
 *   hd     (E, 4)     uint8   ring index of the head
 *   len    (E, 4)     uint8   cells of the goose; 0 = dead (a goose is alive exactly while it has cells)
 *   food   (E, 2)     int8    food cells, -1 = none; new food takes the lowest empty slot
 *   last   (E, 4)     int8    the goose's last action, -1 before its first step
 *   prev   (E, 4)     int8    head cell in the previous state (-1: none -- right after reset, or it was dead)
 *   reward (E, 4)     int32   step * 100 + len as of the last step the goose survived, 0 before
 *   step   (E,)       int32   steps played
 *   game   (E,)       int64   game number: with the seed it fixes every random pick of the game
 *   live   (E,)       uint8   1 while the game runs (two or more geese alive and step < 199)
 *
 * Random picks (public rule, geese.geese_picks): word j of game g at step s is output word j & 3 of Philox4x32-10
 * with key (seed & 0xffffffff, seed >> 32) and counter (g & 0xffffffff, g >> 32, s, j >> 2); a pick among n free
 * cells takes the r-th free cell in ascending order, r = (word * n) >> 32.  Reset (s = 0): words 0-3 the heads,
 * words 4-5 the food.  A step that leaves fewer than two food cells: words 0, 1 of that step.
 *
 * Every entry takes plain pointers and sizes, allocates nothing, never synchronises and is capturable.  P (geese) and
 * A (actions) must both be 4.  HRL_EINVAL (before any HIP call) for a NULL required pointer, E < 0, P != 4, A != 4
 * (observe: Tm < 1 or a NULL t / infer with a record); E == 0: HRL_OK, no launch.  Returns 0, HRL_EINVAL or
 * HRL_ELAUNCH_BASE - hipError_t (hrl_targets.h).
 */
#ifndef HRL_GEESE_H
#define HRL_GEESE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* New games in the slots whose mask byte is set (mask NULL: every slot): slot e plays game number base + rank[e]
 * (rank NULL: base + e), heads and food by the pick rule at s = 0, everything else at its reset value, body zeroed.
 * One lane per game. */
int hrl_geese_reset(uint8_t *body, uint8_t *hd, uint8_t *len, int8_t *food, int8_t *last, int8_t *prev,
                    int32_t *reward, int32_t *step, int64_t *game, uint8_t *live, const uint8_t *mask,
                    const int64_t *rank, int64_t base, uint64_t seed, int64_t E, int64_t P, void *stream);

/* One step of every game whose active byte is set, on actions (E, 4) (only the two low bits of a label are read;
 * a dead goose's is ignored): moves, growth, hunger, collisions, food respawn, rewards, last, prev, live.  A game
 * with active == 0 is not touched.  `active` may alias `live`.  One lane per game. */
int hrl_geese_step(uint8_t *body, uint8_t *hd, uint8_t *len, int8_t *food, int8_t *last, int8_t *prev,
                   int32_t *reward, int32_t *step, const int64_t *game, uint8_t *live, const int64_t *actions,
                   const uint8_t *active, uint64_t seed, int64_t E, int64_t P, int64_t A, void *stream);

/* views (4, E, 17, 7, 11) float: view p of game e is the 17 planes seen by goose p (goose i on planes (i - p) % 4
 * of heads 0-3, tails 4-7, bodies 8-11, previous heads 12-15; food 16).  record (E, Tm, 4, 17, 7, 11) or NULL:
 * the same launch stores view p of game e into slot (e, *t, p) where infer[e * 4 + p] is set (t read on the
 * device; a t outside [0, Tm) stores nothing) and nothing anywhere else.  One wave per (game, view), 16-byte
 * stores between the unaligned edges of a row. */
int hrl_geese_observe(const uint8_t *body, const uint8_t *hd, const uint8_t *len, const int8_t *food,
                      const int8_t *prev, float *views, float *record, const int64_t *t, const uint8_t *infer,
                      int64_t E, int64_t P, int64_t Tm, void *stream);

/* hrl_geese_observe for the streaming per-player generator (rollout.PlayerStreamGenerator): every game records at
 * its own ply index ply[e] ((E,) int64, device memory) and the record is UINT8 (the planes are binary), (E, Tm, 4,
 * 17, 7, 11) bytes.  views (4, E, 17, 7, 11) float is written for every game, as above.  For a game with
 * active[e] != 0 and 0 <= ply[e] < Tm, slot (e, ply[e], p) gets view p where infer[e * 4 + p] is set and ZEROS where
 * it is not (the slot buffers outlive a game: a dead goose's slot must not keep an earlier game's planes); a game
 * with active[e] == 0 or a ply outside [0, Tm) stores nothing into the record.  One wave per (game, view); a view is
 * 1309 bytes, so a slot starts at any byte phase of a 16-byte line: single bytes up to the first aligned one, 16-byte
 * stores, then the tail.  All pointers required; HRL_EINVAL (before any HIP call) for a NULL one, E < 0, P != 4 or
 * Tm < 1; E == 0: HRL_OK, no launch. */
int hrl_geese_observe_at(const uint8_t *body, const uint8_t *hd, const uint8_t *len, const int8_t *food,
                         const int8_t *prev, float *views, uint8_t *record, const int64_t *ply, const uint8_t *infer,
                         const uint8_t *active, int64_t E, int64_t P, int64_t Tm, void *stream);

/* The forward's input rows of the evaluator (evaluation.PlayerEvaluator) in RELATIVE-SEAT order, no record:
 * rows (K, E, 17, 7, 11) float, row k * E + e = the view of goose (seat[e] + k) mod 4 of game e (the planes of
 * hrl_geese_observe), for k < K.  seat (E,) int64 in device memory.  K = 1 writes the home seat's view only (E rows
 * instead of 4 * E: the evaluation against random agents forwards nothing else); with K = 4, rows[:E] feeds the home
 * net and rows[E:] a second net on the three other seats, both as contiguous slices.  K waves per game, the stores of
 * hrl_geese_observe (a 1309-float row starts at any 4-byte phase of a 16-byte line).  HRL_EINVAL (before any HIP
 * call) for a NULL pointer, E < 0, P != 4 or K outside [1, 4]; E == 0: HRL_OK, no launch. */
int hrl_geese_observe_seats(const uint8_t *body, const uint8_t *hd, const uint8_t *len, const int8_t *food,
                            const int8_t *prev, const int64_t *seat, float *rows, int64_t E, int64_t P, int64_t K,
                            void *stream);

/* The greedy rule-based goose (geese.greedy_action_of is the specification; HungryGeeseBatch.greedy_players the
 * batch form).  The rule is THIS PROJECT'S statement of a greedy goose, modelled on the published behaviour of
 * Kaggle's GreedyAgent; kaggle_environments was not consulted and no move-for-move parity with it is claimed.
 *
 * rule (E, 4) int64: rule[e][p] is the label goose p of game e plays, or -1 (the caller then plays a uniform random
 * label).  For a goose that is alive (len > 0), with head its head cell and last its last action:
 *   Blocked cells: every cell of every goose (own cells and tails included), and the four torus neighbours of the
 *     head of every OTHER living goose.
 *   Candidates: the labels in the fixed order NORTH, EAST, SOUTH, WEST (0, 3, 1, 2) whose cell c = translate(head, a)
 *     is not blocked and, when last >= 0, for which a is not the opposite of last.
 *   Distance: d(a) = min over the food cells f >= 0 of |row(c) - row(f)| + |col(c) - col(f)| -- the plain distance on
 *     the 7 x 11 grid, NOT the torus distance; with no food on the board d = 0.
 *   Result: the candidate of smallest d, ties to the earliest in the order above; -1 without a candidate and for a
 *     dead goose.
 * Every slot is written, whatever `live` says (the state of a finished game is still a state).  One wave per game,
 * four games per workgroup: the lanes walk the four rings into the occupancy mask (a wave OR-reduction of two 64-bit
 * words), lanes 0-15 are the (goose, candidate) pairs, a 4-lane minimum over (d, order index) picks the label and
 * one lane per goose stores it.  Nothing else is stored.  HRL_EINVAL (before any HIP call) for a NULL pointer, E < 0
 * or P != 4; E == 0: HRL_OK, no launch. */
int hrl_geese_greedy(const uint8_t *body, const uint8_t *hd, const uint8_t *len, const int8_t *food,
                     const int8_t *last, int64_t *rule, int64_t E, int64_t P, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* HRL_GEESE_H */
