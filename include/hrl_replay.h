/*
 * hrl_replay.h — C ABI of the replay-side batch assembly (libhrl.so).
 *
 * Replaces the reference's Batcher.select_episode + make_batch
 * (handyrl/train.py:284-293 and :33-133) for episodes that live in a ring of
 * device records (rollout.DeviceReplay, rollout.PlayerReplay):
 *
 *   hrl_replay_draw    one launch draws B windows (slot, start, player)
 *   hrl_replay_gather  one launch writes every tensor of the make_batch
 *                      layout for those windows into caller-owned buffers
 *
 * Both are asynchronous on `stream` (a hipStream_t), allocate nothing, never
 * synchronise and read no device memory on the host, so they may be captured
 * into a hipGraph.  The two descriptor structs are HOST memory, read before
 * the call returns.  Return value: 0, HRL_EINVAL (before any HIP call) or
 * HRL_ELAUNCH_BASE - hipError_t.
 */
#ifndef HRL_REPLAY_H
#define HRL_REPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_REPLAY_MAX_LEAVES 8

/* element type of an observation leaf's record */
enum {
    HRL_REPLAY_U8 = 0,  /* uint8 / bool, widened to fp32 by the gather */
    HRL_REPLAY_F32 = 1,
};

/* record layout of the ring and player layout of the batch */
enum {
    /* DeviceReplay: records (N, Tm, ...) of the ply's mover, `turn` (N, Tm) int64 names it.  Batch: observation,
     * policy, action_mask, action with a player axis of 1; value, reward, return, turn_mask, observation_mask,
     * outcome over the P players (value = value * one_hot(turn), both masks = one_hot(turn)). */
    HRL_REPLAY_MOVER_RECORDS = 0,
    /* PlayerReplay: records (N, Tm, P, ...), `tmask` / `omask` (N, Tm, P) bytes.  Every field over the P players. */
    HRL_REPLAY_PLAYERS_ALL = 1,
    /* PlayerReplay, one player per window: `players` (B,) is required, every field has a player axis of 1. */
    HRL_REPLAY_PLAYERS_SOLO = 2,
    /* PlayerReplay, make_batch's first branch (train.py:62-66): observation, policy, action_mask and action come
     * from each ply's first turn player (lowest set index of tmask, 0 if none) with a player axis of 1; the other
     * fields are per player: all P, or the window's one player when `players` is given. */
    HRL_REPLAY_PLAYERS_MOVER = 3,
};

/*
 * The ring.  Every pointer is a DEVICE pointer to a C-contiguous record.  With R = 1 for
 * HRL_REPLAY_MOVER_RECORDS and R = P otherwise (the records' player axis):
 *   obs[l]    (N, Tm, R, obs_width[l])  uint8 or fp32 per obs_type[l], l < nleaves <= 8
 *   policy    (N, Tm, R, A) fp32        amask  (N, Tm, R, A) fp32
 *   action    (N, Tm, R) int64          value  (N, Tm, R) fp32
 *   reward    (N, Tm, P) fp32           ret    (N, Tm, P) fp32
 *   length    (N,) int64                outcome (N, P) fp32
 *   turn      (N, Tm) int64             HRL_REPLAY_MOVER_RECORDS only (else ignored)
 *   tmask, omask (N, Tm, P) bytes 0/1   the PLAYERS layouts only (else ignored)
 * N is the slot count; it bounds nothing the kernel computes and is kept for validation (N >= 1).
 */
typedef struct hrl_replay_ring {
    int64_t N, Tm, P, A;
    int32_t nleaves;
    int32_t obs_type[HRL_REPLAY_MAX_LEAVES];
    int64_t obs_width[HRL_REPLAY_MAX_LEAVES];
    const void *obs[HRL_REPLAY_MAX_LEAVES];
    const float *policy, *amask;
    const int64_t *action;
    const float *value, *reward, *ret;
    const int64_t *length;
    const float *outcome;
    const int64_t *turn;
    const uint8_t *tmask, *omask;
} hrl_replay_ring;

/*
 * The batch: DEVICE pointers to C-contiguous outputs, all required, all written completely.  Pm is the player
 * axis of the four mover fields, Pn that of the others (see the layouts: 1 or P each).
 *   obs[l] (B, T, Pm, obs_width[l]) fp32   policy, amask (B, T, Pm, A) fp32   action (B, T, Pm, 1) int64
 *   value, reward, ret, turn_mask, observation_mask (B, T, Pn, 1) fp32        outcome (B, 1, Pn, 1) fp32
 *   episode_mask (B, T, 1, 1) fp32         progress (B, T, 1) fp32
 */
typedef struct hrl_replay_batch {
    float *obs[HRL_REPLAY_MAX_LEAVES];
    float *policy, *amask;
    int64_t *action;
    float *value, *outcome, *reward, *ret, *episode_mask, *turn_mask, *observation_mask, *progress;
} hrl_replay_batch;

/*
 * Window b covers plies start[b] + [0, T) of the episode in slot slots[b] (length L = length[slot]).  A ply
 * t < L is valid; a ply past the end reads row L-1.  With v = 1.0f for a valid ply and 0.0f otherwise, the fp32
 * operations are those of the torch formulation (rollout.DeviceReplay.gather / PlayerReplay.gather):
 *   observation, policy, reward, return, turn_mask, observation_mask   record * v  (a multiply: -x * 0 = -0)
 *   action        record * (int64)valid
 *   action_mask   valid ? record : 1e32f
 *   value         valid ? value : outcome  (MOVER_RECORDS: value * one_hot(turn) when valid)
 *   episode_mask  v         progress  valid ? (float)t / (float)L : 1.0f  (correctly rounded divide)
 *
 * slots, start, players: (B,) int64 device arrays; players may be NULL except for HRL_REPLAY_PLAYERS_SOLO and
 * must be NULL for HRL_REPLAY_MOVER_RECORDS and HRL_REPLAY_PLAYERS_ALL.
 * Preconditions on DEVICE data, not checked: 0 <= slot < N, 1 <= length <= Tm, 0 <= start, 0 <= player < P,
 * 0 <= turn < P.
 *
 * Addressing: record offsets are formed in 64 bits (a record may exceed 2^32 bytes); outputs are indexed in
 * 32 bits, so a call whose largest output has 2^31 elements or more is rejected.
 *
 * HRL_EINVAL for: a NULL ring / out / slots / start; B < 0; T < 1; N, Tm, P or A < 1; Tm >= 2^31; nleaves not in
 * [1, 8]; an obs_type other than the two above; an obs_width < 1; a NULL required record or output; an unknown
 * layout; players missing or present against the rule above; an output of 2^31 elements or more.
 * B == 0 passes the same validation, returns HRL_OK and launches nothing.
 */
int hrl_replay_gather(int layout, const hrl_replay_ring *ring, const int64_t *slots, const int64_t *start,
                      const int64_t *players, int64_t B, int64_t T, const hrl_replay_batch *out, void *stream);

/*
 * Draws B windows from the n = min(count, maximum_episodes) newest episodes of a ring whose next slot is `ptr`
 * and which holds `count` <= N episodes.  u: (3, B) fp32 uniforms in [0, 1), device memory.
 *
 * The rule is in integers (M = maximum_episodes; i = n-1 is the newest episode):
 *   weight of episode i    M - (n-1-i)                 (train.py:286-289's acceptance probability times M)
 *   C(i)                   (i+1)(M-n+1) + i(i+1)/2     the cumulative weight, int64
 *   x                      floor((double)u[0][b] * (double)C(n-1))   one IEEE multiply
 *   pick                   the smallest i with C(i) > x (binary search; n-1 if none)
 *   slots[b]               (ptr - n + pick) mod N      the ring's age order
 *   start[b]               min((int64)(u[1][b] * (float)cand), cand - 1),  cand = 1 + max(length[slot] - T, 0)
 *   players[b]             min((int64)(u[2][b] * (float)P), P - 1)        players may be NULL
 *
 * HRL_EINVAL for: B < 0; T < 1; P < 1; N < 1; maximum_episodes < 1 or >= 2^31; count < 1 or count > N; ptr
 * outside [0, N); a NULL u, length, slots or start.  B == 0 passes the same validation and launches nothing.
 */
int hrl_replay_draw(const float *u, int64_t B, int64_t ptr, int64_t count, int64_t N, int64_t maximum_episodes,
                    const int64_t *length, int64_t T, int64_t P, int64_t *slots, int64_t *start, int64_t *players,
                    void *stream);

#ifdef __cplusplus
}
#endif

#endif /* HRL_REPLAY_H */
