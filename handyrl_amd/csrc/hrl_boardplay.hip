// hrl_boardplay.hip — whole TicTacToe self-play games in ONE launch (gfx950): the lockstep generator's ply
// (rollout.DeviceGenerator._ply on a TicTacToeBatch with a nn.BoardInference net) for plies t0 <= t < t1, looped
// inside the kernel.  Nothing of a game depends on another game, so the 16 games of a board_infer_kernel tile stay
// in LDS for all their plies:
//   per ply   observation  the mover's view [1, board == color, board == -color] built in LDS from the board
//                          (TicTacToeBatch.observation(turn())), never read from HBM
//             forward      board_forward_tile (hrl_board_fwd.h): the device code board_infer_kernel runs, the weights
//                          streaming from L2 through LDS layer by layer as there
//             sampling     sample_record_kernel's arithmetic (hrl_selfplay.hip): m = legal ? 0 : 1e32f, p = logit - m,
//                          g = p - logf(-logf(u)), argmax by hrl_pick.h's `better` (NaN first, ties to the lowest label)
//             records      slot (e, t) of observation / policy / amask / action / value / turn: the live value of an
//                          active game (winner == 0 && nmoves < 9), else the reset value (0, 0, 1e32, 0, 0, 0); every
//                          slot of [t0, t1) is stored for every game
//             rules        TicTacToeBatch.step for active games: color placed at the cell, winner = color if one of
//                          the eight lines sums to 3 * color, color flipped, nmoves + 1
// The per-game state (9 + 1 + 4 + 1 bytes) is loaded once at t0 and stored once at t1; between the plies only the
// game's uniforms and its records touch HBM.  Rows past E in the last tile are finished games of zeros that store
// nothing.  A tile whose games have all finished skips the forward (a workgroup-uniform test on LDS) and stores the
// reset values.  One workgroup of 4 waves per 16 games; LDS board_infer_kernel's 78,464 B plus the tile's state,
// outputs and Gumbel scores (1,984 B), 80,448 B: two workgroups per CU.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hrl_env.h"
#include "../../include/hrl_targets.h"
#include "hrl_board_fwd.h"
#include "hrl_pick.h"

namespace {

constexpr int kOut = 10;   // a row's outputs: 9 logits and the value

__device__ __forceinline__ bool game_live(const int *s_win, const int *s_nm, int r) {
    return s_win[r] == 0 && s_nm[r] < kCells;
}

__global__ __launch_bounds__(kThreads, 2) void board_selfplay_kernel(
    const uint32_t *__restrict__ pack, int layers, int64_t E, int Tm, int t0, int t1, const float *__restrict__ U,
    int8_t *__restrict__ board, int8_t *__restrict__ color, int32_t *__restrict__ nmoves,
    int8_t *__restrict__ winner, float *__restrict__ obs, float *__restrict__ policy, float *__restrict__ amask,
    int64_t *__restrict__ action, float *__restrict__ value, int64_t *__restrict__ turn) {
    __shared__ __attribute__((aligned(16))) uint32_t w_lds_u[kLayerFragWords];   // 54 KB
    __shared__ float act[kTile * kStride];                                       // 18.1 KB
    __shared__ float obs_lds[kTile * kObs];
    __shared__ float head_w[kHeadWords];
    __shared__ float h_lds[kTile * kHMid];
    __shared__ int s_board[kTile * kCells];
    __shared__ int s_color[kTile], s_nm[kTile], s_win[kTile];
    __shared__ float s_out[kTile * kOut];
    __shared__ float s_g[kTile * kA];

    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kTile;
    const int valid = E - row0 < kTile ? (int)(E - row0) : kTile;   // >= 1: the grid is the tile count

    // the tile's games -> LDS; a row past E is a finished game on an empty board
    if (tid < kTile * kCells) s_board[tid] = tid < valid * kCells ? (int)board[row0 * kCells + tid] : 0;
    if (tid < kTile) {
        const bool in = tid < valid;
        s_color[tid] = in ? (int)color[row0 + tid] : 1;
        s_nm[tid] = in ? (int)nmoves[row0 + tid] : kCells;
        s_win[tid] = in ? (int)winner[row0 + tid] : 0;
    }
    __syncthreads();

#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        // the pack is read again every ply: its loads hoisted out of this loop (the stem's fragments and layer 0's
        // 14 prefetch registers per lane are loop-invariant) cost 100 VGPRs and the second workgroup of the CU
        // workgroup-uniform: every thread reads the same 16 games
        bool any = false;
        for (int r = 0; r < kTile; ++r) any = any || game_live(s_win, s_nm, r);

        // the ply's uniforms (9 per game, contiguous over the tile), in flight during the forward
        float u = 1.0f;
        if (tid < valid * kA) u = U[((int64_t)t * E + row0) * kA + tid];

        // the mover's view of every game -> LDS, and -> slot t of the observation record
        auto view = [&] {
            for (int i = tid; i < kTile * kObs; i += kThreads) {
                const int r = i / kObs, j = i - r * kObs;
                const int plane = j / kCells, cell = j - plane * kCells;
                const int b = s_board[r * kCells + cell], c = s_color[r];
                float v = plane == 0 ? 1.0f : (plane == 1 ? (b == c ? 1.0f : 0.0f) : (b == -c ? 1.0f : 0.0f));
                if (r >= valid) v = 0.0f;
                obs_lds[i] = v;
                if (r < valid) obs[((row0 + r) * Tm + t) * kObs + j] = game_live(s_win, s_nm, r) ? v : 0.0f;
            }
        };

        if (!any) view();   // only the record's reset values are needed
        if (any) {
            board_forward_tile(pack, layers, obs_lds, act, w_lds_u, head_w, h_lds, tid, view);   // hrl_board_fwd.h
            if (tid < kTile * kOut) {
                const int row = tid / kOut, o = tid - row * kOut;
                s_out[tid] = o < kA ? board_policy_out(h_lds, head_w, row, o) : board_value_out(h_lds, head_w, row);
            }
        }
        __syncthreads();   // s_out

        // sample_record_kernel's arithmetic, one lane per (game, label)
        if (tid < valid * kA) {
            const int r = tid / kA, j = tid - r * kA;
            const bool live = game_live(s_win, s_nm, r);
            const float m = s_board[tid] == 0 ? 0.0f : 1e32f;
            const float p = s_out[r * kOut + j] - m;
            s_g[tid] = p - logf(-logf(u));
            const int64_t slot = ((row0 + r) * Tm + t) * kA + j;
            policy[slot] = live ? p : 0.0f;
            amask[slot] = live ? m : 1e32f;
        }
        __syncthreads();   // s_g

        // one lane per game: the argmax, the scalar records, the rules
        if (tid < valid) {
            const int r = tid;
            const bool live = game_live(s_win, s_nm, r);
            float best = s_g[r * kA];
            int ib = 0;
            for (int j = 1; j < kA; ++j) {
                const float g = s_g[r * kA + j];
                if (better(g, j, best, ib)) {
                    best = g;
                    ib = j;
                }
            }
            const int64_t slot = (row0 + r) * Tm + t;
            action[slot] = live ? ib : 0;
            value[slot] = live ? s_out[r * kOut + kA] : 0.0f;
            turn[slot] = live ? s_nm[r] % 2 : 0;
            if (live) {   // TicTacToeBatch.step
                const int c = s_color[r];
                int *b = s_board + r * kCells;
                b[ib] = c;
                bool won = b[0] + b[4] + b[8] == 3 * c || b[2] + b[4] + b[6] == 3 * c;
                for (int k = 0; k < 3; ++k)
                    won = won || b[3 * k] + b[3 * k + 1] + b[3 * k + 2] == 3 * c || b[k] + b[k + 3] + b[k + 6] == 3 * c;
                if (won) s_win[r] = c;
                s_color[r] = -c;
                s_nm[r] += 1;
            }
        }
        __syncthreads();   // the state as the next ply reads it
    }

    if (tid < valid * kCells) board[row0 * kCells + tid] = (int8_t)s_board[tid];
    if (tid < valid) {
        color[row0 + tid] = (int8_t)s_color[tid];
        nmoves[row0 + tid] = s_nm[tid];
        winner[row0 + tid] = (int8_t)s_win[tid];
    }
}

}  // namespace

extern "C" {

int hrl_board_selfplay(const void *pack, int64_t layers, int64_t E, int64_t Tm, int64_t t0, int64_t t1, const float *U,
                       int8_t *board, int8_t *color, int32_t *nmoves, int8_t *winner, float *obs, float *policy,
                       float *amask, int64_t *action, float *value, int64_t *turn, void *stream) {
    if (!pack || !U || !board || !color || !nmoves || !winner || !obs || !policy || !amask || !action || !value ||
        !turn || layers < 1 || layers > kMaxLayers || (reinterpret_cast<uintptr_t>(pack) & 15) || E < 0 ||
        E > 0x7fffffff - kTile || Tm < 1 || Tm > kCells || t0 < 0 || t1 > Tm || t0 > t1)
        return HRL_EINVAL;
    if (E == 0 || t0 == t1) return HRL_OK;
    hipLaunchKernelGGL(board_selfplay_kernel, dim3((unsigned)((E + kTile - 1) / kTile)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint32_t *>(pack), (int)layers, E, (int)Tm,
                       (int)t0, (int)t1, U, board, color, nmoves, winner, obs, policy, amask, action, value, turn);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

}  // extern "C"
