// hrl_replay.hip — batch assembly from the device replay rings (handyrl/train.py:33-133 make_batch and
// :284-293 select_episode), see include/hrl_replay.h.
//
// As torch ops the gather is 40-50 launches (advanced indexing, one_hot, where, multiplies, .contiguous()) with a
// batch-sized temporary per field, followed by a second pass that copies the batch into the learner graph's
// static inputs; here it is ONE launch that writes the learner's buffers directly:
//   a workgroup owns the plies [t0, t0 + TC) of one window; for every field its slice of the output is one
//   contiguous run of TC * row elements, which the 256 lanes walk with a stride of 256 (coalesced stores; the
//   reads are contiguous too while the plies are valid, and the repeated last row past the episode's end);
//   TC is chosen on the host so that a workgroup moves a few thousand elements whatever the env's row widths, and
//   B * ceil(T / TC) workgroups cover the CUs at B = 256 as well as at B = 4096.
// Pure data movement (~30 MB at B=4096, T=32 on TicTacToe): latency bound, no LDS beyond one int per ply.
// Record offsets are 64-bit throughout (a Geister ring of 100,000 episodes has leaves past 2^32 bytes); output
// offsets are 32-bit, which the host guarantees by rejecting larger outputs.
//
// The draw is one lane per window: an inverse-CDF pick over integer weights by binary search on the closed-form
// cumulative weight, so that it equals a torch formulation of the same integers exactly.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrl_replay.h"
#include "../../include/hrl_targets.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTC = 64;          // plies per workgroup at most (one LDS int each)
constexpr int kTargetElems = 4096;  // elements a workgroup should move, roughly

struct GatherArgs {
    hrl_replay_ring r;
    hrl_replay_batch o;
    const int64_t *slots, *start, *players;
    int layout, T, TC, nchunk;
};

__global__ __launch_bounds__(kThreads) void gather_kernel(const GatherArgs a) {
    __shared__ int s_mp[kMaxTC];   // HRL_REPLAY_PLAYERS_MOVER: the ply's first turn player
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.nchunk, c = blockIdx.x - b * a.nchunk;
    const int t0 = c * a.TC;
    const int nT = min(a.TC, a.T - t0);
    const int P = (int)a.r.P, A = (int)a.r.A;
    const int64_t slot = a.slots[b], st = a.start[b], L = a.r.length[slot];
    // plies [0, nv) of this chunk are valid (t < L); the rest read row L-1
    const int64_t left = L - (st + t0);
    const int nv = left <= 0 ? 0 : (left >= nT ? nT : (int)left);
    const int64_t row0 = slot * a.r.Tm, rowv = row0 + st + t0, rowl = row0 + L - 1;
    const bool mover_rec = a.layout == HRL_REPLAY_MOVER_RECORDS;
    const bool first_turn = a.layout == HRL_REPLAY_PLAYERS_MOVER;
    const int R = mover_rec ? 1 : P;                        // player axis of the mover fields' records
    const int p0 = a.players ? (int)a.players[b] : 0;
    const int Pn = a.players ? 1 : P;                       // player axis of the per-player outputs
    const int Pm = (mover_rec || first_turn) ? 1 : Pn;      // ... of observation, policy, action_mask, action
    const int bt = b * a.T + t0;                            // first (window, ply) cell of this workgroup

    if (first_turn) {
        for (int tt = tid; tt < nT; tt += kThreads) {
            const uint8_t *m = a.r.tmask + (tt < nv ? rowv + tt : rowl) * P;
            int q = 0;
            for (int p = P - 1; p >= 0; --p) q = m[p] ? p : q;
            s_mp[tt] = q;
        }
        __syncthreads();
    }

    // a field of `W` elements per (ply, player): out (.., Pm, W) <- record (.., R, W)
    auto wide = [&](auto *src, int W, auto &&store) {
        const int PW = Pm * W, n = nT * PW;
        for (int i = tid; i < n; i += kThreads) {
            const int tt = i / PW, r = i - tt * PW;
            const int q = Pm == 1 ? 0 : r / W, j = r - q * W;
            const bool valid = tt < nv;
            const int sp = mover_rec ? 0 : (first_turn ? s_mp[tt] : p0 + q);
            const int64_t row = valid ? rowv + tt : rowl;
            store(bt * PW + i, src[(row * R + sp) * W + j], valid);
        }
    };

    for (int l = 0; l < a.r.nleaves; ++l) {
        float *out = a.o.obs[l];
        const int W = (int)a.r.obs_width[l];
        if (a.r.obs_type[l] == HRL_REPLAY_U8)
            wide(static_cast<const uint8_t *>(a.r.obs[l]), W,
                 [&](int o, uint8_t x, bool valid) { out[o] = (float)x * (valid ? 1.0f : 0.0f); });
        else
            wide(static_cast<const float *>(a.r.obs[l]), W,
                 [&](int o, float x, bool valid) { out[o] = x * (valid ? 1.0f : 0.0f); });
    }
    wide(a.r.policy, A, [&](int o, float x, bool valid) { a.o.policy[o] = x * (valid ? 1.0f : 0.0f); });
    wide(a.r.amask, A, [&](int o, float x, bool valid) { a.o.amask[o] = valid ? x : 1e32f; });
    wide(a.r.action, 1, [&](int o, int64_t x, bool valid) { a.o.action[o] = x * (int64_t)valid; });

    // the per-player scalars
    for (int i = tid; i < nT * Pn; i += kThreads) {
        const int tt = i / Pn, q = i - tt * Pn, p = p0 + q;
        const bool valid = tt < nv;
        const float v = valid ? 1.0f : 0.0f;
        const int64_t row = valid ? rowv + tt : rowl;
        const int o = bt * Pn + i;
        const float oc = a.r.outcome[slot * P + p];
        a.o.reward[o] = a.r.reward[row * P + p] * v;
        a.o.ret[o] = a.r.ret[row * P + p] * v;
        if (mover_rec) {
            const float onehot = (a.r.turn[row] == p ? 1.0f : 0.0f) * v;
            a.o.value[o] = valid ? onehot * a.r.value[row] : oc;
            a.o.turn_mask[o] = onehot;
            a.o.observation_mask[o] = onehot;
        } else {
            a.o.value[o] = valid ? a.r.value[row * P + p] : oc;
            a.o.turn_mask[o] = (float)a.r.tmask[row * P + p] * v;
            a.o.observation_mask[o] = (float)a.r.omask[row * P + p] * v;
        }
    }
    for (int tt = tid; tt < nT; tt += kThreads) {
        const bool valid = tt < nv;
        a.o.episode_mask[bt + tt] = valid ? 1.0f : 0.0f;
        a.o.progress[bt + tt] = valid ? __fdiv_rn((float)(st + t0 + tt), (float)L) : 1.0f;
    }
    if (c == 0)
        for (int q = tid; q < Pn; q += kThreads) a.o.outcome[b * Pn + q] = a.r.outcome[slot * P + p0 + q];
}

__global__ __launch_bounds__(kThreads) void draw_kernel(const float *__restrict__ u, int64_t B, int64_t ptr,
                                                        int64_t n, int64_t N, int64_t M,
                                                        const int64_t *__restrict__ length, int64_t T, int64_t P,
                                                        int64_t *__restrict__ slots, int64_t *__restrict__ start,
                                                        int64_t *__restrict__ players) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const int64_t base = M - n + 1;
    auto C = [&](int64_t i) { return (i + 1) * base + i * (i + 1) / 2; };
    const int64_t x = (int64_t)floor((double)u[b] * (double)C(n - 1));
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (C(mid) > x)
            hi = mid;
        else
            lo = mid + 1;
    }
    int64_t slot = (ptr - n + lo) % N;
    slot += slot < 0 ? N : 0;
    slots[b] = slot;
    const int64_t over = length[slot] - T;
    const int64_t cand = 1 + (over > 0 ? over : 0);
    const int64_t s = (int64_t)(u[B + b] * (float)cand);
    start[b] = s < cand - 1 ? s : cand - 1;
    if (players) {
        const int64_t p = (int64_t)(u[2 * B + b] * (float)P);
        players[b] = p < P - 1 ? p : P - 1;
    }
}

}  // namespace

extern "C" {

int hrl_replay_gather(int layout, const hrl_replay_ring *ring, const int64_t *slots, const int64_t *start,
                      const int64_t *players, int64_t B, int64_t T, const hrl_replay_batch *out, void *stream) {
    if (!ring || !out || !slots || !start || B < 0 || T < 1) return HRL_EINVAL;
    if (layout < HRL_REPLAY_MOVER_RECORDS || layout > HRL_REPLAY_PLAYERS_MOVER) return HRL_EINVAL;
    if (ring->N < 1 || ring->Tm < 1 || ring->Tm > 0x7fffffff || ring->P < 1 || ring->A < 1) return HRL_EINVAL;
    if (ring->nleaves < 1 || ring->nleaves > HRL_REPLAY_MAX_LEAVES) return HRL_EINVAL;
    const bool mover_rec = layout == HRL_REPLAY_MOVER_RECORDS;
    if (layout == HRL_REPLAY_PLAYERS_SOLO && !players) return HRL_EINVAL;
    if ((mover_rec || layout == HRL_REPLAY_PLAYERS_ALL) && players) return HRL_EINVAL;
    if (!ring->policy || !ring->amask || !ring->action || !ring->value || !ring->reward || !ring->ret ||
        !ring->length || !ring->outcome || (mover_rec ? !ring->turn : (!ring->tmask || !ring->omask)))
        return HRL_EINVAL;
    if (!out->policy || !out->amask || !out->action || !out->value || !out->outcome || !out->reward || !out->ret ||
        !out->episode_mask || !out->turn_mask || !out->observation_mask || !out->progress)
        return HRL_EINVAL;
    const int64_t Pn = players ? 1 : ring->P;
    const int64_t Pm = (mover_rec || layout == HRL_REPLAY_PLAYERS_MOVER) ? 1 : Pn;
    const int64_t kLimit = INT64_C(0x7fffffff);
    if (ring->P > kLimit || ring->A > kLimit) return HRL_EINVAL;
    int64_t widest = ring->A, per_ply = 2 * ring->A + 1;   // elements of the mover fields per (ply, player)
    for (int l = 0; l < ring->nleaves; ++l) {
        if (!ring->obs[l] || !out->obs[l] || ring->obs_width[l] < 1 || ring->obs_width[l] > kLimit ||
            (ring->obs_type[l] != HRL_REPLAY_U8 && ring->obs_type[l] != HRL_REPLAY_F32))
            return HRL_EINVAL;
        widest = ring->obs_width[l] > widest ? ring->obs_width[l] : widest;
        per_ply += ring->obs_width[l];
    }
    // the largest output, in elements, must fit the kernel's int indexing (the division avoids overflow)
    const int64_t row = Pm * widest > Pn ? Pm * widest : Pn;
    if (T > kLimit || row > kLimit / T || (B > 0 && T * row > kLimit / B)) return HRL_EINVAL;
    if (B == 0) return HRL_OK;
    per_ply = per_ply * Pm + 5 * Pn + 2;
    int64_t TC = (kTargetElems + per_ply - 1) / per_ply;
    TC = TC < 1 ? 1 : (TC > kMaxTC ? kMaxTC : TC);
    TC = TC > T ? T : TC;
    const int64_t nchunk = (T + TC - 1) / TC;
    if (nchunk > kLimit / B) return HRL_EINVAL;
    GatherArgs a;
    a.r = *ring;
    a.o = *out;
    a.slots = slots;
    a.start = start;
    a.players = players;
    a.layout = layout;
    a.T = (int)T;
    a.TC = (int)TC;
    a.nchunk = (int)nchunk;
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)(B * nchunk)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

int hrl_replay_draw(const float *u, int64_t B, int64_t ptr, int64_t count, int64_t N, int64_t maximum_episodes,
                    const int64_t *length, int64_t T, int64_t P, int64_t *slots, int64_t *start, int64_t *players,
                    void *stream) {
    if (!u || !length || !slots || !start || B < 0 || T < 1 || P < 1 || N < 1 || maximum_episodes < 1 ||
        maximum_episodes > 0x7fffffff || count < 1 || count > N || ptr < 0 || ptr >= N)
        return HRL_EINVAL;
    if (B == 0) return HRL_OK;
    const int64_t blocks = (B + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return HRL_EINVAL;
    const int64_t n = count < maximum_episodes ? count : maximum_episodes;
    hipLaunchKernelGGL(draw_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), u,
                       B, ptr, n, N, maximum_episodes, length, T, P, slots, start, players);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

}  // extern "C"
