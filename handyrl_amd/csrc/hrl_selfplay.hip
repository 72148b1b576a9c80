// hrl_selfplay.hip — the sampling and recording tail of a self-play ply (handyrl/generation.py:43-62).
//
// Per ply the reference masks the illegal actions' logits (-1e32, generation.py:50-51), samples an action
// from softmax over the legal ones (random.choices, :53) and appends the moment (observation, policy,
// action_mask, action, value, reward, turn) to the episode (:55-62).  DeviceGenerator does that for E games
// at once with Gumbel-max over uniforms drawn up front; as torch ops it is ~25 launches per ply (mask,
// subtract, two logs, argmax, a where + index_copy per record), here ONE launch:
//   one wave per game, lanes over the A action labels:
//     m = legal ? 0 : 1e32;  p = logit - m;  g = p - log(-log(u))      (the torch formulation's fp32 ops)
//     action = argmax g, ties to the lowest label, NaN first (torch.argmax's order), shuffle reduction
//   slot t of each record gets the game's value when it is active and the reset value otherwise
//   (policy 0, action mask 1e32, action / value / turn / reward 0).
// The ply index t is read from device memory, so the launch is replayed unchanged by the ply's HIP graph.
// HBM-light (E*A*(4+1+4 in, 4+4 out) bytes, ~18 MB per ply at E=2048, A=214): latency bound.
//
// The streaming generator (rollout.StreamGenerator: every slot at its own ply, finished games restart in place)
// has its own tail, sample_record_stream_kernel -- slot (e, ply[e]), uniforms from Philox4x32-10 inside the wave,
// no (Tm, E, A) uniform buffer -- and its harvest: harvest_kernel copies a finished game's records into the replay
// ring (DeviceReplay.add's ten index_copy_ launches and the return loop as one launch), harvest_advance_kernel
// restarts the slots and advances the ring state, which lives in device memory.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hrl_env.h"
#include "../../include/hrl_targets.h"
#include "hrl_pick.h"

namespace {

constexpr int kGamesPerBlock = 4;

__global__ __launch_bounds__(kWave *kGamesPerBlock) void sample_record_kernel(
    const float *__restrict__ logits, int64_t lstride, const uint8_t *__restrict__ legal,
    const float *__restrict__ U, const int64_t *__restrict__ tptr, const float *__restrict__ value,
    const uint8_t *__restrict__ active, const int64_t *__restrict__ player, const double *__restrict__ reward,
    int64_t E, int A, int64_t Tm, int P, int64_t *__restrict__ action, float *__restrict__ policy_buf,
    float *__restrict__ amask_buf, int64_t *__restrict__ action_buf, float *__restrict__ value_buf,
    int64_t *__restrict__ turn_buf, double *__restrict__ reward_buf) {
    const int lane = threadIdx.x % kWave;
    const int64_t e = (int64_t)blockIdx.x * kGamesPerBlock + threadIdx.x / kWave;
    if (e >= E) return;
    const int64_t t = *tptr;
    const bool live = active[e] != 0;
    const float *lg = logits + e * lstride;
    const uint8_t *lm = legal + e * A;
    const float *u = U + (t * E + e) * A;
    float *pol = policy_buf + (e * Tm + t) * A;
    float *am = amask_buf + (e * Tm + t) * A;
    float best = 0.0f;
    int ib = A;   // no label yet
    for (int j = lane; j < A; j += kWave) {
        const float m = lm[j] ? 0.0f : 1e32f;
        const float p = lg[j] - m;
        const float g = p - logf(-logf(u[j]));
        if (ib == A || better(g, j, best, ib)) {
            best = g;
            ib = j;
        }
        pol[j] = live ? p : 0.0f;
        am[j] = live ? m : 1e32f;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(ib, off);
        if (oi != A && (ib == A || better(ob, oi, best, ib))) {
            best = ob;
            ib = oi;
        }
    }
    if (lane == 0) {
        action[e] = ib;
        const int64_t s = e * Tm + t;
        action_buf[s] = live ? ib : 0;
        value_buf[s] = live ? value[e] : 0.0f;
        turn_buf[s] = live ? player[e] : 0;
        if (reward && reward_buf)
            for (int q = 0; q < P; ++q) reward_buf[s * P + q] = live ? reward[e * P + q] : 0.0;
    }
}

// ---- the streaming generator's tail: per-game ply index, uniforms from a counter-based generator ----
// Philox4x32-10 (hrl_pick.h).  The rule (key, counter, word, uniform) is public: include/hrl_env.h and
// rollout.stream_uniforms, which this reproduces bit for bit.

// sample_record_kernel with the slot (e, ply[e]) and u computed here; an inactive game stores no record.
__global__ __launch_bounds__(kWave *kGamesPerBlock) void sample_record_stream_kernel(
    const float *__restrict__ logits, int64_t lstride, const uint8_t *__restrict__ legal, uint32_t k0, uint32_t k1,
    const int64_t *__restrict__ game, const int64_t *__restrict__ ply, const float *__restrict__ value,
    const uint8_t *__restrict__ active, const int64_t *__restrict__ player, const double *__restrict__ reward,
    int64_t E, int A, int64_t Tm, int P, int64_t *__restrict__ action, float *__restrict__ policy_buf,
    float *__restrict__ amask_buf, int64_t *__restrict__ action_buf, float *__restrict__ value_buf,
    int64_t *__restrict__ turn_buf, double *__restrict__ reward_buf) {
    const int lane = threadIdx.x % kWave;
    const int64_t e = (int64_t)blockIdx.x * kGamesPerBlock + threadIdx.x / kWave;
    if (e >= E) return;
    const int64_t t = ply[e];
    if (!active[e] || t < 0 || t >= Tm) {   // wave-uniform
        if (lane == 0) action[e] = 0;
        return;
    }
    const uint64_t n = (uint64_t)game[e];
    const uint32_t n0 = (uint32_t)n, n1 = (uint32_t)(n >> 32), tw = (uint32_t)t;
    const float *lg = logits + e * lstride;
    const uint8_t *lm = legal + e * A;
    float *pol = policy_buf + (e * Tm + t) * A;
    float *am = amask_buf + (e * Tm + t) * A;
    float best = 0.0f;
    int ib = A;   // no label yet
    for (int j = lane; j < A; j += kWave) {
        const uint32_t x = philox_word(k0, k1, n0, n1, tw, (uint32_t)(j >> 2), j & 3);
        const float u = ((float)(x >> 9) + 0.5f) * 0x1p-23f;
        const float m = lm[j] ? 0.0f : 1e32f;
        const float p = lg[j] - m;
        const float g = p - logf(-logf(u));
        if (ib == A || better(g, j, best, ib)) {
            best = g;
            ib = j;
        }
        pol[j] = p;
        am[j] = m;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(ib, off);
        if (oi != A && (ib == A || better(ob, oi, best, ib))) {
            best = ob;
            ib = oi;
        }
    }
    if (lane == 0) {
        action[e] = ib;
        const int64_t s = e * Tm + t;
        action_buf[s] = ib;
        value_buf[s] = value[e];
        turn_buf[s] = player[e];
        if (reward && reward_buf)
            for (int q = 0; q < P; ++q) reward_buf[s * P + q] = reward[e * P + q];
    }
}

// ---- the streaming generator's harvest: finished games -> ring rows, their slots restarted ----
// Grid (E / kSlotsPerBlock, kHarvestSplit + 1): a block skips a slot that is not done; for a done one it counts
// the done slots below it (the ring row); kHarvestSplit of them copy a share each of every record of the episode and the
// last one forms the returns (harvest_returns) and stores length, outcome and game number.  A slot's record of one
// field is Tm * width contiguous floats, in the slot and in the ring row alike, so it is copied as one flat run:
// 16 bytes per lane where Tm * width is a multiple of four (every Geister field: Tm = 202 is even and the widths
// 252, 18 and 214 are; value's 202 is not), else element by element.  A ply's validity is a bound on the flat
// index (t < L  <=>  i < L * width), so no lane divides.  ~570 KB per Geister episode, HBM-bound.
constexpr int kHarvestThreads = 256;
constexpr int kHarvestSplit = 8;
constexpr int kFloatFields = HRL_REPLAY_MAX_LEAVES + 3;   // obs leaves, policy, amask, value

struct HarvestArgs {
    const float *fsrc[kFloatFields];
    void *fdst[kFloatFields];
    int64_t fwidth[kFloatFields];
    float ffill[kFloatFields];
    int32_t ftype[kFloatFields];   // HRL_REPLAY_U8 / HRL_REPLAY_F32
    int32_t fvec[kFloatFields];    // 16-byte loads (and 16- / 4-byte stores) are aligned for every slot and row
    int32_t nf, P;
    const int64_t *action, *turn;
    int64_t *r_action, *r_turn;
    const double *reward;
    float *r_reward, *r_ret, *r_outcome;
    int64_t *r_length, *ring_game;
    const float *outcome;
    const int64_t *game, *ply, *state;
    const uint8_t *done;
    int64_t E, Tm, N;
    double gamma;
};

// ret[t] = reward[t] + gamma * ret[t+1] per player, fp64 from t = L-1 down, stored as fp32; zeros from L on.  The
// scan is a dependent chain, so its operands must not come from HBM one by one (202 round trips: 40 us measured):
// the block stages kScanElems rewards at a time in LDS, lane q scans player q there in place, and the block
// stores the chunk coalesced.  More players than lanes or than a chunk holds: the plain loop.
constexpr int kScanElems = 2048;
__device__ void harvest_returns(const HarvestArgs &a, int64_t e, int64_t row, int64_t L) {
    __shared__ double s_rew[kScanElems];
    const int P = a.P;
    const int64_t TP = a.Tm * P;
    float *ret = a.r_ret + row * TP;
    for (int64_t i = L * P + threadIdx.x; i < TP; i += kHarvestThreads) ret[i] = 0.0f;
    if (L == 0) return;
    const double *rew = a.reward + e * TP;
    if (P > kHarvestThreads || P > kScanElems) {
        for (int q = threadIdx.x; q < P; q += kHarvestThreads) {
            double acc = 0.0;
            for (int64_t t = L - 1; t >= 0; --t) {
                acc = rew[t * P + q] + a.gamma * acc;
                ret[t * P + q] = (float)acc;
            }
        }
        return;
    }
    const int64_t per = kScanElems / P;   // plies per chunk
    double acc = 0.0;                     // lane q's carry across the chunks
    for (int64_t hi = L; hi > 0; hi -= per) {
        const int64_t lo = hi > per ? hi - per : 0;
        const int64_t n = (hi - lo) * P;
        for (int64_t i = threadIdx.x; i < n; i += kHarvestThreads) s_rew[i] = rew[lo * P + i];
        __syncthreads();
        if ((int)threadIdx.x < P)
            for (int64_t t = hi - lo - 1; t >= 0; --t) {
                acc = s_rew[t * P + threadIdx.x] + a.gamma * acc;
                s_rew[t * P + threadIdx.x] = acc;
            }
        __syncthreads();
        for (int64_t i = threadIdx.x; i < n; i += kHarvestThreads) ret[lo * P + i] = (float)s_rew[i];
        __syncthreads();
    }
}

// The ring row and the length of done slot e: false when a higher slot claims the row in the same call.  Block-uniform.
__device__ bool harvest_row(const HarvestArgs &a, int64_t e, int *s_r, int *s_c, int64_t *row_out, int64_t *L_out) {
    int r = 0, c = 0;
    for (int64_t i = threadIdx.x; i < a.E; i += kHarvestThreads) {
        const int d = a.done[i] != 0;
        c += d;
        r += d & (i < e);
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        r += __shfl_xor(r, off);
        c += __shfl_xor(c, off);
    }
    if (threadIdx.x % kWave == 0) {
        s_r[threadIdx.x / kWave] = r;
        s_c[threadIdx.x / kWave] = c;
    }
    __syncthreads();
    r = c = 0;
    for (int w = 0; w < kHarvestThreads / kWave; ++w) {
        r += s_r[w];
        c += s_c[w];
    }
    if ((int64_t)r + a.N < (int64_t)c) return false;   // a higher slot claims this row in the same call
    int64_t base = a.state[0] % a.N;
    if (base < 0) base += a.N;
    *row_out = (base + r) % a.N;
    const int64_t L = a.ply[e];
    *L_out = L < 0 ? 0 : L > a.Tm ? a.Tm : L;
    return true;
}

// The slot's last block: the returns, length, outcome, game number.
__device__ void harvest_tail(const HarvestArgs &a, int64_t e, int64_t row, int64_t L) {
    harvest_returns(a, e, row, a.reward ? L : 0);
    for (int q = threadIdx.x; q < a.P; q += kHarvestThreads) a.r_outcome[row * a.P + q] = a.outcome[e * a.P + q];
    if (threadIdx.x == 0) {
        a.r_length[row] = L;
        a.ring_game[row] = a.game[e];
    }
}

// One done slot e, by the block's share blockIdx.y; every branch that leaves is block-uniform.
__device__ void harvest_slot(const HarvestArgs &a, int64_t e, int *s_r, int *s_c) {
    int64_t row, L;
    if (!harvest_row(a, e, s_r, s_c, &row, &L)) return;
    const int64_t TP = a.Tm * a.P;
    if (blockIdx.y == kHarvestSplit) {
        harvest_tail(a, e, row, L);
        return;
    }
    const int64_t first = (int64_t)blockIdx.y * kHarvestThreads + threadIdx.x;
    const int64_t step = (int64_t)kHarvestSplit * kHarvestThreads;
    for (int f = 0; f < a.nf; ++f) {
        const int64_t total = a.Tm * a.fwidth[f], lim = L * a.fwidth[f];
        const float *src = a.fsrc[f] + e * total;
        const float fill = a.ffill[f];
        const bool u8 = a.ftype[f] == HRL_REPLAY_U8;
        float *df = static_cast<float *>(a.fdst[f]) + row * total;
        uint8_t *db = static_cast<uint8_t *>(a.fdst[f]) + row * total;
        if (a.fvec[f]) {
            for (int64_t i = first; i < total / 4; i += step) {
                float4 v = reinterpret_cast<const float4 *>(src)[i];
                const int64_t j = i * 4;
                v.x = j < lim ? v.x : fill;
                v.y = j + 1 < lim ? v.y : fill;
                v.z = j + 2 < lim ? v.z : fill;
                v.w = j + 3 < lim ? v.w : fill;
                if (u8)
                    reinterpret_cast<uchar4 *>(db)[i] =
                        make_uchar4((uint8_t)(int)v.x, (uint8_t)(int)v.y, (uint8_t)(int)v.z, (uint8_t)(int)v.w);
                else
                    reinterpret_cast<float4 *>(df)[i] = v;
            }
        } else {
            for (int64_t i = first; i < total; i += step) {
                const float v = i < lim ? src[i] : fill;
                if (u8)
                    db[i] = (uint8_t)(int)v;
                else
                    df[i] = v;
            }
        }
    }
    for (int64_t i = first; i < a.Tm; i += step) {
        a.r_action[row * a.Tm + i] = i < L ? a.action[e * a.Tm + i] : 0;
        a.r_turn[row * a.Tm + i] = i < L ? a.turn[e * a.Tm + i] : 0;
    }
    for (int64_t i = first; i < TP; i += step)
        a.r_reward[row * TP + i] = (a.reward && i < L * a.P) ? (float)a.reward[e * TP + i] : 0.0f;
}

// A block looks at kSlotsPerBlock slots.  One per block is the measured choice: eight per block (a ninth of the
// workgroups that only read one byte) was slower, 28 against 22 us per Geister ply at E = 2,048 and 31 against 21 us
// for TicTacToe at E = 4,096, where some 500 games end per ply and a block then copies its done slots in turn.
constexpr int kSlotsPerBlock = 1;
__global__ __launch_bounds__(kHarvestThreads) void harvest_kernel(const HarvestArgs a) {
    __shared__ int s_r[kHarvestThreads / kWave], s_c[kHarvestThreads / kWave];
    const int64_t e0 = (int64_t)blockIdx.x * kSlotsPerBlock;
    for (int k = 0; k < kSlotsPerBlock && e0 + k < a.E; ++k) {
        if (!a.done[e0 + k]) continue;   // block-uniform
        harvest_slot(a, e0 + k, s_r, s_c);
        __syncthreads();                 // the next slot reuses the LDS words
    }
}

// One workgroup, after harvest_kernel on the stream: the done slots restart (next game number, ply 0, pending) and
// the ring state advances.  Thread k owns the slots [k * chunk, (k + 1) * chunk).
__global__ __launch_bounds__(kHarvestThreads) void harvest_advance_kernel(
    const uint8_t *__restrict__ done, int64_t E, int64_t N, int64_t *__restrict__ game, int64_t *__restrict__ ply,
    uint8_t *__restrict__ pending, int64_t *__restrict__ state) {
    __shared__ int s_wave[kHarvestThreads / kWave];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int64_t chunk = (E + kHarvestThreads - 1) / kHarvestThreads;
    const int64_t lo = threadIdx.x * chunk < E ? threadIdx.x * chunk : E, hi = lo + chunk < E ? lo + chunk : E;
    int cnt = 0;
    for (int64_t i = lo; i < hi; ++i) cnt += done[i] != 0;
    int incl = cnt;   // inclusive scan over the wave's lanes, then over the waves
    for (int off = 1; off < kWave; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == kWave - 1) s_wave[wave] = incl;
    const int64_t base = state[0], emitted = state[1], next = state[2];
    __syncthreads();
    int64_t pre = incl - cnt, total = 0;
    for (int w = 0; w < kHarvestThreads / kWave; ++w) {
        pre += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
    }
    for (int64_t i = lo; i < hi; ++i)
        if (done[i]) {
            game[i] = next + pre++;
            ply[i] = 0;
            pending[i] = 1;
        }
    if (threadIdx.x == 0 && total > 0) {
        int64_t b = base % N;
        if (b < 0) b += N;
        state[0] = (b + total) % N;
        state[1] = emitted + total;
        state[2] = next + total;
    }
}

// ---- the per-player streaming generator (rollout.PlayerStreamGenerator): simultaneous-move envs ----
// The public rules (w3 of the counter) are in include/hrl_env.h and rollout.stream_player_uniforms /
// stream_select_uniform.

constexpr uint32_t kPlayerW3 = 0x40000000u, kSelectW3 = 0x80000000u;

__device__ __forceinline__ float philox_uniform(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 0x1p-23f; }

// sample_record_stream_kernel with one wave per (game, player): every player's slot of a played game is stored.
__global__ __launch_bounds__(kWave *kGamesPerBlock) void sample_record_players_stream_kernel(
    const float *__restrict__ logits, int64_t lstride, const float *__restrict__ value,
    const uint8_t *__restrict__ legal, int64_t lpstride, const uint8_t *__restrict__ turns,
    const uint8_t *__restrict__ infer, const uint8_t *__restrict__ active, uint32_t k0, uint32_t k1,
    const int64_t *__restrict__ game, const int64_t *__restrict__ ply, int64_t E, int P, int A, int64_t Tm,
    int64_t *__restrict__ action, float *__restrict__ usel, float *__restrict__ policy_buf,
    float *__restrict__ amask_buf, int64_t *__restrict__ action_buf, float *__restrict__ value_buf,
    uint8_t *__restrict__ tmask_buf, uint8_t *__restrict__ omask_buf) {
    const int lane = threadIdx.x % kWave;
    const int64_t w = (int64_t)blockIdx.x * kGamesPerBlock + threadIdx.x / kWave;   // the pair e * P + p
    if (w >= E * P) return;
    const int64_t e = w / P;
    const int p = (int)(w - e * P);
    const int64_t t = ply[e];
    const uint64_t n = (uint64_t)game[e];
    const uint32_t n0 = (uint32_t)n, n1 = (uint32_t)(n >> 32), tw = (uint32_t)(uint64_t)t;
    if (p == 0 && lane == 0) usel[e] = philox_uniform(philox_word(k0, k1, n0, n1, tw, kSelectW3, 0));
    if (!active[e] || t < 0 || t >= Tm) {   // wave-uniform
        if (lane == 0) action[w] = 0;
        return;
    }
    const bool turn = turns[w] != 0;
    const int64_t row = (int64_t)p * E + e;
    const float *lg = logits + row * lstride;
    const uint8_t *lm = legal + e * (lpstride ? (int64_t)P * A : (int64_t)A) + p * lpstride;
    const int64_t s = (e * Tm + t) * P + p;
    float *pol = policy_buf + s * A;
    float *am = amask_buf + s * A;
    const uint32_t w3 = kPlayerW3 + (uint32_t)p * (uint32_t)((A + 3) >> 2);
    float best = 0.0f;
    int ib = A;   // no label yet
    for (int j = lane; j < A; j += kWave) {
        const float u = philox_uniform(philox_word(k0, k1, n0, n1, tw, w3 + (uint32_t)(j >> 2), j & 3));
        const float m = lm[j] ? 0.0f : 1e32f;
        const float pv = lg[j] - m;
        const float g = pv - logf(-logf(u));
        if (ib == A || better(g, j, best, ib)) {
            best = g;
            ib = j;
        }
        pol[j] = turn ? pv : 0.0f;
        am[j] = turn ? m : 1e32f;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(ib, off);
        if (oi != A && (ib == A || better(ob, oi, best, ib))) {
            best = ob;
            ib = oi;
        }
    }
    if (lane == 0) {
        const int64_t a = turn ? ib : 0;
        const bool inf = infer[w] != 0;
        action[w] = a;
        action_buf[s] = a;
        tmask_buf[s] = turn ? 1 : 0;
        value_buf[s] = inf ? value[row] : 0.0f;
        omask_buf[s] = inf ? 1 : 0;
    }
}

// The per-player harvest.  The grid and the row rule are harvest_kernel's (harvest_row, harvest_tail); what differs is
// the copy.  A slot's record of one field is Tm * width contiguous elements (width = P * w), uint8 or fp32 on either
// side, and a Hungry Geese leaf is 1 MB per slot of which the mean game fills a few plies: the source is read for
// the flat indices below lim = L * width only (copy_run), and [lim, total) is stores of the reset value
// (fill_run), 16 bytes per lane between the run's unaligned edges.  The copy's unit -- 16, 4 or 1 source elements
// per lane -- is the largest that is aligned for every slot and row (the host decides: PlayerField::unit).
template <typename T> struct Elem;
template <> struct Elem<float> {
    __device__ static float to_f(float x) { return x; }
    __device__ static float from_f(float x) { return x; }
};
template <> struct Elem<uint8_t> {
    __device__ static float to_f(uint8_t x) { return (float)x; }
    __device__ static uint8_t from_f(float x) { return (uint8_t)(int)x; }
};
// src.to(dst.dtype): uint8 -> uint8 and fp32 -> fp32 keep the bits
template <typename S, typename D> __device__ __forceinline__ D convert(S x) { return Elem<D>::from_f(Elem<S>::to_f(x)); }
template <> __device__ __forceinline__ uint8_t convert<uint8_t, uint8_t>(uint8_t x) { return x; }

// four elements from a 16-byte aligned (fp32) or 4-byte aligned (uint8) address, and four to one
__device__ __forceinline__ void load4(const float *p, float *x) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
}
__device__ __forceinline__ void load4(const uint8_t *p, uint8_t *x) {
    const uchar4 v = *reinterpret_cast<const uchar4 *>(p);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
}
__device__ __forceinline__ void store4(float *p, const float *x) {
    *reinterpret_cast<float4 *>(p) = make_float4(x[0], x[1], x[2], x[3]);
}
__device__ __forceinline__ void store4(uint8_t *p, const uint8_t *x) {
    *reinterpret_cast<uchar4 *>(p) = make_uchar4(x[0], x[1], x[2], x[3]);
}

template <typename S, typename D>
__device__ void copy_run(const S *src, D *dst, int64_t lim, int unit, int64_t first, int64_t step) {
    int64_t done = 0;
    if (sizeof(S) == 1 && unit == 16) {   // uint8 sources only: one 16-byte load per lane
        const int64_t nv = lim >> 4;
        for (int64_t i = first; i < nv; i += step) {
            const uint4 v = reinterpret_cast<const uint4 *>(src)[i];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            D out[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) out[k] = convert<uint8_t, D>((uint8_t)(w[k >> 2] >> (8 * (k & 3))));
#pragma unroll
            for (int k = 0; k < 16; k += 4) store4(dst + i * 16 + k, out + k);
        }
        done = nv << 4;
    } else if (unit == 4) {
        const int64_t nv = lim >> 2;
        for (int64_t i = first; i < nv; i += step) {
            S in[4];
            D out[4];
            load4(src + i * 4, in);
#pragma unroll
            for (int k = 0; k < 4; ++k) out[k] = convert<S, D>(in[k]);
            store4(dst + i * 4, out);
        }
        done = nv << 2;
    }
    for (int64_t i = done + first; i < lim; i += step) dst[i] = convert<S, D>(src[i]);
}

__device__ __forceinline__ uint4 pattern16(float x) {
    const uint32_t b = __float_as_uint(x);
    return make_uint4(b, b, b, b);
}
__device__ __forceinline__ uint4 pattern16(uint8_t x) {
    const uint32_t b = 0x01010101u * x;
    return make_uint4(b, b, b, b);
}

// dst[lim, total) = fill
template <typename D>
__device__ void fill_run(D *dst, int64_t lim, int64_t total, float fill, int64_t first, int64_t step) {
    constexpr int K = 16 / (int)sizeof(D);
    const D x = Elem<D>::from_f(fill);
    D *d = dst + lim;
    const int64_t n = total - lim;
    int64_t lead = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15) / sizeof(D));
    lead = lead < n ? lead : n;
    for (int64_t i = first; i < lead; i += step) d[i] = x;
    const int64_t nv = (n - lead) / K;
    const uint4 pattern = pattern16(x);
    uint4 *dv = reinterpret_cast<uint4 *>(d + lead);
    for (int64_t i = first; i < nv; i += step) dv[i] = pattern;
    for (int64_t i = lead + nv * K + first; i < n; i += step) d[i] = x;
}

template <typename S, typename D>
__device__ void harvest_field(const void *src, void *dst, int64_t e, int64_t row, int64_t total, int64_t lim, int unit,
                              float fill, int64_t first, int64_t step) {
    D *d = static_cast<D *>(dst) + row * total;
    copy_run<S, D>(static_cast<const S *>(src) + e * total, d, lim, unit, first, step);
    fill_run<D>(d, lim, total, fill, first, step);
}

constexpr int kPlayerFields = HRL_REPLAY_MAX_LEAVES + 3;   // obs leaves, policy, amask, value
struct PlayerField {
    const void *src;
    void *dst;
    int64_t width;   // elements per ply: P * w
    float fill;
    int32_t stype, dtype, unit;
};
struct PlayerHarvestArgs {
    HarvestArgs h;   // the rule's operands, the returns and the per-episode records; its own field table stays empty
    PlayerField f[kPlayerFields];
    int32_t nf;
    const int64_t *action;
    int64_t *r_action;
    const uint8_t *tmask, *omask;
    uint8_t *r_tmask, *r_omask;
};

__global__ __launch_bounds__(kHarvestThreads) void harvest_players_kernel(const PlayerHarvestArgs a) {
    __shared__ int s_r[kHarvestThreads / kWave], s_c[kHarvestThreads / kWave];
    const int64_t e = blockIdx.x;
    if (!a.h.done[e]) return;   // block-uniform
    int64_t row, L;
    if (!harvest_row(a.h, e, s_r, s_c, &row, &L)) return;
    if (blockIdx.y == kHarvestSplit) {
        harvest_tail(a.h, e, row, L);
        return;
    }
    const int64_t first = (int64_t)blockIdx.y * kHarvestThreads + threadIdx.x;
    const int64_t step = (int64_t)kHarvestSplit * kHarvestThreads;
    for (int k = 0; k < a.nf; ++k) {
        const PlayerField &f = a.f[k];
        const int64_t total = a.h.Tm * f.width, lim = L * f.width;
        const bool su8 = f.stype == HRL_REPLAY_U8, du8 = f.dtype == HRL_REPLAY_U8;
        if (su8 && du8)
            harvest_field<uint8_t, uint8_t>(f.src, f.dst, e, row, total, lim, f.unit, f.fill, first, step);
        else if (su8)
            harvest_field<uint8_t, float>(f.src, f.dst, e, row, total, lim, f.unit, f.fill, first, step);
        else if (du8)
            harvest_field<float, uint8_t>(f.src, f.dst, e, row, total, lim, f.unit, f.fill, first, step);
        else
            harvest_field<float, float>(f.src, f.dst, e, row, total, lim, f.unit, f.fill, first, step);
    }
    const int64_t TP = a.h.Tm * a.h.P, LP = L * a.h.P;
    for (int64_t i = first; i < TP; i += step) {
        const bool v = i < LP;
        a.r_action[row * TP + i] = v ? a.action[e * TP + i] : 0;
        a.r_tmask[row * TP + i] = v ? a.tmask[e * TP + i] : 0;
        a.r_omask[row * TP + i] = v ? a.omask[e * TP + i] : 0;
        a.h.r_reward[row * TP + i] = (a.h.reward && v) ? (float)a.h.reward[e * TP + i] : 0.0f;
    }
}

// ---- the movers' recurrent state advance (generation.py:38-41): dst[l] row e <- src[l] row e where mask[e] ----
constexpr int kMaxRowLeaves = 16;
struct RowLeaves {
    float *dst[kMaxRowLeaves];
    const float *src[kMaxRowLeaves];
    int64_t dst_stride[kMaxRowLeaves], src_stride[kMaxRowLeaves], F[kMaxRowLeaves];
};

__global__ __launch_bounds__(256) void masked_rows_kernel(const uint8_t *__restrict__ mask, RowLeaves L) {
    const int64_t e = blockIdx.x;
    const int l = blockIdx.y;
    if (!mask[e]) return;
    const float *s = L.src[l] + e * L.src_stride[l];
    float *d = L.dst[l] + e * L.dst_stride[l];
    for (int64_t f = threadIdx.x; f < L.F[l]; f += blockDim.x) d[f] = s[f];
}

}  // namespace

extern "C" {

int hrl_masked_rows_copy(int nleaves, float *const *dst, const int64_t *dst_stride, const float *const *src,
                         const int64_t *src_stride, const int64_t *F, const uint8_t *mask, int64_t E, void *stream) {
    if (nleaves < 1 || nleaves > kMaxRowLeaves || !dst || !dst_stride || !src || !src_stride || !F || !mask || E < 0 ||
        E > 0x7fffffff)
        return HRL_EINVAL;
    RowLeaves L{};
    for (int l = 0; l < nleaves; ++l) {
        if (!dst[l] || !src[l] || F[l] < 1 || dst_stride[l] < F[l] || src_stride[l] < F[l]) return HRL_EINVAL;
        L.dst[l] = dst[l];
        L.src[l] = src[l];
        L.dst_stride[l] = dst_stride[l];
        L.src_stride[l] = src_stride[l];
        L.F[l] = F[l];
    }
    if (E == 0) return HRL_OK;
    hipLaunchKernelGGL(masked_rows_kernel, dim3((unsigned)E, nleaves), dim3(256), 0, static_cast<hipStream_t>(stream),
                       mask, L);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}


int hrl_selfplay_sample_record(const float *logits, int64_t logit_stride, const uint8_t *legal, const float *U,
                               const int64_t *t, const float *value, const uint8_t *active, const int64_t *player,
                               const double *reward, int64_t E, int64_t A, int64_t Tm, int64_t P, int64_t *action,
                               float *policy_buf, float *amask_buf, int64_t *action_buf, float *value_buf,
                               int64_t *turn_buf, double *reward_buf, void *stream) {
    if (E == 0) return HRL_OK;
    if (!logits || !legal || !U || !t || !value || !active || !player || !action || !policy_buf || !amask_buf ||
        !action_buf || !value_buf || !turn_buf || E < 0 || A < 1 || A > (1 << 20) || Tm < 1 || P < 1 ||
        logit_stride < A || ((reward == nullptr) != (reward_buf == nullptr)))
        return HRL_EINVAL;
    const int blocks = (int)((E + kGamesPerBlock - 1) / kGamesPerBlock);
    hipLaunchKernelGGL(sample_record_kernel, dim3(blocks), dim3(kWave * kGamesPerBlock), 0,
                       static_cast<hipStream_t>(stream), logits, logit_stride, legal, U, t, value, active, player,
                       reward, E, (int)A, Tm, (int)P, action, policy_buf, amask_buf, action_buf, value_buf, turn_buf,
                       reward_buf);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

int hrl_selfplay_sample_record_stream(const float *logits, int64_t logit_stride, const uint8_t *legal, uint64_t seed,
                                      const int64_t *game, const int64_t *ply, const float *value,
                                      const uint8_t *active, const int64_t *player, const double *reward, int64_t E,
                                      int64_t A, int64_t Tm, int64_t P, int64_t *action, float *policy_buf,
                                      float *amask_buf, int64_t *action_buf, float *value_buf, int64_t *turn_buf,
                                      double *reward_buf, void *stream) {
    if (!logits || !legal || !game || !ply || !value || !active || !player || !action || !policy_buf || !amask_buf ||
        !action_buf || !value_buf || !turn_buf || E < 0 || A < 1 || A > (1 << 20) || Tm < 1 || P < 1 ||
        P > 0x7fffffff || logit_stride < A || ((reward == nullptr) != (reward_buf == nullptr)))
        return HRL_EINVAL;
    if (E == 0) return HRL_OK;
    const int blocks = (int)((E + kGamesPerBlock - 1) / kGamesPerBlock);
    hipLaunchKernelGGL(sample_record_stream_kernel, dim3(blocks), dim3(kWave * kGamesPerBlock), 0,
                       static_cast<hipStream_t>(stream), logits, logit_stride, legal, (uint32_t)seed,
                       (uint32_t)(seed >> 32), game, ply, value, active, player, reward, E, (int)A, Tm, (int)P, action,
                       policy_buf, amask_buf, action_buf, value_buf, turn_buf, reward_buf);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

int hrl_selfplay_harvest(const uint8_t *done, const hrl_selfplay_slots *slots, int64_t *ply, const float *outcome,
                         double gamma, const hrl_replay_ring *ring, int64_t *ring_game, int64_t *game,
                         uint8_t *pending, int64_t *state, void *stream) {
    if (!done || !slots || !ply || !outcome || !ring || !ring_game || !game || !pending || !state) return HRL_EINVAL;
    const int64_t E = slots->E, Tm = slots->Tm, P = slots->P, A = slots->A, N = ring->N;
    const int nl = slots->nleaves;
    if (E < 0 || E > 0x7fffffff || Tm < 1 || P < 1 || A < 1 || N < 1 || ring->Tm != Tm || ring->P != P ||
        ring->A != A || nl < 1 || nl > HRL_REPLAY_MAX_LEAVES || ring->nleaves != nl)
        return HRL_EINVAL;
    constexpr int64_t kMaxRecord = (int64_t)1 << 31;
    if (Tm >= kMaxRecord || A >= kMaxRecord || P >= kMaxRecord || Tm * A >= kMaxRecord || Tm * P >= kMaxRecord)
        return HRL_EINVAL;
    if (!slots->policy || !slots->amask || !slots->action || !slots->value || !slots->turn || !ring->policy ||
        !ring->amask || !ring->action || !ring->value || !ring->turn || !ring->reward || !ring->ret || !ring->length ||
        !ring->outcome)
        return HRL_EINVAL;
    HarvestArgs a{};
    auto field = [&a, Tm](const float *src, const void *dst, int64_t width, int type, float fill) {
        const int f = a.nf++;
        a.fsrc[f] = src;
        a.fdst[f] = const_cast<void *>(dst);
        a.fwidth[f] = width;
        a.ftype[f] = type;
        a.ffill[f] = fill;
        a.fvec[f] = (Tm * width) % 4 == 0 && (uintptr_t)src % 16 == 0 &&
                    (uintptr_t)dst % (type == HRL_REPLAY_U8 ? 4 : 16) == 0;
    };
    for (int l = 0; l < nl; ++l) {
        const int64_t w = slots->obs_width[l];
        const int type = ring->obs_type[l];
        if (w < 1 || w != ring->obs_width[l] || w >= kMaxRecord || Tm * w >= kMaxRecord || !slots->obs[l] ||
            !ring->obs[l] || (type != HRL_REPLAY_U8 && type != HRL_REPLAY_F32))
            return HRL_EINVAL;
        field(slots->obs[l], ring->obs[l], w, type, 0.0f);
    }
    field(slots->policy, ring->policy, A, HRL_REPLAY_F32, 0.0f);
    field(slots->amask, ring->amask, A, HRL_REPLAY_F32, 1e32f);
    field(slots->value, ring->value, 1, HRL_REPLAY_F32, 0.0f);
    if (E == 0) return HRL_OK;
    a.P = (int32_t)P;
    a.action = slots->action;
    a.turn = slots->turn;
    a.r_action = const_cast<int64_t *>(ring->action);
    a.r_turn = const_cast<int64_t *>(ring->turn);
    a.reward = slots->reward;
    a.r_reward = const_cast<float *>(ring->reward);
    a.r_ret = const_cast<float *>(ring->ret);
    a.r_outcome = const_cast<float *>(ring->outcome);
    a.r_length = const_cast<int64_t *>(ring->length);
    a.ring_game = ring_game;
    a.outcome = outcome;
    a.game = game;
    a.ply = ply;
    a.state = state;
    a.done = done;
    a.E = E;
    a.Tm = Tm;
    a.N = N;
    a.gamma = gamma;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(harvest_kernel, dim3((unsigned)((E + kSlotsPerBlock - 1) / kSlotsPerBlock), kHarvestSplit + 1),
                       dim3(kHarvestThreads), 0, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return HRL_ELAUNCH_BASE - (int)err;
    hipLaunchKernelGGL(harvest_advance_kernel, dim3(1), dim3(kHarvestThreads), 0, s, done, E, N, game, ply, pending,
                       state);
    err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

int hrl_selfplay_sample_record_players_stream(const float *logits, int64_t logit_stride, const float *value,
                                              const uint8_t *legal, int64_t legal_player_stride, const uint8_t *turns,
                                              const uint8_t *infer, const uint8_t *active, uint64_t seed,
                                              const int64_t *game, const int64_t *ply, int64_t E, int64_t P, int64_t A,
                                              int64_t Tm, int64_t *action, float *usel, float *policy_buf,
                                              float *amask_buf, int64_t *action_buf, float *value_buf,
                                              uint8_t *tmask_buf, uint8_t *omask_buf, void *stream) {
    if (!logits || !value || !legal || !turns || !infer || !active || !game || !ply || !action || !usel ||
        !policy_buf || !amask_buf || !action_buf || !value_buf || !tmask_buf || !omask_buf || E < 0 || P < 1 ||
        A < 1 || A > (1 << 20) || Tm < 1 || logit_stride < A || (legal_player_stride != 0 && legal_player_stride != A))
        return HRL_EINVAL;
    constexpr int64_t kLimit = 0x40000000;
    if (P >= kLimit || E >= kLimit || P * E >= kLimit || P * ((A + 3) / 4) >= kLimit) return HRL_EINVAL;
    if (E == 0) return HRL_OK;
    const int blocks = (int)((E * P + kGamesPerBlock - 1) / kGamesPerBlock);
    hipLaunchKernelGGL(sample_record_players_stream_kernel, dim3(blocks), dim3(kWave * kGamesPerBlock), 0,
                       static_cast<hipStream_t>(stream), logits, logit_stride, value, legal, legal_player_stride, turns,
                       infer, active, (uint32_t)seed, (uint32_t)(seed >> 32), game, ply, E, (int)P, (int)A, Tm, action,
                       usel, policy_buf, amask_buf, action_buf, value_buf, tmask_buf, omask_buf);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

int hrl_selfplay_harvest_players(const uint8_t *done, const hrl_selfplay_player_slots *slots, int64_t *ply,
                                 const float *outcome, double gamma, const hrl_replay_ring *ring, int64_t *ring_game,
                                 int64_t *game, uint8_t *pending, int64_t *state, void *stream) {
    if (!done || !slots || !ply || !outcome || !ring || !ring_game || !game || !pending || !state) return HRL_EINVAL;
    const int64_t E = slots->E, Tm = slots->Tm, P = slots->P, A = slots->A, N = ring->N;
    const int nl = slots->nleaves;
    if (E < 0 || E > 0x7fffffff || Tm < 1 || P < 1 || A < 1 || N < 1 || ring->Tm != Tm || ring->P != P ||
        ring->A != A || nl < 1 || nl > HRL_REPLAY_MAX_LEAVES || ring->nleaves != nl)
        return HRL_EINVAL;
    constexpr int64_t kMaxRecord = (int64_t)1 << 31;
    if (Tm >= kMaxRecord || A >= kMaxRecord || P >= kMaxRecord || Tm * P >= kMaxRecord || P * A >= kMaxRecord ||
        Tm * P * A >= kMaxRecord)
        return HRL_EINVAL;
    if (!slots->policy || !slots->amask || !slots->action || !slots->value || !slots->tmask || !slots->omask ||
        !ring->policy || !ring->amask || !ring->action || !ring->value || !ring->tmask || !ring->omask ||
        !ring->reward || !ring->ret || !ring->length || !ring->outcome)
        return HRL_EINVAL;
    PlayerHarvestArgs a{};
    // the copy's unit: the most source elements per lane whose loads and stores are aligned in every slot and row
    auto field = [&a, Tm](const void *src, const void *dst, int64_t width, int stype, int dtype, float fill) {
        PlayerField &f = a.f[a.nf++];
        f.src = src;
        f.dst = const_cast<void *>(dst);
        f.width = width;
        f.stype = stype;
        f.dtype = dtype;
        f.fill = fill;
        const int64_t total = Tm * width;
        const uintptr_t sb = (uintptr_t)src, db = (uintptr_t)dst;
        const int ssize = stype == HRL_REPLAY_U8 ? 1 : 4, dsize = dtype == HRL_REPLAY_U8 ? 1 : 4;
        f.unit = 1;
        for (int unit : {4, 16}) {
            if (unit * ssize > 16) continue;   // one load of at most 16 bytes per lane
            const int store = unit * dsize < 16 ? unit * dsize : 16;
            if (total % unit == 0 && sb % (unit * ssize) == 0 && db % store == 0) f.unit = unit;
        }
    };
    for (int l = 0; l < nl; ++l) {
        const int64_t w = slots->obs_width[l];
        const int stype = slots->obs_type[l], dtype = ring->obs_type[l];
        if (w < 1 || w != ring->obs_width[l] || w >= kMaxRecord || P * w >= kMaxRecord || Tm * P * w >= kMaxRecord ||
            !slots->obs[l] || !ring->obs[l] || (stype != HRL_REPLAY_U8 && stype != HRL_REPLAY_F32) ||
            (dtype != HRL_REPLAY_U8 && dtype != HRL_REPLAY_F32))
            return HRL_EINVAL;
        field(slots->obs[l], ring->obs[l], P * w, stype, dtype, 0.0f);
    }
    field(slots->policy, ring->policy, P * A, HRL_REPLAY_F32, HRL_REPLAY_F32, 0.0f);
    field(slots->amask, ring->amask, P * A, HRL_REPLAY_F32, HRL_REPLAY_F32, 1e32f);
    field(slots->value, ring->value, P, HRL_REPLAY_F32, HRL_REPLAY_F32, 0.0f);
    if (E == 0) return HRL_OK;
    a.h.P = (int32_t)P;
    a.h.reward = slots->reward;
    a.h.r_reward = const_cast<float *>(ring->reward);
    a.h.r_ret = const_cast<float *>(ring->ret);
    a.h.r_outcome = const_cast<float *>(ring->outcome);
    a.h.r_length = const_cast<int64_t *>(ring->length);
    a.h.ring_game = ring_game;
    a.h.outcome = outcome;
    a.h.game = game;
    a.h.ply = ply;
    a.h.state = state;
    a.h.done = done;
    a.h.E = E;
    a.h.Tm = Tm;
    a.h.N = N;
    a.h.gamma = gamma;
    a.action = slots->action;
    a.r_action = const_cast<int64_t *>(ring->action);
    a.tmask = slots->tmask;
    a.omask = slots->omask;
    a.r_tmask = const_cast<uint8_t *>(ring->tmask);
    a.r_omask = const_cast<uint8_t *>(ring->omask);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(harvest_players_kernel, dim3((unsigned)E, kHarvestSplit + 1), dim3(kHarvestThreads), 0, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return HRL_ELAUNCH_BASE - (int)err;
    hipLaunchKernelGGL(harvest_advance_kernel, dim3(1), dim3(kHarvestThreads), 0, s, done, E, N, game, ply, pending,
                       state);
    err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

}  // extern "C"
