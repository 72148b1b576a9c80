// hrl_eval.hip — the device evaluator's ply (handyrl/evaluation.py:64-87, agent.py:13-19, 55-110): the model on one
// seat of every game, a uniform random agent on the others, E slots that restart in place until G games are played.
//
// evaluation.DeviceEvaluator runs, per global step, the env's observation and the net's forward, then
//   match_act_kernel     one wave per slot, lanes over the A labels: the model seat's argmax (or Gumbel-max at a
//                        temperature) of the masked logits, the random seat's k-th legal label (eval_pick); in a match
//                        against a second net the other seats play that net's move at its own temperature, and the
//                        first `opening` plies of a game are eval_pick on every seat.  It is the ONE decision kernel
//                        (one source body, two instantiations: with and without the second net's pointer pair):
//                        hrl_eval_act is hrl_match_act without an opponent and without opening plies;
//   the env's step;
//   eval_finish_kernel   one workgroup: ply += 1, the finished games' outcome and length stored BY GAME NUMBER, the
//                        slots restarted with the next game numbers in slot order or retired, the state advanced.
// Nothing is recorded but the result, so the ply costs two launches besides the env's and the net's.  The rules are
// public (include/hrl_env.h); evaluation.py holds the torch formulation the kernels equal bit for bit.
// masked_rows_fill_kernel zeroes a restarting slot's recurrent-state rows (the twin of hrl_masked_rows_copy).
// evaluation.PlayerEvaluator plays a simultaneous-move env (Hungry Geese) the same way with
//   players_act_kernel   one wave per (slot, player): every player decides in the one launch -- the home net on
//                        seat(g), a second net or eval_pick_player on the others -- from relative-seat-major logits;
// the finish is eval_finish_kernel unchanged.  With a rule pointer (hrl_players_act_rule) the seats without a net play a
// rule-based agent's label (Hungry Geese: hrl_geese_greedy) where it is legal, else eval_pick_player as before.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hrl_env.h"
#include "../../include/hrl_targets.h"
#include "hrl_pick.h"

namespace {

constexpr int kSlotsPerBlock = 4;

struct EvalTrace {   // all four or none (action NULL: no trace)
    int64_t *action, *picked;
    float *policy;
    uint8_t *model_ply;
};

// A net's move for one slot (the whole wave): p = logits - (legal ? 0 : 1e32) goes to pol when pol is given; the
// argmax of p, or at inv_t > 0 the Gumbel-max over p * inv_t, under better().  Label j draws its uniform from the
// Philox call with last counter word w3 + j / 4 (w3 = 0: the mover rule; the players' rule has its own base).
__device__ __forceinline__ int net_pick(const float *__restrict__ lg, const uint8_t *__restrict__ lm, float *pol,
                                        int A, float inv_t, uint32_t k0, uint32_t k1, uint32_t g0, uint32_t g1,
                                        uint32_t tw, uint32_t w3, int lane) {
    float best = 0.0f;
    int ib = A;   // no label yet
    for (int j = lane; j < A; j += kWave) {
        const float m = lm[j] ? 0.0f : 1e32f;
        const float p = lg[j] - m;
        float v = p;
        if (inv_t > 0.0f) {   // Gumbel-max over p / temperature: the fp32 operations of the streaming tail
            const uint32_t x = philox_word(k0, k1, g0, g1, tw, w3 + (uint32_t)(j >> 2), j & 3);
            const float u = ((float)(x >> 9) + 0.5f) * 0x1p-23f;
            v = p * inv_t - logf(-logf(u));
        }
        if (ib == A || better(v, j, best, ib)) {
            best = v;
            ib = j;
        }
        if (pol) pol[j] = p;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(ib, off);
        if (oi != A && (ib == A || better(ob, oi, best, ib))) {
            best = ob;
            ib = oi;
        }
    }
    return ib;
}

// eval_pick for one slot (the whole wave): n legal labels by ballot and popcount, k = (w * n) >> 23, the k-th by
// prefix count; 0 for a row without a legal label.  (c3, word) name the Philox word: (0xffffffff, 0) is eval_pick,
// (0xffffffff - (player >> 2), player & 3) eval_pick_player.
__device__ __forceinline__ int random_pick(const uint8_t *__restrict__ lm, int A, uint32_t k0, uint32_t k1,
                                           uint32_t g0, uint32_t g1, uint32_t tw, uint32_t c3, int word, int lane) {
    int64_t n = 0;
    for (int j0 = 0; j0 < A; j0 += kWave) {
        const int j = j0 + lane;
        n += __popcll(__ballot(j < A && lm[j] != 0));
    }
    const uint64_t w = philox_word(k0, k1, g0, g1, tw, c3, word) >> 9;
    int64_t k = (int64_t)((w * (uint64_t)n) >> 23);   // < n
    for (int j0 = 0; j0 < A && n > 0; j0 += kWave) {
        const int j = j0 + lane;
        const bool ok = j < A && lm[j] != 0;
        const uint64_t b = __ballot(ok);
        const int c = __popcll(b);
        if (k < c) {
            const bool mine = ok && __popcll(b & ((1ull << lane) - 1ull)) == (int)k;
            return j0 + __ffsll((unsigned long long)__ballot(mine)) - 1;
        }
        k -= c;
    }
    return 0;
}

// The slot's last stores (lane 0): the move played, forced or picked, and the trace's three scalar records.
__device__ __forceinline__ void store_move(const int64_t *__restrict__ forced, int64_t s, int pick, bool model,
                                           int64_t *__restrict__ action, const EvalTrace &tr) {
    const int64_t f = forced ? forced[s] : -1;
    const int64_t a = f >= 0 ? f : pick;
    *action = a;
    if (tr.action) {
        tr.action[s] = a;
        tr.picked[s] = pick;
        tr.model_ply[s] = model ? 1 : 0;
    }
}

// The ply's decision, against random agents (opp NULL, opening 0), in a match and in a league.  Per slot: the mover's
// net is home where seat == mover, else opp (or none: opp NULL); its masked logits go to the trace whenever there is
// one; the move is eval_pick at an opening ply or without a net, else that net's argmax / Gumbel-max at its own
// temperature.  kOpp false is the form without a second net (hrl_eval_act): the opp pointer pair is compiled out.
template <bool kOpp>
__global__ __launch_bounds__(kWave *kSlotsPerBlock) void match_act_kernel(
    const float *__restrict__ home, int64_t hstride, const float *__restrict__ opp, int64_t ostride,
    const uint8_t *__restrict__ legal, uint32_t k0, uint32_t k1, float inv_t_home, float inv_t_opp, int64_t opening,
    const int64_t *__restrict__ game, const int64_t *__restrict__ ply, const uint8_t *__restrict__ active,
    const int64_t *__restrict__ seat, int64_t mover, const int64_t *__restrict__ forced, int64_t E, int A, int64_t Tm,
    int64_t G, int64_t *__restrict__ action, EvalTrace tr) {
    const int lane = threadIdx.x % kWave;
    const int64_t e = (int64_t)blockIdx.x * kSlotsPerBlock + threadIdx.x / kWave;
    if (e >= E) return;
    const int64_t t = ply[e], g = game[e];
    if (!active[e] || t < 0 || t >= Tm || g < 0 || g >= G) {   // wave-uniform
        if (lane == 0) action[e] = 0;
        return;
    }
    const uint32_t g0 = (uint32_t)(uint64_t)g, g1 = (uint32_t)((uint64_t)g >> 32), tw = (uint32_t)t;
    const uint8_t *lm = legal + e * A;
    const bool model = seat[e] == mover;   // wave-uniform, as is everything below
    const float *lg = model ? home + e * hstride : kOpp && opp ? opp + e * ostride : nullptr;
    int pick = 0;
    if (lg) {
        float *pol = tr.action ? tr.policy + (g * Tm + t) * A : nullptr;
        if (t >= opening || pol)
            pick = net_pick(lg, lm, pol, A, model ? inv_t_home : inv_t_opp, k0, k1, g0, g1, tw, 0u, lane);
    }
    if (!lg || t < opening) pick = random_pick(lm, A, k0, k1, g0, g1, tw, 0xffffffffu, 0, lane);
    if (lane == 0) store_move(forced, g * Tm + t, pick, model, action + e, tr);
}

// ---- simultaneous-move envs (evaluation.PlayerEvaluator): every player of every slot decides in the one launch ----
constexpr uint32_t kPlayerW3 = 0x40000000u, kSelectW3 = 0x80000000u;   // include/hrl_env.h: the counter's last word

struct PlayersTrace {   // all four or none (action NULL: no trace)
    int64_t *action, *picked;
    float *policy;
    uint8_t *alive;
};

// One wave per (slot, player), lanes over the A labels.  Player p of slot e sits k = (p - seat[e]) mod P seats after the
// home net: k = 0 reads row e of home, k >= 1 row (k - 1) * E + e of opp (or has no net: opp NULL).  A player without
// a net plays rule[e * P + p] where a rule is given and that label is legal (hrl_players_act_rule).  Everything that
// branches is wave-uniform.
__global__ __launch_bounds__(kWave *kSlotsPerBlock) void players_act_kernel(
    const float *__restrict__ home, int64_t hstride, const float *__restrict__ opp, int64_t ostride,
    const uint8_t *__restrict__ legal, int64_t lpstride, const uint8_t *__restrict__ turns, uint32_t k0, uint32_t k1,
    float inv_t_home, float inv_t_opp, int64_t opening, const int64_t *__restrict__ game,
    const int64_t *__restrict__ ply, const uint8_t *__restrict__ active, const int64_t *__restrict__ seat,
    const int64_t *__restrict__ forced, const int64_t *__restrict__ rule, int64_t E, int P, int A, int64_t Tm,
    int64_t G, int64_t *__restrict__ action, float *__restrict__ usel, PlayersTrace tr) {
    const int lane = threadIdx.x % kWave;
    const int64_t w = (int64_t)blockIdx.x * kSlotsPerBlock + threadIdx.x / kWave;   // the pair e * P + p
    if (w >= E * P) return;
    const int64_t e = w / P;
    const int p = (int)(w - e * P);
    const int64_t t = ply[e], g = game[e];
    const uint32_t g0 = (uint32_t)(uint64_t)g, g1 = (uint32_t)((uint64_t)g >> 32), tw = (uint32_t)(uint64_t)t;
    if (p == 0 && lane == 0)
        usel[e] = ((float)(philox_word(k0, k1, g0, g1, tw, kSelectW3, 0) >> 9) + 0.5f) * 0x1p-23f;
    if (!active[e] || t < 0 || t >= Tm || g < 0 || g >= G) {
        if (lane == 0) action[w] = 0;
        return;
    }
    const int64_t s = (g * Tm + t) * P + p;
    if (!turns[w]) {   // the player does not move: no decision, the trace says so
        if (lane == 0) {
            action[w] = 0;
            if (tr.action) {
                tr.action[s] = -1;
                tr.picked[s] = -1;
                tr.alive[s] = 0;
            }
        }
        return;
    }
    const int k = (int)((((int64_t)p - seat[e]) % P + P) % P);
    const uint8_t *lm = legal + e * (lpstride ? (int64_t)P * A : (int64_t)A) + p * lpstride;
    const float *lg = k == 0 ? home + e * hstride : opp ? opp + ((int64_t)(k - 1) * E + e) * ostride : nullptr;
    int pick = 0;
    if (lg) {
        float *pol = tr.action ? tr.policy + s * A : nullptr;
        if (t >= opening || pol)
            pick = net_pick(lg, lm, pol, A, k == 0 ? inv_t_home : inv_t_opp, k0, k1, g0, g1, tw,
                            kPlayerW3 + (uint32_t)p * (uint32_t)((A + 3) >> 2), lane);
    }
    if (!lg || t < opening)
        pick = random_pick(lm, A, k0, k1, g0, g1, tw, 0xffffffffu - (uint32_t)(p >> 2), p & 3, lane);
    if (rule && !lg && t >= opening) {   // a rule-based agent on a seat without a net: its label where legal
        const int64_t r = rule[w];
        if (r >= 0 && r < A && lm[r]) pick = (int)r;
    }
    if (lane == 0) {
        const int64_t f = forced ? forced[s] : -1;
        const int64_t a = f >= 0 ? f : pick;
        action[w] = a;
        if (tr.action) {
            tr.action[s] = a;
            tr.picked[s] = pick;
            tr.alive[s] = 1;
        }
    }
}

// One workgroup; thread k owns the slots [k * chunk, (k + 1) * chunk).  Every store is a plain vector store.
constexpr int kFinishThreads = 256;
__global__ __launch_bounds__(kFinishThreads) void eval_finish_kernel(
    const uint8_t *__restrict__ terminal, const float *__restrict__ outcome, int64_t E, int64_t Tm, int P, int64_t G,
    uint8_t *__restrict__ active, int64_t *__restrict__ ply, int64_t *__restrict__ game, int64_t *__restrict__ seat,
    uint8_t *__restrict__ pending, int64_t *__restrict__ state, float *__restrict__ outcome_out,
    int64_t *__restrict__ length_out) {
    __shared__ int s_wave[kFinishThreads / kWave];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int64_t chunk = (E + kFinishThreads - 1) / kFinishThreads;
    const int64_t lo = threadIdx.x * chunk < E ? threadIdx.x * chunk : E, hi = lo + chunk < E ? lo + chunk : E;
    int cnt = 0;
    for (int64_t i = lo; i < hi; ++i) {
        if (!active[i]) continue;
        const int64_t t = ply[i] + 1;
        ply[i] = t;
        if (terminal[i] || t >= Tm) {
            const int64_t g = game[i];
            if (g >= 0 && g < G) {
                for (int q = 0; q < P; ++q) outcome_out[g * P + q] = outcome[i * P + q];
                length_out[g] = t;
            }
            ++cnt;
        }
    }
    int incl = cnt;   // inclusive scan over the wave's lanes, then over the waves
    for (int off = 1; off < kWave; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == kWave - 1) s_wave[wave] = incl;
    const int64_t finished = state[0], next = state[1];
    __syncthreads();
    int64_t pre = incl - cnt, total = 0;
    for (int w = 0; w < kFinishThreads / kWave; ++w) {
        pre += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
    }
    for (int64_t i = lo; i < hi; ++i) {
        if (!active[i] || !(terminal[i] || ply[i] >= Tm)) continue;   // ply[i] is this thread's own store
        const int64_t g = next + pre++;
        const bool again = g < G;
        active[i] = 0;
        ply[i] = 0;
        game[i] = again ? g : G;
        seat[i] = again ? g % P : 0;
        pending[i] = again ? 1 : 0;
    }
    if (threadIdx.x == 0 && total > 0) {
        state[0] = finished + total;
        state[1] = next + total < G ? next + total : G;
    }
}

constexpr int kMaxRowLeaves = 16;
struct FillLeaves {
    float *dst[kMaxRowLeaves];
    int64_t dst_stride[kMaxRowLeaves], F[kMaxRowLeaves];
};

__global__ __launch_bounds__(256) void masked_rows_fill_kernel(const uint8_t *__restrict__ mask, FillLeaves L) {
    const int64_t e = blockIdx.x;
    const int l = blockIdx.y;
    if (!mask[e]) return;
    float *d = L.dst[l] + e * L.dst_stride[l];
    for (int64_t f = threadIdx.x; f < L.F[l]; f += blockDim.x) d[f] = 0.0f;
}

}  // namespace

extern "C" {

int hrl_eval_act(const float *logits, int64_t logit_stride, const uint8_t *legal, uint64_t seed, double temperature,
                 const int64_t *game, const int64_t *ply, const uint8_t *active, const int64_t *seat, int64_t mover,
                 const int64_t *forced, int64_t E, int64_t A, int64_t Tm, int64_t P, int64_t G, int64_t *action,
                 int64_t *trace_action, int64_t *trace_picked, float *trace_policy, uint8_t *trace_model_ply,
                 void *stream) {
    // no opponent, no opening plies: the same kernel, and for these arguments the same argument checks
    return hrl_match_act(logits, logit_stride, nullptr, 0, legal, seed, temperature, 0.0, 0, game, ply, active, seat,
                         mover, forced, E, A, Tm, P, G, action, trace_action, trace_picked, trace_policy,
                         trace_model_ply, stream);
}

int hrl_match_act(const float *logits_home, int64_t stride_home, const float *logits_opp, int64_t stride_opp,
                  const uint8_t *legal, uint64_t seed, double temperature_home, double temperature_opp,
                  int64_t opening, const int64_t *game, const int64_t *ply, const uint8_t *active,
                  const int64_t *seat, int64_t mover, const int64_t *forced, int64_t E, int64_t A, int64_t Tm,
                  int64_t P, int64_t G, int64_t *action, int64_t *trace_action, int64_t *trace_picked,
                  float *trace_policy, uint8_t *trace_model_ply, void *stream) {
    const int ntrace = (trace_action != nullptr) + (trace_picked != nullptr) + (trace_policy != nullptr) +
                       (trace_model_ply != nullptr);
    if (!logits_home || !legal || !game || !ply || !active || !seat || !action || E < 0 || E > 0x7fffffff || A < 1 ||
        A > (1 << 20) || Tm < 1 || P < 1 || G < 0 || stride_home < A || (logits_opp && stride_opp < A) || mover < 0 ||
        mover >= P || !(temperature_home >= 0.0) || !(temperature_opp >= 0.0) || opening < 0 ||
        (ntrace != 0 && ntrace != 4))
        return HRL_EINVAL;
    if (E == 0) return HRL_OK;
    const float inv_home = temperature_home > 0.0 ? (float)(1.0 / temperature_home) : 0.0f;
    const float inv_opp = temperature_opp > 0.0 ? (float)(1.0 / temperature_opp) : 0.0f;
    EvalTrace tr{trace_action, trace_picked, trace_policy, trace_model_ply};
    const int blocks = (int)((E + kSlotsPerBlock - 1) / kSlotsPerBlock);
    const auto kernel = logits_opp ? match_act_kernel<true> : match_act_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kWave * kSlotsPerBlock), 0,
                       static_cast<hipStream_t>(stream), logits_home, stride_home, logits_opp, stride_opp, legal,
                       (uint32_t)seed, (uint32_t)(seed >> 32), inv_home, inv_opp, opening, game, ply, active, seat,
                       mover, forced, E, (int)A, Tm, G, action, tr);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

int hrl_players_act(const float *logits_home, int64_t stride_home, const float *logits_opp, int64_t stride_opp,
                    const uint8_t *legal, int64_t legal_player_stride, const uint8_t *turns, uint64_t seed,
                    double temperature_home, double temperature_opp, int64_t opening, const int64_t *game,
                    const int64_t *ply, const uint8_t *active, const int64_t *seat, const int64_t *forced, int64_t E,
                    int64_t P, int64_t A, int64_t Tm, int64_t G, int64_t *action, float *usel,
                    int64_t *trace_action, int64_t *trace_picked, float *trace_policy, uint8_t *trace_alive,
                    void *stream) {
    // no rule-based agent: the same kernel, and for these arguments the same argument checks
    return hrl_players_act_rule(logits_home, stride_home, logits_opp, stride_opp, legal, legal_player_stride, turns,
                                seed, temperature_home, temperature_opp, opening, game, ply, active, seat, forced,
                                nullptr, E, P, A, Tm, G, action, usel, trace_action, trace_picked, trace_policy,
                                trace_alive, stream);
}

int hrl_players_act_rule(const float *logits_home, int64_t stride_home, const float *logits_opp, int64_t stride_opp,
                         const uint8_t *legal, int64_t legal_player_stride, const uint8_t *turns, uint64_t seed,
                         double temperature_home, double temperature_opp, int64_t opening, const int64_t *game,
                         const int64_t *ply, const uint8_t *active, const int64_t *seat, const int64_t *forced,
                         const int64_t *rule, int64_t E, int64_t P, int64_t A, int64_t Tm, int64_t G, int64_t *action,
                         float *usel, int64_t *trace_action, int64_t *trace_picked, float *trace_policy,
                         uint8_t *trace_alive, void *stream) {
    const int ntrace = (trace_action != nullptr) + (trace_picked != nullptr) + (trace_policy != nullptr) +
                       (trace_alive != nullptr);
    if (!logits_home || !legal || !turns || !game || !ply || !active || !seat || !action || !usel || E < 0 || P < 1 ||
        A < 1 || A > (1 << 20) || Tm < 1 || G < 0 || stride_home < A || (logits_opp && stride_opp < A) ||
        (legal_player_stride != 0 && legal_player_stride != A) || !(temperature_home >= 0.0) ||
        !(temperature_opp >= 0.0) || opening < 0 || (ntrace != 0 && ntrace != 4) || (rule && logits_opp))
        return HRL_EINVAL;
    constexpr int64_t kLimit = 0x40000000;
    if (P >= kLimit || E >= kLimit || P * E >= kLimit || P * ((A + 3) / 4) >= kLimit) return HRL_EINVAL;
    if (E == 0) return HRL_OK;
    const float inv_home = temperature_home > 0.0 ? (float)(1.0 / temperature_home) : 0.0f;
    const float inv_opp = temperature_opp > 0.0 ? (float)(1.0 / temperature_opp) : 0.0f;
    PlayersTrace tr{trace_action, trace_picked, trace_policy, trace_alive};
    const int blocks = (int)((E * P + kSlotsPerBlock - 1) / kSlotsPerBlock);
    hipLaunchKernelGGL(players_act_kernel, dim3(blocks), dim3(kWave * kSlotsPerBlock), 0,
                       static_cast<hipStream_t>(stream), logits_home, stride_home, logits_opp, stride_opp, legal,
                       legal_player_stride, turns, (uint32_t)seed, (uint32_t)(seed >> 32), inv_home, inv_opp, opening,
                       game, ply, active, seat, forced, rule, E, (int)P, (int)A, Tm, G, action, usel, tr);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

int hrl_eval_finish(const uint8_t *terminal, const float *outcome, int64_t E, int64_t Tm, int64_t P, int64_t G,
                    uint8_t *active, int64_t *ply, int64_t *game, int64_t *seat, uint8_t *pending, int64_t *state,
                    float *outcome_out, int64_t *length_out, void *stream) {
    if (!terminal || !outcome || !active || !ply || !game || !seat || !pending || !state || !outcome_out ||
        !length_out || E < 0 || E > 0x7fffffff || Tm < 1 || P < 1 || P > 0x7fffffff || G < 0)
        return HRL_EINVAL;
    if (E == 0) return HRL_OK;
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(kFinishThreads), 0, static_cast<hipStream_t>(stream),
                       terminal, outcome, E, Tm, (int)P, G, active, ply, game, seat, pending, state, outcome_out,
                       length_out);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

int hrl_masked_rows_fill(int nleaves, float *const *dst, const int64_t *dst_stride, const int64_t *F,
                         const uint8_t *mask, int64_t E, void *stream) {
    if (nleaves < 1 || nleaves > kMaxRowLeaves || !dst || !dst_stride || !F || !mask || E < 0 || E > 0x7fffffff)
        return HRL_EINVAL;
    FillLeaves L{};
    for (int l = 0; l < nleaves; ++l) {
        if (!dst[l] || F[l] < 1 || dst_stride[l] < F[l]) return HRL_EINVAL;
        L.dst[l] = dst[l];
        L.dst_stride[l] = dst_stride[l];
        L.F[l] = F[l];
    }
    if (E == 0) return HRL_OK;
    hipLaunchKernelGGL(masked_rows_fill_kernel, dim3((unsigned)E, nleaves), dim3(256), 0,
                       static_cast<hipStream_t>(stream), mask, L);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

}  // extern "C"
