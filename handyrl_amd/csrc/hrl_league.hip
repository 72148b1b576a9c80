// hrl_league.hip — the league evaluator's ply (evaluation.LeagueEvaluator): K nets, Q pairings of two of them, every
// pairing a block of S slots that plays G games by the rules of the match evaluator (hrl_eval.hip, include/hrl_env.h).
//
// Per global step the evaluator runs the env's observation over the E = Q * S slots, then
//   rows_permute_kernel    the observation leaves from slot order into net-major order (every net's rows adjacent);
//   each net's forward over its own rows only;
//   rows_permute_kernel    the nets' logits back into slot order;
//   match_act_kernel       (hrl_eval.hip: the one decision kernel of every evaluator) both logit pointers at the
//                          slot-ordered buffer;
//   the env's step;
//   league_finish_kernel   one workgroup: ply += 1, a finished game's outcome and length stored at [block][game], the
//                          slot restarted with game + S or retired.  A slot's seat never changes (S is even), so no
//                          slot order is needed among the done slots: the only reduction is their count.
// evaluation.py holds the torch formulation (league_finish_torch, rows_permute_torch) the kernels equal bit for bit.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrl_env.h"
#include "../../include/hrl_targets.h"
#include "hrl_pick.h"

namespace {

// One workgroup; thread k owns the slots k, k + 256, ... (coalesced).  Every store is a plain vector store.
constexpr int kFinishThreads = 256;
__global__ __launch_bounds__(kFinishThreads) void league_finish_kernel(
    const uint8_t *__restrict__ terminal, const float *__restrict__ outcome, int64_t E, int64_t S, int64_t Tm, int P,
    int64_t G, uint8_t *__restrict__ active, int64_t *__restrict__ ply, int64_t *__restrict__ game,
    uint8_t *__restrict__ pending, int64_t *__restrict__ state, float *__restrict__ outcome_out,
    int64_t *__restrict__ length_out) {
    __shared__ int s_wave[kFinishThreads / kWave];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    int cnt = 0;
    for (int64_t i = threadIdx.x; i < E; i += kFinishThreads) {
        if (!active[i]) continue;
        const int64_t t = ply[i] + 1;
        if (!(terminal[i] || t >= Tm)) {
            ply[i] = t;
            continue;
        }
        const int64_t g = game[i];
        if (g >= 0 && g < G) {
            const int64_t row = (i / S) * G + g;
            for (int q = 0; q < P; ++q) outcome_out[row * P + q] = outcome[i * P + q];
            length_out[row] = t;
        }
        const int64_t n = g + S;
        const bool again = n < G;
        active[i] = 0;
        ply[i] = 0;
        game[i] = again ? n : G;
        pending[i] = again ? 1 : 0;
        ++cnt;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) s_wave[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t total = 0;
        for (int w = 0; w < kFinishThreads / kWave; ++w) total += s_wave[w];
        if (total > 0) state[0] += total;
    }
}

constexpr int kMaxRowLeaves = 16;
struct PermuteLeaves {
    float *dst[kMaxRowLeaves];
    const float *src[kMaxRowLeaves];
    int64_t dst_stride[kMaxRowLeaves], src_stride[kMaxRowLeaves], F[kMaxRowLeaves];
    uint8_t vec[kMaxRowLeaves];   // rows of whole, 16-byte aligned float4s on both sides
};

// Workgroup (r, l): row dst_index[r] of leaf l's dst = row src_index[r] of its src (a NULL index: r itself).
__global__ __launch_bounds__(256) void rows_permute_kernel(const int64_t *__restrict__ src_index,
                                                           const int64_t *__restrict__ dst_index, PermuteLeaves L) {
    const int64_t r = blockIdx.x;
    const int l = blockIdx.y;
    const int64_t rs = src_index ? src_index[r] : r, rd = dst_index ? dst_index[r] : r;
    const float *s = L.src[l] + rs * L.src_stride[l];
    float *d = L.dst[l] + rd * L.dst_stride[l];
    const int64_t F = L.F[l];
    if (L.vec[l]) {
        const float4 *s4 = reinterpret_cast<const float4 *>(s);
        float4 *d4 = reinterpret_cast<float4 *>(d);
        for (int64_t f = threadIdx.x; f < F / 4; f += blockDim.x) d4[f] = s4[f];
    } else {
        for (int64_t f = threadIdx.x; f < F; f += blockDim.x) d[f] = s[f];
    }
}

}  // namespace

extern "C" {

int hrl_league_finish(const uint8_t *terminal, const float *outcome, int64_t E, int64_t S, int64_t Tm, int64_t P,
                      int64_t G, uint8_t *active, int64_t *ply, int64_t *game, uint8_t *pending, int64_t *state,
                      float *outcome_out, int64_t *length_out, void *stream) {
    if (!terminal || !outcome || !active || !ply || !game || !pending || !state || !outcome_out || !length_out ||
        E < 0 || E > 0x7fffffff || S < 2 || S % 2 != 0 || E % S != 0 || Tm < 1 || P < 1 || P > 0x7fffffff || G < 0)
        return HRL_EINVAL;
    if (E == 0) return HRL_OK;
    hipLaunchKernelGGL(league_finish_kernel, dim3(1), dim3(kFinishThreads), 0, static_cast<hipStream_t>(stream),
                       terminal, outcome, E, S, Tm, (int)P, G, active, ply, game, pending, state, outcome_out,
                       length_out);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

int hrl_rows_permute(int nleaves, float *const *dst, const int64_t *dst_stride, const float *const *src,
                     const int64_t *src_stride, const int64_t *F, const int64_t *src_index, const int64_t *dst_index,
                     int64_t n, void *stream) {
    if (nleaves < 1 || nleaves > kMaxRowLeaves || !dst || !dst_stride || !src || !src_stride || !F || n < 0 ||
        n > 0x7fffffff)
        return HRL_EINVAL;
    PermuteLeaves L{};
    int64_t widest = 0;
    for (int l = 0; l < nleaves; ++l) {
        if (!dst[l] || !src[l] || F[l] < 1 || dst_stride[l] < F[l] || src_stride[l] < F[l]) return HRL_EINVAL;
        L.dst[l] = dst[l];
        L.src[l] = src[l];
        L.dst_stride[l] = dst_stride[l];
        L.src_stride[l] = src_stride[l];
        L.F[l] = F[l];
        L.vec[l] = F[l] % 4 == 0 && dst_stride[l] % 4 == 0 && src_stride[l] % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(dst[l]) % 16 == 0 && reinterpret_cast<uintptr_t>(src[l]) % 16 == 0;
        const int64_t items = L.vec[l] ? F[l] / 4 : F[l];
        widest = items > widest ? items : widest;
    }
    if (n == 0) return HRL_OK;
    const int threads = widest <= 64 ? 64 : widest <= 128 ? 128 : 256;
    hipLaunchKernelGGL(rows_permute_kernel, dim3((unsigned)n, nleaves), dim3(threads), 0,
                       static_cast<hipStream_t>(stream), src_index, dst_index, L);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

}  // extern "C"
