// hrl_pick.h — what the self-play tail (hrl_selfplay.hip) and the evaluator (hrl_eval.hip) share: torch.argmax's
// order and the counter-based generator of the public sampling rules (include/hrl_env.h).
#ifndef HRL_PICK_H
#define HRL_PICK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kWave = 64;

// torch.argmax's order: NaN beats everything, then larger values, ties to the lower index
__device__ __forceinline__ bool better(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

// Philox4x32-10 (Salmon et al., SC'11).  The rules (key, counter, word) are public: include/hrl_env.h,
// rollout.stream_uniforms and evaluation.eval_pick, which the kernels reproduce bit for bit.
__device__ __forceinline__ uint32_t philox_word(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                                uint32_t c3, int word) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return word == 0 ? c0 : word == 1 ? c1 : word == 2 ? c2 : c3;
}

}  // namespace

#endif  // HRL_PICK_H
