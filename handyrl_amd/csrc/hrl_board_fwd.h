// hrl_board_fwd.h — the TicTacToe net's eval forward on one 16-row tile, as the device code that board_infer_kernel
// (hrl_infer.hip) and board_selfplay_kernel (hrl_boardplay.hip) share: ONE copy, so the two give the same bits.
//
// The pack layout (written by board_infer_pack_kernel, hrl_infer.hip), in 32-bit words:
//   [stem B fragments 1536][stem bias 32][heads 272] then per layer [B fragments 13824][a, b 64]
// board_forward_tile: a workgroup of 4 waves; the caller's load_obs() puts the tile's observations (16 x 27 fp32, rows
// past the end zeros) into obs_lds -- from HBM (board_infer_kernel) or from the boards in LDS (board_selfplay_kernel)
// -- at the place the register allocation of board_infer_kernel was measured with (157 VGPRs; moving it moves that):
//   * the 4 waves share the 9 output cells ({4,0}, {1,3}, {5,7}, {2,6,8}: 13/12/12/12 of the 49 (p, q) taps);
//   * a layer's 54 KB of B fragments are staged in LDS; the next layer's are in flight (global -> registers) while
//     this layer's MFMAs run; the activations (16 x 288 fp32) stay in one LDS tile, rewritten in place once every
//     wave has read it (a layer's outputs wait in the accumulators);
//   * six partial products on v_mfma_f32_16x16x32_bf16, smallest terms first; BN + ReLU as y*a + b, v < 0 ? 0 : v;
//     the heads' 1x1 convs + LeakyReLU(0.1) on the VALU into h_lds (27 mid values per row), then a barrier.
// board_policy_out / board_value_out: a row's policy logit o < 9 and its tanhf value from h_lds.
#ifndef HRL_BOARD_FWD_H
#define HRL_BOARD_FWD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hrl_split.h"

namespace {

using hrl_split::f32x4;
using hrl_split::mfma_bf16;
using hrl_split::mfma_split;
using hrl_split::split8;
using hrl_split::split_part;

constexpr int kCells = 9;
constexpr int kC = 32;
constexpr int kRow = kC * kCells;          // 288 floats per sample
constexpr int kStride = kRow + 2;          // LDS row stride, == 2 (mod 32)
constexpr int kTile = 16;                  // rows per workgroup
constexpr int kThreads = 256;
constexpr int kObs = 27;                   // 3 planes x 9 cells
constexpr int kA = 9;
constexpr int kMaxLayers = 8;
constexpr int kHMid = 28;                  // h_lds row stride (27 mid values)

// the pack, in 32-bit words
constexpr int kStemFragWords = 2 * 3 * 64 * 4;                 // 1536
constexpr int kStemBiasWords = kC;                             // 32
constexpr int kHeadFloats = 270;   // w1p[2][32] | b1p[2] | w1v[32] | b1v | fcp[9][18] | fcv[9]
constexpr int kHeadWords = 272;
constexpr int kHW1p = 0, kHB1p = 64, kHW1v = 66, kHB1v = 98, kHFcp = 99, kHFcv = 261;
constexpr int kLayerFragWords = 9 * 2 * 3 * 64 * 4;            // 13824 (54 KB)
constexpr int kLayerWords = kLayerFragWords + 2 * kC;
constexpr int kHeadOff = kStemFragWords + kStemBiasWords;      // words
constexpr int kLayer0Off = kHeadOff + kHeadWords;              // 1840 words = 7360 B
constexpr int kFragVec = kLayerFragWords / 4;                  // 3456 uint4
constexpr int kStage = (kFragVec + kThreads - 1) / kThreads;   // 14 per thread

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// cells of wave w: {4,0}, {1,3}, {5,7}, {2,6,8}
__device__ __forceinline__ int wave_cell(int wave, int s) {
    const int packed = wave == 0 ? 0x004 : wave == 1 ? 0x031 : wave == 2 ? 0x075 : 0x862;
    return (packed >> (4 * s)) & 15;
}

// a layer's B fragments, global -> registers (thread tid's share of the 3456 uint4)
__device__ __forceinline__ void prefetch(u32x4 (&wst)[kStage], const uint32_t *pack, int layer, int tid) {
    const u32x4 *src = reinterpret_cast<const u32x4 *>(pack + kLayer0Off + (int64_t)layer * kLayerWords);
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
        const int idx = tid + i * kThreads;
        wst[i] = src[idx < kFragVec ? idx : kFragVec - 1];
    }
}

// LDS: w_lds_u kLayerFragWords words (16-byte aligned), act kTile * kStride, head_w kHeadWords, h_lds kTile * kHMid.
// load_obs() stores the tile's observations (16 x 27 fp32, rows past the end zeros) in LDS and obs_lds names them.
// Ends with a barrier: h_lds is whole, and obs_lds, act and w_lds_u may be overwritten.
template <class LoadObs>
__device__ __forceinline__ void board_forward_tile(const uint32_t *pack, int layers, const float *obs_lds, float *act,
                                                   uint32_t *w_lds_u, float *head_w, float *h_lds, int tid,
                                                   LoadObs load_obs) {
    const int lane = tid & 63, wave = tid >> 6;
    const int ar = lane & 15, ak = lane >> 4;
    const int nq = wave == 3 ? 3 : 2;

    // observation tile and head weights -> LDS
    load_obs();
    for (int i = tid; i < kHeadWords; i += kThreads) head_w[i] = __uint_as_float(pack[kHeadOff + i]);

    // layer 0's B fragments: global -> registers now, -> LDS after the stem
    u32x4 wst[kStage];
    prefetch(wst, pack, 0, tid);

    // ---- stem: out[q][co] = relu(sum_k A_q[row][k] W[k][co] + bias[co]), k = ci*9 + tap over the cell's neighbourhood
    {
        const uint4 *sf = reinterpret_cast<const uint4 *>(pack) + lane;
        uint4 B[2][3];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int part = 0; part < 3; ++part) B[ct][part] = sf[(ct * 3 + part) * 64];
        const float sb0 = __uint_as_float(pack[kStemFragWords + ar]);
        const float sb1 = __uint_as_float(pack[kStemFragWords + 16 + ar]);
        __syncthreads();   // obs_lds
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (s >= nq) break;
            const int q = wave_cell(wave, s), qy = q / 3, qx = q - 3 * qy;
            float av[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = 8 * ak + e;
                const int ci = k / 9, t = k - 9 * ci;
                const int py = qy + t / 3 - 1, px = qx + t % 3 - 1;
                const bool ok = k < kObs && py >= 0 && py < 3 && px >= 0 && px < 3;
                const float x = obs_lds[ar * kObs + (ok ? ci * 9 + py * 3 + px : 0)];
                av[e] = ok ? x : 0.f;
            }
            uint4 Ah, Am, Al;
            split8(av, Ah, Am, Al);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                f32x4 c = (f32x4){0.f, 0.f, 0.f, 0.f};
                c = mfma_split(Ah, Am, Al, B[ct][0], B[ct][1], B[ct][2], c);
                const float bias = ct == 0 ? sb0 : sb1;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = ak * 4 + r, co = ct * 16 + ar;      // C/D: row = (lane>>4)*4 + reg, col = lane & 15
                    const float v = c[r] + bias;
                    act[row * kStride + co * kCells + q] = v < 0.f ? 0.f : v;
                }
            }
        }
    }

    // ---- the chain: conv -> BN -> ReLU per layer
    for (int layer = 0; layer < layers; ++layer) {
        {
            u32x4 *dst = reinterpret_cast<u32x4 *>(w_lds_u);
#pragma unroll
            for (int i = 0; i < kStage; ++i) {
                const int idx = tid + i * kThreads;
                if (idx < kFragVec) dst[idx] = wst[i];
            }
        }
        const uint32_t *coef = pack + kLayer0Off + (int64_t)layer * kLayerWords + kLayerFragWords;
        float ca[2], cb[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            ca[ct] = __uint_as_float(coef[ct * 16 + ar]);
            cb[ct] = __uint_as_float(coef[kC + ct * 16 + ar]);
        }
        __syncthreads();   // this layer's weights and its input tile are in LDS
        if (layer + 1 < layers) prefetch(wst, pack, layer + 1, tid);

        f32x4 acc[3][2];
#pragma unroll
        for (int s = 0; s < 3; ++s) acc[s][0] = acc[s][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float *acol = act + ar * kStride + 8 * ak * kCells;
        const uint4 *wb = reinterpret_cast<const uint4 *>(w_lds_u) + lane;
        float an[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) an[e] = acol[e * kCells];
#pragma unroll 1
        for (int p = 0; p < kCells; ++p) {
            float av[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) av[e] = an[e];
            if (p + 1 < kCells) {
#pragma unroll
                for (int e = 0; e < 8; ++e) an[e] = acol[e * kCells + p + 1];
            }
            uint4 Ah, Am, Al;
            split8(av, Ah, Am, Al);
            const int py = p / 3, px = p - 3 * py;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                if (s >= nq) break;
                const int q = wave_cell(wave, s);
                const int dy = py - q / 3 + 1, dx = px - q % 3 + 1;    // wave-uniform: scalar branches
                if (dy < 0 || dy > 2 || dx < 0 || dx > 2) continue;
                const int tap = dy * 3 + dx;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const uint4 *wf = wb + (tap * 2 + ct) * 3 * 64;
                    const uint4 Bh = wf[0], Bm = wf[64], Bl = wf[128];
                    acc[s][ct] = mfma_split(Ah, Am, Al, Bh, Bm, Bl, acc[s][ct]);
                }
            }
        }
        __syncthreads();   // every wave has read the tile and the weights: both may be overwritten
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (s >= nq) break;
            const int q = wave_cell(wave, s);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = ak * 4 + r, co = ct * 16 + ar;
                    const float v = acc[s][ct][r] * ca[ct] + cb[ct];
                    act[row * kStride + co * kCells + q] = v < 0.f ? 0.f : v;
                }
        }
    }
    __syncthreads();   // the last layer's tile is whole

    // ---- heads: 1x1 conv + bias, LeakyReLU(0.1); the 27 mid values of a row are [policy c0 | policy c1 | value]
    const float *as = act;
    for (int i = tid; i < kTile * 27; i += kThreads) {
        const int row = i / 27, j = i - row * 27;
        const int c = j / 9, q = j - 9 * c;
        const float *w1 = head_w + (c < 2 ? kHW1p + c * kC : kHW1v);
        const float *x = as + row * kStride + q;
        float sum = 0.f;
#pragma unroll 8
        for (int ci = 0; ci < kC; ++ci) sum += x[ci * kCells] * w1[ci];
        sum += c < 2 ? head_w[kHB1p + c] : head_w[kHB1v];
        h_lds[row * kHMid + j] = sum > 0.f ? sum : sum * 0.1f;
    }
    __syncthreads();
}

// policy logit o < kA of `row`: the bias-free linear over the 18 policy mid values
__device__ __forceinline__ float board_policy_out(const float *h_lds, const float *head_w, int row, int o) {
    const float *h = h_lds + row * kHMid;
    const float *w = head_w + kHFcp + o * 18;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 18; ++j) sum += h[j] * w[j];
    return sum;
}

// value of `row`: the bias-free linear over the 9 value mid values, tanhf
__device__ __forceinline__ float board_value_out(const float *h_lds, const float *head_w, int row) {
    const float *h = h_lds + row * kHMid;
    const float *w = head_w + kHFcv;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 9; ++j) sum += h[18 + j] * w[j];
    return tanhf(sum);
}

}  // namespace

#endif  // HRL_BOARD_FWD_H
