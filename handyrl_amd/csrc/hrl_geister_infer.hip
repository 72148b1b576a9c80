// hrl_geister_infer.hip — GeisterNet's complete eval forward as ONE launch, the recurrent state resident on chip.
//
// The net (handyrl/envs/geister.py:17-167): stem 3x3 conv 25 -> 32 + BN + ReLU = h_e; DRC of L ConvLSTM cells
// (3x3 conv of [h_e, h_l] 64 -> 128, gates i, f, o, g), every cell fed h_e and its own state, `repeats` times per
// ply; heads on [h_e, h_last].  Each layer reads only its own state, so the L layers are L independent recurrent
// chains: the grid is split over (16-game tile, layer) and nothing is shared or awaited between workgroups.
//
// One workgroup (4 waves, one per SIMD, the whole register file each) and one (tile, layer):
//  * LDS holds two fp32 images [cell][game][channel] of 73,728 B: E (h_e) and H (the stem's 25-channel input
//    first, then h_l).  The 16-byte chunks of a (cell, game) row are XOR-swizzled by (game >> 1) & 7, so the 16
//    lanes of an MFMA A-operand read (one game each, the same 8 channels) hit 16 different bank groups.
//  * stem: the real zero-padded 25-channel conv (the 18 scalar planes are constant over the board but still see
//    the padding: off-board taps are simply never computed), BN + ReLU from the accumulators into E.  Every layer's
//    workgroup recomputes it (1 of 2*repeats*2 + 1 k-steps) instead of waiting for another's.
//  * a wave owns two 16-column tiles of the layer's 128 gate channels for the whole launch.  The pack permutes the
//    columns so that column j of tile T is gate j >> 2 of hidden channel 4T + (j & 3): the four gates of one (game,
//    channel, cell) sit in four lanes of one 16-lane row and meet through a 4 x 4 lane transpose (three
//    ds_bpermute, no memory).  After it a lane owns game 4g + (r >> 2), channel 4T + (r & 3), all 36 cells: its
//    slice of c_l stays in registers across the repeats, and h_l is rewritten in H between two barriers.
//  * per repeat and tile the gates' pre-activations are the K = 64 conv([h_e, h_l]) in one set of 36-cell
//    accumulators: x-half fragments (27 uint4) loaded, E walked, h-half fragments loaded, H walked.  Holding the
//    x half (144 registers per tile) next to the accumulators (144) and the fragments (108) does not fit a wave's
//    512 registers with two tiles, and not 256 with one (8 waves); see DESIGN.
//  * the last layer's workgroup then runs the heads from E and H: the move head's 3x3 conv 64 -> p_filters on the
//    MFMA (a wave per band of 9 cells) with BN + ReLU and the 1x1 conv to 4 planes through lane shuffles, the value
//    / return 1x1 convs + BN + ReLU + fc on the VALU, and head_p_set.
// Arithmetic: the exact three-way bf16 split of hrl_split.h on v_mfma_f32_16x16x32_bf16 (six partial products,
// fp32 accumulation), BatchNorm as y*alpha + beta, ReLU as v < 0 ? 0 : v, lstm_fwd_kernel's sigm / tanhf, fp32 state.
// A row's result depends on nothing but the row.  Bound: MFMA, then the gates' transcendentals.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/hrl_nn.h"
#include "../../include/hrl_targets.h"
#include "hrl_split.h"

#ifndef HRL_GEISTER_INFER_WAVES
#define HRL_GEISTER_INFER_WAVES 4   // 8: the one-tile-per-wave shape (256 registers per wave), kept for the record
#endif

namespace {

using hrl_split::f32x4;
using hrl_split::mfma_split;
using hrl_split::split8;

constexpr int kBW = 6, kHW = 36, kQuads = 9, kTaps = 9;
constexpr int kC = 32;                 // filters
constexpr int kBoardPlanes = 7, kScalars = 18, kCin = kBoardPlanes + kScalars;
constexpr int kMoves = 144, kSets = 70, kActions = kMoves + kSets;
constexpr int kMaxLayers = 4, kMaxRepeats = 8;
constexpr int kNW = HRL_GEISTER_INFER_WAVES, kThreads = 64 * kNW;
constexpr int kTPW = 8 / kNW;          // column tiles per wave
constexpr int kGridCap = 256;          // one resident workgroup per CU; further (tile, layer) items are walked
constexpr int kImg = kHW * 16 * kC;    // floats of one image
constexpr int kCell = 16 * kC;         // floats from one cell to the next

// ---- the pack: fragment sets of 27 x 64 uint4 ([tap][part][lane], hrl_gboard's fragment), then floats
constexpr int kSetVecs = kTaps * 3 * 64;
__host__ __device__ constexpr int set_stem(int ct) { return ct; }
__host__ __device__ constexpr int set_cell(int l, int half, int t) { return 2 + (l * 2 + half) * 8 + t; }
__host__ __device__ constexpr int set_move(int L, int kc) { return 2 + L * 16 + kc; }
__host__ __device__ constexpr int n_sets(int L) { return 4 + L * 16; }
constexpr int F_BN1A = 0, F_BN1B = 32, F_BNPA = 64, F_BNPB = 80, F_VR = 96 /* av, bv, ar, br */, F_W2 = 112,
              F_WV = 144, F_WR = 208, F_FCV = 272, F_FCR = 308, F_PSW = 344, F_PSB = 414, F_BIAS = 496;
__host__ __device__ constexpr int n_floats(int L) { return F_BIAS + 128 * L; }

struct PackArgs {
    const float *stem_w, *cell_w[kMaxLayers], *cell_b[kMaxLayers];
    const float *bn_w[4], *bn_b[4], *bn_mean[4], *bn_var[4];   // bn1, move head, value, return
    double eps[4];
    const float *move_w1, *move_w2, *value_w, *return_w, *value_fc, *return_fc, *set_w, *set_b;
    int L, pf;
    uint32_t *out;
};

__global__ void geister_pack_kernel(PackArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int nfrag = n_sets(a.L) * kSetVecs * 4;
    if (i < nfrag) {
        // lane l of a set holds W^T[ci = 8(l>>4) + e][column l&15], e = 2d, 2d+1 in word d
        const int d = i & 3, l = (i >> 2) & 63;
        int rest = i >> 8;
        const int part = rest % 3;
        rest /= 3;
        const int tap = rest % kTaps, set = rest / kTaps;
        const int j = l & 15, ci = 8 * (l >> 4) + 2 * d;
        const float *w;
        int co, cin_total, ci0, cin, cout;
        if (set < 2) {
            w = a.stem_w, co = 16 * set + j, cin_total = kCin, ci0 = 0, cin = kCin, cout = kC;
        } else if (set < 2 + 16 * a.L) {
            const int s = set - 2, layer = s >> 4, half = (s >> 3) & 1, t = s & 7;
            w = a.cell_w[layer], co = (j >> 2) * kC + 4 * t + (j & 3), cin_total = 2 * kC, ci0 = half * kC, cin = kC;
            cout = 4 * kC;
        } else {
            const int kc = set - 2 - 16 * a.L;
            w = a.move_w1, co = j, cin_total = 2 * kC, ci0 = kc * kC, cin = kC, cout = a.pf;
        }
        auto wv = [&](int c) -> float {
            return (co < cout && c < cin) ? w[((int64_t)co * cin_total + ci0 + c) * kTaps + tap] : 0.f;
        };
        a.out[i] = hrl_split::split_part(wv(ci), part) | (hrl_split::split_part(wv(ci + 1), part) << 16);
        return;
    }
    const int f = i - nfrag;
    if (f >= n_floats(a.L)) return;
    float v = 0.f;
    auto bn = [&](int k, int c, int beta) -> float {   // bn_eval_coef_kernel's operations
        const float invstd = (float)(1.0 / sqrt((double)a.bn_var[k][c] + a.eps[k]));
        const float al = invstd * a.bn_w[k][c];
        return beta ? a.bn_b[k][c] - a.bn_mean[k][c] * al : al;
    };
    if (f < F_BNPA) v = bn(0, f & 31, f >= F_BN1B);
    else if (f < F_VR) v = ((f & 15) < a.pf) ? bn(1, f & 15, f >= F_BNPB) : 0.f;
    else if (f < F_VR + 4) v = bn(2 + ((f - F_VR) >> 1), 0, (f - F_VR) & 1);
    else if (f < F_W2) v = 0.f;
    else if (f < F_WV) v = ((f - F_W2) & 7) < a.pf ? a.move_w2[((f - F_W2) >> 3) * a.pf + ((f - F_W2) & 7)] : 0.f;
    else if (f < F_WR) v = a.value_w[f - F_WV];
    else if (f < F_FCV) v = a.return_w[f - F_WR];
    else if (f < F_FCR) v = a.value_fc[f - F_FCV];
    else if (f < F_PSW) v = a.return_fc[f - F_FCR];
    else if (f < F_PSB) v = a.set_w[f - F_PSW];
    else if (f < F_PSB + kSets) v = a.set_b[f - F_PSB];
    else if (f < F_BIAS) v = 0.f;
    else {
        const int layer = (f - F_BIAS) >> 7;
        v = a.cell_b[layer] ? a.cell_b[layer][(f - F_BIAS) & 127] : 0.f;
    }
    a.out[i] = __float_as_uint(v);
}

// ---- the forward
struct InferArgs {
    const uint4 *frag;
    const float *fl;
    const float *board, *scalar, *h, *c;
    float *policy, *value, *ret, *h_out, *c_out;
    int64_t N;
    int L, repeats, pf;
};

template <int I> using IC = std::integral_constant<int, I>;
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(IC<I>{});
        static_for<I + 1, N>(f);
    }
}

__host__ __device__ constexpr int tap_pq(int p, int q) {   // tap of input cell p for output cell q, -1 off the 3x3
    const int dy = p / kBW - q / kBW + 1, dx = p % kBW - q % kBW + 1;
    return (dy < 0 || dy > 2 || dx < 0 || dx > 2) ? -1 : dy * 3 + dx;
}
__host__ __device__ constexpr bool cells_use(int c0, int c1, int p) {
    for (int q = c0; q < c1; ++q)
        if (tap_pq(p, q) >= 0) return true;
    return false;
}

__device__ __forceinline__ float relu_f(float v) { return v < 0.f ? 0.f : v; }          // NaN stays NaN
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }     // lstm_fwd_kernel's
__device__ __forceinline__ float sel4(const f32x4 &v, int k) {
    return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3]));
}
// float index of (cell, game, channel) in an image
__device__ __forceinline__ int img_at(int cell, int game, int ch) {
    return cell * kCell + game * kC + ((((ch >> 2) ^ ((game >> 1) & 7)) << 2) | (ch & 3));
}

__device__ __forceinline__ void load_b(const uint4 *frag, int set, int lane, uint4 (&B)[kTaps][3]) {
    const uint4 *wp = frag + (int64_t)set * kSetVecs + lane;
    static_for<0, kTaps * 3>([&](auto i_c) __attribute__((always_inline)) {
        constexpr int i = decltype(i_c)::value;
        B[i / 3][i % 3] = wp[i * 64];
    });
}

// acc[q - C0] += sum over the real taps of A(img, cell p) . B[tap(p, q)] for the output cells q in [C0, C1); a0 / a1:
// the lane's float offsets of its two 16-byte chunks (channels 8g .. 8g + 7 of game r) within a cell
template <int C0, int C1>
__device__ __forceinline__ void conv_cells(const float *img, int a0, int a1, const uint4 (&B)[kTaps][3],
                                           f32x4 (&acc)[C1 - C0]) {
    static_for<0, kHW>([&](auto p_c) __attribute__((always_inline)) {
        constexpr int p = decltype(p_c)::value;
        if constexpr (cells_use(C0, C1, p)) {
            const float4 lo = *reinterpret_cast<const float4 *>(img + p * kCell + a0);
            const float4 hi = *reinterpret_cast<const float4 *>(img + p * kCell + a1);
            const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            uint4 Ah, Am, Al;
            split8(v, Ah, Am, Al);
            static_for<C0, C1>([&](auto q_c) __attribute__((always_inline)) {
                constexpr int q = decltype(q_c)::value;
                constexpr int t = tap_pq(p, q);
                if constexpr (t >= 0) acc[q - C0] = mfma_split(Ah, Am, Al, B[t][0], B[t][1], B[t][2], acc[q - C0]);
            });
            __builtin_amdgcn_sched_barrier(0);   // keeps later cells' LDS reads and splits from being hoisted
        }
    });
}

template <int NC>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[NC]) {
    static_for<0, NC>([&](auto q_c) __attribute__((always_inline)) {
        acc[decltype(q_c)::value] = (f32x4){0.f, 0.f, 0.f, 0.f};
    });
}

// the stem for output cells [C0, C1) of column tile ct: conv from H (the input image), BN + ReLU into E
template <int C0, int C1>
__device__ __forceinline__ void stem_cells(const InferArgs &a, const float *imgH, float *imgE, int ct, int lane,
                                           int a0, int a1) {
    uint4 B[kTaps][3];
    f32x4 acc[C1 - C0];
    load_b(a.frag, set_stem(ct), lane, B);
    zero_acc(acc);
    conv_cells<C0, C1>(imgH, a0, a1, B, acc);
    const int r = lane & 15, g = lane >> 4, ch = 16 * ct + r;
    const float al = a.fl[F_BN1A + ch], be = a.fl[F_BN1B + ch];
    static_for<C0, C1>([&](auto q_c) __attribute__((always_inline)) {
        constexpr int q = decltype(q_c)::value;
#pragma unroll
        for (int i = 0; i < 4; ++i) imgE[img_at(q, 4 * g + i, ch)] = relu_f(acc[q - C0][i] * al + be);
    });
}

// the move head for output cells [C0, C1): 3x3 conv of [E, H] -> BN + ReLU -> 1x1 conv to 4 planes -> policy
template <int C0, int C1>
__device__ __forceinline__ void move_cells(const InferArgs &a, const float *imgE, const float *imgH, int64_t n0,
                                           int lane, int a0, int a1) {
    uint4 B[kTaps][3];
    f32x4 acc[C1 - C0];
    zero_acc(acc);
    load_b(a.frag, set_move(a.L, 0), lane, B);
    conv_cells<C0, C1>(imgE, a0, a1, B, acc);
    load_b(a.frag, set_move(a.L, 1), lane, B);
    conv_cells<C0, C1>(imgH, a0, a1, B, acc);
    const int r = lane & 15, g = lane >> 4;
    const float al = a.fl[F_BNPA + r], be = a.fl[F_BNPB + r];
    float w2[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) w2[c] = a.fl[F_W2 + (r & 3) * 8 + c];
    static_for<C0, C1>([&](auto q_c) __attribute__((always_inline)) {
        constexpr int q = decltype(q_c)::value;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = relu_f(acc[q - C0][i] * al + be);   // column r = channel r of the head (0 past p_filters)
            float o = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float vc = __shfl(v, (lane & ~15) | c);
                if (c < a.pf) o = o + w2[c] * vc;               // channels in order, as the pointwise kernel
            }
            const int64_t n = n0 + 4 * g + i;
            if (r < 4 && n < a.N) a.policy[n * kActions + r * kHW + q] = o;
        }
    });
}

__global__ __launch_bounds__(kThreads) void geister_infer_kernel(InferArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kImg + 16 * kHW * 2];
    float *imgE = smem, *imgH = smem + kImg, *scr = smem + 2 * kImg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    // A operand: game r, channels 8g .. 8g + 7 = chunks 2g, 2g + 1, swizzled
    const int sw = (r >> 1) & 7;
    const int a0 = r * kC + (((2 * g) ^ sw) << 2), a1 = r * kC + (((2 * g + 1) ^ sw) << 2);
    // after the gates' transpose: game 4g + kk, hidden channel 4T + cl
    const int kk = r >> 2, cl = r & 3, gm = 4 * g + kk;
    const int64_t ntiles = (a.N + 15) >> 4, nitems = ntiles * a.L;
    const int64_t srow = (int64_t)a.L * kC * kHW;   // floats of one row of the stacked state

    for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int64_t n0 = (item / a.L) * 16;
        const int layer = (int)(item % a.L);
        // ---- the stem's input into H: channels 0..17 the scalars (constant over the board), 18..24 the board
        for (int idx = tid; idx < 16 * kC * kQuads; idx += kThreads) {
            const int quad = idx % kQuads, ch = (idx / kQuads) % kC, game = idx / (kQuads * kC);
            const int64_t n = n0 + game;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < a.N) {
                if (ch < kScalars) {
                    const float s = a.scalar[n * kScalars + ch];
                    v = make_float4(s, s, s, s);
                } else if (ch < kCin) {
                    v = *reinterpret_cast<const float4 *>(a.board + (n * kBoardPlanes + ch - kScalars) * kHW + 4 * quad);
                }
            }
            imgH[img_at(4 * quad + 0, game, ch)] = v.x;
            imgH[img_at(4 * quad + 1, game, ch)] = v.y;
            imgH[img_at(4 * quad + 2, game, ch)] = v.z;
            imgH[img_at(4 * quad + 3, game, ch)] = v.w;
        }
        __syncthreads();
        {   // ---- stem: column tile wave & 1, a band of the cells per wave pair
            const int ct = wave & 1, band = wave >> 1;
            if constexpr (kNW == 4) {
                if (band == 0) stem_cells<0, 18>(a, imgH, imgE, ct, lane, a0, a1);
                else stem_cells<18, 36>(a, imgH, imgE, ct, lane, a0, a1);
            } else {
                switch (band) {
                case 0: stem_cells<0, 9>(a, imgH, imgE, ct, lane, a0, a1); break;
                case 1: stem_cells<9, 18>(a, imgH, imgE, ct, lane, a0, a1); break;
                case 2: stem_cells<18, 27>(a, imgH, imgE, ct, lane, a0, a1); break;
                default: stem_cells<27, 36>(a, imgH, imgE, ct, lane, a0, a1); break;
                }
            }
        }
        __syncthreads();
        // ---- the layer's state: h_l into H, the lane's slice of c_l into registers
        for (int idx = tid; idx < 16 * kC * kQuads; idx += kThreads) {
            const int quad = idx % kQuads, ch = (idx / kQuads) % kC, game = idx / (kQuads * kC);
            const int64_t n = n0 + game;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < a.N) v = *reinterpret_cast<const float4 *>(a.h + n * srow + (layer * kC + ch) * kHW + 4 * quad);
            imgH[img_at(4 * quad + 0, game, ch)] = v.x;
            imgH[img_at(4 * quad + 1, game, ch)] = v.y;
            imgH[img_at(4 * quad + 2, game, ch)] = v.z;
            imgH[img_at(4 * quad + 3, game, ch)] = v.w;
        }
        const int64_t nl = n0 + gm;   // the lane's game
        float cst[kTPW][kHW], hn[kTPW][kHW], bias[kTPW][4];
        static_for<0, kTPW>([&](auto tt_c) __attribute__((always_inline)) {
            constexpr int tt = decltype(tt_c)::value;
            const int ch = 4 * (wave * kTPW + tt) + cl;
            const float *cp = a.c + nl * srow + (layer * kC + ch) * kHW;
            static_for<0, kQuads>([&](auto j_c) __attribute__((always_inline)) {
                constexpr int j = decltype(j_c)::value;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (nl < a.N) v = *reinterpret_cast<const float4 *>(cp + 4 * j);
                cst[tt][4 * j + 0] = v.x;
                cst[tt][4 * j + 1] = v.y;
                cst[tt][4 * j + 2] = v.z;
                cst[tt][4 * j + 3] = v.w;
            });
#pragma unroll
            for (int t = 0; t < 4; ++t) bias[tt][t] = a.fl[F_BIAS + layer * 128 + t * kC + ch];
        });
        __syncthreads();
        // ---- the repeats
        for (int rep = 0; rep < a.repeats; ++rep) {
            static_for<0, kTPW>([&](auto tt_c) __attribute__((always_inline)) {
                constexpr int tt = decltype(tt_c)::value;
                const int T = wave * kTPW + tt;
                uint4 B[kTaps][3];
                f32x4 acc[kHW];
                zero_acc(acc);
                load_b(a.frag, set_cell(layer, 0, T), lane, B);
                conv_cells<0, kHW>(imgE, a0, a1, B, acc);
                load_b(a.frag, set_cell(layer, 1, T), lane, B);
                conv_cells<0, kHW>(imgH, a0, a1, B, acc);
                // gates: the lane holds gate kk of games 4g + i; it takes gates 0..3 of game 4g + kk
                static_for<0, kHW>([&](auto q_c) __attribute__((always_inline)) {
                    constexpr int q = decltype(q_c)::value;
                    float rcv[4];
                    rcv[0] = sel4(acc[q], kk);
#pragma unroll
                    for (int s = 1; s < 4; ++s)   // from the lane of gate (kk + s) & 3: its value for game 4g + kk
                        rcv[s] = __shfl(sel4(acc[q], (kk - s) & 3), (lane & ~12) | (((kk + s) & 3) << 2));
                    float z[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int d = (t - kk) & 3;
                        z[t] = (d == 0 ? rcv[0] : (d == 1 ? rcv[1] : (d == 2 ? rcv[2] : rcv[3]))) + bias[tt][t];
                    }
                    const float si = sigm(z[0]), sf = sigm(z[1]), so = sigm(z[2]), tg = tanhf(z[3]);
                    const float fc = sf * cst[tt][q];
                    const float ig = si * tg;
                    const float cc = fc + ig;
                    cst[tt][q] = cc;
                    hn[tt][q] = so * tanhf(cc);
                    __builtin_amdgcn_sched_barrier(0);   // one cell's exchange and gates at a time
                });
            });
            __syncthreads();   // every wave has read the old h_l
            static_for<0, kTPW>([&](auto tt_c) __attribute__((always_inline)) {
                constexpr int tt = decltype(tt_c)::value;
                const int ch = 4 * (wave * kTPW + tt) + cl;
                static_for<0, kHW>([&](auto q_c) __attribute__((always_inline)) {
                    constexpr int q = decltype(q_c)::value;
                    imgH[img_at(q, gm, ch)] = hn[tt][q];
                });
            });
            __syncthreads();
        }
        // ---- the advanced state (each workgroup reads and writes only its own (tile, layer) slice: in place is safe)
        if (nl < a.N) {
            static_for<0, kTPW>([&](auto tt_c) __attribute__((always_inline)) {
                constexpr int tt = decltype(tt_c)::value;
                const int ch = 4 * (wave * kTPW + tt) + cl;
                float *hp = a.h_out + nl * srow + (layer * kC + ch) * kHW;
                float *cp = a.c_out + nl * srow + (layer * kC + ch) * kHW;
                static_for<0, kQuads>([&](auto j_c) __attribute__((always_inline)) {
                    constexpr int j = decltype(j_c)::value;
                    *reinterpret_cast<float4 *>(hp + 4 * j) =
                        make_float4(hn[tt][4 * j], hn[tt][4 * j + 1], hn[tt][4 * j + 2], hn[tt][4 * j + 3]);
                    *reinterpret_cast<float4 *>(cp + 4 * j) =
                        make_float4(cst[tt][4 * j], cst[tt][4 * j + 1], cst[tt][4 * j + 2], cst[tt][4 * j + 3]);
                });
            });
        }
        // ---- the heads, from E = h_e and H = h_last
        if (layer == a.L - 1) {
            switch (wave) {
            case 0: move_cells<0, 9>(a, imgE, imgH, n0, lane, a0, a1); break;
            case 1: move_cells<9, 18>(a, imgE, imgH, n0, lane, a0, a1); break;
            case 2: move_cells<18, 27>(a, imgE, imgH, n0, lane, a0, a1); break;
            case 3: move_cells<27, 36>(a, imgE, imgH, n0, lane, a0, a1); break;
            default: break;
            }
            // value / return: 1x1 conv 64 -> 1 each (channels in order), BN + ReLU; a thread per (game, cell)
            for (int it = tid; it < 16 * kHW; it += kThreads) {
                const int game = it & 15, cell = it >> 4;
                const int s = (game >> 1) & 7;
                float sv = 0.f, sr = 0.f;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const float *row = (half ? imgH : imgE) + cell * kCell + game * kC;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float4 x = *reinterpret_cast<const float4 *>(row + ((k ^ s) << 2));
                        const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            sv = sv + a.fl[F_WV + half * kC + 4 * k + e] * xs[e];
                            sr = sr + a.fl[F_WR + half * kC + 4 * k + e] * xs[e];
                        }
                    }
                }
                scr[(game * kHW + cell) * 2 + 0] = relu_f(sv * a.fl[F_VR + 0] + a.fl[F_VR + 1]);
                scr[(game * kHW + cell) * 2 + 1] = relu_f(sr * a.fl[F_VR + 2] + a.fl[F_VR + 3]);
            }
            __syncthreads();
            if (tid < 32) {   // the fc 36 -> 1 of each head, cells in order
                const int game = tid >> 1, head = tid & 1;
                float sum = 0.f;
                for (int q = 0; q < kHW; ++q)
                    sum = sum + a.fl[(head ? F_FCR : F_FCV) + q] * scr[(game * kHW + q) * 2 + head];
                const int64_t n = n0 + game;
                if (n < a.N) {
                    if (head) a.ret[n] = sum;
                    else a.value[n] = tanhf(sum);
                }
            }
            for (int idx = tid; idx < 16 * kSets; idx += kThreads) {   // head_p_set: Linear(1, 70) of scalar[:, 0]
                const int game = idx / kSets, j = idx % kSets;
                const int64_t n = n0 + game;
                if (n < a.N) a.policy[n * kActions + kMoves + j] = a.scalar[n * kScalars] * a.fl[F_PSW + j] + a.fl[F_PSB + j];
            }
        }
        __syncthreads();   // the next item refills H and E
    }
}

int status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)e;
}

bool shape_ok(int64_t layers, int64_t p_filters) {
    return layers >= 1 && layers <= kMaxLayers && (p_filters == 1 || p_filters == 2 || p_filters == 4 || p_filters == 8);
}

}  // namespace

extern "C" {

int64_t hrl_geister_infer_pack_bytes(int64_t layers, int64_t p_filters) {
    if (!shape_ok(layers, p_filters)) return 0;
    return (int64_t)n_sets((int)layers) * kSetVecs * 16 + (int64_t)n_floats((int)layers) * 4;
}

int hrl_geister_infer_pack(const float *stem_w, const float *const *cell_w, const float *const *cell_b,
                           int64_t layers, const float *const *bn_w, const float *const *bn_b,
                           const float *const *bn_mean, const float *const *bn_var, const double *bn_eps,
                           const float *move_w1, const float *move_w2, int64_t p_filters, const float *value_w,
                           const float *return_w, const float *value_fc, const float *return_fc, const float *set_w,
                           const float *set_b, void *pack, void *stream) {
    if (!shape_ok(layers, p_filters) || !stem_w || !cell_w || !bn_w || !bn_b || !bn_mean || !bn_var || !bn_eps ||
        !move_w1 || !move_w2 || !value_w || !return_w || !value_fc || !return_fc || !set_w || !set_b || !pack ||
        (reinterpret_cast<uintptr_t>(pack) & 15))
        return HRL_EINVAL;
    PackArgs a{};
    for (int l = 0; l < layers; ++l) {
        if (!cell_w[l]) return HRL_EINVAL;
        a.cell_w[l] = cell_w[l];
        a.cell_b[l] = cell_b ? cell_b[l] : nullptr;
        if ((a.cell_b[l] == nullptr) != (a.cell_b[0] == nullptr)) return HRL_EINVAL;   // biased or bias-free, all cells
    }
    for (int k = 0; k < 4; ++k) {
        if (!bn_w[k] || !bn_b[k] || !bn_mean[k] || !bn_var[k]) return HRL_EINVAL;
        a.bn_w[k] = bn_w[k];
        a.bn_b[k] = bn_b[k];
        a.bn_mean[k] = bn_mean[k];
        a.bn_var[k] = bn_var[k];
        a.eps[k] = bn_eps[k];
    }
    a.stem_w = stem_w;
    a.move_w1 = move_w1;
    a.move_w2 = move_w2;
    a.value_w = value_w;
    a.return_w = return_w;
    a.value_fc = value_fc;
    a.return_fc = return_fc;
    a.set_w = set_w;
    a.set_b = set_b;
    a.L = (int)layers;
    a.pf = (int)p_filters;
    a.out = static_cast<uint32_t *>(pack);
    const int total = n_sets(a.L) * kSetVecs * 4 + n_floats(a.L);
    hipLaunchKernelGGL(geister_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a);
    return status();
}

int hrl_geister_infer(const void *pack, int64_t layers, int64_t num_repeats, int64_t p_filters, const float *board,
                      const float *scalar, const float *h, const float *c, int64_t N, float *policy, float *value,
                      float *ret, float *h_out, float *c_out, void *stream) {
    auto misaligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    if (!shape_ok(layers, p_filters) || num_repeats < 1 || num_repeats > kMaxRepeats || !pack || !board || !scalar ||
        !h || !c || !policy || !value || !ret || !h_out || !c_out || N < 0 || N > ((int64_t)1 << 31) - 17 ||
        misaligned(pack) || misaligned(board) || misaligned(h) || misaligned(c) || misaligned(h_out) ||
        misaligned(c_out))
        return HRL_EINVAL;
    if (N == 0) return HRL_OK;
    InferArgs a{};
    a.frag = static_cast<const uint4 *>(pack);
    a.fl = reinterpret_cast<const float *>(a.frag + (int64_t)n_sets((int)layers) * kSetVecs);
    a.board = board;
    a.scalar = scalar;
    a.h = h;
    a.c = c;
    a.policy = policy;
    a.value = value;
    a.ret = ret;
    a.h_out = h_out;
    a.c_out = c_out;
    a.N = N;
    a.L = (int)layers;
    a.repeats = (int)num_repeats;
    a.pf = (int)p_filters;
    const int64_t items = ((N + 15) >> 4) * layers;
    hipLaunchKernelGGL(geister_infer_kernel, dim3((unsigned)(items < kGridCap ? items : kGridCap)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return status();
}

}  // extern "C"
