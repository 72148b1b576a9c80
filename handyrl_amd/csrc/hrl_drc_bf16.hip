// hrl_drc_bf16.hip — one repeat of a DRC's L ConvLSTM cells at one time step as ONE launch with bf16 h-half operands
// (gfx950): the GeisterNet learner's form of hrl_geister_infer_bf16.hip's cell (train_args precision: bf16_drc).  It
// replaces the pair hrl_gboard_forward_groups + hrl_lstm_gates_forward_grouped and the fp32 zh tensor between them.
//
// Numeric contract (include/hrl_nn.h has the full text): the h-half weights are rounded fp32 -> bf16 at pack time,
// h_in is rounded to bf16 as it is staged into LDS, everything else is fp32.  The MFMA accumulator starts from zx
// (which carries the cell bias) and takes the h half's products after it, input cells in order; gates with
// lstm_fwd_kernel's sigm / tanhf in the order i, f, o, g; c' = f*c + i*g, h' = o*tanh(c'), both written unrounded.
//
// Work item = (16-game tile, layer, 16-column gate tile), one workgroup of 4 waves each; N = 256, L = 3 is 384
// workgroups.  Column j of tile T is gate j >> 2 of hidden channel 4T + (j & 3) (the pack's permutation), so the four
// gates of a hidden channel lie in lanes r, r ^ 4, r ^ 8, r ^ 12 of one 16-lane group.
//  * LDS: one bf16 image [cell 36][game 16][32 ch] of the layer's h, 64 B per (cell, game), 36,864 B (four workgroups
//    per CU by LDS; the 204 registers allow two, and a 128-register build spills: DESIGN 4.31).  A row's four 16-byte chunks are XOR-swizzled by (game >> 2) & 3, hrl_geister_infer_bf16.hip's layout and
//    bank arithmetic: the 16 lanes of an A-operand read (games 0..15, one chunk) cover the 16 bank groups once, one
//    conflict-free ds_read_b128.  The eight column-tile workgroups of a (tile, layer) stage the same image from L2.
//  * wave w owns output cells 9w .. 9w + 8.  Games are the MFMA rows, K = 32 is all h channels: one
//    v_mfma_f32_16x16x32_bf16 per on-board tap, 64 per wave, 256 per item.  Accumulators 36 registers, the B
//    fragments 9 uint4 = 36 (straight from the pack), the A operand double-buffered.
//  * gates: the 4 x 4 lane transpose (three ds_bpermute per cell); after it a lane owns game 4g + (r >> 2), hidden
//    channel 4T + (r & 3) and its wave's 9 cells: 45 transcendentals per lane.  9 consecutive floats per lane and
//    tensor go to h_out, c_out and (where stored) the four gate planes.
// A row's result depends on nothing but the row.  Deterministic.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/hrl_nn.h"
#include "../../include/hrl_targets.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kBW = 6, kHW = 36, kQuads = 9, kTaps = 9;
constexpr int kC = 32;                 // hidden channels = K of one MFMA
constexpr int kMaxLayers = 4;
constexpr int kTiles = 8;              // 16-column tiles of a layer's 128 gate channels
constexpr int kWaves = 4, kThreads = 64 * kWaves, kBand = kHW / kWaves;   // 9 output cells per wave
constexpr int kCellW = 16 * kC / 2;    // 4-byte words from one cell to the next (16 games x 32 bf16)
constexpr int kImgW = kHW * kCellW;    // words of the image (36,864 B)
constexpr int kSetVecs = kTaps * 64;   // uint4 of one (layer, tile) fragment set: [tap][lane], 9,216 B
constexpr int64_t kMaxN = (int64_t)1 << 24;   // at most 2^25 items: the grid and the int index math stay in range

// two fp32 -> two bf16, round to nearest even (a in the low half)
__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

struct PackArgs {
    const float *w[kMaxLayers];
    int L, cin_total, ci0;
    uint32_t *out;
};

// lane l of set (layer, T) holds bf16(W[co][ci0 + 8(l >> 4) + e][tap]) for column j = l & 15,
// co = (j >> 2)*32 + 4T + (j & 3), e = 2d, 2d + 1 in word d
__global__ __launch_bounds__(256) void drc_bf16_pack_kernel(PackArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.L * kTiles * kSetVecs * 4) return;
    const int d = i & 3, l = (i >> 2) & 63;
    const int rest = i >> 8;
    const int tap = rest % kTaps, set = rest / kTaps;
    const int layer = set / kTiles, t = set % kTiles;
    const int j = l & 15, ci = 8 * (l >> 4) + 2 * d;
    const int co = (j >> 2) * kC + 4 * t + (j & 3);
    const float *w = a.w[layer] + ((int64_t)co * a.cin_total + a.ci0 + ci) * kTaps + tap;
    a.out[i] = bf16_pair(w[0], w[kTaps]);
}

struct StepArgs {
    const uint4 *frag;
    const float *zx[kMaxLayers], *h[kMaxLayers], *c[kMaxLayers];
    int64_t zxs[kMaxLayers], hs[kMaxLayers], cs[kMaxLayers];
    float *h_out[kMaxLayers], *c_out[kMaxLayers], *gates[kMaxLayers];
    int64_t N;
    int L;
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
    if (p < 0 || p >= kHW) return false;
    for (int q = c0; q < c1; ++q)
        if (tap_pq(p, q) >= 0) return true;
    return false;
}
__host__ __device__ constexpr int next_used(int c0, int c1, int p) {   // the first input cell past p the band reads
    for (int n = p + 1; n < kHW; ++n)
        if (cells_use(c0, c1, n)) return n;
    return kHW;
}

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }     // lstm_fwd_kernel's
__device__ __forceinline__ float sel4(const f32x4 &v, int k) {
    return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3]));
}
// word index of channels 2cp, 2cp + 1 of (cell, game) in the image
__device__ __forceinline__ int img_w(int cell, int game, int cp) {
    return cell * kCellW + game * 16 + ((((cp >> 2) ^ ((game >> 2) & 3)) << 2) | (cp & 3));
}

__device__ __forceinline__ f32x4 mfma(const uint4 &a, const uint4 &b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                   0, 0);
}

// acc[q - C0] += sum over the on-board taps of A(img, cell p) . B[tap(p, q)] for the output cells q in [C0, C1), the
// input cells p in order; ao: the lane's uint4 index of its chunk (channels 8g .. 8g + 7 of game r) within a cell.
// The next cell's operand is read while this cell's MFMAs issue.
template <int C0, int C1>
__device__ __forceinline__ void conv_cells(const uint32_t *img, int ao, const uint4 (&B)[kTaps],
                                           f32x4 (&acc)[C1 - C0]) {
    const uint4 *ip = reinterpret_cast<const uint4 *>(img) + ao;
    constexpr int first = next_used(C0, C1, -1);
    uint4 A = ip[first * (kCellW / 4)];
    static_for<0, kHW>([&](auto p_c) __attribute__((always_inline)) {
        constexpr int p = decltype(p_c)::value;
        if constexpr (cells_use(C0, C1, p)) {
            constexpr int nx = next_used(C0, C1, p);
            uint4 An = A;
            if constexpr (nx < kHW) An = ip[nx * (kCellW / 4)];
            static_for<C0, C1>([&](auto q_c) __attribute__((always_inline)) {
                constexpr int q = decltype(q_c)::value;
                constexpr int t = tap_pq(p, q);
                if constexpr (t >= 0) acc[q - C0] = mfma(A, B[t], acc[q - C0]);
            });
            A = An;
            __builtin_amdgcn_sched_barrier(0);   // keeps later cells' LDS reads from being hoisted
        }
    });
}

// one wave's band of output cells [C0, C0 + 9) of item (rows n0.., layer, column tile T)
template <int C0>
__device__ __forceinline__ void band(const StepArgs &a, const uint32_t *img, int64_t n0, int layer, int T, int lane) {
    const int r = lane & 15, g = lane >> 4;
    // ---- the accumulators start from the x half: rows = games 4g + i, column r = gate r >> 2 of channel 4T + (r & 3)
    f32x4 acc[kBand];
    {
        const float *zp = a.zx[layer] + ((r >> 2) * kC + 4 * T + (r & 3)) * kHW + C0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // a row past N reads row N - 1 (its results are never stored): no branches
            const int64_t n = n0 + 4 * g + i;
            const float *p = zp + (n < a.N ? n : a.N - 1) * a.zxs[layer];
            static_for<0, kBand>([&](auto q_c) __attribute__((always_inline)) {
                constexpr int q = decltype(q_c)::value;
                acc[q][i] = p[q];
            });
        }
    }
    uint4 B[kTaps];   // the tile's column operands, straight from the pack
    {
        const uint4 *wp = a.frag + (int64_t)(layer * kTiles + T) * kSetVecs + lane;
        static_for<0, kTaps>([&](auto i_c) __attribute__((always_inline)) {
            constexpr int i = decltype(i_c)::value;
            B[i] = wp[i * 64];
        });
    }
    // ---- the h half: A operand = game r, channels 8g .. 8g + 7 = chunk g, swizzled
    conv_cells<C0, C0 + kBand>(img, r * 4 + (g ^ ((r >> 2) & 3)), B, acc);
    // ---- gates: the lane holds gate kk of games 4g + i; after the transpose it has gates 0..3 of game 4g + kk
    const int kk = r >> 2, cl = r & 3, ch = 4 * T + cl;
    const int64_t n = n0 + 4 * g + kk;
    const bool live = n < a.N;
    float cv[kBand];
    {
        const float *ci = a.c[layer] + (live ? n : a.N - 1) * a.cs[layer] + ch * kHW + C0;
#pragma unroll
        for (int q = 0; q < kBand; ++q) cv[q] = ci[q];
    }
    float *hp = a.h_out[layer] + (n * kC + ch) * kHW + C0;
    float *cp = a.c_out[layer] + (n * kC + ch) * kHW + C0;
    float *gp = a.gates[layer];
    if (gp) gp += (n * 4 * kC + ch) * kHW + C0;
    // three cells at a time: their exchange, gates and stores, so that 12 of the 45 activations are held at once
    static_for<0, kBand / 3>([&](auto k_c) __attribute__((always_inline)) {
        constexpr int q0 = 3 * decltype(k_c)::value;
        float gt[4][3], hn[3], cn[3];
        static_for<0, 3>([&](auto j_c) __attribute__((always_inline)) {
            constexpr int j = decltype(j_c)::value, q = q0 + j;
            float rcv[4];
            rcv[0] = sel4(acc[q], kk);
#pragma unroll
            for (int s = 1; s < 4; ++s)   // from the lane of gate (kk + s) & 3: its value for game 4g + kk
                rcv[s] = __shfl(sel4(acc[q], (kk - s) & 3), (lane & ~12) | (((kk + s) & 3) << 2));
            float z[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int d = (t - kk) & 3;
                z[t] = d == 0 ? rcv[0] : (d == 1 ? rcv[1] : (d == 2 ? rcv[2] : rcv[3]));
            }
            const float si = sigm(z[0]), sf = sigm(z[1]), so = sigm(z[2]), tg = tanhf(z[3]);
            const float fc = sf * cv[q];
            const float ig = si * tg;
            const float cc = fc + ig;
            gt[0][j] = si;
            gt[1][j] = sf;
            gt[2][j] = so;
            gt[3][j] = tg;
            cn[j] = cc;
            hn[j] = so * tanhf(cc);
        });
        if (live) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                hp[q0 + j] = hn[j];
                cp[q0 + j] = cn[j];
            }
            if (gp) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int j = 0; j < 3; ++j) gp[t * kC * kHW + q0 + j] = gt[t][j];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    });
}

__global__ __launch_bounds__(kThreads) void drc_bf16_repeat_kernel(StepArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t img[kImgW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = blockIdx.x % kTiles;
    const int layer = (blockIdx.x / kTiles) % a.L;
    const int64_t n0 = (int64_t)(blockIdx.x / (kTiles * a.L)) * 16;
    // ---- bf16(h_l) of the 16 games into the image; rows past N are zeros
#pragma unroll 3
    for (int idx = tid; idx < 16 * 16 * kQuads; idx += kThreads) {
        const int quad = idx % kQuads, cp = (idx / kQuads) & 15, game = idx / (kQuads * 16);
        const int64_t n = n0 + game;
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        if (n < a.N) {
            const float *hp = a.h[layer] + n * a.hs[layer] + 2 * cp * kHW + 4 * quad;
            lo = *reinterpret_cast<const float4 *>(hp);
            hi = *reinterpret_cast<const float4 *>(hp + kHW);
        }
        img[img_w(4 * quad + 0, game, cp)] = bf16_pair(lo.x, hi.x);
        img[img_w(4 * quad + 1, game, cp)] = bf16_pair(lo.y, hi.y);
        img[img_w(4 * quad + 2, game, cp)] = bf16_pair(lo.z, hi.z);
        img[img_w(4 * quad + 3, game, cp)] = bf16_pair(lo.w, hi.w);
    }
    __syncthreads();
    switch (wave) {
    case 0: band<0>(a, img, n0, layer, T, lane); break;
    case 1: band<kBand>(a, img, n0, layer, T, lane); break;
    case 2: band<2 * kBand>(a, img, n0, layer, T, lane); break;
    default: band<3 * kBand>(a, img, n0, layer, T, lane); break;
    }
}

int status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)e;
}

bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

extern "C" {

int64_t hrl_drc_bf16_pack_bytes(int64_t L) {
    if (L < 1 || L > kMaxLayers) return 0;
    return L * kTiles * kSetVecs * 16;
}

int hrl_drc_bf16_pack(const float *const *weights, int64_t L, int64_t w_cin_total, int64_t w_ci0, void *pack,
                      int64_t pack_bytes, void *stream) {
    if (L < 1 || L > kMaxLayers || !weights || !pack || misaligned(pack) || w_ci0 < 0 ||
        w_cin_total < w_ci0 + kC || w_cin_total > (1 << 20) || pack_bytes < hrl_drc_bf16_pack_bytes(L))
        return HRL_EINVAL;
    PackArgs a{};
    for (int l = 0; l < L; ++l) {
        if (!weights[l]) return HRL_EINVAL;
        a.w[l] = weights[l];
    }
    a.L = (int)L;
    a.cin_total = (int)w_cin_total;
    a.ci0 = (int)w_ci0;
    a.out = static_cast<uint32_t *>(pack);
    const int total = a.L * kTiles * kSetVecs * 4;
    hipLaunchKernelGGL(drc_bf16_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a);
    return status();
}

int hrl_drc_bf16_repeat_forward(const void *pack, int64_t pack_bytes, int64_t L, int64_t H, const float *const *zx,
                                const int64_t *zx_strides, const float *const *h_in, const int64_t *h_strides,
                                const float *const *c_in, const int64_t *c_strides, int64_t N, float *const *h_out,
                                float *const *c_out, float *const *gates, void *stream) {
    if (H != kC || L < 1 || L > kMaxLayers || !pack || misaligned(pack) || pack_bytes < hrl_drc_bf16_pack_bytes(L) ||
        !zx || !zx_strides || !h_in || !h_strides || !c_in || !c_strides || !h_out || !c_out || N < 0 || N > kMaxN)
        return HRL_EINVAL;
    StepArgs a{};
    for (int l = 0; l < L; ++l) {
        if (!zx[l] || !h_in[l] || !c_in[l] || !h_out[l] || !c_out[l] || misaligned(zx[l]) || misaligned(h_in[l]) ||
            misaligned(c_in[l]) || misaligned(h_out[l]) || misaligned(c_out[l]) || (gates && misaligned(gates[l])) ||
            zx_strides[l] < 4 * kC * kHW || h_strides[l] < kC * kHW || c_strides[l] < kC * kHW ||
            zx_strides[l] % 4 != 0 || h_strides[l] % 4 != 0 || c_strides[l] % 4 != 0)
            return HRL_EINVAL;
        a.zx[l] = zx[l];
        a.h[l] = h_in[l];
        a.c[l] = c_in[l];
        a.zxs[l] = zx_strides[l];
        a.hs[l] = h_strides[l];
        a.cs[l] = c_strides[l];
        a.h_out[l] = h_out[l];
        a.c_out[l] = c_out[l];
        a.gates[l] = gates ? gates[l] : nullptr;
    }
    if (N == 0) return HRL_OK;
    a.frag = static_cast<const uint4 *>(pack);
    a.N = N;
    a.L = (int)L;
    const int64_t items = ((N + 15) >> 4) * L * kTiles;
    hipLaunchKernelGGL(drc_bf16_repeat_kernel, dim3((unsigned)items), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return status();
}

}  // extern "C"
