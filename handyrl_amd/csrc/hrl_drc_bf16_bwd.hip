// hrl_drc_bf16_bwd.hip — the whole backward of nn._DRCStep at one time step as ONE launch (gfx950): for every live
// layer, the R repeats' gate backward and h-half adjoint conv, with dh and dc kept on chip between the repeats
// (train_args precision: bf16_drc_bwd).  It replaces, per live layer and repeat, hrl_lstm_gates_backward_ex and the
// K-split exact adjoint (hrl_gboard_forward_groups with S = 4 partial input gradients in HBM), and the trailing sum.
//
// Numeric contract (include/hrl_nn.h has the full text): the gate backward is lstm_bwd_ex_kernel's float operations;
// dz_r goes to HBM as fp32, unrounded; dzx = dz_{R-1} + ... + dz_0 in that order; the adjoint's operands are
// bf16(dz_r) (rounded as it is staged into LDS) and bf16(W_h) (rounded at pack time) on v_mfma_f32_16x16x32_bf16,
// fp32 accumulation from zero, taps 0..8 in order and the gate chunks i, f, o, g within a tap; dc never sees bf16.
//
// Work item = (4 games, live layer), one workgroup of 4 waves that walks the R repeats.
//  * gate phase: 1152 float4 items (game, channel, 4 cells), 4.5 per thread, the same items every repeat, so a
//    thread's dc (20 registers) and its share of dzx (80) never leave it.  Lanes 2j, 2j + 1 hold the channels 2cp,
//    2cp + 1 of the same cells: they swap two cells each by DPP and write whole bf16 pairs into the image.
//  * LDS: the bf16 dz image [row = game * 36 + cell][128 gate columns], 256 B per row, 36,864 B, its sixteen 16-byte
//    chunks XOR-swizzled by row & 15 (sixteen consecutive rows of one chunk cover the banks once: an A operand is one
//    ds_read_b128); one row of zeros that the off-board taps read instead of branching (256 B); the fp32 hand-over
//    tile dh [channel 32][row 144, padded to 148] (18,944 B) through which the accumulators reach the gate lanes of
//    the next repeat (and dh_in after the last).  56,064 B in all.
//  * adjoint phase: the MFMA rows are the 144 (game, cell) pairs = nine 16-row tiles, the columns the 32 dh channels
//    = two 16-column tiles, K = 9 taps x 128.  Wave w owns column tile w & 1 and the row tiles of parity w >> 1 (5 or
//    4).  The taps are a loop: per tap a wave loads its column tile's four B fragments straight from the pack (L2), one
//    tap ahead, and runs its row tiles' independent accumulator chains side by side.  (All 36 fragments kept in
//    registers for the R repeats, with every tap's LDS addresses, spilled 1,360 B per lane.)  180 or 144 MFMAs per
//    wave and repeat, 648 per item.
//  * two barriers per repeat: image written -> adjoint, hand-over tile written -> next gate phase.
// A row's result depends on nothing but the row.  Deterministic, no atomics, no workspace.

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
constexpr int kC = 32;                       // hidden channels = the adjoint's output columns
constexpr int kK = 4 * kC;                   // gate columns = K of one tap
constexpr int kKSteps = kK / 32;             // MFMA k-steps per tap (one per gate chunk)
constexpr int kMaxLayers = 4, kMaxRepeats = 8;
constexpr int kG = 4;                        // games per work item
constexpr int kRows = kG * kHW;              // 144 MFMA rows
constexpr int kRowTiles = kRows / 16;        // 9
constexpr int kThreads = 256;
constexpr int kRowW = kK / 2;                // 4-byte words per image row (64)
constexpr int kImgW = kRows * kRowW;         // words of the image; the row of zeros follows it
constexpr int kTS = kRows + 4;               // floats from one channel to the next in the hand-over tile
constexpr int kItems = kG * kC * kQuads;     // float4 items of the gate phase (1152)
constexpr int kIters = (kItems + kThreads - 1) / kThreads;   // 5, the last one half full (waves 0 and 1)
constexpr int kLayerVecs = kTaps * kKSteps * 2 * 64;         // uint4 of one layer's fragments (73,728 B)
constexpr int64_t kMaxN = (int64_t)1 << 24;

__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {   // round to nearest even, a in the low half
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

struct PackArgs {
    const float *w[kMaxLayers];
    int L, cin_total, ci0;
    uint32_t *out;
};

// [layer][tap 9][k-step 4][column tile 2][lane 64][8 bf16]: lane l of (tap, ks, ct) holds
// bf16(W[32 ks + 8 (l >> 4) + e][ci0 + 16 ct + (l & 15)][tap]), e = 2d, 2d + 1 in word d.  The tap is the forward's;
// the kernel reads the dz cell at the mirrored offset.
__global__ __launch_bounds__(256) void drc_bf16_adjoint_pack_kernel(PackArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.L * kLayerVecs * 4) return;
    const int d = i & 3, l = (i >> 2) & 63, ct = (i >> 8) & 1, ks = (i >> 9) & 3;
    const int rest = i >> 11;
    const int tap = rest % kTaps, layer = rest / kTaps;
    const int k = 32 * ks + 8 * (l >> 4) + 2 * d, ci = 16 * ct + (l & 15);
    const int64_t kstride = (int64_t)a.cin_total * kTaps;
    const float *w = a.w[layer] + k * kstride + (a.ci0 + ci) * kTaps + tap;
    a.out[i] = bf16_pair(w[0], w[kstride]);
}

struct BwdArgs {
    const uint4 *frag;
    const float *gates[kMaxLayers][kMaxRepeats], *c[kMaxLayers][kMaxRepeats], *c_out[kMaxLayers][kMaxRepeats];
    float *dz[kMaxLayers][kMaxRepeats];
    const float *gh[kMaxLayers], *gc[kMaxLayers];
    int64_t ghs[kMaxLayers], gcs[kMaxLayers];
    float *dzx[kMaxLayers], *dh_in[kMaxLayers], *dc_in[kMaxLayers];
    int pack_layer[kMaxLayers];
    int64_t N;
    int L, R;
};

template <int I> using IC = std::integral_constant<int, I>;
template <int I, int N, int S = 1, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(IC<I>{});
        static_for<I + S, N, S>(f);
    }
}

__device__ __forceinline__ f32x4 mfma(const uint4 &a, const uint4 &b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                   0, 0);
}

__device__ __forceinline__ float from_neighbour(float v) {   // the value of lane ^ 1 (DPP quad_perm [1, 0, 3, 2])
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}

// word index of gate columns 2kp, 2kp + 1 of an image row
__device__ __forceinline__ int img_w(int row, int kp) {
    return row * kRowW + ((((kp >> 2) ^ (row & 15)) << 2) | (kp & 3));
}

// the adjoint of one repeat for the wave's column tile and the row tiles PAR, PAR + 2, ...:
// dh[row][16 ct + j] = sum over taps, gate columns of img[row mirrored by the tap][k] * B[tap][k][j].
// The taps are a real loop (its addresses are computed per tap, not kept for every tap at once); the next tap's four
// B fragments are loaded from the pack (L2) while this tap's MFMAs issue, the row tiles' chains interleaved.
template <int PAR>
__device__ __forceinline__ void adjoint(const uint32_t *img, float *tile, const uint4 *bp, int ct, int lane) {
    constexpr int NT = (kRowTiles - PAR + 1) / 2;
    const int r = lane & 15, g = lane >> 4;
    const int zero_w = kImgW + (r << 2);
    f32x4 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint4 Bc[kKSteps], Bn[kKSteps];
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) Bc[ks] = bp[ks * 128];
#pragma unroll 1
    for (int tap = 0; tap < kTaps; ++tap) {
        const int nt = tap + 1 < kTaps ? tap + 1 : tap;
#pragma unroll
        for (int ks = 0; ks < kKSteps; ++ks) Bn[ks] = bp[(nt * kKSteps + ks) * 128];
        const int oy = 1 - tap / 3, ox = 1 - tap % 3;
        static_for<0, NT>([&](auto i_c) __attribute__((always_inline)) {
            constexpr int i = decltype(i_c)::value;
            const int row = (PAR + 2 * i) * 16 + r;
            const int cell = row % kHW, y = cell / kBW, x = cell % kBW;
            const bool on = (unsigned)(y + oy) < (unsigned)kBW && (unsigned)(x + ox) < (unsigned)kBW;
            const int src = row + oy * kBW + ox;
#pragma unroll
            for (int ks = 0; ks < kKSteps; ++ks) {
                const int w = on ? src * kRowW + (((4 * ks + g) ^ (src & 15)) << 2) : zero_w;
                acc[i] = mfma(*reinterpret_cast<const uint4 *>(img + w), Bc[ks], acc[i]);
            }
        });
#pragma unroll
        for (int ks = 0; ks < kKSteps; ++ks) Bc[ks] = Bn[ks];
    }
    // lane: column r, rows 4g .. 4g + 3 of each tile
#pragma unroll
    for (int i = 0; i < NT; ++i)
        *reinterpret_cast<f32x4 *>(tile + (16 * ct + r) * kTS + (PAR + 2 * i) * 16 + 4 * g) = acc[i];
}

__global__ __launch_bounds__(kThreads) void drc_bf16_step_bwd_kernel(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t img[kImgW + kRowW];
    __shared__ __attribute__((aligned(16))) float tile[kC * kTS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int layer = blockIdx.x % a.L;
    const int64_t n0 = (int64_t)(blockIdx.x / a.L) * kG;
    const int R = a.R;
    const bool want_dh = a.dh_in[layer] != nullptr;
    if (tid < kRowW) img[kImgW + tid] = 0u;
    const int ct = wave & 1;
    const uint4 *bp = a.frag + (int64_t)a.pack_layer[layer] * kLayerVecs + ct * 64 + lane;   // the wave's columns
    // the thread's items: idx = tid + 256 it -> lanes 2j, 2j + 1 are channels 2cp, 2cp + 1 of (game, quad)
    const int odd = tid & 1;
    f32x4 dcr[kIters], zxa[kIters][4];
    for (int r = R - 1; r >= 0; --r) {
        const bool first = r == R - 1;
        const float *gates = a.gates[layer][r], *cin = a.c[layer][r], *cout = a.c_out[layer][r];
        float *dz = a.dz[layer][r];
        static_for<0, kIters>([&](auto it_c) __attribute__((always_inline)) {
            constexpr int it = decltype(it_c)::value;
            const int idx = tid + kThreads * it;
            if (it < kIters - 1 || idx < kItems) {   // wave-uniform: the last iteration is waves 0 and 1
                const int slot = idx >> 1;
                const int quad = slot % kQuads, cp = (slot / kQuads) % (kC / 2), game = slot / (kQuads * kC / 2);
                const int ch = 2 * cp + odd;
                const int64_t n = n0 + game;
                const bool live = n < a.N;
                const int64_t nn = live ? n : a.N - 1;   // a row past N reads row N - 1 and stores nothing
                const int in_row = ch * kHW + 4 * quad;
                const int64_t zoff = nn * (kK * kHW) + in_row, soff = nn * (kC * kHW) + in_row;
                const f32x4 gi = *reinterpret_cast<const f32x4 *>(gates + zoff);
                const f32x4 gf = *reinterpret_cast<const f32x4 *>(gates + zoff + kC * kHW);
                const f32x4 go = *reinterpret_cast<const f32x4 *>(gates + zoff + 2 * kC * kHW);
                const f32x4 gg = *reinterpret_cast<const f32x4 *>(gates + zoff + 3 * kC * kHW);
                const f32x4 cv = *reinterpret_cast<const f32x4 *>(cin + soff);
                const f32x4 cn = *reinterpret_cast<const f32x4 *>(cout + soff);
                f32x4 dhv = {0.f, 0.f, 0.f, 0.f}, dcv = dhv;
                if (first) {
                    if (a.gh[layer]) dhv = *reinterpret_cast<const f32x4 *>(a.gh[layer] + nn * a.ghs[layer] + in_row);
                    if (a.gc[layer]) dcv = *reinterpret_cast<const f32x4 *>(a.gc[layer] + nn * a.gcs[layer] + in_row);
                } else {
                    dhv = *reinterpret_cast<const f32x4 *>(tile + ch * kTS + game * kHW + 4 * quad);
                    dcv = dcr[it];
                }
                f32x4 d4[4], dprev;
#pragma unroll
                for (int j = 0; j < 4; ++j) {   // lstm_bwd_ex_kernel's operations
                    const float si = gi[j], sf = gf[j], so = go[j], tg = gg[j];
                    const float tc = tanhf(cn[j]);
                    const float d_h = dhv[j], d_c = dcv[j];
                    const float dct = d_c + d_h * so * (1.f - tc * tc);
                    d4[0][j] = dct * tg * (si * (1.f - si));
                    d4[1][j] = dct * cv[j] * (sf * (1.f - sf));
                    d4[2][j] = d_h * tc * (so * (1.f - so));
                    d4[3][j] = dct * si * (1.f - tg * tg);
                    dprev[j] = dct * sf;
                }
                dcr[it] = dprev;
                if (live) {
                    float *zp = dz + n * (kK * kHW) + in_row;
#pragma unroll
                    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4 *>(zp + t * kC * kHW) = d4[t];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) zxa[it][t] = first ? d4[t] : zxa[it][t] + d4[t];
                // bf16(dz) into the image: the even lane writes cells 0, 1 of the quad, the odd lane cells 2, 3
                const int row0 = game * kHW + 4 * quad + 2 * odd;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f32x4 v = d4[t];
                    const float r0 = from_neighbour(odd ? v[0] : v[2]), r1 = from_neighbour(odd ? v[1] : v[3]);
                    img[img_w(row0, t * (kC / 2) + cp)] = odd ? bf16_pair(r0, v[2]) : bf16_pair(v[0], r0);
                    img[img_w(row0 + 1, t * (kC / 2) + cp)] = odd ? bf16_pair(r1, v[3]) : bf16_pair(v[1], r1);
                }
            }
        });
        __syncthreads();
        if (r > 0 || want_dh) {
            if (wave < 2) adjoint<0>(img, tile, bp, ct, lane);
            else adjoint<1>(img, tile, bp, ct, lane);
        }
        __syncthreads();
    }
    // ---- after repeat 0: dzx, dc_in and (from the hand-over tile) dh_in
    static_for<0, kIters>([&](auto it_c) __attribute__((always_inline)) {
        constexpr int it = decltype(it_c)::value;
        const int idx = tid + kThreads * it;
        if (it < kIters - 1 || idx < kItems) {
            const int slot = idx >> 1;
            const int quad = slot % kQuads, cp = (slot / kQuads) % (kC / 2), game = slot / (kQuads * kC / 2);
            const int ch = 2 * cp + odd;
            const int64_t n = n0 + game;
            if (n < a.N) {
                const int in_row = ch * kHW + 4 * quad;
                if (float *p = a.dzx[layer]) {
                    p += n * (kK * kHW) + in_row;
#pragma unroll
                    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4 *>(p + t * kC * kHW) = zxa[it][t];
                }
                if (float *p = a.dc_in[layer]) *reinterpret_cast<f32x4 *>(p + n * (kC * kHW) + in_row) = dcr[it];
                if (want_dh)
                    *reinterpret_cast<f32x4 *>(a.dh_in[layer] + n * (kC * kHW) + in_row) =
                        *reinterpret_cast<const f32x4 *>(tile + ch * kTS + game * kHW + 4 * quad);
            }
        }
    });
}

int status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)e;
}

bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
bool bad(const void *p) { return !p || misaligned(p); }

}  // namespace

extern "C" {

int64_t hrl_drc_bf16_adjoint_pack_bytes(int64_t L) {
    if (L < 1 || L > kMaxLayers) return 0;
    return L * kLayerVecs * 16;
}

int hrl_drc_bf16_adjoint_pack(const float *const *weights, int64_t L, int64_t w_cin_total, int64_t w_ci0, void *pack,
                              int64_t pack_bytes, void *stream) {
    if (L < 1 || L > kMaxLayers || !weights || bad(pack) || w_ci0 < 0 || w_cin_total < w_ci0 + kC ||
        w_cin_total > (1 << 20) || pack_bytes < hrl_drc_bf16_adjoint_pack_bytes(L))
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
    const int total = a.L * kLayerVecs * 4;
    hipLaunchKernelGGL(drc_bf16_adjoint_pack_kernel, dim3((total + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return status();
}

int hrl_drc_bf16_step_backward(const void *pack, int64_t pack_bytes, const int64_t *pack_layer, int64_t L_live,
                               int64_t R, int64_t H, const float *const *gates, const float *const *c,
                               const float *const *c_out, const float *const *gh, const int64_t *gh_strides,
                               const float *const *gc, const int64_t *gc_strides, int64_t N, float *const *dz,
                               float *const *dzx, float *const *dh_in, float *const *dc_in, void *stream) {
    if (H != kC || L_live < 1 || L_live > kMaxLayers || R < 1 || R > kMaxRepeats || bad(pack) || !pack_layer ||
        !gates || !c || !c_out || !gh || !gh_strides || !gc || !gc_strides || !dz || !dzx || !dh_in || !dc_in ||
        N < 0 || N > kMaxN)
        return HRL_EINVAL;
    BwdArgs a{};
    for (int l = 0; l < L_live; ++l) {
        if (pack_layer[l] < 0 || pack_layer[l] >= kMaxLayers ||
            pack_bytes < hrl_drc_bf16_adjoint_pack_bytes(pack_layer[l] + 1))
            return HRL_EINVAL;
        for (int r = 0; r < R; ++r) {
            const int64_t i = l * R + r;
            if (bad(gates[i]) || bad(c[i]) || bad(c_out[i]) || bad(dz[i])) return HRL_EINVAL;
            a.gates[l][r] = gates[i];
            a.c[l][r] = c[i];
            a.c_out[l][r] = c_out[i];
            a.dz[l][r] = dz[i];
        }
        if (misaligned(gh[l]) || misaligned(gc[l]) || misaligned(dzx[l]) || misaligned(dh_in[l]) ||
            misaligned(dc_in[l]) || (gh[l] && (gh_strides[l] < kC * kHW || gh_strides[l] % 4 != 0)) ||
            (gc[l] && (gc_strides[l] < kC * kHW || gc_strides[l] % 4 != 0)))
            return HRL_EINVAL;
        a.pack_layer[l] = (int)pack_layer[l];
        a.gh[l] = gh[l];
        a.gc[l] = gc[l];
        a.ghs[l] = gh[l] ? gh_strides[l] : 0;
        a.gcs[l] = gc[l] ? gc_strides[l] : 0;
        a.dzx[l] = dzx[l];
        a.dh_in[l] = dh_in[l];
        a.dc_in[l] = dc_in[l];
    }
    if (N == 0) return HRL_OK;
    a.frag = static_cast<const uint4 *>(pack);
    a.N = N;
    a.L = (int)L_live;
    a.R = (int)R;
    const int64_t items = ((N + kG - 1) / kG) * L_live;
    hipLaunchKernelGGL(drc_bf16_step_bwd_kernel, dim3((unsigned)items), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return status();
}

}  // extern "C"
