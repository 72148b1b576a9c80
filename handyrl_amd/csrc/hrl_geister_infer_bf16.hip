// hrl_geister_infer_bf16.hip — GeisterNet's complete eval forward as ONE launch with bf16 conv operands and the
// recurrent state h, c in fp32 (gfx950).  The actor's form of hrl_geister_infer.hip: same net, same (16-game tile,
// layer) work items, same gate permutation; a product is ONE v_mfma_f32_16x16x32_bf16 instead of the exact split's six.
//
// Numeric contract (include/hrl_nn.h has the full text): the 3x3 conv weights are rounded fp32 -> bf16 once, at pack
// time; an activation is rounded to bf16 when it is stored as an operand in LDS (the stem's 25 input planes, h_e after
// BN + ReLU, h_l as loaded and after every repeat) and every reader inside the launch reads that copy; accumulation,
// biases, gates (lstm_fwd_kernel's sigm / tanhf), c, BatchNorm as y*alpha + beta, the 1x1 / fc / head_p_set weights
// and the value's tanh are fp32.  c never passes through bf16 and the h_out that reaches memory is the unrounded fp32
// o * tanh(c') of the last repeat.
//
// One workgroup (8 waves, two per SIMD, at most 256 registers each) and one (tile, layer):
//  * LDS holds two bf16 images [cell 36][game 16][32 ch], 64 B per (cell, game), 36,864 B each: E (h_e) and H (the
//    stem's 25-channel input first, then h_l), and 4,608 B for the value / return heads: 78,336 B.  A row's four
//    16-byte chunks are XOR-swizzled by (game >> 2) & 3.  Bank arithmetic of an A-operand read (16 lanes = games
//    r = 0..15, the same chunk k, one ds_read_b128 each): byte r*64 + 16*(k ^ (r >> 2)) lies in 16-byte bank group
//    (4r + (k ^ (r >> 2))) mod 16 = 4*(r & 3) + (k ^ (r >> 2)); (r & 3, r >> 2) -> that is a bijection for a fixed
//    k, so the 16 lanes cover the 16 groups (all 64 banks) once.  Unswizzled, games r and r + 4 would collide (4-way).
//  * a wave owns ONE 16-column tile of the layer's 128 gate channels for the whole item (column j = gate j >> 2 of
//    hidden channel 4T + (j & 3), the pack's permutation), games are the MFMA rows.  Its 36 cells' accumulators are
//    144 registers; the lane's slice of c_l is 36; one half's B fragments are 9 uint4 = 36 (loaded from the pack, L2,
//    per half and repeat); the A operand is double-buffered (8).  The x half is NOT held: 144 more pre-activations do
//    not fit next to 144 accumulators in 256 registers, so a repeat is the K = 64 conv([h_e, h_l]) -- but its x half
//    (which does not depend on h_l) is computed between the two barriers that publish the new h_l, where the waves
//    would otherwise wait for each other, and before the first repeat while h_l is being loaded.
//  * gates: the 4 x 4 lane transpose of the exact form (three ds_bpermute); after it a lane owns game 4g + (r >> 2),
//    hidden channel 4T + (r & 3), all 36 cells.  c_l stays in its registers across the repeats; the new fp32 h_l is
//    rounded into H between two barriers and written to memory once, from registers, in the last repeat.
//  * off-board taps are never computed: 256 MFMAs per half, tile and repeat.
//  * the last layer's workgroup runs the heads from E and H: waves 0..3 the move head's 3x3 conv on the MFMA (9 cells
//    each) + BN + ReLU + the 1x1 conv through lane shuffles, waves 4..7 the value / return 1x1 convs on the VALU,
//    then the two fc and head_p_set.
// Two workgroups per CU would fit the LDS (156,672 of 163,840 B) but need 128 registers per wave, fewer than one tile's
// accumulators: not built.  A row's result depends on nothing but the row.  Bound: the gates' transcendentals (VALU),
// overlapped with the other wave's MFMAs on the same SIMD.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/hrl_nn.h"
#include "../../include/hrl_targets.h"

#ifndef HRL_GEISTER_BF16_WAVES
#define HRL_GEISTER_BF16_WAVES 8   // 4: two column tiles per wave, one wave per SIMD; kept for the record (DESIGN)
#endif

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kBW = 6, kHW = 36, kQuads = 9, kTaps = 9;
constexpr int kC = 32;                 // filters
constexpr int kBoardPlanes = 7, kScalars = 18, kCin = kBoardPlanes + kScalars;
constexpr int kMoves = 144, kSets = 70, kActions = kMoves + kSets;
constexpr int kMaxLayers = 4, kMaxRepeats = 8;
constexpr int kNW = HRL_GEISTER_BF16_WAVES, kThreads = 64 * kNW;
constexpr int kTPW = 8 / kNW;          // column tiles per wave
constexpr int kGridCap = 256;          // one resident workgroup per CU; further (tile, layer) items are walked
constexpr int kCellW = 16 * kC / 2;    // 4-byte words from one cell to the next (16 games x 32 bf16)
constexpr int kImgW = kHW * kCellW;    // words of one image (36,864 B)
static_assert(kNW == 8 || kNW == 4, "8 waves with one column tile each, or 4 with two");

// ---- the pack: fragment sets of 9 x 64 uint4 ([tap][lane], 9,216 B), then floats
constexpr int kSetVecs = kTaps * 64;
__host__ __device__ constexpr int set_stem(int ct) { return ct; }
__host__ __device__ constexpr int set_cell(int l, int half, int t) { return 2 + (l * 2 + half) * 8 + t; }
__host__ __device__ constexpr int set_move(int L, int kc) { return 2 + L * 16 + kc; }
__host__ __device__ constexpr int n_sets(int L) { return 4 + L * 16; }
constexpr int F_BN1A = 0, F_BN1B = 32, F_BNPA = 64, F_BNPB = 80, F_VR = 96 /* av, bv, ar, br */, F_W2 = 112,
              F_WV = 144, F_WR = 208, F_FCV = 272, F_FCR = 308, F_PSW = 344, F_PSB = 414, F_BIAS = 496;
__host__ __device__ constexpr int n_floats(int L) { return F_BIAS + 128 * L; }

// two fp32 -> two bf16, round to nearest even (a in the low half)
__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ uint16_t bf16_one(float a) { return (uint16_t)bf16_pair(a, 0.f); }

struct PackArgs {
    const float *stem_w, *cell_w[kMaxLayers], *cell_b[kMaxLayers];
    const float *bn_w[4], *bn_b[4], *bn_mean[4], *bn_var[4];   // bn1, move head, value, return
    double eps[4];
    const float *move_w1, *move_w2, *value_w, *return_w, *value_fc, *return_fc, *set_w, *set_b;
    int L, pf;
    uint32_t *out;
};

__global__ __launch_bounds__(256) void geister_bf16_pack_kernel(PackArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int nfrag = n_sets(a.L) * kSetVecs * 4;
    if (i < nfrag) {
        // lane l of a set holds bf16(W^T[ci = 8(l>>4) + e][column l&15]), e = 2d, 2d+1 in word d
        const int d = i & 3, l = (i >> 2) & 63;
        const int rest = i >> 8;
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
        a.out[i] = bf16_pair(wv(ci), wv(ci + 1));
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

__device__ __forceinline__ float relu_f(float v) { return v < 0.f ? 0.f : v; }          // NaN stays NaN
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }     // lstm_fwd_kernel's
__device__ __forceinline__ float sel4(const f32x4 &v, int k) {
    return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3]));
}
// word index of channels 2cp, 2cp + 1 of (cell, game) in an image
__device__ __forceinline__ int img_w(int cell, int game, int cp) {
    return cell * kCellW + game * 16 + ((((cp >> 2) ^ ((game >> 2) & 3)) << 2) | (cp & 3));
}
__device__ __forceinline__ void img_put(uint32_t *img, int cell, int game, int ch, float v) {
    reinterpret_cast<uint16_t *>(img)[2 * img_w(cell, game, ch >> 1) + (ch & 1)] = bf16_one(v);
}
__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

__device__ __forceinline__ void load_b(const uint4 *frag, int set, int lane, uint4 (&B)[kTaps]) {
    const uint4 *wp = frag + (int64_t)set * kSetVecs + lane;
    static_for<0, kTaps>([&](auto i_c) __attribute__((always_inline)) {
        constexpr int i = decltype(i_c)::value;
        B[i] = wp[i * 64];
    });
}

__device__ __forceinline__ f32x4 mfma(const uint4 &a, const uint4 &b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                   0, 0);
}

// acc[q - C0] += sum over the real taps of A(img, cell p) . B[tap(p, q)] for the output cells q in [C0, C1); ao: the
// lane's uint4 index of its chunk (channels 8g .. 8g + 7 of game r) within a cell.  The next cell's operand is read
// while this cell's MFMAs issue.
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

template <int NC>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[NC]) {
    static_for<0, NC>([&](auto q_c) __attribute__((always_inline)) {
        acc[decltype(q_c)::value] = (f32x4){0.f, 0.f, 0.f, 0.f};
    });
}

// the stem for output cells [C0, C1) of column tile ct: conv from H (the input image), BN + ReLU, bf16 into E
template <int C0, int C1>
__device__ __forceinline__ void stem_cells(const InferArgs &a, const uint32_t *imgH, uint32_t *imgE, int ct, int lane,
                                           int ao) {
    uint4 B[kTaps];
    f32x4 acc[C1 - C0];
    load_b(a.frag, set_stem(ct), lane, B);
    zero_acc(acc);
    conv_cells<C0, C1>(imgH, ao, B, acc);
    const int r = lane & 15, g = lane >> 4, ch = 16 * ct + r;
    const float al = a.fl[F_BN1A + ch], be = a.fl[F_BN1B + ch];
    static_for<C0, C1>([&](auto q_c) __attribute__((always_inline)) {
        constexpr int q = decltype(q_c)::value;
#pragma unroll
        for (int i = 0; i < 4; ++i) img_put(imgE, q, 4 * g + i, ch, relu_f(acc[q - C0][i] * al + be));
    });
}

// the move head for output cells [C0, C1): 3x3 conv of [E, H] -> BN + ReLU -> 1x1 conv to 4 planes -> policy
template <int C0, int C1>
__device__ __forceinline__ void move_cells(const InferArgs &a, const uint32_t *imgE, const uint32_t *imgH, int64_t n0,
                                           int lane, int ao) {
    uint4 B[kTaps];
    f32x4 acc[C1 - C0];
    zero_acc(acc);
    load_b(a.frag, set_move(a.L, 0), lane, B);
    conv_cells<C0, C1>(imgE, ao, B, acc);
    load_b(a.frag, set_move(a.L, 1), lane, B);
    conv_cells<C0, C1>(imgH, ao, B, acc);
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

__global__ __launch_bounds__(kThreads) void geister_bf16_kernel(InferArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[2 * kImgW + 16 * kHW * 2];
    uint32_t *imgE = smem, *imgH = smem + kImgW;
    float *scr = reinterpret_cast<float *>(smem + 2 * kImgW);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    // A operand: game r, channels 8g .. 8g + 7 = chunk g, swizzled
    const int ao = r * 4 + (g ^ ((r >> 2) & 3));
    // after the gates' transpose: game 4g + kk, hidden channel 4T + cl
    const int kk = r >> 2, cl = r & 3, gm = 4 * g + kk;
    const int64_t ntiles = (a.N + 15) >> 4, nitems = ntiles * a.L;
    const int64_t srow = (int64_t)a.L * kC * kHW;   // floats of one row of the stacked state

    for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int64_t n0 = (item / a.L) * 16;
        const int layer = (int)(item % a.L);
        // ---- the stem's input into H: channels 0..17 the scalars (constant over the board), 18..24 the board
        for (int idx = tid; idx < 16 * 16 * kQuads; idx += kThreads) {
            const int quad = idx % kQuads, cp = (idx / kQuads) & 15, game = idx / (kQuads * 16);
            const int64_t n = n0 + game;
            auto plane = [&](int ch) -> float4 {
                if (n >= a.N || ch >= kCin) return make_float4(0.f, 0.f, 0.f, 0.f);
                if (ch < kScalars) {
                    const float s = a.scalar[n * kScalars + ch];
                    return make_float4(s, s, s, s);
                }
                return *reinterpret_cast<const float4 *>(a.board + (n * kBoardPlanes + ch - kScalars) * kHW + 4 * quad);
            };
            const float4 lo = plane(2 * cp), hi = plane(2 * cp + 1);
            imgH[img_w(4 * quad + 0, game, cp)] = bf16_pair(lo.x, hi.x);
            imgH[img_w(4 * quad + 1, game, cp)] = bf16_pair(lo.y, hi.y);
            imgH[img_w(4 * quad + 2, game, cp)] = bf16_pair(lo.z, hi.z);
            imgH[img_w(4 * quad + 3, game, cp)] = bf16_pair(lo.w, hi.w);
        }
        __syncthreads();
        {   // ---- stem: column tile wave & 1, a band of the cells per wave pair
            const int ct = wave & 1, band = wave >> 1;
            if constexpr (kNW == 4) {
                if (band == 0) stem_cells<0, 18>(a, imgH, imgE, ct, lane, ao);
                else stem_cells<18, 36>(a, imgH, imgE, ct, lane, ao);
            } else {
                switch (band) {
                case 0: stem_cells<0, 9>(a, imgH, imgE, ct, lane, ao); break;
                case 1: stem_cells<9, 18>(a, imgH, imgE, ct, lane, ao); break;
                case 2: stem_cells<18, 27>(a, imgH, imgE, ct, lane, ao); break;
                default: stem_cells<27, 36>(a, imgH, imgE, ct, lane, ao); break;
                }
            }
        }
        __syncthreads();
        // ---- the layer's state: bf16(h_l) into H, the lane's slice of c_l into registers
        for (int idx = tid; idx < 16 * 16 * kQuads; idx += kThreads) {
            const int quad = idx % kQuads, cp = (idx / kQuads) & 15, game = idx / (kQuads * 16);
            const int64_t n = n0 + game;
            float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
            if (n < a.N) {
                const float *hp = a.h + n * srow + (layer * kC + 2 * cp) * kHW + 4 * quad;
                lo = *reinterpret_cast<const float4 *>(hp);
                hi = *reinterpret_cast<const float4 *>(hp + kHW);
            }
            imgH[img_w(4 * quad + 0, game, cp)] = bf16_pair(lo.x, hi.x);
            imgH[img_w(4 * quad + 1, game, cp)] = bf16_pair(lo.y, hi.y);
            imgH[img_w(4 * quad + 2, game, cp)] = bf16_pair(lo.z, hi.z);
            imgH[img_w(4 * quad + 3, game, cp)] = bf16_pair(lo.w, hi.w);
        }
        const int64_t nl = n0 + gm;   // the lane's game
        float cst[kTPW][kHW], bias[kTPW][4];
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
        // ---- the x half of the first repeat (E is complete since the barrier above), then the repeats
        f32x4 acc[kTPW][kHW];
        auto conv_x = [&]() __attribute__((always_inline)) {
            static_for<0, kTPW>([&](auto tt_c) __attribute__((always_inline)) {
                constexpr int tt = decltype(tt_c)::value;
                uint4 B[kTaps];
                load_b(a.frag, set_cell(layer, 0, wave * kTPW + tt), lane, B);
                zero_acc(acc[tt]);
                conv_cells<0, kHW>(imgE, ao, B, acc[tt]);
            });
        };
        conv_x();
        __syncthreads();
        for (int rep = 0; rep < a.repeats; ++rep) {
            float hn[kTPW][kHW];
            static_for<0, kTPW>([&](auto tt_c) __attribute__((always_inline)) {
                constexpr int tt = decltype(tt_c)::value;
                {
                    uint4 B[kTaps];
                    load_b(a.frag, set_cell(layer, 1, wave * kTPW + tt), lane, B);
                    conv_cells<0, kHW>(imgH, ao, B, acc[tt]);
                }
                // gates: the lane holds gate kk of games 4g + i; it takes gates 0..3 of game 4g + kk
                static_for<0, kHW>([&](auto q_c) __attribute__((always_inline)) {
                    constexpr int q = decltype(q_c)::value;
                    float rcv[4];
                    rcv[0] = sel4(acc[tt][q], kk);
#pragma unroll
                    for (int s = 1; s < 4; ++s)   // from the lane of gate (kk + s) & 3: its value for game 4g + kk
                        rcv[s] = __shfl(sel4(acc[tt][q], (kk - s) & 3), (lane & ~12) | (((kk + s) & 3) << 2));
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
                    img_put(imgH, q, gm, ch, hn[tt][q]);
                });
            });
            if (rep + 1 < a.repeats) {
                conv_x();   // the next repeat's x half, while the other waves publish their h_l
            } else if (nl < a.N) {
                // the advanced state, unrounded (each workgroup reads and writes only its own (tile, layer) slice,
                // and read all of it before the first repeat: in place is safe)
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
            __syncthreads();
        }
        // ---- the heads, from E = bf16(h_e) and H = bf16(h_last)
        if (layer == a.L - 1) {
            switch (wave) {
            case 0: move_cells<0, 9>(a, imgE, imgH, n0, lane, ao); break;
            case 1: move_cells<9, 18>(a, imgE, imgH, n0, lane, ao); break;
            case 2: move_cells<18, 27>(a, imgE, imgH, n0, lane, ao); break;
            case 3: move_cells<27, 36>(a, imgE, imgH, n0, lane, ao); break;
            default: break;
            }
            // value / return: 1x1 conv 64 -> 1 each (channels in order), BN + ReLU; a thread per (game, cell), on the
            // waves the move head leaves idle (all of them at 4 waves)
            constexpr int vr0 = kNW == 8 ? 256 : 0;
            for (int it = tid - vr0; it >= 0 && it < 16 * kHW; it += kThreads - vr0) {
                const int game = it & 15, cell = it >> 4;
                const int s = (game >> 2) & 3;
                float sv = 0.f, sr = 0.f;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const uint4 *row = reinterpret_cast<const uint4 *>(half ? imgH : imgE) + cell * (kCellW / 4) + game * 4;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint4 x = row[k ^ s];
                        const float xs[8] = {bf_lo(x.x), bf_hi(x.x), bf_lo(x.y), bf_hi(x.y),
                                             bf_lo(x.z), bf_hi(x.z), bf_lo(x.w), bf_hi(x.w)};
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            sv = sv + a.fl[F_WV + half * kC + 8 * k + e] * xs[e];
                            sr = sr + a.fl[F_WR + half * kC + 8 * k + e] * xs[e];
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

int64_t hrl_geister_infer_bf16_pack_bytes(int64_t layers, int64_t p_filters) {
    if (!shape_ok(layers, p_filters)) return 0;
    return (int64_t)n_sets((int)layers) * kSetVecs * 16 + (int64_t)n_floats((int)layers) * 4;
}

int hrl_geister_infer_bf16_pack(const float *stem_w, const float *const *cell_w, const float *const *cell_b,
                                int64_t layers, const float *const *bn_w, const float *const *bn_b,
                                const float *const *bn_mean, const float *const *bn_var, const double *bn_eps,
                                const float *move_w1, const float *move_w2, int64_t p_filters, const float *value_w,
                                const float *return_w, const float *value_fc, const float *return_fc,
                                const float *set_w, const float *set_b, void *pack, void *stream) {
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
    hipLaunchKernelGGL(geister_bf16_pack_kernel, dim3((total + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return status();
}

int hrl_geister_infer_bf16(const void *pack, int64_t layers, int64_t num_repeats, int64_t p_filters,
                           const float *board, const float *scalar, const float *h, const float *c, int64_t N,
                           float *policy, float *value, float *ret, float *h_out, float *c_out, void *stream) {
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
    hipLaunchKernelGGL(geister_bf16_kernel, dim3((unsigned)(items < kGridCap ? items : kGridCap)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return status();
}

}  // extern "C"
