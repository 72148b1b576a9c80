// hrl_geesenet_bf16.hip — GeeseNet's eval forward with bf16 conv operands, ONE launch per forward (gfx950).
//
// The actor's form of hrl_geesenet.hip's tower (same net, same fold): the conv weights are rounded once to bf16
// (round to nearest even) and every conv reads bf16(h); everything else -- the MFMA's accumulation, alpha, beta,
// the conv bias, the residual stream h, the pool and both heads -- is fp32, in the tower's operation order
// h' = relu([h +] (acc + bias) * alpha + beta).  A product is one v_mfma_f32_16x16x32_bf16 instead of the exact
// split's six, a sample's conv input is 80 * 32 * 2 = 5,120 B and a unit's operands 18,432 B, so a wave keeps its
// sample on chip through the whole net while its workgroup streams the weights.
//
// geese_bf16_pack_kernel (once per inference session), per unit 18,816 B:
//   [tap 9][co-tile 2][lane 64][8 bf16]  the MFMA's row operand as the lane reads it (one 16-byte read):
//                                        W[co = 16 ct + (l & 15)][ci = 8 (l >> 4) + e][tap], the stem's ci >= 17 zero
//   [alpha 32 | beta 32 | bias 32] fp32  hrl_geesenet.hip's (bn_eval_coef_kernel's) coefficients, formed the same way
//   then [head_p (4, 32) | head_v (1, 64)] fp32 after the last unit.
// geese_bf16_kernel: one wave owns one sample for the whole forward; the 8 waves of a workgroup walk the units in
//   lock step and share each unit's weights.  LDS (81,920 B, two workgroups per CU):
//     8 images [cell 80][32 ch] bf16, 64 B per cell, the four 16-byte channel groups swizzled by (cell >> 2) & 3
//       (hrl_geesenet.hip's ps_row on a 16-dword row) so that the 16 cells a tap gathers spread over all banks;
//     2 weight slots of 18,816 B; the heads, 768 B; x[:, 0] of each wave's sample, 8 x 320 B.
//   Operand roles: weights are the rows, cells the columns, so lane l's accumulators of (cell tile mt, co-tile ct)
//   are channels 16 ct + 4 (l >> 4) + 0..3 of cell 16 mt + (l & 15): the next image takes one 8-byte store per quad,
//   and the fp32 residual h lives in 40 registers of that same layout and never leaves them.  A tap is 2 weight
//   reads and 5 gathers (one ds_read_b128 each) for 10 MFMAs.
//   Weights: unit u + 1 goes from global memory through registers to the other slot in three chunks, each loaded
//   before three taps' MFMAs and written after them (4 staging registers next to the 80 of acc and h), and ONE
//   __syncthreads per unit publishes it: a slot is rewritten only by waves that passed the barrier which every wave
//   reaches after its last read of that slot.
//   Every barrier and every staging step is executed by every wave of the workgroup, for every pass the workgroup
//   makes; a wave without a sample (n >= N) skips only its own loads, MFMAs and stores.  Nothing is shared or
//   awaited between workgroups.
//   Tail: in-lane pool sums over the lane's 5 cells (x[:, 0] kept from the stem's load), the head products per
//   lane, then a butterfly of 6 values over each half of the wave and two readlanes.  A row's HBM traffic is x in
//   and 5 floats out.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrl_nn.h"
#include "../../include/hrl_targets.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kCo = 32;
constexpr int kStemC = 17;
constexpr int kActions = 4;
constexpr int kMT = 5;                    // 16-cell tiles: boards of at most 80 cells
constexpr int kMaxCells = kMT * 16;
constexpr int kTaps = 9;
constexpr int kMaxLayers = 16;
constexpr int kMaxUnits = kMaxLayers + 1;

constexpr int kNW = 8;                    // waves (samples) per workgroup
constexpr int kThreads = 64 * kNW;
constexpr int kGridCap = 512;             // two workgroups per CU: kGridCap * kNW = 4096 samples per pass

// the pack, in 4-byte words
constexpr int kWWords = kTaps * 2 * 64 * 4;            // 4608: the bf16 row operands
constexpr int kUnitWords = kWWords + 3 * kCo;          // + alpha | beta | bias (18,816 B)
constexpr int kHeadWords = kActions * kCo + 2 * kCo;   // head_p | head_v
constexpr int kUnitVec = kUnitWords / 4;               // 1176 uint4
constexpr int kChunk = kUnitVec / 3;                   // 392: a third of a unit, one uint4 per staging thread
constexpr int kImgWords = kMaxCells * 16;              // 5,120 B per wave
constexpr int kNbWords = (kMT * 6 + 3) / 4;            // the neighbour table, a byte per field
static_assert(kUnitWords % 4 == 0 && kHeadWords % 4 == 0, "units and the pack end on 16-byte lines");
static_assert(3 * kChunk == kUnitVec && kChunk <= kThreads, "three chunks cover a unit");
static_assert(2 * (kNW * (kImgWords + kMaxCells) + 2 * kUnitWords + kHeadWords) * 4 <= 160 * 1024, "two workgroups per CU");

// two fp32 -> two bf16, round to nearest even (a in the low half)
__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

__device__ __forceinline__ void lds_fence() {
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS operations done
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int opaque(int i) {
    asm volatile("" : "+v"(i));
    return i;
}

template <int M>
__device__ __forceinline__ float swz_xor(float v) {   // lane l gets lane l ^ M's value (M < 32)
    return __uint_as_float(__builtin_amdgcn_ds_swizzle(__float_as_uint(v), (M << 10) | 0x1f));
}

__device__ __forceinline__ float relu(float v) { return v < 0.f ? 0.f : v; }   // NaN stays NaN

// dword of channel group g (8 channels, 16 B) of a cell's image row
__device__ __forceinline__ int img_row(int cell, int g) { return cell * 16 + 4 * (g ^ ((cell >> 2) & 3)); }

// ------------------------------------------------------------------ pack
struct PackArgs {
    const float *conv_w[kMaxUnits], *conv_b[kMaxUnits], *bn_w[kMaxUnits], *bn_b[kMaxUnits], *bn_mean[kMaxUnits],
        *bn_var[kMaxUnits];
    double eps[kMaxUnits];
    const float *head_p, *head_v;
    int units;
    uint32_t *out;
};

__global__ __launch_bounds__(256) void geese_bf16_pack_kernel(PackArgs a) {
    const int total = a.units * kUnitWords + kHeadWords;
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= total) return;
    const int u = w / kUnitWords, i = w - u * kUnitWords;
    uint32_t v;
    if (u >= a.units) {
        v = __float_as_uint(i < kActions * kCo ? a.head_p[i] : a.head_v[i - kActions * kCo]);
    } else if (i < kWWords) {
        const int cin = u == 0 ? kStemC : kCo;
        const int d = i & 3, l = (i >> 2) & 63, ct = (i >> 8) & 1, tap = i >> 9;
        const int oc = ct * 16 + (l & 15), ic = 8 * (l >> 4) + 2 * d;
        const float w0 = ic < cin ? a.conv_w[u][(oc * cin + ic) * kTaps + tap] : 0.f;
        const float w1 = ic + 1 < cin ? a.conv_w[u][(oc * cin + ic + 1) * kTaps + tap] : 0.f;
        v = bf16_pair(w0, w1);
    } else {
        // geese_infer_pack_kernel's (bn_eval_coef_kernel's) operations
        const int j = i - kWWords, c = j & (kCo - 1);
        const float invstd = (float)(1.0 / sqrt((double)a.bn_var[u][c] + a.eps[u]));
        const float al = invstd * a.bn_w[u][c];
        const float be = a.bn_b[u][c] - a.bn_mean[u][c] * al;
        v = __float_as_uint(j < kCo ? al : (j < 2 * kCo ? be : a.conv_b[u][c]));
    }
    a.out[w] = v;
}

// ------------------------------------------------------------------ the forward
struct InferArgs {
    const uint32_t *pack;
    const float *x;          // (N, 17, HW)
    float *policy, *value;   // (N, 4), (N, 1)
    int64_t N;
    int units, H, W;
};

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void geese_bf16_kernel(InferArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t w_lds[2][kUnitWords];
    __shared__ __attribute__((aligned(16))) uint32_t imgs[kNW * kImgWords];
    __shared__ __attribute__((aligned(16))) float heads_s[kHeadWords];
    __shared__ float x0_s[kNW * kMaxCells];   // x[:, 0] of each wave's sample, kept from the stem's load for the pool
    const int64_t N = a.N;
    const int H = a.H, W = a.W, units = a.units;
    const int HW = H * W;
    const int lane0 = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: so are n, active and the image's base
    uint32_t *img = imgs + wave * kImgWords;

    // the first unit's weights and the heads; published by the barrier below
    const uint4 *pack4 = reinterpret_cast<const uint4 *>(a.pack);
    for (int i = threadIdx.x; i < kUnitVec; i += kThreads) reinterpret_cast<uint4 *>(w_lds[0])[i] = pack4[i];
    for (int i = threadIdx.x; i < kHeadWords; i += kThreads)
        heads_s[i] = __uint_as_float(a.pack[(int64_t)units * kUnitWords + i]);

    // the lane's cells' neighbour rows (r + d - 1) * W and columns c + d - 1, a byte each: field 6 mt + d the row,
    // 6 mt + 3 + d the column; cells past the board alias real ones
    uint32_t nbp[kNbWords] = {};
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
        const int cell = (mt * 16 + (lane0 & 15)) % HW;
        const int r = cell / W, c = cell - r * W;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            int rr = r + d - 1, cc = c + d - 1;
            rr = rr < 0 ? rr + H : (rr >= H ? rr - H : rr);
            cc = cc < 0 ? cc + W : (cc >= W ? cc - W : cc);
            nbp[(6 * mt + d) >> 2] |= (uint32_t)(rr * W) << (8 * ((6 * mt + d) & 3));
            nbp[(6 * mt + 3 + d) >> 2] |= (uint32_t)cc << (8 * ((6 * mt + 3 + d) & 3));
        }
    }
    auto nb = [&](int f) { return (int)((nbp[f >> 2] >> (8 * (f & 3))) & 0xffu); };

    // uniform over the workgroup: passes, steps and with them every barrier below
    const int64_t per_pass = (int64_t)gridDim.x * kNW;
    const int passes = (int)((N + per_pass - 1) / per_pass);
    const int steps = passes * units;
    __syncthreads();

    int step = 0;
    for (int pass = 0; pass < passes; ++pass) {
        const int64_t n = (int64_t)pass * per_pass + (int64_t)blockIdx.x * kNW + wave;
        const bool active = n < N;   // wave-uniform
        // opaque copies of the lane index, here and in every unit: what is derived from them (addresses, offsets)
        // is rebuilt where it is used instead of being held in registers across the units, next to acc and h
        const int lane = opaque(lane0), lc = lane & 15, q = lane >> 4;
        f32x4 h[kMT][2];
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt) {
            h[mt][0] = h[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }

        if (active) {
            // the stem's input: channels 8 q .. 8 q + 7 of the lane's cells, converted on load (17..31 zero)
            const float *xs = a.x + n * (kStemC * HW);
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) {
                const int cell = mt * 16 + lc;
                const bool in = cell < HW;
                // every load is in bounds (channel and cell clamped) and unconditional; what is not x becomes 0
                const uint32_t xc = in ? cell : 0;
                float sv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int ch = 8 * q + e;
                    const float v = xs[(uint32_t)((ch < kStemC ? ch : kStemC - 1) * HW) + xc];
                    sv[e] = (in && ch < kStemC) ? v : 0.f;
                }
                if (in)
                    *reinterpret_cast<uint4 *>(img + img_row(cell, q)) = make_uint4(
                        bf16_pair(sv[0], sv[1]), bf16_pair(sv[2], sv[3]), bf16_pair(sv[4], sv[5]), bf16_pair(sv[6], sv[7]));
                if (q == 0) x0_s[wave * kMaxCells + cell] = sv[0];   // plane 0 (0 past the board)
            }
            lds_fence();
        }

        for (int u = 0; u < units; ++u, ++step) {
            const uint32_t *wu = w_lds[step & 1];
            // the next step's weights (the next unit, or unit 0 of the next pass) go to the other slot in three
            // chunks of kChunk uint4, each loaded before three taps' MFMAs and written to LDS after them
            const bool more = step + 1 < steps;
            const u32x4 *src = reinterpret_cast<const u32x4 *>(a.pack) + (int64_t)(u + 1 < units ? u + 1 : 0) * kUnitVec;
            u32x4 *dst = reinterpret_cast<u32x4 *>(w_lds[(step + 1) & 1]);
            const uint32_t tid = (uint32_t)opaque(threadIdx.x);
            const bool mine = more && tid < kChunk;
            // both branches stage the same three chunks; a wave without a sample only stages
            if (active) {
                const int lane = opaque(lane0), lc = lane & 15, q = lane >> 4;
#pragma unroll
                for (int k = 0; k < kNbWords; ++k) asm volatile("" : "+v"(nbp[k]));   // the 45 gather addresses too
                f32x4 acc[kMT][2];
#pragma unroll
                for (int mt = 0; mt < kMT; ++mt) acc[mt][0] = acc[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int tg = 0; tg < 3; ++tg) {
                    u32x4 st = {0u, 0u, 0u, 0u};
                    if (mine) st = src[tg * kChunk + tid];
#pragma unroll
                    for (int t = 3 * tg; t < 3 * tg + 3; ++t) {
                        bf16x8 wa[2];
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct)
                            wa[ct] = __builtin_bit_cast(bf16x8,
                                                        reinterpret_cast<const u32x4 *>(wu)[(t * 2 + ct) * 64 + lane]);
#pragma unroll
                        for (int mt = 0; mt < kMT; ++mt) {
                            const int cell = nb(6 * mt + t / 3) + nb(6 * mt + 3 + t % 3);
                            const bf16x8 xb =
                                __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(img + img_row(cell, q)));
#pragma unroll
                            for (int ct = 0; ct < 2; ++ct)
                                acc[mt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ct], xb, acc[mt][ct], 0, 0, 0);
                        }
                    }
                    if (mine) dst[tg * kChunk + tid] = st;
                }
                lds_fence();   // every lane's gathers done before the image is rewritten

                const bool last = u + 1 == units;
                const float *coef = reinterpret_cast<const float *>(wu) + kWWords;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int c0 = 16 * ct + 4 * q;
                    const f32x4 al = *reinterpret_cast<const f32x4 *>(coef + c0);
                    const f32x4 be = *reinterpret_cast<const f32x4 *>(coef + kCo + c0);
                    const f32x4 bi = *reinterpret_cast<const f32x4 *>(coef + 2 * kCo + c0);
#pragma unroll
                    for (int mt = 0; mt < kMT; ++mt) {
                        f32x4 o;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float v = (acc[mt][ct][r] + bi[r]) * al[r] + be[r];
                            if (u) v = h[mt][ct][r] + v;
                            o[r] = relu(v);
                        }
                        h[mt][ct] = o;
                        const int cell = mt * 16 + lc;
                        if (!last && cell < HW)
                            *reinterpret_cast<uint2 *>(img + img_row(cell, c0 >> 3) + 2 * (q & 1)) =
                                make_uint2(bf16_pair(o[0], o[1]), bf16_pair(o[2], o[3]));
                    }
                }
                lds_fence();
            } else if (mine) {
#pragma unroll
                for (int tg = 0; tg < 3; ++tg) dst[tg * kChunk + tid] = src[tg * kChunk + tid];
            }
            __syncthreads();
        }

        if (active) {
            // h_head = sum_q h * x[:, 0], h_avg = sum_q h / HW, policy = head_p . h_head, value = tanh(head_v . [..])
            const int lane = opaque(lane0), lc = lane & 15, q = lane >> 4;
            float x0[kMT];
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) x0[mt] = x0_s[wave * kMaxCells + mt * 16 + lc];
            float red[kActions + 2] = {};   // the lane's share of the 4 logits, of head_v . h_head and of head_v . sum h
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = 16 * ct + 4 * q + r;
                    float sh = 0.f, sa = 0.f;
#pragma unroll
                    for (int mt = 0; mt < kMT; ++mt)
                        if (mt * 16 + lc < HW) {
                            sh += h[mt][ct][r] * x0[mt];
                            sa += h[mt][ct][r];
                        }
#pragma unroll
                    for (int k = 0; k < kActions; ++k) red[k] += heads_s[k * kCo + c] * sh;
                    red[kActions] += heads_s[kActions * kCo + c] * sh;
                    red[kActions + 1] += heads_s[kActions * kCo + kCo + c] * sa;
                }
            // butterfly over each half of the wave (ds_swizzle's xor mode), then the two halves' sums as scalars
#pragma unroll
            for (int k = 0; k < kActions + 2; ++k) {
                red[k] += swz_xor<1>(red[k]);
                red[k] += swz_xor<2>(red[k]);
                red[k] += swz_xor<4>(red[k]);
                red[k] += swz_xor<8>(red[k]);
                red[k] += swz_xor<16>(red[k]);
                red[k] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(red[k]), 0)) +
                         __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(red[k]), 32));
            }
            if (lane < kActions) {
                float p = red[0];
#pragma unroll
                for (int k = 1; k < kActions; ++k) p = lane == k ? red[k] : p;
                a.policy[n * kActions + lane] = p;
            } else if (lane == kActions) {
                // head_v . [h_head, sum h / HW] with one division (exact sums stay exact up to that rounding)
                a.value[n] = tanhf((red[kActions] * (float)HW + red[kActions + 1]) / (float)HW);
            }
        }
    }
}

int status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)e;
}

}  // namespace

extern "C" {

int64_t hrl_geesenet_infer_bf16_pack_bytes(int64_t layers) {
    if (layers < 1 || layers > kMaxLayers) return 0;
    return 4 * ((layers + 1) * kUnitWords + kHeadWords);
}

int hrl_geesenet_infer_bf16_pack(const float *const *conv_w, const float *const *conv_b, const float *const *bn_w,
                                 const float *const *bn_b, const float *const *bn_mean, const float *const *bn_var,
                                 const double *bn_eps, int64_t layers, const float *head_p, const float *head_v,
                                 void *pack, void *stream) {
    if (!conv_w || !conv_b || !bn_w || !bn_b || !bn_mean || !bn_var || !bn_eps || layers < 1 || layers > kMaxLayers ||
        !head_p || !head_v || !pack || (reinterpret_cast<uintptr_t>(pack) & 15))
        return HRL_EINVAL;
    PackArgs a{};
    for (int u = 0; u <= layers; ++u) {
        if (!conv_w[u] || !conv_b[u] || !bn_w[u] || !bn_b[u] || !bn_mean[u] || !bn_var[u]) return HRL_EINVAL;
        a.conv_w[u] = conv_w[u];
        a.conv_b[u] = conv_b[u];
        a.bn_w[u] = bn_w[u];
        a.bn_b[u] = bn_b[u];
        a.bn_mean[u] = bn_mean[u];
        a.bn_var[u] = bn_var[u];
        a.eps[u] = bn_eps[u];
    }
    a.head_p = head_p;
    a.head_v = head_v;
    a.units = (int)layers + 1;
    a.out = static_cast<uint32_t *>(pack);
    const int total = a.units * kUnitWords + kHeadWords;
    hipLaunchKernelGGL(geese_bf16_pack_kernel, dim3((total + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return status();
}

int hrl_geesenet_infer_bf16(const void *pack, int64_t layers, const float *x, int64_t N, int64_t H, int64_t W,
                            float *policy, float *value, void *stream) {
    if (!pack || (reinterpret_cast<uintptr_t>(pack) & 15) || layers < 1 || layers > kMaxLayers || !x || !policy ||
        !value || N < 0 || H < 1 || W < 1 || H > kMaxCells || W > kMaxCells || H * W > kMaxCells ||
        N >= ((int64_t)1 << 40) / (kCo * kMaxCells))
        return HRL_EINVAL;
    if (N == 0) return HRL_OK;
    InferArgs a{};
    a.pack = static_cast<const uint32_t *>(pack);
    a.x = x;
    a.policy = policy;
    a.value = value;
    a.N = N;
    a.units = (int)layers + 1;
    a.H = (int)H;
    a.W = (int)W;
    const int64_t blocks = (N + kNW - 1) / kNW;
    hipLaunchKernelGGL(geese_bf16_kernel, dim3((unsigned)(blocks < kGridCap ? blocks : kGridCap)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return status();
}

}  // extern "C"
