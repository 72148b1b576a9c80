// hrl_torus_bf16.hip — the GeeseNet learner tower in mixed precision (gfx950): bf16 conv operands and bf16
// stored activations / gradients, fp32 accumulation, statistics and coefficients (contract: include/hrl_nn.h).
//
// Every stored tower tensor (H, Y, DY, G) is channels-last bf16, [sample][cell][32 ch]: 64 B per cell, four
// 16-byte chunks g = channels 8g..8g+7, so chunk j = 4 cell + g of a sample is one coalesced uint4.  That is the
// column operand of v_mfma_f32_16x16x32_bf16 as lane l reads it (cell l & 15, channels 8 (l >> 4) + e), so a
// sample goes to its LDS image with 16-byte copies: no transpose, no split.  Image rows are hrl_geesenet_bf16.hip's:
// chunk g of a cell sits at g ^ ((cell >> 2) & 3) (16 consecutive cells hit 16 distinct bank quads).
//
// torus_bf16_conv_kernel<MODE, G32> (forward and adjoint, one product per k-step, 90 MFMAs per sample):
//   8 waves per workgroup, a wave owns one sample at a time; weights are the rows ([tap][co-tile][lane][8 bf16],
//   18,432 B in LDS once per workgroup), cells the columns, so lane l's accumulators of (cell tile mt, co-tile ct)
//   are channels 16 ct + 4 (l >> 4) + 0..3 of cell 16 mt + (l & 15).
//   staging  STEM: fp32 x (N, 17, HW) -> bf16 image, channels 17..31 zero;
//            PRO1/PRO2: chunk-wise H = bf(relu([float(Hprev) +] float(Yprev) alpha + beta)), stored once and
//            fed to the image;  ADJ: DY copied.  The next sample's chunks are loaded before the MFMAs.
//   forward epilogue: y = acc + bias; sum y and sum y^2 per channel from the fp32 values (fp32 over the lane's
//            cells of a sample, fp64 across samples, fixed folds); bf(y) through the dead image to 16-byte stores.
//   adjoint epilogue: acc -> an fp32 [cell][32] tile in LDS; chunk-wise G = bf(acc + gm), gm = float(Gnext)
//            [Hnext > 0] (G32: the last unit's fp32 masked gradient), and the previous unit's backward sums
//            sum v and sum v (float(Yprev) - mean) over v = float(G) [H > 0].
// torus_bf16_wgrad_kernel<STEM, G32>: dW[tap] (co x ci) += DY (co x 16 cells) . X_tap (16 cells x ci) with
//   v_mfma_f32_32x32x16_bf16, one product per k-step and tap (45 per sample).  Both operands want a channel's
//   consecutive cells, so staging transposes into [ch][cell] bf16 tiles while it forms dy from the BatchNorm
//   backward apply (hrl_torus_conv_wgrad_bn's operations), stores DY and sums db from the rounded values.
// torus_bf16_pack_kernel: bf(W) of every unit in forward and adjoint operand order, one launch per step.
// bn_bf16_output_kernel / bn_bf16_masked_sums_kernel: the two layout crossings, the last unit's output as fp32
//   NCHW for the pool and the pool's fp32 NCHW gradient as masked fp32 channels-last with its backward sums.
// torus_bf16_heads_fwd_kernel / _bwd_kernel (precision 'bf16_heads'): the tail without either crossing, the last
//   unit's output rebuilt from Y, H and the coefficients in registers, pooled and put through both heads; the
//   backward writes the masked fp32 gradient, its sums and the head weight gradients (described at the kernels).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrl_nn.h"
#include "../../include/hrl_targets.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kCo = 32;
constexpr int kStemC = 17;
constexpr int kMT = 5;                     // 16-cell tiles: boards of at most 80 cells
constexpr int kMaxCells = kMT * 16;
constexpr int kTaps = 9;
constexpr int kMaxUnits = 17;
constexpr int kNW = 8;                     // conv: waves (samples) per workgroup
constexpr int kThreads = 64 * kNW;
constexpr int kGridConv = 512;             // conv workgroups: kGridConv * kNW samples per pass
constexpr int kWW = 4;                     // wgrad waves per workgroup
constexpr int kWThreads = 64 * kWW;
constexpr int kGridWgrad = 256;
constexpr int kWWords = kTaps * 2 * 64 * 4;   // one unit's operands of one form, 4-byte words (18,432 B)
constexpr int kImgWords = kMaxCells * 16;     // bf16 image of a sample (5,120 B)
constexpr int kTileWords = kMaxCells * kCo;   // adjoint: fp32 [cell][32] tile (10,240 B)
constexpr int kNCh = kMaxCells * 4 / 64;      // chunks per lane of an 80-cell sample (5)
constexpr int kPart = kTaps * kCo * kCo + kCo;   // wgrad partial: [tap][ci][co] then db
constexpr int kSB = 88;                    // wgrad tile row stride in bf16: 176 B, 16-byte aligned rows

// two fp32 -> two bf16, round to nearest even (a in the low half)
__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ float bf_round(float v) { return bf_lo(bf16_pair(v, 0.f)); }

__device__ __forceinline__ void unpack8(const uint4 &v, float (&f)[8]) {
    f[0] = bf_lo(v.x); f[1] = bf_hi(v.x); f[2] = bf_lo(v.y); f[3] = bf_hi(v.y);
    f[4] = bf_lo(v.z); f[5] = bf_hi(v.z); f[6] = bf_lo(v.w); f[7] = bf_hi(v.w);
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
    return make_uint4(bf16_pair(f[0], f[1]), bf16_pair(f[2], f[3]), bf16_pair(f[4], f[5]), bf16_pair(f[6], f[7]));
}

__device__ __forceinline__ void lds_fence() {
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS operations done
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int opaque(int i) {
    asm volatile("" : "+v"(i));
    return i;
}
__device__ __forceinline__ float relu(float v) { return v < 0.f ? 0.f : v; }   // NaN stays NaN
__device__ __forceinline__ int fdiv(int e, float inv) { return (int)(((float)e + 0.5f) * inv); }

// dword of channel group g (8 channels, 16 B) of a cell's image row
__device__ __forceinline__ int img_row(int cell, int g) { return cell * 16 + 4 * (g ^ ((cell >> 2) & 3)); }
// dword of the 4-channel group c4 of a cell's fp32 tile row
__device__ __forceinline__ int tile_row(int cell, int c4) { return cell * kCo + 4 * (c4 ^ (cell & 7)); }

// the sum of `v` over the 16 lanes l ^ (M, 2M, 4M, 8M), the same fixed order in every lane
template <int M>
__device__ __forceinline__ double fold16(double v) {
#pragma unroll
    for (int s = 0; s < 4; ++s) v += __shfl_xor(v, M << s, 64);
    return v;
}

// ------------------------------------------------------------------ pack
struct PackArgs {
    const float *w[kMaxUnits];
    int units, stem_cin;
    uint32_t *out;   // [unit][forward | adjoint][kWWords]
};

__global__ __launch_bounds__(256) void torus_bf16_pack_kernel(PackArgs a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.units * 2 * kWWords) return;
    const int u = idx / (2 * kWWords), i = idx - u * 2 * kWWords;
    const int adj = i >= kWWords ? 1 : 0, j = i - adj * kWWords;
    const int cin = u == 0 ? a.stem_cin : kCo;
    const int d = j & 3, l = (j >> 2) & 63, ct = (j >> 8) & 1, tap = j >> 9;
    const int oc = ct * 16 + (l & 15), ic = 8 * (l >> 4) + 2 * d;   // this conv's output row, input channel pair
    const float *w = a.w[u];
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        if (!adj) v[e] = ic + e < cin ? w[(oc * cin + ic + e) * kTaps + tap] : 0.f;
        else v[e] = oc < cin ? w[((ic + e) * cin + oc) * kTaps + (kTaps - 1 - tap)] : 0.f;   // W'[ci][co][8 - tap]
    }
    a.out[idx] = bf16_pair(v[0], v[1]);
}

// ------------------------------------------------------------------ forward / adjoint conv
enum { STEM = 0, PRO1 = 1, PRO2 = 2, ADJ = 3 };

struct ConvArgs {
    int64_t N;
    int H, W;
    const uint32_t *wpk;           // the unit's operands of this form
    const float *x;                // STEM: (N, 17, HW) fp32
    const uint4 *yprev, *hprev;    // PRO: the previous unit's conv output and input (residual), channels-last bf16
    const float *alpha, *beta;     // PRO
    uint4 *hout;                   // PRO: this unit's input, written once
    const uint4 *in;               // ADJ: DY
    const float *bias;             // forward
    uint4 *out;                    // Y (forward) or G (adjoint)
    double *part;                  // [gridDim.x][32][2]
    const void *gnext;             // ADJ: G of the next unit (bf16), or with G32 the masked fp32 gradient [n][cell][32]
    const uint4 *hnext;            // ADJ (!G32): the next unit's input (this unit's block output)
    const uint4 *hmask, *ymask;    // ADJ: this unit's input H and the previous unit's conv output Y
    const float *mean;             // ADJ: the previous unit's save_mean
};

template <int MODE, bool G32>
__global__ __launch_bounds__(kThreads) void torus_bf16_conv_kernel(ConvArgs a) {
    constexpr int kRegion = MODE == ADJ ? kTileWords : kImgWords;
    __shared__ __attribute__((aligned(16))) uint32_t w_lds[kWWords];
    __shared__ __attribute__((aligned(16))) uint32_t regions[kNW * kRegion];
    __shared__ __attribute__((aligned(16))) float coef_s[2 * kCo];   // PRO: alpha | beta; ADJ: mean
    __shared__ double red[kNW * kCo * 2];
    const int64_t N = a.N;
    const int H = a.H, W = a.W, HW = H * W, nch = 4 * HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, q = lane >> 4;
    uint32_t *img = regions + wave * kRegion;

    for (int i = threadIdx.x; i < kWWords / 4; i += kThreads)
        reinterpret_cast<uint4 *>(w_lds)[i] = reinterpret_cast<const uint4 *>(a.wpk)[i];
    if constexpr (MODE == PRO1 || MODE == PRO2) {
        if (threadIdx.x < 2 * kCo) coef_s[threadIdx.x] = threadIdx.x < kCo ? a.alpha[threadIdx.x] : a.beta[threadIdx.x - kCo];
    }
    if constexpr (MODE == ADJ) {
        if (threadIdx.x < kCo) coef_s[threadIdx.x] = a.mean[threadIdx.x];
    }
    // the lane's column cells 16 mt + lc (cells past the board alias real ones: their columns are never stored):
    // (row (r + d - 1) * W) | (column (c + d - 1)) << 16
    uint32_t nbp[kMT][3];
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
        const int cell = (mt * 16 + lc) % HW;
        const int r = cell / W, c = cell - r * W;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            int rr = r + d - 1, cc = c + d - 1;
            rr = rr < 0 ? rr + H : (rr >= H ? rr - H : rr);
            cc = cc < 0 ? cc + W : (cc >= W ? cc - W : cc);
            nbp[mt][d] = (uint32_t)(rr * W) | ((uint32_t)cc << 16);
        }
    }
    float bias_v[2][4] = {};
    if constexpr (MODE != ADJ) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) bias_v[ct][r] = a.bias[ct * 16 + 4 * q + r];
    }
    // the lane's 8 channels: forward 16 ct + 4 q + r (slot 4 ct + r), adjoint 8 (lane & 3) + e
    double s1[8], s2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s1[i] = s2[i] = 0.0;

    // staged input of one sample: chunks j = 64 k + lane < 4 HW (clamped loads issue back to back)
    uint4 sa[MODE == STEM ? 1 : kNCh], sb[MODE == PRO2 ? kNCh : 1];
    float sx[MODE == STEM ? kMT : 1][8];
    auto load = [&](int64_t m) {
        if constexpr (MODE == STEM) {
            const float *xs = a.x + m * (kStemC * HW);
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) {
                const int cell = mt * 16 + lc;
                const int xc = cell < HW ? cell : 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int ch = 8 * q + e;
                    const float v = xs[(ch < kStemC ? ch : kStemC - 1) * HW + xc];
                    sx[mt][e] = ch < kStemC ? v : 0.f;
                }
            }
        } else {
            const uint4 *p = (MODE == ADJ ? a.in : a.yprev) + m * nch;
#pragma unroll
            for (int k = 0; k < kNCh; ++k) sa[k] = p[min(k * 64 + lane, nch - 1)];
            if constexpr (MODE == PRO2) {
                const uint4 *r = a.hprev + m * nch;
#pragma unroll
                for (int k = 0; k < kNCh; ++k) sb[k] = r[min(k * 64 + lane, nch - 1)];
            }
        }
    };

    const int64_t stride = (int64_t)gridDim.x * kNW;
    int64_t n = (int64_t)blockIdx.x * kNW + wave;
    if (n < N) load(n);
    __syncthreads();   // weights and coefficients in LDS

    for (; n < N; n += stride) {
        // the 45 gather addresses are rebuilt per tap, not held across the sample next to the staged chunks
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
            for (int d = 0; d < 3; ++d) asm volatile("" : "+v"(nbp[mt][d]));
        // ---- staging: the sample's image
        if constexpr (MODE == STEM) {
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) {
                const int cell = mt * 16 + lc;
                if (cell < HW) *reinterpret_cast<uint4 *>(img + img_row(cell, q)) = pack8(sx[mt]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kNCh; ++k) {
                const int j = opaque(k * 64 + lane);
                if (j < nch) {
                    const int cell = j >> 2, g = j & 3;
                    uint4 v = sa[k];
                    if constexpr (MODE == PRO1 || MODE == PRO2) {
                        float y[8], hp[8], o[8];
                        unpack8(sa[k], y);
                        if constexpr (MODE == PRO2) unpack8(sb[k], hp);
                        const float4 *al = reinterpret_cast<const float4 *>(coef_s + 8 * g);
                        const float4 *be = reinterpret_cast<const float4 *>(coef_s + kCo + 8 * g);
                        const float4 a0 = al[0], a1 = al[1], b0 = be[0], b1 = be[1];
                        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                        const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float t = y[e] * av[e] + bv[e];
                            if constexpr (MODE == PRO2) t = hp[e] + t;
                            o[e] = relu(t);
                        }
                        v = pack8(o);
                        a.hout[n * nch + j] = v;
                    }
                    *reinterpret_cast<uint4 *>(img + img_row(cell, g)) = v;
                }
            }
        }
        lds_fence();
        const int64_t next = n + stride;
        if (next < N) load(next);   // in flight during the MFMAs
        // the adjoint's residual operands, in flight during the MFMAs as well
        uint4 ga[(MODE == ADJ && !G32) ? kNCh : 1], gh[(MODE == ADJ && !G32) ? kNCh : 1];
        if constexpr (MODE == ADJ && !G32) {
            const uint4 *gp = reinterpret_cast<const uint4 *>(a.gnext) + n * nch, *hp = a.hnext + n * nch;
#pragma unroll
            for (int k = 0; k < kNCh; ++k) {
                ga[k] = gp[min(k * 64 + lane, nch - 1)];
                gh[k] = hp[min(k * 64 + lane, nch - 1)];
            }
        }

        f32x4 acc[kMT][2];
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt) acc[mt][0] = acc[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            bf16x8 wa[2];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
                wa[ct] = __builtin_bit_cast(bf16x8, reinterpret_cast<const u32x4 *>(w_lds)[(t * 2 + ct) * 64 + lane]);
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) {
                const int cell = (int)(nbp[mt][t / 3] & 0xffffu) + (int)(nbp[mt][t % 3] >> 16);
                const bf16x8 xb = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(img + img_row(cell, q)));
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    acc[mt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ct], xb, acc[mt][ct], 0, 0, 0);
            }
        }
        lds_fence();   // every lane's image reads done before the region takes the output

        if constexpr (MODE != ADJ) {
            float t1[8], t2[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) t1[i] = t2[i] = 0.f;
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) {
                const int cell = mt * 16 + lc;
                if (cell < HW) {
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        float v[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            v[r] = acc[mt][ct][r] + bias_v[ct][r];
                            t1[4 * ct + r] += v[r];
                            t2[4 * ct + r] += v[r] * v[r];
                        }
                        // channels 16 ct + 4 q ..: half (q & 1) of chunk 2 ct + (q >> 1)
                        *reinterpret_cast<uint2 *>(img + img_row(cell, 2 * ct + (q >> 1)) + 2 * (q & 1)) =
                            make_uint2(bf16_pair(v[0], v[1]), bf16_pair(v[2], v[3]));
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                s1[i] += (double)t1[i];
                s2[i] += (double)t2[i];
            }
            lds_fence();
            for (int j = lane; j < nch; j += 64)
                a.out[n * nch + j] = *reinterpret_cast<const uint4 *>(img + img_row(j >> 2, j & 3));
        } else {
            float *tile = reinterpret_cast<float *>(img);
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) {
                const int cell = mt * 16 + lc;
                if (cell < HW) {
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
                        *reinterpret_cast<f32x4 *>(tile + tile_row(cell, 4 * ct + q)) = acc[mt][ct];
                }
            }
            // this unit's input and the previous unit's conv output, for the sums
            uint4 hm[kNCh], ym[kNCh];
            {
                const uint4 *hp = a.hmask + n * nch, *yp = a.ymask + n * nch;
#pragma unroll
                for (int k = 0; k < kNCh; ++k) {
                    hm[k] = hp[min(k * 64 + lane, nch - 1)];
                    ym[k] = yp[min(k * 64 + lane, nch - 1)];
                }
            }
            lds_fence();
            float t1[8], t2[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) t1[i] = t2[i] = 0.f;
            const int g = lane & 3;   // = j & 3 of every chunk of this lane
#pragma unroll
            for (int k = 0; k < kNCh; ++k) {
                const int j = opaque(k * 64 + lane);
                if (j < nch) {
                    const int cell = j >> 2;
                    const f32x4 c0 = *reinterpret_cast<const f32x4 *>(tile + tile_row(cell, 2 * g));
                    const f32x4 c1 = *reinterpret_cast<const f32x4 *>(tile + tile_row(cell, 2 * g + 1));
                    const float c[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
                    float gm[8];
                    if constexpr (G32) {
                        const float4 *gp = reinterpret_cast<const float4 *>(a.gnext) + (n * nch + j) * 2;
                        const float4 g0 = gp[0], g1 = gp[1];
                        gm[0] = g0.x; gm[1] = g0.y; gm[2] = g0.z; gm[3] = g0.w;
                        gm[4] = g1.x; gm[5] = g1.y; gm[6] = g1.z; gm[7] = g1.w;
                    } else {
                        float gv[8], hv[8];
                        unpack8(ga[k], gv);
                        unpack8(gh[k], hv);
#pragma unroll
                        for (int e = 0; e < 8; ++e) gm[e] = hv[e] > 0.f ? gv[e] : 0.f;
                    }
                    float v[8], hmv[8], yv[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = c[e] + gm[e];
                    const uint4 vb = pack8(v);
                    a.out[n * nch + j] = vb;
                    unpack8(vb, v);   // the sums take the stored (rounded) gradient
                    unpack8(hm[k], hmv);
                    unpack8(ym[k], yv);
                    const float4 m0 = reinterpret_cast<const float4 *>(coef_s + 8 * g)[0];
                    const float4 m1 = reinterpret_cast<const float4 *>(coef_s + 8 * g)[1];
                    const float mu[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float m = hmv[e] > 0.f ? v[e] : 0.f;
                        t1[e] += m;
                        t2[e] += m * (yv[e] - mu[e]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                s1[i] += (double)t1[i];
                s2[i] += (double)t2[i];
            }
        }
        lds_fence();   // the region's reads done before the next image is written
    }

    // fold the 16 lanes that share the lane's channels, then the 8 waves, in a fixed order
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s1[i] = MODE == ADJ ? fold16<4>(s1[i]) : fold16<1>(s1[i]);
        s2[i] = MODE == ADJ ? fold16<4>(s2[i]) : fold16<1>(s2[i]);
    }
    if constexpr (MODE == ADJ) {
        if (lane < 4) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                red[(wave * kCo + 8 * lane + e) * 2 + 0] = s1[e];
                red[(wave * kCo + 8 * lane + e) * 2 + 1] = s2[e];
            }
        }
    } else {
        if (lc == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int co = (i >> 2) * 16 + 4 * q + (i & 3);
                red[(wave * kCo + co) * 2 + 0] = s1[i];
                red[(wave * kCo + co) * 2 + 1] = s2[i];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * kCo) {
        double t = 0.0;
        for (int w = 0; w < kNW; ++w) t += red[w * kCo * 2 + threadIdx.x];
        a.part[(int64_t)blockIdx.x * kCo * 2 + threadIdx.x] = t;
    }
}

// ------------------------------------------------------------------ weight gradient with the BatchNorm backward apply
struct WgArgs {
    int64_t N;
    int H, W;
    const float *x;        // STEM: (N, 17, HW) fp32
    const uint4 *h;        // !STEM: the unit's input, channels-last bf16
    const uint4 *y;        // the unit's conv output
    const void *g;         // the gradient w.r.t. the block output: bf16, or with G32 the masked fp32 [n][cell][32]
    const float *alpha, *beta, *mean, *invstd, *gamma, *kcoef, *gmean;
    int residual;
    uint4 *dy;
    float *partial;
};

template <bool IS_STEM, bool G32>
__global__ __launch_bounds__(kWThreads) void torus_bf16_wgrad_kernel(WgArgs a) {
    constexpr int kTile = kCo * kSB;                          // bf16 elements of a [ch][cell] tile
    constexpr int kNX = (kStemC * kMaxCells + 63) / 64;       // STEM: x floats per lane
    __shared__ __attribute__((aligned(16))) uint16_t tiles[kWW][2][kTile];   // per wave: dY, X
    __shared__ uint32_t nbp_tab[kMaxCells * 3];
    __shared__ __attribute__((aligned(16))) float bnc[7 * kCo];   // mean, k, gmean, invstd, gamma, alpha, beta
    static_assert(sizeof(tiles) >= (kPart + kWW * 2 * kCo) * sizeof(float), "fold buffer");
    const int64_t N = a.N;
    const int H = a.H, W = a.W, HW = H * W, nch = 4 * HW, x_elem = kStemC * HW;
    const float inv_hw = 1.0f / (float)HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint16_t *gs = tiles[wave][0], *xs = tiles[wave][1];
    if (threadIdx.x < kCo) {
        const int c = threadIdx.x;
        bnc[c] = a.mean[c];
        bnc[kCo + c] = a.kcoef[c];
        bnc[2 * kCo + c] = a.gmean[c];
        bnc[3 * kCo + c] = a.invstd[c];
        bnc[4 * kCo + c] = a.gamma ? a.gamma[c] : 1.0f;
        bnc[5 * kCo + c] = a.alpha[c];
        bnc[6 * kCo + c] = a.beta[c];
    }
    for (int i = threadIdx.x; i < kMaxCells * 3; i += kWThreads) {
        const int qc = i / 3, d = i - qc * 3;
        uint32_t v = 0u;   // cells past the board: dY is zero there, any cell will do
        if (qc < HW) {
            const int r = qc / W, c = qc - r * W;
            int rr = r + d - 1, cc = c + d - 1;
            rr = rr < 0 ? rr + H : (rr >= H ? rr - H : rr);
            cc = cc < 0 ? cc + W : (cc >= W ? cc - W : cc);
            v = (uint32_t)(rr * W) | ((uint32_t)cc << 16);
        }
        nbp_tab[i] = v;
    }
    for (int i = lane; i < kTile; i += 64) { gs[i] = 0; xs[i] = 0; }   // cells past the board, channels past Cin
    __syncthreads();

    f32x16 acc[kTaps];
#pragma unroll
    for (int t = 0; t < kTaps; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    float bsum = 0.f;
    const int r = lane & 31, h = lane >> 5;

    uint4 sg[G32 ? 2 * kNCh : kNCh], sy[kNCh], sh[IS_STEM ? 1 : kNCh];
    float sxs[IS_STEM ? kNX : 1];
    auto load = [&](int64_t m) {
#pragma unroll
        for (int k = 0; k < kNCh; ++k) {
            const int j = min(k * 64 + lane, nch - 1);
            sy[k] = a.y[m * nch + j];
            if constexpr (!IS_STEM) sh[k] = a.h[m * nch + j];
            if constexpr (G32) {
                const uint4 *gp = reinterpret_cast<const uint4 *>(a.g) + (m * nch + j) * 2;
                sg[2 * k] = gp[0];
                sg[2 * k + 1] = gp[1];
            } else {
                sg[k] = reinterpret_cast<const uint4 *>(a.g)[m * nch + j];
            }
        }
        if constexpr (IS_STEM) {
            const float *xp = a.x + m * x_elem;
#pragma unroll
            for (int k = 0; k < kNX; ++k) sxs[k] = xp[min(k * 64 + lane, x_elem - 1)];
        }
    };
    const int64_t stride = (int64_t)gridDim.x * kWW;
    int64_t n = (int64_t)blockIdx.x * kWW + wave;
    if (n < N) load(n);
    for (; n < N; n += stride) {
        if constexpr (IS_STEM) {
#pragma unroll
            for (int k = 0; k < kNX; ++k) {
                const int e = opaque(k * 64 + lane);
                if (e < x_elem) {
                    const int c = fdiv(e, inv_hw);
                    xs[c * kSB + (e - c * HW)] = (uint16_t)bf16_pair(sxs[k], 0.f);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kNCh; ++k) {
            const int j = opaque(k * 64 + lane);
            if (j < nch) {
                const int cell = j >> 2, c0 = 8 * (j & 3);
                float y[8], gv[8], hp[8], dyv[8];
                unpack8(sy[k], y);
                if constexpr (G32) {
                    const uint4 g0 = sg[2 * k], g1 = sg[2 * k + 1];
                    const uint32_t gw[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) gv[e] = __uint_as_float(gw[e]);
                } else {
                    unpack8(sg[k], gv);
                }
                if constexpr (!IS_STEM) unpack8(sh[k], hp);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int c = c0 + e;
                    float gmv = gv[e];
                    if constexpr (!G32) {
                        // [H_next > 0] recomputed as the forward formed and stored it
                        const float z = y[e] * bnc[5 * kCo + c] + bnc[6 * kCo + c];
                        const float o = (!IS_STEM && a.residual) ? hp[e] + z : z;
                        gmv = bf_round(relu(o)) > 0.f ? gv[e] : 0.f;
                    }
                    const float t = (y[e] - bnc[c]) * bnc[kCo + c];
                    dyv[e] = (((gmv - bnc[2 * kCo + c]) - t) * bnc[3 * kCo + c]) * bnc[4 * kCo + c];
                }
                const uint4 db = pack8(dyv);
                a.dy[n * nch + j] = db;
                const uint32_t dw[4] = {db.x, db.y, db.z, db.w};
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    gs[(c0 + e) * kSB + cell] = (uint16_t)(dw[e >> 1] >> (16 * (e & 1)));
                if constexpr (!IS_STEM) {
                    const uint32_t hw[4] = {sh[k].x, sh[k].y, sh[k].z, sh[k].w};
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        xs[(c0 + e) * kSB + cell] = (uint16_t)(hw[e >> 1] >> (16 * (e & 1)));
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        lds_fence();
        if (n + stride < N) load(n + stride);   // in flight during the MFMAs

#pragma unroll 1
        for (int ks = 0; ks < kMaxCells / 16; ++ks) {
            const int cell0 = ks * 16 + 8 * h;
            const uint4 A = *reinterpret_cast<const uint4 *>(gs + r * kSB + cell0);   // dY[co = r][cell0 .. + 7]
            float av[8];
            unpack8(A, av);
#pragma unroll
            for (int j = 0; j < 8; ++j) bsum += av[j];
            uint32_t nbp[8][3];
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int d = 0; d < 3; ++d) nbp[j][d] = nbp_tab[(cell0 + j) * 3 + d];
            const uint16_t *xrow = xs + r * kSB;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                uint32_t b[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) b[j] = xrow[(nbp[j][t / 3] & 0xffffu) + (nbp[j][t % 3] >> 16)];
                const uint4 B = make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16),
                                           b[6] | (b[7] << 16));   // X[ci = r][nbr(cell0 + j, tap)]
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A),
                                                                 __builtin_bit_cast(bf16x8, B), acc[t], 0, 0, 0);
            }
        }
        lds_fence();   // the tiles are rewritten for the next sample
    }
    // fold the waves in a fixed order ((w0 + w1) + w2) + w3: red[tap][ci][co], then db per (wave, half)
    float *red = reinterpret_cast<float *>(tiles);
    float *bred = red + kPart;
    __syncthreads();
#pragma unroll 1
    for (int w = 0; w < kWW; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < kTaps; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    // C/D: col = lane & 31 (ci), row = (reg & 3) + 8 (reg >> 2) + 4h (co)
                    const int co = (i & 3) + 8 * (i >> 2) + 4 * h;
                    float *d = red + (t * kCo + r) * kCo + co;
                    *d = w == 0 ? acc[t][i] : *d + acc[t][i];
                }
            bred[(wave * 2 + h) * kCo + r] = bsum;
        }
        __syncthreads();
    }
    float *out = a.partial + (int64_t)blockIdx.x * kPart;
    for (int i = threadIdx.x; i < kTaps * kCo * kCo; i += kWThreads) out[i] = red[i];
    if (threadIdx.x < kCo) {
        float b = 0.f;
        for (int i = 0; i < kWW * 2; ++i) b += bred[i * kCo + threadIdx.x];
        out[kTaps * kCo * kCo + threadIdx.x] = b;
    }
}

// fold per-workgroup partials (fixed order, fp64) into dW (32, Cin, 3, 3) and db (32)
__global__ __launch_bounds__(256) void torus_bf16_wgrad_reduce_kernel(const float *__restrict__ partial, int nparts,
                                                                      int Cin, float *__restrict__ dw,
                                                                      float *__restrict__ db) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kPart) return;
    double s = 0.0;
    for (int w = 0; w < nparts; ++w) s += (double)partial[(int64_t)w * kPart + i];
    if (i < kTaps * kCo * kCo) {
        const int co = i % kCo, ci = (i / kCo) % kCo, tap = i / (kCo * kCo);
        if (ci < Cin) dw[(co * Cin + ci) * kTaps + tap] = (float)s;
    } else if (db) {
        db[i - kTaps * kCo * kCo] = (float)s;
    }
}

// ------------------------------------------------------------------ the two layout crossings
constexpr int kS = 81;   // fp32 [c][cell] tile row stride (odd: a column read walks the banks)

// out (N, 32, HW) fp32 = relu([float(hprev) +] float(y) alpha + beta), unrounded, for the pool
__global__ __launch_bounds__(256) void bn_bf16_output_kernel(const uint4 *__restrict__ y, const uint4 *__restrict__ hprev,
                                                             const float *__restrict__ alpha,
                                                             const float *__restrict__ beta, int64_t N, int HW,
                                                             float *__restrict__ out) {
    __shared__ float tiles[4][kCo * kS];
    __shared__ float coef_s[2 * kCo];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = 4 * HW;
    float *tile = tiles[wave];
    if (threadIdx.x < 2 * kCo) coef_s[threadIdx.x] = threadIdx.x < kCo ? alpha[threadIdx.x] : beta[threadIdx.x - kCo];
    __syncthreads();
    for (int64_t n = (int64_t)blockIdx.x * 4 + wave; n < N; n += (int64_t)gridDim.x * 4) {
        for (int j = lane; j < nch; j += 64) {
            const int cell = j >> 2, c0 = 8 * (j & 3);
            float yv[8], hv[8];
            unpack8(y[n * nch + j], yv);
            if (hprev) unpack8(hprev[n * nch + j], hv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float t = yv[e] * coef_s[c0 + e] + coef_s[kCo + c0 + e];
                if (hprev) t = hv[e] + t;
                tile[(c0 + e) * kS + cell] = relu(t);
            }
        }
        lds_fence();
        const int inv_n = kCo * HW;
        const float inv_hw = 1.0f / (float)HW;
        for (int e = lane; e < inv_n; e += 64) {
            const int c = fdiv(e, inv_hw);
            out[n * inv_n + e] = tile[c * kS + (e - c * HW)];
        }
        lds_fence();
    }
}

// gm [n][cell][32] fp32 = g [bf(out) > 0] from the fp32 (N, 32, HW) gradient and block output of the last unit, and
// its BatchNorm backward sums part[block][c] = (sum gm, sum gm (float(y) - mean[c]))
__global__ __launch_bounds__(256) void bn_bf16_masked_sums_kernel(const float *__restrict__ g, const float *__restrict__ out,
                                                                  const uint4 *__restrict__ y,
                                                                  const float *__restrict__ mean, int64_t N, int HW,
                                                                  float4 *__restrict__ gm, double *__restrict__ part) {
    __shared__ float tiles[4][kCo * kS];
    __shared__ float mean_s[kCo];
    __shared__ double red[4 * kCo * 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = 4 * HW, n_elem = kCo * HW;
    const float inv_hw = 1.0f / (float)HW;
    float *tile = tiles[wave];
    if (threadIdx.x < kCo) mean_s[threadIdx.x] = mean[threadIdx.x];
    __syncthreads();
    double s1[8], s2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s1[i] = s2[i] = 0.0;
    const int c0 = 8 * (lane & 3);
    for (int64_t n = (int64_t)blockIdx.x * 4 + wave; n < N; n += (int64_t)gridDim.x * 4) {
        for (int e = lane; e < n_elem; e += 64) {
            const int c = fdiv(e, inv_hw);
            const float o = out[n * n_elem + e], gv = g[n * n_elem + e];
            tile[c * kS + (e - c * HW)] = bf_round(o) > 0.f ? gv : 0.f;
        }
        lds_fence();
        float t1[8], t2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t1[i] = t2[i] = 0.f;
        for (int j = lane; j < nch; j += 64) {
            const int cell = j >> 2;
            float v[8], yv[8];
            unpack8(y[n * nch + j], yv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[e] = tile[(c0 + e) * kS + cell];
                t1[e] += v[e];
                t2[e] += v[e] * (yv[e] - mean_s[c0 + e]);
            }
            gm[(n * nch + j) * 2] = make_float4(v[0], v[1], v[2], v[3]);
            gm[(n * nch + j) * 2 + 1] = make_float4(v[4], v[5], v[6], v[7]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            s1[i] += (double)t1[i];
            s2[i] += (double)t2[i];
        }
        lds_fence();
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s1[i] = fold16<4>(s1[i]);
        s2[i] = fold16<4>(s2[i]);
    }
    if (lane < 4) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            red[(wave * kCo + 8 * lane + e) * 2 + 0] = s1[e];
            red[(wave * kCo + 8 * lane + e) * 2 + 1] = s2[e];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * kCo) {
        double t = 0.0;
        for (int w = 0; w < 4; ++w) t += red[w * kCo * 2 + threadIdx.x];
        part[(int64_t)blockIdx.x * kCo * 2 + threadIdx.x] = t;
    }
}

// ------------------------------------------------------------------ the fused tail: last unit's output, pool, heads
// A wave owns a sample, 8 waves a workgroup.  Lane l reads chunks j = 64 k + l of Y (and H): always channel group
// g = l & 3 (channels 8 g .. 8 g + 7), cells 16 k + (l >> 2).  out = relu([float(H) +] float(Y) alpha + beta) is
// rebuilt chunk-wise in bn_bf16_output_kernel's operation order and never stored; a channel's sum over the cells
// is the lane's fp32 partial (at most 5 cells) folded over the 16 lanes l ^ (4, 8, 16, 32), after which every lane
// of a group holds its 8 channels of h_head and h_avg.  The head products are 8-channel partials per lane folded
// over l ^ (1, 2).  Head weights, alpha, beta (and mean) sit in LDS; nothing else does.
constexpr int kActions = 4;
constexpr int kHeadW = (kActions + 2) * kCo;   // head_p (4, 32) | head_v (1, 64); also a workgroup's dW partial

template <int M>
__device__ __forceinline__ float swz_xor(float v) {   // lane l gets lane l ^ M's value (M < 32)
    return __uint_as_float(__builtin_amdgcn_ds_swizzle(__float_as_uint(v), (M << 10) | 0x1f));
}
__device__ __forceinline__ float fold_cells(float v) {
    v += swz_xor<4>(v);
    v += swz_xor<8>(v);
    v += swz_xor<16>(v);
    return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ void coef8(const float *p, float (&f)[8]) {
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

struct TailArgs {
    int64_t N, x_stride;
    int HW;
    const uint4 *y, *hprev;                    // the last unit's Y and its input H (residual; NULL: one unit)
    const float *alpha, *beta, *x, *head_p, *head_v;
    float *policy, *value, *pooled;            // forward: outputs; backward: value and pooled are read
    const float *dpolicy, *dvalue, *mean;      // backward
    float4 *gm;
    double *part, *wpart;                      // [gridDim.x][32][2], [gridDim.x][kHeadW]
};

// one sample's staged operands: Y, H and x[:, 0] at the lane's cells (clamped loads issue back to back)
template <bool RES>
struct TailSample {
    uint4 y[kNCh], h[RES ? kNCh : 1];
    float x0[kNCh];
    __device__ __forceinline__ void load(const TailArgs &a, int64_t n, int lane, int nch) {
#pragma unroll
        for (int k = 0; k < kNCh; ++k) {
            const int j = min(k * 64 + lane, nch - 1);
            y[k] = a.y[n * nch + j];
            if constexpr (RES) h[k] = a.hprev[n * nch + j];
            x0[k] = a.x[n * a.x_stride + (j >> 2)];
        }
    }
    // relu([float(H) +] float(Y) alpha + beta) of chunk k, and float(Y)
    __device__ __forceinline__ void out(int k, const float *coef_s, int g, float (&o)[8], float (&yv)[8]) const {
        float hv[8], al[8], be[8];
        unpack8(y[k], yv);
        if constexpr (RES) unpack8(h[k], hv);
        coef8(coef_s + 8 * g, al);
        coef8(coef_s + kCo + 8 * g, be);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float t = yv[e] * al[e] + be[e];
            if constexpr (RES) t = hv[e] + t;
            o[e] = relu(t);
        }
    }
};

__device__ __forceinline__ void tail_constants(const TailArgs &a, float *coef_s, float *head_s, bool with_mean) {
    if (threadIdx.x < 2 * kCo) coef_s[threadIdx.x] = threadIdx.x < kCo ? a.alpha[threadIdx.x] : a.beta[threadIdx.x - kCo];
    else if (with_mean && threadIdx.x < 3 * kCo) coef_s[threadIdx.x] = a.mean[threadIdx.x - 2 * kCo];
    for (int i = threadIdx.x; i < kHeadW; i += kThreads)
        head_s[i] = i < kActions * kCo ? a.head_p[i] : a.head_v[i - kActions * kCo];
    __syncthreads();
}

template <bool RES>
__global__ __launch_bounds__(kThreads) void torus_bf16_heads_fwd_kernel(TailArgs a) {
    __shared__ __attribute__((aligned(16))) float coef_s[2 * kCo];
    __shared__ __attribute__((aligned(16))) float head_s[kHeadW];
    const int HW = a.HW, nch = 4 * HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane & 3;
    const float fhw = (float)HW;
    tail_constants(a, coef_s, head_s, false);
    TailSample<RES> s;
    for (int64_t n = (int64_t)blockIdx.x * kNW + wave; n < a.N; n += (int64_t)gridDim.x * kNW) {
        s.load(a, n, lane, nch);
        float hh[8], ha[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) hh[e] = ha[e] = 0.f;
#pragma unroll
        for (int k = 0; k < kNCh; ++k) {
            if (opaque(k * 64 + lane) < nch) {
                float o[8], yv[8];
                s.out(k, coef_s, opaque(g), o, yv);   // the coefficients are read per chunk, not held
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    hh[e] += o[e] * s.x0[k];
                    ha[e] += o[e];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hh[e] = fold_cells(hh[e]);
            ha[e] = fold_cells(ha[e]) / fhw;   // sum, then divide: hrl_torus_head_pool's mean
        }
        if (lane < 4) {
            float4 *ph = reinterpret_cast<float4 *>(a.pooled + n * (2 * kCo) + 8 * g);
            ph[0] = make_float4(hh[0], hh[1], hh[2], hh[3]);
            ph[1] = make_float4(hh[4], hh[5], hh[6], hh[7]);
            ph[kCo / 4] = make_float4(ha[0], ha[1], ha[2], ha[3]);
            ph[kCo / 4 + 1] = make_float4(ha[4], ha[5], ha[6], ha[7]);
        }
        // the head products in fp64 (exact products, 32 / 64 terms), rounded once
        double r[kActions + 1];
#pragma unroll
        for (int k = 0; k <= kActions; ++k) r[k] = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = 8 * g + e;
#pragma unroll
            for (int k = 0; k <= kActions; ++k) r[k] += (double)head_s[k * kCo + c] * (double)hh[e];
            r[kActions] += (double)head_s[(kActions + 1) * kCo + c] * (double)ha[e];
        }
#pragma unroll
        for (int k = 0; k <= kActions; ++k) {
            r[k] += __shfl_xor(r[k], 1, 64);
            r[k] += __shfl_xor(r[k], 2, 64);
        }
        if (lane < kActions)
            a.policy[n * kActions + lane] = (float)(lane == 0 ? r[0] : lane == 1 ? r[1] : lane == 2 ? r[2] : r[3]);
        if (lane == kActions) a.value[n] = tanhf((float)r[kActions]);
    }
}

template <bool RES>
__global__ __launch_bounds__(kThreads) void torus_bf16_heads_bwd_kernel(TailArgs a) {
    __shared__ __attribute__((aligned(16))) float coef_s[3 * kCo];   // alpha | beta | mean
    __shared__ __attribute__((aligned(16))) float head_s[kHeadW];
    __shared__ double red[kNW * kCo * 2];
    __shared__ double wred[kNW * kHeadW];
    const int HW = a.HW, nch = 4 * HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane & 3;
    const float fhw = (float)HW;
    tail_constants(a, coef_s, head_s, true);
    // the lane's backward sum across samples: channel 8 g + (i & 7), term i >> 3, i = lane >> 2
    double sum = 0.0, wp0 = 0.0, wp1 = 0.0, wv = 0.0;
    TailSample<RES> s;
    for (int64_t n = (int64_t)blockIdx.x * kNW + wave; n < a.N; n += (int64_t)gridDim.x * kNW) {
        s.load(a, n, lane, nch);
        float dp[kActions];
#pragma unroll
        for (int k = 0; k < kActions; ++k) dp[k] = a.dpolicy ? a.dpolicy[n * kActions + k] : 0.f;
        const float val = a.value[n];
        const float dv = (a.dvalue ? a.dvalue[n] : 0.f) * (1.f - val * val);
        // dW_p[k][c] (lanes 0-31: k = 0, 1; lanes 32-63: k = 2, 3; c = lane & 31) and dW_v[lane]
        const float ph = a.pooled[n * (2 * kCo) + (lane & 31)], pl = a.pooled[n * (2 * kCo) + lane];
        wp0 += (double)(lane < 32 ? dp[0] : dp[2]) * (double)ph;
        wp1 += (double)(lane < 32 ? dp[1] : dp[3]) * (double)ph;
        wv += (double)dv * (double)pl;
        // the pool's adjoint for the lane's channels: g[q][c] = dhead[c] x0[q] + davg[c] / HW
        float dh[8], da[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = 8 * g + e;
            double t = (double)dv * (double)head_s[kActions * kCo + c];   // five exact products, one rounding
#pragma unroll
            for (int k = 0; k < kActions; ++k) t += (double)head_s[k * kCo + c] * (double)dp[k];
            dh[e] = (float)t;
            da[e] = (dv * head_s[(kActions + 1) * kCo + c]) / fhw;   // hrl_torus_head_unpool's davg / HW
        }
        float t1[8], t2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t1[i] = t2[i] = 0.f;
#pragma unroll
        for (int k = 0; k < kNCh; ++k) {
            const int j = opaque(k * 64 + lane);
            if (j < nch) {
                float o[8], yv[8], v[8], mu[8];
                s.out(k, coef_s, j & 3, o, yv);   // j & 3 = g: the coefficients are read per chunk, not held
                coef8(coef_s + 2 * kCo + 8 * (j & 3), mu);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[e] = bf_round(o[e]) > 0.f ? dh[e] * s.x0[k] + da[e] : 0.f;   // masked_sums' mask
                    t1[e] += v[e];
                    t2[e] += v[e] * (yv[e] - mu[e]);
                }
                a.gm[(n * nch + j) * 2] = make_float4(v[0], v[1], v[2], v[3]);
                a.gm[(n * nch + j) * 2 + 1] = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
        // the lane's fp32 sums over its cells go to fp64 as masked_sums' do, then fold over the 16 lanes of the
        // channel group; each lane keeps one of the 16 sums
        double pick = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const double f1 = fold16<4>((double)t1[e]), f2 = fold16<4>((double)t2[e]);
            pick = (lane >> 2) == e ? f1 : ((lane >> 2) == 8 + e ? f2 : pick);
        }
        sum += pick;
    }
    red[(wave * kCo + 8 * g + ((lane >> 2) & 7)) * 2 + (lane >> 5)] = sum;
    wred[wave * kHeadW + 2 * (lane >> 5) * kCo + (lane & 31)] = wp0;
    wred[wave * kHeadW + (2 * (lane >> 5) + 1) * kCo + (lane & 31)] = wp1;
    wred[wave * kHeadW + kActions * kCo + lane] = wv;
    __syncthreads();
    if (threadIdx.x < 2 * kCo) {
        double t = 0.0;
        for (int w = 0; w < kNW; ++w) t += red[w * kCo * 2 + threadIdx.x];
        a.part[(int64_t)blockIdx.x * kCo * 2 + threadIdx.x] = t;
    }
    if (threadIdx.x < kHeadW) {
        double t = 0.0;
        for (int w = 0; w < kNW; ++w) t += wred[w * kHeadW + threadIdx.x];
        a.wpart[(int64_t)blockIdx.x * kHeadW + threadIdx.x] = t;
    }
}

// fold the workgroups' head-weight partials in a fixed order: dW_p (4, 32) then dW_v (1, 64)
__global__ __launch_bounds__(kHeadW) void torus_bf16_heads_fold_kernel(const double *__restrict__ wpart, int nparts,
                                                                       float *__restrict__ dwp, float *__restrict__ dwv) {
    const int i = threadIdx.x;
    double t = 0.0;
    for (int w = 0; w < nparts; ++w) t += wpart[(int64_t)w * kHeadW + i];
    if (i < kActions * kCo) dwp[i] = (float)t;
    else dwv[i - kActions * kCo] = (float)t;
}

int status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)e;
}
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool shape_ok(int64_t N, int64_t H, int64_t W) {
    return N >= 1 && N < ((int64_t)1 << 31) && H >= 1 && W >= 1 && H * W <= kMaxCells;
}
// the fused tail's entries take N = 0 (no launch)
bool tail_shape_ok(int64_t N, int64_t H, int64_t W) {
    return N >= 0 && N < ((int64_t)1 << 31) && H >= 1 && W >= 1 && H * W <= kMaxCells;
}
// every conv-role launch (and the sums kernel) writes this many partial rows: one grid for all of them
int conv_grid(int64_t N) {
    const int64_t blocks = (N + kNW - 1) / kNW;
    return (int)(blocks < kGridConv ? blocks : kGridConv);
}
int wgrad_grid(int64_t N) {
    const int64_t blocks = (N + kWW - 1) / kWW;
    return (int)(blocks < kGridWgrad ? blocks : kGridWgrad);
}

}  // namespace

extern "C" {

int64_t hrl_torus_bf16_pack_bytes(int64_t units) {
    return (units < 1 || units > kMaxUnits) ? -1 : units * 2 * kWWords * 4;
}

int64_t hrl_torus_bf16_workspace_bytes(int64_t N) { return N < 1 ? -1 : (int64_t)wgrad_grid(N) * kPart * 4; }

int64_t hrl_torus_bf16_stats_blocks(int64_t N) { return N < 1 ? -1 : conv_grid(N); }

int hrl_torus_bf16_pack(const float *const *weights, int64_t units, int64_t stem_cin, void *pack, int64_t pack_bytes,
                        void *stream) {
    if (!weights || !pack || hrl_torus_bf16_pack_bytes(units) < 0 || pack_bytes < hrl_torus_bf16_pack_bytes(units) ||
        (stem_cin != kStemC && stem_cin != kCo) || !aligned16(pack))
        return HRL_EINVAL;
    PackArgs a{};
    for (int u = 0; u < units; ++u) {
        if (!weights[u]) return HRL_EINVAL;
        a.w[u] = weights[u];
    }
    a.units = (int)units; a.stem_cin = (int)stem_cin; a.out = static_cast<uint32_t *>(pack);
    const int total = (int)units * 2 * kWWords;
    hipLaunchKernelGGL(torus_bf16_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return status();
}

int hrl_torus_bf16_unit_forward(const float *x, const void *y_prev, const void *h_prev, const float *alpha,
                                const float *beta, void *h, int64_t N, int64_t H, int64_t W, const void *pack,
                                int64_t unit, const float *bias, void *y, double *part, void *stream) {
    if (!shape_ok(N, H, W) || !pack || unit < 0 || unit >= kMaxUnits || !bias || !y || !part || !aligned16(pack) ||
        !aligned16(y))
        return HRL_EINVAL;
    if (x) {
        if (unit != 0 || y_prev || h_prev || h) return HRL_EINVAL;
    } else if (!y_prev || !alpha || !beta || !h || unit < 1 || !aligned16(y_prev) || !aligned16(h) || !aligned16(h_prev)) {
        return HRL_EINVAL;
    }
    ConvArgs a{};
    a.N = N; a.H = (int)H; a.W = (int)W; a.wpk = static_cast<const uint32_t *>(pack) + unit * 2 * kWWords;
    a.x = x; a.yprev = static_cast<const uint4 *>(y_prev); a.hprev = static_cast<const uint4 *>(h_prev);
    a.alpha = alpha; a.beta = beta; a.hout = static_cast<uint4 *>(h); a.bias = bias; a.out = static_cast<uint4 *>(y);
    a.part = part;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(conv_grid(N)), block(kThreads);
    if (x) hipLaunchKernelGGL((torus_bf16_conv_kernel<STEM, false>), grid, block, 0, s, a);
    else if (h_prev) hipLaunchKernelGGL((torus_bf16_conv_kernel<PRO2, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((torus_bf16_conv_kernel<PRO1, false>), grid, block, 0, s, a);
    return status();
}

int hrl_torus_bf16_output(const void *y, const void *h_prev, const float *alpha, const float *beta, int64_t N,
                          int64_t H, int64_t W, float *out, void *stream) {
    if (!shape_ok(N, H, W) || !y || !alpha || !beta || !out || !aligned16(y) || !aligned16(h_prev)) return HRL_EINVAL;
    const int64_t blocks = (N + 3) / 4;
    hipLaunchKernelGGL(bn_bf16_output_kernel, dim3((int)(blocks < 2048 ? blocks : 2048)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint4 *>(y),
                       static_cast<const uint4 *>(h_prev), alpha, beta, N, (int)(H * W), out);
    return status();
}

int hrl_torus_bf16_masked_sums(const float *g, const float *out, const void *y, const float *mean, int64_t N,
                               int64_t H, int64_t W, float *gm, double *part, void *stream) {
    if (!shape_ok(N, H, W) || !g || !out || !y || !mean || !gm || !part || !aligned16(y) || !aligned16(gm))
        return HRL_EINVAL;
    // conv_grid(N) rows, as every other producer of `part`; 4 waves walk N with that grid
    hipLaunchKernelGGL(bn_bf16_masked_sums_kernel, dim3(conv_grid(N)), dim3(256), 0, static_cast<hipStream_t>(stream), g,
                       out, static_cast<const uint4 *>(y), mean, N, (int)(H * W), reinterpret_cast<float4 *>(gm), part);
    return status();
}

int hrl_torus_bf16_wgrad_bn(const float *x, const void *h, int64_t N, int64_t H, int64_t W, const void *y,
                            const void *g, int g_fp32, const float *alpha, const float *beta, int residual,
                            const float *gamma, const float *save_mean, const float *save_invstd, const float *kcoef,
                            const float *gmean, void *dy, float *dweight, float *dbias, void *workspace,
                            int64_t workspace_bytes, void *stream) {
    if (!shape_ok(N, H, W) || (x == nullptr) == (h == nullptr) || !y || !g || !alpha || !beta || !save_mean ||
        !save_invstd || !kcoef || !gmean || !dy || !dweight || !workspace)
        return HRL_EINVAL;
    if (x && residual) return HRL_EINVAL;
    if (workspace_bytes < hrl_torus_bf16_workspace_bytes(N)) return HRL_EINVAL;
    for (const void *p : {h, y, g, (const void *)dy})
        if (!aligned16(p)) return HRL_EINVAL;
    WgArgs a{};
    a.N = N; a.H = (int)H; a.W = (int)W; a.x = x; a.h = static_cast<const uint4 *>(h);
    a.y = static_cast<const uint4 *>(y); a.g = g; a.alpha = alpha; a.beta = beta; a.mean = save_mean;
    a.invstd = save_invstd; a.gamma = gamma; a.kcoef = kcoef; a.gmean = gmean; a.residual = residual != 0;
    a.dy = static_cast<uint4 *>(dy); a.partial = static_cast<float *>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int grid = wgrad_grid(N);
    const dim3 block(kWThreads);
    if (x) {
        if (g_fp32) hipLaunchKernelGGL((torus_bf16_wgrad_kernel<true, true>), dim3(grid), block, 0, s, a);
        else hipLaunchKernelGGL((torus_bf16_wgrad_kernel<true, false>), dim3(grid), block, 0, s, a);
    } else {
        if (g_fp32) hipLaunchKernelGGL((torus_bf16_wgrad_kernel<false, true>), dim3(grid), block, 0, s, a);
        else hipLaunchKernelGGL((torus_bf16_wgrad_kernel<false, false>), dim3(grid), block, 0, s, a);
    }
    int rc = status();
    if (rc) return rc;
    hipLaunchKernelGGL(torus_bf16_wgrad_reduce_kernel, dim3((kPart + 255) / 256), dim3(256), 0, s, a.partial, grid,
                       x ? kStemC : kCo, dweight, dbias);
    return status();
}

int hrl_torus_bf16_unit_input_grad(const void *dy, int64_t N, int64_t H, int64_t W, const void *pack, int64_t unit,
                                   const void *g, int g_fp32, const void *h_next, void *dh, const void *h_mask,
                                   const void *y_prev, const float *mean_prev, double *part, void *stream) {
    if (!shape_ok(N, H, W) || !dy || !pack || unit < 1 || unit >= kMaxUnits || !g || (!g_fp32 && !h_next) || !dh ||
        !h_mask || !y_prev || !mean_prev || !part)
        return HRL_EINVAL;
    for (const void *p : {dy, pack, g, h_next, (const void *)dh, h_mask, y_prev})
        if (!aligned16(p)) return HRL_EINVAL;
    ConvArgs a{};
    a.N = N; a.H = (int)H; a.W = (int)W;
    a.wpk = static_cast<const uint32_t *>(pack) + (unit * 2 + 1) * kWWords;
    a.in = static_cast<const uint4 *>(dy); a.out = static_cast<uint4 *>(dh); a.part = part; a.gnext = g;
    a.hnext = static_cast<const uint4 *>(h_next); a.hmask = static_cast<const uint4 *>(h_mask);
    a.ymask = static_cast<const uint4 *>(y_prev); a.mean = mean_prev;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(conv_grid(N)), block(kThreads);
    if (g_fp32) hipLaunchKernelGGL((torus_bf16_conv_kernel<ADJ, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((torus_bf16_conv_kernel<ADJ, false>), grid, block, 0, s, a);
    return status();
}

int64_t hrl_torus_bf16_heads_workspace_bytes(int64_t N) {
    return N < 0 ? -1 : (N == 0 ? 0 : (int64_t)conv_grid(N) * kHeadW * 8);
}

int hrl_torus_bf16_heads_forward(const void *y, const void *h_prev, const float *alpha, const float *beta,
                                 const float *x, int64_t x_stride, const float *head_p, const float *head_v, int64_t N,
                                 int64_t H, int64_t W, float *policy, float *value, float *pooled, void *stream) {
    if (!tail_shape_ok(N, H, W) || !y || !alpha || !beta || !x || x_stride < H * W || !head_p || !head_v || !policy ||
        !value || !pooled || !aligned16(y) || !aligned16(h_prev) || !aligned16(pooled))
        return HRL_EINVAL;
    if (N == 0) return HRL_OK;
    TailArgs a{};
    a.N = N; a.x_stride = x_stride; a.HW = (int)(H * W); a.y = static_cast<const uint4 *>(y);
    a.hprev = static_cast<const uint4 *>(h_prev); a.alpha = alpha; a.beta = beta; a.x = x; a.head_p = head_p;
    a.head_v = head_v; a.policy = policy; a.value = value; a.pooled = pooled;
    const dim3 grid(conv_grid(N)), block(kThreads);   // two resident workgroups per CU, as the conv launches
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (h_prev) hipLaunchKernelGGL(torus_bf16_heads_fwd_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(torus_bf16_heads_fwd_kernel<false>, grid, block, 0, s, a);
    return status();
}

int hrl_torus_bf16_heads_backward(const float *dpolicy, const float *dvalue, const float *value, const float *pooled,
                                  const float *head_p, const float *head_v, const float *x, int64_t x_stride,
                                  const void *y, const void *h_prev, const float *alpha, const float *beta,
                                  const float *save_mean, int64_t N, int64_t H, int64_t W, float *gm, double *part,
                                  float *dhead_p, float *dhead_v, void *workspace, int64_t workspace_bytes,
                                  void *stream) {
    if (!tail_shape_ok(N, H, W) || !value || !pooled || !head_p || !head_v || !x || x_stride < H * W || !y || !alpha ||
        !beta || !save_mean || !gm || !part || !dhead_p || !dhead_v || !workspace ||
        workspace_bytes < hrl_torus_bf16_heads_workspace_bytes(N) || !aligned16(y) || !aligned16(h_prev) ||
        !aligned16(gm) || !aligned16(workspace))
        return HRL_EINVAL;
    if (N == 0) return HRL_OK;
    TailArgs a{};
    a.N = N; a.x_stride = x_stride; a.HW = (int)(H * W); a.y = static_cast<const uint4 *>(y);
    a.hprev = static_cast<const uint4 *>(h_prev); a.alpha = alpha; a.beta = beta; a.x = x; a.head_p = head_p;
    a.head_v = head_v; a.value = const_cast<float *>(value); a.pooled = const_cast<float *>(pooled);
    a.dpolicy = dpolicy; a.dvalue = dvalue; a.mean = save_mean; a.gm = reinterpret_cast<float4 *>(gm); a.part = part;
    a.wpart = static_cast<double *>(workspace);
    // conv_grid(N) rows of part, as every other producer of it
    const dim3 grid(conv_grid(N)), block(kThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (h_prev) hipLaunchKernelGGL(torus_bf16_heads_bwd_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(torus_bf16_heads_bwd_kernel<false>, grid, block, 0, s, a);
    const int rc = status();
    if (rc) return rc;
    hipLaunchKernelGGL(torus_bf16_heads_fold_kernel, dim3(1), dim3(kHeadW), 0, s, a.wpart, (int)grid.x, dhead_p, dhead_v);
    return status();
}

}  // extern "C"
