// hrl_geesenet.hip — GeeseNet's eval forward with BatchNorm folded and the weights packed once (gfx950).
//
// GeeseNet (envs/hungry_geese.py): stem TorusConv2d(17, 32) + BN + ReLU, `layers` residual units
// h = relu(h + bn(conv(h))) on a torus board of at most 80 cells, then h_head = sum_q h * x[:, 0],
// h_avg = mean_q h, policy = head_p . h_head, value = tanh(head_v . [h_head, h_avg]).
//
// geese_infer_pack_kernel (once per inference session) writes what the forward reads, in the layout it reads it:
//   per unit [B operands 36,864 B][alpha, beta, conv bias 384 B], then [head_p (4, 32)][head_v (1, 64)] 768 B
//   * the B operands are hrl_torus.hip's packed fp32 weights [tap][k-step 8][co-tile 2][64] (lane l of k-step s:
//     W[co = 16 ct + (l & 15)][ci = 4 s + (l >> 4)][tap]), the stem's input channels 17..31 zero.  They stay fp32
//     and are split per tap: the three bf16 parts of a unit are 55 KB, which with eight 15 KB sample images is
//     past the CU's 160 KB of LDS (the reason hrl_torus.hip's training kernel gives);
//   * alpha, beta are bn_eval_coef_kernel's coefficients (hrl_bn.hip), formed by the same operations.
// geese_unit_kernel<STEM, TAIL, NW>: one launch per unit, torus_conv_ps_kernel's conv (hrl_torus.hip: one sample
//   per wave, NW waves sharing the packed weights, the sample's image split once into bf16 parts in LDS, the exact
//   split on v_mfma_f32_16x16x32_bf16, the next sample's loads in flight during the MFMAs) with the inference
//   epilogue: the accumulators go to the wave's LDS tile as (acc + bias) * alpha + beta, and the store pass writes
//   h' = relu([h +] tile) -- the residual h is the kernel's own input, re-read by the lane that stores the same
//   float4 (issued before the tile is written), so h is updated in place and no conv output reaches memory.
//   TAIL (the last unit): the finished sample stays in the tile; the wave pools it as torus_head_pool_kernel does
//   (the same sums in the same order) and applies both heads: h_13 is never written, a forward is layers + 1
//   launches.  No statistics, no partial rows, nothing shared between workgroups.
//   NW = 8: one workgroup per CU (160.6 KB of LDS), N <= 2048 is one sample per wave.  NW = 2: 66.6 KB, two
//   workgroups per CU, for small batches (four times the workgroups, one wave per SIMD).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrl_nn.h"
#include "../../include/hrl_targets.h"
#include "hrl_split.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
using hrl_split::split8;
using hrl_split::mfma_split;

constexpr int kCo = 32;
constexpr int kStemC = 17;
constexpr int kActions = 4;
constexpr int kMT = 5;                        // 16-cell tiles: boards of at most 80 cells
constexpr int kMaxCells = kMT * 16;
constexpr int kS = 81;                        // fp32 tile row stride (odd: 16 consecutive rows -> 16 banks)
constexpr int kTaps = 9;
constexpr int kTile = kCo * kS;
constexpr int kRowDw = 48;                    // dwords per cell row of the split image (hrl_torus.hip)
constexpr int kImgDw = kMaxCells * kRowDw;    // dwords per wave image (15 KB)
constexpr int kPU = 4 * kMaxCells / 64;       // staging units per lane
constexpr int kNV = kCo * kMaxCells / 4 / 64; // float4 per lane of an 80-cell sample
constexpr int kNX = kMaxCells / 64 + 1;       // x0 cells per lane
constexpr int kMaxLayers = 16;
constexpr int kMaxUnits = kMaxLayers + 1;

// the pack, in floats
constexpr int kWFloats = kTaps * 8 * 2 * 64;          // 9216
constexpr int kUnitFloats = kWFloats + 3 * kCo;       // + alpha | beta | bias
constexpr int kHeadFloats = kActions * kCo + 2 * kCo; // head_p | head_v
static_assert(kUnitFloats % 4 == 0 && kHeadFloats % 4 == 0, "units and the pack end on 16-byte lines");
static_assert(kImgDw >= kTile + kMaxCells + 2 * kCo, "tile, x0 and the pooled vector live in the image region");

constexpr int kWavesBig = 8, kWavesSmall = 2;
constexpr int kGridBig = 256;      // one workgroup per CU
constexpr int kGridSmall = 512;    // two per CU
constexpr int64_t kSmallN = 1024;  // at or below: the 2-wave form (kGridSmall * kWavesSmall samples in one pass)

__device__ __forceinline__ int fdiv(int e, float inv) { return (int)(((float)e + 0.5f) * inv); }   // hrl_targets.hip

__device__ __forceinline__ int opaque(int i) {
    asm volatile("" : "+v"(i));
    return i;
}

// hrl_torus.hip Quad: the tile slots of the float4 at element 4i of a [c][cell] sample
struct Quad {
    int c0, base, r0;
    __device__ __forceinline__ Quad(int i, int HW, float inv_hw) {
        c0 = fdiv(4 * i, inv_hw);
        r0 = 4 * i - c0 * HW;
        base = c0 * kS + r0;
    }
    __device__ __forceinline__ int slot(int j, int HW) const { return base + j + (r0 + j >= HW ? kS - HW : 0); }
};

__device__ __forceinline__ void lds_fence() {
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS operations done
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float relu(float v) { return v < 0.f ? 0.f : v; }   // NaN stays NaN

__device__ __forceinline__ int ps_row(int cell, int g) { return cell * kRowDw + 4 * (g ^ ((cell >> 2) & 3)); }

// ------------------------------------------------------------------ pack
struct PackArgs {
    const float *conv_w[kMaxUnits], *conv_b[kMaxUnits], *bn_w[kMaxUnits], *bn_b[kMaxUnits], *bn_mean[kMaxUnits],
        *bn_var[kMaxUnits];
    double eps[kMaxUnits];
    const float *head_p, *head_v;
    int units;
    float *out;
};

__global__ __launch_bounds__(256) void geese_infer_pack_kernel(PackArgs a) {
    const int total = a.units * kUnitFloats + kHeadFloats;
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= total) return;
    const int u = w / kUnitFloats, i = w - u * kUnitFloats;
    float v = 0.f;
    if (u >= a.units) {
        v = i < kActions * kCo ? a.head_p[i] : a.head_v[i - kActions * kCo];
    } else if (i < kWFloats) {
        // torus_pack_kernel's layout (hrl_torus.hip)
        const int cin = u == 0 ? kStemC : kCo;
        const int l = i & 63, ct = (i >> 6) & 1, s = (i >> 7) & 7, tap = i >> 10;
        const int oc = ct * 16 + (l & 15), ic = s * 4 + (l >> 4);
        if (ic < cin) v = a.conv_w[u][(oc * cin + ic) * kTaps + tap];
    } else {
        // bn_eval_coef_kernel's operations (hrl_bn.hip)
        const int j = i - kWFloats, c = j & (kCo - 1);
        const float invstd = (float)(1.0 / sqrt((double)a.bn_var[u][c] + a.eps[u]));
        const float al = invstd * a.bn_w[u][c];
        const float be = a.bn_b[u][c] - a.bn_mean[u][c] * al;
        v = j < kCo ? al : (j < 2 * kCo ? be : a.conv_b[u][c]);
    }
    a.out[w] = v;
}

// ------------------------------------------------------------------ one unit
struct UnitArgs {
    const float *unit;     // the unit's pack: B operands | alpha | beta | bias
    const float *src;      // (N, 17 | 32, HW): x (STEM) or h
    float *dst;            // (N, 32, HW); the residual units run with dst == src
    const float *obs;      // TAIL: x (N, 17, HW); plane 0 weights the head pool
    const float *heads;    // TAIL: head_p (4, 32) | head_v (1, 64)
    float *policy, *value; // TAIL: (N, 4), (N, 1)
    int64_t N;
    int H, W;
};

template <bool STEM, bool TAIL, int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW >= 8 ? 2 : 1, 2))) void geese_unit_kernel(UnitArgs a) {
    static_assert(!(STEM && TAIL), "a net has at least one residual unit");
    constexpr int Cin = STEM ? kStemC : kCo;
    constexpr int kThreads = 64 * NW;
    __shared__ __attribute__((aligned(16))) float w_lds[kWFloats];
    __shared__ __attribute__((aligned(16))) uint32_t imgs[NW * kImgDw];
    __shared__ float heads_s[TAIL ? kHeadFloats : 1];
    const int64_t N = a.N;
    const int H = a.H, W = a.W;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int HW = H * W;
    const float inv_hw = 1.0f / (float)HW;
    const int in_elem = Cin * HW;
    const int out_elem = kCo * HW;
    const int nv = out_elem >> 2;
    uint32_t *img = imgs + wave * kImgDw;
    float *tile = reinterpret_cast<float *>(img);

    for (int i = threadIdx.x; i < kWFloats / 4; i += kThreads)
        reinterpret_cast<float4 *>(w_lds)[i] = reinterpret_cast<const float4 *>(a.unit)[i];
    if constexpr (TAIL) {
        for (int i = threadIdx.x; i < kHeadFloats; i += kThreads) heads_s[i] = a.heads[i];
    }

    uint32_t nbp[kMT][3];   // (row (r + d - 1) * W) | (column (c + d - 1)) << 16 of the lane's A cells
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
        int q = mt * 16 + (lane & 15);
        while (q >= HW) q -= HW;
        const int r = q / W, c = q - r * W;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            int rr = r + d - 1, cc = c + d - 1;
            rr = rr < 0 ? rr + H : (rr >= H ? rr - H : rr);
            cc = cc < 0 ? cc + W : (cc >= W ? cc - W : cc);
            nbp[mt][d] = (uint32_t)(rr * W) | ((uint32_t)cc << 16);
        }
    }
    const int g = lane >> 4;
    float al_v[2], be_v[2], bias_v[2];   // of the lane's output channels 16 ct + (lane & 15)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int co = ct * 16 + (lane & 15);
        al_v[ct] = a.unit[kWFloats + co];
        be_v[ct] = a.unit[kWFloats + kCo + co];
        bias_v[ct] = a.unit[kWFloats + 2 * kCo + co];
    }

    // staging unit u = k * 64 + lane (valid below 4 HW): channels 8 gu .. 8 gu + 7 at cell cu
    float sv[kPU][8];
    auto unit = [&](int k, int &gu, int &cu) {
        const int u = opaque(k * 64 + lane);
        gu = fdiv(u, inv_hw);
        cu = u - gu * HW;
        return u < 4 * HW;
    };
    auto load = [&](const float *src) {
#pragma unroll
        for (int k = 0; k < kPU; ++k) {
            int gu, cu;
            const bool ok = unit(k, gu, cu);
            const float *p = src + (ok ? 8 * gu * HW + cu : 0);
#pragma unroll
            for (int e = 0; e < 8; ++e) sv[k][e] = (!ok || 8 * gu + e < Cin) ? p[e * HW] : 0.f;   // rows >= Cin: 0
        }
    };

    const int64_t stride = (int64_t)gridDim.x * NW;
    int64_t n = (int64_t)blockIdx.x * NW + wave;
    if (n < N) load(a.src + n * in_elem);
    __syncthreads();   // weights (and heads) in LDS

    for (; n < N; n += stride) {
        // the staged sample -> split image
#pragma unroll
        for (int k = 0; k < kPU; ++k) {
            int gu, cu;
            if (unit(k, gu, cu)) {
                uint4 Ah, Am, Al;
                split8(sv[k], Ah, Am, Al);
                uint4 *row = reinterpret_cast<uint4 *>(img + ps_row(cu, gu));
                row[0] = Ah;
                row[4] = Am;
                row[8] = Al;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        lds_fence();
        const int64_t next = n + stride;
        if (next < N) load(a.src + next * in_elem);   // in flight during the MFMAs

        f32x4 acc[kMT][2];
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt) acc[mt][0] = acc[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            uint4 Bh[2], Bm[2], Bl[2];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                float bv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int ci = 8 * g + e;
                    bv[e] = w_lds[((t * 8 + (ci >> 2)) * 2 + ct) * 64 + (ci & 3) * 16 + (lane & 15)];
                }
                split8(bv, Bh[ct], Bm[ct], Bl[ct]);
            }
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) {
                const int cell = (int)(nbp[mt][t / 3] & 0xffffu) + (int)(nbp[mt][t % 3] >> 16);
                const uint4 *row = reinterpret_cast<const uint4 *>(img + ps_row(cell, g));
                const uint4 Ah = row[0], Am = row[4], Al = row[8];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    acc[mt][ct] = mfma_split(Ah, Am, Al, Bh[ct], Bm[ct], Bl[ct], acc[mt][ct]);
            }
        }
        lds_fence();   // every lane's A reads done before the image becomes the output tile

        // the residual h (this sample's input, just read: cache hot) and the pool's x0, issued before the tile pass
        float4 rv[STEM ? 1 : kNV] = {};
        if constexpr (!STEM) {
            const float4 *r4 = reinterpret_cast<const float4 *>(a.src + n * in_elem);
#pragma unroll
            for (int k = 0; k < kNV; ++k) rv[k] = r4[min(k * 64 + lane, nv - 1)];
        }
        float xv[TAIL ? kNX : 1];
        if constexpr (TAIL) {
#pragma unroll
            for (int k = 0; k < kNX; ++k) xv[k] = a.obs[n * (kStemC * HW) + min(k * 64 + lane, HW - 1)];
        }

#pragma unroll
        for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int cell = mt * 16 + (lane >> 4) * 4 + r;
                    const int co = ct * 16 + (lane & 15);
                    if (cell < HW) tile[co * kS + cell] = (acc[mt][ct][r] + bias_v[ct]) * al_v[ct] + be_v[ct];
                }
        lds_fence();

        // h' = relu([h +] bn(conv)): to memory, or (TAIL) back into the tile
        float4 *dst = TAIL ? nullptr : reinterpret_cast<float4 *>(a.dst + n * out_elem);
#pragma unroll
        for (int k = 0; k < kNV; ++k) {
            const int i = opaque(k * 64 + lane);
            if (i < nv) {
                const Quad q(i, HW, inv_hw);
                const float r4[4] = {rv[STEM ? 0 : k].x, rv[STEM ? 0 : k].y, rv[STEM ? 0 : k].z, rv[STEM ? 0 : k].w};
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v = tile[q.slot(j, HW)];
                    if constexpr (!STEM) v = r4[j] + v;
                    o[j] = relu(v);
                    if constexpr (TAIL) tile[q.slot(j, HW)] = o[j];
                }
                if constexpr (!TAIL) dst[i] = make_float4(o[0], o[1], o[2], o[3]);
            }
        }

        if constexpr (TAIL) {
            // torus_head_pool_kernel's sums (hrl_torus.hip), then the two bias-free linears
            float *x0 = tile + kTile, *pooled = x0 + kMaxCells;
#pragma unroll
            for (int k = 0; k < kNX; ++k)
                if (k * 64 + lane < HW) x0[k * 64 + lane] = xv[k];
            lds_fence();
            const int c = lane & 31;
            float s = 0.f;
            if (lane < 32) {
                for (int q = 0; q < HW; ++q) s += tile[c * kS + q] * x0[q];
            } else {
                for (int q = 0; q < HW; ++q) s += tile[c * kS + q];
                s = s / (float)HW;
            }
            pooled[lane] = s;   // [h_head | h_avg]
            lds_fence();
            if (lane < kActions) {
                float p = 0.f;
                for (int k = 0; k < kCo; ++k) p += heads_s[lane * kCo + k] * pooled[k];
                a.policy[n * kActions + lane] = p;
            } else if (lane == kActions) {
                float p = 0.f;
                for (int k = 0; k < 2 * kCo; ++k) p += heads_s[kActions * kCo + k] * pooled[k];
                a.value[n] = tanhf(p);
            }
        }
        lds_fence();   // the tile's reads done before the next image is written
    }
}

int status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)e;
}

bool board_ok(int64_t N, int64_t H, int64_t W) {
    return N >= 0 && H >= 1 && W >= 1 && H * W <= kMaxCells && N * kCo * H * W < ((int64_t)1 << 40);
}

// 0: by batch size (default); 1: always the 8-wave form; 2: always the 2-wave form
int g_form = 0;

template <int NW>
void launch_units(const float *pack, int layers, const float *x, int64_t N, int H, int W, float *policy, float *value,
                  float *h, hipStream_t s) {
    const int64_t blocks = (N + NW - 1) / NW;
    const int cap = NW == kWavesBig ? kGridBig : kGridSmall;
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap)), block(64 * NW);
    UnitArgs a{};
    a.N = N;
    a.H = H;
    a.W = W;
    a.obs = x;
    a.heads = pack + (int64_t)(layers + 1) * kUnitFloats;
    a.policy = policy;
    a.value = value;
    a.dst = h;
    for (int u = 0; u <= layers; ++u) {
        a.unit = pack + (int64_t)u * kUnitFloats;
        a.src = u == 0 ? x : h;
        if (u == 0)
            hipLaunchKernelGGL((geese_unit_kernel<true, false, NW>), grid, block, 0, s, a);
        else if (u < layers)
            hipLaunchKernelGGL((geese_unit_kernel<false, false, NW>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((geese_unit_kernel<false, true, NW>), grid, block, 0, s, a);
    }
}

}  // namespace

extern "C" {

int hrl_geesenet_infer_set_form(int form) {
    const int prev = g_form;
    if (form >= 0 && form <= 2) g_form = form;
    return prev;
}

int64_t hrl_geesenet_infer_pack_bytes(int64_t layers) {
    if (layers < 1 || layers > kMaxLayers) return 0;
    return 4 * ((layers + 1) * kUnitFloats + kHeadFloats);
}

int hrl_geesenet_infer_pack(const float *const *conv_w, const float *const *conv_b, const float *const *bn_w,
                            const float *const *bn_b, const float *const *bn_mean, const float *const *bn_var,
                            const double *bn_eps, int64_t layers, const float *head_p, const float *head_v, void *pack,
                            void *stream) {
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
    a.out = static_cast<float *>(pack);
    const int total = a.units * kUnitFloats + kHeadFloats;
    hipLaunchKernelGGL(geese_infer_pack_kernel, dim3((total + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return status();
}

int64_t hrl_geesenet_infer_workspace_bytes(int64_t N, int64_t H, int64_t W) {
    if (!board_ok(N, H, W)) return -1;
    return N * kCo * H * W * 4;   // h, updated in place
}

int hrl_geesenet_infer(const void *pack, int64_t layers, const float *x, int64_t N, int64_t H, int64_t W,
                       float *policy, float *value, void *ws, int64_t ws_bytes, void *stream) {
    if (!pack || (reinterpret_cast<uintptr_t>(pack) & 15) || layers < 1 || layers > kMaxLayers || !x || !policy ||
        !value || !board_ok(N, H, W))
        return HRL_EINVAL;
    if (N == 0) return HRL_OK;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15) || ws_bytes < hrl_geesenet_infer_workspace_bytes(N, H, W))
        return HRL_EINVAL;
    const bool small = g_form == 2 || (g_form == 0 && N <= kSmallN);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (small)
        launch_units<kWavesSmall>(static_cast<const float *>(pack), (int)layers, x, N, (int)H, (int)W, policy, value,
                                  static_cast<float *>(ws), s);
    else
        launch_units<kWavesBig>(static_cast<const float *>(pack), (int)layers, x, N, (int)H, (int)W, policy, value,
                                static_cast<float *>(ws), s);
    return status();
}

}  // extern "C"
