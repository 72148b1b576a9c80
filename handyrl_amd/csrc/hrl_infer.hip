// hrl_infer.hip — the TicTacToe net's whole eval forward as ONE launch, grouped over checkpoints (gfx950).
//
// SimpleConv2dModel (envs/tictactoe.py): stem conv 3->32 + ReLU, L x [conv 32->32 -> BatchNorm(eval) -> ReLU],
// policy / value heads (1x1 conv + LeakyReLU(0.1) + bias-free linear, tanh on the value), all on a 3x3 board.
//
// board_infer_pack_kernel (once per inference session) writes everything the forward reads, in the layout it
// reads it, into one pack buffer per net:
//   [stem B fragments 6144 B][stem bias 128 B][heads 1088 B] then per layer [B fragments 55296 B][a, b 256 B]
//   * B fragments are the exact three-way bf16 split (hrl_split.h) of the weights in hrl_conv.hip's layout
//     [tap][co-tile][part h/m/l][lane] x 16 B (lane l: W'[tap][ci = 8(l>>4) + e][co = 16ct + (l&15)], e = 0..7);
//     the stem's are [co-tile][part][lane] over k = ci*9 + tap (27, zero-padded to 32);
//   * a, b are bn_eval_coef_kernel's coefficients (hrl_bn.hip), formed by the same operations.
// board_infer_kernel: one workgroup of 4 waves per 16-row tile; a tile's rows belong to one net (the tiles are
// laid out span by span; the span table travels by value in the kernel arguments).
//   * the 4 waves share the tile's 9 output cells ({4,0}, {1,3}, {5,7}, {2,6,8}: 13/12/12/12 of the 49 (p, q) taps);
//   * a layer's 54 KB of B fragments are staged in LDS; the next layer's are in flight (global -> registers)
//     while this layer's MFMAs run; the activations (16 x 288 fp32) stay in one LDS tile, rewritten in place once
//     every wave has read it (a layer's outputs wait in the accumulators);
//   * arithmetic: six partial products on v_mfma_f32_16x16x32_bf16, smallest terms first, fp32 accumulation;
//     BN + ReLU as y*a + b, v < 0 ? 0 : v; the heads on the VALU.
//   LDS 78,464 B per workgroup: two workgroups per CU; N = 4096 is 256 tiles, one per CU.
// The tile's forward itself (pack layout constants, stem, chain, heads) is hrl_board_fwd.h, shared with the
// whole-game self-play kernel (hrl_boardplay.hip).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrl_nn.h"
#include "../../include/hrl_targets.h"
#include "hrl_board_fwd.h"

namespace {

constexpr int kMaxNets = 64;               // nets per launch (the span table is a kernel argument)

struct PackArgs {
    const float *stem_w, *stem_b;
    const float *conv_w[kMaxLayers], *bn_w[kMaxLayers], *bn_b[kMaxLayers], *bn_mean[kMaxLayers], *bn_var[kMaxLayers];
    double eps[kMaxLayers];
    const float *w1p, *b1p, *w1v, *b1v, *fcp, *fcv;
    int layers;
    uint32_t *out;
};

__global__ __launch_bounds__(kThreads) void board_infer_pack_kernel(PackArgs a) {
    const int total = kLayer0Off + a.layers * kLayerWords;
    const int w = blockIdx.x * kThreads + threadIdx.x;
    if (w >= total) return;
    uint32_t v;
    if (w < kStemFragWords) {
        const int d = w & 3, l = (w >> 2) & 63, f = w >> 8;          // f = ct*3 + part
        const int part = f % 3, ct = f / 3;
        const int k = 8 * (l >> 4) + 2 * d, co = ct * 16 + (l & 15);
        const float w0 = k < kObs ? a.stem_w[co * kObs + k] : 0.f;
        const float w1 = k + 1 < kObs ? a.stem_w[co * kObs + k + 1] : 0.f;
        v = split_part(w0, part) | (split_part(w1, part) << 16);
    } else if (w < kHeadOff) {
        v = __float_as_uint(a.stem_b[w - kStemFragWords]);
    } else if (w < kLayer0Off) {
        const int i = w - kHeadOff;
        float x = 0.f;
        if (i < kHB1p) x = a.w1p[i];
        else if (i < kHW1v) x = a.b1p[i - kHB1p];
        else if (i < kHB1v) x = a.w1v[i - kHW1v];
        else if (i < kHFcp) x = a.b1v[0];
        else if (i < kHFcv) x = a.fcp[i - kHFcp];
        else if (i < kHeadFloats) x = a.fcv[i - kHFcv];
        v = __float_as_uint(x);
    } else {
        const int r = w - kLayer0Off;
        const int layer = r / kLayerWords, i = r - layer * kLayerWords;
        if (i < kLayerFragWords) {
            const int d = i & 3, l = (i >> 2) & 63, f = i >> 8;      // f = (tap*2 + ct)*3 + part
            const int part = f % 3, tc = f / 3;
            const int tap = tc >> 1, ct = tc & 1;
            const int ci = 8 * (l >> 4) + 2 * d, co = ct * 16 + (l & 15);
            const float *cw = a.conv_w[layer];                       // (co, ci, ky, kx), tap = ky*3 + kx
            const float w0 = cw[(co * kC + ci) * 9 + tap];
            const float w1 = cw[(co * kC + ci + 1) * 9 + tap];
            v = split_part(w0, part) | (split_part(w1, part) << 16);
        } else {
            // bn_eval_coef_kernel's operations (hrl_bn.hip)
            const int c = (i - kLayerFragWords) & (kC - 1);
            const float invstd = (float)(1.0 / sqrt((double)a.bn_var[layer][c] + a.eps[layer]));
            const float al = invstd * a.bn_w[layer][c];
            const float be = a.bn_b[layer][c] - a.bn_mean[layer][c] * al;
            v = __float_as_uint(i - kLayerFragWords < kC ? al : be);
        }
    }
    a.out[w] = v;
}

struct Spans {
    int32_t off[kMaxNets + 1];
};

__global__ __launch_bounds__(kThreads) void board_infer_kernel(const uint8_t *__restrict__ packs,
                                                               int64_t pack_stride, int K, Spans sp,
                                                               const float *__restrict__ obs, int layers,
                                                               float *__restrict__ policy,
                                                               float *__restrict__ value) {
    __shared__ __attribute__((aligned(16))) uint32_t w_lds_u[kLayerFragWords];   // 54 KB
    __shared__ float act[kTile * kStride];                                       // 18.1 KB
    __shared__ float obs_lds[kTile * kObs];
    __shared__ float head_w[kHeadWords];
    __shared__ float h_lds[kTile * kHMid];

    // the tile's net and rows: tiles are laid out span by span
    int b = blockIdx.x, net = 0, row0 = 0, valid = 0;
    for (int k = 0; k < K; ++k) {
        const int len = sp.off[k + 1] - sp.off[k];
        const int nt = (len + kTile - 1) / kTile;
        if (b < nt) {
            net = k;
            row0 = sp.off[k] + b * kTile;
            valid = len - b * kTile;
            break;
        }
        b -= nt;
    }
    if (valid <= 0) return;   // (unreachable: the grid is the tile count)
    if (valid > kTile) valid = kTile;

    const uint32_t *pack = reinterpret_cast<const uint32_t *>(packs + (int64_t)net * pack_stride);
    const int tid = threadIdx.x;

    // hrl_board_fwd.h; the observation tile: rows past the span read as zeros
    board_forward_tile(pack, layers, obs_lds, act, w_lds_u, head_w, h_lds, tid, [&] {
        for (int i = tid; i < kTile * kObs; i += kThreads) {
            const int r = i / kObs;
            obs_lds[i] = r < valid ? obs[(int64_t)row0 * kObs + i] : 0.f;
        }
    });

    if (tid < kTile * 10) {
        const int row = tid / 10, o = tid - row * 10;
        if (row < valid) {
            if (o < kA)
                policy[(int64_t)(row0 + row) * kA + o] = board_policy_out(h_lds, head_w, row, o);
            else
                value[row0 + row] = board_value_out(h_lds, head_w, row);
        }
    }
}

}  // namespace

extern "C" {

int64_t hrl_board_infer_pack_bytes(int64_t layers) {
    if (layers < 1 || layers > kMaxLayers) return 0;
    return 4 * ((int64_t)kLayer0Off + layers * kLayerWords);
}

int hrl_board_infer_pack(const float *stem_w, const float *stem_b, const float *const *conv_w,
                         const float *const *bn_w, const float *const *bn_b, const float *const *bn_mean,
                         const float *const *bn_var, const double *bn_eps, int64_t layers, const float *w1p,
                         const float *b1p, const float *w1v, const float *b1v, const float *fcp, const float *fcv,
                         void *pack, void *stream) {
    if (!stem_w || !stem_b || !conv_w || !bn_w || !bn_b || !bn_mean || !bn_var || !bn_eps || layers < 1 ||
        layers > kMaxLayers || !w1p || !b1p || !w1v || !b1v || !fcp || !fcv || !pack ||
        (reinterpret_cast<uintptr_t>(pack) & 15))
        return HRL_EINVAL;
    PackArgs a{};
    for (int l = 0; l < layers; ++l) {
        if (!conv_w[l] || !bn_w[l] || !bn_b[l] || !bn_mean[l] || !bn_var[l]) return HRL_EINVAL;
        a.conv_w[l] = conv_w[l];
        a.bn_w[l] = bn_w[l];
        a.bn_b[l] = bn_b[l];
        a.bn_mean[l] = bn_mean[l];
        a.bn_var[l] = bn_var[l];
        a.eps[l] = bn_eps[l];
    }
    a.stem_w = stem_w; a.stem_b = stem_b;
    a.w1p = w1p; a.b1p = b1p; a.w1v = w1v; a.b1v = b1v; a.fcp = fcp; a.fcv = fcv;
    a.layers = (int)layers;
    a.out = static_cast<uint32_t *>(pack);
    const int total = kLayer0Off + (int)layers * kLayerWords;
    hipLaunchKernelGGL(board_infer_pack_kernel, dim3((total + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

int hrl_board_infer(const void *pack, int64_t pack_stride_bytes, int64_t K, const int64_t *span, const float *obs,
                    int64_t N, int64_t layers, float *policy, float *value, void *stream) {
    if (!pack || !span || !obs || !policy || !value || layers < 1 || layers > kMaxLayers || N < 0 ||
        N > 0x7fffffff - kTile || K < 1 || K > kMaxNets || (reinterpret_cast<uintptr_t>(pack) & 15) ||
        (pack_stride_bytes & 15) || (K > 1 && pack_stride_bytes < hrl_board_infer_pack_bytes(layers)))
        return HRL_EINVAL;
    if (span[0] != 0 || span[K] != N) return HRL_EINVAL;
    Spans sp{};
    int64_t tiles = 0;
    for (int k = 0; k < K; ++k) {
        if (span[k + 1] < span[k]) return HRL_EINVAL;
        tiles += (span[k + 1] - span[k] + kTile - 1) / kTile;
        sp.off[k + 1] = (int32_t)span[k + 1];
    }
    if (N == 0) return HRL_OK;
    hipLaunchKernelGGL(board_infer_kernel, dim3((unsigned)tiles), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint8_t *>(pack), pack_stride_bytes,
                       (int)K, sp, obs, (int)layers, policy, value);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HRL_OK : HRL_ELAUNCH_BASE - (int)err;
}

}  // extern "C"
