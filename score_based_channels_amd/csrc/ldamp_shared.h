// Device code and launch helpers of Learned D-AMP shared by inference (ldamp.hip) and training (ldamp_train.hip): stage and tensor tables,
// the convolution / transposed-convolution stages with their InstanceNorm + LeakyReLU, prep, finish and the U-Net launch list.
#pragma once
#include "common.h"
#include "host_params.h"
#include "philox.h"
#include "reduce.h"
#include <math.h>
#include <string.h>
#include <string>

namespace sbc {
namespace {

constexpr int NT = 64, NR = 16, PIX = NT * NR;
constexpr int N_TENSORS = 19;
constexpr float IN_EPS = 1e-5f, LRELU = 0.2f;

// stages of one evaluation, in workspace order; floats per image = C * H * W
enum Stage {
    S_R = 0,  // the denoiser's input r, complex interleaved [64][16][2]
    S_X,      // norm(r), planar [2][64][16]
    S_D0A, S_D0, S_P0, S_D1A, S_D1, S_P1, S_D2A, S_D2, S_P2, S_BA, S_BB,
    S_T0, S_U0A, S_U0, S_T1, S_U1A, S_U1, S_T2, S_U2A, S_U2,
    S_STAT,   // (mean_re, std_re, mean_im, std_im)
    N_STAGES
};
struct StageDim { int c, h, w; };
constexpr StageDim STAGE_DIM[N_STAGES] = {
    {2, 64, 16}, {2, 64, 16},
    {16, 64, 16}, {16, 64, 16}, {16, 32, 8}, {32, 32, 8}, {32, 32, 8}, {32, 16, 4}, {64, 16, 4}, {64, 16, 4}, {64, 8, 2}, {128, 8, 2}, {128, 8, 2},
    {64, 16, 4}, {64, 16, 4}, {64, 16, 4}, {32, 32, 8}, {32, 32, 8}, {32, 32, 8}, {16, 64, 16}, {16, 64, 16}, {16, 64, 16},
    {4, 1, 1}};
constexpr int64_t stage_floats(int s) { return (int64_t)STAGE_DIM[s].c * STAGE_DIM[s].h * STAGE_DIM[s].w; }
constexpr int64_t stage_prefix(int s) { return s == 0 ? 0 : stage_prefix(s - 1) + stage_floats(s - 1); }
constexpr int64_t EVAL_FLOATS = stage_prefix(N_STAGES);
// behind the 2B evaluations of a run: z [B][64][16][2], eps [B], directions [unrolls][B][64][16][2] (only without caller directions)
inline int64_t run_extra_floats(int B, int unrolls) { return (int64_t)B * (2 * PIX + 16) + (int64_t)unrolls * B * 2 * PIX; }

// tensors of one net, in the order of the reference module's state_dict; offsets into the net's weight block
struct TensorSpec { const char* name; int numel; };
constexpr TensorSpec TENSORS[N_TENSORS] = {
    {"unet.down_sample_layers.0.layers.0.weight", 16 * 2 * 9},   {"unet.down_sample_layers.0.layers.4.weight", 16 * 16 * 9},
    {"unet.down_sample_layers.1.layers.0.weight", 32 * 16 * 9},  {"unet.down_sample_layers.1.layers.4.weight", 32 * 32 * 9},
    {"unet.down_sample_layers.2.layers.0.weight", 64 * 32 * 9},  {"unet.down_sample_layers.2.layers.4.weight", 64 * 64 * 9},
    {"unet.conv.layers.0.weight", 128 * 64 * 9},                 {"unet.conv.layers.4.weight", 128 * 128 * 9},
    {"unet.up_conv.0.layers.0.weight", 64 * 128 * 9},            {"unet.up_conv.0.layers.4.weight", 64 * 64 * 9},
    {"unet.up_conv.1.layers.0.weight", 32 * 64 * 9},             {"unet.up_conv.1.layers.4.weight", 32 * 32 * 9},
    {"unet.up_conv.2.0.layers.0.weight", 16 * 32 * 9},           {"unet.up_conv.2.0.layers.4.weight", 16 * 16 * 9},
    {"unet.up_conv.2.1.weight", 2 * 16},                         {"unet.up_conv.2.1.bias", 2},
    {"unet.up_transpose_conv.0.layers.0.weight", 128 * 64 * 4},  {"unet.up_transpose_conv.1.layers.0.weight", 64 * 32 * 4},
    {"unet.up_transpose_conv.2.layers.0.weight", 32 * 16 * 4}};
enum { W_D0A, W_D0B, W_D1A, W_D1B, W_D2A, W_D2B, W_BA, W_BB, W_U0A, W_U0B, W_U1A, W_U1B, W_U2A, W_U2B, W_FIN, W_FINB, W_T0, W_T1, W_T2 };
constexpr int64_t tensor_prefix(int t) { return t == 0 ? 0 : tensor_prefix(t - 1) + TENSORS[t - 1].numel; }
constexpr int64_t NET_FLOATS = tensor_prefix(N_TENSORS);

// ---- reductions over a workgroup, fixed order (the wavefront's: reduce.h) ---------------------------------------------------------
// 256 threads; red: 4 floats of LDS.  Every thread gets the result.
template <bool MAX>
__device__ __forceinline__ float block_reduce256(float v, float* red) {
    v = MAX ? wave_max(v) : wave_sum(v);
    __syncthreads();                                   // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : ((red[0] + red[1]) + red[2]) + red[3];
}

// InstanceNorm2d (biased variance, eps inside the root, no affine) + LeakyReLU(0.2) of CT channels of HW pixels held in LDS
// (out_s [CT][HW]), stored to out [CT][HW] (global) and, with POOL, their 2 x 2 mean pool to pool [CT][HW / 4].  A wavefront per channel.
template <int CT, int H, int W, int THREADS, bool POOL>
__device__ __forceinline__ void inorm_lrelu_store(float* out_s, float* __restrict__ out, float* __restrict__ pool) {
    constexpr int HW = H * W, NW = THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < CT; c += NW) {
        float* x = out_s + c * HW;
        float s = 0.f;
        SBC_NO_VEC for (int i = lane; i < HW; i += 64) s += x[i];
        const float mean = wave_sum(s) * (1.f / HW);
        float q = 0.f;
        SBC_NO_VEC for (int i = lane; i < HW; i += 64) { const float d = x[i] - mean; q += d * d; }
        const float rstd = 1.f / sqrtf(wave_sum(q) * (1.f / HW) + IN_EPS);
        SBC_NO_VEC for (int i = lane; i < HW; i += 64) {
            float v = (x[i] - mean) * rstd;
            v = v >= 0.f ? v : LRELU * v;
            out[c * HW + i] = v;
            if (POOL) x[i] = v;
        }
    }
    if (POOL) {
        __syncthreads();
        constexpr int HP = H / 2, WPL = W / 2;
        SBC_NO_VEC for (int e = threadIdx.x; e < CT * HP * WPL; e += THREADS) {
            const int c = e / (HP * WPL), p = e % (HP * WPL), y = p / WPL, xx = p % WPL;
            const float* s = out_s + c * HW + (2 * y) * W + 2 * xx;
            pool[e] = (((s[0] + s[1]) + s[W]) + s[W + 1]) * 0.25f;
        }
    }
}

// Training: the same, and the channels' 1 / sqrt(var + eps) to rstd_out [CT]; the backward needs them and cannot recover them from `out`.
// A copy, not a flag of the function above: sharing one body between the inference kernels and their training twins changed the register
// allocation of the inference kernels, whose device code stays what it was (tools/device_code_diff.py).
template <int CT, int H, int W, int THREADS, bool POOL>
__device__ __forceinline__ void inorm_lrelu_store_rstd(float* out_s, float* __restrict__ out, float* __restrict__ pool, float* __restrict__ rstd_out) {
    constexpr int HW = H * W, NW = THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < CT; c += NW) {
        float* x = out_s + c * HW;
        float s = 0.f;
        SBC_NO_VEC for (int i = lane; i < HW; i += 64) s += x[i];
        const float mean = wave_sum(s) * (1.f / HW);
        float q = 0.f;
        SBC_NO_VEC for (int i = lane; i < HW; i += 64) { const float d = x[i] - mean; q += d * d; }
        const float rstd = 1.f / sqrtf(wave_sum(q) * (1.f / HW) + IN_EPS);
        if (lane == 0) rstd_out[c] = rstd;
        SBC_NO_VEC for (int i = lane; i < HW; i += 64) {
            float v = (x[i] - mean) * rstd;
            v = v >= 0.f ? v : LRELU * v;
            out[c * HW + i] = v;
            if (POOL) x[i] = v;
        }
    }
    if (POOL) {
        __syncthreads();
        constexpr int HP = H / 2, WPL = W / 2;
        SBC_NO_VEC for (int e = threadIdx.x; e < CT * HP * WPL; e += THREADS) {
            const int c = e / (HP * WPL), p = e % (HP * WPL), y = p / WPL, xx = p % WPL;
            const float* s = out_s + c * HW + (2 * y) * W + 2 * xx;
            pool[e] = (((s[0] + s[1]) + s[W]) + s[W + 1]) * 0.25f;
        }
    }
}

// ---- 3 x 3 convolution (pad 1, no bias) + InstanceNorm + LeakyReLU [+ 2 x 2 mean pool] -----------------------------------------
// Input channels [0, CA) from srcA, [CA, CA + CB) from srcB (the concat of the up path is never materialised).  grid (COUT / CT, N);
// a thread owns PXT vertically adjacent pixels x OCT output channels; the input streams through LDS in chunks of CC channels.
template <int H, int W, int CA, int CB, int COUT, int CT, int OCT, int PXT, int CC, bool POOL>
struct Conv3 {
    static constexpr int HW = H * W, CIN = CA + CB, NPG = HW / PXT, NOG = CT / OCT, THREADS = NPG * NOG;
    static constexpr int HP = H + 2, WP = W + 2;
    static constexpr int IN_FLOATS = CC * HP * WP, OUT_FLOATS = CT * HW;
    static constexpr int BUF_FLOATS = IN_FLOATS > OUT_FLOATS ? IN_FLOATS : OUT_FLOATS;
    static constexpr int W_FLOATS = CT * CC * 9;
    static_assert(THREADS % 64 == 0 && THREADS <= 256, "whole wavefronts");
    static_assert(CA % CC == 0 && CB % CC == 0 && COUT % CT == 0 && CT % OCT == 0 && H % PXT == 0, "tiling");
    static_assert((BUF_FLOATS + W_FLOATS) * 4 <= 64 * 1024, "static LDS");
};

template <int H, int W, int CA, int CB, int COUT, int CT, int OCT, int PXT, int CC, bool POOL>
__global__ __launch_bounds__((H * W / PXT) * (CT / OCT)) void conv3_kernel(const float* __restrict__ srcA, const float* __restrict__ srcB,
                                                                          const float* __restrict__ wgt, float* __restrict__ out,
                                                                          float* __restrict__ pool) {
    using K = Conv3<H, W, CA, CB, COUT, CT, OCT, PXT, CC, POOL>;
    __shared__ float buf[K::BUF_FLOATS];
    __shared__ float w_s[K::W_FLOATS];
    const int tid = threadIdx.x, n = blockIdx.y, oc0 = blockIdx.x * CT;
    const int pg = tid % K::NPG, og = tid / K::NPG;
    const int x = pg % W, y0 = (pg / W) * PXT;

    float acc[OCT][PXT];
#pragma unroll
    for (int o = 0; o < OCT; ++o)
#pragma unroll
        for (int p = 0; p < PXT; ++p) acc[o][p] = 0.f;

    for (int c0 = 0; c0 < K::CIN; c0 += CC) {
        const float* src = c0 < CA ? srcA + ((size_t)n * CA + c0) * K::HW : srcB + ((size_t)n * CB + (c0 - CA)) * K::HW;
        __syncthreads();
        for (int e = tid; e < K::IN_FLOATS; e += K::THREADS) {
            const int ci = e / (K::HP * K::WP), rem = e % (K::HP * K::WP), yy = rem / K::WP - 1, xx = rem % K::WP - 1;
            buf[e] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? src[ci * K::HW + yy * W + xx] : 0.f;
        }
        for (int e = tid; e < K::W_FLOATS; e += K::THREADS) {
            const int oc = e / (CC * 9), rem = e % (CC * 9);
            w_s[e] = wgt[((size_t)(oc0 + oc) * K::CIN + c0) * 9 + rem];
        }
        __syncthreads();
        float part[OCT][PXT];
#pragma unroll
        for (int o = 0; o < OCT; ++o)
#pragma unroll
            for (int p = 0; p < PXT; ++p) part[o][p] = 0.f;
#pragma unroll 2
        for (int ci = 0; ci < CC; ++ci) {
            float v[PXT + 2][3];
#pragma unroll
            for (int r = 0; r < PXT + 2; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) v[r][k] = buf[ci * K::HP * K::WP + (y0 + r) * K::WP + x + k];
#pragma unroll
            for (int o = 0; o < OCT; ++o) {
                const float* w9 = w_s + ((og * OCT + o) * CC + ci) * 9;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float wv = w9[ky * 3 + kx];
#pragma unroll
                        for (int p = 0; p < PXT; ++p) part[o][p] = fmaf(v[p + ky][kx], wv, part[o][p]);
                    }
            }
        }
#pragma unroll
        for (int o = 0; o < OCT; ++o)
#pragma unroll
            for (int p = 0; p < PXT; ++p) acc[o][p] += part[o][p];
    }
    __syncthreads();                                   // everyone is done with the input chunk: buf becomes the output tile
#pragma unroll
    for (int o = 0; o < OCT; ++o)
#pragma unroll
        for (int p = 0; p < PXT; ++p) buf[(og * OCT + o) * K::HW + (y0 + p) * W + x] = acc[o][p];
    __syncthreads();
    inorm_lrelu_store<CT, H, W, K::THREADS, POOL>(buf, out + ((size_t)n * COUT + oc0) * K::HW,
                                                  POOL ? pool + ((size_t)n * COUT + oc0) * (K::HW / 4) : nullptr);
}

// training: the same stage (a copy of conv3_kernel, see inorm_lrelu_store_rstd), and rstd [N][COUT] of its InstanceNorm
template <int H, int W, int CA, int CB, int COUT, int CT, int OCT, int PXT, int CC, bool POOL>
__global__ __launch_bounds__((H * W / PXT) * (CT / OCT)) void conv3_train_kernel(const float* __restrict__ srcA, const float* __restrict__ srcB,
                                                                                const float* __restrict__ wgt, float* __restrict__ out,
                                                                                float* __restrict__ pool, float* __restrict__ rstd) {
    using K = Conv3<H, W, CA, CB, COUT, CT, OCT, PXT, CC, POOL>;
    __shared__ float buf[K::BUF_FLOATS];
    __shared__ float w_s[K::W_FLOATS];
    const int tid = threadIdx.x, n = blockIdx.y, oc0 = blockIdx.x * CT;
    const int pg = tid % K::NPG, og = tid / K::NPG;
    const int x = pg % W, y0 = (pg / W) * PXT;

    float acc[OCT][PXT];
#pragma unroll
    for (int o = 0; o < OCT; ++o)
#pragma unroll
        for (int p = 0; p < PXT; ++p) acc[o][p] = 0.f;

    for (int c0 = 0; c0 < K::CIN; c0 += CC) {
        const float* src = c0 < CA ? srcA + ((size_t)n * CA + c0) * K::HW : srcB + ((size_t)n * CB + (c0 - CA)) * K::HW;
        __syncthreads();
        for (int e = tid; e < K::IN_FLOATS; e += K::THREADS) {
            const int ci = e / (K::HP * K::WP), rem = e % (K::HP * K::WP), yy = rem / K::WP - 1, xx = rem % K::WP - 1;
            buf[e] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? src[ci * K::HW + yy * W + xx] : 0.f;
        }
        for (int e = tid; e < K::W_FLOATS; e += K::THREADS) {
            const int oc = e / (CC * 9), rem = e % (CC * 9);
            w_s[e] = wgt[((size_t)(oc0 + oc) * K::CIN + c0) * 9 + rem];
        }
        __syncthreads();
        float part[OCT][PXT];
#pragma unroll
        for (int o = 0; o < OCT; ++o)
#pragma unroll
            for (int p = 0; p < PXT; ++p) part[o][p] = 0.f;
#pragma unroll 2
        for (int ci = 0; ci < CC; ++ci) {
            float v[PXT + 2][3];
#pragma unroll
            for (int r = 0; r < PXT + 2; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) v[r][k] = buf[ci * K::HP * K::WP + (y0 + r) * K::WP + x + k];
#pragma unroll
            for (int o = 0; o < OCT; ++o) {
                const float* w9 = w_s + ((og * OCT + o) * CC + ci) * 9;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float wv = w9[ky * 3 + kx];
#pragma unroll
                        for (int p = 0; p < PXT; ++p) part[o][p] = fmaf(v[p + ky][kx], wv, part[o][p]);
                    }
            }
        }
#pragma unroll
        for (int o = 0; o < OCT; ++o)
#pragma unroll
            for (int p = 0; p < PXT; ++p) acc[o][p] += part[o][p];
    }
    __syncthreads();                                   // everyone is done with the input chunk: buf becomes the output tile
#pragma unroll
    for (int o = 0; o < OCT; ++o)
#pragma unroll
        for (int p = 0; p < PXT; ++p) buf[(og * OCT + o) * K::HW + (y0 + p) * W + x] = acc[o][p];
    __syncthreads();
    inorm_lrelu_store_rstd<CT, H, W, K::THREADS, POOL>(buf, out + ((size_t)n * COUT + oc0) * K::HW,
                                                       POOL ? pool + ((size_t)n * COUT + oc0) * (K::HW / 4) : nullptr, rstd + (size_t)n * COUT + oc0);
}

// ---- ConvTranspose2d 2 x 2 stride 2 (no bias) + InstanceNorm + LeakyReLU ------------------------------------------------------
// out[oc][2y + dy][2x + dx] = sum_ci in[ci][y][x] w[ci][oc][dy][dx].  grid (COUT / CT, N); a thread owns one input pixel x OCT output
// channels (4 outputs each); input and weights stream through LDS in chunks of CC input channels.
template <int HI, int WI, int CIN, int COUT, int CT, int OCT, int CC>
struct TConv {
    static constexpr int HWI = HI * WI, HWO = 4 * HWI, NOG = CT / OCT, THREADS = HWI * NOG;
    static constexpr int IN_FLOATS = CC * HWI, W_FLOATS = CC * CT * 4, OUT_FLOATS = CT * HWO;
    static constexpr int BUF_FLOATS = IN_FLOATS + W_FLOATS > OUT_FLOATS ? IN_FLOATS + W_FLOATS : OUT_FLOATS;
    static_assert(THREADS % 64 == 0 && THREADS <= 256 && CIN % CC == 0 && COUT % CT == 0 && CT % OCT == 0, "tiling");
    static_assert(BUF_FLOATS * 4 <= 64 * 1024, "static LDS");
};

template <int HI, int WI, int CIN, int COUT, int CT, int OCT, int CC>
__global__ __launch_bounds__(HI * WI * (CT / OCT)) void tconv_kernel(const float* __restrict__ src, const float* __restrict__ wgt,
                                                                     float* __restrict__ out) {
    using K = TConv<HI, WI, CIN, COUT, CT, OCT, CC>;
    __shared__ __align__(16) float buf[K::BUF_FLOATS];
    float* in_s = buf;
    float* w_s = buf + K::IN_FLOATS;
    const int tid = threadIdx.x, n = blockIdx.y, oc0 = blockIdx.x * CT;
    const int px = tid % K::HWI, og = tid / K::HWI;
    float acc[OCT][4];
#pragma unroll
    for (int o = 0; o < OCT; ++o)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[o][k] = 0.f;
    for (int c0 = 0; c0 < CIN; c0 += CC) {
        __syncthreads();
        for (int e = tid; e < K::IN_FLOATS; e += K::THREADS) in_s[e] = src[((size_t)n * CIN + c0) * K::HWI + e];
        for (int e = tid; e < K::W_FLOATS; e += K::THREADS) {
            const int ci = e / (CT * 4), rem = e % (CT * 4);
            w_s[e] = wgt[((size_t)(c0 + ci) * COUT + oc0) * 4 + rem];
        }
        __syncthreads();
        float part[OCT][4];
#pragma unroll
        for (int o = 0; o < OCT; ++o)
#pragma unroll
            for (int k = 0; k < 4; ++k) part[o][k] = 0.f;
#pragma unroll 4
        for (int ci = 0; ci < CC; ++ci) {
            const float v = in_s[ci * K::HWI + px];
#pragma unroll
            for (int o = 0; o < OCT; ++o) {
                const float4 w4 = *reinterpret_cast<const float4*>(w_s + (ci * CT + og * OCT + o) * 4);
                part[o][0] = fmaf(v, w4.x, part[o][0]);
                part[o][1] = fmaf(v, w4.y, part[o][1]);
                part[o][2] = fmaf(v, w4.z, part[o][2]);
                part[o][3] = fmaf(v, w4.w, part[o][3]);
            }
        }
#pragma unroll
        for (int o = 0; o < OCT; ++o)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[o][k] += part[o][k];
    }
    __syncthreads();
    const int y = px / WI, x = px % WI;
    constexpr int WO = 2 * WI;
#pragma unroll
    for (int o = 0; o < OCT; ++o) {
        float* d = buf + (og * OCT + o) * K::HWO + (2 * y) * WO + 2 * x;
        d[0] = acc[o][0]; d[1] = acc[o][1]; d[WO] = acc[o][2]; d[WO + 1] = acc[o][3];
    }
    __syncthreads();
    inorm_lrelu_store<CT, 2 * HI, 2 * WI, K::THREADS, false>(buf, out + ((size_t)n * COUT + oc0) * K::HWO, nullptr);
}

// training: the same stage (a copy of tconv_kernel), and rstd [N][COUT]
template <int HI, int WI, int CIN, int COUT, int CT, int OCT, int CC>
__global__ __launch_bounds__(HI * WI * (CT / OCT)) void tconv_train_kernel(const float* __restrict__ src, const float* __restrict__ wgt,
                                                                           float* __restrict__ out, float* __restrict__ rstd) {
    using K = TConv<HI, WI, CIN, COUT, CT, OCT, CC>;
    __shared__ __align__(16) float buf[K::BUF_FLOATS];
    float* in_s = buf;
    float* w_s = buf + K::IN_FLOATS;
    const int tid = threadIdx.x, n = blockIdx.y, oc0 = blockIdx.x * CT;
    const int px = tid % K::HWI, og = tid / K::HWI;
    float acc[OCT][4];
#pragma unroll
    for (int o = 0; o < OCT; ++o)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[o][k] = 0.f;
    for (int c0 = 0; c0 < CIN; c0 += CC) {
        __syncthreads();
        for (int e = tid; e < K::IN_FLOATS; e += K::THREADS) in_s[e] = src[((size_t)n * CIN + c0) * K::HWI + e];
        for (int e = tid; e < K::W_FLOATS; e += K::THREADS) {
            const int ci = e / (CT * 4), rem = e % (CT * 4);
            w_s[e] = wgt[((size_t)(c0 + ci) * COUT + oc0) * 4 + rem];
        }
        __syncthreads();
        float part[OCT][4];
#pragma unroll
        for (int o = 0; o < OCT; ++o)
#pragma unroll
            for (int k = 0; k < 4; ++k) part[o][k] = 0.f;
#pragma unroll 4
        for (int ci = 0; ci < CC; ++ci) {
            const float v = in_s[ci * K::HWI + px];
#pragma unroll
            for (int o = 0; o < OCT; ++o) {
                const float4 w4 = *reinterpret_cast<const float4*>(w_s + (ci * CT + og * OCT + o) * 4);
                part[o][0] = fmaf(v, w4.x, part[o][0]);
                part[o][1] = fmaf(v, w4.y, part[o][1]);
                part[o][2] = fmaf(v, w4.z, part[o][2]);
                part[o][3] = fmaf(v, w4.w, part[o][3]);
            }
        }
#pragma unroll
        for (int o = 0; o < OCT; ++o)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[o][k] += part[o][k];
    }
    __syncthreads();
    const int y = px / WI, x = px % WI;
    constexpr int WO = 2 * WI;
#pragma unroll
    for (int o = 0; o < OCT; ++o) {
        float* d = buf + (og * OCT + o) * K::HWO + (2 * y) * WO + 2 * x;
        d[0] = acc[o][0]; d[1] = acc[o][1]; d[WO] = acc[o][2]; d[WO + 1] = acc[o][3];
    }
    __syncthreads();
    inorm_lrelu_store_rstd<CT, 2 * HI, 2 * WI, K::THREADS, false>(buf, out + ((size_t)n * COUT + oc0) * K::HWO, nullptr, rstd + (size_t)n * COUT + oc0);
}

// ---- prep, finish and the directions: kernels of ldamp.hip ---------------------------------------------------------------------------
// The argument records live in this unnamed namespace (their names are part of the kernels' symbols), so the launchers that other units
// call take them as untyped pointers: ldamp_launch_prep(const PrepArgs*), ldamp_launch_finish(const FinishArgs*).
struct PrepArgs {
    const float* r_in;     // evaluation entry: the denoiser's input [N][64][16][2]; run: NULL
    const float* P;        // [B][Np][64] complex
    const float* z;        // [B][Np][16] complex
    const float* h;        // [B][64][16] complex; NULL = 0 (first unroll)
    const float* eig;      // [B]
    const float* dirs;     // [B][64][16][2] of this unroll
    float* eps;            // [B]
    float* eps_log;        // [B] of this unroll or NULL
    float* r;              // S_R [N][64][16][2]
    float* x;              // S_X [N][2][64][16]
    float* stat;           // S_STAT [N][4]
    int B, Np;
};

struct FinishArgs {
    const float* u2;       // S_U2 [N][16][1024]
    const float* r;        // S_R
    const float* stat;     // S_STAT
    const float* w;        // [2][16]
    const float* bias;     // [2]
    float* h_out;          // [B][64][16][2]: the clean evaluation's output
    int damp;              // 0: evaluation only
    const float* P;        // [B][Np][64]
    const float* Y;        // [B][Np][16]
    float* z;              // [B][Np][16], updated in place
    const float* eps;      // [B]
    const float* dirs;     // [B][64][16][2]
    const float* Htrue;    // [B][64][16][2] or NULL
    float* nmse;           // [B] or NULL: written when `last`
    float* h_log;          // this unroll's [B][64][16][2] or NULL
    float* z_log;          // this unroll's [B][Np][16][2] or NULL
    float* div_log;        // this unroll's [B] or NULL
    int B, Np, last;
};

}  // namespace
// grid: B workgroups (prep, finish) / (B, unrolls) (directions); defined in ldamp.hip
void ldamp_launch_prep(const void* prep_args, int B, hipStream_t s);
void ldamp_launch_finish(const void* finish_args, int B, hipStream_t s);
void ldamp_launch_dirs(float* d, uint64_t seed, int64_t sample0, int unroll0, int B, int unrolls, hipStream_t s);
namespace {

// ---- host ---------------------------------------------------------------------------------------------------------------------
template <bool TRAIN, int H, int W, int CA, int CB, int COUT, int CT, int OCT, int PXT, int CC, bool POOL>
void conv3(const float* a, const float* b, const float* w, float* out, float* pool, int N, hipStream_t s, float* rstd) {
    using K = Conv3<H, W, CA, CB, COUT, CT, OCT, PXT, CC, POOL>;
    if constexpr (TRAIN) hipLaunchKernelGGL((conv3_train_kernel<H, W, CA, CB, COUT, CT, OCT, PXT, CC, POOL>), dim3(COUT / CT, N), dim3(K::THREADS), 0, s, a, b, w, out, pool, rstd);
    else hipLaunchKernelGGL((conv3_kernel<H, W, CA, CB, COUT, CT, OCT, PXT, CC, POOL>), dim3(COUT / CT, N), dim3(K::THREADS), 0, s, a, b, w, out, pool);
}
template <bool TRAIN, int HI, int WI, int CIN, int COUT, int CT, int OCT, int CC>
void tconv(const float* src, const float* w, float* out, int N, hipStream_t s, float* rstd) {
    using K = TConv<HI, WI, CIN, COUT, CT, OCT, CC>;
    if constexpr (TRAIN) hipLaunchKernelGGL((tconv_train_kernel<HI, WI, CIN, COUT, CT, OCT, CC>), dim3(COUT / CT, N), dim3(K::THREADS), 0, s, src, w, out, rstd);
    else hipLaunchKernelGGL((tconv_kernel<HI, WI, CIN, COUT, CT, OCT, CC>), dim3(COUT / CT, N), dim3(K::THREADS), 0, s, src, w, out);
}

struct Ws {
    float* base;
    int N;
    float* at(int stage) const { return base + stage_prefix(stage) * N; }
};

// rstd of the 17 normalised stages (every stage between S_X and S_STAT that is not a pool): stage s of N images at rstd_prefix(s) * N, [N][C]
constexpr bool stage_normed(int s) { return s >= S_D0A && s <= S_U2 && s != S_P0 && s != S_P1 && s != S_P2; }
constexpr int64_t rstd_prefix(int s) { return s == 0 ? 0 : rstd_prefix(s - 1) + (stage_normed(s - 1) ? STAGE_DIM[s - 1].c : 0); }
constexpr int64_t RSTD_FLOATS = rstd_prefix(N_STAGES);

// the U-Net of N normalised images: S_X -> S_U2 (17 launches).  TRAIN: the training twins of the kernels, which also store rstd.
template <bool TRAIN = false>
void unet(const float* net, const Ws& ws, hipStream_t s, float* rstd = nullptr) {
    const int N = ws.N;
    auto w = [&](int t) { return net + tensor_prefix(t); };
    auto R = [&](int st) { return TRAIN ? rstd + rstd_prefix(st) * N : nullptr; };
    //            H   W   CA  CB  COUT CT OCT PXT CC POOL
    conv3<TRAIN, 64, 16, 2, 0, 16, 8, 8, 4, 2, false>(ws.at(S_X), nullptr, w(W_D0A), ws.at(S_D0A), nullptr, N, s, R(S_D0A));
    conv3<TRAIN, 64, 16, 16, 0, 16, 8, 8, 4, 8, true>(ws.at(S_D0A), nullptr, w(W_D0B), ws.at(S_D0), ws.at(S_P0), N, s, R(S_D0));
    conv3<TRAIN, 32, 8, 16, 0, 32, 16, 4, 4, 8, false>(ws.at(S_P0), nullptr, w(W_D1A), ws.at(S_D1A), nullptr, N, s, R(S_D1A));
    conv3<TRAIN, 32, 8, 32, 0, 32, 16, 4, 4, 8, true>(ws.at(S_D1A), nullptr, w(W_D1B), ws.at(S_D1), ws.at(S_P1), N, s, R(S_D1));
    conv3<TRAIN, 16, 4, 32, 0, 64, 32, 4, 4, 8, false>(ws.at(S_P1), nullptr, w(W_D2A), ws.at(S_D2A), nullptr, N, s, R(S_D2A));
    conv3<TRAIN, 16, 4, 64, 0, 64, 32, 4, 4, 8, true>(ws.at(S_D2A), nullptr, w(W_D2B), ws.at(S_D2), ws.at(S_P2), N, s, R(S_D2));
    conv3<TRAIN, 8, 2, 64, 0, 128, 32, 4, 2, 8, false>(ws.at(S_P2), nullptr, w(W_BA), ws.at(S_BA), nullptr, N, s, R(S_BA));
    conv3<TRAIN, 8, 2, 128, 0, 128, 32, 4, 2, 8, false>(ws.at(S_BA), nullptr, w(W_BB), ws.at(S_BB), nullptr, N, s, R(S_BB));
    tconv<TRAIN, 8, 2, 128, 64, 32, 2, 32>(ws.at(S_BB), w(W_T0), ws.at(S_T0), N, s, R(S_T0));
    conv3<TRAIN, 16, 4, 64, 64, 64, 32, 4, 4, 8, false>(ws.at(S_T0), ws.at(S_D2), w(W_U0A), ws.at(S_U0A), nullptr, N, s, R(S_U0A));
    conv3<TRAIN, 16, 4, 64, 0, 64, 32, 4, 4, 8, false>(ws.at(S_U0A), nullptr, w(W_U0B), ws.at(S_U0), nullptr, N, s, R(S_U0));
    tconv<TRAIN, 16, 4, 64, 32, 16, 4, 32>(ws.at(S_U0), w(W_T1), ws.at(S_T1), N, s, R(S_T1));
    conv3<TRAIN, 32, 8, 32, 32, 32, 16, 4, 4, 8, false>(ws.at(S_T1), ws.at(S_D1), w(W_U1A), ws.at(S_U1A), nullptr, N, s, R(S_U1A));
    conv3<TRAIN, 32, 8, 32, 0, 32, 16, 4, 4, 8, false>(ws.at(S_U1A), nullptr, w(W_U1B), ws.at(S_U1), nullptr, N, s, R(S_U1));
    tconv<TRAIN, 32, 8, 32, 16, 8, 8, 32>(ws.at(S_U1), w(W_T2), ws.at(S_T2), N, s, R(S_T2));
    conv3<TRAIN, 64, 16, 16, 16, 16, 8, 8, 4, 8, false>(ws.at(S_T2), ws.at(S_D0), w(W_U2A), ws.at(S_U2A), nullptr, N, s, R(S_U2A));
    conv3<TRAIN, 64, 16, 16, 0, 16, 8, 8, 4, 8, false>(ws.at(S_U2A), nullptr, w(W_U2B), ws.at(S_U2), nullptr, N, s, R(S_U2));
}

}  // namespace
}  // namespace sbc
