// WGAN training: src/score_based_channels/train_wgan.py:123-184 on the generator of csrc/wgan.hip (aux_gan.py:58-112, DCGAN_G_Ours) and the
// critic aux_gan.py:9-56 (DCGAN_D), both in training mode, isize = [16, 64], nz 60, nc 2, ngf 128, ndf 64, n_extra = 0 .. 4 for both nets.
//
//     G  dense 60 -> [128][4][16];  layers k = 1 .. L = 2 + n_extra: [nearest x 2,] Conv (5 x 5 + bias | 3 x 3), BatchNorm on BATCH
//        statistics, ReLU;  Conv 5 x 5 128 -> 2 + bias
//     D  layer 0: Conv 4 x 4 / 2 2 -> 64, LeakyReLU 0.2;  layers 1 .. n_extra: Conv 3 x 3 64 -> 64, BatchNorm, LeakyReLU;
//        layer n_extra + 1: Conv 4 x 4 / 2 64 -> 128, BatchNorm, LeakyReLU;  layer M = n_extra + 2: Conv (4, 16) 128 -> 1;  mean over the batch
//
// One launch per layer and direction.  A layer's forward is: raw = conv (+ bias); (mean, var) = batch statistics of raw, running statistics
// updated; pre = (raw - mean) / sqrt(var + eps) * w + b, act = ReLU / LeakyReLU (pre), the signs of pre as bit masks in wgan.hip's layout
// (one word per 32 pixels of a row; a row of 16 pixels has one word of 16 bits).  Its backward: from gact = d loss / d act the sums
// sum dy and sum dy xhat (dy = gact under the mask and slope): the gradients of the BatchNorm bias and weight; draw = d loss / d raw =
// w invstd (dy - mean(dy) - xhat mean(dy xhat)); the weight gradient from draw and the layer's input; the input gradient from draw.
//
// Arithmetic: fp32.  The generator's 128 -> 128 convolutions run on the fp32 matrix cores in all three directions: forward and input
// gradient through conv128_kernel<100 + KS> (wgan.hip), the weight gradient through wgrad128_kernel here.  The critic (18.4 M MAC per sample
// and pass against the generator's 682 M) and the two small ends of the generator run on the vector ALUs.  Every reduction over the batch
// (statistics, BatchNorm sums, the partial weight gradients, the vector-ALU weight gradients) accumulates in float64 in a fixed order;
// convolution sums are fp32 fmaf chains of one input channel (or one 32-pixel tile) added one after the other.  Nothing is atomic: a
// launch sequence run twice gives the same bits.
#include "common.h"
#include "host_params.h"
#include "reduce.h"
#include "wgan_shared.h"
#include <math.h>
#include <string.h>
#include <string>
#include <vector>

namespace sbc {
namespace {
using namespace wgan_shared;                           // the constants, the layers' geometry and the state dict of the generator

constexpr int NDF = 64, MAX_M = MAX_EXTRA + 2;          // the critic's width and its last layer's highest index
constexpr float BN_MOMENTUM = 0.1f;

// ---- batch statistics: per-channel mean and biased variance over B H W, two passes in float64; running statistics ------------------
// grid (C).  running = (1 - 0.1) running + 0.1 (mean | var N / (N - 1)), as nn.BatchNorm2d in training mode.
struct StatArgs {
    const float* x;            // [B][C][HW]
    float* mean; float* var;   // [C]
    float* run_mean; float* run_var;   // [C], updated in place
    int B, C, HW;
};

__global__ __launch_bounds__(256) void bn_stats_kernel(StatArgs a) {
    __shared__ double red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const double N = (double)a.B * a.HW;
    double s = 0.0;
    for (int b = 0; b < a.B; ++b) {
        const float* x = a.x + ((size_t)b * a.C + c) * a.HW;
        for (int p = tid; p < a.HW; p += 256) s += (double)x[p];
    }
    const double m = block_sum256(s, red) / N;
    double q = 0.0;
    for (int b = 0; b < a.B; ++b) {
        const float* x = a.x + ((size_t)b * a.C + c) * a.HW;
        for (int p = tid; p < a.HW; p += 256) {
            const double d = (double)x[p] - m;
            q += d * d;
        }
    }
    q = block_sum256(q, red);
    if (tid == 0) {
#pragma clang fp contract(off)
        const float mean = (float)m, var = (float)(q / N), unbiased = (float)(q / (N - 1.0));
        a.mean[c] = mean;
        a.var[c] = var;
        a.run_mean[c] = (1.f - BN_MOMENTUM) * a.run_mean[c] + BN_MOMENTUM * mean;
        a.run_var[c] = (1.f - BN_MOMENTUM) * a.run_var[c] + BN_MOMENTUM * unbiased;
    }
}

// ---- normalise + activation: pre = (raw - mean) / sqrt(var + eps) * w + b (bn) or raw; act = pre > 0 ? pre : slope pre; the signs ----
// one thread per element, grid (B C HW / 256); W divides 64, so a wavefront holds whole rows and a row's mask words come out of one ballot
struct ActArgs {
    const float* raw; const float* mean; const float* var; const float* w; const float* b;
    float* pre;                // or NULL
    float* act; uint32_t* mask;
    int C, HW, W, bn;
    float slope;
};

__global__ __launch_bounds__(256) void bn_act_kernel(ActArgs a) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)((e / a.HW) % a.C), lane = threadIdx.x & 63;
    float v = a.raw[e];
    if (a.bn) {
#pragma clang fp contract(off)                           // the reference's order, every operation rounded
        v = (v - a.mean[c]) / sqrtf(a.var[c] + BN_EPS) * a.w[c] + a.b[c];
    }
    const bool pos = v > 0.f;
    if (a.pre) a.pre[e] = v;
    a.act[e] = pos ? v : (a.slope == 0.f ? 0.f : a.slope * v);
    const unsigned long long bal = __ballot(pos);
    const int x = (int)(e % a.W);
    if ((x & 31) == 0) {
        uint32_t word = (uint32_t)(bal >> lane);
        if (a.W < 32) word &= (1u << a.W) - 1u;
        a.mask[(e / a.W) * ((a.W + 31) >> 5) + (x >> 5)] = word;
    }
}

// ---- BatchNorm backward: the two sums (grid (C)), then the apply step (one thread per element) ---------------------------------------
struct BnBwdArgs {
    const float* gact;         // [B][C][HW] d loss / d act
    const float* raw; const uint32_t* mask;
    const float* mean; const float* var; const float* w;
    float* draw;               // [B][C][HW] d loss / d raw
    float* dweight; float* dbias;   // [C] (+= with accumulate)
    float* m1; float* m2;      // [C] mean(dy), mean(dy xhat)
    int B, C, HW, W, bn, accumulate;
    float slope;
};

__device__ __forceinline__ float masked(const BnBwdArgs& a, size_t e, float g) {
    const int x = (int)(e % a.W);
    const uint32_t word = a.mask[(e / a.W) * ((a.W + 31) >> 5) + (x >> 5)];
    return ((word >> (x & 31)) & 1u) ? g : a.slope * g;
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(BnBwdArgs a) {
    __shared__ double red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const float mean = a.mean[c], sd = sqrtf(a.var[c] + BN_EPS);
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < a.B; ++b) {
        const size_t base = ((size_t)b * a.C + c) * a.HW;
        for (int p = tid; p < a.HW; p += 256) {
            const float g = masked(a, base + p, a.gact[base + p]);
            const float xh = (a.raw[base + p] - mean) / sd;
            s1 += (double)g;
            s2 += (double)g * (double)xh;
        }
    }
    s1 = block_sum256(s1, red);
    s2 = block_sum256(s2, red);
    if (tid == 0) {
        const double N = (double)a.B * a.HW;
        a.dbias[c] = a.accumulate ? a.dbias[c] + (float)s1 : (float)s1;
        a.dweight[c] = a.accumulate ? a.dweight[c] + (float)s2 : (float)s2;
        a.m1[c] = (float)(s1 / N);
        a.m2[c] = (float)(s2 / N);
    }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnBwdArgs a) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const float g = masked(a, e, a.gact[e]);
    if (!a.bn) {
        a.draw[e] = g;
        return;
    }
    const int c = (int)((e / a.HW) % a.C);
    const float sd = sqrtf(a.var[c] + BN_EPS), xh = (a.raw[e] - a.mean[c]) / sd;
    a.draw[e] = (g - a.m1[c] - xh * a.m2[c]) * (a.w[c] / sd);
}

// ---- wgrad128: dW[co][ci][ky][kx] = sum_{b, y, x} draw[b][co][y][x] in[b][ci][y + ky - p][x + kx - p] on the fp32 matrix cores ----------
// A product [co] x [ci] per tap with the pixels as the contraction.  grid (KS^2, nsplit): a workgroup owns one tap and a contiguous share
// of the B H (W / 32) row tiles of 32 pixels.  A tile's draw and its input row, shifted by the tap (zero outside the image, read through
// the nearest x 2 map with `up`), are staged pixel-major [32][128 + 1] in LDS: the A operand of v_mfma_f32_32x32x2_f32 is lane l:
// [co = l & 31][pixel = l >> 5], the B operand [pixel = l >> 5][ci = l & 31], both read from consecutive addresses.  A wavefront owns
// 64 x 64 of the 128 x 128 as 2 x 2 blocks.  A tile's 32 products are one fmaf chain; the tiles' sums are added one after the other;
// the shares' partial results [split][tap][co][ci] are summed in ascending order, in float64, by wgrad128_reduce_kernel, which writes
// the torch layout.
struct WgradArgs {
    const float* draw;         // [B][128][H][W]
    const float* in;           // [B][128][H >> up][W >> up]
    float* part;               // [nsplit][KS^2][128][128]
    int B, H, W, up, nsplit;
};
constexpr int WG_PX = 32, WG_LD = CH + 1;

template <int KS>
__global__ __launch_bounds__(256) void wgrad128_kernel(WgradArgs a) {
    __shared__ float a_s[WG_PX * WG_LD];
    __shared__ float b_s[WG_PX * WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1, l31 = lane & 31, kh = lane >> 5;
    const int tap = blockIdx.x, ky = tap / KS, kx = tap % KS, P = KS / 2;
    const int H = a.H, W = a.W, up = a.up, Hs = H >> up, Ws = W >> up, tw = W / WG_PX;
    const long long U = (long long)a.B * H * tw;
    const int u0 = (int)(U * blockIdx.y / a.nsplit), u1 = (int)(U * (blockIdx.y + 1) / a.nsplit);
    f16v acc[2][2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;
    for (int u = u0; u < u1; ++u) {
        const int b = u / (H * tw), y = (u / tw) % H, x0 = (u % tw) * WG_PX;
        const int yy = y + ky - P;
        __syncthreads();                               // everyone is done with the previous tile
#pragma unroll 4
        for (int i = 0; i < CH * WG_PX / 256; ++i) {
            const int e = tid + 256 * i, c = e >> 5, px = e & 31, xx = x0 + px + kx - P;
            a_s[px * WG_LD + c] = a.draw[(((size_t)b * CH + c) * H + y) * W + x0 + px];
            const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
            b_s[px * WG_LD + c] = in ? a.in[(((size_t)b * CH + c) * Hs + (yy >> up)) * Ws + (xx >> up)] : 0.f;
        }
        __syncthreads();
        f16v part[2][2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) part[mb][nb][r] = 0.f;
#pragma unroll
        for (int s = 0; s < WG_PX / 2; ++s) {
            const float* ap = a_s + (2 * s + kh) * WG_LD + wm * 64 + l31;
            const float* bp = b_s + (2 * s + kh) * WG_LD + wn * 64 + l31;
            const float a0 = ap[0], a1 = ap[32], b0 = bp[0], b1 = bp[32];
            part[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, part[0][0], 0, 0, 0);
            part[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, part[0][1], 0, 0, 0);
            part[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, part[1][0], 0, 0, 0);
            part[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, part[1][1], 0, 0, 0);
        }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mb][nb][r] += part[mb][nb][r];
    }
    // D layout: row (co) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the block, column (ci) = lane & 31
    float* out = a.part + ((size_t)blockIdx.y * KS * KS + tap) * CH * CH;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = wm * 64 + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh, ci = wn * 64 + nb * 32 + l31;
                out[(size_t)co * CH + ci] = acc[mb][nb][r];
            }
}

// grid (T 128 128 / 256): thread = one (tap, co, ci) of the partial layout
__global__ __launch_bounds__(256) void wgrad128_reduce_kernel(const float* __restrict__ part, float* __restrict__ dW, int T, int nsplit) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= T * CH * CH) return;
    const int t = e / (CH * CH), co = (e / CH) % CH, ci = e % CH;
    double s = 0.0;
    for (int k = 0; k < nsplit; ++k) s += (double)part[(size_t)k * T * CH * CH + e];
    dW[((size_t)co * CH + ci) * T + t] = (float)s;
}

int wgrad128_splits(int B, int H, int W, int ks) {
    const long long U = (long long)B * H * (W / WG_PX);
    const int want = ks == 5 ? 16 : 32;
    return (int)(U < want ? U : want);
}

// ---- direct convolutions on the vector ALUs (the critic; the generator's output convolution's weight gradient) ---------------------
struct DconvArgs {
    const float* in;           // [B][Ci][Hi][Wi]   (forward: read; backward: the gradient written)
    const float* w;            // [Co][Ci][KH][KW]
    const float* out;          // [B][Co][Ho][Wo]   (forward: written; backward: the gradient read)
    float* dst;                // what the launch writes
    int B, Ci, Hi, Wi, Co, Ho, Wo, KH, KW, stride, padH, padW, accumulate;
};

// The filter size and the stride are template arguments, so that the tap loops unroll: 4 x 4 / 2, 3 x 3, the (4, 16) dot product, and
// 5 x 5 for the weight gradient of G's output convolution (forward and weight gradient of the dot product: final_*_kernel below).
// forward: one thread per output element; an input channel's taps are one fmaf chain, the channels' sums are added one after the other
template <int KH_, int KW_, int S_>
__global__ __launch_bounds__(256) void dconv_fwd_kernel(DconvArgs a) {
    constexpr int KH = KH_, KW = KW_, S = S_;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.B * a.Co * a.Ho * a.Wo) return;
    const int x = (int)(e % a.Wo), y = (int)((e / a.Wo) % a.Ho), co = (int)((e / ((size_t)a.Wo * a.Ho)) % a.Co), b = (int)(e / ((size_t)a.Wo * a.Ho * a.Co));
    const int y0 = y * S - a.padH, x0 = x * S - a.padW;
    float acc = 0.f;
    for (int ci = 0; ci < a.Ci; ++ci) {
        const float* in = a.in + ((size_t)b * a.Ci + ci) * a.Hi * a.Wi;
        const float* w = a.w + ((size_t)co * a.Ci + ci) * KH * KW;
        float part = 0.f;
#pragma unroll
        for (int ky = 0; ky < KH; ++ky) {
            const int yi = y0 + ky;
            if (yi < 0 || yi >= a.Hi) continue;
#pragma unroll
            for (int kx = 0; kx < KW; ++kx) {
                const int xi = x0 + kx;
                if (xi < 0 || xi >= a.Wi) continue;
                part = fmaf(in[yi * a.Wi + xi], w[ky * KW + kx], part);
            }
        }
        acc += part;
    }
    a.dst[e] = acc;
}

// input gradient: one thread per input element; an output channel's taps are one fmaf chain, the channels' sums added one after the other
template <int KH_, int KW_, int S_>
__global__ __launch_bounds__(256) void dconv_bwd_kernel(DconvArgs a) {
    constexpr int KH = KH_, KW = KW_, S = S_;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.B * a.Ci * a.Hi * a.Wi) return;
    const int xi = (int)(e % a.Wi), yi = (int)((e / a.Wi) % a.Hi), ci = (int)((e / ((size_t)a.Wi * a.Hi)) % a.Ci), b = (int)(e / ((size_t)a.Wi * a.Hi * a.Ci));
    float acc = 0.f;
    for (int co = 0; co < a.Co; ++co) {
        const float* g = a.out + ((size_t)b * a.Co + co) * a.Ho * a.Wo;
        const float* w = a.w + ((size_t)co * a.Ci + ci) * KH * KW;
        float part = 0.f;
#pragma unroll
        for (int ky = 0; ky < KH; ++ky) {
            const int ty = yi + a.padH - ky;
            if (ty < 0 || ty % S != 0 || ty / S >= a.Ho) continue;
#pragma unroll
            for (int kx = 0; kx < KW; ++kx) {
                const int tx = xi + a.padW - kx;
                if (tx < 0 || tx % S != 0 || tx / S >= a.Wo) continue;
                part = fmaf(g[(ty / S) * a.Wo + tx / S], w[ky * KW + kx], part);
            }
        }
        acc += part;
    }
    a.dst[e] = acc;
}

// weight gradient: grid (Ci, Co); per tap the workgroup sums the products over (b, y, x) in float64 (a product of two floats is exact
// there), thread t taking pixels t, t + 256, .. of every sample in order; all taps in one pass over the data (KH KW accumulators).
template <int KH_, int KW_, int S_>
__global__ __launch_bounds__(256) void dconv_wgrad_kernel(DconvArgs a) {
    __shared__ double red[4];
    const int ci = blockIdx.x, co = blockIdx.y, tid = threadIdx.x, HWo = a.Ho * a.Wo;
    {
        double s[KH_ * KW_];
#pragma unroll
        for (int t = 0; t < KH_ * KW_; ++t) s[t] = 0.0;
        for (int b = 0; b < a.B; ++b) {
            const float* g = a.out + ((size_t)b * a.Co + co) * HWo;
            const float* in = a.in + ((size_t)b * a.Ci + ci) * a.Hi * a.Wi;
            for (int p = tid; p < HWo; p += 256) {
                const double gv = (double)g[p];
                const int y0 = (p / a.Wo) * S_ - a.padH, x0 = (p % a.Wo) * S_ - a.padW;
#pragma unroll
                for (int ky = 0; ky < KH_; ++ky)
#pragma unroll
                    for (int kx = 0; kx < KW_; ++kx) {
                        const int yi = y0 + ky, xi = x0 + kx;
                        if (yi >= 0 && yi < a.Hi && xi >= 0 && xi < a.Wi) s[ky * KW_ + kx] += gv * (double)in[yi * a.Wi + xi];
                    }
            }
        }
#pragma unroll
        for (int t = 0; t < KH_ * KW_; ++t) {
            const double v = block_sum256(s[t], red);
            if (tid == 0) {
                float* d = a.dst + ((size_t)co * a.Ci + ci) * KH_ * KW_ + t;
                *d = a.accumulate ? *d + (float)v : (float)v;
            }
        }
    }
}

// The critic's last layer has one output per sample, so the two kernels above would leave all but one thread idle.  Its forward is a
// dot product over n = 128 * 4 * 16 values: grid (B), float64, thread t takes elements t, t + 256, .. in order; its weight gradient is
// dW[e] = sum_b draw[b] in[b][e], float64 over b in order, one thread per element.
__global__ __launch_bounds__(256) void final_dot_kernel(const float* __restrict__ in, const float* __restrict__ w, float* __restrict__ out, int n) {
    __shared__ double red[4];
    const float* x = in + (size_t)blockIdx.x * n;
    double s = 0.0;
    for (int e = threadIdx.x; e < n; e += 256) s += (double)x[e] * (double)w[e];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)s;
}

__global__ __launch_bounds__(256) void final_wgrad_kernel(const float* __restrict__ draw, const float* __restrict__ in, float* __restrict__ dW, int B,
                                                          int n, int accumulate) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)draw[b] * (double)in[(size_t)b * n + e];
    dW[e] = accumulate ? dW[e] + (float)s : (float)s;
}

// the form of a direct convolution for its filter
enum { DC_FWD, DC_BWD, DC_WGRAD };
template <int KH, int KW, int S>
void launch_dconv_form(int which, const DconvArgs& a, dim3 grid, hipStream_t s) {
    if (which == DC_FWD) hipLaunchKernelGGL((dconv_fwd_kernel<KH, KW, S>), grid, dim3(256), 0, s, a);
    else if (which == DC_BWD) hipLaunchKernelGGL((dconv_bwd_kernel<KH, KW, S>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((dconv_wgrad_kernel<KH, KW, S>), grid, dim3(256), 0, s, a);
}
void launch_dconv(int which, const DconvArgs& a, hipStream_t s) {
    const dim3 grid = which == DC_WGRAD ? dim3(a.Ci, a.Co)
                                        : dim3((unsigned)(((size_t)a.B * (which == DC_FWD ? a.Co * a.Ho * a.Wo : a.Ci * a.Hi * a.Wi) + 255) / 256));
    if (a.KH == 4 && a.KW == 4 && a.stride == 2) launch_dconv_form<4, 4, 2>(which, a, grid, s);
    else if (a.KH == 3 && a.KW == 3 && a.stride == 1) launch_dconv_form<3, 3, 1>(which, a, grid, s);
    else if (a.KH == 5 && a.KW == 5 && a.stride == 1 && which == DC_WGRAD) hipLaunchKernelGGL((dconv_wgrad_kernel<5, 5, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((dconv_bwd_kernel<4, 16, 1>), grid, dim3(256), 0, s, a);   // the last layer's input gradient (its other directions: final_*_kernel)
}

// ---- small ends -------------------------------------------------------------------------------------------------------------------------
// out[c] = sum_{b, p} x[b][c][p], float64, grid (C): the bias gradients of conv1, conv2 and conv_out
__global__ __launch_bounds__(256) void chan_sum_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, int HW) {
    __shared__ double red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* p = x + ((size_t)b * C + c) * HW;
        for (int i = tid; i < HW; i += 256) s += (double)p[i];
    }
    s = block_sum256(s, red);
    if (tid == 0) out[c] = (float)s;
}

// dense layer: dW[f][j] = sum_b g0[b][f] z[b][j], db[f] = sum_b g0[b][f]; float64 over b in order; grid (8192 * 60 / 256)
__global__ __launch_bounds__(256) void dense_wgrad_kernel(const float* __restrict__ g0, const float* __restrict__ z, float* __restrict__ dW,
                                                          float* __restrict__ db, int B) {
    const int e = blockIdx.x * 256 + threadIdx.x, f = e / NZ, j = e % NZ;
    double s = 0.0, sb = 0.0;
    for (int b = 0; b < B; ++b) {
        const double g = (double)g0[(size_t)b * DENSE + f];
        s += g * (double)z[(size_t)b * NZ + j];
        sb += g;
    }
    dW[e] = (float)s;
    if (j == 0) db[f] = (float)sb;
}

// the critic's output: err = mean_b out[b] (float64, in order); seed[b] = sign / B, the gradient of sign * err; one workgroup
__global__ __launch_bounds__(256) void mean_seed_kernel(const float* __restrict__ out, float* __restrict__ err, float* __restrict__ loss,
                                                        float* __restrict__ seed, int B, float sign) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int b = tid; b < B; b += 256) {
        s += (double)out[b];
        seed[b] = sign * (1.f / (float)B);
    }
    s = block_sum256(s, red);
    if (tid == 0) {
        const float v = (float)(s / (double)B);
        err[0] = v;
        if (loss) loss[0] = v;
    }
}

// ---- RMSprop (torch.optim.RMSprop's defaults: no momentum, not centred) and the weight clamp, element-wise, contraction off ------
//     mode 0: p = min(max(p, lo), hi)
//     mode 1: sq = fma((1 - alpha) g, g, sq alpha);  p = p + (-lr g) / (sqrt(sq) + eps)
__global__ __launch_bounds__(256) void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq, long long n,
                                                      float neg_lr, float alpha, float one_minus_alpha, float eps, float lo, float hi, int mode) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    if (mode == 0) {
        p[e] = fminf(fmaxf(p[e], lo), hi);
        return;
    }
    const float gv = g[e];
    const float s = fmaf(one_minus_alpha * gv, gv, sq[e] * alpha);    // addcmul_ as torch's CPU kernel evaluates it: one fused multiply-add
    sq[e] = s;
    p[e] = p[e] + (neg_lr * gv) / (sqrtf(s) + eps);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
struct Entry {
    std::string name;
    size_t off;
    int64_t numel;
};

// the float tensors of one network on the device: trainable ones first (value, gradient, RMSprop square average), then the running
// statistics.  The values are a ParamImage; the first n_train floats of it have a gradient and a square average at the same offsets.
struct Net {
    ParamImage val;
    std::vector<Entry> entries;
    size_t n_train = 0;
    float *grad = nullptr, *sq = nullptr;
    const Entry* find(const std::string& name) const {
        for (const Entry& e : entries)
            if (e.name == name) return &e;
        return nullptr;
    }
    // reserve every tensor of `names` (trainable ones first, then the running statistics) and copy it from the state dict; false after a miss
    bool fill(const TensorIndex& sd, const std::vector<std::pair<std::string, int64_t>>& names) {
        for (const auto& t : names) {
            const float* p = sd.find(t.first, t.second);
            if (!p) return false;
            entries.push_back({t.first, val.take((size_t)t.second), t.second});
            memcpy(val.host.data() + entries.back().off, p, sizeof(float) * (size_t)t.second);
            if (t.first.find(".running_") == std::string::npos) n_train = val.host.size();
        }
        return true;
    }
    // the values to the current device, the gradients and the square averages zeroed beside them
    int upload(const char* who) {
        const int rc = val.upload(who);
        if (rc) return rc;
        hipError_t e = hipMalloc(&grad, n_train * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(&sq, n_train * sizeof(float));
        if (e == hipSuccess) e = hipMemset(grad, 0, n_train * sizeof(float));
        if (e == hipSuccess) e = hipMemset(sq, 0, n_train * sizeof(float));
        if (e == hipSuccess) return SBC_OK;
        set_error("%s: upload of the parameters failed: %s", who, hipGetErrorString(e));
        return SBC_ERR_HIP;
    }
    void release() {
        val.release();
        if (grad) (void)hipFree(grad);
        if (sq) (void)hipFree(sq);
        grad = sq = nullptr;
    }
};

struct DLayer {
    int Ci, Hi, Wi, Co, Ho, Wo, KH, KW, stride, padH, padW, bn;
    size_t w, bn_w, bn_b, rm, rv;      // offsets into the critic's values
};

int d_layers(int n_extra, DLayer* l) {
    int M = 0;
    l[M++] = {2, NR, NT, NDF, NR / 2, NT / 2, 4, 4, 2, 1, 1, 0, 0, 0, 0, 0, 0};
    for (int t = 0; t < n_extra; ++t) l[M++] = {NDF, NR / 2, NT / 2, NDF, NR / 2, NT / 2, 3, 3, 1, 1, 1, 1, 0, 0, 0, 0, 0};
    l[M++] = {NDF, NR / 2, NT / 2, 2 * NDF, NR / 4, NT / 4, 4, 4, 2, 1, 1, 1, 0, 0, 0, 0, 0};
    l[M] = {2 * NDF, NR / 4, NT / 4, 1, 1, 1, NR / 4, NT / 4, 1, 0, 0, 0, 0, 0, 0, 0, 0};
    return M;                                            // index of the final layer
}

// stage kinds of sbc_wgan_trainer_stage: id = net base + 16 kind + layer; the generator's base is 0, the critic's 256 (real pass) and 512 (fake)
enum { K_ACT = 0, K_RAW, K_PRE, K_MASK, K_MEAN, K_VAR, K_GACT, K_DRAW, K_N, ST_GEN = 128, ST_DGEN = 129, ST_ERR = 130 };

// the workspace for a capacity of Bc samples, in floats; every buffer starts on a 16-byte boundary
struct Lay {
    int L, M;
    DLayer dl[MAX_M + 1];
    int64_t g[K_N][MAX_L + 1], gen, dgen, d[2][K_N][MAX_M + 1], derr[2], tmp, scratch, total;
    Lay(int n_extra, int64_t Bc) : L(2 + n_extra) {
        M = d_layers(n_extra, dl);
        int64_t o = 0;
        auto take = [&](int64_t n) { const int64_t at = o; o += (n + 3) & ~(int64_t)3; return at; };
        for (int q = 0; q < K_N; ++q)
            for (int k = 0; k <= MAX_L; ++k) g[q][k] = -1;
        for (int s = 0; s < 2; ++s)
            for (int q = 0; q < K_N; ++q)
                for (int j = 0; j <= MAX_M; ++j) d[s][q][j] = -1;
        for (int k = 0; k <= L; ++k) {
            const int64_t n = (int64_t)CH * layer_h(k) * layer_w(k) * Bc;
            g[K_ACT][k] = take(n);
            g[K_GACT][k] = take(n);
            if (k == 0) continue;
            g[K_RAW][k] = take(n);
            g[K_PRE][k] = take(n);
            g[K_DRAW][k] = take(n);
            g[K_MASK][k] = take((int64_t)CH * mask_words(layer_h(k), layer_w(k)) * Bc);
            g[K_MEAN][k] = take(CH);
            g[K_VAR][k] = take(CH);
        }
        gen = take((int64_t)2 * PIX * Bc);
        dgen = take((int64_t)2 * PIX * Bc);
        for (int s = 0; s < 2; ++s) {
            for (int j = 0; j <= M; ++j) {
                const DLayer& q = dl[j];
                const int64_t n = (int64_t)q.Co * q.Ho * q.Wo * Bc;
                d[s][K_RAW][j] = take(n);
                d[s][K_DRAW][j] = take(n);
                if (j == M) continue;
                d[s][K_PRE][j] = take(n);
                d[s][K_ACT][j] = take(n);
                d[s][K_GACT][j] = take(n);
                d[s][K_MASK][j] = take((int64_t)q.Co * mask_words(q.Ho, q.Wo) * Bc);
                if (q.bn) {
                    d[s][K_MEAN][j] = take(q.Co);
                    d[s][K_VAR][j] = take(q.Co);
                }
            }
            derr[s] = take(4);
        }
        tmp = take(4 * CH);                              // mean(dy), mean(dy xhat); BatchNorm gradients nobody asked for
        int64_t sc = 0;
        for (int k = 1; k <= L; ++k) {
            const int64_t n = (int64_t)wgrad128_splits((int)Bc, layer_h(k), layer_w(k), layer_ks(k)) * layer_ks(k) * layer_ks(k) * CH * CH;
            sc = n > sc ? n : sc;
        }
        scratch = take(sc);
        total = o;
    }
};

}  // namespace
}  // namespace sbc

struct sbc_wgan_trainer {
    int n_extra = 0;
    sbc::Net G, D;
    float* pack = nullptr;               // the generator's filters packed for conv128: per layer forward, adjoint
    size_t fwd[sbc::MAX_L + 1] = {}, adj[sbc::MAX_L + 1] = {};
    // offsets into G.val (gradients: the same offsets into G.grad)
    size_t dense_w = 0, dense_b = 0, out_w = 0, out_b = 0, conv_w[sbc::MAX_L + 1] = {}, conv_b[sbc::MAX_L + 1] = {}, bn_w[sbc::MAX_L + 1] = {},
           bn_b[sbc::MAX_L + 1] = {}, rm[sbc::MAX_L + 1] = {}, rv[sbc::MAX_L + 1] = {};
    sbc::DLayer dl[sbc::MAX_M + 1];
    int M = 0;
    float neg_lr_d = 0, neg_lr_g = 0, alpha = 0, one_minus_alpha = 0, eps = 0, lo = 0, hi = 0;
};

namespace sbc {
namespace {

int grid_of(size_t n) { return (int)((n + 255) / 256); }

void bn_forward(const float* raw, float* mean, float* var, float* rm, float* rv, const float* w, const float* b, float* pre, float* act,
                uint32_t* mask, int B, int C, int H, int W, int bn, float slope, hipStream_t s) {
    if (bn) {
        StatArgs sa{raw, mean, var, rm, rv, B, C, H * W};
        hipLaunchKernelGGL(bn_stats_kernel, dim3(C), dim3(256), 0, s, sa);
    }
    ActArgs aa{raw, mean, var, w, b, pre, act, mask, C, H * W, W, bn, slope};
    hipLaunchKernelGGL(bn_act_kernel, dim3(grid_of((size_t)B * C * H * W)), dim3(256), 0, s, aa);
}

void bn_backward(const float* gact, const float* raw, const uint32_t* mask, const float* mean, const float* var, const float* w, float* draw,
                 float* dweight, float* dbias, float* tmp, int B, int C, int H, int W, int bn, int accumulate, float slope, hipStream_t s) {
    BnBwdArgs a{gact, raw, mask, mean, var, w, draw, dweight, dbias, tmp, tmp + C, B, C, H * W, W, bn, accumulate, slope};
    if (bn) hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(C), dim3(256), 0, s, a);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_of((size_t)B * C * H * W)), dim3(256), 0, s, a);
}

void wgrad128(const float* draw, const float* in, float* dW, float* scratch, int B, int H, int W, int ks, int up, hipStream_t s) {
    WgradArgs a{draw, in, scratch, B, H, W, up, wgrad128_splits(B, H, W, ks)};
    const dim3 grid(ks * ks, a.nsplit);
    if (ks == 5) hipLaunchKernelGGL(wgrad128_kernel<5>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(wgrad128_kernel<3>, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(wgrad128_reduce_kernel, dim3(ks * ks * CH * CH / 256), dim3(256), 0, s, (const float*)scratch, dW, ks * ks, a.nsplit);
}

struct Ws {
    float* base;
    Lay lay;
    float* g(int kind, int k) const { return base + lay.g[kind][k]; }
    float* d(int slot, int kind, int j) const { return base + lay.d[slot][kind][j]; }
    uint32_t* gmask(int k) const { return reinterpret_cast<uint32_t*>(base + lay.g[K_MASK][k]); }
    uint32_t* dmask(int slot, int j) const { return reinterpret_cast<uint32_t*>(base + lay.d[slot][K_MASK][j]); }
    float* tmp() const { return base + lay.tmp; }
};

void g_forward(sbc_wgan_trainer* h, const Ws& ws, const float* noise, int B, hipStream_t s) {
    const float* v = h->G.val.dev;
    launch_dense(noise, v + h->dense_w, v + h->dense_b, ws.g(K_ACT, 0), B, s);
    for (int k = 1; k <= ws.lay.L; ++k) {
        launch_conv128_raw(ws.g(K_ACT, k - 1), h->pack + h->fwd[k], k <= 2 ? v + h->conv_b[k] : nullptr, ws.g(K_RAW, k), layer_h(k), layer_w(k), layer_ks(k),
                           k <= 2 ? 1 : 0, 0, B, s);
        bn_forward(ws.g(K_RAW, k), ws.g(K_MEAN, k), ws.g(K_VAR, k), h->G.val.dev + h->rm[k], h->G.val.dev + h->rv[k], v + h->bn_w[k], v + h->bn_b[k],
                   ws.g(K_PRE, k), ws.g(K_ACT, k), ws.gmask(k), B, CH, layer_h(k), layer_w(k), 1, 0.f, s);
    }
    launch_out_conv(ws.g(K_ACT, ws.lay.L), v + h->out_w, v + h->out_b, ws.base + ws.lay.gen, B, s);
}

DconvArgs dconv_args(const DLayer& q, const float* in, const float* w, const float* out, float* dst, int B, int accumulate) {
    return DconvArgs{in, w, out, dst, B, q.Ci, q.Hi, q.Wi, q.Co, q.Ho, q.Wo, q.KH, q.KW, q.stride, q.padH, q.padW, accumulate};
}

// the critic on `input` [B][2][16][64] into the stages of `slot`; err = mean_b D(input), the seed of its backward pass is sign / B
void d_forward(sbc_wgan_trainer* h, const Ws& ws, int slot, const float* input, int B, float sign, float* loss, hipStream_t s) {
    float* v = h->D.val.dev;
    const float* in = input;
    const int M = h->M;
    for (int j = 0; j <= M; ++j) {
        const DLayer& q = h->dl[j];
        if (j == M) {
            hipLaunchKernelGGL(final_dot_kernel, dim3(B), dim3(256), 0, s, in, (const float*)(v + q.w), ws.d(slot, K_RAW, j), q.Ci * q.Hi * q.Wi);
            break;
        }
        launch_dconv(DC_FWD, dconv_args(q, in, v + q.w, nullptr, ws.d(slot, K_RAW, j), B, 0), s);
        bn_forward(ws.d(slot, K_RAW, j), q.bn ? ws.d(slot, K_MEAN, j) : nullptr, q.bn ? ws.d(slot, K_VAR, j) : nullptr, v + q.rm, v + q.rv, v + q.bn_w,
                   v + q.bn_b, ws.d(slot, K_PRE, j), ws.d(slot, K_ACT, j), ws.dmask(slot, j), B, q.Co, q.Ho, q.Wo, q.bn, 0.2f, s);
        in = ws.d(slot, K_ACT, j);
    }
    hipLaunchKernelGGL(mean_seed_kernel, dim3(1), dim3(256), 0, s, (const float*)ws.d(slot, K_RAW, M), ws.base + ws.lay.derr[slot], loss,
                       ws.d(slot, K_DRAW, M), B, sign);
}

// backward through the critic from the seed in draw[M]: weight gradients into D.grad (`wgrads`; += with `accumulate`), the gradient
// with respect to the input into `gin` (or NULL)
void d_backward(sbc_wgan_trainer* h, const Ws& ws, int slot, const float* input, int B, bool wgrads, int accumulate, float* gin, hipStream_t s) {
    const float* v = h->D.val.dev;
    for (int j = h->M; j >= 0; --j) {
        const DLayer& q = h->dl[j];
        const float* in = j == 0 ? input : ws.d(slot, K_ACT, j - 1);
        const float* draw = ws.d(slot, K_DRAW, j);
        if (wgrads && j == h->M)
            hipLaunchKernelGGL(final_wgrad_kernel, dim3(grid_of((size_t)q.Ci * q.Hi * q.Wi)), dim3(256), 0, s, draw, in, h->D.grad + q.w, B, q.Ci * q.Hi * q.Wi,
                               accumulate);
        else if (wgrads) launch_dconv(DC_WGRAD, dconv_args(q, in, nullptr, draw, h->D.grad + q.w, B, accumulate), s);
        float* dst = j == 0 ? gin : ws.d(slot, K_GACT, j - 1);
        if (dst) launch_dconv(DC_BWD, dconv_args(q, nullptr, v + q.w, draw, dst, B, 0), s);
        if (j == 0) break;
        const DLayer& p = h->dl[j - 1];
        const bool keep = wgrads && p.bn;
        bn_backward(ws.d(slot, K_GACT, j - 1), ws.d(slot, K_RAW, j - 1), ws.dmask(slot, j - 1), p.bn ? ws.d(slot, K_MEAN, j - 1) : nullptr,
                    p.bn ? ws.d(slot, K_VAR, j - 1) : nullptr, v + p.bn_w, ws.d(slot, K_DRAW, j - 1), keep ? h->D.grad + p.bn_w : ws.tmp() + 2 * CH,
                    keep ? h->D.grad + p.bn_b : ws.tmp() + 3 * CH, ws.tmp(), B, p.Co, p.Ho, p.Wo, p.bn, keep ? accumulate : 0, 0.2f, s);
    }
}

// backward through the generator from dgen = d loss / d gen: every parameter gradient into G.grad
void g_backward(sbc_wgan_trainer* h, const Ws& ws, const float* noise, int B, hipStream_t s) {
    const float* v = h->G.val.dev;
    float* gr = h->G.grad;
    const int L = ws.lay.L;
    const float* dgen = ws.base + ws.lay.dgen;
    const DLayer out{CH, NR, NT, 2, NR, NT, 5, 5, 1, 2, 2, 0, 0, 0, 0, 0, 0};
    launch_dconv(DC_WGRAD, dconv_args(out, ws.g(K_ACT, L), nullptr, dgen, gr + h->out_w, B, 0), s);
    hipLaunchKernelGGL(chan_sum_kernel, dim3(2), dim3(256), 0, s, dgen, gr + h->out_b, B, 2, PIX);
    launch_out_adjoint(dgen, v + h->out_w, ws.g(K_GACT, L), B, s);
    for (int k = L; k >= 1; --k) {
        const int H = layer_h(k), W = layer_w(k);
        bn_backward(ws.g(K_GACT, k), ws.g(K_RAW, k), ws.gmask(k), ws.g(K_MEAN, k), ws.g(K_VAR, k), v + h->bn_w[k], ws.g(K_DRAW, k), gr + h->bn_w[k],
                    gr + h->bn_b[k], ws.tmp(), B, CH, H, W, 1, 0, 0.f, s);
        wgrad128(ws.g(K_DRAW, k), ws.g(K_ACT, k - 1), gr + h->conv_w[k], ws.base + ws.lay.scratch, B, H, W, layer_ks(k), k <= 2 ? 1 : 0, s);
        if (k <= 2) hipLaunchKernelGGL(chan_sum_kernel, dim3(CH), dim3(256), 0, s, (const float*)ws.g(K_DRAW, k), gr + h->conv_b[k], B, CH, H * W);
        launch_conv128_raw(ws.g(K_DRAW, k), h->pack + h->adj[k], nullptr, ws.g(K_GACT, k - 1), H, W, layer_ks(k), 0, k <= 2 ? 1 : 0, B, s);
    }
    hipLaunchKernelGGL(dense_wgrad_kernel, dim3(DENSE * NZ / 256), dim3(256), 0, s, (const float*)ws.g(K_GACT, 0), noise, gr + h->dense_w,
                       gr + h->dense_b, B);
}

void repack(sbc_wgan_trainer* h, hipStream_t s) {
    for (int k = 1; k <= 2 + h->n_extra; ++k) launch_repack128(h->G.val.dev + h->conv_w[k], h->pack + h->fwd[k], h->pack + h->adj[k], layer_ks(k), s);
}

void rmsprop(const sbc_wgan_trainer* h, const Net& n, float neg_lr, int mode, hipStream_t s) {
    hipLaunchKernelGGL(rmsprop_kernel, dim3(grid_of(n.n_train)), dim3(256), 0, s, n.val.dev, (const float*)n.grad, n.sq, (long long)n.n_train, neg_lr,
                       h->alpha, h->one_minus_alpha, h->eps, h->lo, h->hi, mode);
}

int check_step(const char* who, const sbc_wgan_trainer* h, const float* workspace, int B, int B_cap) {
    SBC_REQUIRE(h && workspace, "%s: NULL handle or workspace", who);
    SBC_REQUIRE(B_cap >= 1 && B_cap <= 32768, "%s: the workspace capacity must be in [1, 32768] (got %d)", who, B_cap);
    SBC_REQUIRE(B >= 1 && B <= B_cap, "%s: a batch must be in [1, %d], the capacity of the workspace (got %d)", who, B_cap, B);
    return h->G.val.check_device(who);
}

size_t off_of(const Net& n, const std::string& name) { return n.find(name)->off; }

std::string d_conv(int j, int n_extra) {
    if (j == 0) return "main.initial:2-64:conv";
    if (j <= n_extra) return "main.extra-layers-" + std::to_string(j - 1) + ":64:conv";
    return j == n_extra + 1 ? "main.pyramid:64-128:conv" : "main.final:128-1:conv";
}
std::string d_bn(int j, int n_extra) {
    return j <= n_extra ? "main.extra-layers-" + std::to_string(j - 1) + ":64:batchnorm" : "main.pyramid:128:batchnorm";
}

void destroy(sbc_wgan_trainer* h) {
    h->G.release();
    h->D.release();
    if (h->pack) (void)hipFree(h->pack);
    delete h;
}

}  // namespace
}  // namespace sbc

extern "C" {

int sbc_wgan_trainer_create(const sbc_wgan_trainer_desc* desc, const sbc_tensor_ref* gen, int32_t n_gen, const sbc_tensor_ref* disc, int32_t n_disc,
                            sbc_wgan_trainer** out) {
    using namespace sbc;
    const char* who = "sbc_wgan_trainer_create";
    SBC_REQUIRE(desc && gen && disc && out && n_gen > 0 && n_disc > 0, "%s: need a descriptor, both state dicts and out", who);
    SBC_REQUIRE(desc->lr_d > 0 && desc->lr_g > 0 && desc->alpha >= 0 && desc->alpha < 1 && desc->eps > 0 && desc->clamp_lower <= desc->clamp_upper,
                "%s: need lr > 0, 0 <= alpha < 1, eps > 0 (a parameter whose gradient and square average are 0 divides 0 by it) and clamp_lower <= clamp_upper", who);
    TensorIndex gsd, dsd;
    int n_extra = 0;
    int rc = open_generator(who, gen, n_gen, "generator tensor", gsd, &n_extra);
    if (!rc) rc = dsd.build_unique(who, "critic tensor", disc, n_disc);
    if (rc) return rc;
    SBC_REQUIRE(n_disc == 7 + 5 * n_extra, "%s: a critic with %d extra layers, as many as the generator has, has %d float tensors (got %d)", who,
                n_extra, 7 + 5 * n_extra, n_disc);
    const int L = 2 + n_extra;
    sbc_wgan_trainer* h = new sbc_wgan_trainer;
    h->n_extra = n_extra;
    h->neg_lr_d = (float)-desc->lr_d; h->neg_lr_g = (float)-desc->lr_g; h->alpha = (float)desc->alpha; h->one_minus_alpha = (float)(1.0 - desc->alpha);
    h->eps = (float)desc->eps; h->lo = (float)desc->clamp_lower; h->hi = (float)desc->clamp_upper;
    std::vector<std::pair<std::string, int64_t>> names = generator_tensors(n_extra);
    bool ok = h->G.fill(gsd, names);
    if (ok) {
        h->dense_w = off_of(h->G, "dense.dense_input.weight"); h->dense_b = off_of(h->G, "dense.dense_input.bias");
        h->out_w = off_of(h->G, "conv.conv_out.weight"); h->out_b = off_of(h->G, "conv.conv_out.bias");
        for (int k = 1; k <= L; ++k) {
            h->conv_w[k] = off_of(h->G, conv_name(k) + ".weight");
            if (k <= 2) h->conv_b[k] = off_of(h->G, conv_name(k) + ".bias");
            h->bn_w[k] = off_of(h->G, bn_name(k) + ".weight"); h->bn_b[k] = off_of(h->G, bn_name(k) + ".bias");
            h->rm[k] = off_of(h->G, bn_name(k) + ".running_mean"); h->rv[k] = off_of(h->G, bn_name(k) + ".running_var");
        }
    }
    // the critic
    h->M = d_layers(n_extra, h->dl);
    names.clear();
    for (int j = 0; j <= h->M; ++j) {
        const DLayer& q = h->dl[j];
        names.push_back({d_conv(j, n_extra) + ".weight", (int64_t)q.Co * q.Ci * q.KH * q.KW});
        if (q.bn) {
            names.push_back({d_bn(j, n_extra) + ".weight", q.Co});
            names.push_back({d_bn(j, n_extra) + ".bias", q.Co});
        }
    }
    for (int j = 0; j <= h->M; ++j)
        if (h->dl[j].bn) {
            names.push_back({d_bn(j, n_extra) + ".running_mean", h->dl[j].Co});
            names.push_back({d_bn(j, n_extra) + ".running_var", h->dl[j].Co});
        }
    ok = ok && h->D.fill(dsd, names);
    if (ok) {
        for (int j = 0; j <= h->M; ++j) {
            DLayer& q = h->dl[j];
            q.w = off_of(h->D, d_conv(j, n_extra) + ".weight");
            if (!q.bn) continue;
            q.bn_w = off_of(h->D, d_bn(j, n_extra) + ".weight"); q.bn_b = off_of(h->D, d_bn(j, n_extra) + ".bias");
            q.rm = off_of(h->D, d_bn(j, n_extra) + ".running_mean"); q.rv = off_of(h->D, d_bn(j, n_extra) + ".running_var");
        }
    }
    rc = ok ? SBC_OK : SBC_ERR_INVALID;
    if (!rc) rc = h->G.upload(who);
    if (!rc) rc = h->D.upload(who);
    if (!rc) {
        size_t o = 0;
        for (int k = 1; k <= L; ++k) {
            const size_t n = (size_t)CH * CH * layer_ks(k) * layer_ks(k);
            h->fwd[k] = o; o += n;
            h->adj[k] = o; o += n;
        }
        hipError_t e = hipMalloc(&h->pack, o * sizeof(float));
        if (e == hipSuccess) {
            repack(h, nullptr);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        }
        if (e != hipSuccess) {
            set_error("%s: packing the filters failed: %s", who, hipGetErrorString(e));
            rc = SBC_ERR_HIP;
        }
    }
    if (rc) {
        destroy(h);
        return rc;
    }
    *out = h;
    return SBC_OK;
}

void sbc_wgan_trainer_destroy(sbc_wgan_trainer* h) {
    if (h) sbc::destroy(h);
}

int64_t sbc_wgan_trainer_workspace_floats(const sbc_wgan_trainer* h, int32_t B_cap) {
    if (!h || B_cap < 1 || B_cap > 32768) return -1;
    return sbc::Lay(h->n_extra, B_cap).total;
}

int sbc_wgan_trainer_stage(const sbc_wgan_trainer* h, int32_t stage, int32_t B_cap, int64_t* offset, int32_t* channels, int32_t* height,
                           int32_t* width, int32_t* per_sample) {
    using namespace sbc;
    SBC_REQUIRE(h && offset && channels && height && width && per_sample && B_cap >= 1 && B_cap <= 32768,
                "sbc_wgan_trainer_stage: NULL handle or output, or a capacity outside [1, 32768]");
    const Lay lay(h->n_extra, B_cap);
    const int net = stage >> 8, id = stage & 255, kind = id >> 4, k = id & 15;
    int64_t off = -1;
    int c = 0, hh = 1, ww = 1, per = 1;
    if (stage >= 0 && net == 0 && id == ST_GEN) { off = lay.gen; c = 2; hh = NR; ww = NT; }
    else if (stage >= 0 && net == 0 && id == ST_DGEN) { off = lay.dgen; c = 2; hh = NR; ww = NT; }
    else if (stage >= 0 && (net == 1 || net == 2) && id == ST_ERR) { off = lay.derr[net - 1]; c = 1; per = 0; }
    else if (stage >= 0 && net <= 2 && kind < K_N && k <= (net == 0 ? lay.L : lay.M)) {
        off = net == 0 ? lay.g[kind][k] : lay.d[net - 1][kind][k];
        c = net == 0 ? CH : lay.dl[k].Co;
        hh = net == 0 ? layer_h(k) : lay.dl[k].Ho;
        ww = net == 0 ? layer_w(k) : lay.dl[k].Wo;
        if (kind == K_MASK) ww = (ww + 31) / 32;
        if (kind == K_MEAN || kind == K_VAR) { hh = ww = 1; per = 0; }
    }
    SBC_REQUIRE(off >= 0, "sbc_wgan_trainer_stage: no stage %d in networks with %d extra layers", stage, h->n_extra);
    *offset = off; *channels = c; *height = hh; *width = ww; *per_sample = per;
    return SBC_OK;
}

int sbc_wgan_trainer_critic_step(sbc_wgan_trainer* h, const float* real, int32_t B_real, const float* noise, int32_t B_fake, float* losses,
                                 float* workspace, int32_t B_cap, void* stream) {
    using namespace sbc;
    const char* who = "sbc_wgan_trainer_critic_step";
    int rc = check_step(who, h, workspace, B_real, B_cap);
    if (!rc) rc = check_step(who, h, workspace, B_fake, B_cap);
    if (rc) return rc;
    SBC_REQUIRE(real && noise, "%s: NULL real or noise", who);
    hipStream_t s = (hipStream_t)stream;
    const Ws ws{workspace, Lay(h->n_extra, B_cap)};
    rmsprop(h, h->D, 0.f, 0, s);                                                    // the clamp
    d_forward(h, ws, 0, real, B_real, 1.f, losses, s);
    d_backward(h, ws, 0, real, B_real, true, 0, nullptr, s);
    g_forward(h, ws, noise, B_fake, s);
    const float* fake = ws.base + ws.lay.gen;
    d_forward(h, ws, 1, fake, B_fake, -1.f, losses ? losses + 1 : nullptr, s);
    d_backward(h, ws, 1, fake, B_fake, true, 1, nullptr, s);
    rmsprop(h, h->D, h->neg_lr_d, 1, s);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int sbc_wgan_trainer_generator_step(sbc_wgan_trainer* h, const float* noise, int32_t B, float* loss, float* workspace, int32_t B_cap, void* stream) {
    using namespace sbc;
    const char* who = "sbc_wgan_trainer_generator_step";
    const int rc = check_step(who, h, workspace, B, B_cap);
    if (rc) return rc;
    SBC_REQUIRE(noise, "%s: NULL noise", who);
    hipStream_t s = (hipStream_t)stream;
    const Ws ws{workspace, Lay(h->n_extra, B_cap)};
    g_forward(h, ws, noise, B, s);
    const float* fake = ws.base + ws.lay.gen;
    d_forward(h, ws, 1, fake, B, 1.f, loss, s);
    d_backward(h, ws, 1, fake, B, false, 0, ws.base + ws.lay.dgen, s);
    g_backward(h, ws, noise, B, s);
    rmsprop(h, h->G, h->neg_lr_g, 1, s);
    repack(h, s);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int sbc_wgan_trainer_copy(sbc_wgan_trainer* h, int32_t net, int32_t what, const char* name, float* host, int64_t numel, int32_t to_device) {
    using namespace sbc;
    const char* who = "sbc_wgan_trainer_copy";
    SBC_REQUIRE(h && name && host, "%s: NULL handle, name or host array", who);
    SBC_REQUIRE((net == 0 || net == 1) && what >= 0 && what <= 2, "%s: net is 0 (generator) or 1 (critic), what 0 (value), 1 (gradient) or 2 (square average)", who);
    Net& n = net == 0 ? h->G : h->D;
    const Entry* e = n.find(name);
    SBC_REQUIRE(e, "%s: the %s has no tensor '%s'", who, net == 0 ? "generator" : "critic", name);
    SBC_REQUIRE(e->numel == numel, "%s: tensor '%s' has %lld elements (got %lld)", who, name, (long long)e->numel, (long long)numel);
    SBC_REQUIRE(what == 0 || e->off < n.n_train, "%s: '%s' is a running statistic: it has no gradient and no square average", who, name);
    const int rc = n.val.check_device(who);
    if (rc) return rc;
    float* dev = (what == 0 ? n.val.dev : what == 1 ? n.grad : n.sq) + e->off;
    SBC_CHECK_HIP(hipDeviceSynchronize());
    if (!to_device) {
        SBC_CHECK_HIP(hipMemcpy(host, dev, sizeof(float) * (size_t)numel, hipMemcpyDeviceToHost));
        return SBC_OK;
    }
    SBC_CHECK_HIP(hipMemcpy(dev, host, sizeof(float) * (size_t)numel, hipMemcpyHostToDevice));
    if (net == 0 && what == 0) {
        repack(h, nullptr);
        SBC_CHECK_HIP(hipGetLastError());
        SBC_CHECK_HIP(hipStreamSynchronize(nullptr));
    }
    return SBC_OK;
}

int64_t sbc_wgan_wgrad128_scratch_floats(int32_t B, int32_t H, int32_t W, int32_t ks) {
    using namespace sbc;
    if (B < 1 || B > 32768 || (ks != 3 && ks != 5) || H < 2 || H > 4096 || H % 2 != 0 || (W != 32 && W != 64)) return -1;
    return (int64_t)wgrad128_splits(B, H, W, ks) * ks * ks * CH * CH;
}

int sbc_wgan_wgrad128(const float* draw, const float* in, float* dW, float* scratch, int32_t B, int32_t H, int32_t W, int32_t ks, int32_t up,
                      void* stream) {
    using namespace sbc;
    SBC_REQUIRE(draw && in && dW && scratch, "sbc_wgan_wgrad128: NULL draw, in, dW or scratch");
    SBC_REQUIRE(B >= 1 && B <= 32768 && (ks == 3 || ks == 5) && (up == 0 || up == 1) && H >= 2 && H <= 4096 && H % 2 == 0 && (W == 32 || W == 64),
                "sbc_wgan_wgrad128: need 1 <= B <= 32768, ks 3 or 5, up 0 or 1, an even H in [2, 4096] and W 32 or 64 (got B %d, ks %d, up %d, H %d, W %d)",
                B, ks, up, H, W);
    wgrad128(draw, in, dW, scratch, B, H, W, ks, up, (hipStream_t)stream);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int sbc_wgan_bn_backward(const float* gact, const float* raw, const int32_t* mask, const float* mean, const float* var, const float* weight, float slope,
                         float* draw, float* dweight, float* dbias, float* scratch, int32_t B, int32_t C, int32_t H, int32_t W, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(gact && raw && mask && mean && var && weight && draw && dweight && dbias && scratch, "sbc_wgan_bn_backward: NULL argument");
    SBC_REQUIRE(B >= 1 && B <= 32768 && C >= 1 && C <= 1024 && H >= 1 && H <= 4096 && (W == 16 || W == 32 || W == 64) && ((int64_t)C * H * W) % 256 == 0,
                "sbc_wgan_bn_backward: need 1 <= B <= 32768, 1 <= C <= 1024, 1 <= H <= 4096, W 16, 32 or 64 and C H W a multiple of 256 "
                "(got B %d, C %d, H %d, W %d)", B, C, H, W);
    BnBwdArgs a{gact, raw, reinterpret_cast<const uint32_t*>(mask), mean, var, weight, draw, dweight, dbias, scratch, scratch + C, B, C, H * W, W, 1, 0, slope};
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_of((size_t)B * C * H * W)), dim3(256), 0, (hipStream_t)stream, a);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int sbc_wgan_rmsprop(float* p, const float* g, float* sq, int64_t n, double lr, double alpha, double eps, double clamp_lower, double clamp_upper,
                     int32_t mode, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(p && (mode == 0 || (g && sq)), "sbc_wgan_rmsprop: NULL p, g or sq");
    SBC_REQUIRE(n >= 0 && (mode == 0 || mode == 1), "sbc_wgan_rmsprop: need n >= 0 and mode 0 (clamp) or 1 (step)");
    SBC_REQUIRE(mode == 0 ? clamp_lower <= clamp_upper : (lr > 0 && alpha >= 0 && alpha < 1 && eps > 0),
                "sbc_wgan_rmsprop: need clamp_lower <= clamp_upper (mode 0) or lr > 0, 0 <= alpha < 1, eps > 0 (mode 1)");
    if (n == 0) return SBC_OK;
    hipLaunchKernelGGL(rmsprop_kernel, dim3(grid_of((size_t)n)), dim3(256), 0, (hipStream_t)stream, p, g, sq, (long long)n, (float)-lr, (float)alpha,
                       (float)(1.0 - alpha), (float)eps, (float)clamp_lower, (float)clamp_upper, mode);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

}  // extern "C"
