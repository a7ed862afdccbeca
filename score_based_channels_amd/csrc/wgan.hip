// WGAN latent optimisation (the WGAN baseline of Fig. 5c): src/score_based_channels/test_wgan.py:129-176 with the generator
// aux_gan.py:58-112 (DCGAN_G_Ours), eval mode, isize = [16, 64] (Nr, Nt), nz = 60, nc = 2, ngf = 128 -- the only geometry the
// reference's literal `hidden.view(-1, 128, Nr // 4, Nt // 4)` admits.
//
//     dense   Linear(60 -> 8192) + bias, viewed [128][4][16]
//     layer 1 nearest x 2 -> 8 x 32,  Conv 5 x 5 128 -> 128 (bias, pad 2), BatchNorm (running statistics), ReLU
//     layer 2 nearest x 2 -> 16 x 64, the same
//     layer 3 .. 2 + n_extra          Conv 3 x 3 128 -> 128 (no bias), BatchNorm, ReLU
//     out     Conv 5 x 5 128 -> 2 (bias): G = gen[0] + i gen[1], [16][64]
// One step of sample b:  meas = ||G P - Y||_F^2, reg = ||z||^2, loss = s_b (meas + lambda_b reg), g = d loss / d z, Adam on z.
//
// Arithmetic: exact fp32.  The 128 -> 128 convolutions run on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: bit for bit an fmaf
// chain), fp32 accumulation; every sum has a fixed order and nothing is atomic, and a workgroup works on one sample only: a sample's
// result does not depend on B, on its position in the batch or on repetition.  BatchNorm is applied after conv + bias in the
// reference's order, (x - mean) / sqrt(var + eps) * w + b; it is not folded into the weights.
//
// Launches per step, L = 2 + n_extra: dense, L x conv128 forward, out (conv + residual + logs + dG), out adjoint, L x conv128 on the
// adjoint-packed filters, dense adjoint + Adam = 2 L + 4.  The backward pass needs the ReLU signs only (there is no weight gradient):
// the forward epilogue writes them as bit masks, one 32-bit word per 32 pixels of a row.  Backward stage k holds d loss / d a_k, the
// gradient with respect to the post-ReLU activation of layer k; the mask and the BatchNorm scale of layer k are applied by the
// prologue of the kernel that consumes it.
//
// Every stage of the last call stays readable in the caller's workspace (sbc_wgan_stage); no stage shares memory with another.
#include "common.h"
#include "host_params.h"
#include "reduce.h"
#include "wgan_shared.h"
#include <math.h>
#include <string.h>
#include <map>
#include <string>

namespace sbc {
namespace {
using namespace wgan_shared;                           // the constants, the layers' geometry and the state dict of the generator

// ---- dense: z [60] -> [128][4][16] + bias --------------------------------------------------------------------------------------
// grid (32, B); feature f = c * 64 + h * 16 + w; the sum runs over j = 0 .. 59 in order
__global__ __launch_bounds__(256) void dense_kernel(const float* __restrict__ z, const float* __restrict__ W, const float* __restrict__ bias,
                                                    float* __restrict__ out) {
    __shared__ float z_s[NZ];
    const int tid = threadIdx.x, n = blockIdx.y, f = blockIdx.x * 256 + tid;
    if (tid < NZ) z_s[tid] = z[(size_t)n * NZ + tid];
    __syncthreads();
    const float4* w4 = reinterpret_cast<const float4*>(W + (size_t)f * NZ);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NZ / 4; ++j) {
        const float4 w = w4[j];
        acc = fmaf(w.x, z_s[4 * j], acc);
        acc = fmaf(w.y, z_s[4 * j + 1], acc);
        acc = fmaf(w.z, z_s[4 * j + 2], acc);
        acc = fmaf(w.w, z_s[4 * j + 3], acc);
    }
    out[(size_t)n * DENSE + f] = acc + bias[f];
}

// ---- conv128: KS x KS convolution 128 -> 128 (pad KS / 2) as an implicit GEMM on the fp32 matrix cores ---------------------------
// M = 128 output channels (the A operand: filters), N = the pixels of a tile (the B operand: 4 rows x 32 columns), K = 128 KS^2 in
// chunks of CC input channels: a chunk's filters [KS^2][CC][128] and its input tile [CC][4 + KS - 1][32 + KS - 1] go through LDS.
// A wavefront owns 2 rows x 64 channels = 2 x 2 blocks of 32 x 32; D[channel][pixel], so a register's 32 lanes store 32 adjacent pixels.
// K order (fixed): within a chunk tap (ky, kx), channel pair, one fmaf chain; then the chunks' sums one after the other.
//   forward:  src is read through the nearest x 2 map (`up`); epilogue + bias, BatchNorm, ReLU; writes the activation and its sign mask.
//   backward: the same kernel on the adjoint-packed filters (flipped taps, ci <-> co); the prologue multiplies the incoming gradient by
//             its layer's mask and BatchNorm scale; with `pool` the epilogue sums 2 x 2 blocks (the adjoint of nearest x 2).
struct ConvArgs {
    const float* src;          // [B][128][H >> up][W >> up]
    const float* wpk;          // [128 / CC][KS^2][CC][128]
    const uint32_t* mask_in;   // backward: [B][128][H][W / 32]
    const float* scale_in;     // backward: [128] BatchNorm w / sqrt(var + eps)
    const float* bias;         // forward: [128] (zeros where the convolution has none)
    const float* bn;           // forward: [4][128] running mean, running var, weight, bias
    float* out;                // [B][128][H >> pool][W >> pool]
    uint32_t* mask_out;        // forward: [B][128][H][W / 32]
    int H, W, up, bwd, pool;
};

template <int KS>
struct ConvCfg {
    static constexpr int PAD = KS / 2, CC = KS == 5 ? 4 : 8, TH = 4, TW = 32, RH = TH + KS - 1, RW = TW + KS - 1;
    static constexpr int PLANE = RH * RW, NPOS = (PLANE + 255) / 256;   // positions of one channel's tile; per thread
    static constexpr int IN_FLOATS = CC * RH * RW, W_FLOATS = KS * KS * CC * CH, NCHUNK = CH / CC;
    static_assert((IN_FLOATS + W_FLOATS) * 4 <= 64 * 1024 && W_FLOATS % 4 == 0 && CH % CC == 0 && CC % 2 == 0, "tiling");
};

// RAW (training, wgan_train.hip): the prologue applies no mask and no scale -- in training the incoming gradient is already complete --
// and the epilogue writes the convolution (+ bias where there is one) and nothing else, or its 2 x 2 block sums with `pool`.
// The template argument is KS, + 100 for RAW: the existing instantiations keep their symbols and their code.
template <int KSM>
__global__ __launch_bounds__(256) void conv128_kernel(ConvArgs a) {
    constexpr int KS = KSM % 100;
    constexpr bool RAW = KSM >= 100;
    using K = ConvCfg<KS>;
    __shared__ __align__(16) float w_s[K::W_FLOATS];
    __shared__ float in_s[K::IN_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int l31 = lane & 31, kh = lane >> 5;
    const int n = blockIdx.z, y0 = blockIdx.y * K::TH, x0 = blockIdx.x * K::TW;
    const int H = a.H, W = a.W, up = a.up, Hs = H >> up, Ws = W >> up, MW = W >> 5;
    const bool bwd = a.bwd != 0;
    const float* src = a.src + (size_t)n * CH * Hs * Ws;
    const uint32_t* mk = (!RAW && bwd) ? a.mask_in + (size_t)n * CH * H * MW : nullptr;

    // where this thread's positions of the input tile (the same in every channel and chunk) lie in the source plane and in the mask
    // words; -1: zero padding
    int soff[K::NPOS], moff[K::NPOS], shift[K::NPOS];
#pragma unroll
    for (int i = 0; i < K::NPOS; ++i) {
        const int p = tid + 256 * i, r = p / K::RW, c = p % K::RW;
        const int yy = y0 - K::PAD + r, xx = x0 - K::PAD + c;
        const bool in = p < K::PLANE && yy >= 0 && yy < H && xx >= 0 && xx < W;
        soff[i] = in ? (yy >> up) * Ws + (xx >> up) : -1;
        moff[i] = in ? yy * MW + (xx >> 5) : 0;
        shift[i] = xx & 31;
    }

    // a chunk's products are summed one after the other into `part`, the chunks one after the other into `acc`
    f16v acc[2][2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;

    for (int ch = 0; ch < K::NCHUNK; ++ch) {
        f16v part[2][2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) part[mb][nb][r] = 0.f;
        __syncthreads();                               // everyone is done with the previous chunk
        const float4* wsrc = reinterpret_cast<const float4*>(a.wpk + (size_t)ch * K::W_FLOATS);
        for (int e = tid; e < K::W_FLOATS / 4; e += 256) reinterpret_cast<float4*>(w_s)[e] = wsrc[e];
#pragma unroll
        for (int i = 0; i < K::NPOS; ++i) {
            const int p = tid + 256 * i;
            if (p < K::PLANE) {
#pragma unroll
                for (int ci = 0; ci < K::CC; ++ci) {
                    const int cg = ch * K::CC + ci;
                    float v = 0.f;
                    if (soff[i] >= 0) {
                        v = src[(size_t)cg * Hs * Ws + soff[i]];
                        if constexpr (!RAW)
                            if (bwd) {
                                const uint32_t m = mk[(size_t)cg * H * MW + moff[i]];
                                v = ((m >> shift[i]) & 1u) ? v * a.scale_in[cg] : 0.f;
                            }
                    }
                    in_s[ci * K::PLANE + p] = v;
                }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int ky = 0; ky < KS; ++ky)
#pragma unroll
            for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                for (int cp = 0; cp < K::CC / 2; ++cp) {
                    const int ci = 2 * cp + kh;
                    const float* wp = w_s + ((ky * KS + kx) * K::CC + ci) * CH + wn * 64 + l31;
                    const float* ip = in_s + (ci * K::RH + 2 * wm + ky) * K::RW + l31 + kx;
                    const float w0 = wp[0], w1 = wp[32], i0 = ip[0], i1 = ip[K::RW];
                    part[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, i0, part[0][0], 0, 0, 0);
                    part[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, i0, part[0][1], 0, 0, 0);
                    part[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, i1, part[1][0], 0, 0, 0);
                    part[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, i1, part[1][1], 0, 0, 0);
                }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mb][nb][r] += part[mb][nb][r];
    }

    // D layout: channel (row) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the block, pixel (column) = lane & 31
    const int x = x0 + l31;
    if constexpr (RAW) {
        // the convolution (+ bias) and nothing else; with `pool` (the launcher sets bwd with it) the pooled epilogue below
        if (!a.pool) {
            float* out = a.out + (size_t)n * CH * H * W;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = wn * 64 + nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    const float bias = a.bias ? a.bias[c] : 0.f;
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) out[((size_t)c * H + y0 + 2 * wm + mb) * W + x] = a.bias ? acc[mb][nb][r] + bias : acc[mb][nb][r];
                }
            return;
        }
    }
    if (!bwd) {
        float* out = a.out + (size_t)n * CH * H * W;
        uint32_t* mo = a.mask_out + (size_t)n * CH * H * MW;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = wn * 64 + nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const float bias = a.bias[c], mean = a.bn[c], sd = sqrtf(a.bn[CH + c] + BN_EPS), gw = a.bn[2 * CH + c], gb = a.bn[3 * CH + c];
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
#pragma clang fp contract(off)                       // two roundings for * w + b, as the reference's separate multiply and add
                    const int y = y0 + 2 * wm + mb;
                    float v = acc[mb][nb][r] + bias;
                    v = (v - mean) / sd * gw + gb;
                    const bool pos = v > 0.f;
                    out[((size_t)c * H + y) * W + x] = pos ? v : 0.f;
                    const unsigned long long bal = __ballot(pos);
                    if (l31 == 0) mo[((size_t)c * H + y) * MW + blockIdx.x] = kh ? (uint32_t)(bal >> 32) : (uint32_t)bal;
                }
            }
    } else if (!a.pool) {
        float* out = a.out + (size_t)n * CH * H * W;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = wn * 64 + nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) out[((size_t)c * H + y0 + 2 * wm + mb) * W + x] = acc[mb][nb][r];
            }
    } else {
        // the wavefront's two rows are one row pair (y0 is a multiple of 4): ((a00 + a01) + (a10 + a11))
        const int Hp = H >> 1, Wp = W >> 1;
        float* out = a.out + (size_t)n * CH * Hp * Wp;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = wn * 64 + nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const float t0 = acc[0][nb][r], t1 = acc[1][nb][r];
                const float h0 = t0 + __shfl_xor(t0, 1), h1 = t1 + __shfl_xor(t1, 1);
                if ((lane & 1) == 0) out[((size_t)c * Hp + (y0 >> 1) + wm) * Wp + (x >> 1)] = h0 + h1;
            }
    }
}

// ---- filters of one layer from the torch layout into the two packings of conv128 (pack_conv below, on the device) ----------------
// training repacks after every generator update; grid (CH * CH * KS^2 / 256), thread e = one element of the torch tensor [co][ci][tap]
__global__ __launch_bounds__(256) void repack128_kernel(const float* __restrict__ w, float* __restrict__ fwd, float* __restrict__ adj, int T, int CC) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= CH * CH * T) return;
    const int co = e / (CH * T), ci = (e / T) % CH, t = e % T;
    const float v = w[e];
    fwd[(((size_t)(ci / CC) * T + t) * CC + ci % CC) * CH + co] = v;
    adj[(((size_t)(co / CC) * T + (T - 1 - t)) * CC + co % CC) * CH + ci] = v;
}

// ---- out: 5 x 5 convolution 128 -> 2 + bias; R = G P - Y; meas; oracle NMSE; dG = 2 s R P^H --------------------------------------
// One workgroup per sample.  A thread owns 4 vertically adjacent pixels x both output channels; the input streams through LDS in
// chunks of 4 channels: a chunk's 100 products are summed one after the other in (ci, ky, kx) order, then the chunks' sums.  The scalar logs are summed in float64.
struct OutArgs {
    const float* act;          // [B][128][16][64]
    const float* w;            // [2][128][5][5]
    const float* bias;         // [2]
    const float* P;            // [B][64][Np] complex
    const float* Y;            // [B][16][Np] complex
    const float* Htrue;        // [B][16][64] complex or NULL
    const float* loss_scale;   // [B]
    float* gen;                // [B][2][16][64]
    float* dG;                 // [B][2][16][64]
    float* meas_log;           // [B] of this step or NULL
    float* oracle_log;         // [B] of this step or NULL
    int Np, run;               // run = 0: the generator only
};

constexpr int OUT_RW = NT + 4, OUT_PLANE = (NR + 4) * OUT_RW, OUT_CC = 4;

__global__ __launch_bounds__(256) void out_kernel(OutArgs a) {
    constexpr int BUF = 2 * PIX + 2 * NT * NT + 2 * NR * NT;     // phase 2: gen | P | R
    static_assert(OUT_CC * OUT_PLANE + 2 * CH * 25 <= BUF, "the convolution phase fits the same buffer");
    __shared__ __align__(16) float buf[BUF];
    __shared__ double red[4];
    const int tid = threadIdx.x, n = blockIdx.x;
    const int x = tid & 63, yb = (tid >> 6) * 4;
    float* in_s = buf;
    float* w_s = buf + OUT_CC * OUT_PLANE;
    for (int e = tid; e < 2 * CH * 25; e += 256) w_s[e] = a.w[e];
    float o[2][4];
#pragma unroll
    for (int co = 0; co < 2; ++co)
#pragma unroll
        for (int p = 0; p < 4; ++p) o[co][p] = 0.f;
    const float* act = a.act + (size_t)n * CH * PIX;
    for (int c0 = 0; c0 < CH; c0 += OUT_CC) {
        __syncthreads();
        SBC_NO_VEC for (int e = tid; e < OUT_CC * OUT_PLANE; e += 256) {
            const int ci = e / OUT_PLANE, rem = e % OUT_PLANE, yy = rem / OUT_RW - 2, xx = rem % OUT_RW - 2;
            in_s[e] = (yy >= 0 && yy < NR && xx >= 0 && xx < NT) ? act[(size_t)(c0 + ci) * PIX + yy * NT + xx] : 0.f;
        }
        __syncthreads();
        float part[2][4];
#pragma unroll
        for (int co = 0; co < 2; ++co)
#pragma unroll
            for (int p = 0; p < 4; ++p) part[co][p] = 0.f;
        SBC_NO_VEC_NO_UNROLL for (int ci = 0; ci < OUT_CC; ++ci) {
            float v[8][5];
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int k = 0; k < 5; ++k) v[r][k] = in_s[ci * OUT_PLANE + (yb + r) * OUT_RW + x + k];
#pragma unroll
            for (int co = 0; co < 2; ++co) {
                const float* w25 = w_s + (co * CH + c0 + ci) * 25;
#pragma unroll
                for (int ky = 0; ky < 5; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 5; ++kx) {
                        const float wv = w25[ky * 5 + kx];
#pragma unroll
                        for (int p = 0; p < 4; ++p) part[co][p] = fmaf(v[p + ky][kx], wv, part[co][p]);
                    }
            }
        }
#pragma unroll
        for (int co = 0; co < 2; ++co)
#pragma unroll
            for (int p = 0; p < 4; ++p) o[co][p] += part[co][p];
    }
    __syncthreads();                                   // the convolution's LDS becomes gen | P | R
    float* g_s = buf;
    float2* P_s = reinterpret_cast<float2*>(buf + 2 * PIX);
    float2* R_s = reinterpret_cast<float2*>(buf + 2 * PIX + 2 * NT * NT);
    float* gen = a.gen + (size_t)n * 2 * PIX;
#pragma unroll
    for (int co = 0; co < 2; ++co)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float v = o[co][p] + a.bias[co];
            g_s[co * PIX + (yb + p) * NT + x] = v;
            gen[co * PIX + (yb + p) * NT + x] = v;
        }
    if (!a.run) return;
    const int Np = a.Np;
    const float2* P = reinterpret_cast<const float2*>(a.P) + (size_t)n * NT * Np;
    const float2* Y = reinterpret_cast<const float2*>(a.Y) + (size_t)n * NR * Np;
    for (int e = tid; e < NT * Np; e += 256) P_s[e] = P[e];
    __syncthreads();
    // R[r][p] = sum_t G[r][t] P[t][p] - Y[r][p], t in order
    double m = 0.0;
    for (int e = tid; e < NR * Np; e += 256) {
        const int r = e / Np, p = e % Np;
        float sr = 0.f, si = 0.f;
        for (int t = 0; t < NT; ++t) {
            const float gr = g_s[r * NT + t], gi = g_s[PIX + r * NT + t];
            const float2 pv = P_s[t * Np + p];
            sr = fmaf(gr, pv.x, sr); sr = fmaf(-gi, pv.y, sr);
            si = fmaf(gr, pv.y, si); si = fmaf(gi, pv.x, si);
        }
        const float2 yv = Y[e];
        const float2 rv = make_float2(sr - yv.x, si - yv.y);
        R_s[e] = rv;
        m += (double)rv.x * rv.x + (double)rv.y * rv.y;
    }
    m = block_sum256(m, red);                          // (also orders R_s before the reads below)
    if (a.meas_log && tid == 0) a.meas_log[n] = (float)m;
    if (a.oracle_log && a.Htrue) {
        const float2* Ht = reinterpret_cast<const float2*>(a.Htrue) + (size_t)n * PIX;
        double err = 0.0, hn = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = tid + 256 * k;
            const float2 t = Ht[e];
            const float dx = g_s[e] - t.x, dy = g_s[PIX + e] - t.y;
            err += (double)dx * dx + (double)dy * dy;
            hn += (double)t.x * t.x + (double)t.y * t.y;
        }
        err = block_sum256(err, red);
        hn = block_sum256(hn, red);
        if (tid == 0) a.oracle_log[n] = (float)(err / hn);
    }
    // dG[r][t] = 2 s sum_p R[r][p] conj(P[t][p]), p in order; planes (re, im)
    const float s2 = 2.f * a.loss_scale[n];
    float* dG = a.dG + (size_t)n * 2 * PIX;
    SBC_NO_VEC_NO_UNROLL for (int k = 0; k < 4; ++k) {
        const int e = tid + 256 * k, r = e / NT, t = e % NT;
        float sr = 0.f, si = 0.f;
        for (int p = 0; p < Np; ++p) {
            const float2 rv = R_s[r * Np + p], pv = P_s[t * Np + p];
            sr = fmaf(rv.x, pv.x, sr); sr = fmaf(rv.y, pv.y, sr);
            si = fmaf(rv.y, pv.x, si); si = fmaf(-rv.x, pv.y, si);
        }
        dG[e] = s2 * sr;
        dG[PIX + e] = s2 * si;
    }
}

// ---- out adjoint: g[ci][y][x] = sum_co sum_tap w[co][ci][ky][kx] dG[co][y - ky + 2][x - kx + 2] -----------------------------------
// grid (128 / 32, B).  A thread holds the 2 x 8 x 5 window of dG its 4 vertically adjacent pixels need and walks 32 channels.
constexpr int OA_CG = 32;
__global__ __launch_bounds__(256) void out_adjoint_kernel(const float* __restrict__ dG, const float* __restrict__ w, float* __restrict__ out) {
    __shared__ float dg_s[2 * OUT_PLANE];
    __shared__ float w_s[OA_CG * 50];
    const int tid = threadIdx.x, c0 = blockIdx.x * OA_CG, n = blockIdx.y;
    const float* d = dG + (size_t)n * 2 * PIX;
    SBC_NO_VEC for (int e = tid; e < 2 * OUT_PLANE; e += 256) {
        const int co = e / OUT_PLANE, rem = e % OUT_PLANE, yy = rem / OUT_RW - 2, xx = rem % OUT_RW - 2;
        dg_s[e] = (yy >= 0 && yy < NR && xx >= 0 && xx < NT) ? d[co * PIX + yy * NT + xx] : 0.f;
    }
    for (int e = tid; e < OA_CG * 50; e += 256) {
        const int cl = e / 50, rem = e % 50, co = rem / 25, tap = rem % 25;
        w_s[e] = w[((size_t)co * CH + c0 + cl) * 25 + tap];
    }
    __syncthreads();
    const int x = tid & 63, yb = (tid >> 6) * 4;
    float v[2][8][5];
#pragma unroll
    for (int co = 0; co < 2; ++co)
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int k = 0; k < 5; ++k) v[co][r][k] = dg_s[co * OUT_PLANE + (yb + r) * OUT_RW + x + k];
    float* o = out + ((size_t)n * CH + c0) * PIX + yb * NT + x;
    SBC_NO_VEC_NO_UNROLL for (int cl = 0; cl < OA_CG; ++cl) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int co = 0; co < 2; ++co)
#pragma unroll
            for (int ky = 0; ky < 5; ++ky)
#pragma unroll
                for (int kx = 0; kx < 5; ++kx) {
                    const float wv = w_s[(cl * 2 + co) * 25 + ky * 5 + kx];
#pragma unroll
                    for (int p = 0; p < 4; ++p) s[p] = fmaf(v[co][p + 4 - ky][4 - kx], wv, s[p]);
                }
#pragma unroll
        for (int p = 0; p < 4; ++p) o[(size_t)cl * PIX + p * NT] = s[p];
    }
}

// ---- dense adjoint + Adam -----------------------------------------------------------------------------------------------------
// One workgroup per sample.  gz[j] = sum_f Wt[j][f] g0[f]: a wavefront per j, a lane sums f = lane, lane + 64, .. in order, then the
// butterfly.  g = gz + (2 s lambda) z; then torch.optim.Adam's defaults in its order of operations, without contraction:
//     m += (g - m)(1 - b1);  v = v b2 + (1 - b2) g g;  denom = sqrt(v) / sqrt(1 - b2^t) + eps;  z -= (lr / (1 - b1^t)) (m / denom)
struct AdamArgs {
    const float* g0;           // [B][8192]
    const float* Wt;           // [60][8192]
    float* z; float* m; float* v;   // [B][60]
    const float* lr; const float* lam; const float* scale;   // [B]
    float* reg_log;            // [B] of this step or NULL
    float* z_log;              // [B][60] of this step or NULL: z before the update
    float* g_log;              // [B][60] of this step or NULL
    double bc1, bc2_sqrt;      // 1 - b1^t, sqrt(1 - b2^t)
};

__device__ __forceinline__ void adam_update(float g, float lr, double bc1, double bc2_sqrt, float& z, float& m, float& v) {
#pragma clang fp contract(off)
    const float w1 = (float)(1.0 - 0.9), b2 = (float)0.999, w2 = (float)(1.0 - 0.999), eps = (float)1e-8;
    m = m + (g - m) * w1;
    v = v * b2 + (w2 * g) * g;
    const float denom = sqrtf(v) / (float)bc2_sqrt + eps;
    const float step = (float)((double)lr / bc1);
    z = z - step * (m / denom);
}

__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
    __shared__ float gz[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x;
    const float* g0 = a.g0 + (size_t)n * DENSE;
    for (int j = wave; j < NZ; j += 4) {
        const float* wt = a.Wt + (size_t)j * DENSE;
        float s = 0.f;
        SBC_NO_VEC for (int f = lane; f < DENSE; f += 64) s = fmaf(wt[f], g0[f], s);
        s = wave_sum(s);
        if (lane == 0) gz[j] = s;
    }
    __syncthreads();
    if (tid >= 64) return;
    const size_t i = (size_t)n * NZ + tid;
    float z = tid < NZ ? a.z[i] : 0.f;
    const double reg = wave_sum((double)z * z);
    if (a.reg_log && tid == 0) a.reg_log[n] = (float)reg;
    if (tid >= NZ) return;
    const float g = gz[tid] + (2.f * (a.scale[n] * a.lam[n])) * z;
    if (a.z_log) a.z_log[i] = z;
    if (a.g_log) a.g_log[i] = g;
    float m = a.m[i], v = a.v[i];
    adam_update(g, a.lr[n], a.bc1, a.bc2_sqrt, z, m, v);
    a.z[i] = z; a.m[i] = m; a.v[i] = v;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// workspace of one sample, in floats (masks: 32-bit words), in order: activations 0 .. L, gen, dG, gradients L .. 0, masks 1 .. L
struct Layout {
    int L;
    int64_t act[MAX_L + 1], grad[MAX_L + 1], mask[MAX_L + 1], gen, dg, total;
    explicit Layout(int n_extra) : L(2 + n_extra) {
        int64_t o = 0;
        auto take = [&](int64_t n) { const int64_t at = o; o += n; return at; };
        act[0] = take(DENSE);
        for (int k = 1; k <= L; ++k) act[k] = take((int64_t)CH * layer_h(k) * layer_w(k));
        gen = take(2 * PIX);
        dg = take(2 * PIX);
        for (int k = L; k >= 1; --k) grad[k] = take((int64_t)CH * layer_h(k) * layer_w(k));
        grad[0] = take(DENSE);
        mask[0] = -1;
        for (int k = 1; k <= L; ++k) mask[k] = take((int64_t)CH * mask_words(layer_h(k), layer_w(k)));
        total = o;
    }
};

// stage ids of sbc_wgan_stage
enum { ST_ACT = 0, ST_GEN = 16, ST_DG = 17, ST_GRAD = 32, ST_MASK = 48 };

}  // namespace

// ---- what training launches of this file (wgan_shared.h) --------------------------------------------------------------------------------
namespace wgan_shared {

void launch_dense(const float* z, const float* W, const float* bias, float* out, int B, hipStream_t s) {
    hipLaunchKernelGGL(dense_kernel, dim3(DENSE / 256, B), dim3(256), 0, s, z, W, bias, out);
}

void launch_conv128_raw(const float* src, const float* wpk, const float* bias, float* out, int H, int W, int ks, int up, int pool, int B, hipStream_t s) {
    ConvArgs a{};
    a.src = src; a.wpk = wpk; a.bias = bias; a.out = out; a.H = H; a.W = W; a.up = up; a.pool = pool; a.bwd = pool;
    const dim3 grid(W / 32, H / 4, B);
    if (ks == 5) hipLaunchKernelGGL(conv128_kernel<105>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(conv128_kernel<103>, grid, dim3(256), 0, s, a);
}

void launch_out_conv(const float* act, const float* w, const float* bias, float* gen, int B, hipStream_t s) {
    OutArgs oa{};
    oa.act = act; oa.w = w; oa.bias = bias; oa.gen = gen;
    hipLaunchKernelGGL(out_kernel, dim3(B), dim3(256), 0, s, oa);
}

void launch_out_adjoint(const float* dG, const float* w, float* out, int B, hipStream_t s) {
    hipLaunchKernelGGL(out_adjoint_kernel, dim3(CH / OA_CG, B), dim3(256), 0, s, dG, w, out);
}

void launch_repack128(const float* w, float* fwd, float* adj, int ks, hipStream_t s) {
    const int T = ks * ks;
    hipLaunchKernelGGL(repack128_kernel, dim3(CH * CH * T / 256), dim3(256), 0, s, w, fwd, adj, T, ks == 5 ? ConvCfg<5>::CC : ConvCfg<3>::CC);
}

}  // namespace wgan_shared
}  // namespace sbc

struct sbc_wgan {
    int n_extra = 0;
    sbc::ParamImage params;
    // offsets into params
    size_t dense_w = 0, dense_b = 0, dense_wt = 0, out_w = 0, out_b = 0;
    size_t fwd[sbc::MAX_L + 1] = {}, adj[sbc::MAX_L + 1] = {}, bias[sbc::MAX_L + 1] = {}, bn[sbc::MAX_L + 1] = {}, scale[sbc::MAX_L + 1] = {};
};

namespace sbc {
namespace {

// torch [co][ci][KS][KS] -> [ci / CC][tap][ci % CC][co] (forward) or, adjoint, the same packing of the flipped, transposed filter
// w'[ci][co][ky][kx] = w[co][ci][KS - 1 - ky][KS - 1 - kx]
void pack_conv(const float* w, int KS, int CC, bool adjoint, float* out) {
    const int T = KS * KS;
    for (int k = 0; k < CH; ++k)            // the GEMM's K channel (read from LDS tile)
        for (int t = 0; t < T; ++t)
            for (int j = 0; j < CH; ++j) {  // the GEMM's output channel
                const float v = adjoint ? w[((size_t)k * CH + j) * T + (T - 1 - t)] : w[((size_t)j * CH + k) * T + t];
                out[(((size_t)(k / CC) * T + t) * CC + k % CC) * CH + j] = v;
            }
}

void conv128(const sbc_wgan* h, int k, bool bwd, const float* src, const uint32_t* mask_in, float* out, uint32_t* mask_out, int B, hipStream_t s) {
    ConvArgs a{};
    a.src = src; a.wpk = h->params.dev + (bwd ? h->adj[k] : h->fwd[k]); a.mask_in = mask_in; a.scale_in = h->params.dev + h->scale[k];
    a.bias = h->params.dev + h->bias[k]; a.bn = h->params.dev + h->bn[k]; a.out = out; a.mask_out = mask_out;
    a.H = layer_h(k); a.W = layer_w(k); a.up = (!bwd && k <= 2) ? 1 : 0; a.bwd = bwd ? 1 : 0; a.pool = (bwd && k <= 2) ? 1 : 0;
    const dim3 grid(a.W / 32, a.H / 4, B);
    if (layer_ks(k) == 5) hipLaunchKernelGGL(conv128_kernel<5>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(conv128_kernel<3>, grid, dim3(256), 0, s, a);
}

struct Ws {
    float* base;
    int B;
    Layout lay;
    float* act(int k) const { return base + lay.act[k] * B; }
    float* grad(int k) const { return base + lay.grad[k] * B; }
    uint32_t* mask(int k) const { return reinterpret_cast<uint32_t*>(base + lay.mask[k] * B); }
    float* gen() const { return base + lay.gen * B; }
    float* dg() const { return base + lay.dg * B; }
};

void forward(const sbc_wgan* h, const Ws& ws, const float* z, hipStream_t s) {
    const int B = ws.B, L = ws.lay.L;
    hipLaunchKernelGGL(dense_kernel, dim3(DENSE / 256, B), dim3(256), 0, s, z, h->params.dev + h->dense_w, h->params.dev + h->dense_b, ws.act(0));
    for (int k = 1; k <= L; ++k) conv128(h, k, false, ws.act(k - 1), nullptr, ws.act(k), ws.mask(k), B, s);
}

}  // namespace

}  // namespace sbc

extern "C" {

int sbc_wgan_create(const sbc_tensor_ref* tensors, int32_t n_tensors, sbc_wgan** out) {
    using namespace sbc;
    SBC_REQUIRE(tensors && out && n_tensors > 0, "sbc_wgan_create: need tensors and out");
    TensorIndex sd;
    int n_extra = 0;
    const int rc = open_generator("sbc_wgan_create", tensors, n_tensors, "tensor", sd, &n_extra);
    if (rc) return rc;
    const int L = 2 + n_extra;
    sbc_wgan* h = new sbc_wgan;
    h->n_extra = n_extra;
    std::vector<float>& host = h->params.host;
    auto take = [&](size_t n) { return h->params.take(n); };
    std::map<std::string, int64_t> numel;
    for (const auto& t : generator_tensors(n_extra)) numel.insert(t);
    bool ok = true;                                      // false after the first tensor that is missing or mis-sized: its message stays
    auto fetch = [&](const std::string& name) -> const float* {
        const float* p = ok ? sd.find(name, numel.at(name)) : nullptr;
        if (!p) ok = false;
        return p;
    };
    // a tensor as it is: at `at`, or behind what is there (returns its offset)
    auto place = [&](const std::string& name, size_t at) {
        if (const float* p = fetch(name)) memcpy(host.data() + at, p, sizeof(float) * numel.at(name));
    };
    auto add = [&](const std::string& name) {
        const size_t at = take((size_t)numel.at(name));
        place(name, at);
        return at;
    };
    h->dense_w = add("dense.dense_input.weight");
    h->dense_wt = take((size_t)DENSE * NZ);              // and its transpose, for the dense adjoint
    for (int f = 0; f < DENSE; ++f)
        for (int j = 0; j < NZ; ++j) host[h->dense_wt + (size_t)j * DENSE + f] = host[h->dense_w + (size_t)f * NZ + j];
    h->dense_b = add("dense.dense_input.bias");
    for (int k = 1; k <= L && ok; ++k) {
        const std::string conv = conv_name(k), bn = bn_name(k);
        const int KS = layer_ks(k), CC = KS == 5 ? ConvCfg<5>::CC : ConvCfg<3>::CC;
        if (const float* w = fetch(conv + ".weight")) {
            const size_t wn = (size_t)numel.at(conv + ".weight");
            h->fwd[k] = take(wn);
            pack_conv(w, KS, CC, false, host.data() + h->fwd[k]);
            h->adj[k] = take(wn);
            pack_conv(w, KS, CC, true, host.data() + h->adj[k]);
        }
        h->bias[k] = take(CH);
        if (k <= 2) place(conv + ".bias", h->bias[k]);
        h->bn[k] = take(4 * CH);
        const char* part[4] = {".running_mean", ".running_var", ".weight", ".bias"};
        for (int q = 0; q < 4; ++q) place(bn + part[q], h->bn[k] + (size_t)q * CH);
        h->scale[k] = take(CH);
        if (ok)
            for (int c = 0; c < CH; ++c) {
                const float* b4 = host.data() + h->bn[k];
                host[h->scale[k] + c] = b4[2 * CH + c] * (1.f / sqrtf(b4[CH + c] + BN_EPS));
            }
    }
    h->out_w = add("conv.conv_out.weight");
    h->out_b = add("conv.conv_out.bias");
    const int rc_up = ok ? h->params.upload("sbc_wgan_create") : SBC_ERR_INVALID;
    if (rc_up) {
        delete h;
        return rc_up;
    }
    *out = h;
    return SBC_OK;
}

void sbc_wgan_destroy(sbc_wgan* h) {
    if (!h) return;
    h->params.release();
    delete h;
}

int64_t sbc_wgan_workspace_floats(const sbc_wgan* h, int32_t B) {
    if (!h || B < 0) return -1;
    return sbc::Layout(h->n_extra).total * B;
}

int sbc_wgan_stage(const sbc_wgan* h, int32_t stage, int32_t B, int64_t* offset, int32_t* channels, int32_t* height, int32_t* width) {
    using namespace sbc;
    SBC_REQUIRE(h && B >= 0 && offset && channels && height && width, "sbc_wgan_stage: NULL handle or output, or B < 0");
    const Layout lay(h->n_extra);
    const int L = lay.L;
    int64_t off = -1;
    int c = CH, hh = 0, ww = 0;
    auto dims = [&](int k) { hh = layer_h(k); ww = layer_w(k); };
    if (stage >= ST_ACT && stage <= ST_ACT + L) { off = lay.act[stage - ST_ACT]; dims(stage - ST_ACT); }
    else if (stage == ST_GEN || stage == ST_DG) { off = stage == ST_GEN ? lay.gen : lay.dg; c = 2; hh = NR; ww = NT; }
    else if (stage >= ST_GRAD && stage <= ST_GRAD + L) { off = lay.grad[stage - ST_GRAD]; dims(stage - ST_GRAD); }
    else if (stage >= ST_MASK + 1 && stage <= ST_MASK + L) { off = lay.mask[stage - ST_MASK]; dims(stage - ST_MASK); ww /= 32; }
    SBC_REQUIRE(off >= 0, "sbc_wgan_stage: no stage %d in a generator with %d extra layers", stage, h->n_extra);
    *offset = off * B;
    *channels = c;
    *height = hh;
    *width = ww;
    return SBC_OK;
}

int sbc_wgan_generate(sbc_wgan* h, const float* z, float* out, int32_t B, float* workspace, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(h && z && out && workspace, "sbc_wgan_generate: NULL handle, z, out or workspace");
    SBC_REQUIRE(B >= 0 && B <= 32768, "sbc_wgan_generate: B must be in [0, 32768] (got %d)", B);
    const int rc = h->params.check_device("sbc_wgan_generate");
    if (rc) return rc;
    if (B == 0) return SBC_OK;
    hipStream_t s = (hipStream_t)stream;
    const Ws ws{workspace, B, Layout(h->n_extra)};
    forward(h, ws, z, s);
    OutArgs oa{};
    oa.act = ws.act(ws.lay.L); oa.w = h->params.dev + h->out_w; oa.bias = h->params.dev + h->out_b; oa.gen = ws.gen();
    hipLaunchKernelGGL(out_kernel, dim3(B), dim3(256), 0, s, oa);
    SBC_CHECK_HIP(hipGetLastError());
    SBC_CHECK_HIP(hipMemcpyAsync(out, ws.gen(), sizeof(float) * 2 * PIX * (size_t)B, hipMemcpyDeviceToDevice, s));
    return SBC_OK;
}

int sbc_wgan_run(sbc_wgan* h, const sbc_wgan_run_desc* d, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(h && d, "sbc_wgan_run: NULL handle or descriptor");
    SBC_REQUIRE(d->Np >= 1 && d->Np <= NT, "sbc_wgan_run: Np must be in [1, %d] (got %d)", NT, d->Np);
    SBC_REQUIRE(d->B >= 0 && d->B <= 32768, "sbc_wgan_run: B must be in [0, 32768] (got %d)", d->B);
    SBC_REQUIRE(d->n_steps >= 0 && d->first_step >= 1, "sbc_wgan_run: need n_steps >= 0 and first_step >= 1 (got %d, %d)", d->n_steps, d->first_step);
    const struct { const void* p; const char* name; } need[] = {{d->Y, "Y"}, {d->P, "P"}, {d->z, "z"}, {d->m, "m"}, {d->v, "v"}, {d->lr, "lr"},
                                                                 {d->l2_lam, "l2_lam"}, {d->loss_scale, "loss_scale"}, {d->workspace, "workspace"}};
    for (const auto& q : need) SBC_REQUIRE(q.p, "sbc_wgan_run: NULL %s", q.name);
    SBC_REQUIRE(!d->oracle_log || d->H, "sbc_wgan_run: oracle_log needs H");
    const int rc = h->params.check_device("sbc_wgan_run");
    if (rc) return rc;
    if (d->B == 0 || d->n_steps == 0) return SBC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int B = d->B;
    const Ws ws{d->workspace, B, Layout(h->n_extra)};
    const int L = ws.lay.L;
    for (int k = 0; k < d->n_steps; ++k) {
        const double t = (double)d->first_step + k;
        forward(h, ws, d->z, s);
        OutArgs oa{};
        oa.act = ws.act(L); oa.w = h->params.dev + h->out_w; oa.bias = h->params.dev + h->out_b; oa.P = d->P; oa.Y = d->Y; oa.Htrue = d->H;
        oa.loss_scale = d->loss_scale; oa.gen = ws.gen(); oa.dG = ws.dg();
        oa.meas_log = d->meas_log ? d->meas_log + (size_t)k * B : nullptr;
        oa.oracle_log = d->oracle_log ? d->oracle_log + (size_t)k * B : nullptr;
        oa.Np = d->Np; oa.run = 1;
        hipLaunchKernelGGL(out_kernel, dim3(B), dim3(256), 0, s, oa);
        hipLaunchKernelGGL(out_adjoint_kernel, dim3(CH / OA_CG, B), dim3(256), 0, s, ws.dg(), h->params.dev + h->out_w, ws.grad(L));
        for (int l = L; l >= 1; --l) conv128(h, l, true, ws.grad(l), ws.mask(l), ws.grad(l - 1), nullptr, B, s);
        AdamArgs aa{};
        aa.g0 = ws.grad(0); aa.Wt = h->params.dev + h->dense_wt; aa.z = d->z; aa.m = d->m; aa.v = d->v;
        aa.lr = d->lr; aa.lam = d->l2_lam; aa.scale = d->loss_scale;
        aa.reg_log = d->reg_log ? d->reg_log + (size_t)k * B : nullptr;
        aa.z_log = d->z_log ? d->z_log + (size_t)k * B * NZ : nullptr;
        aa.g_log = d->g_log ? d->g_log + (size_t)k * B * NZ : nullptr;
        aa.bc1 = 1.0 - pow(0.9, t);
        aa.bc2_sqrt = sqrt(1.0 - pow(0.999, t));
        hipLaunchKernelGGL(adam_kernel, dim3(B), dim3(256), 0, s, aa);
    }
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

}  // extern "C"
