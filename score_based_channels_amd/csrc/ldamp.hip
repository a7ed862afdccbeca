// Learned D-AMP (the L-DAMP baseline of Fig. 5c): src/score_based_channels/test_ldamp.py, aux_models.py:62-190 (LDAMP.forward) and
// aux_unet.py (FlippedNormUnet / Unet / ConvBlock / TransposeConvBlock), configuration of train_ldamp.py:41-47: one FlippedNormUnet
// (chans 16, 3 pools) per unroll, Nt x Nr = 64 x 16.
//
// Per unroll u, with denoiser D_u(x) = x - unnorm(U_u(norm(x))):
//     r = h + (1 / eig1) P^H z;  h = D_u(r);  eps = max(1e-3 max|r|, 1e-5);  h' = D_u(r + eps d);
//     div = (1 / eps) mean(d (h' - h));  z = Y - P h + z div
// The clean and the perturbed evaluation run as ONE batch of 2B images through the same launches (image b and image B + b).
//
// Arithmetic: exact fp32 (v_fma_f32), fp32 accumulation.  Every sum has a fixed order: a convolution adds its 9 * 8 (or 9 * 2) products
// of one input-channel chunk one after the other and then the chunks one after the other; statistics are summed per lane in index
// order, then across the lanes of a wavefront by a butterfly, then across wavefronts in wavefront order.  No atomics.  An image's
// arithmetic does not depend on its position in the batch or on the batch size: a workgroup works on one image only.
//
// Activations are planar fp32 [N][C][H][W] in a caller-owned workspace, one buffer per stage (no reuse: every stage output stays
// readable after a call, which is what the per-layer tests read: sbc_ldamp_stage).  Launches per evaluation batch: prep (r, eps,
// perturbation, norm) + 14 convolutions (InstanceNorm + LeakyReLU inside, the 2 x 2 mean pool in the producer's epilogue, the concat
// read from its two sources) + 3 transposed convolutions (with their norm) + finish (1 x 1 convolution, unnorm, residual, divergence,
// z update, NMSE) = 19 per unroll.
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

// ---- directions ---------------------------------------------------------------------------------------------------------------
// d[u][b][e][0..1] = the two N(0,1) draws of philox.h::normal_pair(seed, stream = sample0 + b, step = unroll0 + u, elem = e), e = t * 16 + r
__global__ __launch_bounds__(256) void ldamp_dirs_kernel(float* __restrict__ d, uint64_t seed, int64_t sample0, int unroll0, int B) {
    const int b = blockIdx.x, u = blockIdx.y;
    float2* o = reinterpret_cast<float2*>(d) + ((size_t)u * B + b) * PIX;
    for (int e = threadIdx.x; e < PIX; e += 256) o[e] = normal_pair(seed, sample0 + b, unroll0 + u, e);
}

// ---- prep: r, eps, perturbation, norm -----------------------------------------------------------------------------------------
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

// mean and unbiased standard deviation of the 1024 values a 256-thread workgroup holds four each of, then (v - mean) / std
__device__ __forceinline__ void norm_plane(const float (&v)[4], float* red, float* xo, float* stat) {
    const float mean = block_reduce256<false>((v[0] + v[1]) + (v[2] + v[3]), red) * (1.f / PIX);
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const float d = v[k] - mean; q += d * d; }
    const float sd = sqrtf(block_reduce256<false>(q, red) * (1.f / (PIX - 1)));
#pragma unroll
    for (int k = 0; k < 4; ++k) xo[threadIdx.x + 256 * k] = (v[k] - mean) / sd;
    if (threadIdx.x == 0) { stat[0] = mean; stat[1] = sd; }
}

__global__ __launch_bounds__(256) void ldamp_prep_kernel(PrepArgs a) {
    __shared__ float2 P_s[NT * NT];
    __shared__ float2 z_s[NT * NR];
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    float2 r[4];
    if (a.r_in) {
        const float2* ri = reinterpret_cast<const float2*>(a.r_in) + (size_t)b * PIX;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = ri[tid + 256 * k];
    } else {
        const int Np = a.Np;
        const float2* P = reinterpret_cast<const float2*>(a.P) + (size_t)b * Np * NT;
        const float2* z = reinterpret_cast<const float2*>(a.z) + (size_t)b * Np * NR;
        for (int e = tid; e < Np * NT; e += 256) P_s[e] = P[e];
        for (int e = tid; e < Np * NR; e += 256) z_s[e] = z[e];
        __syncthreads();
        const float inv = 1.f / a.eig[b];
        const float2* h = a.h ? reinterpret_cast<const float2*>(a.h) + (size_t)b * PIX : nullptr;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = tid + 256 * k, t = e / NR, q = e % NR;
            float sr = 0.f, si = 0.f;
            for (int p = 0; p < Np; ++p) {                         // conj(P[p][t]) z[p][q]
                const float2 pv = P_s[p * NT + t], zv = z_s[p * NR + q];
                sr += pv.x * zv.x + pv.y * zv.y;
                si += pv.x * zv.y - pv.y * zv.x;
            }
            const float2 h0 = h ? h[e] : make_float2(0.f, 0.f);
            r[k] = make_float2(h0.x + inv * sr, h0.y + inv * si);
        }
    }
    float2* ro = reinterpret_cast<float2*>(a.r) + (size_t)b * PIX;
#pragma unroll
    for (int k = 0; k < 4; ++k) ro[tid + 256 * k] = r[k];
    {
        float re[4] = {r[0].x, r[1].x, r[2].x, r[3].x}, im[4] = {r[0].y, r[1].y, r[2].y, r[3].y};
        norm_plane(re, red, a.x + (size_t)b * 2 * PIX, a.stat + (size_t)b * 4);
        norm_plane(im, red, a.x + (size_t)b * 2 * PIX + PIX, a.stat + (size_t)b * 4 + 2);
    }
    if (a.r_in) return;
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) m = fmaxf(m, hypotf(r[k].x, r[k].y));
    m = block_reduce256<true>(m, red);
    const float eps = fmaxf(m * 1e-3f, 1e-5f);
    if (tid == 0) {
        a.eps[b] = eps;
        if (a.eps_log) a.eps_log[b] = eps;
    }
    const float2* d = reinterpret_cast<const float2*>(a.dirs) + (size_t)b * PIX;
    const int nb = a.B + b;                                          // the perturbed image
    float2* rp = reinterpret_cast<float2*>(a.r) + (size_t)nb * PIX;
    float re[4], im[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float2 dv = d[tid + 256 * k];
        re[k] = r[k].x + eps * dv.x;
        im[k] = r[k].y + eps * dv.y;
        rp[tid + 256 * k] = make_float2(re[k], im[k]);
    }
    norm_plane(re, red, a.x + (size_t)nb * 2 * PIX, a.stat + (size_t)nb * 4);
    norm_plane(im, red, a.x + (size_t)nb * 2 * PIX + PIX, a.stat + (size_t)nb * 4 + 2);
}

// ---- finish: 1 x 1 convolution + bias, unnorm, residual; divergence; z update; NMSE ----------------------------------------------
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

__device__ __forceinline__ float2 denoised(const FinishArgs& a, int n, int e, const float* w_s) {
    const float* u = a.u2 + (size_t)n * 16 * PIX + e;
    float o0 = 0.f, o1 = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float v = u[k * PIX];
        o0 = fmaf(v, w_s[k], o0);
        o1 = fmaf(v, w_s[16 + k], o1);
    }
    o0 += w_s[32];
    o1 += w_s[33];
    const float* st = a.stat + (size_t)n * 4;
    const float2 rv = reinterpret_cast<const float2*>(a.r)[(size_t)n * PIX + e];
    return make_float2(rv.x - (o0 * st[1] + st[0]), rv.y - (o1 * st[3] + st[2]));
}

__global__ __launch_bounds__(256) void ldamp_finish_kernel(FinishArgs a) {
    __shared__ float2 h_s[PIX];
    __shared__ float w_s[34];
    __shared__ float red[4];
    __shared__ double dred[8];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (tid < 32) w_s[tid] = a.w[tid];
    if (tid < 2) w_s[32 + tid] = a.bias[tid];
    __syncthreads();
    float2 hc[4];
    float2* ho = reinterpret_cast<float2*>(a.h_out) + (size_t)b * PIX;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = tid + 256 * k;
        hc[k] = denoised(a, b, e, w_s);
        ho[e] = hc[k];
        h_s[e] = hc[k];
    }
    if (!a.damp) return;
    if (a.h_log) {
        float2* hl = reinterpret_cast<float2*>(a.h_log) + (size_t)b * PIX;
#pragma unroll
        for (int k = 0; k < 4; ++k) hl[tid + 256 * k] = hc[k];
    }
    const float2* d = reinterpret_cast<const float2*>(a.dirs) + (size_t)b * PIX;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = tid + 256 * k;
        const float2 hp = denoised(a, a.B + b, e, w_s), dv = d[e];
        s += dv.x * (hp.x - hc[k].x);
        s += dv.y * (hp.y - hc[k].y);
    }
    const float mean = block_reduce256<false>(s, red) * (1.f / (2 * PIX));    // (also orders h_s before the reads below)
    const float div = (1.f / a.eps[b]) * mean;
    if (a.div_log && tid == 0) a.div_log[b] = div;
    // z = (Y - P h) + z div
    const int Np = a.Np;
    const float2* P = reinterpret_cast<const float2*>(a.P) + (size_t)b * Np * NT;
    const float2* Y = reinterpret_cast<const float2*>(a.Y) + (size_t)b * Np * NR;
    float2* z = reinterpret_cast<float2*>(a.z) + (size_t)b * Np * NR;
    float2* zl = a.z_log ? reinterpret_cast<float2*>(a.z_log) + (size_t)b * Np * NR : nullptr;
    for (int e = tid; e < Np * NR; e += 256) {
        const int p = e / NR, q = e % NR;
        float sr = 0.f, si = 0.f;
        for (int t = 0; t < NT; ++t) {
            const float2 pv = P[p * NT + t], hv = h_s[t * NR + q];
            sr += pv.x * hv.x - pv.y * hv.y;
            si += pv.x * hv.y + pv.y * hv.x;
        }
        const float2 yv = Y[e], zv = z[e];
        const float2 zn = make_float2((yv.x - sr) + zv.x * div, (yv.y - si) + zv.y * div);
        z[e] = zn;
        if (zl) zl[e] = zn;
    }
    if (!a.last || !a.nmse || !a.Htrue) return;
    const float2* Ht = reinterpret_cast<const float2*>(a.Htrue) + (size_t)b * PIX;
    double err = 0.0, hn = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float2 t = Ht[tid + 256 * k];
        const float dx = hc[k].x - t.x, dy = hc[k].y - t.y;
        err += (double)dx * dx + (double)dy * dy;
        hn += (double)t.x * t.x + (double)t.y * t.y;
    }
    for (int o = 32; o > 0; o >>= 1) {
        err += __shfl_xor(err, o);
        hn += __shfl_xor(hn, o);
    }
    if ((tid & 63) == 0) { dred[tid >> 6] = err; dred[4 + (tid >> 6)] = hn; }
    __syncthreads();
    if (tid == 0) a.nmse[b] = (float)((((dred[0] + dred[1]) + dred[2]) + dred[3]) / (((dred[4] + dred[5]) + dred[6]) + dred[7]));
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
template <int H, int W, int CA, int CB, int COUT, int CT, int OCT, int PXT, int CC, bool POOL>
void conv3(const float* a, const float* b, const float* w, float* out, float* pool, int N, hipStream_t s) {
    using K = Conv3<H, W, CA, CB, COUT, CT, OCT, PXT, CC, POOL>;
    hipLaunchKernelGGL((conv3_kernel<H, W, CA, CB, COUT, CT, OCT, PXT, CC, POOL>), dim3(COUT / CT, N), dim3(K::THREADS), 0, s, a, b, w, out, pool);
}
template <int HI, int WI, int CIN, int COUT, int CT, int OCT, int CC>
void tconv(const float* src, const float* w, float* out, int N, hipStream_t s) {
    using K = TConv<HI, WI, CIN, COUT, CT, OCT, CC>;
    hipLaunchKernelGGL((tconv_kernel<HI, WI, CIN, COUT, CT, OCT, CC>), dim3(COUT / CT, N), dim3(K::THREADS), 0, s, src, w, out);
}

struct Ws {
    float* base;
    int N;
    float* at(int stage) const { return base + stage_prefix(stage) * N; }
};

// the U-Net of N normalised images: S_X -> S_U2 (17 launches)
void unet(const float* net, const Ws& ws, hipStream_t s) {
    const int N = ws.N;
    auto w = [&](int t) { return net + tensor_prefix(t); };
    //     H   W   CA  CB  COUT CT OCT PXT CC POOL
    conv3<64, 16, 2, 0, 16, 8, 8, 4, 2, false>(ws.at(S_X), nullptr, w(W_D0A), ws.at(S_D0A), nullptr, N, s);
    conv3<64, 16, 16, 0, 16, 8, 8, 4, 8, true>(ws.at(S_D0A), nullptr, w(W_D0B), ws.at(S_D0), ws.at(S_P0), N, s);
    conv3<32, 8, 16, 0, 32, 16, 4, 4, 8, false>(ws.at(S_P0), nullptr, w(W_D1A), ws.at(S_D1A), nullptr, N, s);
    conv3<32, 8, 32, 0, 32, 16, 4, 4, 8, true>(ws.at(S_D1A), nullptr, w(W_D1B), ws.at(S_D1), ws.at(S_P1), N, s);
    conv3<16, 4, 32, 0, 64, 32, 4, 4, 8, false>(ws.at(S_P1), nullptr, w(W_D2A), ws.at(S_D2A), nullptr, N, s);
    conv3<16, 4, 64, 0, 64, 32, 4, 4, 8, true>(ws.at(S_D2A), nullptr, w(W_D2B), ws.at(S_D2), ws.at(S_P2), N, s);
    conv3<8, 2, 64, 0, 128, 32, 4, 2, 8, false>(ws.at(S_P2), nullptr, w(W_BA), ws.at(S_BA), nullptr, N, s);
    conv3<8, 2, 128, 0, 128, 32, 4, 2, 8, false>(ws.at(S_BA), nullptr, w(W_BB), ws.at(S_BB), nullptr, N, s);
    tconv<8, 2, 128, 64, 32, 2, 32>(ws.at(S_BB), w(W_T0), ws.at(S_T0), N, s);
    conv3<16, 4, 64, 64, 64, 32, 4, 4, 8, false>(ws.at(S_T0), ws.at(S_D2), w(W_U0A), ws.at(S_U0A), nullptr, N, s);
    conv3<16, 4, 64, 0, 64, 32, 4, 4, 8, false>(ws.at(S_U0A), nullptr, w(W_U0B), ws.at(S_U0), nullptr, N, s);
    tconv<16, 4, 64, 32, 16, 4, 32>(ws.at(S_U0), w(W_T1), ws.at(S_T1), N, s);
    conv3<32, 8, 32, 32, 32, 16, 4, 4, 8, false>(ws.at(S_T1), ws.at(S_D1), w(W_U1A), ws.at(S_U1A), nullptr, N, s);
    conv3<32, 8, 32, 0, 32, 16, 4, 4, 8, false>(ws.at(S_U1A), nullptr, w(W_U1B), ws.at(S_U1), nullptr, N, s);
    tconv<32, 8, 32, 16, 8, 8, 32>(ws.at(S_U1), w(W_T2), ws.at(S_T2), N, s);
    conv3<64, 16, 16, 16, 16, 8, 8, 4, 8, false>(ws.at(S_T2), ws.at(S_D0), w(W_U2A), ws.at(S_U2A), nullptr, N, s);
    conv3<64, 16, 16, 0, 16, 8, 8, 4, 8, false>(ws.at(S_U2A), nullptr, w(W_U2B), ws.at(S_U2), nullptr, N, s);
}

}  // namespace
}  // namespace sbc

struct sbc_ldamp {
    int n_nets = 0;
    sbc::ParamImage params;                             // [n_nets][NET_FLOATS]
};

extern "C" {

int sbc_ldamp_create(const sbc_tensor_ref* tensors, int32_t n_tensors, int32_t n_nets, sbc_ldamp** out) {
    using namespace sbc;
    SBC_REQUIRE(tensors && out && n_nets >= 1 && n_nets <= 64, "sbc_ldamp_create: need tensors, out and 1 <= n_nets <= 64 (got %d)", n_nets);
    SBC_REQUIRE(n_tensors == n_nets * N_TENSORS, "sbc_ldamp_create: %d nets have %d tensors (got %d)", n_nets, n_nets * N_TENSORS, n_tensors);
    TensorIndex sd;
    const int rc = sd.build_unique("sbc_ldamp_create", "tensor", tensors, n_tensors);
    if (rc) return rc;
    ParamImage params;
    const size_t base = params.take((size_t)n_nets * NET_FLOATS);
    for (int u = 0; u < n_nets; ++u)
        for (int t = 0; t < N_TENSORS; ++t) {
            const float* w = sd.find("update_nets." + std::to_string(u) + "." + TENSORS[t].name, TENSORS[t].numel);
            if (!w) return SBC_ERR_INVALID;
            memcpy(params.host.data() + base + (size_t)u * NET_FLOATS + tensor_prefix(t), w, sizeof(float) * TENSORS[t].numel);
        }
    const int rc_up = params.upload("sbc_ldamp_create");
    if (rc_up) return rc_up;
    sbc_ldamp* h = new sbc_ldamp;
    h->n_nets = n_nets;
    h->params = params;
    *out = h;
    return SBC_OK;
}

void sbc_ldamp_destroy(sbc_ldamp* h) {
    if (!h) return;
    h->params.release();
    delete h;
}

int64_t sbc_ldamp_workspace_floats(int32_t B, int32_t num_unrolls) {
    if (B < 0 || num_unrolls < 0) return -1;
    return 2 * (int64_t)B * sbc::EVAL_FLOATS + sbc::run_extra_floats(B, num_unrolls);
}

int sbc_ldamp_stage(int32_t stage, int32_t n_images, int64_t* offset, int32_t* channels, int32_t* height, int32_t* width) {
    using namespace sbc;
    SBC_REQUIRE(stage >= 0 && stage < N_STAGES && n_images >= 0 && offset && channels && height && width,
                "sbc_ldamp_stage: stage must be in [0, %d) and the outputs non-NULL (got stage %d)", N_STAGES, stage);
    *offset = stage_prefix(stage) * n_images;
    *channels = STAGE_DIM[stage].c;
    *height = STAGE_DIM[stage].h;
    *width = STAGE_DIM[stage].w;
    return SBC_OK;
}

int sbc_ldamp_denoise(sbc_ldamp* h, int32_t net, const float* r, float* out, int32_t B, float* workspace, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(h && r && out && workspace, "sbc_ldamp_denoise: NULL handle, r, out or workspace");
    SBC_REQUIRE(net >= 0 && net < h->n_nets, "sbc_ldamp_denoise: net %d out of range [0, %d)", net, h->n_nets);
    SBC_REQUIRE(B >= 0 && B <= 32768, "sbc_ldamp_denoise: B must be in [0, 32768] (got %d)", B);
    const int rc = h->params.check_device("sbc_ldamp_denoise");
    if (rc) return rc;
    if (B == 0) return SBC_OK;
    hipStream_t s = (hipStream_t)stream;
    const Ws ws{workspace, B};
    const float* wn = h->params.dev + (size_t)net * NET_FLOATS;
    PrepArgs pa{};
    pa.r_in = r; pa.r = ws.at(S_R); pa.x = ws.at(S_X); pa.stat = ws.at(S_STAT); pa.B = B;
    hipLaunchKernelGGL(ldamp_prep_kernel, dim3(B), dim3(256), 0, s, pa);
    unet(wn, ws, s);
    FinishArgs fa{};
    fa.u2 = ws.at(S_U2); fa.r = ws.at(S_R); fa.stat = ws.at(S_STAT); fa.w = wn + tensor_prefix(W_FIN); fa.bias = wn + tensor_prefix(W_FINB);
    fa.h_out = out; fa.B = B;
    hipLaunchKernelGGL(ldamp_finish_kernel, dim3(B), dim3(256), 0, s, fa);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int sbc_ldamp_run(sbc_ldamp* h, const sbc_ldamp_run_desc* d, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(h && d, "sbc_ldamp_run: NULL handle or descriptor");
    SBC_REQUIRE(d->Nt == NT && d->Nr == NR, "sbc_ldamp_run: supported geometry is Nt = %d, Nr = %d (got %d x %d)", NT, NR, d->Nt, d->Nr);
    SBC_REQUIRE(d->Np >= 1 && d->Np <= NT, "sbc_ldamp_run: Np must be in [1, %d] (got %d)", NT, d->Np);
    SBC_REQUIRE(d->B >= 0 && d->B <= 16384, "sbc_ldamp_run: B must be in [0, 16384] (got %d)", d->B);
    SBC_REQUIRE(d->num_unrolls >= 1 && d->num_unrolls <= h->n_nets, "sbc_ldamp_run: num_unrolls must be in [1, %d] (got %d)", h->n_nets, d->num_unrolls);
    const struct { const void* p; const char* name; } need[] = {{d->Y_herm, "Y_herm"}, {d->P_herm, "P_herm"}, {d->eig1, "eig1"}, {d->H_hat, "H_hat"},
                                                                 {d->workspace, "workspace"}};
    for (const auto& q : need) SBC_REQUIRE(q.p, "sbc_ldamp_run: NULL %s", q.name);
    SBC_REQUIRE(!d->nmse || d->Htrue, "sbc_ldamp_run: nmse needs Htrue");
    const int rc = h->params.check_device("sbc_ldamp_run");
    if (rc) return rc;
    if (d->B == 0) return SBC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int B = d->B, Np = d->Np, U = d->num_unrolls;
    const Ws ws{d->workspace, 2 * B};
    float* z = d->workspace + 2 * (int64_t)B * EVAL_FLOATS;
    float* eps = z + (size_t)B * 2 * PIX;
    float* own_dirs = eps + (size_t)B * 16;
    const float* dirs = d->directions;
    if (!dirs) {
        hipLaunchKernelGGL(ldamp_dirs_kernel, dim3(B, U), dim3(256), 0, s, own_dirs, d->seed, d->sample0, 0, B);
        dirs = own_dirs;
    }
    SBC_CHECK_HIP(hipMemcpyAsync(z, d->Y_herm, sizeof(float) * 2 * (size_t)B * Np * NR, hipMemcpyDeviceToDevice, s));
    for (int u = 0; u < U; ++u) {
        const float* wn = h->params.dev + (size_t)u * NET_FLOATS;
        const float* du = dirs + (size_t)u * B * 2 * PIX;
        PrepArgs pa{};
        pa.P = d->P_herm; pa.z = z; pa.h = u ? d->H_hat : nullptr; pa.eig = d->eig1; pa.dirs = du; pa.eps = eps;
        pa.eps_log = d->eps_log ? d->eps_log + (size_t)u * B : nullptr;
        pa.r = ws.at(S_R); pa.x = ws.at(S_X); pa.stat = ws.at(S_STAT); pa.B = B; pa.Np = Np;
        hipLaunchKernelGGL(ldamp_prep_kernel, dim3(B), dim3(256), 0, s, pa);
        unet(wn, ws, s);
        FinishArgs fa{};
        fa.u2 = ws.at(S_U2); fa.r = ws.at(S_R); fa.stat = ws.at(S_STAT); fa.w = wn + tensor_prefix(W_FIN); fa.bias = wn + tensor_prefix(W_FINB);
        fa.h_out = d->H_hat; fa.damp = 1; fa.P = d->P_herm; fa.Y = d->Y_herm; fa.z = z; fa.eps = eps; fa.dirs = du;
        fa.Htrue = d->Htrue; fa.nmse = d->nmse;
        fa.h_log = d->h_log ? d->h_log + (size_t)u * B * 2 * PIX : nullptr;
        fa.z_log = d->z_log ? d->z_log + (size_t)u * B * 2 * Np * NR : nullptr;
        fa.div_log = d->div_log ? d->div_log + (size_t)u * B : nullptr;
        fa.B = B; fa.Np = Np; fa.last = u == U - 1;
        hipLaunchKernelGGL(ldamp_finish_kernel, dim3(B), dim3(256), 0, s, fa);
    }
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int sbc_debug_ldamp_directions(uint64_t seed, int64_t sample, int32_t unroll, float* out) {
    using namespace sbc;
    SBC_REQUIRE(out && unroll >= 0, "sbc_debug_ldamp_directions: need out and unroll >= 0");
    float* dev = nullptr;
    SBC_CHECK_HIP(hipMalloc(&dev, sizeof(float) * 2 * PIX));
    hipLaunchKernelGGL(ldamp_dirs_kernel, dim3(1, 1), dim3(256), 0, nullptr, dev, seed, sample, unroll, 1);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, dev, sizeof(float) * 2 * PIX, hipMemcpyDeviceToHost);
    (void)hipFree(dev);
    SBC_CHECK_HIP(e);
    return SBC_OK;
}

}  // extern "C"
