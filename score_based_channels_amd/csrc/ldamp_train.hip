// Training of Learned D-AMP: src/score_based_channels/train_ldamp.py:107-141 -- the unrolled forward of aux_models.py:62-190 with the
// activations of every unroll kept, loss = mean_b sum |h - H|^2, its gradient with respect to every tensor of the num_unrolls denoisers
// and one Adam step (torch.optim.Adam defaults).  The forward runs the launches of ldamp.hip (ldamp_shared.h): the training twins of the
// convolution stages differ from the inference kernels in one store, the rstd of the InstanceNorm, so h, z, div and eps are the bits of
// sbc_ldamp_run.
//
// What is differentiated: the clean evaluation only.  div and eps are constants (the reference computes them under no_grad,
// aux_models.py:148-171), so the perturbed evaluation has no backward.  Per unroll u, from the last to the first, with gh = dL/dh_u and
// gz' = dL/dz_{u+1} (complex numbers stand for (d/dRe, d/dIm)):
//     finish backward   gh -= P^H gz';  h = r - (c std + mean), c = conv1x1(u2) + bias:  dr = gh, dc = -gh std, dmean = -sum gh,
//                       dstd = -sum gh c, du2 = W^T dc, dW = sum dc u2, dbias = sum dc
//     17 stages         LeakyReLU mask and InstanceNorm backward (ldamp_inorm_bwd_kernel: the sign and the normalised value come from the
//                       stored activation, slope 0.2 > 0; a pooled stage first adds 1/4 of its pool's gradient to its own), then the input
//                       gradient (the concat splits into its two sources) and the weight gradient
//     norm + loop       x = (r - mean) / std (unbiased std, no eps) back to r;  r = h_{u-1} + P^H z_u / eig:  gh_{u-1} = dr,
//                       gz_u = div_u gz' + P dr / eig
//
// Arithmetic: exact fp32 (v_fma_f32), fixed summation orders, no atomics.  Stage gradients of a sample are computed by workgroups that
// see that sample only; parameter gradients sum over (sample, pixel) in index order per lane, then by the wavefront butterfly.
// Launches per step: forward 19 per unroll (+ 1 directions, + 1 copy), loss 2, backward 54 per unroll (finish backward + its reduction,
// 17 x (norm backward, input gradient, weight gradient), norm + loop backward), Adam 1.
#include "ldamp_shared.h"

namespace sbc {
namespace {

constexpr int FIN_PART = 34;                             // 2 x 16 weights + 2 biases of the 1 x 1 convolution
constexpr int64_t GPRE_FLOATS = 16 * PIX;                // the largest stage of an image

// ---- workspace of a step ---------------------------------------------------------------------------------------------------------------
struct TrainLayout {
    int64_t fwd, rstd, grad, gh, gz, gpre, div, eps, z, hhat, err, part, dirs, total;
    TrainLayout(int B, int U, bool own_dirs) {
        int64_t o = 0;
        auto take = [&](int64_t n) { const int64_t at = o; o += (n + 3) & ~(int64_t)3; return at; };
        fwd = take((int64_t)U * 2 * B * EVAL_FLOATS);    // [U] evaluations of 2B images (clean b, perturbed B + b), stages as sbc_ldamp_stage
        rstd = take((int64_t)U * 2 * B * RSTD_FLOATS);   // [U] rstd of the 17 norms, [2B][C] each
        grad = take((int64_t)U * B * EVAL_FLOATS);       // [U] gradients of the clean stages, B images
        gh = take((int64_t)U * B * 2 * PIX);             // [U] dL/dh_u as it arrives (loss, or dr of unroll u + 1)
        gz = take((int64_t)(U + 1) * B * 2 * PIX);       // [U + 1] dL/dz_u, z_u entering unroll u; slot U is never written (zero gradient)
        gpre = take((int64_t)B * GPRE_FLOATS);           // gradient in front of the norm of the stage at work
        div = take((int64_t)U * B);
        eps = take((int64_t)B * 16);
        z = take((int64_t)B * 2 * PIX);
        hhat = take((int64_t)B * 2 * PIX);
        err = take((int64_t)B * 2);
        part = take((int64_t)B * FIN_PART);
        dirs = take(own_dirs ? (int64_t)U * B * 2 * PIX : 0);
        total = o;
    }
};

// ---- loss ------------------------------------------------------------------------------------------------------------------------------
// gh = (2 / B) (h - H);  err[b] = (sum |h - H|^2, sum |H|^2), summed in double as the NMSE of ldamp_finish_kernel
__global__ __launch_bounds__(256) void ldamp_loss_kernel(const float* __restrict__ h, const float* __restrict__ Ht, float* __restrict__ gh,
                                                         float* __restrict__ err, int B) {
    __shared__ double dred[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float2* hv = reinterpret_cast<const float2*>(h) + (size_t)b * PIX;
    const float2* tv = reinterpret_cast<const float2*>(Ht) + (size_t)b * PIX;
    float2* g = reinterpret_cast<float2*>(gh) + (size_t)b * PIX;
    const float sc = 2.f / (float)B;
    double e = 0.0, hn = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float2 a = hv[tid + 256 * k], t = tv[tid + 256 * k];
        const float dx = a.x - t.x, dy = a.y - t.y;
        g[tid + 256 * k] = make_float2(sc * dx, sc * dy);
        e += (double)dx * dx + (double)dy * dy;
        hn += (double)t.x * t.x + (double)t.y * t.y;
    }
    e = block_sum256(e, dred);
    hn = block_sum256(hn, dred);
    if (tid == 0) { err[2 * b] = (float)e; err[2 * b + 1] = (float)hn; }
}

// out[0] = mean_b err_b, out[1] = mean_b err_b / |H_b|^2, samples in index order
__global__ __launch_bounds__(64) void ldamp_loss_reduce_kernel(const float* __restrict__ err, float* __restrict__ out, int B) {
    if (threadIdx.x != 0) return;
    double l = 0.0, n = 0.0;
    for (int b = 0; b < B; ++b) { l += (double)err[2 * b]; n += (double)err[2 * b] / (double)err[2 * b + 1]; }
    out[0] = (float)(l / B);
    out[1] = (float)(n / B);
}

// ---- finish backward -------------------------------------------------------------------------------------------------------------------
struct FinBwdArgs {
    const float* u2;       // S_U2 of the unroll, clean images first
    const float* stat;     // S_STAT
    const float* w;        // [2][16]
    const float* bias;     // [2]
    const float* gh;       // [B][64][16][2]
    const float* gz_next;  // [B][Np][16][2] or NULL (last unroll)
    const float* P;        // [B][Np][64]
    float* g_r;            // gradient of S_R: here the direct path dr = gh - P^H gz'
    float* g_u2;           // gradient of S_U2
    float* g_stat;         // gradient of S_STAT
    float* part;           // [B][34] this sample's share of dW, dbias
    int Np;
};

__global__ __launch_bounds__(256) void ldamp_finish_bwd_kernel(FinBwdArgs a) {
    __shared__ float2 P_s[NT * NT];
    __shared__ float2 gz_s[NT * NR];
    __shared__ float w_s[34];
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.x, Np = a.Np;
    if (tid < 32) w_s[tid] = a.w[tid];
    if (tid < 2) w_s[32 + tid] = a.bias[tid];
    if (a.gz_next) {
        const float2* P = reinterpret_cast<const float2*>(a.P) + (size_t)b * Np * NT;
        const float2* gz = reinterpret_cast<const float2*>(a.gz_next) + (size_t)b * Np * NR;
        for (int e = tid; e < Np * NT; e += 256) P_s[e] = P[e];
        for (int e = tid; e < Np * NR; e += 256) gz_s[e] = gz[e];
    }
    __syncthreads();
    const float* st = a.stat + (size_t)b * 4;
    const float sd0 = st[1], sd1 = st[3];
    float pw[32], pb0 = 0.f, pb1 = 0.f, dm0 = 0.f, dm1 = 0.f, ds0 = 0.f, ds1 = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) pw[k] = 0.f;
    const float2* gh = reinterpret_cast<const float2*>(a.gh) + (size_t)b * PIX;
    float2* gr = reinterpret_cast<float2*>(a.g_r) + (size_t)b * PIX;
#pragma unroll 1
    for (int k4 = 0; k4 < 4; ++k4) {
        const int e = tid + 256 * k4, t = e / NR, q = e % NR;
        float2 g = gh[e];
        if (a.gz_next) {
            float sr = 0.f, si = 0.f;
            for (int p = 0; p < Np; ++p) {                         // conj(P[p][t]) gz[p][q]
                const float2 pv = P_s[p * NT + t], zv = gz_s[p * NR + q];
                sr += pv.x * zv.x + pv.y * zv.y;
                si += pv.x * zv.y - pv.y * zv.x;
            }
            g.x -= sr;
            g.y -= si;
        }
        gr[e] = g;
        const float* u = a.u2 + (size_t)b * 16 * PIX + e;
        float uv[16], c0 = 0.f, c1 = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            uv[k] = u[k * PIX];
            c0 = fmaf(uv[k], w_s[k], c0);
            c1 = fmaf(uv[k], w_s[16 + k], c1);
        }
        c0 += w_s[32];
        c1 += w_s[33];
        const float dc0 = -g.x * sd0, dc1 = -g.y * sd1;
        dm0 -= g.x; dm1 -= g.y;
        ds0 -= g.x * c0; ds1 -= g.y * c1;
        pb0 += dc0; pb1 += dc1;
        float* gu = a.g_u2 + (size_t)b * 16 * PIX + e;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            gu[k * PIX] = dc0 * w_s[k] + dc1 * w_s[16 + k];
            pw[k] = fmaf(dc0, uv[k], pw[k]);
            pw[16 + k] = fmaf(dc1, uv[k], pw[16 + k]);
        }
    }
    float* gs = a.g_stat + (size_t)b * 4;
    float* part = a.part + (size_t)b * FIN_PART;
    float v;
    v = block_reduce256<false>(dm0, red); if (tid == 0) gs[0] = v;
    v = block_reduce256<false>(ds0, red); if (tid == 0) gs[1] = v;
    v = block_reduce256<false>(dm1, red); if (tid == 0) gs[2] = v;
    v = block_reduce256<false>(ds1, red); if (tid == 0) gs[3] = v;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        v = block_reduce256<false>(pw[k], red);
        if (tid == 0) part[k] = v;
    }
    v = block_reduce256<false>(pb0, red); if (tid == 0) part[32] = v;
    v = block_reduce256<false>(pb1, red); if (tid == 0) part[33] = v;
}

// dW, dbias of the 1 x 1 convolution: the samples' shares in sample order (the two tensors are adjacent in a net's block)
__global__ __launch_bounds__(64) void ldamp_finish_wgrad_kernel(const float* __restrict__ part, float* __restrict__ gw, int B) {
    const int j = threadIdx.x;
    if (j >= FIN_PART) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += part[(size_t)b * FIN_PART + j];
    gw[j] = s;
}

// ---- LeakyReLU + InstanceNorm backward ---------------------------------------------------------------------------------------------------
// grid (C, B), one wavefront per plane.  g: dL/dy of the stored activation y; with gpool, 1/4 of the pool's gradient is added first and the
// sum stored back (the stage's whole gradient stays readable).  gpre = rstd (gx - mean(gx) - xhat mean(gx xhat)), gx = g * (y >= 0 ? 1 : 0.2),
// xhat = y >= 0 ? y : y / 0.2.
__global__ __launch_bounds__(64) void ldamp_inorm_bwd_kernel(const float* __restrict__ y, float* __restrict__ g, const float* __restrict__ gpool,
                                                             const float* __restrict__ rstd, float* __restrict__ gpre, int C, int H, int W) {
    const int lane = threadIdx.x, c = blockIdx.x, n = blockIdx.y, HW = H * W;
    const size_t base = ((size_t)n * C + c) * HW;
    const float* gp = gpool ? gpool + ((size_t)n * C + c) * (HW / 4) : nullptr;
    float s1 = 0.f, s2 = 0.f;
    SBC_NO_VEC for (int i = lane; i < HW; i += 64) {
        float gv = g[base + i];
        if (gp) {
            gv += 0.25f * gp[((i / W) >> 1) * (W >> 1) + ((i % W) >> 1)];
            g[base + i] = gv;
        }
        const float yv = y[base + i];
        const bool pos = yv >= 0.f;
        const float gx = pos ? gv : LRELU * gv, xh = pos ? yv : yv / LRELU;
        s1 += gx;
        s2 += gx * xh;
        gpre[base + i] = gx;
    }
    const float m1 = wave_sum(s1) * (1.f / HW), m2 = wave_sum(s2) * (1.f / HW), r = rstd[(size_t)n * C + c];
    SBC_NO_VEC for (int i = lane; i < HW; i += 64) {
        const float yv = y[base + i], xh = yv >= 0.f ? yv : yv / LRELU;
        gpre[base + i] = r * ((gpre[base + i] - m1) - xh * m2);
    }
}

// ---- 3 x 3 convolution: input gradient --------------------------------------------------------------------------------------------------
// gin[n][ci][y][x] = sum_oc sum_k gpre[n][oc][y + 1 - ky][x + 1 - kx] w[oc][ci][ky][kx]; channels [0, CA) go to gA, the rest to gB.
// grid (ceil(CIN H W / 256), B): a thread per input element, output channels in index order.
__global__ __launch_bounds__(256) void ldamp_conv3_dgrad_kernel(const float* __restrict__ gpre, const float* __restrict__ wgt, float* __restrict__ gA,
                                                               float* __restrict__ gB, int CA, int CB, int COUT, int H, int W) {
    const int HW = H * W, CIN = CA + CB, n = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= CIN * HW) return;
    const int ci = idx / HW, pix = idx % HW, y = pix / W, x = pix % W;
    const float* g = gpre + (size_t)n * COUT * HW;
    float acc = 0.f;
    for (int oc = 0; oc < COUT; ++oc) {
        const float* w9 = wgt + ((size_t)oc * CIN + ci) * 9;
        const float* go = g + (size_t)oc * HW;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = y + 1 - ky;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = x + 1 - kx;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) acc = fmaf(go[yy * W + xx], w9[ky * 3 + kx], acc);
            }
        }
    }
    if (ci < CA) gA[((size_t)n * CA + ci) * HW + pix] = acc;
    else gB[((size_t)n * CB + (ci - CA)) * HW + pix] = acc;
}

// ---- 3 x 3 convolution: weight gradient -------------------------------------------------------------------------------------------------
// dW[oc][ci][ky][kx] = sum_n sum_pix gpre[n][oc][pix] in[n][ci][y + ky - 1][x + kx - 1].  grid (CIN, COUT), one wavefront per filter plane:
// lane l sums the (sample, pixel) pairs l, l + 64, ... in that order, then the butterfly.
__global__ __launch_bounds__(64) void ldamp_conv3_wgrad_kernel(const float* __restrict__ gpre, const float* __restrict__ srcA,
                                                              const float* __restrict__ srcB, float* __restrict__ gw, int CA, int CB, int COUT,
                                                              int H, int W, int B) {
    const int HW = H * W, CIN = CA + CB, ci = blockIdx.x, oc = blockIdx.y, lane = threadIdx.x;
    const float* src = ci < CA ? srcA + (size_t)ci * HW : srcB + (size_t)(ci - CA) * HW;
    const size_t sstride = (size_t)(ci < CA ? CA : CB) * HW;
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.f;
    for (int e = lane; e < B * HW; e += 64) {
        const int n = e / HW, pix = e % HW, y = pix / W, x = pix % W;
        const float gv = gpre[((size_t)n * COUT + oc) * HW + pix];
        const float* in = src + (size_t)n * sstride;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = y + ky - 1;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = x + kx - 1;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) acc[ky * 3 + kx] = fmaf(gv, in[yy * W + xx], acc[ky * 3 + kx]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float s = wave_sum(acc[k]);
        if (lane == 0) gw[((size_t)oc * CIN + ci) * 9 + k] = s;
    }
}

// ---- transposed convolution 2 x 2 stride 2: input and weight gradient ---------------------------------------------------------------------
// gin[n][ci][y][x] = sum_oc sum_d gpre[n][oc][2y + dy][2x + dx] w[ci][oc][dy][dx].  grid (ceil(CIN HI WI / 256), B)
__global__ __launch_bounds__(256) void ldamp_tconv_dgrad_kernel(const float* __restrict__ gpre, const float* __restrict__ wgt, float* __restrict__ gin,
                                                               int CIN, int COUT, int HI, int WI) {
    const int HWI = HI * WI, WO = 2 * WI, HWO = 4 * HWI, n = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= CIN * HWI) return;
    const int ci = idx / HWI, pix = idx % HWI, y = pix / WI, x = pix % WI;
    float acc = 0.f;
    for (int oc = 0; oc < COUT; ++oc) {
        const float* go = gpre + ((size_t)n * COUT + oc) * HWO + (2 * y) * WO + 2 * x;
        const float* w4 = wgt + ((size_t)ci * COUT + oc) * 4;
        acc = fmaf(go[0], w4[0], acc);
        acc = fmaf(go[1], w4[1], acc);
        acc = fmaf(go[WO], w4[2], acc);
        acc = fmaf(go[WO + 1], w4[3], acc);
    }
    gin[((size_t)n * CIN + ci) * HWI + pix] = acc;
}

// dW[ci][oc][dy][dx] = sum_n sum_pix in[n][ci][y][x] gpre[n][oc][2y + dy][2x + dx].  grid (COUT, CIN), one wavefront per 2 x 2 filter
__global__ __launch_bounds__(64) void ldamp_tconv_wgrad_kernel(const float* __restrict__ gpre, const float* __restrict__ src, float* __restrict__ gw,
                                                              int CIN, int COUT, int HI, int WI, int B) {
    const int HWI = HI * WI, WO = 2 * WI, HWO = 4 * HWI, oc = blockIdx.x, ci = blockIdx.y, lane = threadIdx.x;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int e = lane; e < B * HWI; e += 64) {
        const int n = e / HWI, pix = e % HWI, y = pix / WI, x = pix % WI;
        const float v = src[((size_t)n * CIN + ci) * HWI + pix];
        const float* go = gpre + ((size_t)n * COUT + oc) * HWO + (2 * y) * WO + 2 * x;
        acc[0] = fmaf(v, go[0], acc[0]);
        acc[1] = fmaf(v, go[1], acc[1]);
        acc[2] = fmaf(v, go[WO], acc[2]);
        acc[3] = fmaf(v, go[WO + 1], acc[3]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float s = wave_sum(acc[k]);
        if (lane == 0) gw[((size_t)ci * COUT + oc) * 4 + k] = s;
    }
}

// ---- norm and loop algebra backward ------------------------------------------------------------------------------------------------------
struct PrepBwdArgs {
    const float* r;        // S_R of the unroll
    const float* stat;     // S_STAT
    const float* g_x;      // gradient of S_X [B][2][1024]
    const float* g_stat;   // gradient of S_STAT from the finish
    float* g_r;            // in: the direct path; out: dL/dr
    const float* P;        // [B][Np][64]
    const float* eig;      // [B]
    const float* div;      // [B] of this unroll
    const float* gz_next;  // dL/dz_{u+1} or NULL
    float* gz;             // dL/dz_u
    float* gh_prev;        // dL/dh_{u-1} or NULL (first unroll)
    int Np;
};

__global__ __launch_bounds__(256) void ldamp_prep_bwd_kernel(PrepBwdArgs a) {
    __shared__ float2 dr_s[PIX];
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.x, Np = a.Np;
    const float2* r = reinterpret_cast<const float2*>(a.r) + (size_t)b * PIX;
    float2* gr = reinterpret_cast<float2*>(a.g_r) + (size_t)b * PIX;
    const float* st = a.stat + (size_t)b * 4;
    const float* gs = a.g_stat + (size_t)b * 4;
    float out[2][4];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        const float mean = st[2 * pl], sd = st[2 * pl + 1];
        const float* gx = a.g_x + ((size_t)b * 2 + pl) * PIX;
        float dx[4], d[4], a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float2 rv = r[tid + 256 * k];
            dx[k] = gx[tid + 256 * k];
            d[k] = (pl ? rv.y : rv.x) - mean;
            a1 += dx[k];
            a2 += dx[k] * d[k];
        }
        const float S1 = block_reduce256<false>(a1, red) / sd, S2 = block_reduce256<false>(a2, red) / (sd * sd);
        const float dm = (gs[2 * pl] - S1) * (1.f / PIX), dsd = (gs[2 * pl + 1] - S2) / ((PIX - 1) * sd);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[pl][k] = dx[k] / sd + dm + d[k] * dsd;
    }
    float2* ghp = a.gh_prev ? reinterpret_cast<float2*>(a.gh_prev) + (size_t)b * PIX : nullptr;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = tid + 256 * k;
        const float2 g0 = gr[e];
        const float2 g = make_float2(g0.x + out[0][k], g0.y + out[1][k]);
        gr[e] = g;
        dr_s[e] = g;
        if (ghp) ghp[e] = g;
    }
    __syncthreads();
    // gz_u = div gz' + (1 / eig) P dr
    const float2* P = reinterpret_cast<const float2*>(a.P) + (size_t)b * Np * NT;
    const float2* gzn = a.gz_next ? reinterpret_cast<const float2*>(a.gz_next) + (size_t)b * Np * NR : nullptr;
    float2* gz = reinterpret_cast<float2*>(a.gz) + (size_t)b * Np * NR;
    const float inv = 1.f / a.eig[b], div = a.div[b];
    for (int e = tid; e < Np * NR; e += 256) {
        const int p = e / NR, q = e % NR;
        float sr = 0.f, si = 0.f;
        for (int t = 0; t < NT; ++t) {
            const float2 pv = P[p * NT + t], dv = dr_s[t * NR + q];
            sr += pv.x * dv.x - pv.y * dv.y;
            si += pv.x * dv.y + pv.y * dv.x;
        }
        float2 o = make_float2(inv * sr, inv * si);
        if (gzn) { const float2 zn = gzn[e]; o.x += div * zn.x; o.y += div * zn.y; }
        gz[e] = o;
    }
}

// ---- Adam (torch.optim.Adam defaults: betas 0.9 / 0.999, eps 1e-8, no weight decay), one launch over the block of the nets used --------------
//   exp_avg = b1 exp_avg + (1 - b1) g;  exp_avg_sq = b2 exp_avg_sq + (1 - b2) g^2
//   p -= (lr / (1 - b1^t)) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - b2^t) + eps)
// The bias corrections are evaluated in double on the host, as torch computes them as python floats.
__global__ __launch_bounds__(256) void ldamp_adam_kernel(const float* __restrict__ g, float* __restrict__ p, float* __restrict__ m_, float* __restrict__ v_,
                                                         int64_t n, float step_size, float bc2s) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float w1 = (float)(1.0 - 0.9), b2 = 0.999f, w2 = (float)(1.0 - 0.999), eps = 1e-8f;
    const float gv = g[i];
    float m = m_[i], v = v_[i];
    m = m + (gv - m) * w1;                                   // exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + w2 * (gv * gv);                             // mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    m_[i] = m;
    v_[i] = v;
    p[i] = p[i] - step_size * (m / (sqrtf(v) / bc2s + eps));
}

// ---- the backward of one U-Net ---------------------------------------------------------------------------------------------------------
struct Bwd {
    const float* net;      // this net's weights
    float* gnet;           // this net's gradients
    Ws f;                  // forward stages (2B images, the clean ones first)
    Ws g;                  // stage gradients (B images)
    const float* rstd;     // [stage][2B][C]
    float* gpre;
    int B;
    hipStream_t s;

    const float* R(int st) const { return rstd + rstd_prefix(st) * f.N; }
    void inorm(int st, int pool_st) const {
        const StageDim d = STAGE_DIM[st];
        hipLaunchKernelGGL(ldamp_inorm_bwd_kernel, dim3(d.c, B), dim3(64), 0, s, f.at(st), g.at(st), pool_st >= 0 ? g.at(pool_st) : nullptr, R(st), gpre,
                           d.c, d.h, d.w);
    }
    // stage `out` = conv3(concat(inA, inB)) with tensor t; pool_st: the pool of `out` (its gradient is added first) or -1
    void conv(int out, int inA, int inB, int t, int pool_st = -1) const {
        const StageDim d = STAGE_DIM[out];
        const int CA = STAGE_DIM[inA].c, CB = inB >= 0 ? STAGE_DIM[inB].c : 0, cin = CA + CB;
        inorm(out, pool_st);
        hipLaunchKernelGGL(ldamp_conv3_dgrad_kernel, dim3((cin * d.h * d.w + 255) / 256, B), dim3(256), 0, s, gpre, net + tensor_prefix(t), g.at(inA),
                           inB >= 0 ? g.at(inB) : nullptr, CA, CB, d.c, d.h, d.w);
        hipLaunchKernelGGL(ldamp_conv3_wgrad_kernel, dim3(cin, d.c), dim3(64), 0, s, gpre, f.at(inA), inB >= 0 ? f.at(inB) : nullptr,
                           gnet + tensor_prefix(t), CA, CB, d.c, d.h, d.w, B);
    }
    void tconv(int out, int in, int t) const {
        const StageDim d = STAGE_DIM[out], di = STAGE_DIM[in];
        inorm(out, -1);
        hipLaunchKernelGGL(ldamp_tconv_dgrad_kernel, dim3((di.c * di.h * di.w + 255) / 256, B), dim3(256), 0, s, gpre, net + tensor_prefix(t), g.at(in),
                           di.c, d.c, di.h, di.w);
        hipLaunchKernelGGL(ldamp_tconv_wgrad_kernel, dim3(d.c, di.c), dim3(64), 0, s, gpre, f.at(in), gnet + tensor_prefix(t), di.c, d.c, di.h, di.w, B);
    }
    // S_U2's gradient -> S_X's gradient and the 17 tensors' gradients (51 launches).  The skip stages d0, d1, d2 receive their share of the
    // concat from the up path first and the pool's share when their own stage is differentiated.
    void unet() const {
        conv(S_U2, S_U2A, -1, W_U2B);
        conv(S_U2A, S_T2, S_D0, W_U2A);
        tconv(S_T2, S_U1, W_T2);
        conv(S_U1, S_U1A, -1, W_U1B);
        conv(S_U1A, S_T1, S_D1, W_U1A);
        tconv(S_T1, S_U0, W_T1);
        conv(S_U0, S_U0A, -1, W_U0B);
        conv(S_U0A, S_T0, S_D2, W_U0A);
        tconv(S_T0, S_BB, W_T0);
        conv(S_BB, S_BA, -1, W_BB);
        conv(S_BA, S_P2, -1, W_BA);
        conv(S_D2, S_D2A, -1, W_D2B, S_P2);
        conv(S_D2A, S_P1, -1, W_D2A);
        conv(S_D1, S_D1A, -1, W_D1B, S_P1);
        conv(S_D1A, S_P0, -1, W_D1A);
        conv(S_D0, S_D0A, -1, W_D0B, S_P0);
        conv(S_D0A, S_X, -1, W_D0A);
    }
};

}  // namespace
}  // namespace sbc

struct sbc_ldamp_trainer {
    int n_nets = 0, device = 0;
    int64_t step = 0;                                    // Adam steps taken
    float* params = nullptr;                             // [n_nets][NET_FLOATS]; behind it grads, exp_avg, exp_avg_sq of the same shape
    int64_t n() const { return (int64_t)n_nets * sbc::NET_FLOATS; }
    float* grads() const { return params + n(); }
    float* m() const { return params + 2 * n(); }
    float* v() const { return params + 3 * n(); }
};

namespace sbc {
namespace {
int trainer_device(const sbc_ldamp_trainer* h, const char* who) {
    int cur = 0;
    SBC_CHECK_HIP(hipGetDevice(&cur));
    SBC_REQUIRE(cur == h->device, "%s: the handle lives on device %d, the current device is %d", who, h->device, cur);
    return SBC_OK;
}
}  // namespace
}  // namespace sbc

extern "C" {

int sbc_ldamp_trainer_create(const sbc_tensor_ref* tensors, int32_t n_tensors, int32_t n_nets, sbc_ldamp_trainer** out) {
    using namespace sbc;
    SBC_REQUIRE(tensors && out && n_nets >= 1 && n_nets <= 64, "sbc_ldamp_trainer_create: need tensors, out and 1 <= n_nets <= 64 (got %d)", n_nets);
    SBC_REQUIRE(n_tensors == n_nets * N_TENSORS, "sbc_ldamp_trainer_create: %d nets have %d tensors (got %d)", n_nets, n_nets * N_TENSORS, n_tensors);
    TensorIndex sd;
    const int rc = sd.build_unique("sbc_ldamp_trainer_create", "tensor", tensors, n_tensors);
    if (rc) return rc;
    std::vector<float> host((size_t)n_nets * NET_FLOATS);
    for (int u = 0; u < n_nets; ++u)
        for (int t = 0; t < N_TENSORS; ++t) {
            const float* w = sd.find("update_nets." + std::to_string(u) + "." + TENSORS[t].name, TENSORS[t].numel);
            if (!w) return SBC_ERR_INVALID;
            memcpy(host.data() + (size_t)u * NET_FLOATS + tensor_prefix(t), w, sizeof(float) * TENSORS[t].numel);
        }
    sbc_ldamp_trainer* h = new sbc_ldamp_trainer;
    h->n_nets = n_nets;
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = hipMalloc(&h->params, sizeof(float) * 4 * h->n());
    if (e == hipSuccess) e = hipMemset(h->params, 0, sizeof(float) * 4 * h->n());
    if (e == hipSuccess) e = hipMemcpy(h->params, host.data(), sizeof(float) * h->n(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("sbc_ldamp_trainer_create: allocation or upload of the parameters failed: %s", hipGetErrorString(e));
        if (h->params) (void)hipFree(h->params);
        delete h;
        return SBC_ERR_HIP;
    }
    *out = h;
    return SBC_OK;
}

void sbc_ldamp_trainer_destroy(sbc_ldamp_trainer* h) {
    if (!h) return;
    if (h->params) (void)hipFree(h->params);
    delete h;
}

int64_t sbc_ldamp_trainer_workspace_floats(int32_t B, int32_t num_unrolls, int32_t own_directions) {
    if (B < 0 || num_unrolls < 0 || B > 128 || num_unrolls > 64) return -1;
    return sbc::TrainLayout(B, num_unrolls, own_directions != 0).total;
}

int sbc_ldamp_trainer_stage(int32_t kind, int32_t stage, int32_t unroll, int32_t B, int32_t num_unrolls, int64_t* offset, int32_t* n_images,
                            int32_t* channels, int32_t* height, int32_t* width) {
    using namespace sbc;
    SBC_REQUIRE(offset && n_images && channels && height && width, "sbc_ldamp_trainer_stage: NULL output");
    SBC_REQUIRE(B >= 0 && B <= 128 && num_unrolls >= 1 && num_unrolls <= 64, "sbc_ldamp_trainer_stage: B must be in [0, 128] and num_unrolls in [1, 64]");
    SBC_REQUIRE(unroll >= 0 && unroll < num_unrolls, "sbc_ldamp_trainer_stage: unroll %d out of range [0, %d)", unroll, num_unrolls);
    const TrainLayout L(B, num_unrolls, false);
    switch (kind) {
    case SBC_LDAMP_TRAIN_FORWARD:
    case SBC_LDAMP_TRAIN_GRAD: {
        SBC_REQUIRE(stage >= 0 && stage < N_STAGES, "sbc_ldamp_trainer_stage: stage must be in [0, %d) (got %d)", N_STAGES, stage);
        const int N = kind == SBC_LDAMP_TRAIN_FORWARD ? 2 * B : B;
        *offset = (kind == SBC_LDAMP_TRAIN_FORWARD ? L.fwd : L.grad) + (int64_t)unroll * N * EVAL_FLOATS + stage_prefix(stage) * N;
        *n_images = N; *channels = STAGE_DIM[stage].c; *height = STAGE_DIM[stage].h; *width = STAGE_DIM[stage].w;
        return SBC_OK;
    }
    case SBC_LDAMP_TRAIN_RSTD:
        SBC_REQUIRE(stage >= 0 && stage < N_STAGES && stage_normed(stage), "sbc_ldamp_trainer_stage: stage %d has no InstanceNorm", stage);
        *offset = L.rstd + (int64_t)unroll * 2 * B * RSTD_FLOATS + rstd_prefix(stage) * 2 * B;
        *n_images = 2 * B; *channels = STAGE_DIM[stage].c; *height = 1; *width = 1;
        return SBC_OK;
    case SBC_LDAMP_TRAIN_GH:
    case SBC_LDAMP_TRAIN_GZ:
        *offset = (kind == SBC_LDAMP_TRAIN_GH ? L.gh : L.gz) + (int64_t)unroll * B * 2 * PIX;
        *n_images = B; *channels = 1; *height = 2 * PIX; *width = 1;
        return SBC_OK;
    case SBC_LDAMP_TRAIN_DIV:
        *offset = L.div + (int64_t)unroll * B;
        *n_images = B; *channels = 1; *height = 1; *width = 1;
        return SBC_OK;
    default:
        SBC_REQUIRE(false, "sbc_ldamp_trainer_stage: unknown kind %d", kind);
    }
    return SBC_OK;
}

int sbc_ldamp_trainer_step(sbc_ldamp_trainer* h, const sbc_ldamp_step_desc* d, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(h && d, "sbc_ldamp_trainer_step: NULL handle or descriptor");
    SBC_REQUIRE(d->Nt == NT && d->Nr == NR, "sbc_ldamp_trainer_step: supported geometry is Nt = %d, Nr = %d (got %d x %d)", NT, NR, d->Nt, d->Nr);
    SBC_REQUIRE(d->Np >= 1 && d->Np <= NT, "sbc_ldamp_trainer_step: Np must be in [1, %d] (got %d)", NT, d->Np);
    SBC_REQUIRE(d->B >= 0 && d->B <= 128, "sbc_ldamp_trainer_step: B must be in [0, 128] (got %d)", d->B);
    SBC_REQUIRE(d->num_unrolls >= 1 && d->num_unrolls <= h->n_nets, "sbc_ldamp_trainer_step: num_unrolls must be in [1, %d] (got %d)", h->n_nets,
                d->num_unrolls);
    const struct { const void* p; const char* name; } need[] = {{d->Y_herm, "Y_herm"}, {d->P_herm, "P_herm"}, {d->eig1, "eig1"}, {d->Htrue, "Htrue"},
                                                                 {d->loss, "loss"}, {d->workspace, "workspace"}};
    for (const auto& q : need) SBC_REQUIRE(q.p, "sbc_ldamp_trainer_step: NULL %s", q.name);
    SBC_REQUIRE(d->step >= 0, "sbc_ldamp_trainer_step: step must be >= 0 (got %lld)", (long long)d->step);
    SBC_REQUIRE(d->step == 0 || (d->lr >= 0.0 && d->lr == d->lr), "sbc_ldamp_trainer_step: lr must be >= 0 (got %g)", d->lr);
    const int rc = trainer_device(h, "sbc_ldamp_trainer_step");
    if (rc) return rc;
    if (d->B == 0) return SBC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int B = d->B, Np = d->Np, U = d->num_unrolls;
    const TrainLayout L(B, U, !d->directions);
    float* ws = d->workspace;
    float *z = ws + L.z, *eps = ws + L.eps, *hhat = ws + L.hhat, *divs = ws + L.div;
    const float* dirs = d->directions;
    if (!dirs) {
        ldamp_launch_dirs(ws + L.dirs, d->seed, d->sample0, 0, B, U, s);
        dirs = ws + L.dirs;
    }
    SBC_CHECK_HIP(hipMemcpyAsync(z, d->Y_herm, sizeof(float) * 2 * (size_t)B * Np * NR, hipMemcpyDeviceToDevice, s));
    // ---- forward: the launches of sbc_ldamp_run, every unroll in a workspace of its own
    for (int u = 0; u < U; ++u) {
        const float* wn = h->params + (size_t)u * NET_FLOATS;
        const float* du = dirs + (size_t)u * B * 2 * PIX;
        const Ws f{ws + L.fwd + (int64_t)u * 2 * B * EVAL_FLOATS, 2 * B};
        PrepArgs pa{};
        pa.P = d->P_herm; pa.z = z; pa.h = u ? hhat : nullptr; pa.eig = d->eig1; pa.dirs = du; pa.eps = eps;
        pa.eps_log = d->eps_log ? d->eps_log + (size_t)u * B : nullptr;
        pa.r = f.at(S_R); pa.x = f.at(S_X); pa.stat = f.at(S_STAT); pa.B = B; pa.Np = Np;
        ldamp_launch_prep(&pa, B, s);
        unet<true>(wn, f, s, ws + L.rstd + (int64_t)u * 2 * B * RSTD_FLOATS);
        FinishArgs fa{};
        fa.u2 = f.at(S_U2); fa.r = f.at(S_R); fa.stat = f.at(S_STAT); fa.w = wn + tensor_prefix(W_FIN); fa.bias = wn + tensor_prefix(W_FINB);
        fa.h_out = hhat; fa.damp = 1; fa.P = d->P_herm; fa.Y = d->Y_herm; fa.z = z; fa.eps = eps; fa.dirs = du;
        fa.h_log = d->h_log ? d->h_log + (size_t)u * B * 2 * PIX : nullptr;
        fa.z_log = d->z_log ? d->z_log + (size_t)u * B * 2 * Np * NR : nullptr;
        fa.div_log = divs + (size_t)u * B;
        fa.B = B; fa.Np = Np; fa.last = 0;
        ldamp_launch_finish(&fa, B, s);
    }
    if (d->div_log) SBC_CHECK_HIP(hipMemcpyAsync(d->div_log, divs, sizeof(float) * (size_t)U * B, hipMemcpyDeviceToDevice, s));
    // ---- loss
    hipLaunchKernelGGL(ldamp_loss_kernel, dim3(B), dim3(256), 0, s, hhat, d->Htrue, ws + L.gh + (int64_t)(U - 1) * B * 2 * PIX, ws + L.err, B);
    hipLaunchKernelGGL(ldamp_loss_reduce_kernel, dim3(1), dim3(64), 0, s, ws + L.err, d->loss, B);
    // ---- backward, from the last unroll to the first
    for (int u = U - 1; u >= 0; --u) {
        const float* wn = h->params + (size_t)u * NET_FLOATS;
        float* gn = h->grads() + (size_t)u * NET_FLOATS;
        const Ws f{ws + L.fwd + (int64_t)u * 2 * B * EVAL_FLOATS, 2 * B};
        const Ws g{ws + L.grad + (int64_t)u * B * EVAL_FLOATS, B};
        float* gh = ws + L.gh + (int64_t)u * B * 2 * PIX;
        const float* gz_next = u == U - 1 ? nullptr : ws + L.gz + (int64_t)(u + 1) * B * 2 * PIX;
        FinBwdArgs fb{};
        fb.u2 = f.at(S_U2); fb.stat = f.at(S_STAT); fb.w = wn + tensor_prefix(W_FIN); fb.bias = wn + tensor_prefix(W_FINB); fb.gh = gh;
        fb.gz_next = gz_next; fb.P = d->P_herm; fb.g_r = g.at(S_R); fb.g_u2 = g.at(S_U2); fb.g_stat = g.at(S_STAT); fb.part = ws + L.part; fb.Np = Np;
        hipLaunchKernelGGL(ldamp_finish_bwd_kernel, dim3(B), dim3(256), 0, s, fb);
        hipLaunchKernelGGL(ldamp_finish_wgrad_kernel, dim3(1), dim3(64), 0, s, ws + L.part, gn + tensor_prefix(W_FIN), B);
        const Bwd bw{wn, gn, f, g, ws + L.rstd + (int64_t)u * 2 * B * RSTD_FLOATS, ws + L.gpre, B, s};
        bw.unet();
        PrepBwdArgs pb{};
        pb.r = f.at(S_R); pb.stat = f.at(S_STAT); pb.g_x = g.at(S_X); pb.g_stat = g.at(S_STAT); pb.g_r = g.at(S_R); pb.P = d->P_herm; pb.eig = d->eig1;
        pb.div = divs + (size_t)u * B; pb.gz_next = gz_next; pb.gz = ws + L.gz + (int64_t)u * B * 2 * PIX;
        pb.gh_prev = u ? ws + L.gh + (int64_t)(u - 1) * B * 2 * PIX : nullptr; pb.Np = Np;
        hipLaunchKernelGGL(ldamp_prep_bwd_kernel, dim3(B), dim3(256), 0, s, pb);
    }
    // ---- Adam on the nets that were used (a net without a gradient is skipped, as torch skips a parameter whose .grad is None)
    if (d->step > 0) {
        const double t = (double)d->step, bc1 = 1.0 - pow(0.9, t), bc2 = 1.0 - pow(0.999, t);
        const int64_t n = (int64_t)U * NET_FLOATS;
        hipLaunchKernelGGL(ldamp_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->grads(), h->params, h->m(), h->v(), n,
                           (float)(d->lr / bc1), (float)sqrt(bc2));
        h->step = d->step;
    }
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int sbc_ldamp_trainer_adam(sbc_ldamp_trainer* h, const float* grads, int32_t n_nets, double lr, int64_t step, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(h && n_nets >= 1 && n_nets <= h->n_nets, "sbc_ldamp_trainer_adam: need a handle and 1 <= n_nets <= %d (got %d)", h ? h->n_nets : 0, n_nets);
    SBC_REQUIRE(step >= 1 && lr >= 0.0 && lr == lr, "sbc_ldamp_trainer_adam: need step >= 1 and lr >= 0 (got %lld, %g)", (long long)step, lr);
    const int rc = trainer_device(h, "sbc_ldamp_trainer_adam");
    if (rc) return rc;
    const double t = (double)step, bc1 = 1.0 - pow(0.9, t), bc2 = 1.0 - pow(0.999, t);
    const int64_t n = (int64_t)n_nets * NET_FLOATS;
    hipLaunchKernelGGL(ldamp_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grads ? grads : h->grads(), h->params,
                       h->m(), h->v(), n, (float)(lr / bc1), (float)sqrt(bc2));
    SBC_CHECK_HIP(hipGetLastError());
    h->step = step;
    return SBC_OK;
}

// what: 0 parameters, 1 gradients of the last step, 2 exp_avg, 3 exp_avg_sq
int sbc_ldamp_trainer_get_state(sbc_ldamp_trainer* h, int32_t what, float* out, int64_t* step) {
    using namespace sbc;
    SBC_REQUIRE(h && what >= 0 && what <= 3, "sbc_ldamp_trainer_get_state: need a handle and what in [0, 3] (got %d)", what);
    const int rc = trainer_device(h, "sbc_ldamp_trainer_get_state");
    if (rc) return rc;
    SBC_CHECK_HIP(hipDeviceSynchronize());
    if (out) SBC_CHECK_HIP(hipMemcpy(out, h->params + what * h->n(), sizeof(float) * h->n(), hipMemcpyDeviceToHost));
    if (step) *step = h->step;
    return SBC_OK;
}

int sbc_ldamp_trainer_set_state(sbc_ldamp_trainer* h, int32_t what, const float* in, int64_t step) {
    using namespace sbc;
    SBC_REQUIRE(h && what >= 0 && what <= 3 && step >= 0, "sbc_ldamp_trainer_set_state: need a handle, what in [0, 3] and step >= 0 (got %d, %lld)", what,
                (long long)step);
    const int rc = trainer_device(h, "sbc_ldamp_trainer_set_state");
    if (rc) return rc;
    SBC_CHECK_HIP(hipDeviceSynchronize());
    if (in) SBC_CHECK_HIP(hipMemcpy(h->params + what * h->n(), in, sizeof(float) * h->n(), hipMemcpyHostToDevice));
    h->step = step;
    return SBC_OK;
}

}  // extern "C"
