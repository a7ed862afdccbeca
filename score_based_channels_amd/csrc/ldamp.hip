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
#include "ldamp_shared.h"

namespace sbc {
namespace {

// ---- directions ---------------------------------------------------------------------------------------------------------------
// d[u][b][e][0..1] = the two N(0,1) draws of philox.h::normal_pair(seed, stream = sample0 + b, step = unroll0 + u, elem = e), e = t * 16 + r
__global__ __launch_bounds__(256) void ldamp_dirs_kernel(float* __restrict__ d, uint64_t seed, int64_t sample0, int unroll0, int B) {
    const int b = blockIdx.x, u = blockIdx.y;
    float2* o = reinterpret_cast<float2*>(d) + ((size_t)u * B + b) * PIX;
    for (int e = threadIdx.x; e < PIX; e += 256) o[e] = normal_pair(seed, sample0 + b, unroll0 + u, e);
}

// ---- prep: r, eps, perturbation, norm -----------------------------------------------------------------------------------------

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

}  // namespace

void ldamp_launch_prep(const void* prep_args, int B, hipStream_t s) {
    hipLaunchKernelGGL(ldamp_prep_kernel, dim3(B), dim3(256), 0, s, *static_cast<const PrepArgs*>(prep_args));
}
void ldamp_launch_finish(const void* finish_args, int B, hipStream_t s) {
    hipLaunchKernelGGL(ldamp_finish_kernel, dim3(B), dim3(256), 0, s, *static_cast<const FinishArgs*>(finish_args));
}
void ldamp_launch_dirs(float* d, uint64_t seed, int64_t sample0, int unroll0, int B, int unrolls, hipStream_t s) {
    hipLaunchKernelGGL(ldamp_dirs_kernel, dim3(B, unrolls), dim3(256), 0, s, d, seed, sample0, unroll0, B);
}

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
