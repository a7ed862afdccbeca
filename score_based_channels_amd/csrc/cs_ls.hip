// Regularised least squares (the ML baseline of Fig. 5c): per problem
//     (P^H P + s2 I_Nt) H = P^H Y,   s2 = 10^(-SNR/10)                      (src/score_based_channels/test_ml.py:132-138)
// which the reference solves with np.linalg.lstsq on the Nt x Nt normal equations.  For s2 > 0 the system is solved in its
// equivalent form of size n = min(Np, Nt): with Np <= Nt,  H = P^H (P P^H + s2 I_Np)^-1 Y  (push-through identity); otherwise
// the normal equations themselves.  One 256-thread workgroup per problem: the n x n matrix and the n x Nr right-hand side in
// LDS, an in-place fp32 Cholesky factorisation M = L L^H, forward and back substitution, then H and its NMSE
// ||H - Htrue||^2 / ||Htrue||^2 (test_ml.py:141-145).  Fixed summation orders throughout.  The sums over Nt or Np (up to 1024 terms)
// are added in blocks of 64 -- one term after the other inside a block, then block after block -- so that the rounding error of a
// long sum grows like that of its blocks, not with its whole length; a sum of at most 64 terms is the plain running sum.
#include "common.h"
#include <math.h>

namespace sbc {
namespace {

constexpr int LS_THREADS = 256, LS_MAX_N = 64, LS_MAX_NR = 64, LS_BLOCK = 64;

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) {     // a * conj(b)
    return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

// sum_{t < len} term(t) in blocks of LS_BLOCK terms
template <class F>
__device__ __forceinline__ float2 blocked_sum(int len, F term) {
    float2 acc = make_float2(0.f, 0.f);
    for (int s = 0; s < len; s += LS_BLOCK) {
        const int end = s + LS_BLOCK < len ? s + LS_BLOCK : len;
        float2 part = make_float2(0.f, 0.f);
        for (int t = s; t < end; ++t) {
            const float2 v = term(t);
            part.x += v.x; part.y += v.y;
        }
        acc.x += part.x; acc.y += part.y;
    }
    return acc;
}

__global__ __launch_bounds__(LS_THREADS) void ls_regularized_kernel(sbc_ls_desc d) {
    extern __shared__ float2 sm[];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Nt = d.Nt, Nr = d.Nr, Np = d.Np;
    const bool small = Np <= Nt;                       // solve in the pilot dimension
    const int n = small ? Np : Nt, ms = n + 1;         // system size, padded row stride of M
    double* red = reinterpret_cast<double*>(sm);
    float2* M = sm + 4;
    float2* R = M + n * ms;
    const int pi = d.p_index ? d.p_index[b] : b;
    const int hi = d.Htrue ? (d.h_index ? d.h_index[b] : b) : 0;
    if (pi < 0 || pi >= d.nP || (d.Htrue && (hi < 0 || hi >= d.nH))) {  // bad index: NaN out, nothing read out of bounds
        if (d.nmse && tid == 0) d.nmse[b] = NAN;
        float2* o = reinterpret_cast<float2*>(d.H_hat) + (size_t)b * Nt * Nr;
        for (int e = tid; e < Nt * Nr; e += LS_THREADS) o[e] = make_float2(NAN, NAN);
        return;
    }
    const float2* P = reinterpret_cast<const float2*>(d.P) + (size_t)pi * Np * Nt;    // [Np][Nt]
    const float2* Y = reinterpret_cast<const float2*>(d.Y) + (size_t)b * Np * Nr;     // [Np][Nr]
    const float s2 = d.noise_var[b];

    // M = P P^H + s2 I (small) or P^H P + s2 I;  R = Y or P^H Y
    for (int e = tid; e < n * n; e += LS_THREADS) {
        const int i = e / n, j = e % n;
        float2 acc = small ? blocked_sum(Nt, [&](int t) { return cmulc(P[i * Nt + t], P[j * Nt + t]); })
                           : blocked_sum(Np, [&](int p) { return cmulc(P[p * Nt + j], P[p * Nt + i]); });   // conj(P[p][i]) P[p][j]
        if (i == j) acc.x += s2;
        M[i * ms + j] = acc;
    }
    for (int e = tid; e < n * Nr; e += LS_THREADS) {
        const int i = e / Nr, q = e % Nr;
        if (small) {
            R[e] = Y[e];
        } else {
            R[e] = blocked_sum(Np, [&](int p) { return cmulc(Y[p * Nr + q], P[p * Nt + i]); });   // conj(P[p][i]) Y[p][q]
        }
    }
    __syncthreads();

    // Cholesky, right-looking, lower triangle in place (the diagonal holds real L[j][j])
    for (int j = 0; j < n; ++j) {
        if (tid == 0) M[j * ms + j] = make_float2(sqrtf(M[j * ms + j].x), 0.f);
        __syncthreads();
        const float djj = M[j * ms + j].x;
        for (int i = j + 1 + tid; i < n; i += LS_THREADS) {
            const float2 v = M[i * ms + j];
            M[i * ms + j] = make_float2(v.x / djj, v.y / djj);
        }
        __syncthreads();
        const int cnt = n - j - 1;
        for (int e = tid; e < cnt * cnt; e += LS_THREADS) {
            const int i = j + 1 + e / cnt, k = j + 1 + e % cnt;
            if (k <= i) {
                const float2 v = cmulc(M[i * ms + j], M[k * ms + j]);
                M[i * ms + k].x -= v.x;
                M[i * ms + k].y -= v.y;
            }
        }
        __syncthreads();
    }
    // L Z = R, then L^H W = Z, one right-hand-side column per thread, in place in R
    for (int q = tid; q < Nr; q += LS_THREADS) {
        for (int i = 0; i < n; ++i) {
            float2 s = R[i * Nr + q];
            for (int k = 0; k < i; ++k) {
                const float2 v = cmul(M[i * ms + k], R[k * Nr + q]);
                s.x -= v.x; s.y -= v.y;
            }
            const float dii = M[i * ms + i].x;
            R[i * Nr + q] = make_float2(s.x / dii, s.y / dii);
        }
        for (int i = n - 1; i >= 0; --i) {
            float2 s = R[i * Nr + q];
            for (int k = i + 1; k < n; ++k) {
                const float2 v = cmulc(R[k * Nr + q], M[k * ms + i]);       // conj(L[k][i]) W[k][q]
                s.x -= v.x; s.y -= v.y;
            }
            const float dii = M[i * ms + i].x;
            R[i * Nr + q] = make_float2(s.x / dii, s.y / dii);
        }
    }
    __syncthreads();

    // H = P^H W (small) or W; squared error against Htrue
    const float2* Ht = d.Htrue ? reinterpret_cast<const float2*>(d.Htrue) + (size_t)hi * Nt * Nr : nullptr;
    float2* out = reinterpret_cast<float2*>(d.H_hat) + (size_t)b * Nt * Nr;
    double err = 0.0, hn = 0.0;
    for (int e = tid; e < Nt * Nr; e += LS_THREADS) {
        const int t = e / Nr, q = e % Nr;
        float2 h;
        if (small) {
            h = make_float2(0.f, 0.f);
            for (int p = 0; p < Np; ++p) {
                const float2 v = cmulc(R[p * Nr + q], P[p * Nt + t]);        // conj(P[p][t]) W[p][q]
                h.x += v.x; h.y += v.y;
            }
        } else {
            h = R[e];
        }
        out[e] = h;
        if (Ht) {
            const float2 r = Ht[e];
            const float dx = h.x - r.x, dy = h.y - r.y;
            err += (double)dx * dx + (double)dy * dy;
            hn += (double)r.x * r.x + (double)r.y * r.y;
        }
    }
    if (!d.nmse || !Ht) return;
    for (int o = 32; o > 0; o >>= 1) {
        err += __shfl_xor(err, o);
        hn += __shfl_xor(hn, o);
    }
    __syncthreads();                                   // everyone is done with R before red (which precedes M) is reused
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) { red[wave] = err; }
    __syncthreads();
    double se = 0.0;
    if (tid == 0)
        for (int w = 0; w < LS_THREADS / 64; ++w) se += red[w];
    __syncthreads();
    if (lane == 0) red[wave] = hn;
    __syncthreads();
    if (tid == 0) {
        double sh = 0.0;
        for (int w = 0; w < LS_THREADS / 64; ++w) sh += red[w];
        d.nmse[b] = (float)(se / sh);
    }
}

}  // namespace
}  // namespace sbc

extern "C" int sbc_ls_regularized(const sbc_ls_desc* d, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(d, "sbc_ls_regularized: NULL descriptor");
    const int n = d->Np < d->Nt ? d->Np : d->Nt;
    if (d->Nt < 1 || d->Nr < 1 || d->Np < 1 || n > LS_MAX_N || d->Nr > LS_MAX_NR || d->Nt > 1024 || d->Np > 1024) {
        set_error("sbc_ls_regularized: unsupported geometry Nt=%d Nr=%d Np=%d (supported: min(Np, Nt) <= %d, Nr <= %d, Nt, Np <= 1024)",
                  d->Nt, d->Nr, d->Np, LS_MAX_N, LS_MAX_NR);
        return SBC_ERR_UNSUPPORTED;
    }
    SBC_REQUIRE(d->B >= 0 && d->nP >= 1 && (!d->Htrue || d->nH >= 1),
                "sbc_ls_regularized: need B >= 0, nP >= 1 and (with Htrue) nH >= 1 (got B=%d nP=%d nH=%d)", d->B, d->nP, d->nH);
    const struct { const void* p; const char* name; } need[] = {{d->P, "P"}, {d->Y, "Y"}, {d->noise_var, "noise_var"}, {d->H_hat, "H_hat"}};
    for (const auto& q : need) SBC_REQUIRE(q.p, "sbc_ls_regularized: NULL %s", q.name);
    SBC_REQUIRE(!d->nmse || d->Htrue, "sbc_ls_regularized: nmse needs Htrue");
    if (d->B == 0) return SBC_OK;
    const size_t lds = (4 + (size_t)n * (n + 1) + (size_t)n * d->Nr) * sizeof(float2);
    int rc = ensure_dyn_lds((const void*)ls_regularized_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(ls_regularized_kernel, dim3((unsigned)d->B), dim3(LS_THREADS), lds, (hipStream_t)stream, *d);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}
