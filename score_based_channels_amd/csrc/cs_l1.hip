// Lifted-DFT l1 channel estimation (the Lasso / fsAD baselines of Fig. 5c): accelerated proximal gradient on
//     min_X 1/2 || P Ld X Rd - Y ||_F^2 + lambda || X ||_1
// as the reference runs it with sigpy (src/score_based_channels/test_l1Fourier_lifted.py:125-190):
//     x = z = 0, t = 1;  per step:  v = z - lr grad f(z);  x' = soft(lambda lr, v);  t' = (1 + sqrt(1 + 4 t^2)) / 2;
//     z = x' + (t - 1) / t' (x' - x);  log = ||Ld x' Rd - H||^2 / ||H||^2
// (sigpy.alg.GradientMethod(accelerate=True) with proxg = sigpy.prox.L1Reg).  grad f(z) = Ld^H (G Hz - b) Rd^H with
// G = P^H P and b = P^H Y formed once per problem, and Hz = Ld z Rd = Hx' + c (Hx' - Hx) by linearity, so a step is one
// forward product Ld x Rd (which the log needs anyway) and one adjoint product.
//
// One workgroup of 4 L waves per problem runs every step in one launch: the iterate x and the momentum point z live in registers
// (wave w owns n1 rows 16 w .. 16 w + 15; each lane holds L 16x16 tiles of x and of z in the MFMA accumulator layout), everything else (G, b, E = G Hz - b, the Nt x Nr
// estimates, the n1 x Nr intermediates U and T, the twiddle tables) in LDS.  The products run on the exact-fp32 MFMA
// v_mfma_f32_16x16x4_f32, each complex product as four real products.  Per problem-step at lifting L (n1 = 64 L, n2 = 16 L):
//     forward  T = x Rd       n1 x n2 x Nr  CMAC  (registers -> LDS, contraction over n2)
//              Hx = Ld T      Nt x n1 x Nr       (LDS -> LDS)
//     Gram     E = G Hz - b   Nt x Nt x Nr
//     adjoint  U = Ld^H E     n1 x Nt x Nr
//              D = U Rd^H     n1 x Nr x n2       (LDS -> registers, followed by the prox / momentum update in place)
// At L = 4 that is 4 x 262144 + 65536 CMAC = 8 x 1114112 real FLOP = 8.91 MFLOP per problem-step.
// Every sum has a fixed order and no problem reads another's data: a problem's result does not depend on the batch.
#include "common.h"
#include "reduce.h"
#include <math.h>
#include <map>
#include <mutex>
#include <vector>

namespace sbc {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int L1_NT = 64, L1_NR = 16;      // the supported geometry (BASELINE configs 1-4)
constexpr int GS = L1_NT + 1;              // padded row stride of G (float2): the A-operand reads of G are column walks
constexpr int US = L1_NR + 1;              // padded row stride of U and T

__device__ __forceinline__ f4 mfma(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <int L>
struct Geo {
    static constexpr int N1 = L1_NT * L, N2 = L1_NR * L;          // lifted shape
    static constexpr int T1 = N1 / 16, T2 = N2 / 16;              // 16-wide tiles along n1 / n2
    static constexpr int NW = 4 * L, TPW = T1 / NW;             // waves (one n1 tile each)
    static constexpr int THREADS = NW * 64;
    // LDS carve-up in float2 units: 16 doubles of reduction scratch and 64 ints of lane columns first
    static constexpr int o_tw1 = 48, o_tw2 = o_tw1 + N1, o_g = o_tw2 + N2, o_b = o_g + L1_NT * GS, o_hx = o_b + L1_NT * L1_NR,
                         o_hz = o_hx + L1_NT * L1_NR, o_ht = o_hz + L1_NT * L1_NR, o_e = o_ht + L1_NT * L1_NR,
                         o_u = o_e + L1_NT * L1_NR, o_t = o_u + N1 * US, total = o_t + N1 * US;
    static_assert(T1 % NW == 0, "n1 tiles must split evenly over the waves");
};

// Lane l of a wave: c = l & 15, g = l >> 4.  16x16x4 MFMA: A[i = c][k = g], B[k = g][j = c], D[4 g + r][c].
// x / z tile (tp, a) of a lane, element r:  x[m = 16 (wave TPW + tp) + c][n = 16 a + 4 g + r]   (the layout of D^T = conj(Rd) U^T).
template <int L>
__global__ __launch_bounds__(Geo<L>::THREADS) void l1_lifted_kernel(sbc_l1_lifted_desc d, const float2* __restrict__ tw1g,
                                                                    const float2* __restrict__ tw2g) {
    using Gm = Geo<L>;
    constexpr int N1 = Gm::N1, N2 = Gm::N2, T2 = Gm::T2, NW = Gm::NW, TPW = Gm::TPW, TH = Gm::THREADS;
    constexpr int NT = L1_NT, NR = L1_NR;
    extern __shared__ float2 sm[];
    double* red = reinterpret_cast<double*>(sm);
    float2* tw1 = sm + Gm::o_tw1;
    float2* tw2 = sm + Gm::o_tw2;
    float2* G = sm + Gm::o_g;
    float2* bv = sm + Gm::o_b;
    float2* Hx = sm + Gm::o_hx;
    float2* Hz = sm + Gm::o_hz;
    float2* Ht = sm + Gm::o_ht;
    float2* E = sm + Gm::o_e;
    float2* U = sm + Gm::o_u;
    float2* T = sm + Gm::o_t;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int b = blockIdx.x, B = d.B, Np = d.Np;
    const int pi = d.p_index ? d.p_index[b] : b, hi = d.h_index ? d.h_index[b] : b;
    if (pi < 0 || pi >= d.nP || hi < 0 || hi >= d.nH) {            // bad index: NaN log and outputs, nothing read out of bounds
        for (int k = tid; k < d.steps; k += TH) d.nmse[(size_t)k * B + b] = NAN;
        if (d.H_hat) {
            float2* o = reinterpret_cast<float2*>(d.H_hat) + (size_t)b * NT * NR;
            for (int e = tid; e < NT * NR; e += TH) o[e] = make_float2(NAN, NAN);
        }
        if (d.X) {
            float2* o = reinterpret_cast<float2*>(d.X) + (size_t)b * N1 * N2;
            for (int e = tid; e < N1 * N2; e += TH) o[e] = make_float2(NAN, NAN);
        }
        return;
    }
    const float2* P = reinterpret_cast<const float2*>(d.P) + (size_t)pi * Np * NT;
    const float2* Y = reinterpret_cast<const float2*>(d.Y) + (size_t)b * Np * NR;
    const float2* H = reinterpret_cast<const float2*>(d.Htrue) + (size_t)hi * NT * NR;
    const float lr = d.lr[b];
    const float tau = (float)((double)d.lmbda[b] * (double)lr);     // L1Reg.prox(alpha, .) = soft_thresh(lambda alpha, .)

    // ---- prologue: twiddles, G = P^H P, b = P^H Y, H, ||H||^2, Hx = Hz = 0
    for (int i = tid; i < N1; i += TH) tw1[i] = tw1g[i];
    for (int i = tid; i < N2; i += TH) tw2[i] = tw2g[i];
    for (int e = tid; e < NT * NT; e += TH) {
        const int i = e / NT, j = e % NT;
        float re = 0.f, im = 0.f;
        for (int p = 0; p < Np; ++p) {
            const float2 u = P[p * NT + i], v = P[p * NT + j];
            re += u.x * v.x + u.y * v.y;
            im += u.x * v.y - u.y * v.x;
        }
        G[i * GS + j] = make_float2(re, im);
    }
    double hn = 0.0;
    for (int e = tid; e < NT * NR; e += TH) {
        const int i = e / NR, q = e % NR;
        float re = 0.f, im = 0.f;
        for (int p = 0; p < Np; ++p) {
            const float2 u = P[p * NT + i], v = Y[p * NR + q];
            re += u.x * v.x + u.y * v.y;
            im += u.x * v.y - u.y * v.x;
        }
        bv[e] = make_float2(re, im);
        const float2 h = H[e];
        Ht[e] = h;
        Hx[e] = Hz[e] = make_float2(0.f, 0.f);
        hn += (double)h.x * h.x + (double)h.y * h.y;
    }
    hn = wave_sum(hn);
    if (lane == 0) red[wave] = hn;
    __syncthreads();
    double hnorm = 0.0;
    for (int w = 0; w < NW; ++w) hnorm += red[w];
    __syncthreads();

    f4 xr[TPW][T2], xi[TPW][T2], zr[TPW][T2], zi[TPW][T2];
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
        for (int a = 0; a < T2; ++a) xr[tp][a] = xi[tp][a] = zr[tp][a] = zi[tp][a] = f4{0.f, 0.f, 0.f, 0.f};

    float* Ef = reinterpret_cast<float*>(E);
    float* Hxf = reinterpret_cast<float*>(Hx);
    float* Hzf = reinterpret_cast<float*>(Hz);
    const float* Htf = reinterpret_cast<const float*>(Ht);
    const float* bf = reinterpret_cast<const float*>(bv);

    // The twiddle and LDS addresses of a step are cheap to form but loop-invariant: hoisted out of the step loop they would take
    // most of the register file and push the state into scratch.  Reading the lane id from LDS (volatile) each step keeps them per step.
    volatile int* lane_col = reinterpret_cast<volatile int*>(red + 16);
    if (tid < 64) lane_col[tid] = tid;
    __syncthreads();

    double t = 1.0;
    for (int k = 0; k < d.steps; ++k) {
        const int ln = lane_col[lane], c = ln & 15, g = ln >> 4;
        const double tn = (1.0 + sqrt(1.0 + 4.0 * t * t)) / 2.0;
        const float cf = (float)((t - 1.0) / tn);                   // momentum coefficient of this step
        t = tn;

        // ---- E = G Hz - b   (8 jobs: 4 row tiles x {re, im})
        for (int job = wave; job < 8; job += NW) {
            const int tt = job >> 1, part = job & 1;
            f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
            for (int s = 0; s < NT / 4; ++s) {
                const float2 a = G[(16 * tt + c) * GS + 4 * s + g], h = Hz[(4 * s + g) * NR + c];
                if (part == 0) { acc = mfma(a.x, h.x, acc); acc = mfma(-a.y, h.y, acc); }
                else { acc = mfma(a.x, h.y, acc); acc = mfma(a.y, h.x, acc); }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = (16 * tt + 4 * g + r) * NR + c;
                Ef[2 * e + part] = acc[r] - bf[2 * e + part];
            }
        }
        __syncthreads();

        // ---- U = Ld^H E for this wave's n1 tiles; Ld^H[m][kk] = conj(tw1[kk m mod n1])
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp) {
            const int bt = wave * TPW + tp, m = 16 * bt + c;
            f4 ur = {0.f, 0.f, 0.f, 0.f}, ui = ur;
#pragma unroll 2
            for (int s = 0; s < NT / 4; ++s) {
                const int kk = 4 * s + g;
                const float2 w = tw1[(kk * m) & (N1 - 1)], e = E[kk * NR + c];
                ur = mfma(w.x, e.x, ur); ur = mfma(w.y, e.y, ur);          // conj: (wr - i wi)(er + i ei)
                ui = mfma(w.x, e.y, ui); ui = mfma(-w.y, e.x, ui);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) U[(16 * bt + 4 * g + r) * US + c] = make_float2(ur[r], ui[r]);
        }
        __syncthreads();

        // ---- D^T = conj(Rd) U^T tile by tile, then v = z - lr D, x' = soft(tau, v), z = x' + cf (x' - x); then T = x' Rd
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp) {
            const int bt = wave * TPW + tp;
#pragma unroll
            for (int a = 0; a < T2; ++a) {
                __builtin_amdgcn_sched_barrier(0);                      // one tile at a time: bounds the live registers
                const int n = 16 * a + c;
                f4 dr = {0.f, 0.f, 0.f, 0.f}, di = dr;
#pragma unroll
                for (int s = 0; s < NR / 4; ++s) {
                    const int q = 4 * s + g;
                    const float2 w = tw2[(n * q) & (N2 - 1)], u = U[(16 * bt + c) * US + q];
                    dr = mfma(w.x, u.x, dr); dr = mfma(w.y, u.y, dr);      // conj(Rd[n][q]) U[m][q]
                    di = mfma(w.x, u.y, di); di = mfma(-w.y, u.x, di);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float vr = zr[tp][a][r] - lr * dr[r], vi = zi[tp][a][r] - lr * di[r];
                    const float av = sqrtf(vr * vr + vi * vi);
                    float mg = av - tau;
                    mg = (fabsf(mg) + mg) * 0.5f;                             // sigpy.util soft_thresh, NaN kept
                    const float sr = av > 0.f ? vr / av : 0.f, si = av > 0.f ? vi / av : 0.f;
                    const float nr = mg * sr, ni = mg * si;
                    zr[tp][a][r] = nr + cf * (nr - xr[tp][a][r]);
                    zi[tp][a][r] = ni + cf * (ni - xi[tp][a][r]);
                    xr[tp][a][r] = nr;
                    xi[tp][a][r] = ni;
                }
            }
            // T^T[q][m] = sum_n Rd[n][q] x'[m][n]: A[i = q = c][k] = Rd[16 a + 4 g + r][c], B = the lane's own x' registers
            f4 tr = {0.f, 0.f, 0.f, 0.f}, ti = tr;
#pragma unroll
            for (int a = 0; a < T2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float2 w = tw2[((16 * a + 4 * g + r) * c) & (N2 - 1)];
                    tr = mfma(w.x, xr[tp][a][r], tr); tr = mfma(-w.y, xi[tp][a][r], tr);
                    ti = mfma(w.x, xi[tp][a][r], ti); ti = mfma(w.y, xr[tp][a][r], ti);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) T[(16 * bt + c) * US + 4 * g + r] = make_float2(tr[r], ti[r]);
        }
        __syncthreads();

        // ---- Hx' = Ld T (8 jobs), Hz = Hx' + cf (Hx' - Hx), and the squared error of Hx'
        double err = 0.0;
        for (int job = wave; job < 8; job += NW) {
            const int tt = job >> 1, part = job & 1, ti_ = 16 * tt + c;
            // the longest sum of a step (n1 terms per product): the two real products of the complex one are accumulated apart and added
            // at the end, which halves the chain of dependent accumulations and its rounding error (H_hat element-wise against float64
            // after 3 steps at L = 4: 1.1e-5 with one chain, 6e-6 with two; tests/test_gpu_cs_baselines.py::
            // test_l1_first_steps_at_every_pilot_count).  Not unrolled: the second accumulator's registers come out of the unrolling.
            f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll 1
            for (int s = 0; s < N1 / 4; ++s) {
                const int mm = 4 * s + g;
                const float2 w = tw1[(ti_ * mm) & (N1 - 1)], tv = T[mm * US + c];
                if (part == 0) { a0 = mfma(w.x, tv.x, a0); a1 = mfma(-w.y, tv.y, a1); }
                else { a0 = mfma(w.x, tv.y, a0); a1 = mfma(w.y, tv.x, a1); }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = 2 * ((16 * tt + 4 * g + r) * NR + c) + part;
                const float nv = a0[r] + a1[r], ov = Hxf[e];
                Hxf[e] = nv;
                Hzf[e] = nv + cf * (nv - ov);
                const float df = nv - Htf[e];
                err += (double)df * df;
            }
        }
        err = wave_sum(err);
        if (lane == 0) red[wave] = err;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int w = 0; w < NW; ++w) s += red[w];
            d.nmse[(size_t)k * B + b] = (float)(s / hnorm);
        }
    }

    // ---- outputs
    if (d.H_hat) {
        float2* o = reinterpret_cast<float2*>(d.H_hat) + (size_t)b * NT * NR;
        for (int e = tid; e < NT * NR; e += TH) o[e] = Hx[e];
    }
    if (d.X) {
        float2* o = reinterpret_cast<float2*>(d.X) + (size_t)b * N1 * N2;
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
            for (int a = 0; a < T2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    o[(size_t)(16 * (wave * TPW + tp) + c) * N2 + 16 * a + 4 * g + r] = make_float2(xr[tp][a][r], xi[tp][a][r]);
    }
}

// Twiddle tables of the current device: for L in {1, 2, 4}, w1[j] = exp(-2 pi i j / n1) / sqrt(n1) (j < n1) followed by
// w2[j] = exp(+2 pi i j / n2) / sqrt(n2) (j < n2), evaluated in float64 and rounded to float32.  So Ld[k][m] = w1[k m mod n1]
// (= conj(ifft(eye(Nt), n=n1, norm='ortho')), test_l1Fourier_lifted.py:125-126) and Rd[m][k] = w2[k m mod n2]
// (= ifft(eye(Nr), n=n2, norm='ortho').T, :127-128).  Uploaded once per device.
int twiddles(int L, const float2** w1, const float2** w2) {
    static std::mutex mu;
    static std::map<int, float2*> tables;
    int dev = 0;
    SBC_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    float2*& tab = tables[dev];
    const int lifts[3] = {1, 2, 4};
    if (!tab) {
        std::vector<float2> h;
        for (int l : lifts) {
            const int n1 = L1_NT * l, n2 = L1_NR * l;
            for (int j = 0; j < n1; ++j) {
                const double ph = -2.0 * M_PI * j / n1;
                h.push_back(make_float2((float)(cos(ph) / sqrt((double)n1)), (float)(sin(ph) / sqrt((double)n1))));
            }
            for (int j = 0; j < n2; ++j) {
                const double ph = 2.0 * M_PI * j / n2;
                h.push_back(make_float2((float)(cos(ph) / sqrt((double)n2)), (float)(sin(ph) / sqrt((double)n2))));
            }
        }
        float2* p = nullptr;
        SBC_CHECK_HIP(hipMalloc((void**)&p, h.size() * sizeof(float2)));
        SBC_CHECK_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice));
        tab = p;
    }
    size_t off = 0;
    for (int l : lifts) {
        if (l == L) break;
        off += (size_t)(L1_NT + L1_NR) * l;
    }
    *w1 = tab + off;
    *w2 = tab + off + (size_t)L1_NT * L;
    return SBC_OK;
}

template <int L>
int launch_l1(const sbc_l1_lifted_desc& d, hipStream_t stream) {
    using Gm = Geo<L>;
    const float2 *w1 = nullptr, *w2 = nullptr;
    int rc = twiddles(L, &w1, &w2);
    if (rc) return rc;
    const size_t lds = (size_t)Gm::total * sizeof(float2);
    rc = ensure_dyn_lds((const void*)l1_lifted_kernel<L>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(l1_lifted_kernel<L>, dim3((unsigned)d.B), dim3(Gm::THREADS), lds, stream, d, w1, w2);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

}  // namespace
}  // namespace sbc

extern "C" int sbc_l1_lifted_run(const sbc_l1_lifted_desc* d, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(d, "sbc_l1_lifted_run: NULL descriptor");
    if (d->Nt != L1_NT || d->Nr != L1_NR || !(d->lifting == 1 || d->lifting == 2 || d->lifting == 4) || d->Np < 1 ||
        d->Np > d->Nt) {
        set_error("sbc_l1_lifted_run: unsupported geometry Nt=%d Nr=%d Np=%d lifting=%d (supported: Nt=64, Nr=16, 1 <= Np <= Nt, "
                  "lifting 1, 2 or 4)", d->Nt, d->Nr, d->Np, d->lifting);
        return SBC_ERR_UNSUPPORTED;
    }
    SBC_REQUIRE(d->B >= 0 && d->steps >= 1 && d->nP >= 1 && d->nH >= 1,
                "sbc_l1_lifted_run: need B >= 0, steps >= 1, nP >= 1, nH >= 1 (got B=%d steps=%d nP=%d nH=%d)", d->B, d->steps, d->nP,
                d->nH);
    const struct { const void* p; const char* name; } need[] = {{d->P, "P"}, {d->Y, "Y"}, {d->Htrue, "Htrue"}, {d->lmbda, "lmbda"},
                                                                {d->lr, "lr"}, {d->nmse, "nmse"}};
    for (const auto& q : need) SBC_REQUIRE(q.p, "sbc_l1_lifted_run: NULL %s", q.name);
    if (d->B == 0) return SBC_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (d->lifting) {
        case 1: return launch_l1<1>(*d, s);
        case 2: return launch_l1<2>(*d, s);
        default: return launch_l1<4>(*d, s);
    }
}
