// EM-GM-AMP channel estimation (the EM-GM-AMP baseline of Fig. 5c, matlab/test_em_gm_amp.m): Bernoulli Gaussian-mixture GAMP with
// an EM-learned prior and noise variance on the script's operator  Y = A1 X Fr + noise,  A1 = P Fl,  X = fft2(H)  (:99-101).
// The script only calls EMGMAMP(...) from a MATLAB toolbox whose source is not in the reference's tree: what runs here is the
// algorithm DEFINED in include/sbc_hip.h (sbc_em_gm_amp_run) and DESIGN.md section 18, restated from the published method, not a
// port of the toolbox; its yardstick is the float64 numpy restatement of that definition (tests/gamp_oracle.py).
//
// One workgroup of 4 waves per problem runs every EM and GAMP iteration in one launch.  Wave w owns rows 16 w .. 16 w + 15 of the
// 64 x 16 unknown: xhat, taux, s and the previous EM iteration's xhat live in registers in the accumulator layout of the float64
// MFMA (a lane holds rows 16 w + g + 4 r, r = 0..3, of column c); A1 (Np padded to a multiple of 16 with zero rows), Y, s, xhat,
// H and the twiddles live in LDS, carved up for the padded Np (119 KB at the script's Np = 38, 142 KB at Np = 64: one workgroup
// per CU).  Per GAMP iteration, with each complex product as four real products on v_mfma_f64_16x16x4_f64:
//     T = A1 xhat        NpP x 64 x 16  CMAC   (wave w: pilot rows 16 w ..; waves beyond the padded Np idle)
//     Z = T Fr           NpP x 16 x 16         followed in registers by the output step (phat, s, zhat)
//     U = A1^H s         64 x NpP x 16
//     V = U Fr^H         64 x 16 x 16          followed in registers by rhat and the denoiser
// = 8 x 103936 real FLOP = 0.83 MFLOP at Np = 38.  The two variance products (a2 rowsum(taux), a2^T taus, a2 = |A1|^2 formed from
// A1 where it is used) are real matrix-vector products on the vector ALUs, one thread per output.
//
// WHY FLOAT64.  The iteration is not contractive at fp32 resolution: on the fp32 MFMA with fp32 state this kernel missed the bound
// its tests hold it to (4 x the float32 restatement's own distance from float64, floor 8 ulp) on 5 of 2520 short-horizon
// comparisons (lambda, psi, NMSE: 9-13 ulp after 10-30 iterations).  The whole iteration is therefore float64; the operands
// P, Y, H and the outputs stay fp32.  Products over 64 terms keep the two real halves of the complex
// product in separate accumulators: four independent MFMA chains of 16 in flight instead of two of 32.
// Every sum has a fixed order (MFMA chains, lane butterflies, then the four waves in order); nothing is atomic, nothing is read
// from or written to global memory inside the iteration except the log word at the end of an EM iteration.
#include "common.h"
#include "reduce.h"
#include <math.h>
#include <map>
#include <mutex>
#include <vector>

namespace sbc {
namespace {

constexpr int GA_NT = 64, GA_NR = 16, GA_N = GA_NT * GA_NR;   // the supported geometry
constexpr int GA_TH = 256, GA_NW = 4;
constexpr int GA_AS = GA_NT + 1;                              // padded row stride of A1 (double2)
constexpr int GA_TS = GA_NR + 1;                              // padded row stride of the T / U transit buffer
constexpr int GA_L = 4;                                       // Gaussian components of the prior
constexpr int GA_RED = 12;                                    // widest block reduction
constexpr float GA_SENTINEL = 1000.f;                         // complete_log's fill (:71)

typedef double d4 __attribute__((ext_vector_type(4)));
// v_mfma_f64_16x16x4_f64: A[i = c][k = g], B[k = g][j = c] as the fp32 form, one f64 per lane; D[g + 4 r][c] (NOT the fp32 form's 4 g + r)
__device__ __forceinline__ d4 mfma(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// LDS carve-up in floats for Np padded to npp rows
struct Carve {
    int red, cst, tp, ts, tr, rs, twr, twl, a1, y, s, x, tu, h, total;
};
__host__ __device__ inline Carve carve(int npp) {
    Carve c;
    c.red = 0;                                   // 4 x GA_RED doubles
    c.cst = c.red + 2 * GA_NW * GA_RED;          // per row of X: the five log-weight constants and 1 / variances, double [64][10]
    c.tp = c.cst + 2 * GA_NT * 2 * (GA_L + 1);   // taup, double [64]
    c.ts = c.tp + 128;                           // taus, double [64]
    c.tr = c.ts + 128;                           // taur, double [64]
    c.rs = c.tr + 128;                           // row sums of taux, double [64]
    c.twr = c.rs + 128;                          // exp(+2 pi i q / Nr) / Nr, double2 [Nr]
    c.twl = c.twr + 4 * GA_NR;                   // exp(+2 pi i q / Nt) / Nt, double2 [Nt]
    c.a1 = c.twl + 4 * GA_NT;                    // double2 [npp][GA_AS]   (a2 = |A1|^2 is formed from it where it is used)
    c.y = c.a1 + 4 * npp * GA_AS;                // float2  [npp][Nr]
    c.s = c.y + 2 * npp * GA_NR;                 // double2 [npp][Nr]
    c.x = c.s + 4 * npp * GA_NR;                 // double2 [Nt][Nr]
    c.tu = c.x + 4 * GA_N;                       // double2 [Nt][GA_TS]
    c.h = c.tu + 4 * GA_NT * GA_TS;              // float2  [Nt][Nr]
    c.total = c.h + 2 * GA_N;
    return c;
}

// K sums over the workgroup, every thread gets them: lane butterflies, then the waves in order
template <int K>
__device__ __forceinline__ void block_sums(double (&v)[K], double* red, int lane, int wave) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();                                   // red may still be read from the previous reduction
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
}

// Hh = Fl (x Fr) for this wave's 16 rows, x read from LDS (Xs); TU is the transit buffer.  Ends behind a barrier-free read of TU:
// the caller synchronises before TU is written again.
__device__ __forceinline__ void spatial(const double2* Xs, double2* TU, const double2* twr, const double2* twl, int wave, int c, int g,
                                        double (&hr)[4], double (&hi)[4]) {
    d4 wr = {0.0, 0.0, 0.0, 0.0}, wi = wr;
#pragma unroll
    for (int s = 0; s < GA_NR / 4; ++s) {
        const int q = 4 * s + g;
        const double2 x = Xs[(16 * wave + c) * GA_NR + q], f = twr[(q * c) & (GA_NR - 1)];
        wr = mfma(x.x, f.x, wr); wr = mfma(-x.y, f.y, wr);
        wi = mfma(x.x, f.y, wi); wi = mfma(x.y, f.x, wi);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) TU[(16 * wave + g + 4 * r) * GA_TS + c] = make_double2(wr[r], wi[r]);
    __syncthreads();
    d4 r0 = {0.0, 0.0, 0.0, 0.0}, r1 = r0, i0 = r0, i1 = r0;
#pragma unroll 4
    for (int s = 0; s < GA_NT / 4; ++s) {
        const int m = 4 * s + g;
        const double2 f = twl[((16 * wave + c) * m) & (GA_NT - 1)], w = TU[m * GA_TS + c];
        r0 = mfma(f.x, w.x, r0); r1 = mfma(-f.y, w.y, r1);
        i0 = mfma(f.x, w.y, i0); i1 = mfma(f.y, w.x, i1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        hr[r] = r0[r] + r1[r];
        hi[r] = i0[r] + i1[r];
    }
}

__global__ __launch_bounds__(GA_TH) void em_gm_amp_kernel(sbc_em_gm_amp_desc d, const double2* __restrict__ tldg,
                                                          const double2* __restrict__ trdg) {
    constexpr int NT = GA_NT, NR = GA_NR, TH = GA_TH;
    extern __shared__ __align__(16) float smf[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int b = blockIdx.x, B = d.B, Np = d.Np, npp = (Np + 15) & ~15, ntile = npp >> 4;
    const Carve cv = carve(npp);
    double* red = reinterpret_cast<double*>(smf + cv.red);
    double* cst = reinterpret_cast<double*>(smf + cv.cst);
    double* tpv = reinterpret_cast<double*>(smf + cv.tp);
    double* tsv = reinterpret_cast<double*>(smf + cv.ts);
    double* trv = reinterpret_cast<double*>(smf + cv.tr);
    double* rs = reinterpret_cast<double*>(smf + cv.rs);
    double2* twr = reinterpret_cast<double2*>(smf + cv.twr);
    double2* twl = reinterpret_cast<double2*>(smf + cv.twl);
    double2* A1 = reinterpret_cast<double2*>(smf + cv.a1);
    float2* Yv = reinterpret_cast<float2*>(smf + cv.y);
    double2* Ss = reinterpret_cast<double2*>(smf + cv.s);
    double2* Xs = reinterpret_cast<double2*>(smf + cv.x);
    double2* TU = reinterpret_cast<double2*>(smf + cv.tu);
    float2* Ht = reinterpret_cast<float2*>(smf + cv.h);

    const int pi = d.p_index ? d.p_index[b] : b, hi_ = d.Htrue ? (d.h_index ? d.h_index[b] : b) : 0;
    if (pi < 0 || pi >= d.nP || (d.Htrue && (hi_ < 0 || hi_ >= d.nH))) {   // bad index: NaN outputs, nothing read out of bounds
        if (d.nmse)
            for (int k = tid; k < d.em_iters; k += TH) d.nmse[(size_t)k * B + b] = NAN;
        for (int e = tid; e < GA_N; e += TH) {
            if (d.H_hat) reinterpret_cast<float2*>(d.H_hat)[(size_t)b * GA_N + e] = make_float2(NAN, NAN);
            if (d.X) reinterpret_cast<float2*>(d.X)[(size_t)b * GA_N + e] = make_float2(NAN, NAN);
        }
        if (d.params && tid < 2 + 2 * GA_L) d.params[(size_t)b * (2 + 2 * GA_L) + tid] = NAN;
        if (d.stop_iter && tid == 0) d.stop_iter[b] = -1;
        return;
    }
    const float2* P = reinterpret_cast<const float2*>(d.P) + (size_t)pi * Np * NT;
    const float2* Y = reinterpret_cast<const float2*>(d.Y) + (size_t)b * Np * NR;
    const double theta = (double)d.theta;

    // ---- prologue: twiddles, A1 = P Fl, Y, H and their norms
    if (tid < NR) twr[tid] = trdg[tid];
    if (tid < NT) twl[tid] = tldg[tid];
    double nrm[3] = {0.0, 0.0, 0.0};                 // ||A1||_F^2, ||Y||^2, ||H||^2
    for (int e = tid; e < npp * NT; e += TH) {
        const int p = e / NT, i = e % NT;
        double re = 0.0, im = 0.0;
        if (p < Np) {
            for (int k = 0; k < NT; ++k) {
                const float2 u = P[p * NT + k];
                const double2 w = tldg[(k * i) & (NT - 1)];
                re += (double)u.x * w.x - (double)u.y * w.y;
                im += (double)u.x * w.y + (double)u.y * w.x;
            }
        }
        A1[p * GA_AS + i] = make_double2(re, im);
        nrm[0] += re * re + im * im;
    }
    for (int e = tid; e < npp * NR; e += TH) {
        const int p = e / NR;
        const float2 y = p < Np ? Y[e] : make_float2(0.f, 0.f);
        Yv[e] = y;
        Ss[e] = make_double2(0.0, 0.0);
        nrm[1] += (double)y.x * y.x + (double)y.y * y.y;
    }
    if (d.Htrue) {
        const float2* H = reinterpret_cast<const float2*>(d.Htrue) + (size_t)hi_ * GA_N;
        for (int e = tid; e < GA_N; e += TH) {
            const float2 h = H[e];
            Ht[e] = h;
            nrm[2] += (double)h.x * h.x + (double)h.y * h.y;
        }
    }
    if (tid < 64) tsv[tid] = 0.0;
    block_sums<3>(nrm, red, lane, wave);
    const double hnorm = nrm[2];

    // ---- initialisation
    const double Mm = (double)Np * NR;
    double lam = 0.5 * Np / NT;
    double psi = nrm[1] / (101.0 * Mm);
    const double phibar = (nrm[1] - Mm * psi) / (nrm[0] * lam);
    double om[GA_L], phi[GA_L];
#pragma unroll
    for (int l = 0; l < GA_L; ++l) {
        om[l] = 0.25;
        phi[l] = phibar * ((double)(1 << (2 * l)) * 4.0 / 85.0);
    }
    double hr[4] = {0.0, 0.0, 0.0, 0.0}, hi[4] = {0.0, 0.0, 0.0, 0.0};
    double xr[4], xi[4], tx[4], pr[4], pim[4], sr[4], si[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        xr[r] = xi[r] = pr[r] = pim[r] = sr[r] = si[r] = 0.0;
        tx[r] = lam * phibar;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 16 * wave + g + 4 * r;
        Xs[i * NR + c] = make_double2(0.0, 0.0);
        double v = tx[r];
        v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
        if (c == 0) rs[i] = v;
    }
    __syncthreads();

    int ran = 0;
    bool first = true;
    for (int k = 0; k < d.em_iters; ++k) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pr[r] = xr[r];
            pim[r] = xi[r];
        }
        // The log-weights: log a_l = (log w_l - log v_l) - |rhat|^2 / v_l is the difference of two numbers that reach the hundreds
        // for a strong coefficient; in fp32 its rounding (|log a| 2^-24, absolute) would become the relative error of the weight.
        // Per row of X the constants are computed once (taur is the same along a row).
        const double l0 = log(1.0 - lam);
        double ll[GA_L];
#pragma unroll
        for (int l = 0; l < GA_L; ++l) ll[l] = log(lam * om[l]);
        double st[GA_RED];                                   // sum beta_l [4], sum beta_l m_l [4], psi, |x - x_prev|^2, |x|^2, (nmse)
#pragma unroll
        for (int q = 0; q < GA_RED; ++q) st[q] = 0.0;

        for (int t = 0; t < d.nit; ++t) {
            const bool last = t == d.nit - 1;
            // ---- taup, taus (one thread per pilot row) and T = A1 xhat
            if (tid < Np) {
                double q0 = 0.0, q1 = 0.0;
                for (int i = 0; i < NT; i += 2) {
                    const double2 a0 = A1[tid * GA_AS + i], a1 = A1[tid * GA_AS + i + 1];
                    q0 += (a0.x * a0.x + a0.y * a0.y) * rs[i];
                    q1 += (a1.x * a1.x + a1.y * a1.y) * rs[i + 1];
                }
                const double tp = (q0 + q1) * (1.0 / (NR * NR));
                const double tsn = 1.0 / (tp + psi);
                tpv[tid] = tp;
                tsv[tid] = first ? tsn : (1.0 - theta) * tsv[tid] + theta * tsn;
            }
            if (wave < ntile) {
                d4 r0 = {0.0, 0.0, 0.0, 0.0}, r1 = r0, i0 = r0, i1 = r0;
#pragma unroll 4
                for (int s = 0; s < NT / 4; ++s) {
                    const int m = 4 * s + g;
                    const double2 a = A1[(16 * wave + c) * GA_AS + m], x = Xs[m * NR + c];
                    r0 = mfma(a.x, x.x, r0); r1 = mfma(-a.y, x.y, r1);
                    i0 = mfma(a.x, x.y, i0); i1 = mfma(a.y, x.x, i1);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) TU[(16 * wave + g + 4 * r) * GA_TS + c] = make_double2(r0[r] + r1[r], i0[r] + i1[r]);
            }
            __syncthreads();

            // ---- taur (one thread per row of X), Z = T Fr and the output step
            if (tid < NT) {
                double q0 = 0.0, q1 = 0.0;
                int p = 0;
                for (; p + 1 < Np; p += 2) {
                    const double2 a0 = A1[p * GA_AS + tid], a1 = A1[(p + 1) * GA_AS + tid];
                    q0 += (a0.x * a0.x + a0.y * a0.y) * tsv[p];
                    q1 += (a1.x * a1.x + a1.y * a1.y) * tsv[p + 1];
                }
                if (p < Np) {
                    const double2 a0 = A1[p * GA_AS + tid];
                    q0 += (a0.x * a0.x + a0.y * a0.y) * tsv[p];
                }
                const double trf = (double)NR / (q0 + q1);
                trv[tid] = trf;
                cst[tid * 10] = l0 - log(trf);
                cst[tid * 10 + 5] = 1.0 / trf;
#pragma unroll
                for (int l = 0; l < GA_L; ++l) {
                    const double vd = phi[l] + trf;
                    cst[tid * 10 + 1 + l] = ll[l] - log(vd);
                    cst[tid * 10 + 6 + l] = 1.0 / vd;
                }
            }
            if (wave < ntile) {
                d4 zr = {0.0, 0.0, 0.0, 0.0}, zi = zr;
#pragma unroll
                for (int s = 0; s < NR / 4; ++s) {
                    const int q = 4 * s + g;
                    const double2 tv = TU[(16 * wave + c) * GA_TS + q], f = twr[(q * c) & (NR - 1)];
                    zr = mfma(tv.x, f.x, zr); zr = mfma(-tv.y, f.y, zr);
                    zi = mfma(tv.x, f.y, zi); zi = mfma(tv.y, f.x, zi);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int p = 16 * wave + g + 4 * r, e = p * NR + c;
                    if (p < Np) {                                        // the zero rows of the padding stay out of s and psi
                        const double tp = tpv[p], den = tp + psi;
                        const float2 y = Yv[e];
                        const double phr = zr[r] - tp * sr[r], phi_ = zi[r] - tp * si[r];
                        const double nr_ = ((double)y.x - phr) / den, ni_ = ((double)y.y - phi_) / den;
                        sr[r] = first ? nr_ : (1.0 - theta) * sr[r] + theta * nr_;
                        si[r] = first ? ni_ : (1.0 - theta) * si[r] + theta * ni_;
                        if (last) {
                            const double dr = (double)y.x - (phr + tp * nr_), di = (double)y.y - (phi_ + tp * ni_);
                            st[8] += (dr * dr + di * di) + tp * psi / den;
                        }
                    }
                    Ss[e] = make_double2(sr[r], si[r]);
                }
            }
            __syncthreads();

            // ---- U = A1^H s for this wave's rows of X
            {
                d4 r0 = {0.0, 0.0, 0.0, 0.0}, r1 = r0, i0 = r0, i1 = r0;
                for (int tt = 0; tt < ntile; ++tt) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int p = 16 * tt + 4 * s + g;
                        const double2 a = A1[p * GA_AS + 16 * wave + c], sv = Ss[p * NR + c];
                        r0 = mfma(a.x, sv.x, r0); r1 = mfma(a.y, sv.y, r1);          // conj(a) s
                        i0 = mfma(a.x, sv.y, i0); i1 = mfma(-a.y, sv.x, i1);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) TU[(16 * wave + g + 4 * r) * GA_TS + c] = make_double2(r0[r] + r1[r], i0[r] + i1[r]);
            }
            __syncthreads();

            // ---- V = U Fr^H, rhat = xhat + taur V, the denoiser
            {
                d4 vr = {0.0, 0.0, 0.0, 0.0}, vi = vr;
#pragma unroll
                for (int s = 0; s < NR / 4; ++s) {
                    const int q = 4 * s + g;
                    const double2 u = TU[(16 * wave + c) * GA_TS + q], f = twr[(q * c) & (NR - 1)];
                    vr = mfma(u.x, f.x, vr); vr = mfma(u.y, f.y, vr);            // u conj(f)
                    vi = mfma(u.y, f.x, vi); vi = mfma(-u.x, f.y, vi);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * wave + g + 4 * r;
                    const double tr = trv[i];
                    const double rr = xr[r] + tr * vr[r], ri = xi[r] + tr * vi[r];
                    const double r2 = rr * rr + ri * ri;
                    const double la0 = cst[i * 10] - r2 * cst[i * 10 + 5];
                    double la[GA_L], mx = la0;
#pragma unroll
                    for (int l = 0; l < GA_L; ++l) {
                        la[l] = cst[i * 10 + 1 + l] - r2 * cst[i * 10 + 6 + l];
                        mx = fmax(mx, la[l]);
                    }
                    double tot = exp(la0 - mx), al[GA_L], asum = 0.0;
#pragma unroll
                    for (int l = 0; l < GA_L; ++l) {
                        al[l] = exp(la[l] - mx);
                        asum += al[l];
                    }
                    tot += asum;
                    double sg = 0.0, sm = 0.0;
#pragma unroll
                    for (int l = 0; l < GA_L; ++l) {
                        const double iv = cst[i * 10 + 6 + l];                     // 1 / (phi_l + taur)
                        const double be = al[l] / tot, gl = phi[l] * iv;
                        const double ml = phi[l] * tr * iv + gl * gl * r2;
                        sg += be * gl;
                        sm += be * ml;
                        if (last) {
                            st[l] += be;
                            st[GA_L + l] += be * ml;
                        }
                    }
                    xr[r] = sg * rr;
                    xi[r] = sg * ri;
                    tx[r] = sm - (xr[r] * xr[r] + xi[r] * xi[r]);
                    Xs[i * NR + c] = make_double2(xr[r], xi[r]);
                    double v = tx[r];
                    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
                    if (c == 0) rs[i] = v;
                }
            }
            first = false;
            __syncthreads();
        }

        // ---- EM update from the last GAMP iteration's quantities; every thread computes the same numbers
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double dr = xr[r] - pr[r], di = xi[r] - pim[r];
            st[9] += dr * dr + di * di;
            st[10] += xr[r] * xr[r] + xi[r] * xi[r];
        }
        block_sums<GA_RED>(st, red, lane, wave);
        const double spi = ((st[0] + st[1]) + st[2]) + st[3];
        lam = fmin(fmax(spi / (double)GA_N, 1.0 / (double)GA_N), 1.0);
        if (!(spi == spi)) lam = spi;                                         // NaN stays NaN
#pragma unroll
        for (int l = 0; l < GA_L; ++l) {
            om[l] = st[l] / spi;
            if (st[l] != 0.0) {
                const double q = st[GA_L + l] / st[l];
                phi[l] = q == q ? fmax(q, 1e-12 * phibar) : q;               // NaN stays NaN
            }
        }
        psi = st[8] / Mm;
        ran = k + 1;

        // ---- the log row: ||Fl xhat Fr - H||^2 / ||H||^2
        if (d.nmse) {
            spatial(Xs, TU, twr, twl, wave, c, g, hr, hi);
            double er[1] = {0.0};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float2 h = Ht[(16 * wave + g + 4 * r) * NR + c];
                const float dr = (float)hr[r] - h.x, di = (float)hi[r] - h.y;   // of the very fp32 H_hat that is returned
                er[0] += (double)dr * dr + (double)di * di;
            }
            block_sums<1>(er, red, lane, wave);
            if (tid == 0) d.nmse[(size_t)k * B + b] = (float)(er[0] / hnorm);
        }
        if (d.tol > 0.f && st[9] < (double)d.tol * st[10]) break;
    }

    // ---- outputs
    if (d.nmse)
        for (int k = ran + tid; k < d.em_iters; k += TH) d.nmse[(size_t)k * B + b] = GA_SENTINEL;
    if (d.H_hat) {
        if (!d.nmse) {
            __syncthreads();
            spatial(Xs, TU, twr, twl, wave, c, g, hr, hi);
        }
        float2* o = reinterpret_cast<float2*>(d.H_hat) + (size_t)b * GA_N;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(16 * wave + g + 4 * r) * NR + c] = make_float2((float)hr[r], (float)hi[r]);
    }
    if (d.X) {
        float2* o = reinterpret_cast<float2*>(d.X) + (size_t)b * GA_N;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(16 * wave + g + 4 * r) * NR + c] = make_float2((float)xr[r], (float)xi[r]);
    }
    if (d.params && tid == 0) {
        float* o = d.params + (size_t)b * (2 + 2 * GA_L);
        o[0] = (float)lam;
#pragma unroll
        for (int l = 0; l < GA_L; ++l) {
            o[1 + l] = (float)om[l];
            o[1 + GA_L + l] = (float)phi[l];
        }
        o[1 + 2 * GA_L] = (float)psi;
    }
    if (d.stop_iter && tid == 0) d.stop_iter[b] = ran;
}

// Twiddle tables of the current device, evaluated in float64: tl[q] = exp(+2 pi i q / Nt) / Nt and tr[q] = exp(+2 pi i q / Nr) / Nr,
// so that Fl[k][i] = tl[k i mod Nt] = conj(dftmtx(Nt)) / Nt (:37) and Fr[j][r] = tr[j r mod Nr] (:38).  Allocated and uploaded
// (synchronously) on the first call per device and kept for the life of the process, as cs_l1.hip keeps its tables.
struct Tables {
    double2* tld;
    double2* trd;
};
int tables(Tables* out) {
    static std::mutex mu;
    static std::map<int, Tables> per_device;
    int dev = 0;
    SBC_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto it = per_device.find(dev);
    if (it == per_device.end()) {
        std::vector<double2> hd(GA_NT + GA_NR);
        for (int q = 0; q < GA_NT; ++q) {
            const double ph = 2.0 * M_PI * q / GA_NT;
            hd[q] = make_double2(cos(ph) / GA_NT, sin(ph) / GA_NT);
        }
        for (int q = 0; q < GA_NR; ++q) {
            const double ph = 2.0 * M_PI * q / GA_NR;
            hd[GA_NT + q] = make_double2(cos(ph) / GA_NR, sin(ph) / GA_NR);
        }
        double2* p = nullptr;
        SBC_CHECK_HIP(hipMalloc((void**)&p, hd.size() * sizeof(double2)));
        SBC_CHECK_HIP(hipMemcpy(p, hd.data(), hd.size() * sizeof(double2), hipMemcpyHostToDevice));
        Tables t;
        t.tld = p;
        t.trd = p + GA_NT;
        it = per_device.emplace(dev, t).first;
    }
    *out = it->second;
    return SBC_OK;
}

}  // namespace
}  // namespace sbc

extern "C" int sbc_em_gm_amp_run(const sbc_em_gm_amp_desc* d, void* stream) {
    using namespace sbc;
    SBC_REQUIRE(d, "sbc_em_gm_amp_run: NULL descriptor");
    if (d->Nt != GA_NT || d->Nr != GA_NR || d->Np < 1 || d->Np > d->Nt || d->nit < 1 || d->em_iters < 1 ||
        !(d->theta > 0.f && d->theta <= 1.f)) {
        set_error("sbc_em_gm_amp_run: unsupported Nt=%d Nr=%d Np=%d nit=%d em_iters=%d theta=%g (supported: Nt=64, Nr=16, "
                  "1 <= Np <= Nt, nit >= 1, em_iters >= 1, 0 < theta <= 1)", d->Nt, d->Nr, d->Np, d->nit, d->em_iters, (double)d->theta);
        return SBC_ERR_UNSUPPORTED;
    }
    SBC_REQUIRE(d->tol >= 0.f && d->tol < INFINITY, "sbc_em_gm_amp_run: tol must be finite and >= 0 (got %g)", (double)d->tol);
    SBC_REQUIRE(d->B >= 0 && d->nP >= 1 && (!d->Htrue || d->nH >= 1),
                "sbc_em_gm_amp_run: need B >= 0, nP >= 1 and (with Htrue) nH >= 1 (got B=%d nP=%d nH=%d)", d->B, d->nP, d->nH);
    SBC_REQUIRE(d->P, "sbc_em_gm_amp_run: NULL P");
    SBC_REQUIRE(d->Y, "sbc_em_gm_amp_run: NULL Y");
    SBC_REQUIRE(!d->nmse || d->Htrue, "sbc_em_gm_amp_run: nmse needs Htrue");
    if (d->B == 0) return SBC_OK;
    Tables t;
    int rc = tables(&t);
    if (rc) return rc;
    const size_t lds = (size_t)carve((d->Np + 15) & ~15).total * sizeof(float);
    rc = ensure_dyn_lds((const void*)em_gm_amp_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(em_gm_amp_kernel, dim3((unsigned)d->B), dim3(GA_TH), lds, (hipStream_t)stream, *d, t.tld, t.trd);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}
