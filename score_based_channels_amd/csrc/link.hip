// Coded link simulation (matlab/test_end_to_end.m, testPackets.m, ComputeLLRMIMO.m 'ml'; semantics in include/sbc_hip.h): what a
// channel estimate is worth to a receiver, as coded BER / BLER with ideal against estimated CSI.  Exact fp32, fixed summation orders,
// every packet computed by its own wave / its own share of a workgroup: results do not depend on the chunk or the position in it.
//
//   link_encode_kernel   one workgroup per packet: payload (caller's or Philox) packed to words in LDS, parity = (B^-1 A) payload as
//                        popcounts of bit-packed generator rows, interleave, QPSK
//   link_index_kernel    device randomness only: a packet's channel indices, one thread per packet
//   link_llr_kernel<S>   one wave per (packet, channel use): y from the symbols, Hp_ideal[idx] and the noise, then for both channel sets
//                        the 4^S metrics |y - Hp s|^2 in the direct form (a lane owns the candidates that differ in the last stream and
//                        shares their partial sum), and per (stream, bit, value) class a log-sum-exp around the class minimum
//   link_decode_kernel   several codewords per workgroup, messages, totals and channel LLRs resident in LDS next to the edge tables;
//                        flooding schedule: checks (forward / backward [+] recursion in registers), variables, parity; stops per codeword
//   link_errors_kernel   one wave per packet: bit errors of sign(-soft) against the payload
#include "common.h"
#include "philox.h"
#include "link_tables.h"
#include <math.h>
#include <mutex>
#include <new>

namespace sbc {
namespace {

constexpr int LINK_THREADS = 256, LINK_WAVES = LINK_THREADS / 64, LINK_MAX_NR = 64;
constexpr int LINK_MAX_CW = 8;                 // codewords of one decoder workgroup
constexpr size_t LINK_LDS_BUDGET = 72 * 1024;  // of a decoder workgroup: two of them fit a CU's 160 KiB
constexpr int PURPOSE_PAYLOAD = 0, PURPOSE_INDEX = 1, PURPOSE_NOISE = 2;
constexpr float LINK_CLIP = 6.f;

// qammod(., 4, 'InputType', 'bit', 'UnitAveragePower', true): the first bit of a pair is the MSB of the integer, and MATLAB's default
// Gray map sends the integers 0, 1, 2, 3 to (-1+j, -1-j, 1+j, 1-j) / sqrt 2.  The ONE table of the unit (encoder and candidates).
__device__ __forceinline__ float2 qpsk(int v) {
    const float a = 0.70710678118654752f;
    return make_float2((v & 2) ? a : -a, (v & 1) ? -a : a);
}

__device__ __forceinline__ int stream_step(int snr_index, int purpose) { return snr_index * 4 + purpose; }

// ---- encoder ---------------------------------------------------------------------------------------------------------------------
struct EncodeParams {
    uint8_t* payload; uint8_t* codeword; float2* symbols;
    const uint32_t* gen; const int32_t* P;
    int K, M, N, Kw, nsym;
    sbc_link_random rnd;
};

__global__ __launch_bounds__(LINK_THREADS) void link_encode_kernel(EncodeParams p) {
    extern __shared__ uint32_t enc_sm[];
    uint32_t* u = enc_sm;                                          // [Kw] packed payload
    uint8_t* cw = reinterpret_cast<uint8_t*>(enc_sm + p.Kw);       // [N]
    const int tid = threadIdx.x, pk = blockIdx.x;
    uint8_t* pay = p.payload + (size_t)pk * p.K;
    const bool random = p.rnd.flags & SBC_LINK_DEVICE_RANDOM;
    for (int w = tid; w < p.Kw; w += LINK_THREADS) {
        uint32_t word = 0;
        const int left = p.K - 32 * w, nb = left < 32 ? left : 32;
        if (random) {
            const uint4 r = noise_block(p.rnd.seed, p.rnd.packet0 + pk, stream_step(p.rnd.snr_index, PURPOSE_PAYLOAD), w >> 2);
            const uint32_t c[4] = {r.x, r.y, r.z, r.w};
            word = (w & 3) == 0 ? c[0] : (w & 3) == 1 ? c[1] : (w & 3) == 2 ? c[2] : c[3];
            if (nb < 32) word &= (1u << nb) - 1u;
        } else {
            for (int i = 0; i < nb; ++i) word |= (uint32_t)(pay[32 * w + i] & 1) << i;
        }
        u[w] = word;
    }
    __syncthreads();
    for (int k = tid; k < p.K; k += LINK_THREADS) {
        const uint8_t bit = (u[k >> 5] >> (k & 31)) & 1u;
        cw[k] = bit;
        if (random) pay[k] = bit;
    }
    for (int j = tid; j < p.M; j += LINK_THREADS) {
        const uint32_t* g = p.gen + (size_t)j * p.Kw;
        uint32_t acc = 0;
        for (int w = 0; w < p.Kw; ++w) acc ^= g[w] & u[w];
        cw[p.K + j] = __popc(acc) & 1;
    }
    __syncthreads();
    if (p.codeword)
        for (int k = tid; k < p.N; k += LINK_THREADS) p.codeword[(size_t)pk * p.N + k] = cw[k];
    for (int k = tid; k < p.nsym; k += LINK_THREADS)
        p.symbols[(size_t)pk * p.nsym + k] = qpsk(2 * cw[p.P[2 * k]] + cw[p.P[2 * k + 1]]);
}

// ---- channel indices of a packet (device randomness) -----------------------------------------------------------------------------
__global__ __launch_bounds__(LINK_THREADS) void link_index_kernel(int32_t* chan_index, int Npk, int uses, int pool, sbc_link_random rnd) {
    const int pk = blockIdx.x * LINK_THREADS + threadIdx.x;
    if (pk >= Npk) return;
    int32_t* row = chan_index + (size_t)pk * uses;
    const bool distinct = pool >= uses;
    uint4 r = make_uint4(0, 0, 0, 0);
    int have = 0;
    for (uint32_t t = 0; have < uses; ++t) {
        if ((t & 3) == 0) r = noise_block(rnd.seed, rnd.packet0 + pk, stream_step(rnd.snr_index, PURPOSE_INDEX), (int)(t >> 2));
        const uint32_t draw = (t & 3) == 0 ? r.x : (t & 3) == 1 ? r.y : (t & 3) == 2 ? r.z : r.w;
        const int32_t idx = (int32_t)__umulhi(draw, (uint32_t)pool);
        bool fresh = true;
        if (distinct)
            for (int i = 0; i < have; ++i) fresh = fresh && row[i] != idx;
        if (fresh) row[have++] = idx;
    }
}

// ---- ML soft bits ----------------------------------------------------------------------------------------------------------------
struct LlrParams {
    const float2* symbols; const float2* Hp[2]; const int32_t* chan_index; float2* noise; float* llr[2];
    const int32_t* P;
    float noise_power;
    int Npk, pool, Nr, N, uses;
    sbc_link_random rnd;
};

// the lanes of one wave exchange data through LDS: order the wave's own LDS writes before its later reads
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float wave_min(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int S>
__global__ __launch_bounds__(LINK_THREADS) void link_llr_kernel(LlrParams p) {
    constexpr int NCAND = 1 << (2 * S);
    constexpr int NJ = NCAND > 64 ? NCAND / 64 : 1;        // candidates of a lane: they differ in the last stream's symbol (S = 4)
    constexpr int SL = NJ > 1 ? S - 1 : S;                 // streams whose symbol the lane index holds
    __shared__ float2 sm_hp[LINK_WAVES][LINK_MAX_NR * S];
    __shared__ float2 sm_y[LINK_WAVES][LINK_MAX_NR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t item = (int64_t)blockIdx.x * LINK_WAVES + wave;
    if (item >= (int64_t)p.Npk * p.uses) return;           // (no workgroup barrier below: a wave is on its own)
    const int pk = (int)(item / p.uses), use = (int)(item % p.uses);
    const int Nr = p.Nr;
    float2* hp = sm_hp[wave];
    float2* y = sm_y[wave];
    const int idx = p.chan_index[item];
    const bool bad = idx < 0 || idx >= p.pool;
    const float npow = p.noise_power;
    const bool live = lane < NCAND;
    int sym[S];
#pragma unroll
    for (int s = 0; s < S; ++s) sym[s] = (lane >> (2 * s)) & 3;

    for (int csi = 0; csi < 2; ++csi) {
        float out[2 * S];
        if (bad) {
#pragma unroll
            for (int q = 0; q < 2 * S; ++q) out[q] = NAN;
        } else {
            const float2* H = p.Hp[csi] + (size_t)idx * Nr * S;
            for (int e = lane; e < Nr * S; e += 64) hp[e] = H[e];
            wave_sync();
            if (csi == 0) {
                // y = Hp_ideal x + sqrt(noise_power) w, streams in ascending order, then the noise
                const float2* x = p.symbols + (size_t)item * S;
                const float amp = sqrtf(p.noise_power);
                if (lane < Nr) {
                    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const float2 h = hp[lane * S + s], xs = x[s];
                        acc.x += h.x * xs.x - h.y * xs.y;
                        acc.y += h.x * xs.y + h.y * xs.x;
                    }
                    float2 w;
                    if (p.rnd.flags & SBC_LINK_DEVICE_RANDOM) {
                        w = complex_normal(p.rnd.seed, p.rnd.packet0 + pk, stream_step(p.rnd.snr_index, PURPOSE_NOISE), use * Nr + lane);
                        if (p.noise) p.noise[(size_t)item * Nr + lane] = w;
                    } else {
                        w = p.noise[(size_t)item * Nr + lane];
                    }
                    y[lane] = make_float2(acc.x + amp * w.x, acc.y + amp * w.y);
                }
                wave_sync();
            }
            // metrics of the lane's candidates
            float met[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) met[j] = 0.f;
            float2 t[S];
#pragma unroll
            for (int s = 0; s < S; ++s) t[s] = qpsk(sym[s]);
            for (int r = 0; r < Nr; ++r) {
                float2 d = y[r];
#pragma unroll
                for (int s = 0; s < SL; ++s) {
                    const float2 h = hp[r * S + s];
                    d.x -= h.x * t[s].x - h.y * t[s].y;
                    d.y -= h.x * t[s].y + h.y * t[s].x;
                }
                if (NJ > 1) {
                    const float2 h = hp[r * S + S - 1];
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const float2 tj = qpsk(j);
                        const float dx = d.x - (h.x * tj.x - h.y * tj.y), dy = d.y - (h.x * tj.y + h.y * tj.x);
                        met[j] += dx * dx + dy * dy;
                    }
                } else {
                    met[0] += d.x * d.x + d.y * d.y;
                }
            }
            // per (stream, bit): log-sum-exp of -metric / noise_power over the candidates with bit = 0 minus the same with bit = 1
#pragma unroll
            for (int s = 0; s < S; ++s) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    float lse[2];
#pragma unroll
                    for (int v = 0; v < 2; ++v) {
                        float lo = INFINITY;
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            const int sv = (NJ > 1 && s == S - 1) ? j : sym[s];
                            if (live && ((sv >> (1 - b)) & 1) == v) lo = fminf(lo, met[j]);
                        }
                        lo = wave_min(lo);
                        float sum = 0.f;
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            const int sv = (NJ > 1 && s == S - 1) ? j : sym[s];
                            if (live && ((sv >> (1 - b)) & 1) == v) sum += expf((lo - met[j]) / npow);
                        }
                        sum = wave_sum(sum);
                        lse[v] = -lo / npow + logf(sum);
                    }
                    out[2 * s + b] = lse[0] - lse[1];
                }
            }
            wave_sync();               // every lane is done with hp before the next channel set replaces it
        }
        // flat index bit + 2 stream + 2S use; deinterleaved position P[flat]; the padded tail is written by the packet's first use
        float* dst = p.llr[csi] + (size_t)pk * p.N;
        float mine = 0.f;
#pragma unroll
        for (int q = 0; q < 2 * S; ++q) mine = lane == q ? out[q] : mine;
        if (!(p.rnd.flags & SBC_LINK_NO_CLIP) && fabsf(mine) >= LINK_CLIP) mine = copysignf(LINK_CLIP, mine);
        if (lane < 2 * S) dst[p.P[use * 2 * S + lane]] = mine;
        if (use == 0)
            for (int q = p.uses * 2 * S + lane; q < p.N; q += 64) dst[p.P[q]] = 0.f;
    }
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------
struct DecodeParams {
    const float* llr; float* soft; float* totals; int32_t* iters;
    const uint16_t* cptr; const uint16_t* vptr; const uint16_t* evar; const uint16_t* vedge;
    int Npk, N, M, K, E, max_iters, early_stop, ncw;
};

// a [+] b = sign a sign b min(|a|, |b|) + log1p(e^-|a+b|) - log1p(e^-|a-b|): exact, and finite where fp32 tanh / atanh is not
__device__ __forceinline__ float boxplus(float a, float b) {
    const float mag = fminf(fabsf(a), fabsf(b));
    const float sm = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, mag) ^ ((__builtin_bit_cast(uint32_t, a) ^ __builtin_bit_cast(uint32_t, b)) & 0x80000000u));
    return sm + log1pf(expf(-fabsf(a + b))) - log1pf(expf(-fabsf(a - b)));
}

__global__ __launch_bounds__(LINK_THREADS) void link_decode_kernel(DecodeParams p) {
    extern __shared__ float dec_sm[];
    const int tid = threadIdx.x, ncw = p.ncw, N = p.N, M = p.M, E = p.E;
    float* msg = dec_sm;                                   // [ncw][E]
    float* tot = msg + (size_t)ncw * E;                    // [ncw][N]
    float* ch = tot + (size_t)ncw * N;                     // [ncw][N]
    int* state = reinterpret_cast<int*>(ch + (size_t)ncw * N);      // done[8], fail[8], iters[8], all_done
    uint16_t* cptr = reinterpret_cast<uint16_t*>(state + 32);       // [M + 1]
    uint16_t* vptr = cptr + (M + 2);                                // [N + 1]
    uint16_t* evar = vptr + (N + 2);                                // [E]
    uint16_t* vedge = evar + E;                                     // [E]
    int* done = state, *fail = state + 8, *its = state + 16, *all_done = state + 24;
    const int first = blockIdx.x * ncw;

    for (int i = tid; i <= M; i += LINK_THREADS) cptr[i] = p.cptr[i];
    for (int i = tid; i <= N; i += LINK_THREADS) vptr[i] = p.vptr[i];
    for (int i = tid; i < E; i += LINK_THREADS) { evar[i] = p.evar[i]; vedge[i] = p.vedge[i]; }
    if (tid < LINK_MAX_CW) {
        done[tid] = !(tid < ncw && first + tid < p.Npk);
        fail[tid] = 0;
        its[tid] = 0;
    }
    if (tid == 0) *all_done = 0;
    for (int i = tid; i < ncw * N; i += LINK_THREADS) {
        const int c = i / N, v = i % N;
        const float l = first + c < p.Npk ? p.llr[(size_t)(first + c) * N + v] : 0.f;
        ch[i] = l;
        tot[i] = l;
    }
    __syncthreads();
    for (int i = tid; i < ncw * E; i += LINK_THREADS) {
        const int c = i / E, e = i % E;
        msg[i] = ch[c * N + evar[e]];
    }
    __syncthreads();

    for (int it = 0; it < p.max_iters && !*all_done; ++it) {
        // checks: extrinsic [+] of the other edges' messages, forward / backward over the check's edges, in place
        for (int i = tid; i < ncw * M; i += LINK_THREADS) {
            const int c = i / M, m = i % M;
            if (done[c]) continue;
            const int base = cptr[m], d = cptr[m + 1] - base;
            float* mm = msg + (size_t)c * E + base;
            float in[LINK_MAX_DC], f[LINK_MAX_DC], b[LINK_MAX_DC];
#pragma unroll
            for (int k = 0; k < LINK_MAX_DC; ++k) in[k] = k < d ? mm[k] : INFINITY;
            f[0] = in[0];
#pragma unroll
            for (int k = 1; k < LINK_MAX_DC; ++k) f[k] = k < d ? boxplus(f[k - 1], in[k]) : f[k - 1];
            b[LINK_MAX_DC - 1] = in[LINK_MAX_DC - 1];
#pragma unroll
            for (int k = LINK_MAX_DC - 2; k >= 0; --k) b[k] = k + 1 < d ? boxplus(b[k + 1], in[k]) : in[k];
#pragma unroll
            for (int k = 0; k < LINK_MAX_DC; ++k) {
                if (k < d) {
                    float o;
                    if (k == 0) o = b[1];
                    else if (k == d - 1) o = f[k - 1];
                    else o = boxplus(f[k - 1], b[k + 1 < LINK_MAX_DC ? k + 1 : k]);
                    mm[k] = o;
                }
            }
        }
        __syncthreads();
        // variables: total = channel + every check's message (ascending check), then the extrinsic message of each edge
        for (int i = tid; i < ncw * N; i += LINK_THREADS) {
            const int c = i / N, v = i % N;
            if (done[c]) continue;
            float* mm = msg + (size_t)c * E;
            const int e0 = vptr[v], e1 = vptr[v + 1];
            float t = ch[i];
            for (int q = e0; q < e1; ++q) t += mm[vedge[q]];
            tot[i] = t;
            for (int q = e0; q < e1; ++q) {
                const int e = vedge[q];
                mm[e] = t - mm[e];
            }
        }
        __syncthreads();
        // parity of the hard decisions (total < 0 -> 1)
        if (p.early_stop) {
            for (int i = tid; i < ncw * M; i += LINK_THREADS) {
                const int c = i / M, m = i % M;
                if (done[c]) continue;
                const float* tt = tot + (size_t)c * N;
                int x = 0;
                for (int q = cptr[m]; q < cptr[m + 1]; ++q) x ^= tt[evar[q]] < 0.f;
                if (x) fail[c] = 1;
            }
            __syncthreads();
        }
        if (tid == 0) {
            int all = 1;
            for (int c = 0; c < LINK_MAX_CW; ++c) {
                if (!done[c]) {
                    its[c] = it + 1;
                    if (p.early_stop && !fail[c]) done[c] = 1;
                }
                fail[c] = 0;
                all &= done[c];
            }
            *all_done = all;
        }
        __syncthreads();
    }

    for (int i = tid; i < ncw * N; i += LINK_THREADS) {
        const int c = i / N, v = i % N;
        if (first + c >= p.Npk) continue;
        const float t = tot[i];
        if (v < p.K) p.soft[(size_t)(first + c) * p.K + v] = t;
        if (p.totals) p.totals[(size_t)(first + c) * N + v] = t;
    }
    if (p.iters && tid < ncw && first + tid < p.Npk) p.iters[first + tid] = its[tid];
}

// ---- bit and block errors --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LINK_THREADS) void link_errors_kernel(const float* soft, const uint8_t* payload, int Npk, int K, float* ber, float* bler) {
    const int lane = threadIdx.x & 63, pk = blockIdx.x * LINK_WAVES + (threadIdx.x >> 6);
    if (pk >= Npk) return;
    int wrong = 0;
    for (int k = lane; k < K; k += 64) {
        const float s = soft[(size_t)pk * K + k];
        const int bit = payload[(size_t)pk * K + k];
        // payload_hat = (sign(-s) + 1) / 2: 1 for s < 0, 0 for s > 0, 0.5 (an error either way) for s = 0; NaN is an error too
        wrong += !((s > 0.f && bit == 0) || (s < 0.f && bit == 1));
    }
    for (int o = 32; o > 0; o >>= 1) wrong += __shfl_xor(wrong, o);
    if (lane == 0) {
        ber[pk] = (float)wrong / (float)K;
        bler[pk] = wrong > 0 ? 1.f : 0.f;
    }
}

}  // namespace
}  // namespace sbc

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct sbc_link_code {
    sbc::LinkTables t;
    int device = 0;
    uint32_t* gen = nullptr;
    int32_t* P = nullptr;
    uint16_t* cptr = nullptr, *vptr = nullptr, *evar = nullptr, *vedge = nullptr;
    int ncw = 1;                // codewords of a decoder workgroup
    size_t dec_lds = 0;
    std::mutex mu;              // the workspace of sbc_link_simulate
    void* ws = nullptr;
    size_t ws_bytes = 0;
};

namespace sbc {
namespace {

size_t decode_lds_bytes(const LinkTables& t, int ncw) {
    return ((size_t)ncw * (t.E + 2 * t.N) + 32) * 4 + ((size_t)(t.M + 2) + (t.N + 2) + 2 * (size_t)t.E) * 2;
}

int check_code(const sbc_link_code* c, const char* who) {
    SBC_REQUIRE(c, "%s: NULL code handle", who);
    int dev = 0;
    SBC_CHECK_HIP(hipGetDevice(&dev));
    SBC_REQUIRE(dev == c->device, "%s: the code was created on device %d, the current device is %d", who, c->device, dev);
    return SBC_OK;
}

int check_streams(const char* who, int S, int N) {
    if (S != 2 && S != 4) {
        set_error("%s: S = %d streams (supported: 2 and 4, QPSK; 4^S candidates are searched exhaustively)", who, S);
        return SBC_ERR_UNSUPPORTED;
    }
    SBC_REQUIRE(N >= 2 * S, "%s: a codeword of %d bits does not fill one channel use of %d QPSK streams", who, N, S);
    return SBC_OK;
}

int encode_launch(sbc_link_code* c, const sbc_link_encode_desc& d, hipStream_t stream) {
    const LinkTables& t = c->t;
    EncodeParams p;
    p.payload = (uint8_t*)d.payload; p.codeword = (uint8_t*)d.codeword; p.symbols = (float2*)d.symbols;
    p.gen = c->gen; p.P = c->P;
    p.K = t.K; p.M = t.M; p.N = t.N; p.Kw = t.Kw; p.nsym = t.N / (2 * d.S) * d.S;
    p.rnd = d.rnd;
    const size_t lds = (size_t)t.Kw * 4 + (size_t)t.N;
    hipLaunchKernelGGL(link_encode_kernel, dim3((unsigned)d.Npk), dim3(LINK_THREADS), lds, stream, p);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int llr_launch(sbc_link_code* c, const sbc_link_llr_desc& d, hipStream_t stream) {
    const LinkTables& t = c->t;
    LlrParams p;
    p.symbols = (const float2*)d.symbols; p.Hp[0] = (const float2*)d.Hp_ideal; p.Hp[1] = (const float2*)d.Hp_est;
    p.chan_index = (const int32_t*)d.chan_index; p.noise = (float2*)d.noise; p.llr[0] = (float*)d.llr_ideal; p.llr[1] = (float*)d.llr_est;
    p.P = c->P; p.noise_power = d.noise_power;
    p.Npk = d.Npk; p.pool = d.pool; p.Nr = d.Nr; p.N = t.N; p.uses = t.N / (2 * d.S);
    p.rnd = d.rnd;
    if (d.rnd.flags & SBC_LINK_DEVICE_RANDOM) {
        hipLaunchKernelGGL(link_index_kernel, dim3((unsigned)((d.Npk + LINK_THREADS - 1) / LINK_THREADS)), dim3(LINK_THREADS), 0, stream,
                           (int32_t*)d.chan_index, d.Npk, p.uses, d.pool, d.rnd);
        SBC_CHECK_HIP(hipGetLastError());
    }
    const int64_t items = (int64_t)d.Npk * p.uses;
    const dim3 grid((unsigned)((items + LINK_WAVES - 1) / LINK_WAVES));
    if (d.S == 2) hipLaunchKernelGGL(link_llr_kernel<2>, grid, dim3(LINK_THREADS), 0, stream, p);
    else hipLaunchKernelGGL(link_llr_kernel<4>, grid, dim3(LINK_THREADS), 0, stream, p);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int decode_launch(sbc_link_code* c, const float* llr, int Npk, int max_iters, int early_stop, float* soft, float* totals, int32_t* iters,
                  hipStream_t stream) {
    const LinkTables& t = c->t;
    DecodeParams p;
    p.llr = llr; p.soft = soft; p.totals = totals; p.iters = iters;
    p.cptr = c->cptr; p.vptr = c->vptr; p.evar = c->evar; p.vedge = c->vedge;
    p.Npk = Npk; p.N = t.N; p.M = t.M; p.K = t.K; p.E = t.E; p.max_iters = max_iters; p.early_stop = early_stop; p.ncw = c->ncw;
    int rc = ensure_dyn_lds((const void*)link_decode_kernel, c->dec_lds);
    if (rc) return rc;
    hipLaunchKernelGGL(link_decode_kernel, dim3((unsigned)((Npk + c->ncw - 1) / c->ncw)), dim3(LINK_THREADS), c->dec_lds, stream, p);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int errors_launch(sbc_link_code* c, const float* soft, const void* payload, int Npk, float* ber, float* bler, hipStream_t stream) {
    hipLaunchKernelGGL(link_errors_kernel, dim3((unsigned)((Npk + LINK_WAVES - 1) / LINK_WAVES)), dim3(LINK_THREADS), 0, stream, soft,
                       (const uint8_t*)payload, Npk, c->t.K, ber, bler);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

int check_random(const char* who, const sbc_link_random& r) {
    SBC_REQUIRE((r.flags & ~(SBC_LINK_DEVICE_RANDOM | SBC_LINK_NO_CLIP)) == 0, "%s: unknown flag bits 0x%x", who, r.flags);
    SBC_REQUIRE(r.snr_index >= 0 && r.snr_index < (1 << 28) && r.packet0 >= 0, "%s: need 0 <= snr_index < 2^28 and packet0 >= 0", who);
    return SBC_OK;
}

int check_llr_geometry(const char* who, const sbc_link_code* c, int S, int Nr, int pool, int Npk, float noise_power) {
    int rc = check_streams(who, S, c->t.N);
    if (rc) return rc;
    if (Nr < 1 || Nr > LINK_MAX_NR) {
        set_error("%s: Nr = %d receive antennas (supported: 1 .. %d)", who, Nr, LINK_MAX_NR);
        return SBC_ERR_UNSUPPORTED;
    }
    SBC_REQUIRE(pool >= 1 && Npk >= 0, "%s: need a pool of at least one channel and Npk >= 0 (got pool=%d Npk=%d)", who, pool, Npk);
    SBC_REQUIRE(noise_power > 0.f && isfinite(noise_power), "%s: noise_power must be finite and > 0", who);
    return SBC_OK;
}

template <class T>
int upload(T** dst, const std::vector<T>& src) {
    SBC_CHECK_HIP(hipMalloc((void**)dst, src.size() * sizeof(T)));
    SBC_CHECK_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return SBC_OK;
}

}  // namespace
}  // namespace sbc

extern "C" void sbc_link_code_destroy(sbc_link_code* c) {
    if (!c) return;
    for (void* q : {(void*)c->gen, (void*)c->P, (void*)c->cptr, (void*)c->vptr, (void*)c->evar, (void*)c->vedge, c->ws})
        if (q) (void)hipFree(q);
    delete c;
}

extern "C" int sbc_link_code_create(const sbc_link_code_desc* d, sbc_link_code** out) {
    using namespace sbc;
    SBC_REQUIRE(d && out, "sbc_link_code_create: NULL descriptor or output");
    *out = nullptr;
    sbc_link_code* c = new (std::nothrow) sbc_link_code;
    SBC_REQUIRE(c, "sbc_link_code_create: out of host memory");
    std::string why;
    const int bad = build_link_tables(d->base, d->rows, d->cols, d->Z, d->interleaver, c->t, why);
    if (bad) {
        set_error("sbc_link_code_create: %s (rows=%d cols=%d Z=%d)", why.c_str(), d->rows, d->cols, d->Z);
        delete c;
        return bad == 1 ? SBC_ERR_INVALID : SBC_ERR_UNSUPPORTED;
    }
    c->ncw = 0;
    for (int n = LINK_MAX_CW; n >= 1 && !c->ncw; --n)
        if (decode_lds_bytes(c->t, n) <= LINK_LDS_BUDGET) c->ncw = n;
    if (!c->ncw) {
        set_error("sbc_link_code_create: one codeword (N=%d, %d edges) does not fit the decoder's %zu bytes of LDS", c->t.N, c->t.E, LINK_LDS_BUDGET);
        delete c;
        return SBC_ERR_UNSUPPORTED;
    }
    c->dec_lds = decode_lds_bytes(c->t, c->ncw);
    int rc = SBC_OK;
    if (hipGetDevice(&c->device) != hipSuccess) { set_error("sbc_link_code_create: no HIP device"); rc = SBC_ERR_HIP; }
    if (!rc) rc = upload(&c->gen, c->t.gen);
    if (!rc) rc = upload(&c->P, c->t.P);
    if (!rc) rc = upload(&c->cptr, c->t.cptr);
    if (!rc) rc = upload(&c->vptr, c->t.vptr);
    if (!rc) rc = upload(&c->evar, c->t.evar);
    if (!rc) rc = upload(&c->vedge, c->t.vedge);
    if (rc) { sbc_link_code_destroy(c); return rc; }
    *out = c;
    return SBC_OK;
}

extern "C" int sbc_link_encode(sbc_link_code* c, const sbc_link_encode_desc* d, void* stream) {
    using namespace sbc;
    int rc = check_code(c, "sbc_link_encode");
    if (rc) return rc;
    SBC_REQUIRE(d, "sbc_link_encode: NULL descriptor");
    if ((rc = check_streams("sbc_link_encode", d->S, c->t.N))) return rc;
    if ((rc = check_random("sbc_link_encode", d->rnd))) return rc;
    SBC_REQUIRE(d->Npk >= 0 && d->payload && d->symbols, "sbc_link_encode: need Npk >= 0, payload and symbols");
    if (d->Npk == 0) return SBC_OK;
    return encode_launch(c, *d, (hipStream_t)stream);
}

extern "C" int sbc_link_llr(sbc_link_code* c, const sbc_link_llr_desc* d, void* stream) {
    using namespace sbc;
    int rc = check_code(c, "sbc_link_llr");
    if (rc) return rc;
    SBC_REQUIRE(d, "sbc_link_llr: NULL descriptor");
    if ((rc = check_llr_geometry("sbc_link_llr", c, d->S, d->Nr, d->pool, d->Npk, d->noise_power))) return rc;
    if ((rc = check_random("sbc_link_llr", d->rnd))) return rc;
    SBC_REQUIRE(d->symbols && d->Hp_ideal && d->Hp_est && d->chan_index && d->llr_ideal && d->llr_est,
                "sbc_link_llr: NULL symbols, Hp_ideal, Hp_est, chan_index, llr_ideal or llr_est");
    SBC_REQUIRE(d->noise || (d->rnd.flags & SBC_LINK_DEVICE_RANDOM), "sbc_link_llr: noise is needed without SBC_LINK_DEVICE_RANDOM");
    if (d->Npk == 0) return SBC_OK;
    return llr_launch(c, *d, (hipStream_t)stream);
}

extern "C" int sbc_link_decode(sbc_link_code* c, const float* llr, int32_t Npk, int32_t max_iters, int32_t early_stop, float* soft, float* totals,
                               int32_t* iters, void* stream) {
    using namespace sbc;
    int rc = check_code(c, "sbc_link_decode");
    if (rc) return rc;
    SBC_REQUIRE(llr && soft && Npk >= 0 && max_iters >= 1, "sbc_link_decode: need llr, soft, Npk >= 0 and max_iters >= 1 (got Npk=%d max_iters=%d)",
                Npk, max_iters);
    if (Npk == 0) return SBC_OK;
    return decode_launch(c, llr, Npk, max_iters, early_stop, soft, totals, iters, (hipStream_t)stream);
}

extern "C" int sbc_link_errors(sbc_link_code* c, const float* soft, const void* payload, int32_t Npk, float* ber, float* bler, void* stream) {
    using namespace sbc;
    int rc = check_code(c, "sbc_link_errors");
    if (rc) return rc;
    SBC_REQUIRE(soft && payload && ber && bler && Npk >= 0, "sbc_link_errors: need soft, payload, ber, bler and Npk >= 0");
    if (Npk == 0) return SBC_OK;
    return errors_launch(c, soft, payload, Npk, ber, bler, (hipStream_t)stream);
}

extern "C" int sbc_link_simulate(sbc_link_code* c, const sbc_link_sim_desc* d, void* stream) {
    using namespace sbc;
    int rc = check_code(c, "sbc_link_simulate");
    if (rc) return rc;
    SBC_REQUIRE(d, "sbc_link_simulate: NULL descriptor");
    if ((rc = check_llr_geometry("sbc_link_simulate", c, d->S, d->Nr, d->pool, d->Npk, d->noise_power))) return rc;
    if ((rc = check_random("sbc_link_simulate", d->rnd))) return rc;
    SBC_REQUIRE(!(d->rnd.flags & SBC_LINK_NO_CLIP), "sbc_link_simulate: the decoder's soft bits are clipped");
    SBC_REQUIRE(d->Hp_ideal && d->Hp_est && d->payload && d->chan_index && d->ber_ideal && d->bler_ideal && d->ber_est && d->bler_est,
                "sbc_link_simulate: NULL Hp_ideal, Hp_est, payload, chan_index or result array");
    SBC_REQUIRE(d->noise || (d->rnd.flags & SBC_LINK_DEVICE_RANDOM), "sbc_link_simulate: noise is needed without SBC_LINK_DEVICE_RANDOM");
    SBC_REQUIRE(d->max_iters >= 1, "sbc_link_simulate: max_iters must be >= 1 (got %d)", d->max_iters);
    if (d->Npk == 0) return SBC_OK;
    const LinkTables& t = c->t;
    const size_t nsym = (size_t)(t.N / (2 * d->S)) * d->S;
    const size_t sym_b = (size_t)d->Npk * nsym * sizeof(float2), llr_b = (size_t)d->Npk * t.N * 4, soft_b = (size_t)d->Npk * t.K * 4;
    const size_t need = sym_b + 2 * llr_b + soft_b;
    std::lock_guard<std::mutex> lock(c->mu);
    if (need > c->ws_bytes) {
        // a larger chunk than ever before: earlier launches may still use the old workspace
        SBC_CHECK_HIP(hipDeviceSynchronize());
        if (c->ws) SBC_CHECK_HIP(hipFree(c->ws));
        c->ws = nullptr; c->ws_bytes = 0;
        SBC_CHECK_HIP(hipMalloc(&c->ws, need));
        c->ws_bytes = need;
    }
    char* w = (char*)c->ws;
    float2* sym = (float2*)w;
    float* llr_i = (float*)(w + sym_b), *llr_e = (float*)(w + sym_b + llr_b), *soft = (float*)(w + sym_b + 2 * llr_b);
    hipStream_t s = (hipStream_t)stream;
    sbc_link_encode_desc e = {d->payload, nullptr, sym, d->Npk, d->S, d->rnd};
    if ((rc = encode_launch(c, e, s))) return rc;
    sbc_link_llr_desc l = {sym, d->Hp_ideal, d->Hp_est, d->chan_index, d->noise, llr_i, llr_e, d->noise_power, d->Npk, d->pool, d->Nr, d->S, d->rnd};
    if ((rc = llr_launch(c, l, s))) return rc;
    if ((rc = decode_launch(c, llr_i, d->Npk, d->max_iters, 1, soft, nullptr, (int32_t*)d->iters_ideal, s))) return rc;
    if ((rc = errors_launch(c, soft, d->payload, d->Npk, (float*)d->ber_ideal, (float*)d->bler_ideal, s))) return rc;
    if ((rc = decode_launch(c, llr_e, d->Npk, d->max_iters, 1, soft, nullptr, (int32_t*)d->iters_est, s))) return rc;
    return errors_launch(c, soft, d->payload, d->Npk, (float*)d->ber_est, (float*)d->bler_est, s);
}
