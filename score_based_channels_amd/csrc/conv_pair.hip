// One RCU block of the score network in ONE launch (SBC_OP_CONV_PAIR):
//       out = x + conv2(ELU(conv1(ELU(x))))        ncsnv2/models/layers.py:126-134 (n_stages = 2, 3x3, no bias)
// for 32-channel NHWC fp32 tensors.  The unfused pair streams five tensors through HBM (x; t out, t in; x again, out) and
// both launches sit at 0.6 of the achievable HBM rate; here the intermediate t = conv1(ELU(x)) never leaves the chip.
//
// Persistent workgroups (two per CU, 256 threads) walk tiles of R output rows of one sample:
//   1. the tile's R + 4 input rows (one contiguous run of NHWC memory) arrive by LDS-DMA (global_load_lds_dwordx4) -- the
//      request for tile k + 1 is issued as soon as tile k's raw copy has been converted, so it flies during both K loops;
//   2. convert: raw fp32 -> ELU -> x act_scale -> two fp16 terms (conv_mode f16x2; one rounded term for f16w) -> operand
//      planes [term][k-group of 8 channels][row][W + 2 pixels][8 halves]: zero columns left and right stand in for the
//      padding, and 16 consecutive pixels of a row are 16 consecutive 16-byte slots (conflict-free ds_read_b128);
//   3. conv1 as a direct implicit GEMM on v_mfma_f32_16x16x32_f16: D[16 couts][16 pixels] += W[16 couts][32 cin] X[32 cin][16
//      pixels] per tap and term pair -- (h,l) (l,h) (h,h), the split-fp16 products of conv_x3.hip -- for the R + 2 rows conv2
//      needs; ALL filter fragments of both convolutions (2 x 9 taps x 2 terms x 4 registers for this wave's 16 output
//      channels) stay in registers for the life of the workgroup, so the K loop is LDS reads and matrix instructions only;
//   4. the accumulators go x descale1 -> ELU -> x act_scale -> split -> a second set of planes (rows outside the sample: zeros);
//   5. conv2 the same way on the R output rows; its epilogue adds the residual x (re-read from L2, fp32) and stores float4s.
// A 16 x 16 unit is one image row (W = 16), two rows (W = 8) or part of a row (W >= 32); wave w owns output-channel half w & 1
// and every second unit, so with R = 8 at W = 16 the four waves run 5 + 4 units each: no idle wave in either convolution.
#include <type_traits>
#include "conv_pair.h"

namespace sbc {

typedef float f32x4v __attribute__((ext_vector_type(4)));

// NW waves per workgroup: 4 (two workgroups per CU) for images 8 / 16 pixels wide; 8 (one workgroup per CU, its LDS) for 64-pixel
// rows, where wave pair `sub` owns column block `sub` of every row of the tile.
// C channels (input = intermediate = output): 32, or 64 in the fp16-weight mode (one term: 2 x 9 taps x 2 k-halves x 4 registers
// per wave -- the same 144 as 32 channels with two terms); a wave owns 16 output channels (C / 16 "quarters" hf) and NSUB = NW /
// (C / 16) unit groups.
template <int W, int R, int MODE, int NW = 4, int C = 32>
__global__ __launch_bounds__(64 * NW, 2) void conv_pair_kernel(PairParams p) {
    constexpr int NTH = 64 * NW, NHF = C / 16, NSUB = NW / NHF;
    constexpr int KGS = C / 8, KH = C / 32, C4 = C / 4;   // 8-channel plane groups, 32-channel halves of the contraction, channel quads
    static_assert(C == 32 || (C == 64 && MODE == 1), "64 channels: fp16-weight mode only (filter fragments must fit in registers)");
    constexpr int NT = MODE == 2 ? 2 : 1;            // fp16 terms per operand
    constexpr int RI = R + 4, RM = R + 2;             // staged input rows, intermediate rows
    constexpr int WP = W + 2;                         // row of a plane: zero pixel, W pixels, zero pixel
    constexpr int XPS = (RI * WP * 16 + 255) / 256 * 256;     // bytes of one k-group plane (multiple of the 256-byte bank row)
    constexpr int MPS = (RM * WP * 16 + 255) / 256 * 256;
    constexpr int RAW_BYTES = RI * W * C * 4;
    constexpr int X_OFF = RAW_BYTES, M_OFF = X_OFF + NT * KGS * XPS;
    constexpr int NQ = RI * W * C4;                   // 16-byte chunks of the raw tile
    static_assert(NQ % NTH == 0, "raw tile must divide over the workgroup's threads");
    constexpr int CB = W >= 16 ? W / 16 : 1;          // units per image row (W >= 16)
    constexpr int RPU = W >= 16 ? 1 : 16 / W;         // image rows per unit (W < 16)
    constexpr bool COLS = CB > 1;                     // wide rows: wave pair `sub` owns column block `sub`, unit i = row i
    static_assert(!COLS || CB == NSUB, "one wave pair per column block");
    constexpr int NU1T = COLS ? RM : RM * W / 16, NU2T = COLS ? R : R * W / 16;   // units per output-channel half (and column block)
    constexpr int USTEP = COLS ? 1 : NSUB;            // unit index step between a wave's consecutive units
    constexpr int NU1 = (NU1T + USTEP - 1) / USTEP, NU2 = (NU2T + USTEP - 1) / USTEP;  // per wave
    static_assert(RM % RPU == 0 && R % RPU == 0, "units must not straddle the tile");
    extern __shared__ __attribute__((aligned(256))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hf = wave % NHF, sub = wave / NHF;      // 16-output-channel group; unit parity / column block of this wave
    const int kq = lane >> 4, c = lane & 15;          // k-group (8 input channels) / pixel of the unit
    const int H = p.H;
    // unit i of this wave: first plane row and slot column of its 16 pixels (this lane: pixel c), and the step to unit i + 1
    const int u0 = COLS ? 0 : sub;
    const int urow0 = u0 * RPU + (W >= 16 ? 0 : c / W);
    const int ucol = COLS ? sub * 16 + c : (W >= 16 ? c : c % W);
    constexpr int UROWS = USTEP * RPU;                 // image rows from a wave's unit i to its unit i + 1

    // ---- filter fragments of both convolutions, resident for the whole launch (A operand: lane = cout l & 15, k-group l >> 4)
    // (packed layout [tap][C/16 input groups g][C/32 output blocks nb][terms][64 lanes]: lane l' = cout % 32 + 32 * (cin group half))
    uint4 wf[2][9][KH][NT];
    {
        const int lsrc = (16 * (hf & 1) + c) + 32 * (kq & 1), nb = hf >> 1;
#pragma unroll
        for (int cv = 0; cv < 2; ++cv) {
            const uint4* w = cv == 0 ? p.w1 : p.w2;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int kh = 0; kh < KH; ++kh)
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        wf[cv][tap][kh][t] = w[(((tap * (C / 16) + 2 * kh + (kq >> 1)) * (C / 32) + nb) * NT + t) * 64 + lsrc];
        }
    }
    float scale1 = 1.f, descale1 = 1.f, scale2 = 1.f, descale2 = 1.f;
    // range tracking (tile.h): per tile, max |x| of what this lane converts for conv1 (ta) / writes as the intermediate (tb); the
    // wave-level verdicts accumulate in `rbits`
    unsigned rbits = 0;
    if constexpr (MODE == 2) {
        const float4 t1 = f16x2_trailer(reinterpret_cast<const float4*>(p.w1), 9 * (C / 16) * (C / 32) * NT);
        const float4 t2 = f16x2_trailer(reinterpret_cast<const float4*>(p.w2), 9 * (C / 16) * (C / 32) * NT);
        scale1 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t1.x)));
        scale2 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t2.x)));
        descale1 = t1.y; descale2 = t2.y;
        // the calibration found one of the two convolutions' inputs below 2^-4 (fourth trailer word): this kernel evaluates ELU as
        // exp(x) - 1 only (it has no registers for the accurate form of common.h) -- say so, the host re-runs the batch in bf16x3
        if (t1.w != 0.f || t2.w != 0.f) rbits |= 4u;
    }

    // ---- zero the padding columns of every plane once (nothing writes them afterwards)
    for (int i = tid; i < NT * KGS * RI * 2; i += NTH) {
        const int side = i & 1, row = (i >> 1) % RI, pl = (i >> 1) / RI;
        *reinterpret_cast<uint4*>(smem + X_OFF + pl * XPS + (row * WP + side * (W + 1)) * 16) = make_uint4(0, 0, 0, 0);
    }
    for (int i = tid; i < NT * KGS * RM * 2; i += NTH) {
        const int side = i & 1, row = (i >> 1) % RM, pl = (i >> 1) / RM;
        *reinterpret_cast<uint4*>(smem + M_OFF + pl * MPS + (row * WP + side * (W + 1)) * 16) = make_uint4(0, 0, 0, 0);
    }

    // ---- tile walk: XCD x (= blockIdx % 8) owns a contiguous run of tiles, its workgroups take consecutive tiles of it
    const int xcd = blockIdx.x & 7, jw = blockIdx.x >> 3;
    const int t_begin = xcd * p.tiles_per_xcd;
    const int t_end = min(t_begin + p.tiles_per_xcd, p.ntiles);
    auto issue_dma = [&](int tile) {
        const int n = tile / p.tiles_per_sample, r0 = (tile - n * p.tiles_per_sample) * R;
        const char* src = reinterpret_cast<const char*>(p.in) + ((size_t)(n * H + r0 - 2) * W * C) * 4;   // may point before the sample: masked
#pragma unroll
        for (int k = 0; k < NQ / NTH; ++k) {
            const int j = k * NW + wave;                                  // wave-instruction: chunks j * 64 .. + 63
            const int ri = (j * 64) / (W * C4);                           // its (single) tile row
            const int grow = r0 - 2 + ri;
            if (grow >= 0 && grow < H) {
                // by hand: hipcc puts an s_waitcnt vmcnt(0) in front of every __builtin_amdgcn_global_load_lds of this loop
                // (each piece would wait for the one before: six serialised HBM round trips per tile).  M0 = LDS byte address of
                // the wave's 1 KiB piece; lane l lands at M0 + 16 l.  hipcc does not count these requests: the waits are explicit.
                // (scalar base + 32-bit lane offset: per-lane 64-bit source pointers for six pieces would be hoisted and spilled)
                const char* sbase = src + (size_t)j * 1024;
                const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem + j * 1024;
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(lane * 16), "s"(dst), "s"(sbase) : "memory");
            }
        }
    };
    int tile = t_begin + jw;
    if (tile < t_end) issue_dma(tile);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // first tile (and the filter fragments) landed

    for (; tile < t_end; tile += p.wgs_per_xcd) {
        const int n = tile / p.tiles_per_sample, r0 = (tile - n * p.tiles_per_sample) * R;
        // (1) raw tile landed, for every wave (each wave waited for its own pieces before its previous epilogue / the loop)
        asm volatile("s_barrier" ::: "memory");
        // (2) convert raw -> operand planes of conv1
        float ta = 0.f, tb = 0.f;
#pragma unroll
        for (int k = 0; k < NQ / NTH; ++k) {
            const int q = k * NTH + tid;
            const int px = q / C4, c4 = q % C4;
            const int ri = px / W, col = px - ri * W;
            const int grow = r0 - 2 + ri;
            float4 v = *reinterpret_cast<const float4*>(smem + q * 16);
            if (grow < 0 || grow >= H) v = make_float4(0.f, 0.f, 0.f, 0.f);
            v = elu4(v);
            unsigned char* dst = smem + X_OFF + (c4 >> 1) * XPS + (ri * WP + col + 1) * 16 + (c4 & 1) * 8;
            if constexpr (MODE == 2) {
                StageScale ss{scale1, ta};
                scale_track(v, &ss);
                ta = ss.amax;
                uint2 h, l;
                split_f16x2(v, scale1, h, l);
                *reinterpret_cast<uint2*>(dst) = h;
                *reinterpret_cast<uint2*>(dst + KGS * XPS) = l;
            } else {
                f16x4 h;
                h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
                *reinterpret_cast<f16x4*>(dst) = h;
            }
        }
        if constexpr (MODE == 2) pair_range_tile(ta, scale1, rbits, p.calib);
        lds_barrier();
        // the raw copy is consumed: request the next tile of this workgroup; it flies during both K loops
        if (tile + p.wgs_per_xcd < t_end) issue_dma(tile + p.wgs_per_xcd);

        // one convolution over units `sub`, `sub + 2`, ...: acc[i] = D[16 couts of this wave][16 pixels of unit i]
        auto conv = [&](auto cvc, const int plane_off, const int PS, auto nuc, auto nutc, f32x4v* acc) {
            constexpr int CV = decltype(cvc)::value, NU = decltype(nuc)::value, NUT = decltype(nutc)::value;
            constexpr int DU = UROWS * WP * 16;                            // bytes from a wave's unit i to its unit i + 1
            // source pixel of tap (0, 0) of the wave's first unit = plane row urow0 (the row above the output row), slot column ucol (-1 + 1)
            const int ub0 = plane_off + kq * PS + (urow0 * WP + ucol) * 16;
            // flat walk over (tap, unit) steps; the X fragments of a step are requested D - 1 steps ahead of its MFMAs through a
            // ring of statically indexed registers (the scheduler would otherwise hoist every read of the loop and spill)
            constexpr int NS = 9 * KH * NU, D = NT == 2 ? 3 : 6;             // steps: (tap, k-half, unit)
            f16x8 ring[D][NT];
            auto ld = [&](int s) {                                          // s is a compile-time constant at every call
                const int tap = s / (KH * NU), kh = (s / NU) % KH, i = s % NU;
                const int off = i * DU + ((tap / 3) * WP + (tap % 3)) * 16 + kh * 4 * PS;
                if (NUT % USTEP == 0 || u0 + USTEP * i < NUT) {
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        ring[s % D][t] = *reinterpret_cast<const f16x8*>(smem + ub0 + (off + t * KGS * PS));
                }
            };
#pragma unroll
            for (int s = 0; s < D - 1; ++s) ld(s);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int tap = s / (KH * NU), kh = (s / NU) % KH, i = s % NU;
                if (s + D - 1 < NS) ld(s + D - 1);
                if (NUT % USTEP == 0 || u0 + USTEP * i < NUT) {
                    const f16x8 xh = ring[s % D][0];
                    const f16x8 wh = __builtin_bit_cast(f16x8, wf[CV][tap][kh][0]);
                    // the first matrix instruction of a unit takes a literal zero as its addend (no register zeroing per tile)
                    const f32x4v c0 = (tap == 0 && kh == 0) ? f32x4v{0.f, 0.f, 0.f, 0.f} : acc[i];
                    if constexpr (NT == 2) {
                        const f16x8 xl = ring[s % D][NT - 1];
                        const f16x8 wl = __builtin_bit_cast(f16x8, wf[CV][tap][kh][NT - 1]);
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, c0, 0, 0, 0);
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc[i], 0, 0, 0);
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc[i], 0, 0, 0);
                    } else {
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, c0, 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };

        // (3) conv1 on the RM intermediate rows -> ELU -> split -> intermediate planes
        {
            f32x4v acc[NU1];
            conv(std::integral_constant<int, 0>{}, X_OFF, XPS, std::integral_constant<int, NU1>{}, std::integral_constant<int, NU1T>{}, acc);
            const int cq = 4 * hf + kq;                                    // channel quad of this lane's four outputs
#pragma unroll
            for (int i = 0; i < NU1; ++i) {
                if (u0 + USTEP * i < NU1T) {
                    const int prow = urow0 + i * UROWS, pcol = ucol;
                    const int grow = r0 - 1 + prow;
                    float4 v = make_float4(acc[i][0] * descale1, acc[i][1] * descale1, acc[i][2] * descale1, acc[i][3] * descale1);
                    v = elu4(v);
                    if (grow < 0 || grow >= H) v = make_float4(0.f, 0.f, 0.f, 0.f);    // zero padding of conv2, not conv1 of padding
                    unsigned char* dst = smem + M_OFF + (cq >> 1) * MPS + (prow * WP + pcol + 1) * 16 + (cq & 1) * 8;
                    if constexpr (MODE == 2) {
                        StageScale ss{scale2, tb};
                        scale_track(v, &ss);
                        tb = ss.amax;
                        uint2 h, l;
                        split_f16x2(v, scale2, h, l);
                        *reinterpret_cast<uint2*>(dst) = h;
                        *reinterpret_cast<uint2*>(dst + KGS * MPS) = l;
                    } else {
                        f16x4 h;
                        h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
                        *reinterpret_cast<f16x4*>(dst) = h;
                    }
                }
            }
        }
        if constexpr (MODE == 2) pair_range_tile(tb, scale2, rbits, p.calib ? p.calib + 1 : nullptr);
        lds_barrier();
        // (4) conv2 on the R output rows, + residual, store
        {
            f32x4v acc[NU2];
            // the residual operand: requested before the K loop (an L2 hit: this workgroup's DMA fetched the same lines), used after it
            const int cq = 4 * hf + kq;
            float4 xr[NU2];
            constexpr int DO = UROWS * W * C;                               // elements from a wave's unit i to its unit i + 1
            const unsigned o0 = (unsigned)(((n * H + r0 + urow0) * W + ucol) * C + cq * 4);
#pragma unroll
            for (int i = 0; i < NU2; ++i)
                if (NU2T % USTEP == 0 || u0 + USTEP * i < NU2T) xr[i] = *reinterpret_cast<const float4*>(p.in + o0 + i * DO);
            conv(std::integral_constant<int, 1>{}, M_OFF, MPS, std::integral_constant<int, NU2>{}, std::integral_constant<int, NU2T>{}, acc);
            // everything this wave has in flight -- the residual, its pieces of the next tile's DMA -- has landed; the stores below
            // are never waited for explicitly (the same wait one iteration later covers them)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < NU2; ++i) {
                if (NU2T % USTEP == 0 || u0 + USTEP * i < NU2T) {
                    float4 y;
                    y.x = fmaf(acc[i][0], descale2, xr[i].x); y.y = fmaf(acc[i][1], descale2, xr[i].y);
                    y.z = fmaf(acc[i][2], descale2, xr[i].z); y.w = fmaf(acc[i][3], descale2, xr[i].w);
                    st_out(p.out + o0 + i * DO, y);
                }
            }
        }
        // the next iteration's barrier (1) orders conv2's reads of the intermediate planes before anything rewrites them
    }
    if constexpr (MODE == 2) {
        if (rbits && (threadIdx.x & 63) == 0) atomicOr(p.range_flag, rbits);
    }
}

// The same block as a three-stage pipeline over a RUN of tiles (W = 16, 32 channels; the row-ring kernel): one persistent workgroup
// per CU of twelve waves in three roles of four --
//   role 2 (conversion): keeps one item of LDS-DMA in flight and turns the raw copy of item i into rows of the operand planes X;
//   role 0 (conv1):      K loop of conv1 on the X rows of item i - 1, ELU, split -> rows of the intermediate planes M;
//   role 1 (conv2):      K loop of conv2 on the M rows of item i - 2, + x, store.
// The raw copy is double buffered and the planes hold three items (below), so ONE workgroup barrier per item is all the
// synchronisation there is; each role keeps only its own filter fragments (72 registers in f16x2), which is what lets three waves
// share a SIMD (168 registers each): two of them are always inside a K loop while the third does the vector-ALU work.
// A workgroup owns a contiguous run of tiles, so the rows two vertically adjacent tiles share are converted and convolved once.
// The operand planes are rings over rows:
//   X (conv1's input, fp16 terms): 24 rows in three slots of 8 + a 4-row copy of rows 20..23 in front of row 0;
//   M (the intermediate):          24 rows in three slots of 8 + a 2-row copy of rows 22, 23 in front of row 0.
// Item k of the run uses slot k % 3.  A TILE item (output rows r0 .. r0+7 of sample n) converts the EIGHT input rows r0+2 .. r0+9
// into its X slot, computes the EIGHT intermediate rows r0+1 .. r0+8 into its M slot (conv1 reads X rows slot-4 .. slot+7: the four
// rows before the slot are the previous item's last four) and the eight output rows (conv2 reads M rows slot-2 .. slot+7).  Where no
// previous tile of the same sample precedes it in the run -- the run's first tile, the first tile of every sample -- a PRE item
// comes first: it fills only the last four X rows (input rows r0-2 .. r0+1; zeros outside the image) and the last two M rows (r0-1,
// r0) of its slot and stores nothing.  A sample of 64 rows converts 68 rows and evaluates conv1 on 66 (a pipeline whose every tile
// brings its own halo: 96 and 80) and reads every input row from memory once (+ the PRE rows of a run that starts mid-sample).
// The copies in front of row 0 make every window contiguous: a value written to rows 20..23 (X) / 22, 23 (M) is written twice.
// Each role advances its own cursor over the run (scalar registers); the writer of iteration `it` (X slot it % 3, M slot
// (it - 1) % 3) never touches the rows the readers of that iteration use (X: slot (it - 1) % 3 and the four rows before it; M: slot
// (it - 2) % 3 and the two rows before it).
// Every output is the same sum in the same order as in conv_pair_kernel: identical bit for bit.
// Measurements behind the three roles, from the per-tile-halo form of this pipeline (removed; history: 54de329), 13 600 tiles: 180 us
// in the network against 203 for conv_pair_kernel (matrix pipe 0.57 busy against 0.51).  Two roles -- four matrix waves that keep
// both convolutions' fragments, four conversion waves -- were slower than conv_pair_kernel, 256 us against 244 back to back: ONE
// matrix wave per SIMD does not keep the matrix pipe fed.  The same holds inside the pipeline: matrix waves that own all 32 output
// channels of their units -- half the LDS reads, two waves per matrix role -- ran 279 us against 231.  Two items in flight (the
// conversion waves counting themselves in through LDS before they reuse a raw buffer) measured slower as well: the waiting waves
// take issue slots from the matrix waves.
template <int MODE>
__global__ __launch_bounds__(768, 3) void conv_pair_roll_kernel(PairParams p) {
    constexpr int W = 16, R = 8, C = 32, NW = 4, NTH = 64 * NW;
    constexpr int KGS = C / 8, C4 = C / 4;
    constexpr int NT = MODE == 2 ? 2 : 1;
    constexpr int WP = W + 2, ROWB = WP * 16;          // bytes of one plane row
    constexpr int RING = 24, XMIR = 4, MMIR = 2;       // ring rows; rows copied in front of row 0
    constexpr int XPS = ((RING + XMIR) * ROWB + 255) / 256 * 256;
    constexpr int MPS = ((RING + MMIR) * ROWB + 255) / 256 * 256;
    constexpr int RAW_BYTES = R * W * C * 4;
    constexpr int X_OFF = 2 * RAW_BYTES, M_OFF = X_OFF + NT * KGS * XPS;
    constexpr int NK = R * W * C4 / NTH;               // 16-byte chunks per thread and TILE item (4); a PRE item: the last two
    extern __shared__ __attribute__((aligned(256))) unsigned char smem[];

    const int role = __builtin_amdgcn_readfirstlane((int)threadIdx.x / NTH);      // 0: conv1 waves, 1: conv2 waves, 2: conversion waves
    const int tid = threadIdx.x - role * NTH, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hf = wave & 1, sub = wave >> 1;          // 16-output-channel half; row parity of this wave's units
    const int kq = lane >> 4, c = lane & 15;
    const int H = p.H;

    uint4 wf[9][NT];
    if (role < 2) {
        const int lsrc = (16 * hf + c) + 32 * (kq & 1);
        const uint4* w = role == 0 ? p.w1 : p.w2;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int t = 0; t < NT; ++t) wf[tap][t] = w[((tap * (C / 16) + (kq >> 1)) * NT + t) * 64 + lsrc];
    }
    float scale1 = 1.f, descale1 = 1.f, scale2 = 1.f, descale2 = 1.f;
    unsigned rbits = 0;
    if constexpr (MODE == 2) {
        const float4 t1 = f16x2_trailer(reinterpret_cast<const float4*>(p.w1), 9 * (C / 16) * (C / 32) * NT);
        const float4 t2 = f16x2_trailer(reinterpret_cast<const float4*>(p.w2), 9 * (C / 16) * (C / 32) * NT);
        scale1 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t1.x)));
        scale2 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t2.x)));
        descale1 = t1.y; descale2 = t2.y;
        if (t1.w != 0.f || t2.w != 0.f) rbits |= 4u;     // (conv_pair_kernel: the four-instruction ELU only)
    }

    // ---- zero the padding columns of every plane row once
    for (int i = threadIdx.x; i < NT * KGS * (RING + XMIR) * 2; i += 3 * NTH) {
        const int side = i & 1, row = (i >> 1) % (RING + XMIR), pl = (i >> 1) / (RING + XMIR);
        *reinterpret_cast<uint4*>(smem + X_OFF + pl * XPS + row * ROWB + side * (W + 1) * 16) = make_uint4(0, 0, 0, 0);
    }
    for (int i = threadIdx.x; i < NT * KGS * (RING + MMIR) * 2; i += 3 * NTH) {
        const int side = i & 1, row = (i >> 1) % (RING + MMIR), pl = (i >> 1) / (RING + MMIR);
        *reinterpret_cast<uint4*>(smem + M_OFF + pl * MPS + row * ROWB + side * (W + 1) * 16) = make_uint4(0, 0, 0, 0);
    }

    // ---- this workgroup's run: XCD x owns tiles [t_begin, t_end), its workgroups take equal contiguous pieces [a, b) of it
    const int xcd = blockIdx.x & 7, jw = blockIdx.x >> 3;
    const int t_begin = xcd * p.tiles_per_xcd;
    const int cnt = max(min(t_begin + p.tiles_per_xcd, p.ntiles) - t_begin, 0);
    const int a = t_begin + jw * cnt / p.wgs_per_xcd, b = t_begin + (jw + 1) * cnt / p.wgs_per_xcd;
    if (a >= b) return;                                               // (whole workgroup)
    const int tps = p.tiles_per_sample;
    const int n_items = (b - a) + 1 + ((b - 1) / tps - a / tps);    // tiles + the run's PRE + one PRE per sample that starts inside
    // cursor over the run: the next item is PRE (pre != 0) or TILE of tile j of sample n
    struct Cur { int n, j, pre; };
    auto cur_first = [&]() { Cur q; q.n = a / tps; q.j = a - q.n * tps; q.pre = 1; return q; };
    auto cur_next = [&](Cur& q) {
        if (q.pre) { q.pre = 0; return; }
        if (++q.j == tps) { q.j = 0; ++q.n; q.pre = 1; }
    };
    auto next_slot = [](int s) { return s == 16 ? 0 : s + 8; };

    if (role == 2) {
        // ================================================================= conversion: LDS-DMA one item ahead, raw -> X slot
        auto issue_dma = [&](const Cur& q, int buf) {
            const int rb = R * q.j - (q.pre ? R : 0) + 2;            // image row of the slot's row 0
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                if (k < NK / 2 && q.pre) continue;                   // (uniform)
                const int j = k * NW + wave;                          // piece: 64 chunks = half a row
                const int ri = j >> 1;
                const int grow = min(max(rb + ri, 0), H - 1);         // rows outside the image: any row inside (converted to zeros)
                const char* sbase = reinterpret_cast<const char*>(p.in) + ((size_t)(q.n * H + grow) * W * C) * 4 + (size_t)(j & 1) * 1024;
                const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem + buf * RAW_BYTES + j * 1024;
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(lane * 16), "s"(dst), "s"(sbase) : "memory");
            }
        };
        auto convert = [&](const Cur& q, int buf, int slot) {
            const int rb = R * q.j - (q.pre ? R : 0) + 2;
            float ta = 0.f;
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) {
                if (kk < NK / 2 && q.pre) continue;
                const int qi = kk * NTH + tid;
                const int px = qi / C4, c4 = qi % C4;
                const int ri = px / W, col = px - ri * W;
                const int grow = rb + ri;
                float4 v = *reinterpret_cast<const float4*>(smem + buf * RAW_BYTES + qi * 16);
                if (grow < 0 || grow >= H) v = make_float4(0.f, 0.f, 0.f, 0.f);
                v = elu4(v);
                unsigned char* dst = smem + X_OFF + (c4 >> 1) * XPS + ((slot + ri + XMIR) * WP + col + 1) * 16 + (c4 & 1) * 8;
                if constexpr (MODE == 2) {
                    StageScale ss{scale1, ta};
                    scale_track(v, &ss);
                    ta = ss.amax;
                    uint2 h, l;
                    split_f16x2(v, scale1, h, l);
                    *reinterpret_cast<uint2*>(dst) = h;
                    *reinterpret_cast<uint2*>(dst + KGS * XPS) = l;
                    if (kk >= NK / 2 && slot == 16) {                 // rows 20..23: the copy in front of row 0
                        *reinterpret_cast<uint2*>(dst - RING * ROWB) = h;
                        *reinterpret_cast<uint2*>(dst - RING * ROWB + KGS * XPS) = l;
                    }
                } else {
                    f16x4 h;
                    h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
                    *reinterpret_cast<f16x4*>(dst) = h;
                    if (kk >= NK / 2 && slot == 16) *reinterpret_cast<f16x4*>(dst - RING * ROWB) = h;
                }
            }
            if constexpr (MODE == 2) pair_range_tile(ta, scale1, rbits, p.calib);
        };
        Cur qd = cur_first(), qc = qd;
        issue_dma(qd, 0);
        cur_next(qd);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int slot = 0;
        for (int it = 0; it < n_items + 2; ++it) {
            lds_barrier();
            if (it + 1 < n_items) { issue_dma(qd, (it + 1) & 1); cur_next(qd); }
            if (it < n_items) { convert(qc, it & 1, slot); cur_next(qc); slot = next_slot(slot); }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // item it + 1 has landed before the next barrier publishes it
        }
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // filter fragments
        // one convolution over NU units two plane rows apart, the first one's tap (0, 0) source at byte ub0 of term 0
        auto conv = [&](auto nuc, const int ub0, const int PS, f32x4v* acc) {
            constexpr int NU = decltype(nuc)::value;
            constexpr int DU = 2 * ROWB;
            constexpr int NS = 9 * NU, D = NT == 2 ? 3 : 6;
            f16x8 ring[D][NT];
            auto ld = [&](int s) {
                const int tap = s / NU, i = s % NU;
                const int off = i * DU + ((tap / 3) * WP + (tap % 3)) * 16;
#pragma unroll
                for (int t = 0; t < NT; ++t) ring[s % D][t] = *reinterpret_cast<const f16x8*>(smem + ub0 + (off + t * KGS * PS));
            };
#pragma unroll
            for (int s = 0; s < D - 1 && s < NS; ++s) ld(s);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int tap = s / NU, i = s % NU;
                if (s + D - 1 < NS) ld(s + D - 1);
                const f16x8 xh = ring[s % D][0];
                const f16x8 wh = __builtin_bit_cast(f16x8, wf[tap][0]);
                const f32x4v c0 = tap == 0 ? f32x4v{0.f, 0.f, 0.f, 0.f} : acc[i];
                if constexpr (NT == 2) {
                    const f16x8 xl = ring[s % D][NT - 1];
                    const f16x8 wl = __builtin_bit_cast(f16x8, wf[tap][NT - 1]);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, c0, 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc[i], 0, 0, 0);
                } else {
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, c0, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        const int cq = 4 * hf + kq;                                    // channel quad of this lane's four outputs
        if (role == 0) {
            // ============================================================= conv1: X window -> ELU -> split -> M slot
            // intermediate row m of the slot (image row r0 + 1 + m) reads X rows slot + m - 2 .. slot + m
            auto conv1_item = [&](const Cur& q, int slot, auto nuc) {
                constexpr int NU = decltype(nuc)::value, I0 = 4 - NU;   // a PRE item: the wave's last unit only (m = 6 + sub)
                const int r0 = R * q.j - (q.pre ? R : 0);
                f32x4v acc[NU];
                conv(nuc, X_OFF + kq * XPS + ((slot + sub + 2 * I0 - 2 + XMIR) * WP + c) * 16, XPS, acc);
                // A PRE item's single accumulator is read right behind its last matrix instruction.  hipcc inserts the wait states a
                // vector instruction needs behind v_mfma (11 for this shape) in front of its own instructions but does not look
                // inside inline assembly -- and in the fp16-weight mode (descale1 == 1 folds away) elu4's asm block is the first reader.
                if constexpr (NU == 1) asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
                float tb = 0.f;
#pragma unroll
                for (int i = 0; i < NU; ++i) {
                    const int m = sub + 2 * (I0 + i);
                    const int grow = r0 + 1 + m;
                    float4 v = make_float4(acc[i][0] * descale1, acc[i][1] * descale1, acc[i][2] * descale1, acc[i][3] * descale1);
                    v = elu4(v);
                    if (grow < 0 || grow >= H) v = make_float4(0.f, 0.f, 0.f, 0.f);    // zero padding of conv2, not conv1 of padding
                    unsigned char* dst = smem + M_OFF + (cq >> 1) * MPS + ((slot + m + MMIR) * WP + c + 1) * 16 + (cq & 1) * 8;
                    if constexpr (MODE == 2) {
                        StageScale ss{scale2, tb};
                        scale_track(v, &ss);
                        tb = ss.amax;
                        uint2 h, l;
                        split_f16x2(v, scale2, h, l);
                        *reinterpret_cast<uint2*>(dst) = h;
                        *reinterpret_cast<uint2*>(dst + KGS * MPS) = l;
                        if (I0 + i == 3 && slot == 16) {               // rows 22, 23: the copy in front of row 0
                            *reinterpret_cast<uint2*>(dst - RING * ROWB) = h;
                            *reinterpret_cast<uint2*>(dst - RING * ROWB + KGS * MPS) = l;
                        }
                    } else {
                        f16x4 h;
                        h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
                        *reinterpret_cast<f16x4*>(dst) = h;
                        if (I0 + i == 3 && slot == 16) *reinterpret_cast<f16x4*>(dst - RING * ROWB) = h;
                    }
                }
                if constexpr (MODE == 2) pair_range_tile(tb, scale2, rbits, p.calib ? p.calib + 1 : nullptr);
            };
            Cur q = cur_first();
            int slot = 0;
            for (int it = 0; it < n_items + 2; ++it) {
                lds_barrier();
                if (it < 1 || it - 1 >= n_items) continue;
                if (q.pre) conv1_item(q, slot, std::integral_constant<int, 1>{});
                else conv1_item(q, slot, std::integral_constant<int, 4>{});
                cur_next(q);
                slot = next_slot(slot);
            }
        } else {
            // ============================================================= conv2: M window, + x, store (TILE items only)
            // output row o of the tile (image row r0 + o) reads M rows slot + o - 2 .. slot + o
            Cur q = cur_first();
            int slot = 0;
            for (int it = 0; it < n_items + 2; ++it) {
                lds_barrier();
                if (it < 2) continue;
                if (!q.pre) {
                    constexpr int NU = 4, DO = 2 * W * C;
                    const int r0 = R * q.j;
                    f32x4v acc[NU];
                    float4 xr[NU];
                    const unsigned o0 = (unsigned)(((q.n * H + r0 + sub) * W + c) * C + cq * 4);
#pragma unroll
                    for (int i = 0; i < NU; ++i) xr[i] = *reinterpret_cast<const float4*>(p.in + o0 + i * DO);
                    conv(std::integral_constant<int, NU>{}, M_OFF + kq * MPS + ((slot + sub - 2 + MMIR) * WP + c) * 16, MPS, acc);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                    for (int i = 0; i < NU; ++i) {
                        float4 y;
                        y.x = fmaf(acc[i][0], descale2, xr[i].x); y.y = fmaf(acc[i][1], descale2, xr[i].y);
                        y.z = fmaf(acc[i][2], descale2, xr[i].z); y.w = fmaf(acc[i][3], descale2, xr[i].w);
                        st_out(p.out + o0 + i * DO, y);
                    }
                }
                cur_next(q);
                slot = next_slot(slot);
            }
        }
    }
    if constexpr (MODE == 2) {
        if (rbits && (threadIdx.x & 63) == 0) atomicOr(p.range_flag, rbits);
    }
}

// One stage of a CRP block in ONE launch (SBC_OP_CONV_POOL):
//       out = conv3x3(ELU?(MaxPool5x5(x))) [+ (res2 + ELU(res1))]            ncsnv2/models/layers.py:76-83
// for 32-channel NHWC fp32 tensors, 16 pixels wide.  Unfused, a stage is a max-pool launch (one tensor read, one written) and a
// convolution launch (read it again, write the result, read two residual operands): at 223 MB per tensor the CRP block of the
// full-resolution level moves 2.2 GB per step; here the pooled tensor never exists in memory.
// A two-stage pipeline over tiles, double buffered: a persistent workgroup per CU of twelve waves in two roles --
//   conversion (4 waves, one per SIMD): keep the R + 6 raw rows of the next tile in flight by LDS-DMA; pool tile i -- the vertical
//           5-maximum in registers from the LDS copy, the horizontal one by DPP row shifts (a 16-pixel row is one DPP row;
//           out-of-image columns leave the lane's running maximum alone, rows outside the image were requested from the nearest row
//           inside: both are what MaxPool2d's -inf padding computes) --, ELU, two fp16 terms -> operand planes X[i & 1];
//   matrix (8 waves, two per SIMD): the K loop of the convolution on X[(i-1) & 1], two units (image rows) per wave, filter
//           fragments resident in registers; + residual operands (requested before the K loop), store.
// Both plane sets and the raw copies exist twice (the raw copy three times, see NRAW), so the writer of iteration i never touches
// what the readers of that iteration use: ONE workgroup barrier per tile.  The tile is bound by VECTOR-INSTRUCTION ISSUE, not by the
// matrix pipe: pooling costs ~20 vector instructions per value (8 vertical v_max3 + 20 DPP maxima + ELU 16 + split 8 + ... per four
// values), and every arrangement of the roles measured the same ~5-7 k cycles per tile (per-phase cycle counters of an instrumented
// build, history: 54de329: 4 conversion + 8 matrix waves 6.9 k with the builtins' ten-instruction DPP maxima; 8 + 4: 6.2 k, one
// matrix wave per SIMD needs 46 cycles per matrix instruction; 8 + 8: 5.3 k).  Four conversion waves issue the fewest instructions
// per tile (five pooled rows per lane share nine LDS reads).  Conversion wave w owns channel quads 2 (w & 3), + 1 and one half of the
// pooled rows: both pool passes of a value stay inside one wave, so the role needs no synchronisation of its own.
__device__ __forceinline__ float4 vmax5(float4 a, float4 b, float4 c, float4 d, float4 e) {
    // (v_max3_f32 by hand: fmaxf() costs a canonicalising v_max per operand)
    float4 m;
    asm("v_max3_f32 %0, %4, %8, %12\n\tv_max3_f32 %1, %5, %9, %13\n\tv_max3_f32 %2, %6, %10, %14\n\tv_max3_f32 %3, %7, %11, %15\n\t"
        "v_max3_f32 %0, %0, %16, %20\n\tv_max3_f32 %1, %1, %17, %21\n\tv_max3_f32 %2, %2, %18, %22\n\tv_max3_f32 %3, %3, %19, %23"
        : "=&v"(m.x), "=&v"(m.y), "=&v"(m.z), "=&v"(m.w)
        : "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w), "v"(c.x), "v"(c.y), "v"(c.z), "v"(c.w),
          "v"(d.x), "v"(d.y), "v"(d.z), "v"(d.w), "v"(e.x), "v"(e.y), "v"(e.z), "v"(e.w));
    return m;
}

template <int W, int R, int MODE, int NWC = 4, int C = 32>
__global__ __launch_bounds__(64 * (8 + NWC)) void conv_pool_kernel(PairParams p) {
    constexpr int NWM = 8;                            // matrix waves (two per SIMD); NWC = 4 or 8 conversion waves
    constexpr int KGS = C / 8, C4 = C / 4;
    static_assert(C == 32 && W == 16, "instantiated for 32 channels, 16-pixel rows");
    constexpr int NT = MODE == 2 ? 2 : 1;             // fp16 terms per operand
    constexpr int RI = R + 6, RP = R + 2;             // raw rows (conv halo + pool halo), pooled rows
    constexpr int WP = W + 2;
    constexpr int XPS = (RP * WP * 16 + 255) / 256 * 256;
    constexpr int RAW_BYTES = RI * W * C * 4;
    constexpr int XSZ = NT * KGS * XPS;
    constexpr int NRAW = 3;                           // raw tiles in LDS: in flight, being pooled, and one tile back (the matrix waves read
                                                      // the residual operand res2 from it when it is the kernel's own input: CRP's path0)
    constexpr int X_OFF = NRAW * RAW_BYTES;
    constexpr int NPIECE = RAW_BYTES / 1024;          // LDS-DMA requests of a tile (1 KB each)
    constexpr int NU = 2;                             // units (image rows of 16 pixels) per matrix wave: 8 waves x 2 = 2 halves x R
    static_assert(R == 8, "eight output rows: four unit groups of two rows per output-channel half");
    extern __shared__ __attribute__((aligned(256))) unsigned char smem[];

    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);        // 0 .. 7: matrix waves, 8 .. 15: conversion waves
    const bool matrix = wv < NWM;
    const int lane = threadIdx.x & 63;
    const int hf = wv & 1, sub = (wv >> 1) & 3;        // matrix: 16-output-channel half; unit group (rows sub, sub + 4)
    const int kq = lane >> 4, c = lane & 15;
    const int H = p.H;

    float scale1 = 1.f, descale1 = 1.f;
    unsigned rbits = 0;
    if constexpr (MODE == 2) {
        const float4 t1 = f16x2_trailer(reinterpret_cast<const float4*>(p.w1), 9 * (C / 16) * (C / 32) * NT);
        scale1 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t1.x)));
        descale1 = t1.y;
        if (t1.w != 0.f && (p.flags & SBC_PRO_ELU)) rbits |= 4u;   // small inputs: this kernel has the exp(x) - 1 form of ELU only (SBC_RANGE_ELU)
    }
    // padding columns of both plane sets
    for (int i = threadIdx.x; i < 2 * NT * KGS * RP * 2; i += 64 * (NWM + NWC)) {
        const int side = i & 1, row = (i >> 1) % RP, pl = (i >> 1) / RP;
        *reinterpret_cast<uint4*>(smem + X_OFF + pl * XPS + (row * WP + side * (W + 1)) * 16) = make_uint4(0, 0, 0, 0);
    }

    const int xcd = blockIdx.x & 7, jw = blockIdx.x >> 3;
    const int t_begin = xcd * p.tiles_per_xcd;
    const int t_end = min(t_begin + p.tiles_per_xcd, p.ntiles);
    const int first = t_begin + jw;
    const int n_my = first < t_end ? (t_end - first + p.wgs_per_xcd - 1) / p.wgs_per_xcd : 0;
    if (n_my == 0) return;
    auto tile_of = [&](int k) { return first + k * p.wgs_per_xcd; };

    // ---- conversion role
    const int wc = wv - NWM;                           // 0 .. 7
    auto issue_dma = [&](int tile, int buf) {
        const int n = tile / p.tiles_per_sample, r0 = (tile - n * p.tiles_per_sample) * R;
#pragma unroll
        for (int k = 0; k < (NPIECE + NWC - 1) / NWC; ++k) {
            const int j = k * NWC + wc;                                        // piece: chunks j * 64 .. + 63 of the raw tile
            if (NPIECE % NWC == 0 || j < NPIECE) {
                const int ri = (j * 64) / (W * C4), within = j * 64 - ri * (W * C4);
                const int grow = min(max(r0 - 3 + ri, 0), H - 1);              // rows outside the image: the nearest row inside (see header)
                const char* sbase = reinterpret_cast<const char*>(p.in) + ((size_t)(n * H + grow) * W * C) * 4 + (size_t)within * 16;
                const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem + buf * RAW_BYTES + j * 1024;
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(lane * 16), "s"(dst), "s"(sbase) : "memory");
            }
        }
    };
    // lane = (column c, channel quad 2 (wc & 3) + ql, row group): the ten pooled rows in two groups of five (four conversion waves:
    // group = lane half) or in groups of 3, 2, 3, 2 (eight waves: group = 2 (wc >> 2) + lane half)
    const int ql = (lane >> 4) & 1, grp = NWC == 4 ? (lane >> 5) : 2 * (wc >> 2) + (lane >> 5);
    const int cq_c = 2 * (wc & 3) + ql;
    constexpr int NRG = NWC == 4 ? 5 : 3;              // pooled rows per lane (at most)
    const int prow0 = NWC == 4 ? 5 * grp : (grp == 0 ? 0 : grp == 1 ? 3 : grp == 2 ? 5 : 8);
    const bool full = NWC == 4 || (grp & 1) == 0;      // (uniform over a wave half: lanes 0..31 / 32..63)
    auto convert_tile = [&](int k, int rb, int xb) {
        const int tile = tile_of(k);
        const int n = tile / p.tiles_per_sample, r0 = (tile - n * p.tiles_per_sample) * R;
        (void)n;
        const unsigned char* raw = smem + rb * RAW_BYTES + (c * C4 + cq_c) * 16 + prow0 * (W * C4 * 16);
        // pooled row prow0 + j (image row r0 - 1 + prow0 + j) is the maximum over raw rows prow0 + j .. + 4 (image row r0 - 3 + ...)
        float4 rv[NRG + 4];
#pragma unroll
        for (int i = 0; i < NRG + 4; ++i) rv[i] = *reinterpret_cast<const float4*>(raw + (i < NRG + 3 || full ? i : NRG + 2) * (W * C4 * 16));
        float ta = 0.f;
#pragma unroll
        for (int j = 0; j < NRG; ++j) {
            if (j == NRG - 1 && !full) break;
            float4 v = vmax5(rv[j], rv[j + 1], rv[j + 2], rv[j + 3], rv[j + 4]);
            // horizontal 5-maximum over the 16 lanes of the row (= the image row): v_max_f32 with a DPP row shift on its first source;
            // a lane whose shifted source lies outside the row is disabled for that instruction and keeps its running maximum.  By hand:
            // from the builtins hipcc emits a v_mov_b32_dpp, a copy for its `old` operand and a v_max per shift (ten instructions per
            // value instead of five).  (vmax5 is an asm block too: the s_nop gives its last write the two wait states a DPP read needs.)
            {
                float4 m;
                asm("s_nop 1\n\t"
                    "v_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tv_mov_b32 %2, %6\n\tv_mov_b32 %3, %7\n\t"
                    "v_max_f32_dpp %0, %4, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_max_f32_dpp %1, %5, %1 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                    "v_max_f32_dpp %2, %6, %2 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_max_f32_dpp %3, %7, %3 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                    "v_max_f32_dpp %0, %4, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\tv_max_f32_dpp %1, %5, %1 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                    "v_max_f32_dpp %2, %6, %2 row_shr:2 row_mask:0xf bank_mask:0xf\n\tv_max_f32_dpp %3, %7, %3 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                    "v_max_f32_dpp %0, %4, %0 row_shl:1 row_mask:0xf bank_mask:0xf\n\tv_max_f32_dpp %1, %5, %1 row_shl:1 row_mask:0xf bank_mask:0xf\n\t"
                    "v_max_f32_dpp %2, %6, %2 row_shl:1 row_mask:0xf bank_mask:0xf\n\tv_max_f32_dpp %3, %7, %3 row_shl:1 row_mask:0xf bank_mask:0xf\n\t"
                    "v_max_f32_dpp %0, %4, %0 row_shl:2 row_mask:0xf bank_mask:0xf\n\tv_max_f32_dpp %1, %5, %1 row_shl:2 row_mask:0xf bank_mask:0xf\n\t"
                    "v_max_f32_dpp %2, %6, %2 row_shl:2 row_mask:0xf bank_mask:0xf\n\tv_max_f32_dpp %3, %7, %3 row_shl:2 row_mask:0xf bank_mask:0xf"
                    : "=&v"(m.x), "=&v"(m.y), "=&v"(m.z), "=&v"(m.w) : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
                v = m;
            }
            if (p.flags & SBC_PRO_ELU) v = elu4(v);
            const int prow = prow0 + j;
            const int grow = r0 - 1 + prow;
            if (grow < 0 || grow >= H) v = make_float4(0.f, 0.f, 0.f, 0.f);        // zero padding of the convolution
            unsigned char* dst = smem + X_OFF + xb * XSZ + (cq_c >> 1) * XPS + (prow * WP + c + 1) * 16 + (cq_c & 1) * 8;
            if constexpr (MODE == 2) {
                StageScale ss{scale1, ta};
                scale_track(v, &ss);
                ta = ss.amax;
                uint2 h, l;
                split_f16x2(v, scale1, h, l);
                *reinterpret_cast<uint2*>(dst) = h;
                *reinterpret_cast<uint2*>(dst + KGS * XPS) = l;
            } else {
                f16x4 h;
                h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
                *reinterpret_cast<f16x4*>(dst) = h;
            }
        }
        if constexpr (MODE == 2) pair_range_tile(ta, scale1, rbits, p.calib);
    };
    // The two roles run SEPARATE loops with the same barrier sequence (n_my + 1 workgroup barriers each): in one loop the filter
    // fragments (72 registers) would stay allocated through the conversion code, which then spills at 128 registers per wave.
    if (!matrix) {
        issue_dma(tile_of(0), 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (int it = 0; it < n_my + 1; ++it) {
            lds_barrier();
            if (it + 1 < n_my) issue_dma(tile_of(it + 1), (it + 1) % NRAW);
            if (it < n_my) convert_tile(it, it % NRAW, it & 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    } else {
        uint4 wf[9][NT];
        {
            const int lsrc = (16 * hf + c) + 32 * (kq & 1);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    wf[tap][t] = p.w1[(((tap * (C / 16) + (kq >> 1)) * (C / 32)) * NT + t) * 64 + lsrc];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const bool res2_lds = p.res2 == p.in;            // CRP: the second residual operand is this launch's own input
        for (int it = 0; it < n_my + 1; ++it) {
            lds_barrier();
            const int t1 = it - 1;
            if (t1 < 0) continue;
            const int tile = tile_of(t1);
            const int n = tile / p.tiles_per_sample, r0 = (tile - n * p.tiles_per_sample) * R;
            // this wave's two units: image rows r0 + sub and r0 + sub + 4, output channels 16 hf .. + 15
            f32x4v acc[NU];
            const int cq = 4 * hf + kq;
            float4 x1[NU];
            constexpr int DO = 4 * W * C;
            const unsigned o0 = (unsigned)(((n * H + r0 + sub) * W + c) * C + cq * 4);
            if (p.res1) {
#pragma unroll
                for (int i = 0; i < NU; ++i) x1[i] = *reinterpret_cast<const float4*>(p.res1 + o0 + i * DO);
            }
            {
                constexpr int DU = 4 * WP * 16;                            // bytes from unit i to unit i + 1 (four plane rows)
                const int ub0 = X_OFF + (t1 & 1) * XSZ + kq * XPS + (sub * WP + c) * 16;
                constexpr int NS = 9 * NU, D = NT == 2 ? 3 : 6;
                f16x8 ring[D][NT];
                auto ld = [&](int s) {
                    const int tap = s / NU, i = s % NU;
                    const int off = i * DU + ((tap / 3) * WP + (tap % 3)) * 16;
#pragma unroll
                    for (int t = 0; t < NT; ++t) ring[s % D][t] = *reinterpret_cast<const f16x8*>(smem + ub0 + (off + t * KGS * XPS));
                };
#pragma unroll
                for (int s = 0; s < D - 1; ++s) ld(s);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int tap = s / NU, i = s % NU;
                    if (s + D - 1 < NS) ld(s + D - 1);
                    const f16x8 xh = ring[s % D][0];
                    const f16x8 wh = __builtin_bit_cast(f16x8, wf[tap][0]);
                    const f32x4v c0 = tap == 0 ? f32x4v{0.f, 0.f, 0.f, 0.f} : acc[i];
                    if constexpr (NT == 2) {
                        const f16x8 xl = ring[s % D][NT - 1];
                        const f16x8 wl = __builtin_bit_cast(f16x8, wf[tap][NT - 1]);
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, c0, 0, 0, 0);
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc[i], 0, 0, 0);
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc[i], 0, 0, 0);
                    } else {
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, c0, 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                float4 y = make_float4(acc[i][0] * descale1, acc[i][1] * descale1, acc[i][2] * descale1, acc[i][3] * descale1);
                if (p.res1) {
                    // r = res1 [ELU];  if res2: r = res2 + r;  y = y + r     (include/sbc_hip.h: the CONV epilogue)
                    float4 rr = x1[i];
                    // (the four-instruction ELU: a CRP block's res1 is the tensor its FIRST stage pools -- if the calibration found
                    // that one small, the first stage has raised SBC_RANGE_ELU and the host re-runs the batch in bf16x3)
                    if (p.flags & SBC_EPI_RES1_ELU) rr = elu4(rr);
                    if (p.res2) {
                        // (the tile's own raw copy, three rows down from its first row, when res2 is the launch's input; else memory)
                        const float4 r2 = res2_lds ? *reinterpret_cast<const float4*>(smem + (t1 % NRAW) * RAW_BYTES +
                                                                                      (((sub + 4 * i + 3) * W + c) * C4 + cq) * 16)
                                                   : *reinterpret_cast<const float4*>(p.res2 + o0 + i * DO);
                        rr.x = r2.x + rr.x; rr.y = r2.y + rr.y; rr.z = r2.z + rr.z; rr.w = r2.w + rr.w;
                    }
                    y.x += rr.x; y.y += rr.y; y.z += rr.z; y.w += rr.w;
                }
                st_out(p.out + o0 + i * DO, y);
            }
        }
    }
    if constexpr (MODE == 2) {
        if (rbits && (threadIdx.x & 63) == 0) atomicOr(p.range_flag, rbits);
    }
}

// ------------------------------------------------------------------------------------------------ dispatch
// Common tail of the launchers below: tiles of R rows of one sample; each XCD owns a contiguous eighth of them and runs `per_cu`
// persistent workgroups for each of its share of the CUs the plan may count on -- never more than it has tiles.
template <class K>
static int launch_tiles(K kern, const PairParams& p0, int R, int per_cu, int threads, size_t lds, hipStream_t stream, bool dry) {
    { const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds); if (rc) return rc; }
    if (dry) return SBC_OK;
    PairParams p = p0;
    p.tiles_per_sample = p.H / R;
    p.ntiles = p.B * p.tiles_per_sample;
    int dev = 0, cus = 256;
    SBC_CHECK_HIP(hipGetDevice(&dev));
    SBC_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    p.tiles_per_xcd = (p.ntiles + 7) / 8;
    p.wgs_per_xcd = max(1, min(per_cu * persistent_cus(cus) / 8, p.tiles_per_xcd));
    hipLaunchKernelGGL(kern, dim3(8 * p.wgs_per_xcd), dim3(threads), lds, stream, p);
    SBC_CHECK_HIP(hipGetLastError());
    return SBC_OK;
}

template <int W, int R, int MODE, int NW = 4, int C = 32>
static int launch_pair(const PairParams& p, hipStream_t stream, bool dry) {
    constexpr int NT = MODE == 2 ? 2 : 1;
    constexpr int RI = R + 4, RM = R + 2, WP = W + 2;
    constexpr int XPS = (RI * WP * 16 + 255) / 256 * 256, MPS = (RM * WP * 16 + 255) / 256 * 256;
    constexpr size_t lds = (size_t)RI * W * C * 4 + (size_t)NT * (C / 8) * (XPS + MPS);
    constexpr int PER_CU = NW == 4 ? 2 : 1;                              // workgroups per CU (two waves per SIMD either way)
    static_assert(lds <= 160 * 1024 / PER_CU, "LDS of the resident workgroups");
    return launch_tiles(conv_pair_kernel<W, R, MODE, NW, C>, p, R, PER_CU, 64 * NW, lds, stream, dry);
}

template <int MODE>
static int launch_pair_roll(const PairParams& p, hipStream_t stream, bool dry) {
    constexpr int NT = MODE == 2 ? 2 : 1, ROWB = 18 * 16;
    constexpr int XPS = (28 * ROWB + 255) / 256 * 256, MPS = (26 * ROWB + 255) / 256 * 256;
    constexpr size_t lds = (size_t)2 * 8 * 16 * 32 * 4 + (size_t)NT * 4 * (XPS + MPS);
    static_assert(lds <= 160 * 1024, "LDS of the one resident workgroup");
    return launch_tiles(conv_pair_roll_kernel<MODE>, p, 8, 1, 768, lds, stream, dry);
}

template <int MODE>
static int launch_pool(const PairParams& p, hipStream_t stream, bool dry) {
    constexpr int W = 16, R = 8, C = 32, NT = MODE == 2 ? 2 : 1;
    constexpr int RI = R + 6, RP = R + 2, WP = W + 2;
    constexpr int XPS = (RP * WP * 16 + 255) / 256 * 256;
    constexpr size_t lds = (size_t)3 * RI * W * C * 4 + (size_t)2 * NT * (C / 8) * XPS;
    static_assert(lds <= 160 * 1024, "LDS of the one resident workgroup");
    constexpr int NWC = 4;
    return launch_tiles(conv_pool_kernel<W, R, MODE, NWC, C>, p, R, 1, 64 * (8 + NWC), lds, stream, dry);
}

int launch_conv_pool(const sbc_op& op, hipStream_t stream, bool dry) {
    SBC_REQUIRE(op.in && op.out && op.weight_split, "conv_pool: in / out / weight_split must be set");
    SBC_REQUIRE(op.cin == 32 && op.cout == 32 && op.ksize == 3 && op.dil == 1 && op.W == 16 && op.H % 8 == 0 && op.H >= 8,
                "conv_pool: 32 -> 32 channels, 3x3, undilated, 16-pixel rows, H a multiple of 8 (got %d -> %d, %dx%d)", op.cin, op.cout, op.H, op.W);
    SBC_REQUIRE(op.B > 0, "conv_pool: bad batch %d", op.B);
    const bool x2 = (op.flags & SBC_CONV_F16X2) != 0, f16w = (op.flags & SBC_CONV_F16W) != 0;
    SBC_REQUIRE(x2 != f16w, "conv_pool: exactly one of SBC_CONV_F16X2 / SBC_CONV_F16W (the forms of weight_split it reads)");
    SBC_REQUIRE(!op.bias && !(op.flags & (SBC_PRO_NORM | SBC_EPI_POOL | SBC_EPI_UP | SBC_EPI_ELUGRAD | SBC_EPI_MOMENTS_OUT)),
                "conv_pool: no bias, prologue = max pool [+ ELU], epilogue = residual operands only");
    SBC_REQUIRE(!op.res2 || op.res1, "conv_pool: res2 only together with res1");
    // (persistent workgroups read the 3-row halos of neighbouring tiles by LDS-DMA while other workgroups store: no aliasing)
    SBC_REQUIRE(op.out != op.in && op.out != op.res1 && op.out != op.res2, "conv_pool: out must not alias in / res1 / res2");
    SBC_REQUIRE((long)op.B * op.H * op.W * op.cin <= 0x7fffffffL, "conv_pool: tensor exceeds the 32-bit element index");
    PairParams p{};
    p.in = (const float*)op.in; p.out = (float*)op.out;
    p.w1 = (const uint4*)op.weight_split; p.w2 = nullptr;
    p.res1 = (const float*)op.res1; p.res2 = (const float*)op.res2; p.flags = op.flags;
    p.B = op.B; p.H = op.H;
    p.calib = (float*)op.calib;
    if (x2) {
        unsigned* word = nullptr;
        const int rc = range_flag_ptr(&word);
        if (rc) return rc;
        p.range_flag = word;
    }
    return x2 ? launch_pool<2>(p, stream, dry) : launch_pool<1>(p, stream, dry);
}

int launch_conv_pair(const sbc_op& op, hipStream_t stream, bool dry) {
    SBC_REQUIRE(op.in && op.out && op.weight_split && op.weight2_split, "conv_pair: in / out / weight_split / weight2_split must be set");
    SBC_REQUIRE(op.cin == op.cout && (op.cin == 32 || op.cin == 64) && op.ksize == 3 && op.dil == 1,
                "conv_pair: C -> C -> C channels with C = 32 (or 64 with SBC_CONV_F16W), 3x3, undilated");
    SBC_REQUIRE(op.B > 0 && op.H > 0 && op.W > 0, "conv_pair: bad shape B=%d H=%d W=%d", op.B, op.H, op.W);
    const bool x2 = (op.flags & SBC_CONV_F16X2) != 0, f16w = (op.flags & SBC_CONV_F16W) != 0;
    SBC_REQUIRE(x2 != f16w, "conv_pair: exactly one of SBC_CONV_F16X2 / SBC_CONV_F16W (the forms of weight_split it reads)");
    SBC_REQUIRE(op.out != op.in, "conv_pair: out must not alias in (tiles read their neighbours' halo rows while others store)");
    SBC_REQUIRE((long)op.B * op.H * op.W * op.cin <= 0x7fffffffL, "conv_pair: tensor exceeds the 32-bit element index");
    PairParams p{};
    p.in = (const float*)op.in; p.out = (float*)op.out;
    p.w1 = (const uint4*)op.weight_split; p.w2 = (const uint4*)op.weight2_split;
    p.B = op.B; p.H = op.H;
    p.calib = (float*)op.calib;
    if (x2) {
        unsigned* word = nullptr;
        const int rc = range_flag_ptr(&word);
        if (rc) return rc;
        p.range_flag = word;
    }
    if (op.cin == 64) {
        // 64 channels (the half- and quarter-resolution levels of BASELINE config 5), fp16-weight mode: 8-wave workgroups, one
        // per CU -- four 16-output-channel groups x two unit groups (rows of a 16-pixel image; column blocks of a 32-pixel one)
        SBC_REQUIRE(f16w, "conv_pair: 64 channels need SBC_CONV_F16W (two-term filter fragments would not fit in registers)");
        if (op.W == 16 && op.H % 8 == 0) return launch_pair<16, 8, 1, 8, 64>(p, stream, dry);
        if (op.W == 32 && op.H % 4 == 0) return launch_pair<32, 4, 1, 8, 64>(p, stream, dry);
        set_error("conv_pair: no 64-channel kernel for image %dx%d", op.H, op.W);
        return SBC_ERR_UNSUPPORTED;
    }
    // 16-pixel rows, H % 8 == 0: the row-ring kernel from 1024 tiles -- a workgroup's run is then at least four tiles at full grid
    // width, eight at half width (850 trajectories per GPU 2.51 -> 2.44 ms per step, 425: 1.57 -> 1.53 against the tile kernel; below
    // ~16 tiles per workgroup a pipeline's fill and drain cost more than it gains: 1040 tiles 21.8 us against 21.3 for the
    // per-tile-halo pipeline, 6800 tiles 112 against 122, 13600 tiles 230 against 242) -- the tile kernel below (identical results)
    if (op.W == 16 && op.H % 8 == 0 && (long)op.B * (op.H / 8) >= 1024)
        return x2 ? launch_pair_roll<2>(p, stream, dry) : launch_pair_roll<1>(p, stream, dry);
    if (op.W == 16 && op.H % 8 == 0) return x2 ? launch_pair<16, 8, 2>(p, stream, dry) : launch_pair<16, 8, 1>(p, stream, dry);
    // 32-pixel rows (the half-resolution level of a 256 x 64 array): tiles of 4 rows, wave pair `sub` owns column block `sub`
    if (op.W == 32 && op.H % 4 == 0 && f16w) return launch_pair<32, 4, 1, 4>(p, stream, dry);
    if (op.W == 8 && op.H % 8 == 0) return x2 ? launch_pair<8, 8, 2>(p, stream, dry) : launch_pair<8, 8, 1>(p, stream, dry);
    // 64-pixel rows (the full-resolution level of a 256 x 64 array, BASELINE config 5): one 8-wave workgroup per CU, tiles of
    // 4 rows x 64 pixels; the fp16-weight mode only (two terms would not fit the LDS next to the 64 KB raw tile)
    if (op.W == 64 && op.H % 4 == 0 && f16w) return launch_pair<64, 4, 1, 8>(p, stream, dry);
    set_error("conv_pair: no kernel for image %dx%d", op.H, op.W);
    return SBC_ERR_UNSUPPORTED;
}

}  // namespace sbc
