// Wavefront and workgroup reductions in a fixed order, and the loop pragmas of the kernels that sum in strided loops
// (wgan.hip, wgan_train.hip, ldamp.hip, cs_l1.hip).
#pragma once
#include "common.h"

// the library carries no packed-fp32 arithmetic (Makefile: check-no-packed); the loop vectoriser would form it in strided loops
#define SBC_NO_VEC _Pragma("clang loop vectorize(disable) interleave(disable)")
#define SBC_NO_VEC_NO_UNROLL _Pragma("clang loop vectorize(disable) interleave(disable) unroll(disable)")

namespace sbc {

// butterflies over the 64 lanes: every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// 256 threads; red: 4 doubles of LDS.  Every thread gets the result.
__device__ __forceinline__ double block_sum256(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();                                   // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace sbc
