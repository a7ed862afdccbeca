// Parameters of the fused RCU / CRP kernels (conv_pair.hip).
#pragma once
#include "conv_common.h"

namespace sbc {

struct PairParams {
    const float* __restrict__ in;
    float* __restrict__ out;
    const uint4* __restrict__ w1;       // sbc_pack_conv_weight_f16x2 / _f16 layout of conv1 (32 -> 32, 3x3)
    const uint4* __restrict__ w2;
    unsigned* __restrict__ range_flag;
    float* __restrict__ calib;          // sbc_f16x2_calibrate: two amax slots (conv1's input, the intermediate), else NULL
    const float* __restrict__ res1;     // conv_pool_kernel: residual operands of the CONV epilogue (or NULL)
    const float* __restrict__ res2;
    int flags;                          // conv_pool_kernel: SBC_PRO_ELU, SBC_EPI_RES1_ELU
    int B, H, ntiles, tiles_per_sample, wgs_per_xcd, tiles_per_xcd;
};

}  // namespace sbc
