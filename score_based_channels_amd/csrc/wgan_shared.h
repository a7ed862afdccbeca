// The generator kernels of csrc/wgan.hip that WGAN training (csrc/wgan_train.hip) launches as they are: host launchers only, the kernels
// stay where they are.  Every launcher is asynchronous on `s` and checks nothing: its callers have.
#pragma once
#include "common.h"

namespace sbc {
namespace wgan_shared {

constexpr int NR = 16, NT = 64, NZ = 60, CH = 128, PIX = NR * NT, DENSE = CH * (NR / 4) * (NT / 4), MAX_EXTRA = 4;

// dense: out [B][128][4][16] = W z + bias
void launch_dense(const float* z, const float* W, const float* bias, float* out, int B, hipStream_t s);
// conv128_kernel<100 + ks>: out [B][128][H >> pool][W >> pool] = the ks x ks convolution of src [B][128][H >> up][W >> up] with the packed
// filters `wpk` (+ bias, or NULL), read through the nearest x 2 map with `up`, summed over 2 x 2 blocks with `pool`
void launch_conv128_raw(const float* src, const float* wpk, const float* bias, float* out, int H, int W, int ks, int up, int pool, int B, hipStream_t s);
// out_kernel without the measurement terms: gen [B][2][16][64] = conv_out(act) + bias
void launch_out_conv(const float* act, const float* w, const float* bias, float* gen, int B, hipStream_t s);
// out_adjoint_kernel: out [B][128][16][64] = d / d act of <dG, conv_out(act)>
void launch_out_adjoint(const float* dG, const float* w, float* out, int B, hipStream_t s);
// repack128_kernel: torch [128][128][ks][ks] -> the forward and the adjoint packing of conv128
void launch_repack128(const float* w, float* fwd, float* adj, int ks, hipStream_t s);

}  // namespace wgan_shared
}  // namespace sbc
