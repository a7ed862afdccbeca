// The one description of the WGAN generator (DCGAN_G_Ours at 16 x 64) for latent optimisation (csrc/wgan.hip) and training
// (csrc/wgan_train.hip): its constants, the geometry of its layers, the float tensors of its state dict and how a *_create call opens
// one; and the generator kernels of wgan.hip that training launches as they are (host launchers only, the kernels stay where they are).
#pragma once
#include <string>
#include <utility>
#include <vector>
#include "common.h"
#include "host_params.h"

namespace sbc {
namespace wgan_shared {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int NR = 16, NT = 64, NZ = 60, CH = 128, PIX = NR * NT, DENSE = CH * (NR / 4) * (NT / 4);
constexpr int MAX_EXTRA = 4, MAX_L = 2 + MAX_EXTRA;
constexpr float BN_EPS = 1e-5f;

// geometry of layer k = 0 .. L: its OUTPUT is H x W.  0 is the dense output, 4 x 16; the hidden layers 1 and 2 read their input through
// the nearest x 2 map; layer_ks: the filter of hidden layer k = 1 .. L
__host__ __device__ constexpr int layer_h(int k) { return k == 0 ? NR / 4 : k == 1 ? NR / 2 : NR; }
__host__ __device__ constexpr int layer_w(int k) { return k == 0 ? NT / 4 : k == 1 ? NT / 2 : NT; }
__host__ __device__ constexpr int layer_ks(int k) { return k <= 2 ? 5 : 3; }
// sign-mask words of one h x w plane: one 32-bit word per 32 pixels of a row (a row of 16 pixels has one word of 16 bits)
__host__ __device__ constexpr int mask_words(int h, int w) { return h * ((w + 31) / 32); }

// ---- the state dict ---------------------------------------------------------------------------------------------------------------
// the state-dict prefixes of hidden layer k = 1 .. L: its convolution and its BatchNorm
inline std::string conv_name(int k) { return k <= 2 ? "conv.conv" + std::to_string(k) : "conv.extra_conv" + std::to_string(k - 3); }
inline std::string bn_name(int k) { return k <= 2 ? "conv.bn" + std::to_string(k) : "conv.extra_bn" + std::to_string(k - 3); }

// the float tensors of a generator with n_extra extra layers as (name, numel): the parameters in state-dict order, then the running
// statistics of layers 1 .. L
inline std::vector<std::pair<std::string, int64_t>> generator_tensors(int n_extra) {
    const int L = 2 + n_extra;
    std::vector<std::pair<std::string, int64_t>> t = {{"dense.dense_input.weight", (int64_t)DENSE * NZ}, {"dense.dense_input.bias", DENSE}};
    for (int k = 1; k <= L; ++k) {
        t.push_back({conv_name(k) + ".weight", (int64_t)CH * CH * layer_ks(k) * layer_ks(k)});
        if (k <= 2) t.push_back({conv_name(k) + ".bias", CH});
        t.push_back({bn_name(k) + ".weight", CH});
        t.push_back({bn_name(k) + ".bias", CH});
    }
    t.push_back({"conv.conv_out.weight", 2 * CH * 25});
    t.push_back({"conv.conv_out.bias", 2});
    for (int k = 1; k <= L; ++k) {
        t.push_back({bn_name(k) + ".running_mean", CH});
        t.push_back({bn_name(k) + ".running_var", CH});
    }
    return t;
}

// Index the n refs of a generator's state dict in `sd` and count its extra layers.  SBC_OK, or the error set on behalf of `who`: a ref
// without name or data, a name given twice (`what` is that message's noun), more than MAX_EXTRA extra layers, or not exactly the
// float tensors of a generator with that many.
inline int open_generator(const char* who, const sbc_tensor_ref* refs, int n, const char* what, TensorIndex& sd, int* n_extra) {
    const int rc = sd.build_unique(who, what, refs, n);
    if (rc) return rc;
    int e = 0;
    while (sd.has(conv_name(3 + e) + ".weight")) ++e;
    SBC_REQUIRE(e <= MAX_EXTRA, "%s: at most %d extra layers are supported (got %d)", who, MAX_EXTRA, e);
    const int want = (int)generator_tensors(e).size();   // 16 + 5 e
    SBC_REQUIRE(n == want, "%s: a generator with %d extra layers has %d float tensors (got %d)", who, e, want, n);
    *n_extra = e;
    return SBC_OK;
}

// ---- launchers of wgan.hip's kernels, asynchronous on `s`; they check nothing: their callers have ------------------------------------
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
