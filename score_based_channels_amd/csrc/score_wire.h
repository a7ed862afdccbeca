// The wiring of NCSNv2Deepest (ncsnv2/models/ncsnv2.py:269-300) into fused launch records: which records exist, in which order, on
// which launch lane, which logical tensors share storage -- and their binding: which packed form of which parameter goes into which
// sbc_op field over a host's memory.  Host only -- no HIP header, no device: score.hip (sbc_score_create, a C host) and scorenet.py
// (through sbc_score_wiring_*, include/sbc_hip.h) pack weights, allocate, and call bind().  Every fusion rule, profiling tag, shape
// predicate, conv_mode gate and binding rule of the network lives in this unit and nowhere else.
#pragma once
#include <array>
#include <string>
#include <vector>
#include "../../include/sbc_hip.h"

namespace sbc {

void set_error(const char* fmt, ...);        // the text behind sbc_last_error() (api.hip)

namespace wire {

// profiling tags (sbc_op.tag; bench.py times each class through sbc_plan_profile)
enum Tag {
    TAG_CONV_TOP = 1,        // 3x3 convolutions ngf -> ngf at full resolution
    TAG_PAIR_TOP = 2,        // SBC_OP_CONV_PAIR at full resolution
    TAG_CONV_MID = 3,        // undilated 3x3 convolutions 2 ngf -> 2 ngf at half resolution
    TAG_POOL_TOP = 4,        // SBC_OP_CONV_POOL at full resolution
    TAG_DIRECT_MID = 5,      // the TAG_CONV_MID layers without a norm prologue / resize / tile-moment output (csrc/conv_dp.hip takes them)
    TAG_RES_TOP = 6,         // SBC_OP_RES_BLOCK at full resolution
    TAG_CHAIN = 7,           // SBC_OP_CHAIN: 7 + the index of the record's (channels, width) in CHAIN_KERNELS
    TAG_DOWN = 12            // SBC_OP_CONV_DOWN: 12 at 16-pixel rows, 13 at 8
};

struct Shape { int c, w; };                  // (channels, width)
constexpr Shape CHAIN_KERNELS[] = {{128, 2}, {64, 2}, {64, 4}, {64, 8}, {32, 8}};     // the instantiations of csrc/conv_chain.hip
// RCU blocks fused into SBC_OP_CONV_PAIR (csrc/conv_pair.hip; it also takes 32 channels at a width of 8: measured slower than two launches)
constexpr Shape PAIR_SHAPES[] = {{32, 16}};
// ... in the fp16-weight mode (a 256 x 64 array): also 32- and 64-pixel rows, and the 64-channel levels
constexpr Shape PAIR_SHAPES_F16W[] = {{32, 16}, {32, 32}, {32, 64}, {64, 16}, {64, 32}};

struct Tensor {                              // a logical per-sample NHWC tensor [h][w][c]
    std::string name;
    int h, w, c;
    int slot = -1;                           // the physical buffer it lives in
    size_t elems() const { return (size_t)h * w * c; }
};

struct Block {                               // one block of an SBC_OP_CHAIN record; RES blocks carry everything behind w2
    int type;
    std::string w1, w2;
    int dil = 1;
    std::string bias1, bias2, norm1, norm2, w3, bias3;
};

struct Record {                              // one launch; strings are state_dict keys, empty = none; tensors are indices, -1 = none
    int kind = 0, flags = 0, ksize = 3, dil = 1, tag = 0;
    std::string name;
    int src = -1, dst = -1, stats = -1, res1 = -1, res2 = -1, up = -1;
    int moments = -1;                        // second output: tile moments of dst (SBC_EPI_MOMENTS_OUT)
    int geom = -1;                           // SBC_OP_INORM_STATS from tile moments: the tensor whose (H, W, C) the launch describes
    std::string norm_key;                    // SBC_PRO_NORM_SELF: the norm whose (alpha | gamma | beta) the record's `stats` points at
    std::string weight, bias, weight2;       // weight2: the second convolution of an SBC_OP_CONV_PAIR / SBC_OP_RES_BLOCK / SBC_OP_CONV_DOWN
    std::string bias2, norm2;                // the second convolution's bias; SBC_OP_RES_BLOCK: the second norm
    std::vector<Block> blocks;               // SBC_OP_CHAIN: its blocks in execution order
    bool side = false, join = false;         // SBC_OP_SIDE / SBC_OP_JOIN (SBC_WIRING_OVERLAP)
    int lane = 0, signal = 0, wait0 = 0, wait1 = 0;      // sbc_op.lane / signal / wait
    std::array<int, 5> inputs() const { return {src, stats, res1, res2, up}; }
};

struct Wiring {
    std::vector<Tensor> tensors;
    std::vector<Record> records;
    std::vector<size_t> slot_elems;          // per-sample float32 elements of each physical buffer
    int x = -1, out = -1;                    // the network's input and output tensors [nt][nr][channels]
};

// SBC_OK, or SBC_ERR_INVALID with the reason in sbc_last_error().  Wires what `d` asks for behind the gates of d.conv_mode
// (include/sbc_hip.h); which SBC_SCORE_FUSE_* a mode can run is the caller's business (sbc_score_create, scorenet.ScoreNet).
__attribute__((visibility("hidden"))) int build(const sbc_score_wiring_desc& d, Wiring& out);      // (the library exports the C calls only)
// sbc_score_wiring_bind on a Wiring: ops [w.records.size()], chains [one per SBC_OP_CHAIN record]
__attribute__((visibility("hidden"))) int bind(const Wiring& w, const sbc_score_bind_desc& d, sbc_op* ops, sbc_chain* chains);

}  // namespace wire
}  // namespace sbc
