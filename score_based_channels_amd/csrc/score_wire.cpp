// score_wire.h: the one wiring of the score network (reference lines in brackets).
//
// Fusion rules:
//   * InstanceNorm++ -> ELU -> conv [layers.py:444-449]: a statistics record writes (mu, scale, shift) per (sample, channel); the
//     convolution applies the affine + ELU while staging its input tile (SBC_PRO_NORM | SBC_PRO_ELU).
//   * ELU -> conv of RCU blocks [layers.py:130-131]: SBC_PRO_ELU; `x += residual` [:133] is the convolution's res1.
//   * ResidualBlock `shortcut + output` [:456]: res1 of conv2; pooled blocks run the 1x1 shortcut first and add it after conv2's
//     own 2x2 mean pool [ConvMeanPool :311-312].
//   * CRP [layers.py:76-83]: `x = act(x)` is never materialised: maxpool(ELU(x)) == ELU(maxpool(x)), and the running sum
//     `x = path + x` is folded into the second convolution's epilogue as path1 + (path0 + ELU(x)).
//   * MSF [layers.py:178-184]: `sums = 0 + conv0(h0) + resize(conv1(h1))`: conv1 runs first at its own resolution, conv0 adds its
//     (bilinear, align_corners) resize in the epilogue.
//   * `h = 2x - 1` [ncsnv2.py:270-273] lives in the begin convolution; normalizer -> ELU -> end_conv -> / sigma [:291-298] is one kernel.
#include "score_wire.h"
#include <string.h>
#include <algorithm>
#include <map>

#define WIRE_REQUIRE(cond, ...)            \
    do {                                   \
        if (!(cond)) {                     \
            ::sbc::set_error(__VA_ARGS__); \
            return SBC_ERR_INVALID;        \
        }                                  \
    } while (0)

namespace sbc {
namespace wire {
namespace {

// ---- the shapes the fused launches take -------------------------------------------------------------------------------------
template <size_t N>
int shape_index(const Shape (&v)[N], int c, int w) {
    for (size_t i = 0; i < N; ++i)
        if (v[i].c == c && v[i].w == w) return (int)i;
    return -1;
}
// SBC_OP_CONV_PAIR: (channels, width) in `shapes`, heights that are multiples of its tile (8 rows at a width of 16, 4 rows at 32 / 64)
bool pair_fusable(const Tensor& x, const std::vector<Shape>& shapes) {
    for (const Shape& s : shapes)
        if (s.c == x.c && s.w == x.w) return x.h % (x.w == 16 ? 8 : 4) == 0;
    return false;
}
// SBC_OP_CONV_POOL (a CRP stage as one launch): 32 channels, 16-pixel rows, heights that are multiples of 8
bool pool_fusable(const Tensor& x) { return x.c == 32 && x.w == 16 && x.h % 8 == 0; }
// SBC_OP_RES_BLOCK: 32 -> 32 channels, no resampling or dilation, 64 x 16 samples (two fp16 operand planes of a whole sample fill
// the LDS of a CU)
bool res_fusable(const Tensor& x, int cout, bool down, int dilation) {
    return x.c == 32 && cout == 32 && !down && !dilation && x.h == 64 && x.w == 16;
}
// SBC_OP_CONV_DOWN: 32 -> 64 channels at 16-pixel rows, 64 -> 64 at 8 (res2.0 / res3.0 of a 64 x 16 array), heights that are
// multiples of 16
bool down_fusable(const Tensor& x, int cout) {
    return x.h % 16 == 0 && ((x.w == 16 && x.c == 32 && cout == 64) || (x.w == 8 && x.c == 64 && cout == 64));
}
// SBC_OP_CHAIN: 8 x 2 samples of 64 or 128 channels, 16 x 4 samples of 64 channels (the two lowest levels of a 64 x 16 array), and
// 32 x 8 samples of 32 or 64 channels (a wave holds half a sample there).  The kernel also takes ResidualBlocks at 32 x 8 -- res2.1 --
// through the ABI, but measured no gain over its two Winograd launches with folded statistics (4.26-4.32 against 4.24-4.25 ms per
// two-stream step): the wiring does not use it.
bool chain_fusable(const Tensor& x, int type) {
    if (x.h == 16 && x.w == 4 && x.c == 64) return true;
    if (x.h == 32 && x.w == 8 && (x.c == 32 || x.c == 64)) return type != SBC_CHAIN_RES;
    return x.h == 8 && x.w == 2 && (x.c == 64 || x.c == 128);
}
// SBC_OP_END_CONV forms the normalizer's statistics itself (SBC_PRO_NORM_SELF): 32 channels, 1024 pixels (the normalised sample of a
// 64 x 16 array fills the LDS of a CU)
bool end_fusable(int h, int w, int c) { return c == 32 && h * w == 1024; }

// The skip branches of the decoder: refineK's adapt convolutions of its FIRST input (the encoder output layerK, layers.py:234-249,
// ncsnv2.py:284-289) depend on nothing the decoder computes before refineK's MSF convolution adds them.  For small batches the
// low-resolution launches between the encoder output and that MSF convolution are latency-bound and leave most of the chip idle;
// the skip branches then run beside them on a lane of their own.  ONE lane: measured (profiles/r06_skip_lanes.txt) -- two or three
// are slower than none, one is -8 % per step at 213 and 425 trajectories.
const sbc_skip_branch DEFAULT_SKIP_SPEC[] = {{"refine5.adapt_convs.0.", "res3.1.", 1}, {"refine4.adapt_convs.0.", "res3.1.", 1},
                                             {"refine3.adapt_convs.0.", "res3.1.", 1}, {"refine31.adapt_convs.0.", "res31.1.", 1},
                                             {"refine2.adapt_convs.0.", "res4.1.", 1}};

struct Builder {
    static constexpr int SELF_NORM = -2;     // stats(): no statistics record, the consuming convolution computes them itself
    const int ngf, nt, nr, flags;
    std::vector<Shape> pair_shapes;          // SBC_SCORE_FUSE_PAIRS: the RCU shapes that become SBC_OP_CONV_PAIR records
    std::vector<Tensor>& t;
    std::vector<Record>& ops;
    std::map<int, int> producer;             // tensor -> index of the record that writes it
    std::string pending_norm;                // the norm of the last SELF_NORM
    bool side_now = false;                   // SBC_WIRING_OVERLAP: records emitted while set carry `side`

    bool on(int flag) const { return (flags & flag) != 0; }
    int tensor(const std::string& n, int h, int w, int c) {
        Tensor x;
        x.name = n; x.h = h; x.w = w; x.c = c;
        t.push_back(x);
        return (int)t.size() - 1;
    }
    Record& emit(int kind, const std::string& name, int src, int dst, bool side = false) {
        Record o;
        o.kind = kind; o.name = name; o.src = src; o.dst = dst; o.side = side;
        producer[dst] = (int)ops.size();
        ops.push_back(o);
        return ops.back();
    }
    int top(int x, int tag) const { return t[x].h == nt ? tag : 0; }
    // Branches are overlapped only below full resolution: full-resolution launches fill the chip on their own
    bool low_res(int x) const { return on(SBC_WIRING_OVERLAP) && t[x].h < nt; }

    int conv(const std::string& name, int src, const std::string& wkey, int cout, bool bias = true, int cflags = 0, int stats = -1,
             int res1 = -1, int res2 = -1, int up = -1, int ksize = 3, int dil = 1) {
        const bool pool = cflags & SBC_EPI_POOL;
        const int sh = t[src].h, sw = t[src].w, sc = t[src].c;
        const int dst = tensor(name, pool ? sh / 2 : sh, pool ? sw / 2 : sw, cout);
        Record& o = emit(SBC_OP_CONV, name, src, dst, side_now);
        o.weight = wkey + ".weight";
        if (bias) o.bias = wkey + ".bias";
        o.res1 = res1; o.res2 = res2; o.up = up; o.ksize = ksize; o.dil = dil;
        o.flags = cflags | (up >= 0 ? SBC_EPI_UP : 0);
        if (stats == SELF_NORM) { o.norm_key = pending_norm; o.flags |= SBC_PRO_NORM_SELF; }
        else o.stats = stats;
        if (ksize == 3 && sc == ngf && cout == ngf && sh == nt) o.tag = TAG_CONV_TOP;
        if (ksize == 3 && dil == 1 && sc == 2 * ngf && cout == 2 * ngf && !pool && 2 * sh == nt) o.tag = TAG_CONV_MID;
        return dst;
    }
    // InstanceNorm++ statistics of `src` for the norm `nkey`.  With SBC_SCORE_FOLD_STATS, for images of at most 64 pixels (the 16x4
    // and 8x2 levels of a 64x16 array) there is no statistics record at all: a workgroup of the consuming 3x3 convolution holds whole
    // samples and computes them itself (SELF_NORM, which conv() understands); and for 32- and 64-channel tensors of whole 128-pixel
    // tiles that come out of the begin convolution, an unpooled undilated 3x3 convolution or an SBC_OP_RES_BLOCK, the producer also
    // writes the moments of its 128-pixel tiles (SBC_EPI_MOMENTS_OUT) and the statistics record reads THOSE (SBC_PRO_NORM_MOMENTS:
    // HW / 128 x C x 8 bytes per sample instead of the tensor); consumers see ordinary statistics either way.
    int stats(const std::string& name, int src, const std::string& nkey, bool consumer_is_conv = true) {
        const int hw = t[src].h * t[src].w, sw = t[src].w, sc = t[src].c;
        const bool fold = on(SBC_SCORE_FOLD_STATS);
        if (fold && consumer_is_conv && hw <= 64 && !(hw & (hw - 1)) && sw >= 2 && !(sw & (sw - 1))) {
            pending_norm = nkey;
            return SELF_NORM;
        }
        const int dst = tensor(name, 1, 3, sc);
        int moments = -1;
        auto it = producer.find(src);
        if (fold && it != producer.end() && (sc == 32 || sc == 64) && hw % 128 == 0 && hw >= 256 && 128 % (2 * sw) == 0 &&
            t[src].h % std::max(1, 128 / sw) == 0) {
            Record& pr = ops[it->second];
            if ((pr.kind == SBC_OP_BEGIN_CONV && sc == 32) || pr.kind == SBC_OP_RES_BLOCK ||
                (pr.kind == SBC_OP_CONV && pr.ksize == 3 && pr.dil == 1 && !(pr.flags & SBC_EPI_POOL))) {
                if (pr.moments < 0) {
                    pr.moments = tensor(t[src].name + ".moments", hw / 128, sc, 2);     // [tile][channel][(mean, M2)]
                    pr.flags |= SBC_EPI_MOMENTS_OUT;
                }
                moments = pr.moments;
            }
        }
        Record& o = emit(SBC_OP_INORM_STATS, name, moments >= 0 ? moments : src, dst);
        o.weight = nkey;
        if (moments >= 0) { o.flags = SBC_PRO_NORM_MOMENTS; o.geom = src; }
        return dst;
    }
    int maxpool(const std::string& name, int src, bool elu) {
        const int dst = tensor(name, t[src].h, t[src].w, t[src].c);
        emit(SBC_OP_MAXPOOL5, name, src, dst).flags = elu ? SBC_PRO_ELU : 0;
        return dst;
    }
    int residual_block(const std::string& p, int x, int cout, bool down, int dilation) {      // layers.py:443-456
        const int d = dilation ? dilation : 1;
        const bool pooled = down && !dilation;
        const int c1 = down ? t[x].c : cout;
        if (on(SBC_SCORE_FUSE_CHAIN) && chain_fusable(t[x], SBC_CHAIN_RES) && t[x].c == cout && !pooled && (d == 1 || t[x].w == 2)) {
            // the whole block as a RES block of a CHAIN record: the launch forms both norms' statistics itself (a workgroup holds
            // whole samples), so neither statistics records nor the intermediate tensor exist
            Block bl{SBC_CHAIN_RES, p + "conv1.weight", p + "conv2.weight"};
            bl.dil = d; bl.bias1 = p + "conv1.bias"; bl.bias2 = p + "conv2.bias"; bl.norm1 = p + "normalize1"; bl.norm2 = p + "normalize2";
            if (down) { bl.w3 = p + "shortcut.weight"; bl.bias3 = p + "shortcut.bias"; }
            return chain(p + "chain", x, {bl});
        }
        const int s1 = stats(p + "normalize1", x, p + "normalize1");
        if (on(SBC_SCORE_FUSE_RES) && res_fusable(t[x], cout, down, dilation) && s1 != SELF_NORM) {
            // the whole block in one launch: a workgroup owns a sample and forms normalize2's statistics itself; the intermediate
            // tensor, its statistics record and two tensor round trips do not exist
            const int out = tensor(p + "conv2", t[x].h, t[x].w, cout);
            Record& o = emit(SBC_OP_RES_BLOCK, p + "block", x, out, side_now);
            o.stats = s1; o.weight = p + "conv1.weight"; o.weight2 = p + "conv2.weight"; o.bias = p + "conv1.bias";
            o.bias2 = p + "conv2.bias"; o.norm2 = p + "normalize2"; o.tag = top(x, TAG_RES_TOP);
            return out;
        }
        const int a = conv(p + "conv1", x, p + "conv1", c1, true, SBC_PRO_NORM | SBC_PRO_ELU, s1, -1, -1, -1, 3, d);
        const int s2 = stats(p + "normalize2", a, p + "normalize2");
        if (pooled && on(SBC_SCORE_FUSE_DOWN) && down_fusable(t[x], cout) && s2 != SELF_NORM) {
            // pooled conv2 + pooled 1x1 shortcut as ONE launch of stride-2 convolutions with the pooled filters: both inputs read
            // once, the pooled shortcut tensor never exists
            const int out = tensor(p + "conv2", t[x].h / 2, t[x].w / 2, cout);
            Record& o = emit(SBC_OP_CONV_DOWN, p + "down", a, out);
            o.stats = s2; o.res1 = x; o.weight = p + "conv2.conv.weight"; o.weight2 = p + "shortcut.conv.weight";
            o.bias = p + "conv2.conv.bias"; o.bias2 = p + "shortcut.conv.bias"; o.tag = TAG_DOWN + (t[x].w == 16 ? 0 : 1);
            return out;
        }
        int sc = x;
        bool joined = false;
        if (pooled || t[x].c != cout || down) {
            // the shortcut convolution only meets the main branch again at conv2's residual add
            joined = side_now = low_res(x);
            sc = pooled ? conv(p + "shortcut", x, p + "shortcut.conv", cout, true, SBC_EPI_POOL, -1, -1, -1, -1, 1, 1)
                        : conv(p + "shortcut", x, p + "shortcut", cout, true, 0, -1, -1, -1, -1, 3, d);
            side_now = false;
        }
        const int out = pooled ? conv(p + "conv2", a, p + "conv2.conv", cout, true, SBC_PRO_NORM | SBC_PRO_ELU | SBC_EPI_POOL, s2, sc)
                               : conv(p + "conv2", a, p + "conv2", cout, true, SBC_PRO_NORM | SBC_PRO_ELU, s2, sc, -1, -1, 3, d);
        ops.back().join = joined;
        return out;
    }
    static std::vector<Block> rcu_blocks(const std::string& p, int n_blocks, std::vector<Block> v = {}) {
        for (int i = 1; i <= n_blocks; ++i)
            v.push_back(Block{SBC_CHAIN_RCU, p + std::to_string(i) + "_1_conv.weight", p + std::to_string(i) + "_2_conv.weight"});
        return v;
    }
    // `blocks` in execution order on x as SBC_OP_CHAIN records of at most SBC_CHAIN_MAX_BLOCKS blocks each
    int chain(const std::string& name, int x, const std::vector<Block>& blocks) {
        for (size_t k = 0; k < blocks.size(); k += SBC_CHAIN_MAX_BLOCKS) {
            const std::string part = name + "." + std::to_string(k / SBC_CHAIN_MAX_BLOCKS);
            const int dst = tensor(part, t[x].h, t[x].w, t[x].c);
            Record& o = emit(SBC_OP_CHAIN, part, x, dst, side_now);
            o.tag = TAG_CHAIN + shape_index(CHAIN_KERNELS, t[x].c, t[x].w);
            o.blocks.assign(blocks.begin() + k, blocks.begin() + std::min(blocks.size(), k + (size_t)SBC_CHAIN_MAX_BLOCKS));
            x = dst;
        }
        return x;
    }
    int rcu(const std::string& p, int x, int n_blocks) {                                        // layers.py:126-134 (n_stages = 2, no bias)
        if (on(SBC_SCORE_FUSE_CHAIN) && chain_fusable(t[x], SBC_CHAIN_RCU)) return chain(p + "chain", x, rcu_blocks(p, n_blocks));
        for (int i = 1; i <= n_blocks; ++i) {
            const std::string a = p + std::to_string(i) + "_1_conv", b = p + std::to_string(i) + "_2_conv";
            if (pair_fusable(t[x], pair_shapes)) {
                // x + conv2(ELU(conv1(ELU(x)))) in one launch, the intermediate tensor never exists in memory
                const int dst = tensor(b, t[x].h, t[x].w, t[x].c);
                Record& o = emit(SBC_OP_CONV_PAIR, p + std::to_string(i) + "_pair", x, dst, side_now);
                o.weight = a + ".weight"; o.weight2 = b + ".weight"; o.tag = top(x, TAG_PAIR_TOP);
                x = dst;
                continue;
            }
            const int tt = conv(a, x, a, t[x].c, false, SBC_PRO_ELU);
            x = conv(b, tt, b, t[x].c, false, SBC_PRO_ELU, -1, x);
        }
        return x;
    }
    int crp(const std::string& p, int x) {                                                     // layers.py:76-83 (two stages, max pooling)
        if (on(SBC_SCORE_FUSE_PAIRS) && pool_fusable(t[x])) {
            // each stage -- max pool, convolution, running sum -- as ONE launch: the pooled tensors never exist in memory
            const int path0 = tensor(p + "convs.0", t[x].h, t[x].w, t[x].c);
            Record& a = emit(SBC_OP_CONV_POOL, p + "pool_conv0", x, path0, side_now);
            a.weight = p + "convs.0.weight"; a.flags = SBC_PRO_ELU; a.tag = top(x, TAG_POOL_TOP);
            const int out = tensor(p + "convs.1", t[x].h, t[x].w, t[x].c);
            Record& b = emit(SBC_OP_CONV_POOL, p + "pool_conv1", path0, out, side_now);
            b.weight = p + "convs.1.weight"; b.flags = SBC_EPI_RES1_ELU; b.res1 = x; b.res2 = path0; b.tag = top(x, TAG_POOL_TOP);
            return out;
        }
        const int p0 = maxpool(p + "pool0", x, true);
        const int path0 = conv(p + "convs.0", p0, p + "convs.0", t[x].c, false);
        const int p1 = maxpool(p + "pool1", path0, false);
        return conv(p + "convs.1", p1, p + "convs.1", t[x].c, false, SBC_EPI_RES1_ELU, -1, x, path0);
    }
    // layers.py:234-249; MSF (layers.py:178-184) for two inputs, the second may be at half resolution.  The second input's adapt
    // convolutions and its MSF convolution do not depend on the first input's: with SBC_WIRING_OVERLAP they are issued first as side
    // records and the first input's MSF convolution (which adds their result) joins them.
    int refine(const std::string& p, const std::vector<int>& xs, int features, bool end = false) {
        const bool chains = on(SBC_SCORE_FUSE_CHAIN);
        const Block crp_block{SBC_CHAIN_CRP, p + "crp.convs.0.weight", p + "crp.convs.1.weight"};
        if (xs.size() == 1 && chains && chain_fusable(t[xs[0]], SBC_CHAIN_CRP) && features == t[xs[0]].c) {
            // the whole RefineBlock is one chain: adapt RCU x 2, CRP, output RCU
            std::vector<Block> bl = rcu_blocks(p + "adapt_convs.0.", 2);
            bl.push_back(crp_block);
            return chain(p + "chain", xs[0], rcu_blocks(p + "output_convs.", end ? 3 : 1, bl));
        }
        int h;
        if (xs.size() == 1) {
            h = rcu(p + "adapt_convs.0.", xs[0], 2);
        } else {
            const bool joined = side_now = low_res(xs[0]);
            const int h1 = rcu(p + "adapt_convs.1.", xs[1], 2);
            const int t1 = conv(p + "msf.convs.1", h1, p + "msf.convs.1", features);
            side_now = false;
            const int h0 = rcu(p + "adapt_convs.0.", xs[0], 2);
            h = conv(p + "msf.convs.0", h0, p + "msf.convs.0", features, true, 0, -1, -1, -1, t1);
            ops.back().join = joined;
        }
        if (chains && chain_fusable(t[h], SBC_CHAIN_CRP)) return chain(p + "tail", h, rcu_blocks(p + "output_convs.", end ? 3 : 1, {crp_block}));
        h = crp(p + "crp.", h);
        return rcu(p + "output_convs.", h, end ? 3 : 1);
    }
};

// Adjacent CHAIN records where the second one is the only consumer of the first one's output become ONE record (up to
// SBC_CHAIN_MAX_BLOCKS blocks): res5.0 + res5.1 + the whole of refine1, for instance.
void merge_chains(std::vector<Record>& ops) {
    for (size_t k = 0; k + 1 < ops.size();) {
        Record& a = ops[k];
        const Record& b = ops[k + 1];
        bool ok = a.kind == SBC_OP_CHAIN && b.kind == SBC_OP_CHAIN && b.src == a.dst && !(a.side || b.side || a.join || b.join) &&
                  a.blocks.size() + b.blocks.size() <= SBC_CHAIN_MAX_BLOCKS;
        for (size_t j = k + 2; ok && j < ops.size(); ++j)
            for (int id : ops[j].inputs()) ok = ok && id != a.dst;
        if (!ok) { ++k; continue; }
        a.name += "+" + b.name;
        a.blocks.insert(a.blocks.end(), b.blocks.begin(), b.blocks.end());
        a.dst = b.dst;
        ops.erase(ops.begin() + k + 1);
    }
}

// SBC_SCORE_SKIP_LANES: move every branch of `spec` -- the contiguous run of records whose names start with the prefix -- behind the
// LAST record in front of it whose name starts with its anchor, onto its lane: the branch's first record waits for an event the anchor
// record signals, its last record signals the event its consumer (the first later record that reads the branch's result) waits for.
// Every record stays the same launch with the same arguments: results are identical bit for bit.  Branches that do not exist in this
// wiring (other fusion settings) are skipped.
int hoist_skip_branches(Wiring& w, const sbc_skip_branch* spec, int n_spec) {
    std::vector<Record>& ops = w.records;
    auto starts = [](const std::string& v, const char* pre) { return v.compare(0, strlen(pre), pre) == 0; };
    int next_evt = 1;
    auto signal_of = [&](Record& o) {        // 0: out of events
        if (!o.signal && next_evt <= SBC_MAX_EVENTS) o.signal = next_evt++;
        return o.signal;
    };
    for (int e = 0; e < n_spec; ++e) {
        const char *prefix = spec[e].branch, *anchor = spec[e].anchor;
        const int lane = spec[e].lane, n_ops = (int)ops.size();
        WIRE_REQUIRE(prefix && anchor, "skip branch %d lacks its branch or anchor prefix", e);
        int i0 = -1, i1 = -1, count = 0;
        for (int i = 0; i < n_ops; ++i)
            if (starts(ops[i].name, prefix)) { if (i0 < 0) i0 = i; i1 = i; ++count; }
        if (!count) continue;
        WIRE_REQUIRE(count == i1 - i0 + 1 && lane > 0 && lane < SBC_MAX_LANES,
                     "skip branch '%s' is not one contiguous run of records (or bad lane %d)", prefix, lane);
        for (int i = i0; i <= i1; ++i)
            WIRE_REQUIRE(!ops[i].lane && !ops[i].side && !ops[i].join, "skip branch '%s' is already on a lane", prefix);
        int a = -1;
        for (int i = 0; i < i0; ++i) if (starts(ops[i].name, anchor)) a = i;
        WIRE_REQUIRE(a >= 0, "anchor '%s' of skip branch '%s' not found in front of it", anchor, prefix);
        // the branch reads only tensors that exist at the anchor (its own intermediates aside)
        std::vector<char> have(w.tensors.size(), 0);
        have[w.x] = 1;
        for (int i = 0; i <= i1; ++i)
            if (i <= a || i >= i0)
                for (int id : {ops[i].dst, ops[i].moments}) if (id >= 0) have[id] = 1;
        for (int i = i0; i <= i1; ++i)
            for (int id : ops[i].inputs())
                WIRE_REQUIRE(id < 0 || have[id], "skip branch '%s' reads %s, which record '%s' does not have yet", prefix,
                             w.tensors[id].name.c_str(), ops[a].name.c_str());
        std::vector<Record> branch(ops.begin() + i0, ops.begin() + i1 + 1);
        ops.erase(ops.begin() + i0, ops.begin() + i1 + 1);
        int consumer = -1;
        for (int i = i0; i < (int)ops.size() && consumer < 0; ++i)
            for (int id : ops[i].inputs()) if (id == branch.back().dst) consumer = i;
        WIRE_REQUIRE(consumer >= 0, "no record reads the result of skip branch '%s'", prefix);
        for (const Record* o : {&ops[consumer], &branch.front()})
            WIRE_REQUIRE(!o->wait1, "record '%s' already waits for two events", o->name.c_str());
        for (Record& o : branch) o.lane = lane;
        const int start = signal_of(ops[a]), done = start ? signal_of(branch.back()) : 0;
        WIRE_REQUIRE(start && done, "more than %d lane events", SBC_MAX_EVENTS);
        (branch.front().wait0 ? branch.front().wait1 : branch.front().wait0) = start;
        (ops[consumer].wait0 ? ops[consumer].wait1 : ops[consumer].wait0) = done;
        ops.insert(ops.begin() + a + 1, branch.begin(), branch.end());
    }
    return SBC_OK;
}

// Share storage between logical tensors with disjoint lifetimes (linear scan over the records; outputs never alias inputs of their
// own record).  The network input and output keep private slots: they are caller-visible.
void assign_slots(Wiring& w) {
    const std::vector<Record>& ops = w.records;
    const int n_ops = (int)ops.size();
    // a side record may still be running until the next join record: what it reads stays live until then
    std::vector<int> done_at(n_ops);
    for (int i = n_ops - 1, next_join = n_ops - 1; i >= 0; --i) {
        if (ops[i].join) next_join = i;
        done_at[i] = ops[i].side ? next_join : i;
    }
    // a record on a lane is known to be complete at the first run-stream record that waits for an event which its lane signals at or
    // behind it (records of one lane run in list order); without one, at the end of the list (sbc_plan_run joins every lane there)
    for (int i = 0; i < n_ops; ++i) {
        if (!ops[i].lane) continue;
        done_at[i] = n_ops - 1;
        for (int k = i; k < n_ops && done_at[i] == n_ops - 1; ++k) {
            if (ops[k].lane != ops[i].lane || !ops[k].signal) continue;
            for (int m = k + 1; m < n_ops; ++m)
                if (!ops[m].lane && (ops[m].wait0 == ops[k].signal || ops[m].wait1 == ops[k].signal)) { done_at[i] = m; break; }
        }
    }
    std::vector<int> last_use(w.tensors.size(), -1);
    for (int i = 0; i < n_ops; ++i)
        for (int id : ops[i].inputs())
            if (id >= 0) last_use[id] = std::max(last_use[id], done_at[i]);
    std::map<size_t, std::vector<int>> free_slots;          // elements -> slots
    std::vector<int> live;
    auto pinned = [&](int id) { return id == w.x || id == w.out; };
    auto alloc = [&](int id) {
        Tensor& x = w.tensors[id];
        std::vector<int>& pool = free_slots[x.elems()];
        if (!pool.empty() && !pinned(id)) { x.slot = pool.back(); pool.pop_back(); }
        else { x.slot = (int)w.slot_elems.size(); w.slot_elems.push_back(x.elems()); }
    };
    alloc(w.x);
    for (int i = 0; i < n_ops; ++i) {
        const int dst = ops[i].dst, mom = ops[i].moments;
        for (int id : {dst, mom})
            if (id >= 0) { alloc(id); live.push_back(id); }
        for (size_t k = 0; k < live.size();) {
            const int id = live[k];
            if (!pinned(id) && id != dst && id != mom && last_use[id] <= i) {
                free_slots[w.tensors[id].elems()].push_back(w.tensors[id].slot);
                live.erase(live.begin() + k);
            } else {
                ++k;
            }
        }
    }
}

}  // namespace

int build(const sbc_score_wiring_desc& d, Wiring& w) {
    const int ngf = d.ngf, nt = d.nt, nr = d.nr;
    WIRE_REQUIRE(nt > 0 && nr > 0 && nt % 8 == 0 && nr % 8 == 0, "Nt and Nr must be multiples of 8 (three 2x mean-pools), got %dx%d", nt, nr);
    WIRE_REQUIRE(ngf > 0 && d.channels > 0, "ngf and channels must be positive, got %d and %d", ngf, d.channels);
    WIRE_REQUIRE(d.conv_mode >= -1 && d.conv_mode <= 3, "conv_mode must be -1 (none) or 0 bf16x3, 1 f32, 2 f16w, 3 f16x2, got %d", d.conv_mode);
    int flags = d.flags;
    // the gates of a conv_mode: the tile moments are written by the Winograd split kernels (not fp32), and conv_wx3 takes power-of-two images
    if (d.conv_mode >= 0 && (d.conv_mode == 1 || (nt & (nt - 1)) || (nr & (nr - 1)))) flags &= ~SBC_SCORE_FOLD_STATS;
    const bool lanes = (flags & SBC_SCORE_SKIP_LANES) != 0;
    WIRE_REQUIRE(!(lanes && (flags & SBC_WIRING_OVERLAP)), "skip_overlap and overlap (SBC_OP_SIDE records) do not mix");
    WIRE_REQUIRE(d.n_pair_shapes >= 0 && d.n_skip >= 0, "negative count of pair shapes or skip branches");
    w = Wiring();
    Builder b{ngf, nt, nr, flags, {}, w.tensors, w.records};
    if (flags & SBC_SCORE_FUSE_PAIRS) {
        if (d.pair_shapes) for (int i = 0; i < d.n_pair_shapes; ++i) b.pair_shapes.push_back({d.pair_shapes[2 * i], d.pair_shapes[2 * i + 1]});
        else if (d.conv_mode == 2) b.pair_shapes.assign(std::begin(PAIR_SHAPES_F16W), std::end(PAIR_SHAPES_F16W));
        else b.pair_shapes.assign(std::begin(PAIR_SHAPES), std::end(PAIR_SHAPES));
    }
    w.x = b.tensor("x", nt, nr, d.channels);
    int h = b.tensor("begin_conv", nt, nr, ngf);
    { Record& o = b.emit(SBC_OP_BEGIN_CONV, "begin_conv", w.x, h); o.weight = "begin_conv.weight"; o.bias = "begin_conv.bias"; }
    struct Stage { const char* name; int cout; bool down; int dil; };
    const Stage stages[6] = {{"res1", ngf, false, 0}, {"res2", 2 * ngf, true, 0}, {"res3", 2 * ngf, true, 0},
                             {"res31", 2 * ngf, true, 0}, {"res4", 4 * ngf, true, 2}, {"res5", 4 * ngf, true, 4}};
    int layers[6];
    for (int i = 0; i < 6; ++i) {
        h = b.residual_block(std::string(stages[i].name) + ".0.", h, stages[i].cout, stages[i].down, stages[i].dil);
        h = b.residual_block(std::string(stages[i].name) + ".1.", h, stages[i].cout, false, stages[i].dil);
        layers[i] = h;
    }
    const int ref1 = b.refine("refine1.", {layers[5]}, 4 * ngf);
    const int ref2 = b.refine("refine2.", {layers[4], ref1}, 2 * ngf);
    const int ref31 = b.refine("refine31.", {layers[3], ref2}, 2 * ngf);
    const int ref3 = b.refine("refine3.", {layers[2], ref31}, 2 * ngf);
    const int ref4 = b.refine("refine4.", {layers[1], ref3}, ngf);
    const int ref5 = b.refine("refine5.", {layers[0], ref4}, ngf, true);
    w.out = b.tensor("score", nt, nr, d.channels);
    const bool self = (flags & SBC_SCORE_FUSE_END) && end_fusable(nt, nr, ngf);
    // (SBC_SCORE_FUSE_END: the normalizer's statistics are formed inside the end-convolution launch -- a workgroup holds whole samples,
    // the tensor is read once instead of twice, and there is no statistics record)
    const int sn = self ? -1 : b.stats("normalizer", ref5, "normalizer", false);
    Record& end = b.emit(SBC_OP_END_CONV, "end_conv", ref5, w.out);
    end.weight = "end_conv.weight"; end.bias = "end_conv.bias"; end.stats = sn;
    if (self) { end.flags = SBC_PRO_NORM_SELF; end.norm_key = "normalizer"; }
    merge_chains(w.records);
    if (lanes) {
        const bool own = d.skip != nullptr;
        const int rc = hoist_skip_branches(w, own ? d.skip : DEFAULT_SKIP_SPEC, own ? d.n_skip : (int)(sizeof(DEFAULT_SKIP_SPEC) / sizeof(DEFAULT_SKIP_SPEC[0])));
        if (rc) return rc;
    }
    for (Record& o : w.records)             // (after the statistics folding, which adds SBC_EPI_MOMENTS_OUT to producers)
        if (o.tag == TAG_CONV_MID && !(o.flags & (SBC_PRO_NORM | SBC_EPI_UP | SBC_EPI_MOMENTS_OUT))) o.tag = TAG_DIRECT_MID;
    if (flags & SBC_WIRING_PRIVATE_SLOTS) {
        for (size_t i = 0; i < w.tensors.size(); ++i) { w.tensors[i].slot = (int)i; w.slot_elems.push_back(w.tensors[i].elems()); }
    } else {
        assign_slots(w);
    }
    return SBC_OK;
}

// ---- binding: the records over a host's memory (include/sbc_hip.h: sbc_score_wiring_bind) ---------------------------------------
int bind(const Wiring& w, const sbc_score_bind_desc& d, sbc_op* ops, sbc_chain* chains) {
    WIRE_REQUIRE(ops && d.batch > 0 && d.conv_mode >= 0 && d.conv_mode <= 3,
                 "sbc_score_wiring_bind: ops, a positive batch and conv_mode in {0 bf16x3, 1 f32, 2 f16w, 3 f16x2} required");
    WIRE_REQUIRE(d.slots && d.n_slots == (int)w.slot_elems.size(), "sbc_score_wiring_bind: the wiring has %d slots, got %d",
                 (int)w.slot_elems.size(), d.n_slots);
    WIRE_REQUIRE(d.n_params >= 0 && (d.params || !d.n_params) && d.endconv, "sbc_score_wiring_bind: params or endconv is NULL");
    std::map<std::string, const void*> table;
    for (int i = 0; i < d.n_params; ++i) {
        WIRE_REQUIRE(d.params[i].name && d.params[i].ptr, "sbc_score_wiring_bind: parameter %d has no name or pointer", i);
        table[d.params[i].name] = d.params[i].ptr;
    }
    const bool f32 = d.conv_mode == 1, f16w = d.conv_mode == 2, f16x2 = d.conv_mode == 3;
    const Record* rec = nullptr;
    const char* lacks = nullptr;             // the first form `rec` reads that the table lacks
    auto need = [&](const std::string& key) -> const void* {      // what the record's kernel reads ("": the record has none)
        if (key.empty()) return nullptr;
        const auto it = table.find(key);
        if (it != table.end()) return it->second;
        if (!lacks) {
            lacks = key.c_str();
            set_error("sbc_score_wiring_bind: record '%s' reads '%s', which params lacks", rec->name.c_str(), lacks);
        }
        return nullptr;
    };
    auto calib = [&](const std::string& key) -> const void* {     // what only sbc_f16x2_calibrate writes a scale into: where the host has it
        const auto it = f16x2 ? table.find(key) : table.end();
        return it == table.end() ? nullptr : it->second;
    };
    auto slot = [&](int tensor) -> void* { return tensor < 0 ? nullptr : d.slots[w.tensors[tensor].slot]; };
    for (const Record& o : w.records) {
        rec = &o;
        sbc_op& r = *ops++;
        memset(&r, 0, sizeof(r));
        const Tensor& src = w.tensors[o.geom >= 0 ? o.geom : o.src];     // (statistics from tile moments: the image's dims)
        r.kind = o.kind; r.flags = o.flags | (o.side ? SBC_OP_SIDE : 0) | (o.join ? SBC_OP_JOIN : 0);
        r.B = d.batch; r.H = src.h; r.W = src.w; r.cin = src.c; r.cout = w.tensors[o.dst].c;
        r.ksize = o.ksize; r.dil = o.dil; r.tag = o.tag;
        r.lane = o.lane; r.signal = o.signal; r.wait[0] = o.wait0; r.wait[1] = o.wait1;
        r.in = slot(o.src); r.out = slot(o.dst); r.aux = slot(o.moments);
        r.res1 = slot(o.res1); r.res2 = slot(o.res2); r.up = slot(o.up);
        if (o.up >= 0) { r.up_h = w.tensors[o.up].h; r.up_w = w.tensors[o.up].w; }
        r.stats = o.norm_key.empty() ? slot(o.stats) : need(o.norm_key);     // SBC_PRO_NORM_SELF: the norm's (alpha | gamma | beta)
        r.bias = need(o.bias);
        const bool wino = o.ksize == 3 && o.dil == 1;
        switch (o.kind) {
        case SBC_OP_CONV:
            if (f32) {
                r.weight = need(o.weight);
                if (wino) r.weight_wino = need(o.weight + "#winograd");
            } else {
                r.weight_split = need(o.weight + "#split");
                if (wino) r.weight_wino_split = need(o.weight + "#winograd_split");
                r.flags |= f16w ? SBC_CONV_F16W : f16x2 ? SBC_CONV_F16X2 : 0;
            }
            // the exact modes: ELU keeps its relative accuracy for small inputs too
            if (d.conv_mode <= 1 && (o.flags & SBC_PRO_ELU)) r.flags |= SBC_PRO_ELU_ACC;
            break;
        case SBC_OP_CONV_PAIR: case SBC_OP_CONV_POOL: case SBC_OP_RES_BLOCK:     // (the fused kernels read the direct fp16 forms only)
            r.weight_split = need(o.weight + "#split");
            r.weight_wino_split = calib(o.weight + "#winograd_split");
            if (!o.weight2.empty()) {
                r.weight2_split = need(o.weight2 + "#split");
                r.weight2_wino_split = calib(o.weight2 + "#winograd_split");
            }
            r.bias2 = need(o.bias2); r.norm2 = need(o.norm2);
            r.flags |= f16w && o.kind != SBC_OP_RES_BLOCK ? SBC_CONV_F16W : SBC_CONV_F16X2;
            break;
        case SBC_OP_CONV_DOWN:               // the pooled stride-2 filters; the layers' unpooled forms for the calibration
            r.weight_split = need(o.weight + "#pool");
            r.weight2_split = need(o.weight2 + "#pool");
            r.bias2 = need(o.bias2);
            r.weight = calib(o.weight + "#split");
            r.weight_wino_split = calib(o.weight + "#winograd_split");
            r.weight_wino = calib(o.weight2 + "#split");
            r.flags |= SBC_CONV_F16X2;
            break;
        case SBC_OP_CHAIN: {
            WIRE_REQUIRE(chains, "sbc_score_wiring_bind: the wiring has SBC_OP_CHAIN records, chains is NULL");
            sbc_chain& ch = *chains++;
            memset(&ch, 0, sizeof(ch));
            ch.n_blocks = (int32_t)o.blocks.size();
            for (size_t k = 0; k < o.blocks.size(); ++k) {
                const Block& bl = o.blocks[k];
                ch.type[k] = bl.type;
                ch.w1[k] = need(bl.w1 + "#split"); ch.w2[k] = need(bl.w2 + "#split");
                if (bl.dil == 1) {           // (a dilated layer runs in no Winograd launch at any array size: its form gets no scale)
                    ch.w1_wino[k] = calib(bl.w1 + "#winograd_split"); ch.w2_wino[k] = calib(bl.w2 + "#winograd_split");
                }
                if (bl.type != SBC_CHAIN_RES) continue;
                ch.dil[k] = bl.dil;
                ch.bias1[k] = (const float*)need(bl.bias1); ch.bias2[k] = (const float*)need(bl.bias2);
                ch.norm1[k] = (const float*)need(bl.norm1); ch.norm2[k] = (const float*)need(bl.norm2);
                if (!bl.w3.empty()) { ch.w3[k] = need(bl.w3 + "#split"); ch.bias3[k] = (const float*)need(bl.bias3); }
            }
            r.ext = &ch;
            r.flags |= SBC_CONV_F16X2;
            break;
        }
        default:                             // begin / end convolution: torch layout; statistics: the norm's (alpha | gamma | beta)
            r.weight = need(o.weight);
            if (o.kind == SBC_OP_END_CONV) r.ext = d.endconv;
        }
        if (lacks) return SBC_ERR_INVALID;
    }
    return SBC_OK;
}

}  // namespace wire
}  // namespace sbc

// ---- the C ABI (include/sbc_hip.h) --------------------------------------------------------------------------------------------
struct sbc_score_wiring {
    sbc::wire::Wiring w;                     // owns every string the arrays below point at
    std::vector<sbc_wiring_tensor> tensors;
    std::vector<sbc_wiring_record> records;
    std::vector<sbc_wiring_block> blocks;
    std::vector<int64_t> slot_elems;
};

extern "C" {

int sbc_score_wiring_create(const sbc_score_wiring_desc* desc, sbc_score_wiring** out) {
    WIRE_REQUIRE(desc && out, "sbc_score_wiring_create: desc or out is NULL");
    sbc_score_wiring* s = new sbc_score_wiring();
    const int rc = sbc::wire::build(*desc, s->w);
    if (rc) {
        delete s;
        return rc;
    }
    auto str = [](const std::string& v) { return v.empty() ? nullptr : v.c_str(); };
    for (const auto& t : s->w.tensors) s->tensors.push_back({t.name.c_str(), t.h, t.w, t.c, t.slot});
    for (const auto& o : s->w.records) {
        sbc_wiring_record r = {o.kind, o.flags, o.ksize, o.dil, o.tag, o.src, o.dst, o.stats, o.res1, o.res2, o.up, o.moments, o.geom,
                               o.side, o.join, o.lane, o.signal, {o.wait0, o.wait1}, (int32_t)s->blocks.size(), (int32_t)o.blocks.size(),
                               o.name.c_str(), str(o.weight), str(o.bias), str(o.weight2), str(o.bias2), str(o.norm2), str(o.norm_key)};
        for (const auto& b : o.blocks)
            s->blocks.push_back({b.type, b.dil, b.w1.c_str(), b.w2.c_str(), str(b.bias1), str(b.bias2), str(b.norm1), str(b.norm2), str(b.w3), str(b.bias3)});
        s->records.push_back(r);
    }
    s->slot_elems.assign(s->w.slot_elems.begin(), s->w.slot_elems.end());
    *out = s;
    return SBC_OK;
}

int sbc_score_wiring_read(const sbc_score_wiring* s, sbc_score_wiring_view* view) {
    WIRE_REQUIRE(s && view, "sbc_score_wiring_read: handle or view is NULL");
    *view = {s->tensors.data(), s->records.data(), s->blocks.data(), s->slot_elems.data(), (int32_t)s->tensors.size(),
             (int32_t)s->records.size(), (int32_t)s->blocks.size(), (int32_t)s->slot_elems.size(), s->w.x, s->w.out,
             (int32_t)std::count_if(s->w.records.begin(), s->w.records.end(), [](const sbc::wire::Record& o) { return o.kind == SBC_OP_CHAIN; })};
    return SBC_OK;
}

int sbc_score_wiring_bind(const sbc_score_wiring* s, const sbc_score_bind_desc* desc, sbc_op* ops, sbc_chain* chains) {
    WIRE_REQUIRE(s && desc, "sbc_score_wiring_bind: handle or desc is NULL");
    return sbc::wire::bind(s->w, *desc, ops, chains);
}

void sbc_score_wiring_destroy(sbc_score_wiring* s) { delete s; }

}  // extern "C"
