// `make check-wiring`: the wiring unit under the address and undefined-behaviour sanitizers.  A stand-alone host program: builds,
// reads and frees every wiring of the matrix tests/test_plan_golden_cpu.py checks (9 array sizes x 13 argument sets) through the C
// ABI and binds each one, in every conv_mode that can run it, to a table of every packed form and to the table of a host that packs
// for one array size; then the gates of a conv_mode and every refusal.  It is linked with score_wire.cpp alone -- the two functions of
// api.hip that unit calls are defined here.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "score_wire.h"

static char g_err[512] = "";
namespace sbc {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace sbc
extern "C" const char* sbc_last_error(void) { return g_err; }

namespace {

int failures = 0, bindings = 0;

// sbc_score_wiring_bind in conv_mode `mode` over fake buffers (nothing is dereferenced): every slot and every packed form is a cell of
// an arena, and every pointer of every record must be NULL or lie in the arena it belongs to.  `lean`: the table of a host with this
// one array size, which packs only what its records run (sbc_score_create); otherwise every form of every layer (scorenet.py).
void bind_check(const sbc_score_wiring* h, const sbc_score_wiring_view& v, int mode, bool lean, const char* drop = nullptr) {
    std::vector<std::string> names;
    auto add = [&](const char* key, const char* form) { if (key && std::string(key) + form != (drop ? drop : "")) names.push_back(std::string(key) + form); };
    auto fused_layer = [&](const char* w) { add(w, "#split"); if (!lean) add(w, "#winograd_split"); };
    for (int i = 0; i < v.n_records; ++i) {
        const sbc_wiring_record& r = v.records[i];
        for (const char* k : {r.bias, r.bias2, r.norm2, r.norm_key}) add(k, "");
        if (r.kind == SBC_OP_CONV) {
            add(r.weight, mode == 1 ? "" : "#split");
            if (r.ksize == 3) add(r.weight, mode == 1 ? "#winograd" : "#winograd_split");
        } else if (r.kind == SBC_OP_CONV_DOWN) {
            for (const char* w : {r.weight, r.weight2}) { add(w, "#pool"); if (!lean) fused_layer(w); }
        } else if (r.kind == SBC_OP_CONV_PAIR || r.kind == SBC_OP_CONV_POOL || r.kind == SBC_OP_RES_BLOCK) {
            fused_layer(r.weight); fused_layer(r.weight2);
        } else {
            add(r.weight, "");
        }
        for (int k = 0; k < r.n_blocks; ++k) {
            const sbc_wiring_block& b = v.blocks[r.first_block + k];
            for (const char* w : {b.w1, b.w2, b.w3}) fused_layer(w);
            for (const char* s : {b.bias1, b.bias2, b.bias3, b.norm1, b.norm2}) add(s, "");
        }
    }
    std::vector<float> param_mem(4 * names.size() + 4), slot_mem(4 * (size_t)v.n_slots + 4);
    std::vector<sbc_named_ptr> params;
    for (size_t i = 0; i < names.size(); ++i) params.push_back({names[i].c_str(), &param_mem[4 * i]});
    std::vector<void*> slots;
    for (int i = 0; i < v.n_slots; ++i) slots.push_back(&slot_mem[4 * i]);
    std::vector<sbc_op> ops(v.n_records);
    std::vector<sbc_chain> chains(v.n_chains);
    const sbc_endconv endc = {};
    const sbc_score_bind_desc bd = {3, mode, slots.data(), v.n_slots, params.data(), (int32_t)params.size(), &endc};
    const int rc = sbc_score_wiring_bind(h, &bd, ops.data(), chains.data());
    ++bindings;
    if (drop) {
        if (rc != SBC_ERR_INVALID || !strstr(g_err, drop) || !strstr(g_err, "record '")) { printf("FAIL: bind without %s: %d '%s'\n", drop, rc, g_err); ++failures; }
        return;
    }
    if (rc) { printf("FAIL: bind (mode %d, lean %d): %s\n", mode, lean, g_err); ++failures; return; }
    auto fail = [&](int i, const char* what) { printf("FAIL: record %d (%s), mode %d, lean %d: %s\n", i, v.records[i].name, mode, lean, what); ++failures; };
    auto in = [](const void* p, const std::vector<float>& mem) { return (const float*)p >= mem.data() && (const float*)p < mem.data() + mem.size(); };
    auto param = [&](const void* p) { return !p || in(p, param_mem); };
    auto slot = [&](const void* p) { return !p || in(p, slot_mem); };
    int n_chains = 0;
    for (int i = 0; i < v.n_records; ++i) {
        const sbc_op& o = ops[i];
        const sbc_wiring_record& r = v.records[i];
        if (o.kind != r.kind || o.B != 3 || !o.in || !o.out) fail(i, "kind, batch, in or out");
        for (const void* p : {o.in, (const void*)o.out, (const void*)o.aux, o.res1, o.res2, o.up}) if (!slot(p)) fail(i, "an activation pointer outside the slots");
        if (!(r.norm_key ? o.stats && param(o.stats) : slot(o.stats))) fail(i, "stats");
        for (const void* p : {o.weight, o.bias, o.weight_wino, o.weight_split, o.weight_wino_split, o.weight2_split, o.bias2, o.norm2, o.weight2_wino_split})
            if (!param(p)) fail(i, "a parameter pointer outside the table");
        if (o.grad || o.wgrad || o.bgrad || o.calib) fail(i, "a training field is set");
        const bool calib = mode == 3 && !lean;          // the forms that ride along for sbc_f16x2_calibrate: bound where the table has them
        if (o.kind == SBC_OP_CONV_PAIR || o.kind == SBC_OP_RES_BLOCK) { if (calib != (o.weight_wino_split && o.weight2_wino_split)) fail(i, "calibration-only forms"); }
        if (o.kind == SBC_OP_CONV_POOL && calib != (o.weight_wino_split != nullptr)) fail(i, "calibration-only form");
        if (o.kind == SBC_OP_CONV_DOWN && calib != (o.weight && o.weight_wino && o.weight_wino_split)) fail(i, "calibration-only forms");
        if (o.kind == SBC_OP_CHAIN) {
            if (o.ext != &chains[n_chains]) { fail(i, "ext is not the next sbc_chain"); continue; }
            const sbc_chain& ch = chains[n_chains++];
            if (ch.n_blocks != r.n_blocks) fail(i, "n_blocks");
            for (int k = 0; k < SBC_CHAIN_MAX_BLOCKS; ++k) {
                for (const void* p : {ch.w1[k], ch.w2[k], ch.w1_wino[k], ch.w2_wino[k], ch.w3[k], (const void*)ch.bias1[k], (const void*)ch.bias2[k],
                                      (const void*)ch.bias3[k], (const void*)ch.norm1[k], (const void*)ch.norm2[k]})
                    if (!param(p) || (p && k >= ch.n_blocks)) fail(i, "a chain pointer outside the table or behind the last block");
                if (k < ch.n_blocks && (!ch.w1[k] || !ch.w2[k] || (calib && ch.dil[k] <= 1) != (ch.w1_wino[k] && ch.w2_wino[k]))) fail(i, "a chain block's forms");
            }
        } else if (o.ext != (o.kind == SBC_OP_END_CONV ? &endc : nullptr)) {
            fail(i, "ext");
        }
    }
    if (n_chains != v.n_chains) { printf("FAIL: %d chains bound, the view says %d\n", n_chains, v.n_chains); ++failures; }
}

// create + read + walk every string and index + bind in every conv_mode that runs the flags + destroy; returns the status of create
int run(sbc_score_wiring_desc d, size_t* n_records = nullptr) {
    sbc_score_wiring* h = nullptr;
    const int rc = sbc_score_wiring_create(&d, &h);
    if (rc) {
        if (h) { printf("FAIL: a handle came back with status %d\n", rc); ++failures; }
        return rc;
    }
    sbc_score_wiring_view v;
    if (sbc_score_wiring_read(h, &v)) { printf("FAIL: read: %s\n", g_err); ++failures; }
    size_t chars = 0;
    auto len = [&](const char* s) { if (s) chars += strlen(s); };
    // (a tensor that a merged chain keeps on chip is still listed, without a slot: no record may name it)
    auto tensor = [&](int32_t i) { if (i < -1 || i >= v.n_tensors || (i >= 0 && v.tensors[i].slot < 0)) { printf("FAIL: tensor index %d\n", i); ++failures; } };
    for (int i = 0; i < v.n_tensors; ++i) {
        const sbc_wiring_tensor& t = v.tensors[i];
        len(t.name);
        if (t.slot < -1 || t.slot >= v.n_slots || (t.slot >= 0 && v.slot_elems[t.slot] != (int64_t)t.h * t.w * t.c)) { printf("FAIL: slot of tensor %d\n", i); ++failures; }
    }
    for (int i = 0; i < v.n_records; ++i) {
        const sbc_wiring_record& r = v.records[i];
        for (const char* s : {r.name, r.weight, r.bias, r.weight2, r.bias2, r.norm2, r.norm_key}) len(s);
        for (int32_t t : {r.src, r.dst, r.stats, r.res1, r.res2, r.up, r.moments, r.geom}) tensor(t);
        if (r.first_block < 0 || r.first_block + r.n_blocks > v.n_blocks) { printf("FAIL: blocks of record %d\n", i); ++failures; }
        for (int k = 0; k < r.n_blocks; ++k) {
            const sbc_wiring_block& b = v.blocks[r.first_block + k];
            for (const char* s : {b.w1, b.w2, b.bias1, b.bias2, b.norm1, b.norm2, b.w3, b.bias3}) len(s);
        }
    }
    tensor(v.x); tensor(v.out);
    if (!chars) { printf("FAIL: no names\n"); ++failures; }
    if (n_records) *n_records = (size_t)v.n_records;
    const int fused = SBC_SCORE_FUSE_RES | SBC_SCORE_FUSE_CHAIN | SBC_SCORE_FUSE_DOWN;
    for (int mode = d.flags & fused ? 3 : d.flags & SBC_SCORE_FUSE_PAIRS ? 2 : 0; mode <= 3; ++mode)
        for (bool lean : {false, true}) bind_check(h, v, mode, lean);
    if (d.flags & fused)                     // one form of each kind that a kernel reads, missing: refused with the record and the form
        for (const char* drop : {"res1.0.conv1.weight#split", "res1.0.normalize1", "res2.0.conv1.bias", "begin_conv.weight", "normalizer"})
            bind_check(h, v, 3, true, drop);
    sbc_score_wiring_destroy(h);
    return rc;
}

void refuses(const char* what, sbc_score_wiring_desc d, const char* text) {
    g_err[0] = 0;
    if (run(d) != SBC_ERR_INVALID || !strstr(g_err, text)) { printf("FAIL: %s: '%s'\n", what, g_err); ++failures; }
}

}  // namespace

int main() {
    const int geometries[9][2] = {{64, 16}, {256, 64}, {32, 32}, {32, 16}, {128, 8}, {24, 8}, {48, 16}, {8, 8}, {16, 64}};
    const int FOLD = SBC_SCORE_FOLD_STATS, PAIRS = SBC_SCORE_FUSE_PAIRS, RES = SBC_SCORE_FUSE_RES, CHAIN = SBC_SCORE_FUSE_CHAIN;
    const int SIX = FOLD | PAIRS | RES | CHAIN | SBC_SCORE_FUSE_DOWN | SBC_SCORE_FUSE_END, LANES = SBC_SCORE_SKIP_LANES;
    const int32_t f16w[10] = {32, 16, 32, 32, 32, 64, 64, 16, 64, 32};
    const sbc_skip_branch three[3] = {{"refine5.adapt_convs.0.", "res3.1.", 1}, {"refine4.adapt_convs.0.", "res3.1.", 2}, {"refine3.adapt_convs.0.", "res3.1.", 3}};
    struct Set { int flags; const int32_t* shapes; int n_shapes; const sbc_skip_branch* skip; int n_skip; };
    const Set sets[13] = {{0}, {FOLD}, {PAIRS}, {PAIRS | FOLD, f16w, 5}, {FOLD | PAIRS | RES}, {PAIRS | CHAIN}, {SIX}, {SIX | LANES}, {FOLD | LANES},
                          {FOLD | PAIRS | RES | SBC_SCORE_FUSE_END | SBC_WIRING_OVERLAP}, {SBC_WIRING_OVERLAP}, {SBC_WIRING_PRIVATE_SLOTS},
                          {SIX | LANES, nullptr, 0, three, 3}};
    const size_t records_64x16[13] = {150, 136, 143, 129, 125, 65, 54, 54, 136, 124, 150, 150, 54};
    auto desc = [](int nt, int nr, const Set& s, int conv_mode = -1) { return sbc_score_wiring_desc{32, 2, nt, nr, s.flags, s.shapes, s.n_shapes, s.skip, s.n_skip, conv_mode}; };
    for (const auto& g : geometries)
        for (int k = 0; k < 13; ++k) {
            size_t n = 0;
            if (run(desc(g[0], g[1], sets[k]), &n)) { printf("FAIL: %dx%d set %d: %s\n", g[0], g[1], k, g_err); ++failures; }
            if (g[0] == 64 && g[1] == 16 && n != records_64x16[k]) { printf("FAIL: 64x16 set %d has %zu records\n", k, n); ++failures; }
        }
    // the gates of a conv_mode: folded statistics go in mode 1 and off powers of two, mode 2 has the longer list of pair shapes
    {
        size_t plain = 0, folded = 0, n = 0;
        run(desc(64, 16, sets[0]), &plain); run(desc(64, 16, sets[1]), &folded);
        for (int mode = 0; mode <= 3; ++mode)
            if (run(desc(64, 16, sets[1], mode), &n) || n != (mode == 1 ? plain : folded)) { printf("FAIL: fold gate, mode %d: %zu records\n", mode, n); ++failures; }
        run(desc(48, 16, sets[0]), &plain);
        if (run(desc(48, 16, sets[1], 0), &n) || n != plain) { printf("FAIL: fold gate at 48x16: %zu records\n", n); ++failures; }
        run(desc(256, 64, sets[3]), &folded);
        if (run(desc(256, 64, Set{PAIRS | FOLD}, 2), &n) || n != folded) { printf("FAIL: pair shapes of mode 2: %zu records\n", n); ++failures; }
        refuses("conv_mode", desc(64, 16, sets[0], 4), "conv_mode");
    }
    // the refusals (tests/test_plan_golden_cpu.py: REFUSALS)
    auto with_skip = [&](const std::vector<sbc_skip_branch>& v) { return desc(64, 16, Set{LANES, nullptr, 0, v.data(), (int)v.size()}); };
    refuses("Nt", desc(12, 4, sets[0]), "multiples of 8");
    refuses("Nr", desc(64, 20, sets[0]), "multiples of 8");
    refuses("lanes + overlap", desc(64, 16, Set{LANES | SBC_WIRING_OVERLAP}), "do not mix");
    refuses("run", with_skip({{"res1.0.conv", "begin_conv", 1}}), "not one contiguous run");
    refuses("lane 4", with_skip({{"refine5.adapt_convs.0.", "res3.1.", 4}}), "bad lane 4");
    refuses("lane 0", with_skip({{"refine5.adapt_convs.0.", "res3.1.", 0}}), "bad lane 0");
    refuses("anchor", with_skip({{"refine5.adapt_convs.0.", "nope.", 1}}), "not found in front of it");
    refuses("third wait", with_skip({{"res2.0.conv2", "res2.0.shortcut", 1}, {"res2.0.normalize2", "res2.0.conv1", 2}, {"res2.0.shortcut", "res2.0.normalize2", 3}}),
            "already waits for two events");
    refuses("twice", with_skip({{"refine5.adapt_convs.0.", "res3.1.", 1}, {"refine5.adapt_convs.0.1_1", "res3.1.", 1}}), "already on a lane");
    refuses("not ready", with_skip({{"refine4.adapt_convs.1.", "res3.1.", 1}}), "does not have yet");
    refuses("NULL prefix", with_skip({{nullptr, "res3.1.", 1}}), "lacks its branch or anchor");
    {   // more than SBC_MAX_EVENTS events: single-record branches behind the record in front of them, two events each
        sbc::wire::Wiring w;
        if (sbc::wire::build(desc(64, 16, sets[0]), w)) { printf("FAIL: %s\n", g_err); ++failures; }
        std::vector<sbc_skip_branch> many;
        for (size_t k = 2; k < w.records.size() && many.size() < 33; k += 3) {
            int matches = 0;
            for (const auto& o : w.records) matches += o.name.compare(0, w.records[k].name.size(), w.records[k].name) == 0;
            if (matches == 1) many.push_back({w.records[k].name.c_str(), w.records[k - 1].name.c_str(), 1});
        }
        refuses("events", with_skip(many), "more than 64 lane events");
        many.pop_back();
        if (many.size() != 32 || run(with_skip(many))) { printf("FAIL: 32 branches: %s\n", g_err); ++failures; }
    }
    if (sbc_score_wiring_create(nullptr, nullptr) != SBC_ERR_INVALID || sbc_score_wiring_read(nullptr, nullptr) != SBC_ERR_INVALID) { printf("FAIL: NULL arguments\n"); ++failures; }
    sbc_score_wiring_destroy(nullptr);
    printf("%s: 117 wirings, %d bindings, 13 refusals, %d failures\n", failures ? "FAILED" : "ok", bindings, failures);
    return failures ? 1 : 0;
}
