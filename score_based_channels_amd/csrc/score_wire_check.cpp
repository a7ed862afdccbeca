// `make check-wiring`: the wiring unit under the address and undefined-behaviour sanitizers.  A stand-alone host program: builds,
// reads and frees every wiring of the matrix tests/test_plan_golden_cpu.py checks (9 array sizes x 13 argument sets) through the C
// ABI, then every refusal.  It is linked with score_wire.cpp alone -- the two functions of api.hip that unit calls are defined here.
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

int failures = 0;

// create + read + walk every string and index + destroy; returns the status of create
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
    auto desc = [](int nt, int nr, const Set& s) { return sbc_score_wiring_desc{32, 2, nt, nr, s.flags, s.shapes, s.n_shapes, s.skip, s.n_skip}; };
    for (const auto& g : geometries)
        for (int k = 0; k < 13; ++k) {
            size_t n = 0;
            if (run(desc(g[0], g[1], sets[k]), &n)) { printf("FAIL: %dx%d set %d: %s\n", g[0], g[1], k, g_err); ++failures; }
            if (g[0] == 64 && g[1] == 16 && n != records_64x16[k]) { printf("FAIL: 64x16 set %d has %zu records\n", k, n); ++failures; }
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
    printf("%s: 117 wirings, 12 refusals, %d failures\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
