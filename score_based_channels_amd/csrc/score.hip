// sbc_score_*: the whole NCSNv2Deepest score network behind ONE C call, for hosts that are not Python.
//
// score_wire.cpp wires ncsnv2/models/ncsnv2.py:269-300 into ~150 fused operator records, shares activation storage between
// tensors with disjoint lifetimes and binds the records to a host's memory -- for this file and, through sbc_score_wiring_*, for the
// product's Python host (plan.py / scorenet.py).  This file packs the forms of the weights its one array size runs, allocates device
// memory and hands both to that binder, so that a C / C++ / Go / Rust host gets a
// score evaluation from (state_dict tensors, batch size): sbc_score_create -> sbc_score_buffers -> sbc_score_forward, or
// sbc_score_ops to extend the record list with SBC_OP_LANGEVIN / SBC_OP_STEP_INC into a full annealed-Langevin step plan
// (sbc_plan_create).  tests/test_gpu_capi.py holds packing and the choice of forms to the Python host: identical records,
// bit-identical outputs.
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "common.h"
#include "host_params.h"
#include "score_wire.h"

using Tn = sbc::wire::Tensor;
using POp = sbc::wire::Record;

struct sbc_score {
    sbc_score_desc desc;
    sbc::wire::Wiring w;                 // tensors, records, slot sizes, the indices of x and out
    std::vector<float*> slots;           // device, [B * slot_elems]
    sbc::ParamImage params;              // all parameters, packed
    float* sigmas = nullptr;             // device [num_classes]
    int64_t* labels = nullptr;           // device [B]
    sbc_endconv endc;
    std::vector<sbc_op> ops;
    std::vector<sbc_chain> chains;       // ext structs of the SBC_OP_CHAIN records (sized before the records point into it)
    sbc_plan* plan = nullptr;
};

namespace {

// ---- the steps of sbc_score_create behind the wiring, in the order they run -----------------------------------------------------

// 1. the wiring of this handle's flags behind the gates of its conv_mode and array size
int wire(sbc_score& s) {
    const sbc_score_desc& d = s.desc;
    sbc_score_wiring_desc wd;
    memset(&wd, 0, sizeof(wd));
    wd.ngf = d.ngf; wd.channels = d.channels; wd.nt = d.nt; wd.nr = d.nr; wd.conv_mode = d.conv_mode;
    wd.flags = d.flags & (SBC_SCORE_FOLD_STATS | SBC_SCORE_FUSE_PAIRS | SBC_SCORE_FUSE_RES | SBC_SCORE_FUSE_CHAIN | SBC_SCORE_FUSE_DOWN |
                          SBC_SCORE_FUSE_END | SBC_SCORE_SKIP_LANES);
    const int rc = sbc::wire::build(wd, s.w);
    if (rc) sbc::set_error("sbc_score_create: %s", std::string(sbc_last_error()).c_str());
    return rc;
}

// 2. parameters: one flat host image (16-byte aligned entries), packed by the library's own packers
int pack_params(sbc_score& s, const sbc::TensorIndex& sd) {
    const int conv_mode = s.desc.conv_mode;
    const bool f16w = conv_mode == 2, f16x2 = conv_mode == 3;
    sbc::ParamImage& im = s.params;
    std::vector<float> tmp;
    auto rounded = [&](const float* p, size_t n) {      // fp16 parameters for conv_mode f16w (module.half() semantics)
        if (!f16w) return p;
        tmp.assign(p, p + n);
        for (auto& v : tmp) v = (float)(_Float16)v;
        return (const float*)tmp.data();
    };
    auto norm = [&](const std::string& nkey, int c) {   // a norm's (alpha | gamma | beta), [3][C]; false: a tensor is missing
        if (nkey.empty() || im.has(nkey)) return true;
        for (int k = 0; k < 3; ++k) {
            const char* suffix[3] = {".alpha", ".gamma", ".beta"};
            const float* v = sd.find(nkey + suffix[k], c);
            if (!v) return false;
            if (k == 0) im.reserve(nkey, 3 * (size_t)c);
            memcpy(im.at(nkey) + (size_t)k * c, rounded(v, c), sizeof(float) * c);
        }
        return true;
    };
    auto u16 = [&](const std::string& key, size_t n_floats) { return (uint16_t*)im.reserve(key, n_floats); };
    for (const POp& o : s.w.records) {
        const Tn& src = s.w.tensors[o.geom >= 0 ? o.geom : o.src];
        const Tn& dst = s.w.tensors[o.dst];
        if (!norm(o.kind == SBC_OP_INORM_STATS ? o.weight : o.kind == SBC_OP_RES_BLOCK ? o.norm2 : o.norm_key, src.c)) return SBC_ERR_INVALID;
        for (const auto& bl : o.blocks)                      // the norms of the RES blocks of a CHAIN record
            if (!norm(bl.norm1, src.c) || !norm(bl.norm2, src.c)) return SBC_ERR_INVALID;
        if (o.kind == SBC_OP_INORM_STATS) continue;
        if (o.weight.empty() && o.blocks.empty()) continue;   // max pooling has no parameters
        const int k = o.ksize, cin = src.c, cout = dst.c;
        const size_t wn = (size_t)cout * cin * k * k;
        std::vector<std::string> wkeys{o.weight, o.weight2};
        for (const auto& bl : o.blocks) { wkeys.push_back(bl.w1); wkeys.push_back(bl.w2); wkeys.push_back(bl.w3); }
        for (const std::string& wkey : wkeys) {
            if (wkey.empty()) continue;
            if (o.kind == SBC_OP_CONV_DOWN) {
                // the pooled stride-2 filters: 3x3 -> 4x4 (conv2), 1x1 -> 2x2 (shortcut)   (scorenet.load_state_dict: '#pool')
                if (im.has(wkey + "#pool")) continue;
                const int kk = wkey == o.weight2 ? 1 : 3;
                const float* w2 = sd.find(wkey, (int64_t)cout * cin * kk * kk);
                if (!w2) return SBC_ERR_INVALID;
                sbc_pack_conv_weight_pooled_f16x2(w2, cout, cin, kk, u16(wkey + "#pool", sbc_f16x2_elems((kk + 1) * (kk + 1), cin, cout) / 2));
                continue;
            }
            if (im.has(wkey) || im.has(wkey + "#split")) continue;
            const float* w = sd.find(wkey, (int64_t)wn);
            if (!w) return SBC_ERR_INVALID;
            w = rounded(w, wn);
            const std::vector<float> wkeep(w, w + wn);
            if (o.kind == SBC_OP_CONV_PAIR || o.kind == SBC_OP_CONV_POOL || o.kind == SBC_OP_RES_BLOCK || o.kind == SBC_OP_CHAIN) {
                // the fused kernels read the direct fp16 forms only
                if (f16x2) sbc_pack_conv_weight_f16x2(wkeep.data(), cout, cin, k, u16(wkey + "#split", sbc_f16x2_elems(k * k, cin, cout) / 2));
                else sbc_pack_conv_weight_f16(wkeep.data(), cout, cin, k, u16(wkey + "#split", (wn + 1) / 2));
            } else if (o.kind != SBC_OP_CONV) {
                memcpy(im.reserve(o.weight, wn), wkeep.data(), sizeof(float) * wn);
            } else if (conv_mode == 1) {
                sbc_pack_conv_weight(wkeep.data(), cout, cin, k, im.reserve(o.weight, wn));
                if (k == 3) sbc_pack_conv_weight_winograd(wkeep.data(), cout, cin, im.reserve(o.weight + "#winograd", (size_t)cout * cin * 16));
            } else if (conv_mode == 0) {
                sbc_pack_conv_weight_split(wkeep.data(), cout, cin, k, u16(o.weight + "#split", wn * 3 / 2));
                if (k == 3) sbc_pack_conv_weight_winograd_split(wkeep.data(), cout, cin, u16(o.weight + "#winograd_split", (size_t)cout * cin * 16 * 3 / 2));
            } else if (f16x2) {
                sbc_pack_conv_weight_f16x2(wkeep.data(), cout, cin, k, u16(o.weight + "#split", sbc_f16x2_elems(k * k, cin, cout) / 2));
                if (k == 3) sbc_pack_conv_weight_winograd_f16x2(wkeep.data(), cout, cin, u16(o.weight + "#winograd_split", sbc_f16x2_elems(16, cin, cout) / 2));
            } else {
                sbc_pack_conv_weight_f16(wkeep.data(), cout, cin, k, u16(o.weight + "#split", (wn + 1) / 2));
                if (k == 3) sbc_pack_conv_weight_winograd_f16(wkeep.data(), cout, cin, u16(o.weight + "#winograd_split", (size_t)cout * cin * 16 / 2));
            }
        }
        std::vector<std::string> bkeys{o.bias, o.bias2};
        for (const auto& bl : o.blocks) { bkeys.push_back(bl.bias1); bkeys.push_back(bl.bias2); bkeys.push_back(bl.bias3); }
        for (const std::string& bkey : bkeys) {
            if (bkey.empty() || im.has(bkey)) continue;
            const float* bv = sd.find(bkey, cout);
            if (!bv) return SBC_ERR_INVALID;
            memcpy(im.reserve(bkey, cout), rounded(bv, cout), sizeof(float) * cout);
        }
    }
    return SBC_OK;
}

// 3. device memory: the parameter image, the noise levels, the labels, one buffer per activation slot
int allocate(sbc_score& s) {
    const sbc_score_desc& d = s.desc;
    int rc = s.params.upload("sbc_score_create");
    if (rc) return rc;
    hipError_t e;
    auto hip_fail = [&](const char* what) {
        sbc::set_error("sbc_score_create: %s failed: %s", what, hipGetErrorString(e));
        return SBC_ERR_HIP;
    };
    if ((e = hipMalloc((void**)&s.sigmas, d.num_classes * sizeof(float))) != hipSuccess) return hip_fail("hipMalloc(sigmas)");
    if ((e = hipMemcpy(s.sigmas, d.sigmas, d.num_classes * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return hip_fail("hipMemcpy(sigmas)");
    if ((e = hipMalloc((void**)&s.labels, d.batch * sizeof(int64_t))) != hipSuccess) return hip_fail("hipMalloc(labels)");
    if ((e = hipMemset(s.labels, 0, d.batch * sizeof(int64_t))) != hipSuccess) return hip_fail("hipMemset(labels)");
    s.slots.assign(s.w.slot_elems.size(), nullptr);
    for (size_t i = 0; i < s.w.slot_elems.size(); ++i)
        if ((e = hipMalloc((void**)&s.slots[i], (size_t)d.batch * s.w.slot_elems[i] * sizeof(float))) != hipSuccess)
            return hip_fail("hipMalloc(activation slot)");
    s.endc.sigmas = s.sigmas; s.endc.labels = s.labels; s.endc.sigma_of_step = nullptr; s.endc.step = nullptr;
    return SBC_OK;
}

// 4. records: the one binder (score_wire.cpp) over this handle's slots and whatever pack_params put into the image; and the plan
// that runs them
int bind_records(sbc_score& s) {
    std::vector<sbc_named_ptr> params;
    for (const auto& kv : s.params.off) params.push_back({kv.first.c_str(), s.params.dev + kv.second});
    std::vector<void*> slots(s.slots.begin(), s.slots.end());
    const sbc_score_bind_desc bd = {s.desc.batch, s.desc.conv_mode, slots.data(), (int32_t)slots.size(), params.data(), (int32_t)params.size(), &s.endc};
    s.ops.resize(s.w.records.size());
    s.chains.resize(std::count_if(s.w.records.begin(), s.w.records.end(), [](const POp& o) { return o.kind == SBC_OP_CHAIN; }));
    const int rc = sbc::wire::bind(s.w, bd, s.ops.data(), s.chains.data());
    if (rc) {
        sbc::set_error("sbc_score_create: %s", std::string(sbc_last_error()).c_str());
        return rc;
    }
    return sbc_plan_create(s.ops.data(), (int32_t)s.ops.size(), &s.plan);
}

// 5. conv_mode f16x2: per-layer activation scales (include/sbc_hip.h: sbc_f16x2_calibrate; scorenet.ScoreNet._ensure_calibrated), one
// pass over the fixed calibration input in the first sample of the x buffer
int calibrate(sbc_score& s) {
    const size_t n = (size_t)s.desc.nt * s.desc.nr * s.desc.channels;
    std::vector<float> pat(n);
    const int rc = sbc_f16x2_calibration_input(pat.data(), (int64_t)n);
    if (rc) return rc;
    if (hipMemcpy(s.slots[s.w.tensors[s.w.x].slot], pat.data(), n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        sbc::set_error("sbc_score_create: upload of the calibration input failed");
        return SBC_ERR_HIP;
    }
    return sbc_f16x2_calibrate(s.ops.data(), (int32_t)s.ops.size(), nullptr);
}

}  // namespace

extern "C" {

int sbc_score_create(const sbc_score_desc* d, const sbc_tensor_ref* tensors, int32_t n_tensors, sbc_score** out) {
    SBC_REQUIRE(d && tensors && out && n_tensors > 0, "sbc_score_create: bad arguments");
    SBC_REQUIRE(d->ngf == 32 && d->channels == 2, "sbc_score_create: kernels are instantiated for ngf = 32, 2 channels");
    SBC_REQUIRE(d->nt > 0 && d->nr > 0 && d->nt % 8 == 0 && d->nr % 8 == 0,
                "sbc_score_create: Nt and Nr must be multiples of 8 (three 2x mean pools), got %dx%d", d->nt, d->nr);
    SBC_REQUIRE(d->batch > 0 && d->conv_mode >= 0 && d->conv_mode <= 3 && d->sigmas && d->num_classes > 0,
                "sbc_score_create: batch, conv_mode in {0 bf16x3, 1 f32, 2 f16w, 3 f16x2}, sigmas required");
    SBC_REQUIRE(!(d->flags & SBC_SCORE_FUSE_RES) || d->conv_mode == 3, "sbc_score_create: SBC_SCORE_FUSE_RES needs conv_mode 3 (f16x2)");
    SBC_REQUIRE(!(d->flags & SBC_SCORE_FUSE_CHAIN) || d->conv_mode == 3, "sbc_score_create: SBC_SCORE_FUSE_CHAIN needs conv_mode 3 (f16x2)");
    SBC_REQUIRE(!(d->flags & SBC_SCORE_FUSE_DOWN) || d->conv_mode == 3, "sbc_score_create: SBC_SCORE_FUSE_DOWN needs conv_mode 3 (f16x2)");
    SBC_REQUIRE(!(d->flags & SBC_SCORE_FUSE_PAIRS) || d->conv_mode >= 2,
                "sbc_score_create: SBC_SCORE_FUSE_PAIRS needs the fp16 weight forms (conv_mode 2 or 3)");
    sbc::TensorIndex sd;                     // (a name given twice: the last ref counts)
    int rc = sd.build("sbc_score_create", tensors, n_tensors);
    if (rc) return rc;
    sbc_score* s = new sbc_score();
    s->desc = *d;
    rc = wire(*s);
    if (!rc) rc = pack_params(*s, sd);
    if (!rc) rc = allocate(*s);
    if (!rc) rc = bind_records(*s);
    if (!rc && d->conv_mode == 3) rc = calibrate(*s);
    if (rc) {
        sbc_score_destroy(s);
        return rc;
    }
    *out = s;
    return SBC_OK;
}

int sbc_score_buffers(sbc_score* s, float** x, float** out, int64_t** labels) {
    SBC_REQUIRE(s, "sbc_score_buffers: handle is NULL");
    if (x) *x = s->slots[s->w.tensors[s->w.x].slot];
    if (out) *out = s->slots[s->w.tensors[s->w.out].slot];
    if (labels) *labels = s->labels;
    return SBC_OK;
}

int sbc_score_ops(sbc_score* s, const sbc_op** ops, int32_t* n_ops) {
    SBC_REQUIRE(s && ops && n_ops, "sbc_score_ops: bad arguments");
    *ops = s->ops.data();
    *n_ops = (int32_t)s->ops.size();
    return SBC_OK;
}

int sbc_score_level_source(sbc_score* s, const float* sigma_of_step, const int32_t* step) {
    SBC_REQUIRE(s, "sbc_score_level_source: handle is NULL");
    SBC_REQUIRE((sigma_of_step == nullptr) == (step == nullptr), "sbc_score_level_source: both pointers or neither");
    s->endc.sigma_of_step = sigma_of_step;
    s->endc.step = step;
    s->endc.labels = step ? nullptr : s->labels;
    // the score plan holds a copy of the end-conv extension: rebuild it
    sbc_plan_destroy(s->plan);
    s->plan = nullptr;
    return sbc_plan_create(s->ops.data(), (int32_t)s->ops.size(), &s->plan);
}

int sbc_score_forward(sbc_score* s, void* stream) {
    SBC_REQUIRE(s && s->plan, "sbc_score_forward: handle is NULL");
    return sbc_plan_run(s->plan, stream, 1, 0);
}

void sbc_score_destroy(sbc_score* s) {
    if (!s) return;
    if (s->plan) sbc_plan_destroy(s->plan);
    for (float* p : s->slots) if (p) (void)hipFree(p);
    s->params.release();
    if (s->sigmas) (void)hipFree(s->sigmas);
    if (s->labels) (void)hipFree(s->labels);
    delete s;
}

}  // extern "C"
