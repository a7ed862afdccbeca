// Host side of the *_create calls: the caller's sbc_tensor_ref[] by name, and the flat float image of a handle's parameters that is
// laid out on the host, uploaded once and freed with the handle.  `who` is the public function on whose behalf a message is written.
#pragma once
#include <map>
#include <string>
#include <vector>
#include "common.h"

namespace sbc {

class TensorIndex {
public:
    // SBC_OK, or SBC_ERR_INVALID with the error set for a ref without name or data.  A name given more than once keeps its last ref;
    // *duplicate (optional) is the first such name, or NULL: whether that is an error is the caller's decision.
    int build(const char* who, const sbc_tensor_ref* tensors, int n, const char** duplicate = nullptr) {
        who_ = who;
        if (duplicate) *duplicate = nullptr;
        for (int i = 0; i < n; ++i) {
            SBC_REQUIRE(tensors[i].name && tensors[i].data, "%s: tensor %d has no name or data", who, i);
            const bool fresh = by_name_.insert_or_assign(tensors[i].name, &tensors[i]).second;
            if (!fresh && duplicate && !*duplicate) *duplicate = tensors[i].name;
        }
        return SBC_OK;
    }
    // build() for a state dict that must name every tensor once: `what` is the message's noun ("tensor", "critic tensor")
    int build_unique(const char* who, const char* what, const sbc_tensor_ref* tensors, int n) {
        const char* twice = nullptr;
        const int rc = build(who, tensors, n, &twice);
        if (rc) return rc;
        SBC_REQUIRE(!twice, "%s: %s '%s' given twice", who, what, twice);
        return SBC_OK;
    }
    bool has(const std::string& name) const { return by_name_.count(name) != 0; }
    // the tensor's data, or NULL with the error set: no such tensor, or not `numel` elements
    const float* find(const std::string& name, int64_t numel) const {
        const auto it = by_name_.find(name);
        if (it == by_name_.end()) {
            set_error("%s: tensor '%s' missing from the state dict", who_, name.c_str());
            return nullptr;
        }
        if (it->second->numel != numel) {
            set_error("%s: tensor '%s' has %lld elements, expected %lld", who_, name.c_str(), (long long)it->second->numel, (long long)numel);
            return nullptr;
        }
        return it->second->data;
    }

private:
    const char* who_ = "";
    std::map<std::string, const sbc_tensor_ref*> by_name_;
};

struct ParamImage {
    std::vector<float> host;             // filled before upload(), released by it
    std::map<std::string, size_t> off;   // offsets of the entries reserved under a key
    float* dev = nullptr;
    int device = 0;                      // the device `dev` lives on

    // n zeroed floats behind what is there; every entry starts on a 16-byte boundary.  Offsets, not pointers: `host` grows.
    size_t take(size_t n) {
        const size_t at = host.size();
        host.resize(at + ((n + 3) & ~(size_t)3), 0.f);
        return at;
    }
    float* reserve(const std::string& key, size_t n) {
        const size_t o = off[key] = take(n);
        return host.data() + o;
    }
    bool has(const std::string& key) const { return off.count(key) != 0; }
    float* at(const std::string& key) { return host.data() + off.at(key); }
    const float* dev_at(const std::string& key) const {      // NULL: nothing was reserved under `key`
        const auto it = off.find(key);
        return it == off.end() ? nullptr : dev + it->second;
    }

    // copy the image to the current device; on failure nothing stays allocated
    int upload(const char* who) {
        hipError_t e = hipGetDevice(&device);
        if (e == hipSuccess) e = hipMalloc(&dev, host.size() * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_error("%s: upload of the parameters failed: %s", who, hipGetErrorString(e));
            release();
            return SBC_ERR_HIP;
        }
        std::vector<float>().swap(host);
        return SBC_OK;
    }
    void release() {
        if (dev) (void)hipFree(dev);
        dev = nullptr;
    }
    // a handle is used on the device its parameters were uploaded to
    int check_device(const char* who) const {
        int cur = 0;
        SBC_CHECK_HIP(hipGetDevice(&cur));
        SBC_REQUIRE(cur == device, "%s: the handle lives on device %d, the current device is %d", who, device, cur);
        return SBC_OK;
    }
};

}  // namespace sbc
