// model_device.cpp -- a test-only model of the HIP runtime and of the C ABI entries stager.cpp calls, so the
// stager's whole life (stage, launch, wait, window reuse, error paths) runs on the CPU under the sanitizers
// (Makefile targets sanitize_stager / tsan_stager; tests/sanitize/stager_driver.cpp drives it).  Unlike
// aeon_amd/csrc/sanitize/no_device.cpp, whose launches all fail, this device works: "device" memory is host
// memory, copies are memcpy, events and streams complete at once, and the two batch entries write, per record,
// a function of the source bytes they read through src_base + desc.offset and of the params
// (model_record_output below), which the driver recomputes.  Memory from hipHostMalloc is reported by
// hipPointerGetAttributes as mapped host memory whose device address is its host address.  Any entry can be
// told to fail its k-th call from now (model_fail_call).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>

#include "../../include/aeon_hip.h"
#include "model_device.hpp"

namespace {

std::mutex                 g_mu;
std::map<uintptr_t, size_t> g_pinned; // hipHostMalloc blocks: base -> size
struct Script {
    int  countdown = 0; // > 0: calls left until the failing one
    int  error     = 0;
    long calls     = 0;
};
std::map<std::string, Script> g_script;
thread_local std::string      g_last_error;

// Counts the call and returns the error scripted for it (0: none).
int scripted(const char* fn)
{
    std::lock_guard<std::mutex> l(g_mu);
    Script& s = g_script[fn];
    s.calls++;
    if (s.countdown > 0 && --s.countdown == 0) return s.error;
    return 0;
}

#define MODEL_CALL(name)                                      \
    do {                                                      \
        if (const int e_ = scripted(name)) return (hipError_t)e_; \
    } while (0)

uint64_t mix(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001b3ull; }

int model_batch(const char* name, uint64_t kind, int n, const aeon_img_desc* descs, const void* src_base,
                const aeon_aug_params* params, const aeon_out_desc* out, void* dst)
{
    if (const int e = scripted(name)) {
        g_last_error = std::string(name) + ": scripted failure";
        return e;
    }
    if (n < 0 || !descs || !src_base || !params || !out || !dst) {
        g_last_error = std::string(name) + ": null argument";
        return AEON_HIP_EINVAL;
    }
    for (int i = 0; i < n; i++)
        model_record_output(kind, (const uint8_t*)src_base + descs[i].offset, descs[i], params[i],
                            (uint8_t*)dst + (size_t)i * out->item_stride, out->item_stride);
    return 0;
}

} // namespace

extern "C" {

// ---- the model's own interface (model_device.hpp) ----
void model_fail_call(const char* fn, int kth, int error)
{
    std::lock_guard<std::mutex> l(g_mu);
    g_script[fn].countdown = kth;
    g_script[fn].error     = error;
}

void model_reset(void)
{
    std::lock_guard<std::mutex> l(g_mu);
    g_script.clear();
}

long model_calls(const char* fn)
{
    std::lock_guard<std::mutex> l(g_mu);
    return g_script[fn].calls;
}

void model_record_output(uint64_t kind, const uint8_t* src, aeon_img_desc d, aeon_aug_params p, uint8_t* out,
                         size_t item_stride)
{
    const size_t n = (size_t)d.stride * d.height;
    uint64_t     h = 0xcbf29ce484222325ull;
    h              = mix(h, kind);
    for (int32_t v : {d.width, d.height, d.stride, d.channels, d.elem_bytes, p.crop_x, p.crop_y, p.crop_w, p.crop_h,
                      p.out_w, p.out_h, p.flip, p.angle})
        h = mix(h, (uint32_t)v);
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        std::memcpy(&w, src + i, 8);
        h = mix(h, w);
    }
    for (; i < n; i++) h = mix(h, src[i]);
    const size_t head = item_stride >= 8 ? std::min(n, item_stride - 8) : 0;
    std::memcpy(out, src, head);
    if (item_stride >= 8) {
        std::memset(out + head, 0, item_stride - 8 - head);
        std::memcpy(out + item_stride - 8, &h, 8);
    }
}

// ---- HIP runtime ----
hipError_t hipMalloc(void** p, size_t n)
{
    MODEL_CALL("hipMalloc");
    *p = std::malloc(n ? n : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p)
{
    MODEL_CALL("hipFree");
    std::free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned int)
{
    MODEL_CALL("hipHostMalloc");
    *p = std::malloc(n ? n : 1);
    if (!*p) return hipErrorOutOfMemory;
    std::lock_guard<std::mutex> l(g_mu);
    g_pinned[(uintptr_t)*p] = n ? n : 1;
    return hipSuccess;
}
hipError_t hipHostFree(void* p)
{
    MODEL_CALL("hipHostFree");
    {
        std::lock_guard<std::mutex> l(g_mu);
        g_pinned.erase((uintptr_t)p);
    }
    std::free(p);
    return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* a, const void* p)
{
    MODEL_CALL("hipPointerGetAttributes");
    std::lock_guard<std::mutex> l(g_mu);
    auto it = g_pinned.upper_bound((uintptr_t)p);
    if (it == g_pinned.begin()) return hipErrorInvalidValue;
    --it;
    if ((uintptr_t)p >= it->first + it->second) return hipErrorInvalidValue; // pageable
    std::memset(a, 0, sizeof(*a));
    a->type          = hipMemoryTypeHost;
    a->hostPointer   = (void*)it->first;
    a->devicePointer = (void*)it->first;
    return hipSuccess;
}
hipError_t hipGetDevice(int* d)
{
    MODEL_CALL("hipGetDevice");
    *d = 0;
    return hipSuccess;
}
hipError_t hipSetDevice(int)
{
    MODEL_CALL("hipSetDevice");
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "model device: scripted failure"; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int)
{
    MODEL_CALL("hipStreamCreateWithFlags");
    *s = reinterpret_cast<hipStream_t>(new int(0));
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    MODEL_CALL("hipStreamDestroy");
    delete reinterpret_cast<int*>(s);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t)
{
    MODEL_CALL("hipStreamSynchronize");
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned)
{
    MODEL_CALL("hipEventCreateWithFlags");
    *e = reinterpret_cast<hipEvent_t>(new int(0));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    MODEL_CALL("hipEventDestroy");
    delete reinterpret_cast<int*>(e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t)
{
    MODEL_CALL("hipEventRecord");
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t)
{
    MODEL_CALL("hipEventSynchronize");
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t)
{
    MODEL_CALL("hipMemcpyAsync");
    std::memcpy(dst, src, n);
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind)
{
    MODEL_CALL("hipMemcpy");
    std::memcpy(dst, src, n);
    return hipSuccess;
}

// ---- the entries of include/aeon_hip.h the stager calls ----
int aeon_hip_augment_batch(aeon_hip_ctx*, int n, const aeon_img_desc* descs, const void* src_base,
                           const aeon_aug_params* params, const aeon_out_desc* out, void* dst, void*)
{
    return model_batch("aeon_hip_augment_batch", MODEL_KIND_AUGMENT, n, descs, src_base, params, out, dst);
}
int aeon_hip_mask_batch(aeon_hip_ctx*, int n, const aeon_img_desc* descs, const void* src_base,
                        const aeon_aug_params* params, const aeon_out_desc* out, void* dst, void*)
{
    return model_batch("aeon_hip_mask_batch", MODEL_KIND_MASK, n, descs, src_base, params, out, dst);
}
int aeon_hip_synchronize(aeon_hip_ctx*, void*)
{
    if (const int e = scripted("aeon_hip_synchronize")) {
        g_last_error = "aeon_hip_synchronize: scripted failure";
        return e;
    }
    return 0;
}
int aeon_hip_release_stream(aeon_hip_ctx*, void*)
{
    (void)scripted("aeon_hip_release_stream");
    return 0;
}
const char* aeon_hip_last_error(void) { return g_last_error.c_str(); }

} // extern "C"
