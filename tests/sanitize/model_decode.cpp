// model_decode.cpp -- the stager's model device (see model_device.cpp: "device" memory is host memory, copies are
// memcpy, events and streams complete at once, the augment / mask entries write a function of the source bytes
// they read, any call can be told to fail) with the decode stages added, for the stager's encoded half
// (aeon_amd/csrc/stager_encoded.cpp; Makefile targets sanitize_stager_encoded / tsan_stager_encoded,
// tests/sanitize/stager_encoded_driver.cpp drives it).  The four decode entries write record i at
// dst_base + descs[i].offset: PNG, BMP / PNM and TIFF files through the library's own host decoders
// (aeon_decode_png / _pixmap / _tiff, linked as they are), a JPEG file as a pattern keyed by the file's hash
// (model_jpeg_pattern).  The model also keeps the host ranges that host-to-device copies uploaded and counts the
// files of a decode entry whose bytes one of those copies carried as well (model_double_uploads).
// This build links the real abi_host.cpp: aeon_hip_last_error is the library's.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>

#include "../../aeon_amd/csrc/error.hpp"
#include "../../include/aeon_hip.h"
#include "model_decode.hpp"

namespace {

std::mutex                  g_mu;
std::map<uintptr_t, size_t> g_pinned;  // hipHostMalloc blocks: base -> size
std::map<uintptr_t, size_t> g_uploads; // host ranges copied host-to-device: start -> the longest copy from it
long                        g_double_uploads = 0, g_copied_bytes = 0, g_file_bytes = 0;
struct Script {
    int  countdown = 0; // > 0: calls left until the failing one
    int  error     = 0;
    long calls     = 0;
};
std::map<std::string, Script> g_script;

// Counts the call and returns the error scripted for it (0: none).
int scripted(const char* fn)
{
    std::lock_guard<std::mutex> l(g_mu);
    Script& s = g_script[fn];
    s.calls++;
    if (s.countdown > 0 && --s.countdown == 0) return s.error;
    return 0;
}

#define MODEL_CALL(name)                                          \
    do {                                                          \
        if (const int e_ = scripted(name)) return (hipError_t)e_; \
    } while (0)

uint64_t mix(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001b3ull; }

int failed(const char* name, const char* what, int code)
{
    aeon_hip::set_last_error((std::string(name) + ": " + what).c_str());
    return code;
}

int model_batch(const char* name, uint64_t kind, int n, const aeon_img_desc* descs, const void* src_base,
                const aeon_aug_params* params, const aeon_out_desc* out, void* dst)
{
    if (const int e = scripted(name)) return failed(name, "scripted failure", e);
    if (n < 0 || !descs || !src_base || !params || !out || !dst) return failed(name, "null argument", AEON_HIP_EINVAL);
    for (int i = 0; i < n; i++)
        model_record_output(kind, (const uint8_t*)src_base + descs[i].offset, descs[i], params[i],
                            (uint8_t*)dst + (size_t)i * out->item_stride, out->item_stride);
    return 0;
}

// Did a host-to-device copy carry this file's bytes?  By address (the file lies in a copied range) or by content
// (its first bytes are found inside one).
bool uploaded_by_copy(const uint8_t* data, size_t size)
{
    const size_t                probe = std::min<size_t>(size, 48);
    std::lock_guard<std::mutex> l(g_mu);
    for (const auto& u : g_uploads) {
        const uint8_t* lo = (const uint8_t*)u.first;
        const uint8_t* hi = lo + u.second;
        if (data < hi && data + size > lo) return true;
        if (probe >= 16 && u.second >= probe)
            if (std::search(lo, hi, data, data + probe) != hi) return true;
    }
    return false;
}

int model_decode(const char* name, int format, int n, const void* const* data, const size_t* sizes, const int* modes,
                 const aeon_img_desc* descs, void* dst_base)
{
    if (const int e = scripted(name)) return failed(name, "scripted failure", e);
    if (n < 0 || !data || !sizes || !descs || !dst_base) return failed(name, "null argument", AEON_HIP_EINVAL);
    if (n > 512) return failed(name, "more than 512 files in one call", AEON_HIP_EINVAL);
    for (int i = 0; i < n; i++) {
        const bool twice = uploaded_by_copy((const uint8_t*)data[i], sizes[i]);
        {
            std::lock_guard<std::mutex> l(g_mu);
            g_double_uploads += twice ? 1 : 0;
            g_file_bytes += (long)sizes[i];
        }
        uint8_t*     dst    = (uint8_t*)dst_base + descs[i].offset;
        const size_t stride = (size_t)descs[i].stride;
        int          rc     = 0;
        if (format == AEON_FORMAT_JPEG) model_jpeg_pattern(data[i], sizes[i], descs[i], dst);
        else if (format == AEON_FORMAT_PNG) rc = aeon_decode_png(data[i], sizes[i], modes[i], dst, stride, nullptr);
        else if (format == AEON_FORMAT_PIXMAP) rc = aeon_decode_pixmap(data[i], sizes[i], modes[i], dst, stride, nullptr);
        else rc = aeon_decode_tiff(data[i], sizes[i], modes[i], dst, stride, nullptr);
        if (rc != 0) return rc;
    }
    return 0;
}

} // namespace

extern "C" {

// ---- the model's own interface (model_decode.hpp) ----
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
    g_uploads.clear();
    g_double_uploads = g_copied_bytes = g_file_bytes = 0;
}

long model_calls(const char* fn)
{
    std::lock_guard<std::mutex> l(g_mu);
    return g_script[fn].calls;
}

long model_double_uploads(void)
{
    std::lock_guard<std::mutex> l(g_mu);
    return g_double_uploads;
}

long model_copied_bytes(void)
{
    std::lock_guard<std::mutex> l(g_mu);
    return g_copied_bytes;
}

long model_file_bytes(void)
{
    std::lock_guard<std::mutex> l(g_mu);
    return g_file_bytes;
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

void model_jpeg_pattern(const void* data, size_t size, aeon_img_desc d, uint8_t* dst)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < size; i++) h = mix(h, ((const uint8_t*)data)[i]);
    uint64_t     x   = h | 1;
    const size_t row = (size_t)d.width * d.channels;
    for (int y = 0; y < d.height; y++)
        for (size_t k = 0; k < row; k++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            dst[(size_t)y * d.stride + k] = (uint8_t)(x >> 24);
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
        auto it = g_pinned.find((uintptr_t)p);
        if (it != g_pinned.end()) { // (uploads from the block are forgotten with it)
            g_uploads.erase(g_uploads.lower_bound(it->first), g_uploads.lower_bound(it->first + it->second));
            g_pinned.erase(it);
        }
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
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t)
{
    MODEL_CALL("hipMemcpyAsync");
    if (kind == hipMemcpyHostToDevice) {
        std::lock_guard<std::mutex> l(g_mu);
        size_t& len = g_uploads[(uintptr_t)src];
        len         = std::max(len, n);
        g_copied_bytes += (long)n;
    }
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
int aeon_hip_decode_jpeg_batch(aeon_hip_ctx*, int n, const void* const* data, const size_t* sizes, const aeon_img_desc* descs,
                               void* dst_base, void*)
{
    return model_decode("aeon_hip_decode_jpeg_batch", AEON_FORMAT_JPEG, n, data, sizes, nullptr, descs, dst_base);
}
int aeon_hip_decode_png_batch(aeon_hip_ctx*, int n, const void* const* data, const size_t* sizes, const int* modes,
                              const aeon_img_desc* descs, void* dst_base, void*)
{
    return model_decode("aeon_hip_decode_png_batch", AEON_FORMAT_PNG, n, data, sizes, modes, descs, dst_base);
}
int aeon_hip_decode_pixmap_batch(aeon_hip_ctx*, int n, const void* const* data, const size_t* sizes, const int* modes,
                                 const aeon_img_desc* descs, void* dst_base, void*)
{
    return model_decode("aeon_hip_decode_pixmap_batch", AEON_FORMAT_PIXMAP, n, data, sizes, modes, descs, dst_base);
}
int aeon_hip_decode_tiff_batch(aeon_hip_ctx*, int n, const void* const* data, const size_t* sizes, const int* modes,
                               const aeon_img_desc* descs, void* dst_base, void*)
{
    return model_decode("aeon_hip_decode_tiff_batch", AEON_FORMAT_TIFF, n, data, sizes, modes, descs, dst_base);
}
int aeon_hip_synchronize(aeon_hip_ctx*, void*)
{
    if (const int e = scripted("aeon_hip_synchronize")) return failed("aeon_hip_synchronize", "scripted failure", e);
    return 0;
}
int aeon_hip_release_stream(aeon_hip_ctx*, void*)
{
    (void)scripted("aeon_hip_release_stream");
    return 0;
}

} // extern "C"
