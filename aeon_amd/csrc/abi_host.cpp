// abi_host.cpp -- the host-only entries of the C ABI (include/aeon_hip.h): the param factory, the PNG and
// pixmap decoders, the JPEG header and entropy probes, aeon's rounding and scale helpers, and the thread-local text
// behind aeon_hip_last_error.  No entry touches a device, and nothing here needs the runtime: the sanitizer
// builds link this file as it is.
#include <climits>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"
#include "error.hpp"
#include "jpeg.hpp"
#include "json.hpp"
#include "param_factory.hpp"
#include "pixmap.hpp"
#include "tiff.hpp"
#include "png.hpp"
#include "rcnn_host.hpp"

using namespace aeon_hip;

struct aeon_param_factory {
    param_factory f;
    std::mutex    mu; // make_params calls are serialised (the lighting normal_distribution caches a draw)
    explicit aeon_param_factory(const Json& j) : f(j) {}
};

namespace {
thread_local std::string g_err;
using TrackedEngine = tracked_engine; // rcnn_host.hpp
} // namespace

void aeon_hip::set_last_error(const char* what) { g_err = what; }

extern "C" {

int aeon_param_factory_create(const char* aug_json, aeon_param_factory** out)
{
    return guarded([&] {
        if (!out) fail(AEON_HIP_EINVAL, "null out");
        Json j = aug_json && *aug_json ? Json::parse(aug_json) : Json();
        *out   = new aeon_param_factory(j);
        return 0;
    });
}

int aeon_param_factory_destroy(aeon_param_factory* f)
{
    delete f;
    return 0;
}

int aeon_make_params(aeon_param_factory* f, uint32_t* state, int in_w, int in_h, int out_w, int out_h,
                     aeon_aug_params* out)
{
    return guarded([&] {
        if (!f || !state || !out) fail(AEON_HIP_EINVAL, "null argument");
        std::lock_guard<std::mutex> lock(f->mu);
        TrackedEngine eng(*state);
        f->f.make_params(eng, in_w, in_h, out_w, out_h, out);
        *state = eng.last;
        return 0;
    });
}

int aeon_make_ssd_params(aeon_param_factory* f, uint32_t* state, int in_w, int in_h, int out_w, int out_h,
                         const float* boxes, int n_boxes, aeon_aug_params* out)
{
    return guarded([&] {
        if (!f || !state || !out || n_boxes < 0 || (n_boxes > 0 && !boxes)) fail(AEON_HIP_EINVAL, "null argument");
        std::lock_guard<std::mutex> lock(f->mu);
        TrackedEngine eng(*state);
        f->f.make_ssd_params(eng, in_w, in_h, out_w, out_h, boxes, n_boxes, out);
        *state = eng.last;
        return 0;
    });
}

int aeon_param_factory_emit(aeon_param_factory* f, int* type, float* min_overlap)
{
    return guarded([&] {
        if (!f || !type || !min_overlap) fail(AEON_HIP_EINVAL, "null argument");
        *type        = f->f.emit_type();
        *min_overlap = f->f.emit_constraint_min_overlap;
        return 0;
    });
}

int aeon_png_info(const void* data, size_t size, int* width, int* height, int* bit_depth, int* color_type)
{
    return guarded([&] {
        if (!data || !width || !height || !bit_depth || !color_type) fail(AEON_HIP_EINVAL, "null argument");
        png_header(data, size, width, height, bit_depth, color_type);
        return 0;
    });
}

int aeon_decode_png(const void* data, size_t size, int mode, void* dst, size_t stride, int* elem_bytes)
{
    return guarded([&] {
        if (!data || !dst) fail(AEON_HIP_EINVAL, "null argument");
        if (mode < AEON_PNG_BGR8 || mode > AEON_PNG_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown PNG decode mode");
        int w, h, depth, ctype;
        png_header(data, size, &w, &h, &depth, &ctype);
        const size_t eb = (mode == AEON_PNG_ANYDEPTH && depth == 16 && ctype != 3) ? 2 : 1;
        if (stride < (size_t)w * (mode == AEON_PNG_BGR8 ? 3 : 1) * eb) fail(AEON_HIP_EINVAL, "stride too small");
        png_decode(data, size, mode, dst, stride, elem_bytes);
        return 0;
    });
}

int aeon_png_host_stage(const void* data, size_t size, int mode, int* gpu_route, int64_t* staged_bytes)
{
    return guarded([&] {
        if (!data || !gpu_route || !staged_bytes) fail(AEON_HIP_EINVAL, "null argument");
        if (mode < AEON_PNG_BGR8 || mode > AEON_PNG_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown PNG decode mode");
        PngPlan P;
        png_plan(data, size, mode, P);
        *gpu_route = P.route;
        if (P.route) {
            PngJob               J;
            std::vector<uint8_t> comp(P.clen + 8);
            png_stage(data, size, mode, P, J, comp.data());
            *staged_bytes = (int64_t)(((P.clen + 7) & ~(size_t)7) + sizeof(PngJob));
        } else {
            const size_t         stride = (size_t)P.w * P.channels * P.elem_bytes;
            std::vector<uint8_t> px(stride * P.h);
            png_decode(data, size, mode, px.data(), stride, nullptr);
            *staged_bytes = (int64_t)px.size();
        }
        return 0;
    });
}

int aeon_png_decoder_route(const void* data, size_t size, int* device)
{
    return guarded([&] {
        if (!data || !device) fail(AEON_HIP_EINVAL, "null argument");
        *device = png_routed(data, size) ? 1 : 0;
        return 0;
    });
}

int aeon_png_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride)
{
    return guarded([&] {
        if (!data || !dst) fail(AEON_HIP_EINVAL, "null argument");
        if (mode < AEON_PNG_BGR8 || mode > AEON_PNG_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown PNG decode mode");
        PngPlan P;
        png_plan(data, size, mode, P);
        if (stride < (size_t)P.w * P.channels * P.elem_bytes || stride > INT32_MAX) fail(AEON_HIP_EINVAL, "stride too small");
        const int r = png_gpu_emulate(data, size, mode, dst, stride);
        if (r == 0) fail(AEON_HIP_EUNSUPPORTED, "PNG: the file is not routed to the device (interlaced, or too wide)");
        if (r < 0) fail(AEON_HIP_EDEVICE, "PNG: image data corrupt or truncated (GPU stage)");
        return 0;
    });
}

int aeon_pixmap_info(const void* data, size_t size, int* width, int* height, int* bit_depth, int* channels, int* format)
{
    return guarded([&] {
        if (!data || !width || !height || !bit_depth || !channels || !format) fail(AEON_HIP_EINVAL, "null argument");
        pixmap_header(data, size, width, height, bit_depth, channels, format);
        return 0;
    });
}

namespace {
// the header parse, the mode and the stride of the three pixmap entries that write a record
void pixmap_checked_plan(const void* data, size_t size, int mode, size_t stride, PixmapPlan& P)
{
    if (mode < AEON_DECODE_BGR8 || mode > AEON_DECODE_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown pixmap decode mode");
    pixmap_plan(data, size, mode, P);
    if (stride < (size_t)P.w * P.channels * P.elem_bytes || stride > INT32_MAX) fail(AEON_HIP_EINVAL, "stride too small");
}
} // namespace

int aeon_decode_pixmap(const void* data, size_t size, int mode, void* dst, size_t stride, int* elem_bytes)
{
    return guarded([&] {
        if (!data || !dst) fail(AEON_HIP_EINVAL, "null argument");
        PixmapPlan P;
        pixmap_checked_plan(data, size, mode, stride, P);
        pixmap_decode(data, size, mode, dst, stride, elem_bytes);
        return 0;
    });
}

int aeon_pixmap_host_stage(const void* data, size_t size, int mode, int* gpu_route, int64_t* staged_bytes)
{
    return guarded([&] {
        if (!data || !gpu_route || !staged_bytes) fail(AEON_HIP_EINVAL, "null argument");
        if (mode < AEON_DECODE_BGR8 || mode > AEON_DECODE_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown pixmap decode mode");
        PixmapPlan P;
        pixmap_plan(data, size, mode, P);
        *gpu_route = P.route;
        if (P.route) {
            PixmapJob            J;
            std::vector<uint8_t> file(size + 16);
            pixmap_stage(data, size, mode, P, J, file.data());
            *staged_bytes = (int64_t)size;
        } else {
            const size_t         stride = (size_t)P.w * P.channels * P.elem_bytes;
            std::vector<uint8_t> px(stride * P.h);
            pixmap_decode(data, size, mode, px.data(), stride, nullptr);
            *staged_bytes = (int64_t)px.size();
        }
        return 0;
    });
}

int aeon_pixmap_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride)
{
    return guarded([&] {
        if (!data || !dst) fail(AEON_HIP_EINVAL, "null argument");
        PixmapPlan P;
        pixmap_checked_plan(data, size, mode, stride, P);
        if (!pixmap_gpu_emulate(data, size, mode, dst, stride))
            fail(AEON_HIP_EUNSUPPORTED, "PNM: the file is not routed to the device (ASCII samples)");
        return 0;
    });
}

int aeon_tiff_info(const void* data, size_t size, int* width, int* height, int* channels, int* elem_bytes)
{
    return guarded([&] {
        if (!data || !width || !height || !channels || !elem_bytes) fail(AEON_HIP_EINVAL, "null argument");
        TiffPlan P;
        tiff_plan(data, size, AEON_DECODE_ANYDEPTH, P);
        *width = P.w, *height = P.h, *channels = P.file_channels, *elem_bytes = P.elem_bytes;
        return 0;
    });
}

namespace {
// the IFD parse, the mode and the stride of the three TIFF entries that write a record
void tiff_checked_plan(const void* data, size_t size, int mode, size_t stride, TiffPlan& P)
{
    if (mode < AEON_DECODE_BGR8 || mode > AEON_DECODE_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown TIFF decode mode");
    tiff_plan(data, size, mode, P);
    if (stride < (size_t)P.w * P.channels * P.elem_bytes || stride > INT32_MAX) fail(AEON_HIP_EINVAL, "stride too small");
}
} // namespace

int aeon_decode_tiff(const void* data, size_t size, int mode, void* dst, size_t stride, int* elem_bytes)
{
    return guarded([&] {
        if (!data || !dst) fail(AEON_HIP_EINVAL, "null argument");
        TiffPlan P;
        tiff_checked_plan(data, size, mode, stride, P);
        tiff_decode(data, size, mode, dst, stride, elem_bytes);
        return 0;
    });
}

int aeon_tiff_host_stage(const void* data, size_t size, int mode, int* gpu_route, int64_t* staged_bytes)
{
    return guarded([&] {
        if (!data || !gpu_route || !staged_bytes) fail(AEON_HIP_EINVAL, "null argument");
        if (mode < AEON_DECODE_BGR8 || mode > AEON_DECODE_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown TIFF decode mode");
        TiffPlan P;
        tiff_plan(data, size, mode, P);
        *gpu_route = P.route;
        if (P.route) {
            TiffJob                J;
            std::vector<TiffStrip> strips;
            std::vector<TiffBand>  bands;
            std::vector<uint8_t>   file(size + 16);
            tiff_stage(data, size, mode, P, 0, J, strips, bands, file.data());
            *staged_bytes = (int64_t)size;
        } else {
            const size_t         stride = (size_t)P.w * P.channels * P.elem_bytes;
            std::vector<uint8_t> px(stride * P.h);
            tiff_decode(data, size, mode, px.data(), stride, nullptr);
            *staged_bytes = (int64_t)px.size();
        }
        return 0;
    });
}

int aeon_tiff_decoder_route(const void* data, size_t size, int* device)
{
    return guarded([&] {
        if (!data || !device) fail(AEON_HIP_EINVAL, "null argument");
        *device = tiff_routed(data, size) ? 1 : 0;
        return 0;
    });
}

int aeon_tiff_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride)
{
    return guarded([&] {
        if (!data || !dst) fail(AEON_HIP_EINVAL, "null argument");
        TiffPlan P;
        tiff_checked_plan(data, size, mode, stride, P);
        const int r = tiff_gpu_emulate(data, size, mode, dst, stride);
        if (r == 0) fail(AEON_HIP_EUNSUPPORTED, "TIFF: the file is not routed to the device (an LZW / PackBits strip above 32 KiB)");
        if (r < 0) fail(AEON_HIP_EDEVICE, "TIFF: strip data corrupt or truncated (GPU stage)");
        return 0;
    });
}

// pixel_provider::inspect's sniff and header parse (host.cpp), for callers that hold the file themselves
int aeon_encoded_info(const void* data, size_t size, int mask, int* format, int* width, int* height, int* file_channels,
                      int* elem_bytes, int* device_route)
{
    return guarded([&] {
        if (!data || !format || !width || !height) fail(AEON_HIP_EINVAL, "null argument");
        static const uint8_t kPngSig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
        int                  fcn = 0, eb = 1, route = 1;
        if (size >= 8 && std::memcmp(data, kPngSig, 8) == 0) {
            int depth = 0, ctype = 0;
            png_header(data, size, width, height, &depth, &ctype);
            *format = AEON_FORMAT_PNG;
            fcn     = ctype == 0 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 3;
            eb      = (mask && depth == 16 && ctype != 3) ? 2 : 1;
            route   = png_routed(data, size) ? 1 : 0;
        } else if (pixmap_sniff(data, size)) {
            int depth = 0, fmt = 0;
            pixmap_header(data, size, width, height, &depth, &fcn, &fmt);
            *format = AEON_FORMAT_PIXMAP;
            eb      = (mask && depth == 16) ? 2 : 1;
            route   = pixmap_routed(data, size) ? 1 : 0;
        } else if (tiff_sniff(data, size)) {
            TiffPlan P;
            tiff_plan(data, size, AEON_DECODE_ANYDEPTH, P);
            *format = AEON_FORMAT_TIFF;
            *width = P.w, *height = P.h, fcn = P.file_channels;
            eb    = mask ? P.elem_bytes : 1;
            route = tiff_routed(data, size) ? 1 : 0;
        } else {
            if (mask)
                fail(AEON_HIP_ERUNTIME, "encoded pixel masks are decoded from PNG files only (JPEG masks: pass the "
                                        "decoded mask)");
            jpeg_info(data, size, width, height, &fcn);
            *format = AEON_FORMAT_JPEG;
        }
        if (file_channels) *file_channels = fcn;
        if (elem_bytes) *elem_bytes = eb;
        if (device_route) *device_route = route;
        return 0;
    });
}

int aeon_batch_sample_patches(aeon_param_factory* f, int sampler, uint32_t* state, const float* nboxes, int n,
                              float* out, int cap, int* n_out)
{
    return guarded([&] {
        if (!f || !state || !n_out || n < 0 || (n > 0 && !nboxes) || cap < 0 || (cap > 0 && !out))
            fail(AEON_HIP_EINVAL, "null argument");
        std::lock_guard<std::mutex> lock(f->mu);
        if (sampler < 0 || sampler >= (int)f->f.batch_samplers.size()) fail(AEON_HIP_EINVAL, "sampler index out of range");
        TrackedEngine     eng(*state);
        std::vector<nbox> objects, samples;
        for (int i = 0; i < n; i++)
            objects.emplace_back(nboxes[4 * i], nboxes[4 * i + 1], nboxes[4 * i + 2], nboxes[4 * i + 3]);
        f->f.batch_samplers[sampler].sample_patches(eng, objects, samples);
        *n_out = (int)samples.size();
        for (int i = 0; i < (int)samples.size() && i < cap; i++) {
            out[4 * i] = samples[i].xmin, out[4 * i + 1] = samples[i].ymin;
            out[4 * i + 2] = samples[i].xmax, out[4 * i + 3] = samples[i].ymax;
        }
        *state = eng.last;
        return 0;
    });
}

int aeon_seed_slots(uint32_t seed, int n, uint32_t* states)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && !states)) fail(AEON_HIP_EINVAL, "bad arguments");
        std::minstd_rand0 g(seed);
        for (int i = 0; i < n; i++) {
            uint32_t s = g() % 2147483647u;
            states[i]  = s == 0 ? 1 : s;
        }
        return 0;
    });
}

int aeon_jpeg_info(const void* data, size_t size, int* width, int* height, int* components)
{
    return guarded([&] {
        if (!data || !width || !height || !components) fail(AEON_HIP_EINVAL, "null argument");
        jpeg_info(data, size, width, height, components);
        return 0;
    });
}

int aeon_jpeg_entropy_decode(const void* data, size_t size, int* width, int* height, int* components,
                             int64_t* n_blocks, int64_t* n_values, uint64_t* hash)
{
    return guarded([&] {
        if (!data || !width || !height || !components || !n_blocks || !n_values || !hash)
            fail(AEON_HIP_EINVAL, "null argument");
        jpeg_entropy_only(data, size, width, height, components, n_blocks, n_values, hash);
        return 0;
    });
}

int aeon_jpeg_host_stage(const void* data, size_t size, int* gpu_entropy, int64_t* staged_bytes)
{
    return guarded([&] {
        if (!data || !gpu_entropy || !staged_bytes) fail(AEON_HIP_EINVAL, "null argument");
        jpeg_host_stage(data, size, gpu_entropy, staged_bytes);
        return 0;
    });
}

int aeon_jpeg_huff_layout(const void* data, size_t size, int lanes, int32_t* out, int32_t* seg_nsub, int seg_cap)
{
    return guarded([&] {
        if (!data || !out || seg_cap < 0 || (seg_cap > 0 && !seg_nsub)) fail(AEON_HIP_EINVAL, "null argument");
        if (lanes != 256 && lanes != 512 && lanes != 1024) fail(AEON_HIP_EINVAL, "jpeg_huff runs 256, 512 or 1024 lanes");
        jpeg_huff_layout(data, size, lanes, out, seg_nsub, seg_cap);
        return 0;
    });
}

int aeon_unbiased_round(float x, int64_t* out)
{
    return guarded([&] {
        if (!out) fail(AEON_HIP_EINVAL, "null out");
        *out = unbiased_round(x);
        return 0;
    });
}

int aeon_calculate_scale(int width, int height, int output_width, int output_height, float* scale)
{
    return guarded([&] {
        if (!scale) fail(AEON_HIP_EINVAL, "null out");
        *scale = calculate_scale(width, height, output_width, output_height);
        return 0;
    });
}

int aeon_cropbox_max_proportional(float in_w, float in_h, float out_w, float out_h, float* res_w, float* res_h)
{
    return guarded([&] {
        if (!res_w || !res_h) fail(AEON_HIP_EINVAL, "null out");
        cropbox_max_proportional(in_w, in_h, out_w, out_h, res_w, res_h);
        return 0;
    });
}

const char* aeon_hip_last_error(void) { return g_err.c_str(); }

const char* aeon_hip_version(void) { return "aeon-hip 0.1 (gfx950)"; }

} // extern "C"
