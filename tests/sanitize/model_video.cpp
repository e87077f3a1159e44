// model_video.cpp -- aeon_hip_video_batch for the stager's model device (model_decode.cpp: "device" memory is host
// memory): the checks of the real call's arguments that the stager can get wrong (counts, the params' output size,
// item_stride, 65,535 frames a call) and, per clip, a function of everything the real call reads -- model_clip_output.
// For the builds of the stager's video half (Makefile targets sanitize_stager_clip / tsan_stager_clip).
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>

#include "../../aeon_amd/csrc/error.hpp"
#include "model_video.hpp"

namespace {

std::mutex g_mu;
int        g_countdown = 0, g_error = 0;
long       g_calls = 0, g_max_frames = 0;

uint64_t mix(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001b3ull; }

int failed(const std::string& what, int code)
{
    aeon_hip::set_last_error(("aeon_hip_video_batch: " + what).c_str());
    return code;
}

} // namespace

extern "C" {

void model_video_fail_call(int kth, int error)
{
    std::lock_guard<std::mutex> l(g_mu);
    g_countdown = kth, g_error = error;
}

long model_video_calls(void)
{
    std::lock_guard<std::mutex> l(g_mu);
    return g_calls;
}

long model_video_max_frames(void)
{
    std::lock_guard<std::mutex> l(g_mu);
    return g_max_frames;
}

void model_video_reset(void)
{
    std::lock_guard<std::mutex> l(g_mu);
    g_countdown = g_error = 0;
    g_calls = g_max_frames = 0;
}

void model_clip_output(const uint8_t* src_base, const aeon_img_desc* row, int count, int D, int out_w, int out_h,
                       aeon_aug_params p, uint8_t* out)
{
    uint64_t h = mix(0xcbf29ce484222325ull, MODEL_KIND_VIDEO);
    for (int32_t v : {count, D, out_w, out_h, p.crop_x, p.crop_y, p.crop_w, p.crop_h, p.out_w, p.out_h, p.flip, p.angle})
        h = mix(h, (uint32_t)v);
    for (int d = 0; d < count; d++) {
        const aeon_img_desc& f = row[d];
        for (int32_t v : {f.width, f.height, f.stride, f.channels, f.elem_bytes}) h = mix(h, (uint32_t)v);
        const uint8_t* src = src_base + f.offset;
        const size_t   n   = (size_t)f.stride * f.height;
        for (size_t i = 0; i < n; i++) h = mix(h, src[i]);
    }
    const size_t item = 3 * (size_t)D * out_h * out_w;
    if (item < 8) return;
    const size_t head = count > 0 ? std::min((size_t)row[0].stride * row[0].height, item - 8) : 0;
    if (head) std::memcpy(out, src_base + row[0].offset, head);
    std::memset(out + head, 0, item - 8 - head);
    std::memcpy(out + item - 8, &h, 8);
}

int aeon_hip_video_batch(aeon_hip_ctx*, int n, const int32_t* frame_counts, const aeon_img_desc* descs, const void* src_base,
                         const aeon_aug_params* params, int max_frames, int out_w, int out_h, void* out_dev,
                         uint64_t item_stride, void*)
{
    {
        std::lock_guard<std::mutex> l(g_mu);
        g_calls++;
        if (g_countdown > 0 && --g_countdown == 0) return failed("scripted failure", g_error);
    }
    if (n < 0 || (n > 0 && (!frame_counts || !descs || !params || !out_dev || !src_base)))
        return failed("null argument", AEON_HIP_EINVAL);
    if (max_frames <= 0 || out_w <= 0 || out_h <= 0) return failed("invalid max_frame_count or frame size", AEON_HIP_EINVAL);
    if (item_stride < 3 * (uint64_t)max_frames * out_h * out_w) return failed("output item does not fit item_stride", AEON_HIP_EINVAL);
    long total = 0;
    for (int i = 0; i < n; i++) {
        if (frame_counts[i] < 0 || frame_counts[i] > max_frames) return failed("frame count outside [0, max_frame_count]", AEON_HIP_EINVAL);
        if (params[i].out_w != out_w || params[i].out_h != out_h) return failed("output_size differs from the frame size", AEON_HIP_EINVAL);
        total += frame_counts[i];
    }
    if (total > 65535) return failed("at most 65535 frames per call", AEON_HIP_EINVAL);
    {
        std::lock_guard<std::mutex> l(g_mu);
        g_max_frames = std::max(g_max_frames, total);
    }
    for (int i = 0; i < n; i++)
        model_clip_output((const uint8_t*)src_base, descs + (size_t)i * max_frames, frame_counts[i], max_frames, out_w, out_h,
                          params[i], (uint8_t*)out_dev + (size_t)i * item_stride);
    return 0;
}

} // extern "C"
