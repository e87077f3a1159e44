// stager_clip.cpp -- the video half of the aeon-side drop-in: what provider::video holds (include/aeon_hip.h).
//   aeon_clip_info               -- host only: the demux of the kept frames and the first one's decoded size, which
//                                   is what provider::video calls make_params with (provider.cpp:503-513)
//   aeon_hip_stager_stage_clip   -- provide() with the record's AVI datum: video::extractor (cv::imdecode of every
//                                   frame on aeon's pool, etl_video.cpp:23-41) goes away with the pixels' trip over
//                                   PCIe; the kept frames' JPEG files are copied and the window's launch decodes them
//   aeon_hip_stager_stage_frames -- provide() after aeon's own video::extractor: the decoded frames into pinned staging
// The entries do what the decoder's video_provider does per element (host.cpp: inspect, layout_record, launch),
// against the public C ABI alone.  stager.cpp knows the JPEG stage and the video call only through the hooks
// installed here (stager_clip.hpp).
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"
#include "stager_clip.hpp"

namespace {

using aeon_hip::stager_clip_frame;
using aeon_hip::stager_file;

// (the JPEG stage's staging sets stay at the size the decoder sizes them to: host.cpp, stage_sources)
constexpr size_t kCallFiles = 512;

// The window's frames through the JPEG stage, at most kCallFiles a call.
int decode_frames(aeon_hip_ctx* ctx, const stager_file* files, size_t n, void* dst_base, void* stream)
{
    std::vector<const void*>   data(n);
    std::vector<size_t>        sizes(n);
    std::vector<aeon_img_desc> descs(n);
    for (size_t i = 0; i < n; i++) data[i] = files[i].data, sizes[i] = files[i].size, descs[i] = files[i].desc;
    for (size_t f = 0; f < n; f += kCallFiles) {
        const int k = (int)std::min(kCallFiles, n - f);
        if (const int rc = aeon_hip_decode_jpeg_batch(ctx, k, data.data() + f, sizes.data() + f, descs.data() + f, dst_base, stream))
            return rc;
    }
    return 0;
}

struct clip_error {
    int         code;
    std::string what;
};

// video::extractor without the decode: the first min(count, max_frames) frames of the datum and the first one's
// decoded size.  every_header: each kept non-empty frame's header is parsed and must give the first one's size.
void demux_clip(const void* data, size_t size, int max_frames, bool every_header, std::vector<aeon_avi_frame>& frames,
                int& width, int& height)
{
    int count = 0;
    frames.assign((size_t)max_frames, aeon_avi_frame{});
    if (const int rc = aeon_avi_frames(data, size, frames.data(), max_frames, &count, nullptr, nullptr))
        throw clip_error{rc, aeon_avi_last_error()};
    frames.resize((size_t)std::min(count, max_frames));
    for (size_t d = 0; d < frames.size(); d++) {
        if (frames[d].size == 0) continue; // repeats the previous frame (the demux refuses an empty first one)
        int fw = 0, fh = 0, comps = 0;
        if (const int rc = aeon_jpeg_info((const uint8_t*)data + frames[d].offset, frames[d].size, &fw, &fh, &comps))
            throw clip_error{rc, aeon_hip_last_error()};
        if (d == 0) width = fw, height = fh;
        else if (fw != width || fh != height) // (the decoder's text: host.cpp, video_provider::inspect)
            throw clip_error{AEON_HIP_EINVAL, "video: frame " + std::to_string(d) + " is " + std::to_string(fw) + "x" +
                                                  std::to_string(fh) + ", the first frame " + std::to_string(width) + "x" +
                                                  std::to_string(height)};
        if (!every_header) break;
    }
}

// The entry's checks before any byte of the clip is read; 0, or the code with the text set.
int refuse(const char* entry, aeon_hip_stager* s, const void* batch_out, int idx, const aeon_aug_params* params)
{
    if (!s || !batch_out || !params) {
        aeon_hip::stager_set_error("null argument");
        return AEON_HIP_EINVAL;
    }
    aeon_hip::stager_clip_shape shape{};
    aeon_hip::stager_clip_describe(s, &shape);
    if (shape.base_kind != AEON_STAGER_VIDEO) {
        aeon_hip::stager_set_error(std::string(entry) + " on " + (shape.base_kind == AEON_STAGER_MASK ? "a mask" : "an image") +
                                   " stager, which takes records (aeon_hip_stager_stage / _stage_encoded), at idx " +
                                   std::to_string(idx));
        return AEON_HIP_EINVAL;
    }
    aeon_hip::stager_set_clip_hooks(decode_frames, aeon_hip_video_batch);
    return 0;
}

} // namespace

extern "C" {

int aeon_clip_info(const void* data, size_t size, int max_frames, int* kept, int* width, int* height)
try {
    if (!kept || !width || !height || max_frames <= 0) {
        aeon_hip::stager_set_error(max_frames <= 0 ? "max_frames must be > 0" : "null argument");
        return AEON_HIP_EINVAL;
    }
    std::vector<aeon_avi_frame> frames;
    int                         w = 0, h = 0;
    demux_clip(data, size, max_frames, false, frames, w, h);
    *kept = (int)frames.size(), *width = w, *height = h;
    return 0;
} catch (const clip_error& e) {
    aeon_hip::stager_set_error(e.what);
    return e.code;
} catch (const std::exception& e) {
    aeon_hip::stager_set_error(e.what());
    return AEON_HIP_ERUNTIME;
}

int aeon_hip_stager_stage_clip(aeon_hip_stager* s, void* batch_out, int idx, const void* data, size_t size,
                               const aeon_aug_params* params)
try {
    if (const int rc = refuse("aeon_hip_stager_stage_clip", s, batch_out, idx, params)) return rc;
    const std::string at = ", at idx " + std::to_string(idx);
    if (!data || size == 0) {
        aeon_hip::stager_set_error("received encoded video with size 0" + at);
        return AEON_HIP_EINVAL;
    }
    aeon_hip::stager_clip_shape shape{};
    aeon_hip::stager_clip_describe(s, &shape);
    std::vector<aeon_avi_frame> frames;
    int                         w = 0, h = 0;
    try {
        demux_clip(data, size, shape.max_frames, true, frames, w, h);
    } catch (const clip_error& e) {
        aeon_hip::stager_set_error(e.what + at);
        return e.code;
    }
    // one file per distinct frame; an empty chunk's frame is the previous one again (cap_mjpeg_decoder.cpp:138-141)
    std::vector<stager_clip_frame> clip(frames.size());
    for (size_t d = 0; d < frames.size(); d++)
        clip[d] = frames[d].size ? stager_clip_frame{(const uint8_t*)data + frames[d].offset, frames[d].size}
                                 : stager_clip_frame{nullptr, 0};
    return aeon_hip::stager_stage_clip_frames(s, batch_out, idx, (int)clip.size(), clip.data(), 1, w, h, w * 3, params);
} catch (const std::exception& e) {
    aeon_hip::stager_set_error(e.what());
    return AEON_HIP_ERUNTIME;
}

int aeon_hip_stager_stage_frames(aeon_hip_stager* s, void* batch_out, int idx, int n_frames, const void* const* pixels,
                                 int width, int height, int stride, const aeon_aug_params* params)
try {
    if (const int rc = refuse("aeon_hip_stager_stage_frames", s, batch_out, idx, params)) return rc;
    if (!pixels) {
        aeon_hip::stager_set_error("null argument");
        return AEON_HIP_EINVAL;
    }
    // (n_frames is checked against the stager's max_frames by the stager, with the other arguments, before it
    // reads a frame: no entry past max_frames is read here either)
    aeon_hip::stager_clip_shape shape{};
    aeon_hip::stager_clip_describe(s, &shape);
    std::vector<stager_clip_frame> clip((size_t)std::max(1, std::min(n_frames, shape.max_frames)), stager_clip_frame{nullptr, 0});
    for (int d = 0; d < std::min(n_frames, shape.max_frames); d++) clip[d] = stager_clip_frame{pixels[d], 0};
    return aeon_hip::stager_stage_clip_frames(s, batch_out, idx, n_frames, clip.data(), 0, width, height,
                                              stride ? stride : width * 3, params);
} catch (const std::exception& e) {
    aeon_hip::stager_set_error(e.what());
    return AEON_HIP_ERUNTIME;
}

} // extern "C"
