// stager_clip.hpp -- what stager.cpp offers stager_clip.cpp (aeon_hip_stager_stage_clip / _stage_frames): the way a
// clip enters a window of a video stager, and the hooks through which that window's launch reaches the JPEG stage
// and the video call.  stager.cpp itself names neither aeon_hip_video_batch nor the demux nor the JPEG parser: a
// link of it without stager_clip.cpp (the stager's sanitizer model, tests/sanitize/model_device.cpp) has nothing
// undefined, and a window of an image or mask stager never looks at the hooks.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aeon_hip.h"
#include "stager_encoded.hpp"

namespace aeon_hip {

// aeon_hip_video_batch's signature.
using stager_video_fn = int (*)(aeon_hip_ctx* ctx, int n, const int32_t* frame_counts, const aeon_img_desc* descs,
                                const void* src_base, const aeon_aug_params* params, int max_frames, int out_w, int out_h,
                                void* out_dev, uint64_t item_stride, void* stream);
// The hooks of a video stager's windows: `decode` takes the window's frames still encoded (JPEG files all), ahead
// of `video`, one call per batch (or per 65,535 frames of it).  Kept apart from stager_set_decode's hook: a
// process may hold image stagers and video stagers.
void stager_set_clip_hooks(stager_decode_fn decode, stager_video_fn video);

// The stager's kind without AEON_STAGER_DEVICE_OUT and, of a video stager, its geometry.
struct stager_clip_shape {
    int base_kind, max_frames, out_w, out_h;
};
void stager_clip_describe(const aeon_hip_stager* s, stager_clip_shape* shape);

// One frame of a clip: data == nullptr repeats the frame before it (never the first); else the frame's JPEG file
// (encoded; `size` bytes) or its BGR pixels (`size` is not read).
struct stager_clip_frame {
    const void* data;
    size_t      size;
};
// Clip idx of batch_out: n_frames frames of width x height.  encoded != 0: every frame with data is copied, kept
// until the window's launch and gets a slot of the window's device source arena; else its pixels (rows `stride`
// bytes apart) are copied into the window's pinned staging.  Checks the kind, idx, n_frames against max_frames and
// the params' output size against the stager's.  Returns as the C entries do.
int stager_stage_clip_frames(aeon_hip_stager* s, void* batch_out, int idx, int n_frames, const stager_clip_frame* frames,
                             int encoded, int width, int height, int stride, const aeon_aug_params* params);

} // namespace aeon_hip
