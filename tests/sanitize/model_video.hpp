// model_video.hpp -- what tests/sanitize/stager_clip_driver.cpp uses of the model of the video call
// (model_video.cpp), which stands beside the decoding model device (model_decode.cpp, unchanged) in the builds of
// the stager's video half.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/aeon_hip.h"

#define MODEL_KIND_VIDEO 0x71d0ull

extern "C" {
// The model's "kernel" for one clip: out[0 .. 3*D*out_h*out_w - 8) = the first frame's first source bytes (zero
// filled past them), the 8 bytes behind = a 64-bit checksum of the frame count, D, the output size, the params'
// crop / size / flip / angle and, frame by frame, the desc's geometry and every source byte at src_base + offset
// (the offsets themselves are not hashed: the clip may lie anywhere).  No byte from 3*D*out_h*out_w on is written.
void model_clip_output(const uint8_t* src_base, const aeon_img_desc* row, int count, int D, int out_w, int out_h,
                       aeon_aug_params p, uint8_t* out);
// The kth call of the model's aeon_hip_video_batch from now (1 = the next one) fails with `error`; later calls
// succeed.  model_decode.cpp keeps its script (model_fail_call) to the entries it defines, so the video call has
// its own.
void model_video_fail_call(int kth, int error);
// Calls of the model's aeon_hip_video_batch, and the most frames one of them took, since model_video_reset.
long model_video_calls(void);
long model_video_max_frames(void);
void model_video_reset(void);
}
