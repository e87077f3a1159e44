// video_stubs.cpp -- the device half of the video provider for the host-only sanitizer builds (next to
// aeon_amd/csrc/sanitize/no_device.cpp, box_stubs.cpp and rcnn_stubs.cpp): there is no device, so the launch entry fails.
#include <stddef.h>

#include "../../include/aeon_hip.h"

extern "C" int aeon_hip_video_batch(aeon_hip_ctx*, int, const int32_t*, const aeon_img_desc*, const void*,
                                    const aeon_aug_params*, int, int, int, void*, uint64_t, void*)
{
    return AEON_HIP_ERUNTIME;
}
