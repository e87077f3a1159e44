// rcnn_stubs.cpp -- the device half of the localization_rcnn targets for the host-only sanitizer builds
// (next to aeon_amd/csrc/sanitize/no_device.cpp and box_stubs.cpp): there is no device, so the launch entries fail.
#include <stddef.h>

#include "../../include/aeon_hip.h"

extern "C" int aeon_hip_rcnn_targets_batch(aeon_hip_ctx*, int, const aeon_box_record*, const float*, const int32_t*,
                                           const int32_t*, const aeon_aug_params*, uint32_t*, int, const aeon_rcnn_out*,
                                           void*)
{
    return AEON_HIP_ERUNTIME;
}

namespace aeon_hip {
int rcnn_targets_staged(aeon_hip_ctx*, int, const void*, size_t, const aeon_rcnn_out&, int, uint32_t*, void*)
{
    return AEON_HIP_ERUNTIME;
}
} // namespace aeon_hip
