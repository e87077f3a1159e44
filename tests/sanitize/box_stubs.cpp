// box_stubs.cpp -- the device half of the box targets for the host-only sanitizer builds (next to
// aeon_amd/csrc/sanitize/no_device.cpp): there is no device, so the launch entries fail like the other stubs'.
#include <stddef.h>

#include "../../include/aeon_hip.h"

extern "C" int aeon_hip_box_targets_batch(aeon_hip_ctx*, int, const aeon_box_record*, const float*, const int32_t*,
                                          const int32_t*, const aeon_aug_params*, const aeon_box_out*, void*)
{
    return AEON_HIP_ERUNTIME;
}

namespace aeon_hip {
int box_targets_staged(aeon_hip_ctx*, int, const void*, size_t, const aeon_box_out&, void*) { return AEON_HIP_ERUNTIME; }
} // namespace aeon_hip
