// model_device.hpp -- what tests/sanitize/stager_driver.cpp uses of the model device (model_device.cpp)
// besides the HIP and aeon_hip entries it stands in for.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/aeon_hip.h"

#define MODEL_KIND_AUGMENT 0x1a6eull
#define MODEL_KIND_MASK    0x3a5cull

extern "C" {
// The kth call from now (1 = the next one) of the entry named fn -- a HIP function or one of the aeon_hip
// entries of the model -- fails with `error` (a hipError_t, or an AEON_HIP_E* code); later calls succeed.
void model_fail_call(const char* fn, int kth, int error);
// Calls of fn since the last model_reset.
long model_calls(const char* fn);
// Forgets every count and every scripted failure.
void model_reset(void);
// The model's "kernel" for one record: out[0 .. item_stride-8) = the record's first source bytes (zero
// filled past stride*height of them), out[item_stride-8 ..) = a 64-bit checksum of kind, the desc's
// geometry, the params' crop / size / flip / angle and every source byte.
void model_record_output(uint64_t kind, const uint8_t* src, aeon_img_desc d, aeon_aug_params p, uint8_t* out,
                         size_t item_stride);
}
