// model_decode.hpp -- what tests/sanitize/stager_encoded_driver.cpp uses of the decoding model device
// (model_decode.cpp) besides the HIP and aeon_hip entries it stands in for.
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
// Forgets every count, every scripted failure and the upload log.
void model_reset(void);
// The model's "kernel" for one record: out[0 .. item_stride-8) = the record's first source bytes (zero filled
// past stride*height of them), out[item_stride-8 ..) = a 64-bit checksum of kind, the desc's geometry, the
// params' crop / size / flip / angle and every source byte.
void model_record_output(uint64_t kind, const uint8_t* src, aeon_img_desc d, aeon_aug_params p, uint8_t* out,
                         size_t item_stride);
// What the model's JPEG stage writes for a file: d.height rows of d.width * d.channels bytes at d.stride, a
// pattern keyed by an FNV-1a hash of the file's bytes (the product has no host IDCT; the layout is under test).
void model_jpeg_pattern(const void* data, size_t size, aeon_img_desc d, uint8_t* dst);
// Files handed to a decode entry whose bytes also lay in a host range a host-to-device copy uploaded (found by
// address, or by content: the file's first bytes inside the copied range): encoded bytes that travelled twice.
long model_double_uploads(void);
// Bytes of every host-to-device copy, and of every file a decode entry took, since the last model_reset.
long model_copied_bytes(void);
long model_file_bytes(void);
}
