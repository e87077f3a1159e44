// stager_encoded.hpp -- what stager.cpp offers stager_encoded.cpp (aeon_hip_stager_stage_encoded): the two ways a
// record that arrived encoded enters a window, and the hook through which the window's launch reaches the decode
// stages.  stager.cpp itself names no decode entry: a link of it without stager_encoded.cpp (the stager's
// sanitizer model, tests/sanitize/model_device.cpp) has nothing undefined, and a window without encoded records
// never looks at the hook.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>

#include "../../include/aeon_hip.h"

namespace aeon_hip {

// One file of a launching window that the device decodes: record `desc` of dst_base.
struct stager_file {
    const void*   data;
    size_t        size;
    int           format; // AEON_FORMAT_*
    int           mode;   // AEON_DECODE_* (not read for JPEG: desc.channels says it)
    aeon_img_desc desc;
};
// The window's files through the decode stages on `stream`; an AEON_HIP_E* code with its message in
// aeon_hip_last_error.  The files may be released when it returns.
using stager_decode_fn = int (*)(aeon_hip_ctx* ctx, const stager_file* files, size_t n, void* dst_base, void* stream);
void stager_set_decode(stager_decode_fn fn);

// The stager's kind without AEON_STAGER_DEVICE_OUT and its output channels (they pick the decode mode).
void stager_describe(const aeon_hip_stager* s, int* base_kind, int* out_channels);
// The calling thread's aeon_hip_stager_last_error text.
void stager_set_error(const std::string& what);

// A record decoded on the calling thread: pinned staging for width x height x channels x elem_bytes is reserved
// as aeon_hip_stager_stage reserves it, fill(arg, dst, row_bytes) writes the pixels there (unlocked) and the
// record is published.  fill returns 0 or an AEON_HIP_E* code, having set the error text; the idx then stays
// unstaged.  Returns as the C entries do.
using stager_fill_fn = int (*)(void* arg, uint8_t* dst, size_t row_bytes);
int stager_stage_decoded(aeon_hip_stager* s, void* batch_out, int idx, int width, int height, int channels,
                         int elem_bytes, const aeon_aug_params* params, int format, stager_fill_fn fill, void* arg);
// A record the window's launch decodes on the device: `bytes` (the caller's copy of the file) is kept until
// then, and the record gets a slot of the window's device source arena behind its staged pixels.
int stager_stage_file(aeon_hip_stager* s, void* batch_out, int idx, int width, int height, int channels,
                      int elem_bytes, const aeon_aug_params* params, int format, int mode,
                      std::unique_ptr<uint8_t[]> bytes, size_t size);

} // namespace aeon_hip
