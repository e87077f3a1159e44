// png.hpp -- the PNG decoder's two host functions (png_host.cpp), behind aeon_png_info / aeon_decode_png
// and the decoder's providers.  Both throw jpeg_error (error.hpp) on a malformed file.
#pragma once
#include <stddef.h>

namespace aeon_hip {

// the IHDR's width, height, bit depth and colour type
void png_header(const void* data, size_t size, int* w, int* h, int* depth, int* ctype);
// decodes to `mode` (AEON_PNG_*) into rows `stride` bytes apart; out_elem_bytes (optional): 1 or 2
void png_decode(const void* data, size_t size, int mode, void* dst, size_t stride, int* out_elem_bytes);

} // namespace aeon_hip
