// png.hpp -- the PNG decoder: its host functions (png_host.cpp) behind aeon_png_info / aeon_decode_png and the
// decoder's providers, and the descriptors the host half of the PNG stage shares with its kernels
// (png_kernels.hip, png_inflate.hpp).  The host functions throw jpeg_error (error.hpp) on a malformed file.
//
// The stage (aeon_hip_decode_png_batch): the host walks each file's chunks (signature, CRCs of the critical
// chunks, IHDR, PLTE), checks the zlib header and copies the IDAT payloads back to back into pinned staging;
// png_inflate (one wave per file) inflates the stream into the file's device scratch, png_unfilter (one
// workgroup per file) undoes the row filters there and converts the rows into the record.  Interlaced files,
// very wide rows and streams of 2^31 bytes or more stay with png_decode on the host (png_route).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/aeon_hip.h" // AEON_PNG_*

namespace aeon_hip {

// the IHDR's width, height, bit depth and colour type
void png_header(const void* data, size_t size, int* w, int* h, int* depth, int* ctype);
// decodes to `mode` (AEON_PNG_*) into rows `stride` bytes apart; out_elem_bytes (optional): 1 or 2
void png_decode(const void* data, size_t size, int mode, void* dst, size_t stride, int* out_elem_bytes);

constexpr int kPngCorruptBit    = 1024;  // device error word: a PNG stream or row the GPU stage refuses
constexpr int kPngWindow        = 32768; // deflate's window
constexpr int kPngUnfilterFixed = 768;   // png_unfilter's LDS ahead of the rows: the palette
constexpr int kPngUnfilterLds   = 64 * 1024; // most LDS a png_unfilter workgroup takes
constexpr int kPngMaxRow        = 16 * 1024; // widest row (filter byte included) the device takes: three rows
                                             // (the previous one and a band of two) fit kPngUnfilterLds

// png_unfilter's LDS for rows of rowb bytes: the palette, the previous row and a band of up to 64 rows.
inline int png_unfilter_lds(int rowb)
{
    const long want = (long)kPngUnfilterFixed + ((rowb + 15) & ~15) + 16 + 64L * (rowb + 1);
    return (int)(want < kPngUnfilterLds ? want : kPngUnfilterLds);
}

// One device-decoded file (device addresses; the emulation's are host addresses).
struct alignas(16) PngJob {
    uint64_t comp; // the zlib stream (IDAT payloads back to back), 8-byte aligned, zero-padded to a multiple of 8
    uint64_t raw;  // scratch for the inflated scanlines: (rowb + 1) * h bytes, 16-byte aligned and padded
    uint64_t out;  // the record
    uint32_t clen, need; // compressed bytes, inflated bytes
    int32_t  w, h, depth, ctype, samples, npal, mode, elem_bytes;
    int32_t  rowb, bpp; // bytes of a row, the filters' byte distance
    int32_t  out_row_bytes, stride;
    uint8_t  pal[768];
};
static_assert(sizeof(PngJob) % 16 == 0, "PngJob: 16-byte aligned array elements");

// What the host half learns from a file's chunks without touching its pixels.
struct PngPlan {
    int    w = 0, h = 0, depth = 0, ctype = 0, interlace = 0, channels = 0, elem_bytes = 1;
    int    route = 0;   // 1: the device inflates and unfilters the file (png_route)
    size_t clen = 0;    // bytes of its zlib stream
    size_t need = 0;    // bytes of its inflated scanlines (routed files)
};
// The chunk walk of png_decode (same refusals, same messages) plus the zlib header check, and the routing rule.
void png_plan(const void* data, size_t size, int mode, PngPlan& P);
// What the decoder's inspect step asks: does this file go through the stage?  The chunk walk without the CRCs
// (the batch call checks them), png_plan's routing rule, and the measured one on top: png_inflate's time goes
// with the symbols it decodes (the compressed bytes), the host decoder's with the inflated bytes, and the
// device wins only where the stream is small beside its scanlines (masks, flat or smooth
// images; not noisy photographs) -- at least kPngDecoderMinRatio inflated bytes per compressed byte.  False
// also for a file the walk refuses, which then takes the host decoder's path and gets its error there.
constexpr size_t kPngDecoderMinRatio = 8;
bool             png_routed(const void* data, size_t size);
// A routed file's job (everything but the three addresses) and its zlib stream copied to comp_dst
// (P.clen bytes; the caller pads).
void png_stage(const void* data, size_t size, int mode, const PngPlan& P, PngJob& J, uint8_t* comp_dst);
// The stage's kernels run on this thread, lane after lane (png_inflate.hpp): 1 decoded, 0 the file is not
// routed to the device (nothing written), -1 the device would set kPngCorruptBit.
int png_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride);

} // namespace aeon_hip
