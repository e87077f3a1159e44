// pixmap.hpp -- the pixmap decoder (BMP and PNM files, what cv::imdecode reads beside JPEG and PNG): its host
// functions (pixmap_host.cpp) behind aeon_pixmap_info / aeon_decode_pixmap and the decoder's providers, and the
// descriptors the host half of the pixmap stage shares with its kernel (pixmap_kernels.hip, pixmap_rows.hpp).
// The host functions throw jpeg_error (error.hpp) on a file they refuse; messages start with "BMP:" / "PNM:".
//
// The stage (aeon_hip_decode_pixmap_batch): the host parses each header, refuses what can be refused (a short
// file is a host-side fact), builds the file's 256-entry table (palette and gray of each entry) and copies the
// file as it is into pinned staging; pixmap_convert (one workgroup per file and band of rows) stages the
// band's source bytes in LDS with aligned loads and converts them into the record.  ASCII PNM files stay with
// pixmap_decode on the host (pixmap_route).  The decode rules are DESIGN section 20.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/aeon_hip.h" // AEON_DECODE_*, AEON_PIXMAP_*

namespace aeon_hip {

// How a file's samples lie in a source row (PixmapJob::kind)
enum PixmapKind : int32_t {
    kPmBits1 = 0, // 1 bit per pixel, MSB first, through the table (P4, 1-bit BMP)
    kPmBits4,     // 4 bits per pixel, high nibble first, through the table (4-bit BMP)
    kPmIndex8,    // a byte per pixel through the table (8-bit BMP)
    kPmGray8,     // P5, maxval <= 255
    kPmGray16,    // P5, maxval > 255: big-endian
    kPmRgb8,      // P6, maxval <= 255: R, G, B
    kPmRgb16,     // P6, maxval > 255: big-endian R, G, B
    kPmBgr8,      // 24-bit BMP: B, G, R
    kPmBgra8,     // 32-bit BMP: B, G, R, x
};

constexpr int kPixmapLanes     = 256;       // pixmap_convert workgroup
constexpr int kPixmapBandBytes = 16 * 1024; // most source bytes of one band (LDS: these + 8, and the 1 KiB table)
constexpr size_t kPixmapMaxPixels = (size_t)1 << 28;

// colour -> gray, one formula everywhere (8- and 16-bit samples, palette entries); parity unpinned
constexpr uint32_t pixmap_gray(uint32_t b, uint32_t g, uint32_t r) { return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14; }

// One device-decoded file (device addresses; the emulation's are host addresses).
struct alignas(16) PixmapJob {
    uint64_t src;  // the file in the staging: 16-byte aligned, at least 16 zero bytes behind it
    uint64_t out;  // the record
    int64_t  off;  // byte offset in the file of the source row of output row 0, unaligned as it comes
    int32_t  pitch; // bytes from one output row's source to the next; negative: BMP bottom-up
    int32_t  kind, w, h;
    int32_t  sbits;       // source bits per pixel
    int32_t  mode, elem_bytes;
    int32_t  stride;      // bytes between the record's rows
    int32_t  pad_[2];
    uint32_t table[256];  // entry i: B | G << 8 | R << 16 | gray << 24 of index i (table kinds)
};
static_assert(sizeof(PixmapJob) % 16 == 0, "PixmapJob: 16-byte aligned array elements");

// One workgroup's work: rows [y0, y0 + rows) of a job, pixels [p0, p0 + np) of them (p0 > 0 only where one row's
// source is wider than a band: then rows == 1 and p0 is a multiple of 8, a whole source byte at every depth).
struct alignas(16) PixmapBand {
    int32_t job, y0, rows, p0, np, pad_[3];
};

// What the host half learns from a file's header.
struct PixmapPlan {
    int     format = 0; // AEON_PIXMAP_BMP, or 1..6 for P1..P6
    int     w = 0, h = 0, bit_depth = 8, file_channels = 1;
    int     channels = 1, elem_bytes = 1; // of the record in the requested mode
    int     kind = 0, sbits = 0, maxval = 255;
    int     route = 0;      // 1: the device converts the file (pixmap_route)
    int64_t off  = 0;       // as PixmapJob::off; ASCII PNM: where the samples start
    int32_t pitch = 0;      // as PixmapJob::pitch
    uint32_t table[256] = {};
};

// header only: AEON_PIXMAP_* format, width, height, decoded bits per sample (8 or 16), the file's channels
void pixmap_header(const void* data, size_t size, int* w, int* h, int* bit_depth, int* channels, int* format);
// true when the first bytes are a BMP's or a PNM's as the decoder's inspect step sniffs them (strict: anything
// else is left to the JPEG parser and its error)
bool pixmap_sniff(const void* data, size_t size);
// the whole decode on the calling thread into rows `stride` bytes apart; out_elem_bytes (optional): 1 or 2
void pixmap_decode(const void* data, size_t size, int mode, void* dst, size_t stride, int* out_elem_bytes);
// The header parse of pixmap_decode (same refusals, same messages), the table and the routing rule.
void pixmap_plan(const void* data, size_t size, int mode, PixmapPlan& P);
// The routing rule: binary PNM and uncompressed BMP below 2^31 bytes go to the device.
bool pixmap_route(const PixmapPlan& P, size_t size);
// What the decoder's inspect step asks: does this file go through the stage?  pixmap_route's plain rule (DESIGN
// section 20 holds the measurement behind it).  False also for a file the parse refuses, which then takes the
// host decoder's path and gets its error there.
bool pixmap_routed(const void* data, size_t size);
// A routed file's job (everything but the two addresses and the stride) and the file copied to file_dst (size bytes;
// the caller pads).
void pixmap_stage(const void* data, size_t size, int mode, const PixmapPlan& P, PixmapJob& J, uint8_t* file_dst);
// The bands of job `job`, appended.
template <typename Vec>
inline void pixmap_bands(const PixmapJob& J, int job, Vec& bands)
{
    const int64_t ap = J.pitch < 0 ? -(int64_t)J.pitch : J.pitch;
    if (ap <= kPixmapBandBytes) {
        const int R = (int)(kPixmapBandBytes / (ap ? ap : 1));
        for (int y0 = 0; y0 < J.h; y0 += R) bands.push_back(PixmapBand{job, y0, J.h - y0 < R ? J.h - y0 : R, 0, J.w, {0, 0, 0}});
        return;
    }
    const int P = (int)((int64_t)kPixmapBandBytes * 8 / J.sbits) & ~7;
    for (int y = 0; y < J.h; y++)
        for (int p0 = 0; p0 < J.w; p0 += P) bands.push_back(PixmapBand{job, y, 1, p0, J.w - p0 < P ? J.w - p0 : P, {0, 0, 0}});
}
// The stage's kernel code run on this thread, lane after lane (pixmap_rows.hpp): true decoded, false the file is
// not routed to the device (nothing written).
bool pixmap_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride);

} // namespace aeon_hip
