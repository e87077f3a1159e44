// pixmap_host.cpp -- the BMP and PNM half of image::extractor::extract / pixel_mask::extractor::extract (aeon
// src/etl_image.cpp:83-99, src/etl_pixel_mask.cpp:30-53): what cv::imdecode reads beside JPEG and PNG, restated
// from the formats and this project's reading of OpenCV 2.4.9 (DESIGN section 20 says which rules are pinned by
// the format and which are "parity unpinned").  Two users: pixmap_decode, the whole decode of one file on the
// calling thread (aeon_decode_pixmap, and the ASCII files the stage leaves to the host), and the host half of
// the pixmap stage (aeon_hip_decode_pixmap_batch): pixmap_plan / pixmap_stage parse the header, refuse what a
// file can be refused for, build the table and copy the file; the conversion is the kernel's
// (pixmap_kernels.hip).  pixmap_gpu_emulate runs the kernel's own code (pixmap_rows.hpp) on the host.
//
// Every read of the file is checked against `size` first: the header reader never passes the end, and the
// pixel data's extent is checked before a byte of it is read.
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"
#include "error.hpp" // jpeg_error: an error carrying its AEON_HIP_E* code
#include "pixmap.hpp"
#include "pixmap_rows.hpp"

namespace aeon_hip {
namespace {

[[noreturn]] void bmp_bad(const std::string& m, int code = AEON_HIP_EINVAL) { throw jpeg_error(code, "BMP: " + m); }
[[noreturn]] void pnm_bad(const std::string& m) { throw jpeg_error(AEON_HIP_EINVAL, "PNM: " + m); }

uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }
bool     is_space(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

uint32_t table_entry(uint32_t b, uint32_t g, uint32_t r) { return b | g << 8 | r << 16 | pixmap_gray(b, g, r) << 24; }

bool sniff_pnm(const uint8_t* d, size_t size) { return size >= 3 && d[0] == 'P' && d[1] >= '1' && d[1] <= '6' && is_space(d[2]); }
bool sniff_bmp(const uint8_t* d, size_t size)
{
    if (size < 18 || d[0] != 'B' || d[1] != 'M') return false;
    const uint32_t hs = le32(d + 14);
    return hs == 12 || hs >= 40;
}

// The next decimal token from position p on: whitespace and #-comments skipped, digits read.
uint32_t pnm_token(const uint8_t* d, size_t size, size_t& p, const char* what)
{
    for (;;) {
        while (p < size && is_space(d[p])) p++;
        if (p < size && d[p] == '#') {
            while (p < size && d[p] != '\n' && d[p] != '\r') p++;
            continue;
        }
        break;
    }
    if (p >= size) pnm_bad(std::string("the file ends before its ") + what);
    if (d[p] < '0' || d[p] > '9') pnm_bad(std::string("bad ") + what);
    uint64_t v = 0;
    while (p < size && d[p] >= '0' && d[p] <= '9') {
        v = v * 10 + (d[p++] - '0');
        if (v > (uint64_t)INT32_MAX) pnm_bad(std::string("bad ") + what);
    }
    return (uint32_t)v;
}

void plan_pnm(const uint8_t* d, size_t size, PixmapPlan& P, bool need_data)
{
    P.format = d[1] - '0';
    size_t p = 2;
    const uint32_t w = pnm_token(d, size, p, "width"), h = pnm_token(d, size, p, "height");
    uint32_t       maxval = 1;
    const bool     bits = P.format == 1 || P.format == 4, ascii = P.format <= 3, rgb = P.format == 3 || P.format == 6;
    if (!bits) {
        maxval = pnm_token(d, size, p, "maxval");
        if (maxval < 1 || maxval > 65535) pnm_bad("maxval outside 1..65535");
    }
    if (w < 1 || h < 1 || (uint64_t)w * h > kPixmapMaxPixels) pnm_bad("bad image size");
    if (p >= size || !is_space(d[p])) pnm_bad("no whitespace byte between the header and the data");
    p++;
    P.w = (int)w, P.h = (int)h, P.maxval = (int)maxval;
    P.bit_depth     = maxval > 255 ? 16 : 8;
    P.file_channels = rgb ? 3 : 1;
    P.off           = (int64_t)p;
    if (bits) {
        P.kind = kPmBits1, P.sbits = 1;
        P.table[0] = table_entry(255, 255, 255), P.table[1] = 0; // bit 0 is white
    } else if (rgb) {
        P.kind = maxval > 255 ? kPmRgb16 : kPmRgb8, P.sbits = maxval > 255 ? 48 : 24;
    } else {
        P.kind = maxval > 255 ? kPmGray16 : kPmGray8, P.sbits = maxval > 255 ? 16 : 8;
    }
    const uint64_t rowb = ((uint64_t)w * P.sbits + 7) / 8; // w <= 2^28: below 2^31
    P.pitch = (int32_t)rowb;
    if (!need_data) return;
    if (!ascii && rowb * h > size - p) pnm_bad("truncated pixel data");
    // an ASCII sample is a character at least, and a separator too unless it is a P1's: a file too short for
    // its samples is refused here, before anything is sized by its header
    const uint64_t ns = (uint64_t)w * h * (rgb ? 3 : 1);
    if (ascii && (bits ? ns : 2 * ns - 1) > size - p) pnm_bad("the file ends before its samples");
}

void plan_bmp(const uint8_t* d, size_t size, PixmapPlan& P, bool need_data)
{
    P.format = AEON_PIXMAP_BMP;
    const uint32_t offbits = le32(d + 10), hs = le32(d + 14);
    if (hs != 12 && hs < 40) bmp_bad("bad info header size " + std::to_string(hs));
    if (hs > size - 14) bmp_bad("truncated header");
    int64_t  w, h;
    uint32_t bpp, comp = 0, used = 0;
    if (hs == 12) {
        w = le16(d + 18), h = le16(d + 20), bpp = le16(d + 24);
    } else {
        w = (int32_t)le32(d + 18), h = (int32_t)le32(d + 22), bpp = le16(d + 28), comp = le32(d + 30), used = le32(d + 46);
    }
    const int64_t ah = h < 0 ? -h : h;
    if (w < 1 || ah < 1 || (uint64_t)w * (uint64_t)ah > kPixmapMaxPixels) bmp_bad("bad image size");
    if (comp == 1 || comp == 2) bmp_bad(std::string(comp == 1 ? "RLE8" : "RLE4") + " compressed files are not supported", AEON_HIP_EUNSUPPORTED);
    if (comp == 3 || bpp == 16) bmp_bad("16-bit (555 / 565 / bitfields) files are not supported", AEON_HIP_EUNSUPPORTED);
    if (comp != 0) bmp_bad("unknown compression " + std::to_string(comp));
    if (bpp != 1 && bpp != 4 && bpp != 8 && bpp != 24 && bpp != 32) bmp_bad("bad bit count " + std::to_string(bpp));
    if (bpp <= 8) {
        const uint32_t n = (hs == 12 || used == 0) ? 1u << bpp : used, esz = hs == 12 ? 3 : 4;
        if (n > 256) bmp_bad("a palette of more than 256 entries");
        const size_t at = 14 + (size_t)hs;
        if ((size_t)n * esz > size - at) bmp_bad("truncated palette");
        for (uint32_t i = 0; i < n; i++) P.table[i] = table_entry(d[at + i * esz], d[at + i * esz + 1], d[at + i * esz + 2]);
        // (entries past the stored ones stay zero: an index past the palette decodes as black)
    }
    const uint64_t pitch = ((((uint64_t)w * bpp + 7) / 8) + 3) & ~(uint64_t)3;
    if (need_data && (offbits > size || pitch * (uint64_t)ah > size - offbits)) bmp_bad("truncated pixel data");
    P.w = (int)w, P.h = (int)ah, P.bit_depth = 8, P.file_channels = 3, P.sbits = (int)bpp;
    P.kind  = bpp == 1 ? kPmBits1 : bpp == 4 ? kPmBits4 : bpp == 8 ? kPmIndex8 : bpp == 24 ? kPmBgr8 : kPmBgra8;
    // height > 0: bottom-up, output row 0 is the last stored row
    P.off   = h < 0 ? (int64_t)offbits : (int64_t)offbits + (int64_t)pitch * (ah - 1);
    P.pitch = h < 0 ? (int32_t)pitch : -(int32_t)pitch;
}

// need_data false: the header alone (aeon_pixmap_info), the pixel data's extent unchecked
void plan_any(const void* data, size_t size, PixmapPlan& P, bool need_data = true)
{
    const uint8_t* d = (const uint8_t*)data;
    if (sniff_pnm(d, size)) plan_pnm(d, size, P, need_data);
    else if (size >= 18 && d[0] == 'B' && d[1] == 'M') plan_bmp(d, size, P, need_data);
    else throw jpeg_error(AEON_HIP_EINVAL, "BMP / PNM: neither a BMP nor a PNM file");
}

// The samples of an ASCII file: P1 single characters 0 / 1, P2 / P3 decimal tokens clamped to maxval and, up to
// maxval 255, scaled v * 255 / maxval; whitespace and comments between them.
struct AsciiReader {
    const uint8_t* d;
    size_t         size, p;
    int            format, maxval;
    uint32_t next()
    {
        if (format != 1) {
            uint32_t v = pnm_token(d, size, p, "samples");
            if (v > (uint32_t)maxval) v = (uint32_t)maxval;
            return maxval > 255 ? v : v * 255u / (uint32_t)maxval;
        }
        for (;;) {
            while (p < size && is_space(d[p])) p++;
            if (p < size && d[p] == '#') {
                while (p < size && d[p] != '\n' && d[p] != '\r') p++;
                continue;
            }
            break;
        }
        if (p >= size) pnm_bad("the file ends before its samples");
        if (d[p] != '0' && d[p] != '1') pnm_bad("bad samples");
        return d[p++] == '0' ? 255u : 0u;
    }
};

void emit(uint8_t* dst, size_t x, int mode, bool out16, bool wide, uint32_t b, uint32_t g, uint32_t r, bool gray)
{
    if (wide && !out16) b >>= 8, g >>= 8, r >>= 8; // each sample's high byte
    if (mode == AEON_DECODE_BGR8) {
        dst[3 * x] = (uint8_t)b, dst[3 * x + 1] = (uint8_t)g, dst[3 * x + 2] = (uint8_t)r;
        return;
    }
    const uint32_t v = gray ? b : pixmap_gray(b, g, r);
    if (out16) {
        const uint16_t v16 = (uint16_t)v;
        std::memcpy(dst + 2 * x, &v16, 2);
    } else {
        dst[x] = (uint8_t)v;
    }
}

void set_mode(PixmapPlan& P, int mode)
{
    P.channels   = mode == AEON_DECODE_BGR8 ? 3 : 1;
    P.elem_bytes = (mode == AEON_DECODE_ANYDEPTH && P.bit_depth == 16) ? 2 : 1;
}

} // namespace

bool pixmap_sniff(const void* data, size_t size) { return sniff_pnm((const uint8_t*)data, size) || sniff_bmp((const uint8_t*)data, size); }

void pixmap_header(const void* data, size_t size, int* w, int* h, int* bit_depth, int* channels, int* format)
{
    PixmapPlan P;
    plan_any(data, size, P, false);
    *w = P.w, *h = P.h, *bit_depth = P.bit_depth, *channels = P.file_channels, *format = P.format;
}

void pixmap_plan(const void* data, size_t size, int mode, PixmapPlan& P)
{
    plan_any(data, size, P);
    set_mode(P, mode);
    P.route = pixmap_route(P, size) ? 1 : 0;
}

bool pixmap_route(const PixmapPlan& P, size_t size)
{
    return (P.format == AEON_PIXMAP_BMP || P.format >= 4) && size < ((size_t)1 << 31);
}

bool pixmap_routed(const void* data, size_t size)
{
    PixmapPlan P;
    try {
        plan_any(data, size, P);
    } catch (const jpeg_error&) {
        return false;
    }
    return pixmap_route(P, size);
}

void pixmap_decode(const void* data, size_t size, int mode, void* dst_, size_t stride, int* out_elem_bytes)
{
    PixmapPlan P;
    plan_any(data, size, P);
    set_mode(P, mode);
    if (out_elem_bytes) *out_elem_bytes = P.elem_bytes;
    const uint8_t* d     = (const uint8_t*)data;
    uint8_t*       dst   = (uint8_t*)dst_;
    const bool     out16 = P.elem_bytes == 2, wide = P.bit_depth == 16;
    if (P.format >= 1 && P.format <= 3) {
        AsciiReader R{d, size, (size_t)P.off, P.format, P.maxval};
        for (int y = 0; y < P.h; y++)
            for (int x = 0; x < P.w; x++) {
                uint32_t r = R.next(), g = r, b = r;
                if (P.format == 3) g = R.next(), b = R.next();
                emit(dst + (size_t)y * stride, (size_t)x, mode, out16, wide, b, g, r, P.format != 3);
            }
        return;
    }
    for (int y = 0; y < P.h; y++) {
        const uint8_t* row = d + P.off + (int64_t)y * P.pitch;
        uint8_t*       o   = dst + (size_t)y * stride;
        for (int x = 0; x < P.w; x++) {
            uint32_t b, g, r;
            bool     gray = false;
            switch (P.kind) {
            case kPmBits1:
            case kPmBits4:
            case kPmIndex8: {
                const uint32_t idx = P.kind == kPmBits1   ? (row[x >> 3] >> (7 - (x & 7))) & 1u
                                     : P.kind == kPmBits4 ? (row[x >> 1] >> ((x & 1) ? 0 : 4)) & 15u
                                                          : row[x];
                const uint32_t e = P.table[idx];
                if (mode == AEON_DECODE_BGR8) o[3 * x] = (uint8_t)e, o[3 * x + 1] = (uint8_t)(e >> 8), o[3 * x + 2] = (uint8_t)(e >> 16);
                else o[x] = (uint8_t)(e >> 24); // the gray of the palette entry
                continue;
            }
            case kPmGray8: b = g = r = row[x], gray = true; break;
            case kPmGray16: b = g = r = (uint32_t)row[2 * (size_t)x] << 8 | row[2 * (size_t)x + 1], gray = true; break;
            case kPmRgb8: r = row[3 * (size_t)x], g = row[3 * (size_t)x + 1], b = row[3 * (size_t)x + 2]; break;
            case kPmRgb16: {
                const uint8_t* p = row + 6 * (size_t)x;
                r = (uint32_t)p[0] << 8 | p[1], g = (uint32_t)p[2] << 8 | p[3], b = (uint32_t)p[4] << 8 | p[5];
                break;
            }
            case kPmBgr8: b = row[3 * (size_t)x], g = row[3 * (size_t)x + 1], r = row[3 * (size_t)x + 2]; break;
            default: b = row[4 * (size_t)x], g = row[4 * (size_t)x + 1], r = row[4 * (size_t)x + 2]; break; // kPmBgra8
            }
            emit(o, (size_t)x, mode, out16, wide, b, g, r, gray);
        }
    }
}

void pixmap_stage(const void* data, size_t size, int mode, const PixmapPlan& P, PixmapJob& J, uint8_t* file_dst)
{
    std::memset(&J, 0, sizeof(J));
    J.off = P.off, J.pitch = P.pitch, J.kind = P.kind, J.w = P.w, J.h = P.h, J.sbits = P.sbits;
    J.mode = mode, J.elem_bytes = P.elem_bytes;
    std::memcpy(J.table, P.table, sizeof(J.table));
    std::memcpy(file_dst, data, size);
}

bool pixmap_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride)
{
    PixmapPlan P;
    pixmap_plan(data, size, mode, P);
    if (!P.route) return false;
    PixmapJob             J;
    std::vector<uint64_t> file((size + 15) / 16 * 2 + 2, 0); // 16-byte aligned, 16 zero bytes behind the file
    pixmap_stage(data, size, mode, P, J, (uint8_t*)file.data());
    J.src = (uint64_t)file.data(), J.out = (uint64_t)dst, J.stride = (int32_t)stride;
    std::vector<PixmapBand> bands;
    pixmap_bands(J, 0, bands);
    std::vector<uint32_t> tab(256), lds(kPixmapBandBytes / 4 + 2);
    for (const PixmapBand& B : bands) pmdev::convert_band(J, B, tab.data(), (uint8_t*)lds.data());
    return true;
}

} // namespace aeon_hip
