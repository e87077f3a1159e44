// tiff_host.cpp -- the TIFF half of image::extractor::extract / pixel_mask::extractor::extract (aeon
// src/etl_image.cpp:83-99, src/etl_pixel_mask.cpp:30-53): classic TIFF files in strips, restated from the TIFF 6.0
// specification (DESIGN section 21 says which decode rules are pinned against libtiff and which are "parity
// unpinned").  Two users: tiff_decode, the whole decode of one file on the calling thread (aeon_decode_tiff, and
// the files the stage leaves to the host), and the host half of the TIFF stage (aeon_hip_decode_tiff_batch):
// tiff_plan / tiff_stage parse the IFD, refuse what a file can be refused for from its header and the first bytes
// of its strips, build the palette table, the strip and band tables and copy the file; the strips' decoders and
// the conversion are the kernels' (tiff_kernels.hip).  tiff_gpu_emulate runs the kernels' own code
// (tiff_strips.hpp) on the host.  The host's LZW and PackBits decoders here are written apart from the device's
// (a prefix / suffix table, not ranges of the output), and its Deflate is zlib's: the tests hold each against the other.
//
// Every read of the file is checked against `size` first.
#include <zlib.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"
#include "error.hpp" // jpeg_error: an error carrying its AEON_HIP_E* code
#include "pixmap.hpp"
#include "tiff.hpp"
#include "tiff_strips.hpp"

namespace aeon_hip {
namespace {

[[noreturn]] void bad(const std::string& m) { throw jpeg_error(AEON_HIP_EINVAL, "TIFF: " + m); }
[[noreturn]] void unsupported(const std::string& m) { throw jpeg_error(AEON_HIP_EUNSUPPORTED, "TIFF: " + m + " not supported"); }

struct Reader {
    const uint8_t* d;
    size_t         size;
    bool           big;
    uint32_t u16(size_t at) const { return big ? (uint32_t)d[at] << 8 | d[at + 1] : (uint32_t)d[at] | (uint32_t)d[at + 1] << 8; }
    uint32_t u32(size_t at) const { return big ? u16(at) << 16 | u16(at + 2) : u16(at) | u16(at + 2) << 16; }
};

struct Tag {
    uint32_t type = 0, count = 0;
    size_t   at = 0; // where the values lie
    bool     present = false;
};

// The values of a BYTE / SHORT / LONG tag
std::vector<uint32_t> values(const Reader& R, const Tag& t)
{
    std::vector<uint32_t> v(t.count);
    for (uint32_t i = 0; i < t.count; i++)
        v[i] = t.type == 1 ? R.d[t.at + i] : t.type == 3 ? R.u16(t.at + 2 * (size_t)i) : R.u32(t.at + 4 * (size_t)i);
    return v;
}
uint32_t value(const Reader& R, const Tag& t, int tag, uint32_t dflt)
{
    if (!t.present) return dflt;
    if (t.count < 1) bad("tag " + std::to_string(tag) + " holds no value");
    return values(R, Tag{t.type, 1, t.at, true})[0];
}

uint32_t table_entry(uint32_t b, uint32_t g, uint32_t r) { return b | g << 8 | r << 16 | pixmap_gray(b, g, r) << 24; }

bool sniff(const uint8_t* d, size_t size)
{
    if (size < 8) return false;
    const bool ii = d[0] == 'I' && d[1] == 'I' && d[2] == 42 && d[3] == 0, mm = d[0] == 'M' && d[1] == 'M' && d[2] == 0 && d[3] == 42;
    if (!ii && !mm) return false;
    const Reader R{d, size, mm};
    const uint32_t ifd = R.u32(4);
    return ifd >= 8 && (size_t)ifd + 2 <= size;
}

void set_mode(TiffPlan& P, int mode)
{
    P.channels   = mode == AEON_DECODE_BGR8 ? 3 : 1;
    P.elem_bytes = (mode == AEON_DECODE_ANYDEPTH && P.bps == 16 && P.photo <= 1) ? 2 : 1;
}

// The first IFD: every tag the decoder reads, every refusal.  Strip extents are checked against the file, and the
// first bytes of each compressed strip for what makes its whole decoder inapplicable (old-style LZW, a zlib header
// inflate refuses).
void parse(const void* data, size_t size, TiffPlan& P)
{
    const uint8_t* d = (const uint8_t*)data;
    if (size < 8 || !((d[0] == 'I' && d[1] == 'I') || (d[0] == 'M' && d[1] == 'M'))) bad("not a TIFF file");
    Reader R{d, size, d[0] == 'M'};
    const uint32_t version = R.u16(2);
    if (version == 43) unsupported("BigTIFF (version 43) is");
    if (version != 42) bad("bad version " + std::to_string(version));
    const size_t ifd = R.u32(4);
    if (ifd < 8 || ifd + 2 > size) bad("the IFD lies past the end of the file");
    const uint32_t ne = R.u16(ifd);
    if ((size_t)ne * 12 > size - ifd - 2) bad("the IFD lies past the end of the file");
    enum { W, H, BPS, COMP, PHOTO, FILL, SOFF, ORIENT, SPP, RPS, SCNT, PLANAR, PRED, CMAP, TILEW, EXTRA, SFMT, NTAGS };
    static const int ids[NTAGS] = {256, 257, 258, 259, 262, 266, 273, 274, 277, 278, 279, 284, 317, 320, 322, 338, 339};
    Tag tags[NTAGS];
    for (uint32_t e = 0; e < ne; e++) {
        const size_t   at = ifd + 2 + 12 * (size_t)e;
        const uint32_t tag = R.u16(at), type = R.u16(at + 2), count = R.u32(at + 4);
        int k = -1;
        for (int i = 0; i < NTAGS; i++)
            if (ids[i] == (int)tag) k = i;
        if (k < 0) continue;
        if (type != 1 && type != 3 && type != 4) bad("tag " + std::to_string(tag) + " has type " + std::to_string(type));
        const uint64_t bytes = (uint64_t)count * (type == 1 ? 1 : type == 3 ? 2 : 4);
        size_t         where = at + 8;
        if (bytes > 4) {
            where = R.u32(at + 8);
            if (where > size || bytes > size - where) bad("the values of tag " + std::to_string(tag) + " lie past the end of the file");
        }
        tags[k] = Tag{type, count, where, true};
    }
    if (tags[TILEW].present) unsupported("tiled files (TileWidth present) are");
    if (!tags[W].present || !tags[H].present) bad("no ImageWidth / ImageLength");
    const uint32_t w = value(R, tags[W], 256, 0), h = value(R, tags[H], 257, 0);
    if (w < 1 || h < 1) bad("bad image size");
    if (w > INT32_MAX || h > INT32_MAX) unsupported("images above 2^28 pixels are");
    if ((uint64_t)w * h > kTiffMaxPixels) unsupported("images above 2^28 pixels are");
    const uint32_t spp = value(R, tags[SPP], 277, 1);
    if (spp < 1 || spp > 4) unsupported(std::to_string(spp) + " samples per pixel are");
    uint32_t bps = 1;
    if (tags[BPS].present) {
        const std::vector<uint32_t> v = values(R, tags[BPS]);
        if (v.empty()) bad("tag 258 holds no value");
        if (v.size() != 1 && v.size() != spp) bad("BitsPerSample holds " + std::to_string(v.size()) + " values for " + std::to_string(spp) + " samples");
        for (uint32_t b : v)
            if (b != v[0]) unsupported("samples of different widths are");
        bps = v[0];
    }
    if (bps != 8 && bps != 16) unsupported(std::to_string(bps) + "-bit samples are");
    if (tags[SFMT].present) {
        for (uint32_t f : values(R, tags[SFMT])) {
            if (f == 3) unsupported("float samples are");
            if (f != 1 && f != 4) unsupported("signed or complex samples (SampleFormat " + std::to_string(f) + ") are");
        }
    }
    const uint32_t comp = value(R, tags[COMP], 259, 1);
    switch (comp) {
    case 1: P.comp = kTfNone; break;
    case 5: P.comp = kTfLzw; break;
    case 8:
    case 32946: P.comp = kTfDeflate; break;
    case 32773: P.comp = kTfPackBits; break;
    case 2:
    case 3:
    case 4: unsupported("CCITT compression is");
    case 6: unsupported("old-style JPEG compression is");
    case 7: unsupported("JPEG compression is");
    default: unsupported("compression " + std::to_string(comp) + " is");
    }
    if (value(R, tags[PLANAR], 284, 1) == 2 && spp > 1) unsupported("planar-separate files (PlanarConfiguration 2) are");
    if (value(R, tags[PLANAR], 284, 1) > 2 || value(R, tags[PLANAR], 284, 1) < 1) bad("bad PlanarConfiguration");
    const uint32_t fill = value(R, tags[FILL], 266, 1);
    if (fill == 2) unsupported("FillOrder 2 is");
    if (fill != 1) bad("bad FillOrder");
    uint32_t pred = value(R, tags[PRED], 317, 1);
    if (pred == 3) unsupported("the floating-point predictor (Predictor 3) is");
    if (pred != 1 && pred != 2) bad("bad Predictor");
    // libtiff knows the tag under the LZW and Deflate codecs only: an uncompressed or PackBits file's is ignored
    if (P.comp == kTfNone || P.comp == kTfPackBits) pred = 1;
    if (!tags[PHOTO].present) bad("no PhotometricInterpretation");
    const uint32_t photo = value(R, tags[PHOTO], 262, 0);
    if (photo == 5) unsupported("CMYK files are");
    if (photo == 6) unsupported("YCbCr files are");
    if (photo == 8 || photo == 9 || photo == 10) unsupported("CIELab files are");
    if (photo > 3) unsupported("PhotometricInterpretation " + std::to_string(photo) + " is");
    const uint32_t colour = photo == 2 ? 3 : 1;
    if (spp != colour && spp != colour + 1) unsupported(std::to_string(spp) + " samples per pixel with PhotometricInterpretation " + std::to_string(photo) + " are");
    if (tags[EXTRA].present) {
        const std::vector<uint32_t> v = values(R, tags[EXTRA]);
        if (v.size() != spp - colour) bad("ExtraSamples disagrees with SamplesPerPixel");
        for (uint32_t x : v) {
            if (x == 2) unsupported("unassociated alpha (ExtraSamples 2) is");
            if (x > 2) bad("bad ExtraSamples");
        }
    }
    if (photo == 3) {
        if (bps != 8) unsupported("16-bit palette files are");
        if (!tags[CMAP].present || tags[CMAP].type != 3 || tags[CMAP].count != 768) bad("a palette file without a ColorMap of 3 x 256 shorts");
        const std::vector<uint32_t> m = values(R, tags[CMAP]);
        for (int i = 0; i < 256; i++) P.table[i] = table_entry(m[512 + i] >> 8, m[256 + i] >> 8, m[i] >> 8);
    }
    (void)ORIENT; // read by nobody: cv::imdecode of OpenCV 2.4 ignores it
    P.w = (int)w, P.h = (int)h, P.spp = (int)spp, P.bps = (int)bps, P.photo = (int)photo, P.pred = (int)pred, P.big = R.big ? 1 : 0;
    P.file_channels = photo >= 2 ? 3 : 1;
    P.rowb = (size_t)w * spp * (bps / 8);
    uint32_t rps = value(R, tags[RPS], 278, h);
    if (rps < 1) bad("RowsPerStrip 0");
    if (rps > h) rps = h;
    P.rps = rps;
    const uint32_t ns = (h + rps - 1) / rps;
    if (!tags[SOFF].present) bad("no StripOffsets");
    if (tags[SOFF].count < ns) bad(std::to_string(tags[SOFF].count) + " strips where the geometry needs " + std::to_string(ns));
    if (tags[SOFF].type == 1) bad("tag 273 has type 1");
    P.offs = values(R, Tag{tags[SOFF].type, ns, tags[SOFF].at, true});
    if (tags[SCNT].present) {
        if (tags[SCNT].count < ns) bad("StripByteCounts holds " + std::to_string(tags[SCNT].count) + " counts for " + std::to_string(ns) + " strips");
        if (tags[SCNT].type == 1) bad("tag 279 has type 1");
        P.counts = values(R, Tag{tags[SCNT].type, ns, tags[SCNT].at, true});
    } else {
        if (ns != 1 || P.comp != kTfNone) bad("no StripByteCounts");
        P.counts.assign(1, (uint32_t)std::min<uint64_t>(P.rowb * h, UINT32_MAX));
    }
    for (uint32_t s = 0; s < ns; s++) {
        const std::string which = "strip " + std::to_string(s);
        const uint64_t    rows = std::min<uint32_t>(rps, h - s * rps), need = rows * P.rowb;
        if (P.offs[s] > size || P.counts[s] > size - P.offs[s]) bad(which + " lies past the end of the file");
        const uint8_t* p = d + P.offs[s];
        if (P.comp == kTfNone && P.counts[s] < need) bad(which + " holds fewer bytes than its rows");
        if (P.comp == kTfLzw) {
            if (P.counts[s] < 2) bad(which + ": the LZW data ends before its first code");
            if (p[0] != 0x80 || (p[1] & 0x80)) unsupported("old-style LZW (codes LSB first; " + which + " does not start with ClearCode) is");
        }
        if (P.comp == kTfDeflate) {
            // the zlib header as inflate checks it: deflate, a window of 32 KiB at most, no preset dictionary, FCHECK
            if (P.counts[s] < 2) bad(which + ": corrupt or truncated Deflate data");
            const uint32_t cmf = p[0], flg = p[1];
            if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 0x20) || ((cmf << 8) | flg) % 31 != 0) bad(which + ": corrupt or truncated Deflate data");
        }
    }
}

// ---- the host's strip decoders ------------------------------------------------------------------------

// TIFF's LZW with the textbook table: code -> (prefix code, last byte), strings written back to front.
void lzw_host(const uint8_t* p, size_t n, uint8_t* out, size_t need, const std::string& which)
{
    std::vector<uint16_t> prefix(kTiffLzwCodes), length(kTiffLzwCodes);
    std::vector<uint8_t>  suffix(kTiffLzwCodes), first(kTiffLzwCodes);
    for (int i = 0; i < 256; i++) prefix[i] = 0, length[i] = 1, suffix[i] = first[i] = (uint8_t)i;
    size_t   bit = 0, o = 0;
    int      width = 9, next = 258, prev = -1;
    std::vector<uint8_t> str;
    while (o < need) {
        if (bit + width > 8 * n) bad(which + ": the LZW data ends before its rows");
        uint32_t code = 0;
        for (int k = 0; k < width; k++, bit++) code = code << 1 | ((p[bit >> 3] >> (7 - (bit & 7))) & 1u);
        if (code == 256) {
            width = 9, next = 258, prev = -1;
            continue;
        }
        if (code == 257) break;
        if (prev < 0) {
            if (code > 255) bad(which + ": corrupt LZW data (no literal after ClearCode)");
            out[o++] = (uint8_t)code, prev = (int)code;
            continue;
        }
        if ((int)code > next) bad(which + ": corrupt LZW data (code " + std::to_string(code) + " above the table)");
        // the string of `code`: its own, or prev's plus prev's first byte
        str.clear();
        int c = (int)code;
        if (c == next) str.push_back(first[prev]), c = prev; // (next == 4096 cannot be a code)
        for (; c >= 258; c = prefix[c]) str.push_back(suffix[c]);
        str.push_back((uint8_t)c);
        const uint8_t head = str.back();
        for (size_t i = str.size(); i-- > 0 && o < need;) out[o++] = str[i];
        if (next < kTiffLzwCodes) {
            prefix[next] = (uint16_t)prev, suffix[next] = head, first[next] = first[prev];
            next++;
            if (next + 1 >= (1 << width) && width < 12) width++;
        }
        prev = (int)code;
    }
    if (o < need) bad(which + ": the LZW data ends before its rows");
}

void packbits_host(const uint8_t* p, size_t n, uint8_t* out, size_t need, const std::string& which)
{
    size_t i = 0, o = 0;
    while (o < need) {
        if (i >= n) bad(which + ": the PackBits data ends before its rows");
        const int c = (int8_t)p[i++];
        if (c == -128) continue;
        const size_t cnt = c >= 0 ? (size_t)c + 1 : (size_t)(1 - c);
        if (cnt > need - o) bad(which + ": a PackBits run past the strip's rows");
        if (c >= 0) {
            if (cnt > n - i) bad(which + ": a PackBits run past the strip's bytes");
            std::memcpy(out + o, p + i, cnt), i += cnt;
        } else {
            if (i >= n) bad(which + ": a PackBits run past the strip's bytes");
            std::memset(out + o, p[i++], cnt);
        }
        o += cnt;
    }
}

void deflate_host(const uint8_t* p, size_t n, uint8_t* out, size_t need, const std::string& which)
{
    z_stream zs{};
    if (inflateInit(&zs) != Z_OK) bad("inflateInit failed");
    zs.next_in = (Bytef*)p, zs.avail_in = (uInt)n;
    zs.next_out = out, zs.avail_out = (uInt)need;
    const int    zr  = inflate(&zs, Z_FINISH);
    const size_t got = need - zs.avail_out;
    inflateEnd(&zs);
    if ((zr != Z_STREAM_END && zr != Z_BUF_ERROR && zr != Z_OK) || got < need) bad(which + ": corrupt or truncated Deflate data");
}

// One row of native samples (the predictor undone) into the record's row
void emit_row(const TiffPlan& P, int mode, const uint16_t* s, uint8_t* o)
{
    const bool     wide = P.bps == 16, out16 = P.elem_bytes == 2;
    const uint32_t max = wide ? 65535 : 255;
    for (int x = 0; x < P.w; x++, s += P.spp) {
        uint32_t b, g, r;
        bool     gray = true;
        if (P.photo == 3) {
            const uint32_t e = P.table[s[0] & 255];
            if (mode == AEON_DECODE_BGR8) o[3 * x] = (uint8_t)e, o[3 * x + 1] = (uint8_t)(e >> 8), o[3 * x + 2] = (uint8_t)(e >> 16);
            else o[x] = (uint8_t)(e >> 24);
            continue;
        }
        if (P.photo == 2) r = s[0], g = s[1], b = s[2], gray = false;
        else b = g = r = P.photo == 0 ? max - s[0] : s[0];
        if (out16) {
            const uint16_t v = (uint16_t)r;
            std::memcpy(o + 2 * (size_t)x, &v, 2);
            continue;
        }
        if (wide) b >>= 8, g >>= 8, r >>= 8;
        if (mode == AEON_DECODE_BGR8) o[3 * x] = (uint8_t)b, o[3 * x + 1] = (uint8_t)g, o[3 * x + 2] = (uint8_t)r;
        else o[x] = (uint8_t)(gray ? r : pixmap_gray(b, g, r));
    }
}

} // namespace

bool tiff_sniff(const void* data, size_t size) { return sniff((const uint8_t*)data, size); }

bool tiff_route(const TiffPlan& P, size_t size)
{
    if (size >= ((size_t)1 << 31) || P.rowb * (size_t)P.h >= ((size_t)1 << 31)) return false;
    if ((P.comp == kTfLzw || P.comp == kTfPackBits) && (size_t)P.rps * P.rowb > (size_t)kTiffStripCap) return false;
    return true;
}

void tiff_plan(const void* data, size_t size, int mode, TiffPlan& P)
{
    parse(data, size, P);
    set_mode(P, mode);
    P.route = tiff_route(P, size) ? 1 : 0;
}

bool tiff_routed(const void* data, size_t size)
{
    TiffPlan P;
    try {
        parse(data, size, P);
    } catch (const jpeg_error&) {
        return false;
    }
    if (!tiff_route(P, size)) return false;
    if (P.comp != kTfDeflate) return true;
    uint64_t comp_bytes = 0;
    for (uint32_t c : P.counts) comp_bytes += c;
    return comp_bytes * kTiffDecoderDeflateMinRatio <= (uint64_t)P.rowb * (uint64_t)P.h;
}

void tiff_decode(const void* data, size_t size, int mode, void* dst_, size_t stride, int* out_elem_bytes)
{
    TiffPlan P;
    parse(data, size, P);
    set_mode(P, mode);
    if (out_elem_bytes) *out_elem_bytes = P.elem_bytes;
    const uint8_t*        d = (const uint8_t*)data;
    uint8_t*              dst = (uint8_t*)dst_;
    const size_t          ns_row = (size_t)P.w * P.spp;
    std::vector<uint8_t>  buf;
    std::vector<uint16_t> row(ns_row);
    for (size_t s = 0; s < P.offs.size(); s++) {
        const std::string which = "strip " + std::to_string(s);
        const int         y0 = (int)(s * P.rps), rows = std::min<int>((int)P.rps, P.h - y0);
        const size_t      need = (size_t)rows * P.rowb;
        const uint8_t*    src = d + P.offs[s];
        if (P.comp != kTfNone) {
            buf.resize(need);
            if (P.comp == kTfLzw) lzw_host(src, P.counts[s], buf.data(), need, which);
            else if (P.comp == kTfPackBits) packbits_host(src, P.counts[s], buf.data(), need, which);
            else deflate_host(src, P.counts[s], buf.data(), need, which);
            src = buf.data();
        }
        for (int r = 0; r < rows; r++) {
            const uint8_t* p = src + (size_t)r * P.rowb;
            for (size_t i = 0; i < ns_row; i++)
                row[i] = P.bps == 8 ? p[i] : P.big ? (uint16_t)(p[2 * i] << 8 | p[2 * i + 1]) : (uint16_t)(p[2 * i] | p[2 * i + 1] << 8);
            if (P.pred == 2) {
                const uint32_t mask = P.bps == 8 ? 255 : 65535;
                for (size_t i = (size_t)P.spp; i < ns_row; i++) row[i] = (uint16_t)((row[i] + row[i - P.spp]) & mask);
            }
            emit_row(P, mode, row.data(), dst + (size_t)(y0 + r) * stride);
        }
    }
}

size_t tiff_scratch_bytes(const TiffPlan& P)
{
    if (P.comp == kTfNone) return 0;
    size_t total = 16; // (the band loads' aligned over-read behind the last strip)
    for (size_t s = 0; s < P.offs.size(); s++) {
        const size_t rows = std::min<size_t>(P.rps, (size_t)P.h - s * P.rps);
        total += (rows * P.rowb + 15) & ~(size_t)15;
    }
    return total;
}

void tiff_stage(const void* data, size_t size, int mode, const TiffPlan& P, int job, TiffJob& J, std::vector<TiffStrip>& strips,
                std::vector<TiffBand>& bands, uint8_t* file_dst)
{
    std::memset(&J, 0, sizeof(J));
    J.w = P.w, J.h = P.h, J.spp = P.spp, J.bps = P.bps, J.photo = P.photo, J.pred = P.pred, J.big = P.big, J.comp = P.comp;
    J.mode = mode, J.elem_bytes = P.elem_bytes, J.rowb = (int32_t)P.rowb;
    std::memcpy(J.table, P.table, sizeof(J.table));
    const int band_rows = P.rowb <= (size_t)kTiffBandBytes ? (int)((size_t)kTiffBandBytes / P.rowb) : 1;
    size_t    soff = 0;
    for (size_t s = 0; s < P.offs.size(); s++) {
        const int    y0 = (int)(s * P.rps), rows = std::min<int>((int)P.rps, P.h - y0);
        const size_t need = (size_t)rows * P.rowb;
        int64_t      src = P.offs[s];
        if (P.comp != kTfNone) {
            strips.push_back(TiffStrip{job, P.comp, P.offs[s], P.counts[s], y0, rows, (uint32_t)need, 0, soff, 0});
            src = (int64_t)soff;
            soff += (need + 15) & ~(size_t)15;
        }
        for (int r = 0; r < rows; r += band_rows)
            bands.push_back(TiffBand{job, y0 + r, std::min(band_rows, rows - r), 0, src + (int64_t)((size_t)r * P.rowb), 0});
    }
    if (file_dst) std::memcpy(file_dst, data, size);
}

int tiff_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride)
{
    TiffPlan P;
    tiff_plan(data, size, mode, P);
    if (!P.route) return 0;
    TiffJob                J;
    std::vector<TiffStrip> strips;
    std::vector<TiffBand>  bands;
    std::vector<uint64_t>  file((size + 15) / 16 * 2 + 2, 0), raw(tiff_scratch_bytes(P) / 8 + 2, 0); // 16-byte aligned, zero padding behind
    tiff_stage(data, size, mode, P, 0, J, strips, bands, (uint8_t*)file.data());
    J.src = (uint64_t)file.data(), J.raw = (uint64_t)raw.data(), J.out = (uint64_t)dst, J.stride = (int32_t)stride;
    std::vector<tiffdev::ExpandMem> mem(1);
    for (const TiffStrip& T : strips)
        if (!tiffdev::expand_strip(J, T, mem[0])) return -1;
    std::vector<uint32_t> tab(256), lds(kTiffBandBytes / 4 + 2);
    for (const TiffBand& B : bands) tiffdev::convert_band(J, B, tab.data(), (uint8_t*)lds.data());
    return 1;
}

} // namespace aeon_hip
