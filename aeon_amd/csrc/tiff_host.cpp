// tiff_host.cpp -- the TIFF half of image::extractor::extract / pixel_mask::extractor::extract (aeon
// src/etl_image.cpp:83-99, src/etl_pixel_mask.cpp:30-53): classic TIFF files in strips or tiles, restated from the TIFF 6.0
// specification (DESIGN section 21 says which decode rules are pinned against libtiff and which are "parity
// unpinned").  Two users: tiff_decode, the whole decode of one file on the calling thread (aeon_decode_tiff, and
// the files the stage leaves to the host), and the host half of the TIFF stage (aeon_hip_decode_tiff_batch):
// tiff_plan / tiff_stage parse the IFD, refuse what a file can be refused for from its header and the first bytes
// of its strips, build the palette table, the strip and band tables and copy the file; the strips' decoders and
// the conversion are the kernels' (tiff_kernels.hip).  tiff_gpu_emulate runs the kernels' own code
// (tiff_strips.hpp) on the host; with `large`, under the opt-in call's routing (tiff_route_large), tiff_expand_large's too.  The host's LZW and PackBits decoders here are written apart from the device's
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
    enum { W, H, BPS, COMP, PHOTO, FILL, SOFF, ORIENT, SPP, RPS, SCNT, PLANAR, PRED, CMAP, TILEW, TILEL, TOFF, TCNT, EXTRA, SFMT, NTAGS };
    static const int ids[NTAGS] = {256, 257, 258, 259, 262, 266, 273, 274, 277, 278, 279, 284, 317, 320, 322, 323, 324, 325, 338, 339};
    Tag tags[NTAGS];
    bool tiled = false;
    for (uint32_t e = 0; e < ne; e++) tiled = tiled || R.u16(ifd + 2 + 12 * (size_t)e) == 322;
    for (uint32_t e = 0; e < ne; e++) {
        const size_t   at = ifd + 2 + 12 * (size_t)e;
        const uint32_t tag = R.u16(at), type = R.u16(at + 2), count = R.u32(at + 4);
        int k = -1;
        for (int i = 0; i < NTAGS; i++)
            if (ids[i] == (int)tag) k = i;
        if (k < 0) continue;
        if (!tiled && (k == TILEL || k == TOFF || k == TCNT)) continue; // a strip file's stray tile tags: not read at all
        if (type != 1 && type != 3 && type != 4) bad("tag " + std::to_string(tag) + " has type " + std::to_string(type));
        const uint64_t bytes = (uint64_t)count * (type == 1 ? 1 : type == 3 ? 2 : 4);
        size_t         where = at + 8;
        if (bytes > 4) {
            where = R.u32(at + 8);
            if (where > size || bytes > size - where) bad("the values of tag " + std::to_string(tag) + " lie past the end of the file");
        }
        tags[k] = Tag{type, count, where, true};
    }
    if (tiled && !(tags[TILEL].present && tags[TOFF].present && tags[TCNT].present))
        unsupported("tiled files (TileWidth present) without TileLength, TileOffsets and TileByteCounts are");
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
    uint32_t ns;
    if (tiled) {
        const uint32_t tw = value(R, tags[TILEW], 322, 0), tl = value(R, tags[TILEL], 323, 0);
        if (tw < 16 || tw % 16) unsupported("TileWidth " + std::to_string(tw) + " (not a multiple of 16) is");
        if (tl < 16 || tl % 16) unsupported("TileLength " + std::to_string(tl) + " (not a multiple of 16) is");
        if ((uint64_t)tw * tl > kTiffMaxPixels) unsupported("tiles above 2^28 pixels are");
        P.tw = tw, P.tl = tl, P.tacross = (w - 1) / tw + 1, P.tdown = (h - 1) / tl + 1;
        const uint64_t nt = (uint64_t)P.tacross * P.tdown;
        if (tags[TOFF].count != nt) bad(std::to_string(tags[TOFF].count) + " tiles where the geometry needs " + std::to_string(nt));
        if (tags[TCNT].count != nt) bad("TileByteCounts holds " + std::to_string(tags[TCNT].count) + " counts for " + std::to_string(nt) + " tiles");
        if (tags[TOFF].type == 1) bad("tag 324 has type 1");
        if (tags[TCNT].type == 1) bad("tag 325 has type 1");
        ns      = (uint32_t)nt;
        rps     = std::min(tl, h);
        P.offs   = values(R, tags[TOFF]);
        P.counts = values(R, tags[TCNT]);
    } else {
        if (rps < 1) bad("RowsPerStrip 0");
        if (rps > h) rps = h;
        ns = (h + rps - 1) / rps;
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
    }
    P.rps = rps;
    // every strip's (tile's) extent, and the first bytes of a compressed one
    for (uint32_t s = 0; s < ns; s++) {
        const std::string which = (tiled ? "tile " : "strip ") + std::to_string(s);
        const uint64_t    need = tiled ? P.tile_bytes() : std::min<uint32_t>(rps, h - s * rps) * (uint64_t)P.rowb;
        if (P.offs[s] > size || P.counts[s] > size - P.offs[s]) bad(which + " lies past the end of the file");
        const uint8_t* p = d + P.offs[s];
        if (P.comp == kTfNone && P.counts[s] < need) bad(which + (tiled ? " holds fewer bytes than a tile" : " holds fewer bytes than its rows"));
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

namespace {
// cap: the most bytes an LZW / PackBits strip or tile may decode to
bool route(const TiffPlan& P, size_t size, size_t cap)
{
    if (size >= ((size_t)1 << 31) || P.rowb * (size_t)P.h >= ((size_t)1 << 31)) return false;
    if (P.tw) {
        if ((uint64_t)P.offs.size() * ((P.tile_bytes() + 15) & ~(size_t)15) >= ((uint64_t)1 << 31)) return false;
        if ((size_t)P.tw * P.spp * (P.bps / 8) > (size_t)kTiffBandBytes) return false; // one tile row is the least a band stages
        return !((P.comp == kTfLzw || P.comp == kTfPackBits) && P.tile_bytes() > cap);
    }
    if ((P.comp == kTfLzw || P.comp == kTfPackBits) && (size_t)P.rps * P.rowb > cap) return false;
    return true;
}
} // namespace

bool tiff_route(const TiffPlan& P, size_t size) { return route(P, size, (size_t)kTiffStripCap); }
bool tiff_route_large(const TiffPlan& P, size_t size) { return route(P, size, SIZE_MAX); } // (a strip is below 2^31 as its rows are)

void tiff_plan(const void* data, size_t size, int mode, TiffPlan& P, bool large)
{
    parse(data, size, P);
    set_mode(P, mode);
    P.route = (large ? tiff_route_large(P, size) : tiff_route(P, size)) ? 1 : 0;
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
    const uint64_t decoded = P.tw ? (uint64_t)P.tile_bytes() * P.offs.size() : (uint64_t)P.rowb * (uint64_t)P.h;
    return comp_bytes * kTiffDecoderDeflateMinRatio <= decoded;
}

namespace {

// Strip or tile s decoded: `need` bytes, in the file itself or in buf
const uint8_t* unit_bytes(const TiffPlan& P, const uint8_t* d, size_t s, size_t need, std::vector<uint8_t>& buf, const std::string& which)
{
    const uint8_t* src = d + P.offs[s];
    if (P.comp == kTfNone) return src;
    buf.resize(need);
    if (P.comp == kTfLzw) lzw_host(src, P.counts[s], buf.data(), need, which);
    else if (P.comp == kTfPackBits) packbits_host(src, P.counts[s], buf.data(), need, which);
    else deflate_host(src, P.counts[s], buf.data(), need, which);
    return buf.data();
}

// ns stored samples at p made native, the predictor undone from the first pixel on
void native_row(const TiffPlan& P, const uint8_t* p, size_t ns, uint16_t* row)
{
    for (size_t i = 0; i < ns; i++)
        row[i] = P.bps == 8 ? p[i] : P.big ? (uint16_t)(p[2 * i] << 8 | p[2 * i + 1]) : (uint16_t)(p[2 * i] | p[2 * i + 1] << 8);
    if (P.pred == 2) {
        const uint32_t mask = P.bps == 8 ? 255 : 65535;
        for (size_t i = (size_t)P.spp; i < ns; i++) row[i] = (uint16_t)((row[i] + row[i - P.spp]) & mask);
    }
}

// A tiled file: one row of tiles at a time, every tile's live rows put side by side (the predictor runs along
// each tile's own rows), then the image's rows emitted up to w.
void decode_tiles(const TiffPlan& P, int mode, const uint8_t* d, uint8_t* dst, size_t stride)
{
    const size_t          seg = (size_t)P.tw * P.spp, segb = seg * (P.bps / 8), pitch = seg * P.tacross;
    std::vector<uint8_t>  buf;
    std::vector<uint16_t> rows(pitch * std::min<size_t>(P.tl, (size_t)P.h));
    for (uint32_t ty = 0; ty < P.tdown; ty++) {
        const int y0 = (int)(ty * P.tl), live = std::min<int>((int)P.tl, P.h - y0);
        for (uint32_t tx = 0; tx < P.tacross; tx++) {
            const size_t   t = (size_t)ty * P.tacross + tx;
            const uint8_t* src = unit_bytes(P, d, t, P.tile_bytes(), buf, "tile " + std::to_string(t));
            for (int r = 0; r < live; r++) native_row(P, src + (size_t)r * segb, seg, rows.data() + (size_t)r * pitch + tx * seg);
        }
        for (int r = 0; r < live; r++) emit_row(P, mode, rows.data() + (size_t)r * pitch, dst + (size_t)(y0 + r) * stride);
    }
}

} // namespace

void tiff_decode(const void* data, size_t size, int mode, void* dst_, size_t stride, int* out_elem_bytes)
{
    TiffPlan P;
    parse(data, size, P);
    set_mode(P, mode);
    if (out_elem_bytes) *out_elem_bytes = P.elem_bytes;
    const uint8_t*        d = (const uint8_t*)data;
    uint8_t*              dst = (uint8_t*)dst_;
    if (P.tw) return decode_tiles(P, mode, d, dst, stride);
    const size_t          ns_row = (size_t)P.w * P.spp;
    std::vector<uint8_t>  buf;
    std::vector<uint16_t> row(ns_row);
    for (size_t s = 0; s < P.offs.size(); s++) {
        const int      y0 = (int)(s * P.rps), rows = std::min<int>((int)P.rps, P.h - y0);
        const uint8_t* src = unit_bytes(P, d, s, (size_t)rows * P.rowb, buf, "strip " + std::to_string(s));
        for (int r = 0; r < rows; r++) {
            native_row(P, src + (size_t)r * P.rowb, ns_row, row.data());
            emit_row(P, mode, row.data(), dst + (size_t)(y0 + r) * stride);
        }
    }
}

size_t tiff_scratch_bytes(const TiffPlan& P)
{
    if (P.comp == kTfNone) return 0;
    size_t total = 16; // (the band loads' aligned over-read behind the last strip)
    if (P.tw) return total + P.offs.size() * ((P.tile_bytes() + 15) & ~(size_t)15);
    for (size_t s = 0; s < P.offs.size(); s++) {
        const size_t rows = std::min<size_t>(P.rps, (size_t)P.h - s * P.rps);
        total += (rows * P.rowb + 15) & ~(size_t)15;
    }
    return total;
}

namespace {

// The table a compressed strip or tile of `need` decoded bytes belongs to: tiff_expand's, or tiff_expand_large's
std::vector<TiffStrip>& table_of(TiffTables& T, int comp, size_t need)
{
    return (comp == kTfLzw || comp == kTfPackBits) && need > (size_t)kTiffStripCap ? T.large : T.strips;
}

// A tiled file's tables: every compressed tile a strip of tiff_expand's, tile after tile in the scratch; every row
// of tiles cut into bands of at most kTiffBandBytes -- all its tiles across times the rows that fit, or, where one
// row of them is too wide, equal runs of tiles across, row by row.
void stage_tiles(const TiffPlan& P, int job, TiffJob& J, TiffTables& T)
{
    J.tw = (int32_t)P.tw, J.tl = (int32_t)P.tl, J.tacross = (int32_t)P.tacross, J.tile0 = (int32_t)T.tile_src.size();
    const size_t need = P.tile_bytes(), slot = (need + 15) & ~(size_t)15, segb = need / P.tl;
    for (size_t t = 0; t < P.offs.size(); t++) {
        if (P.comp != kTfNone) table_of(T, P.comp, need).push_back(TiffStrip{job, P.comp, P.offs[t], P.counts[t], 0, (int32_t)P.tl, (uint32_t)need, 0, t * slot, 0});
        T.tile_src.push_back(P.comp != kTfNone ? (uint32_t)(t * slot) : P.offs[t]);
    }
    const uint32_t most = (uint32_t)((size_t)kTiffBandBytes / segb), runs = (P.tacross + most - 1) / most, nt = (P.tacross + runs - 1) / runs;
    const int      band_rows = std::max<int>(1, (int)((size_t)kTiffBandBytes / (nt * segb)));
    for (uint32_t ty = 0; ty < P.tdown; ty++) {
        const int y0 = (int)(ty * P.tl), live = std::min<int>((int)P.tl, P.h - y0);
        for (int r = 0; r < live; r += band_rows)
            for (uint32_t tx = 0; tx < P.tacross; tx += nt)
                T.tbands.push_back(TiffTileBand{job, y0 + r, std::min(band_rows, live - r), (int32_t)std::min(nt, P.tacross - tx),
                                                (int32_t)(ty * P.tacross + tx), r, (int32_t)(tx * P.tw), 0});
    }
}

} // namespace

void tiff_stage(const void* data, size_t size, int mode, const TiffPlan& P, int job, TiffJob& J, TiffTables& T, uint8_t* file_dst)
{
    std::vector<TiffBand>& bands = T.bands;
    std::memset(&J, 0, sizeof(J));
    J.w = P.w, J.h = P.h, J.spp = P.spp, J.bps = P.bps, J.photo = P.photo, J.pred = P.pred, J.big = P.big, J.comp = P.comp;
    J.mode = mode, J.elem_bytes = P.elem_bytes, J.rowb = (int32_t)P.rowb;
    std::memcpy(J.table, P.table, sizeof(J.table));
    if (P.tw) {
        stage_tiles(P, job, J, T);
        if (file_dst) std::memcpy(file_dst, data, size);
        return;
    }
    const int band_rows = P.rowb <= (size_t)kTiffBandBytes ? (int)((size_t)kTiffBandBytes / P.rowb) : 1;
    size_t    soff = 0;
    for (size_t s = 0; s < P.offs.size(); s++) {
        const int    y0 = (int)(s * P.rps), rows = std::min<int>((int)P.rps, P.h - y0);
        const size_t need = (size_t)rows * P.rowb;
        int64_t      src = P.offs[s];
        if (P.comp != kTfNone) {
            table_of(T, P.comp, need).push_back(TiffStrip{job, P.comp, P.offs[s], P.counts[s], y0, rows, (uint32_t)need, 0, soff, 0});
            src = (int64_t)soff;
            soff += (need + 15) & ~(size_t)15;
        }
        for (int r = 0; r < rows; r += band_rows)
            bands.push_back(TiffBand{job, y0 + r, std::min(band_rows, rows - r), 0, src + (int64_t)((size_t)r * P.rowb), 0});
    }
    if (file_dst) std::memcpy(file_dst, data, size);
}

int tiff_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride, bool large)
{
    TiffPlan P;
    tiff_plan(data, size, mode, P, large);
    if (!P.route) return 0;
    TiffJob               J;
    TiffTables            T;
    std::vector<uint64_t> file((size + 15) / 16 * 2 + 2, 0), raw(tiff_scratch_bytes(P) / 8 + 2, 0); // 16-byte aligned, zero padding behind
    tiff_stage(data, size, mode, P, 0, J, T, (uint8_t*)file.data());
    J.src = (uint64_t)file.data(), J.raw = (uint64_t)raw.data(), J.out = (uint64_t)dst, J.stride = (int32_t)stride;
    std::vector<tiffdev::ExpandMem> mem(1);
    for (const TiffStrip& S : T.strips)
        if (!tiffdev::expand_strip(J, S, mem[0])) return -1;
    std::vector<tiffdev::LargeMem> wide(T.large.empty() ? 0 : 1);
    for (const TiffStrip& S : T.large)
        if (!tiffdev::expand_strip_large(J, S, wide[0])) return -1;
    std::vector<uint32_t> tab(256), lds(kTiffBandBytes / 4 + 2);
    for (const TiffBand& B : T.bands) tiffdev::convert_band(J, B, tab.data(), (uint8_t*)lds.data());
    for (const TiffTileBand& B : T.tbands) tiffdev::convert_tiled_band(J, B, T.tile_src.data(), tab.data(), (uint8_t*)lds.data());
    return 1;
}

} // namespace aeon_hip
