// tiff.hpp -- the TIFF decoder (classic TIFF in strips or tiles, what cv::imdecode reads beside JPEG, PNG, BMP and PNM): its
// host functions (tiff_host.cpp) behind aeon_tiff_info / aeon_decode_tiff and the decoder's providers, and the
// descriptors the host half of the TIFF stage shares with its kernels (tiff_kernels.hip, tiff_strips.hpp).
// The host functions throw jpeg_error (error.hpp) on a file they refuse; messages start with "TIFF:".
//
// The stage (aeon_hip_decode_tiff_batch): the host parses each file's first IFD, refuses what can be refused from
// the header and the first bytes of each strip, builds the file's 256-entry table (palette and gray of each
// entry), the call's strip table and band table, and copies the file as it is into pinned staging; tiff_expand
// (one wave per compressed strip) decodes LZW, PackBits and Deflate strips into the file's scratch, tiff_convert
// (one workgroup per band of rows) makes the samples native, undoes the horizontal predictor and converts the
// rows into the record.  A tiled file's tiles stand where strips stand in tiff_expand; tiff_convert_tiled (one
// workgroup per tiled band) puts their rows together in LDS and converts them.  Files with LZW / PackBits strips
// or tiles above 32 KiB stay with tiff_decode on the host (tiff_route) -- unless the caller asks for them
// (aeon_hip_decode_tiff_large_batch, tiff_route_large): then tiff_expand_large, one wave per such strip or tile, decodes
// them through a 16 KiB window of LDS, many LZW codes a step.  The decode rules are DESIGN section 21.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/aeon_hip.h" // AEON_DECODE_*

namespace aeon_hip {

enum TiffComp : int32_t { kTfNone = 0, kTfLzw, kTfDeflate, kTfPackBits };

constexpr int    kTiffCorruptBit = 2048;      // device error word: a TIFF strip the GPU stage refuses
constexpr int    kTiffLanes      = 256;       // tiff_convert workgroup
constexpr int    kTiffBandBytes  = 16 * 1024; // most source bytes of one band or piece of a row (LDS: these + 8)
constexpr int    kTiffStripCap   = 32 * 1024; // most decoded bytes of an LZW / PackBits strip on the device (LDS)
constexpr int    kTiffChunk      = 16 * 1024; // tiff_expand_large: the window of a strip's output that a wave holds in LDS
constexpr int    kTiffLzwCodes   = 4096;
constexpr size_t kTiffMaxPixels  = (size_t)1 << 28;

// One device-decoded file (device addresses; the emulation's are host addresses).
struct alignas(16) TiffJob {
    uint64_t src; // the file in the staging: 16-byte aligned, at least 16 zero bytes behind it
    uint64_t raw; // compressed files: the scratch of the file's decoded strips (each 16-byte aligned)
    uint64_t out; // the record
    int32_t  w, h;
    int32_t  spp, bps;    // samples per pixel in the file (an extra one included), bits per sample (8 or 16)
    int32_t  photo, pred; // PhotometricInterpretation 0..3, Predictor 1 or 2
    int32_t  big, comp;   // 1: big-endian file; TiffComp
    int32_t  mode, elem_bytes;
    int32_t  stride; // bytes between the record's rows
    int32_t  rowb;   // bytes of a source row
    int32_t  tw, tl;  // tiled files: TileWidth, TileLength (0: strips)
    int32_t  tacross; // ... tiles across
    int32_t  tile0;   // ... the file's first entry in the call's table of tile sources
    uint32_t table[256]; // entry i: B | G << 8 | R << 16 | gray << 24 of palette index i
};
static_assert(sizeof(TiffJob) % 16 == 0, "TiffJob: 16-byte aligned array elements");

// One compressed strip or tile: tiff_expand's unit of work, and tiff_expand_large's (an LZW / PackBits one above kTiffStripCap).
struct alignas(16) TiffStrip {
    int32_t  job, comp;
    uint32_t off, bytes; // the strip's bytes in the file
    int32_t  y0, rows;
    uint32_t need, pad_; // decoded bytes: rows * rowb; a tile's TileLength * TileWidth * bytes per pixel, padding included
    uint64_t soff;       // where they go in the job's scratch (16-byte aligned, room for `need` rounded up to 16)
    uint64_t pad2_;
};
static_assert(sizeof(TiffStrip) == 48, "TiffStrip layout");

// One workgroup's work in tiff_convert: rows [y0, y0 + rows) of a job, all inside one strip, whose source bytes
// start at `src` (a byte offset into the file, or into the scratch of a compressed file).  A row wider than
// kTiffBandBytes is a band of its own (rows == 1) that the workgroup walks in pieces.
struct alignas(16) TiffBand {
    int32_t job, y0, rows, pad_;
    int64_t src;
    int64_t pad2_;
};

// One workgroup's work in tiff_convert_tiled: image rows [y0, y0 + rows) -- all inside one row of tiles, r0 rows below
// its top -- times `nt` tiles across from the job's tile `tile` (pixels from px0 on).  The band's source bytes,
// rows * nt * TileWidth * bytes per pixel, fit kTiffBandBytes.
struct alignas(16) TiffTileBand {
    int32_t job, y0, rows, nt;
    int32_t tile, r0, px0, pad_;
};

// What the host half learns from a file's IFD.
struct TiffPlan {
    int      w = 0, h = 0, spp = 1, bps = 1, photo = -1, pred = 1, big = 0, comp = kTfNone;
    int      channels = 1, elem_bytes = 1; // of the record in the requested mode
    int      file_channels = 1;            // 3: RGB or palette, 1: gray
    uint32_t rps = 0;                      // rows per strip, at most h
    uint32_t tw = 0, tl = 0;               // tiled files: TileWidth, TileLength (0: strips), both multiples of 16
    uint32_t tacross = 0, tdown = 0;       // ... ceil(w / tw), ceil(h / tl)
    int      route = 0;                    // 1: the device decodes the file (tiff_route)
    size_t   rowb = 0;
    std::vector<uint32_t> offs, counts;    // per strip (ceil(h / rps) of them) or per tile (tacross * tdown, row by row)
    uint32_t table[256] = {};
    size_t   tile_bytes() const { return (size_t)tl * tw * spp * (bps / 8); } // a decoded tile, padding included
};

// The tables of one device call, which tiff_stage appends a file's entries to.
struct TiffTables {
    std::vector<TiffStrip>    strips;
    std::vector<TiffStrip>    large; // the LZW / PackBits strips and tiles above kTiffStripCap (tiff_route_large alone admits them)
    std::vector<TiffBand>     bands;
    std::vector<TiffTileBand> tbands;
    std::vector<uint32_t>     tile_src; // per tile of every tiled file: its first byte in the file, or in the file's scratch
};

// true when the first bytes are a classic TIFF's as the decoder's inspect step sniffs them (strict: II 2A 00 /
// MM 00 2A and an IFD offset inside the file; anything else is left to the JPEG parser and its error)
bool tiff_sniff(const void* data, size_t size);
// The IFD parse (refusals and messages of tiff_decode), the table and the routing rule.
// (large: P.route by tiff_route_large)
void tiff_plan(const void* data, size_t size, int mode, TiffPlan& P, bool large = false);
// the whole decode on the calling thread into rows `stride` bytes apart; out_elem_bytes (optional): 1 or 2
void tiff_decode(const void* data, size_t size, int mode, void* dst, size_t stride, int* out_elem_bytes);
// The routing rule: a file below 2^31 bytes (decoded too, a tiled file's padding included) whose LZW / PackBits
// strips or tiles decode to at most kTiffStripCap bytes each goes to the device.  (Rows of any width fit
// tiff_convert: it walks a wide row in pieces; tiff_convert_tiled cuts a row of tiles into bands, and only a
// tile whose single row is above kTiffBandBytes, 2,048 pixels of four 16-bit samples, stays on the host.)
bool tiff_route(const TiffPlan& P, size_t size);
// The same rule with the strip cap lifted (the 2^31 limits and the tiled band-width limit stay): what the opt-in
// call sends to the device, its LZW / PackBits strips above the cap through tiff_expand_large.
bool tiff_route_large(const TiffPlan& P, size_t size);
// What the decoder's inspect step asks: does this file go through the stage?  tiff_route's plain rule, and for
// Deflate files the measured one on top, as kPngDecoderMinRatio is for PNG: a wave inflates at the rate of the
// symbols it decodes (the compressed bytes), the pool's zlib at the rate of the decoded bytes, and 16 host threads
// beat the device where the strips hold more than about 1 byte for 2.4 decoded ones (host faster in
// every pair at 1.7 decoded bytes per compressed byte, device faster in every pair at 3.4 and 8.4).  The rule reads
// the header alone: the sum of StripByteCounts against rows x row bytes (of TileByteCounts against the decoded tiles).  LZW, PackBits and uncompressed files were
// faster on the device in every class measured and keep the plain rule.  False also for a file the parse refuses,
// which then takes the host decoder's path and gets its error there.
constexpr uint64_t kTiffDecoderDeflateMinRatio = 3;
bool               tiff_routed(const void* data, size_t size);
// Bytes of device scratch a routed file needs (0 for an uncompressed file).
size_t tiff_scratch_bytes(const TiffPlan& P);
// A routed file's job (everything but the three addresses and the stride), its strips and bands -- a tiled file's
// tiles, tiled bands and tile sources -- appended (strips' soff and bands' src relative to the file's scratch / the
// file), and the file copied to file_dst (size bytes; the caller pads).
void tiff_stage(const void* data, size_t size, int mode, const TiffPlan& P, int job, TiffJob& J, TiffTables& T, uint8_t* file_dst);
// The stage's kernels run on this thread, lane after lane (tiff_strips.hpp): 1 decoded, 0 the file is not routed
// to the device (nothing written), -1 the device would set kTiffCorruptBit.  large: the opt-in call's routing.
int tiff_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride, bool large = false);

} // namespace aeon_hip
