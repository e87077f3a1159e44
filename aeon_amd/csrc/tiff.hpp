// tiff.hpp -- the TIFF decoder (classic TIFF in strips, what cv::imdecode reads beside JPEG, PNG, BMP and PNM): its
// host functions (tiff_host.cpp) behind aeon_tiff_info / aeon_decode_tiff and the decoder's providers, and the
// descriptors the host half of the TIFF stage shares with its kernels (tiff_kernels.hip, tiff_strips.hpp).
// The host functions throw jpeg_error (error.hpp) on a file they refuse; messages start with "TIFF:".
//
// The stage (aeon_hip_decode_tiff_batch): the host parses each file's first IFD, refuses what can be refused from
// the header and the first bytes of each strip, builds the file's 256-entry table (palette and gray of each
// entry), the call's strip table and band table, and copies the file as it is into pinned staging; tiff_expand
// (one wave per compressed strip) decodes LZW, PackBits and Deflate strips into the file's scratch, tiff_convert
// (one workgroup per band of rows) makes the samples native, undoes the horizontal predictor and converts the
// rows into the record.  Files with LZW / PackBits strips above 32 KiB stay with tiff_decode on the host
// (tiff_route).  The decode rules are DESIGN section 21.
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
    uint32_t table[256]; // entry i: B | G << 8 | R << 16 | gray << 24 of palette index i
};
static_assert(sizeof(TiffJob) % 16 == 0, "TiffJob: 16-byte aligned array elements");

// One compressed strip: tiff_expand's unit of work.
struct alignas(16) TiffStrip {
    int32_t  job, comp;
    uint32_t off, bytes; // the strip's bytes in the file
    int32_t  y0, rows;
    uint32_t need, pad_; // decoded bytes: rows * rowb
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

// What the host half learns from a file's IFD.
struct TiffPlan {
    int      w = 0, h = 0, spp = 1, bps = 1, photo = -1, pred = 1, big = 0, comp = kTfNone;
    int      channels = 1, elem_bytes = 1; // of the record in the requested mode
    int      file_channels = 1;            // 3: RGB or palette, 1: gray
    uint32_t rps = 0;                      // rows per strip, at most h
    int      route = 0;                    // 1: the device decodes the file (tiff_route)
    size_t   rowb = 0;
    std::vector<uint32_t> offs, counts;    // per strip (ceil(h / rps) of them)
    uint32_t table[256] = {};
};

// true when the first bytes are a classic TIFF's as the decoder's inspect step sniffs them (strict: II 2A 00 /
// MM 00 2A and an IFD offset inside the file; anything else is left to the JPEG parser and its error)
bool tiff_sniff(const void* data, size_t size);
// The IFD parse (refusals and messages of tiff_decode), the table and the routing rule.
void tiff_plan(const void* data, size_t size, int mode, TiffPlan& P);
// the whole decode on the calling thread into rows `stride` bytes apart; out_elem_bytes (optional): 1 or 2
void tiff_decode(const void* data, size_t size, int mode, void* dst, size_t stride, int* out_elem_bytes);
// The routing rule: a file below 2^31 bytes (decoded too) whose LZW / PackBits strips decode to at most
// kTiffStripCap bytes each goes to the device.  (Rows of any width fit tiff_convert: it walks a wide row in pieces.)
bool tiff_route(const TiffPlan& P, size_t size);
// What the decoder's inspect step asks: does this file go through the stage?  tiff_route's plain rule, and for
// Deflate files the measured one on top, as kPngDecoderMinRatio is for PNG: a wave inflates at the rate of the
// symbols it decodes (the compressed bytes), the pool's zlib at the rate of the decoded bytes, and 16 host threads
// beat the device where the strips hold more than about 1 byte for 2.4 decoded ones (host faster in
// every pair at 1.7 decoded bytes per compressed byte, device faster in every pair at 3.4 and 8.4).  The rule reads
// the header alone: the sum of StripByteCounts against rows x row bytes.  LZW, PackBits and uncompressed files were
// faster on the device in every class measured and keep the plain rule.  False also for a file the parse refuses,
// which then takes the host decoder's path and gets its error there.
constexpr uint64_t kTiffDecoderDeflateMinRatio = 3;
bool               tiff_routed(const void* data, size_t size);
// Bytes of device scratch a routed file needs (0 for an uncompressed file).
size_t tiff_scratch_bytes(const TiffPlan& P);
// A routed file's job (everything but the three addresses and the stride), its strips and bands appended (strips'
// soff and bands' src relative to the file's scratch / the file), and the file copied to file_dst (size bytes;
// the caller pads).
void tiff_stage(const void* data, size_t size, int mode, const TiffPlan& P, int job, TiffJob& J, std::vector<TiffStrip>& strips,
                std::vector<TiffBand>& bands, uint8_t* file_dst);
// The stage's kernels run on this thread, lane after lane (tiff_strips.hpp): 1 decoded, 0 the file is not routed
// to the device (nothing written), -1 the device would set kTiffCorruptBit.
int tiff_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride);

} // namespace aeon_hip
