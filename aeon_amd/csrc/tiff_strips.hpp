// tiff_strips.hpp -- the TIFF stage's per-wave and per-band logic (tiff_kernels.hip), written once for the device
// and for the host: tiff_expand runs expand_strip on the 64 lanes of one wave, tiff_convert runs convert_band on
// the 256 lanes of a workgroup; tiff_host.cpp's tiff_gpu_emulate runs the same code with every lane loop walked
// serially (the PNG_* lane macros of png_inflate.hpp in the wave code, the PM_* ones of pixmap_rows.hpp in the
// band code), so the CPU tests and the sanitizer program cover what the kernels run.  The one piece written
// twice is the predictor's scan (scan_rows): shuffles across a wave on the device, a running sum on the host.
// Everything outside a lane loop is wave-uniform.  See DESIGN section 21.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pixmap.hpp" // pixmap_gray: the project's one colour -> gray formula
#include "pixmap_rows.hpp"
#include "png_inflate.hpp"
#include "tiff.hpp"

namespace aeon_hip {
namespace tiffdev {

// ---- tiff_expand: one compressed strip -----------------------------------------------------------------

// An LZW or PackBits strip's whole output (at most kTiffStripCap bytes) and the LZW string table: entry c is the
// range of the strip's own output that code c stands for, position | length << 16.
struct LzwMem {
    uint8_t  out[kTiffStripCap];
    uint32_t tab[kTiffLzwCodes];
};
// The wave's LDS (tiff_expand) or the emulation's heap block
union alignas(16) ExpandMem {
    pngdev::InflateMem inf;
    LzwMem             lzw;
};

// A strip's bytes as the wave reads them: aligned words from `w`, the strip's first byte `a` (0..3) bytes in,
// `n` bytes long.  A word wholly past the strip reads as zero; the callers check every byte and bit they use
// against n first.
struct In {
    const PNG_GLOBAL uint32_t* w;
    uint32_t                   a, n;
};
PNG_FN uint32_t in_word(const In& I, uint32_t byte) { return byte < I.a + I.n ? PNG_UNI(I.w[byte >> 2]) : 0u; }
PNG_FN uint32_t in_byte(const In& I, uint32_t i) { return (in_word(I, (I.a + i) & ~3u) >> (8 * ((I.a + i) & 3))) & 0xff; }

// The finished strip leaves the LDS for its scratch: 16 bytes per lane and store (the scratch has room for
// `need` rounded up to 16, and so has `out`).
PNG_FN void store_strip(const uint8_t* out, PNG_GLOBAL uint8_t* raw, uint32_t need)
{
    PNG_SYNC();
    const uint32_t n16 = (need + 15) >> 4;
    for (uint32_t c = PNG_LANE0; c < n16; c += PNG_LANE_STEP) {
        const uint32_t* w = (const uint32_t*)(out + 16 * c);
        *(PNG_GLOBAL pngdev::u32x4*)(raw + 16 * (size_t)c) = pngdev::u32x4{w[0], w[1], w[2], w[3]};
    }
}

// TIFF's LZW: codes MSB first, 9 to 12 bits wide, the width growing one entry early.  Every table entry's string
// is a range of the output so far -- (where the previous code's string began, its length + 1) -- so a code is
// emitted as inflate's match copy, by all lanes; the code about to be defined (KwKwK) is that range overlapping
// its own output by one byte, copied as a match of that distance is.  False: a code above the next free entry,
// a first code after a clear that is no literal, or the strip ends (its bytes, or EOI) before `need` bytes are out.
PNG_FN bool lzw_strip(LzwMem& M, const In& I, uint32_t need)
{
    uint64_t       hold = __builtin_bswap32(in_word(I, 0));
    uint32_t       nb = 32 - 8 * I.a, ip = 4;
    const uint64_t total = (uint64_t)8 * I.n;
    uint64_t       used = 0;
    uint32_t       width = 9, next = 258, p = 0, prev_pos = 0, prev_len = 0; // prev_len 0: just cleared
    while (p < need) {
        if (used + width > total) return false;
        if (nb < width) {
            hold = hold << 32 | __builtin_bswap32(in_word(I, ip));
            nb += 32, ip += 4;
        }
        const uint32_t code = (uint32_t)(hold >> (nb - width)) & ((1u << width) - 1);
        nb -= width, used += width;
        if (code == 256) {
            width = 9, next = 258, prev_len = 0;
            continue;
        }
        if (code == 257) break;
        if (prev_len == 0 && code > 255) return false;
        uint32_t src = p, len = 1;
        if (code < 256) {
            for (int l = PNG_LANE0; l < 1; l += PNG_LANE_STEP) M.out[p] = (uint8_t)code;
        } else {
            if (code < next) {
                const uint32_t e = PNG_UNI(M.tab[code]);
                src = e & 0xffff, len = e >> 16;
            } else if (code == next) {
                src = prev_pos, len = prev_len + 1;
            } else {
                return false;
            }
            const uint32_t n = len < need - p ? len : need - p, dist = p - src; // (len <= dist + 1)
            PNG_SYNC();
            for (uint32_t i = PNG_LANE0; i < n; i += PNG_LANE_STEP) M.out[p + i] = M.out[src + (i < dist ? i : i - dist)];
            len = n;
        }
        if (prev_len && next < (uint32_t)kTiffLzwCodes) {
            M.tab[next++] = prev_pos | (prev_len + 1) << 16; // (every lane the same value)
            if (next + 1 >= (1u << width) && width < 12) width++;
        }
        prev_pos = p, prev_len = len, p += len;
    }
    return p == need;
}

// PackBits: the control bytes walked wave-uniformly, a literal run copied and a repeat run filled by the lanes.
// False: a run past the strip's bytes or past `need`, or the bytes end before `need` bytes are out.
PNG_FN bool packbits_strip(LzwMem& M, const In& I, uint32_t need)
{
    const PNG_GLOBAL uint8_t* bytes = (const PNG_GLOBAL uint8_t*)I.w + I.a;
    uint32_t                  i = 0, p = 0;
    while (p < need) {
        if (i >= I.n) return false;
        const uint32_t c = in_byte(I, i++);
        if (c == 128) continue;
        if (c < 128) {
            const uint32_t cnt = c + 1;
            if (cnt > I.n - i || cnt > need - p) return false;
            for (uint32_t k = PNG_LANE0; k < cnt; k += PNG_LANE_STEP) M.out[p + k] = bytes[i + k];
            i += cnt, p += cnt;
        } else {
            const uint32_t cnt = 257 - c;
            if (i >= I.n || cnt > need - p) return false;
            const uint32_t v = in_byte(I, i++);
            for (uint32_t k = PNG_LANE0; k < cnt; k += PNG_LANE_STEP) M.out[p + k] = (uint8_t)v;
            p += cnt;
        }
    }
    return true;
}

// One strip of the call's strip table into its place in its file's scratch.  False: the strip is refused
// (kTiffCorruptBit).  Nothing is read outside the file and its padding, nothing written outside the strip's scratch.
PNG_FN bool expand_strip(const TiffJob& J, const TiffStrip& T, ExpandMem& M)
{
    const uint64_t at  = J.src + T.off;
    PNG_GLOBAL uint8_t* raw = (PNG_GLOBAL uint8_t*)(J.raw + T.soff);
    In I;
    I.w = (const PNG_GLOBAL uint32_t*)(at & ~(uint64_t)3), I.a = (uint32_t)(at & 3), I.n = T.bytes;
    if (T.comp == kTfDeflate) {
        pngdev::Inflate S;
        S.in = I.w, S.raw = raw, S.clen = I.a + I.n, S.need = T.need;
        return pngdev::inflate_file<true>(M.inf, S, I.a);
    }
    if (T.need > (uint32_t)kTiffStripCap) return false; // (the routing rule keeps such a strip on the host)
    const bool ok = T.comp == kTfLzw ? lzw_strip(M.lzw, I, T.need) : packbits_strip(M.lzw, I, T.need);
    if (ok) store_strip(M.lzw.out, raw, T.need);
    return ok;
}

// ---- tiff_convert: one band of rows ----------------------------------------------------------------------

// Predictor 2 undone in the staged rows: every sample the sum of its row's samples of its channel up to it,
// mod 2^bps.  `row0` is the first row's first staged pixel, np pixels of each of `rows` rows `pitch` bytes apart;
// carry: the sums at the piece's left edge (a wide row's pieces pass them on; rows > 1: zero).
#if defined(__HIP_DEVICE_COMPILE__)
// A wave per row, its lanes on 64 consecutive pixels: an inclusive scan across the lanes per channel, the row's
// running sums carried from chunk to chunk in registers.
__device__ __forceinline__ void scan_rows(uint8_t* row0, int rows, int pitch, int np, int spp, int bs, uint32_t (&carry)[4])
{
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    for (int r = wave; r < rows; r += kTiffLanes / 64) {
        uint32_t sum[4] = {carry[0], carry[1], carry[2], carry[3]};
        if (rows > 1) sum[0] = sum[1] = sum[2] = sum[3] = 0;
        uint8_t* row = row0 + (size_t)r * pitch;
        for (int x0 = 0; x0 < np; x0 += 64) {
            const int  px = x0 + lane;
            const bool in = px < np;
            uint8_t*   s  = row + (size_t)px * spp * bs;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (c >= spp) continue;
                uint32_t v = 0;
                if (in) v = bs == 2 ? (uint32_t)s[2 * c] | (uint32_t)s[2 * c + 1] << 8 : s[c];
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(v, d, 64);
                    if (lane >= d) v += up;
                }
                v += sum[c];
                if (in) {
                    s[bs * c] = (uint8_t)v;
                    if (bs == 2) s[2 * c + 1] = (uint8_t)(v >> 8);
                }
                sum[c] = __shfl(v, 63, 64); // (lanes past the row hold zeros: lane 63 has the chunk's total)
            }
        }
        if (rows == 1) carry[0] = sum[0], carry[1] = sum[1], carry[2] = sum[2], carry[3] = sum[3];
    }
}
#else
inline void scan_rows(uint8_t* row0, int rows, int pitch, int np, int spp, int bs, uint32_t (&carry)[4])
{
    for (int r = 0; r < rows; r++) {
        uint32_t sum[4] = {carry[0], carry[1], carry[2], carry[3]};
        if (rows > 1) sum[0] = sum[1] = sum[2] = sum[3] = 0;
        uint8_t* row = row0 + (size_t)r * pitch;
        for (int px = 0; px < np; px++)
            for (int c = 0; c < spp; c++) {
                uint8_t* s = row + ((size_t)px * spp + c) * bs;
                sum[c] += bs == 2 ? (uint32_t)s[0] | (uint32_t)s[1] << 8 : s[0];
                s[0] = (uint8_t)sum[c];
                if (bs == 2) s[1] = (uint8_t)(sum[c] >> 8);
            }
        if (rows == 1) carry[0] = sum[0], carry[1] = sum[1], carry[2] = sum[2], carry[3] = sum[3];
    }
}
#endif

// What out_byte needs of a job, in registers
struct RowForm {
    int  photo, bs, bpp; // bytes per sample, per pixel
    bool bgr, out16;
};

// Byte k of an output row from the staged row of native samples; `row` points at pixel p0 of the row.
PM_FN uint32_t out_byte(const RowForm& F, const uint32_t* tab, const uint8_t* row, uint32_t p0, uint32_t k)
{
    const uint32_t px = F.bgr ? k / 3 : F.out16 ? k >> 1 : k;
    const uint32_t ch = F.bgr ? k - 3 * px : 0;
    const uint8_t* s  = row + (size_t)(px - p0) * F.bpp;
    const int      hi = F.bs - 1; // a 16-bit sample (native: low byte first) is reduced to its high byte
    if (F.photo == 3) {
        const uint32_t e = tab[s[0]];
        return F.bgr ? (e >> (8 * ch)) & 0xff : e >> 24;
    }
    if (F.photo <= 1) {
        if (F.out16) {
            uint32_t v = (uint32_t)s[0] | (uint32_t)s[1] << 8;
            if (F.photo == 0) v = 65535 - v;
            return (v >> (8 * (k & 1))) & 0xff;
        }
        const uint32_t v = s[hi];
        return F.photo == 0 ? 255 - v : v;
    }
    if (F.bgr) return s[(2 - ch) * F.bs + hi];
    return pixmap_gray(s[2 * F.bs + hi], s[F.bs + hi], s[hi]);
}

// Pixels [p0, p0 + np) of the band's rows: their source bytes -- contiguous from row to row -- into `lds` as
// aligned words at their own offset mod 4, 16-bit samples made native, the predictor undone, then every lane
// four consecutive output bytes of a row per step, stored as one dword where the destination is aligned and
// bytewise at a row's unaligned head and tail.
PM_FN void convert_piece(const TiffJob& J, const TiffBand& B, uint32_t p0, uint32_t np, const uint32_t* tab, uint8_t* lds,
                         uint32_t (&carry)[4])
{
    const int      rows = B.rows, bs = J.bps >> 3, spp = J.spp, bpp = bs * spp, pitch = J.rowb;
    const uint64_t base = J.comp == kTfNone ? J.src : J.raw;
    const int64_t  g0 = B.src + (int64_t)p0 * bpp, g1 = g0 + (int64_t)(rows - 1) * pitch + (int64_t)np * bpp;
    const uint32_t sh = (uint32_t)(g0 & 3);
    PM_SYNC();
    {
        const PM_GLOBAL uint32_t* gw = (const PM_GLOBAL uint32_t*)(base + (uint64_t)(g0 - sh));
        uint32_t*                 lw = (uint32_t*)lds;
        const int                 nw = (int)((g1 - (g0 - sh) + 3) >> 2);
        for (int i = PM_LANE0; i < nw; i += PM_LANE_STEP) lw[i] = gw[i];
    }
    PM_SYNC();
    uint8_t* row0 = lds + sh;
    if (bs == 2 && J.big) {
        const uint32_t ns = np * (uint32_t)spp, all = (uint32_t)rows * ns;
        for (uint32_t i = (uint32_t)PM_LANE0; i < all; i += PM_LANE_STEP) {
            const uint32_t r = i / ns;
            uint8_t*       s = row0 + (size_t)r * pitch + 2 * (size_t)(i - r * ns);
            const uint8_t  t = s[0];
            s[0] = s[1], s[1] = t;
        }
        PM_SYNC();
    }
    if (J.pred == 2) {
        scan_rows(row0, rows, pitch, (int)np, spp, bs, carry);
        PM_SYNC();
    }
    RowForm F;
    F.photo = J.photo, F.bs = bs, F.bpp = bpp, F.bgr = J.mode == AEON_DECODE_BGR8, F.out16 = J.elem_bytes == 2;
    const uint32_t opp = F.bgr ? 3 : F.out16 ? 2 : 1;
    const uint32_t k0 = p0 * opp, n = np * opp;
    const uint32_t G = n / 4 + 2; // groups of a row: the head, the aligned dwords, the tail
    const uint64_t total = (uint64_t)rows * G;
    for (uint64_t item = (uint64_t)PM_LANE0; item < total; item += PM_LANE_STEP) {
        const uint32_t r = (uint32_t)(item / G), g = (uint32_t)(item - (uint64_t)r * G);
        const uint64_t da = J.out + (uint64_t)(B.y0 + (int64_t)r) * (uint64_t)J.stride + k0;
        const uint32_t head = (uint32_t)(-da) & 3;
        const uint32_t start = g ? head + 4 * (g - 1) : 0;
        uint32_t       end   = g ? start + 4 : head;
        if (end > n) end = n;
        if (start >= end) continue;
        const uint8_t* row = row0 + (size_t)r * pitch;
        uint32_t       v   = 0;
        for (uint32_t j = start; j < end; j++) v |= out_byte(F, tab, row, p0, k0 + j) << (8 * (j - start));
        PM_GLOBAL uint8_t* d = (PM_GLOBAL uint8_t*)(da + start);
        if (end - start == 4 && g) *(PM_GLOBAL uint32_t*)d = v;
        else
            for (uint32_t j = 0; j < end - start; j++) d[j] = (uint8_t)(v >> (8 * j));
    }
}

// Pixels of a wide row's piece: what fits kTiffBandBytes, a multiple of 64 (the scan's chunk)
PM_FN uint32_t piece_pixels(int bpp) { return (uint32_t)(kTiffBandBytes / bpp) & ~63u; }

// One band.  tab: 256 words; lds: kTiffBandBytes + 8 bytes, 4-byte aligned.
PM_FN void convert_band(const TiffJob& J, const TiffBand& B, uint32_t* tab, uint8_t* lds)
{
    if (J.photo == 3)
        for (int i = PM_LANE0; i < 256; i += PM_LANE_STEP) tab[i] = J.table[i];
    uint32_t carry[4] = {0, 0, 0, 0};
    if (J.rowb <= kTiffBandBytes) {
        convert_piece(J, B, 0, (uint32_t)J.w, tab, lds, carry);
        return;
    }
    const uint32_t P = piece_pixels((J.bps >> 3) * J.spp);
    for (uint32_t p0 = 0; p0 < (uint32_t)J.w; p0 += P)
        convert_piece(J, B, p0, (uint32_t)J.w - p0 < P ? (uint32_t)J.w - p0 : P, tab, lds, carry);
}

} // namespace tiffdev
} // namespace aeon_hip
