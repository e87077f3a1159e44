// tiff_strips.hpp -- the TIFF stage's per-wave and per-band logic (tiff_kernels.hip), written once for the device
// and for the host: tiff_expand runs expand_strip on the 64 lanes of one wave, tiff_convert runs convert_band and
// tiff_convert_tiled convert_tiled_band on the 256 lanes of a workgroup; tiff_host.cpp's tiff_gpu_emulate runs the
// same code with every lane loop walked serially (the PNG_* lane macros of png_inflate.hpp in the wave code, the
// PM_* ones of pixmap_rows.hpp in the band code), so the CPU tests and the sanitizer program cover what the
// kernels run.  tiff_expand_large runs expand_strip_large on one wave the same way.  The pieces written twice are the
// predictor's scan (scan_rows, finish_segment) and the large strips' ballot and scan (wave_mask, wave_exscan):
// shuffles across a wave on the device, a loop over the lanes on the host.
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

// ---- tiff_expand_large: one LZW / PackBits strip of any size --------------------------------------------------
// The wave holds a window of the strip's output in LDS -- chunk: bytes [base, base + kTiffChunk), base a multiple of
// kTiffChunk -- and a full window leaves for the scratch (flush_chunk).  A string's source below `base` is read back
// from the scratch, one at or above it from the window (out_at).  LZW decodes up to 64 codes a step (lzw_large): a
// lane extracts a code, the lengths of codes that name entries defined inside the batch are resolved by pointer
// doubling, a scan of the lengths places every code, and the bytes are written in two passes.  The batch's per-lane
// state lives in 64-entry LDS arrays between PNG_SYNC()s, so the host emulation walks the same lane loops serially;
// the ballot and the scan (wave_mask, wave_exscan) are written twice.

struct alignas(16) LargeMem {
    uint8_t  chunk[kTiffChunk];
    uint32_t pos[kTiffLzwCodes]; // the LZW string table: entry c is `len` bytes of the strip's own output from `pos`
    uint16_t len[kTiffLzwCodes];
    uint32_t b_code[64], b_len[64], b_ptr[64], b_pos[64], b_flag[64]; // the batch, per lane
};

// The strip's output: the scratch, `need` bytes, and where the window stands
struct Out {
    PNG_GLOBAL uint8_t* raw;
    uint32_t            base, need;
};

#if defined(__HIP_DEVICE_COMPILE__)
// bit l: lane l's flag is set
__device__ __forceinline__ uint64_t wave_mask(const uint32_t* flag) { return __ballot(flag[threadIdx.x] != 0); }
// out[l] = in[0] + ... + in[l - 1]
__device__ __forceinline__ void wave_exscan(const uint32_t* in, uint32_t* out)
{
    const int      lane = (int)threadIdx.x;
    const uint32_t v = in[lane];
    uint32_t       s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(s, d, 64);
        if (lane >= d) s += up;
    }
    out[lane] = s - v;
}
#else
inline uint64_t wave_mask(const uint32_t* flag)
{
    uint64_t m = 0;
    for (int l = 0; l < 64; l++) m |= (uint64_t)(flag[l] != 0) << l;
    return m;
}
inline void wave_exscan(const uint32_t* in, uint32_t* out)
{
    uint32_t s = 0;
    for (int l = 0; l < 64; l++) out[l] = s, s += in[l];
}
#endif
PNG_FN uint32_t first_lane(uint64_t mask) { return mask ? (uint32_t)__builtin_ctzll(mask) : 64u; }

// The first `n` bytes of the window leave for the scratch, 16 bytes per lane and store as store_strip's (n < kTiffChunk
// only for the strip's last bytes: the scratch has room for `need` rounded up to 16), and the window moves on.  The
// barrier behind the stores is what lets the wave read its own flushed bytes back: DESIGN section 21.
PNG_FN void flush_chunk(LargeMem& M, Out& O, uint32_t n)
{
    PNG_SYNC();
    const uint32_t n16 = (n + 15) >> 4;
    for (uint32_t c = PNG_LANE0; c < n16; c += PNG_LANE_STEP) {
        const uint32_t* w = (const uint32_t*)(M.chunk + 16 * c);
        *(PNG_GLOBAL pngdev::u32x4*)(O.raw + O.base + 16 * (size_t)c) = pngdev::u32x4{w[0], w[1], w[2], w[3]};
    }
    O.base += (uint32_t)kTiffChunk;
    PNG_SYNC();
}

// Output byte q (below the position being written)
PNG_FN uint32_t out_at(const LargeMem& M, const Out& O, uint32_t q) { return q >= O.base ? M.chunk[q - O.base] : O.raw[q]; }

// n bytes at p from the string at src < p (n <= p - src + 1: a string may overlap its own output by one byte), by
// all lanes, as lzw_strip copies one: every source is below p.  A copy that reaches the window's end flushes it
// and goes on in the next.
PNG_FN void emit_copy(LargeMem& M, Out& O, uint32_t p, uint32_t src, uint32_t n)
{
    const uint32_t dist = p - src;
    for (uint32_t i0 = 0; i0 < n;) {
        const uint32_t room = O.base + (uint32_t)kTiffChunk - (p + i0), m = n - i0 < room ? n - i0 : room;
        PNG_SYNC();
        for (uint32_t i = i0 + PNG_LANE0; i < i0 + m; i += PNG_LANE_STEP)
            M.chunk[p + i - O.base] = (uint8_t)out_at(M, O, src + (i < dist ? i : i - dist));
        i0 += m;
        if (m == room) flush_chunk(M, O, (uint32_t)kTiffChunk);
    }
}

// A lane's own word of the strip (in_word is the wave-uniform one)
PNG_FN uint32_t in_word_lane(const In& I, uint32_t byte) { return byte < I.a + I.n ? I.w[byte >> 2] : 0u; }
// The w bits (9..12) from bit `bit` of the strip on, MSB first; the caller has checked bit + w against the strip.
PNG_FN uint32_t code_at(const In& I, uint64_t bit, uint32_t w)
{
    const uint32_t at = I.a + (uint32_t)(bit >> 3), word = at & ~3u, sh = 8 * (at & 3) + (uint32_t)(bit & 7);
    const uint64_t v = (uint64_t)__builtin_bswap32(in_word_lane(I, word)) << 32 | __builtin_bswap32(in_word_lane(I, word + 4));
    return (uint32_t)(v >> (64 - sh - w)) & ((1u << w) - 1);
}
// Between two ClearCodes a code's width follows from the table's next free entry when it is read (the width grows
// one entry early), so the bits of the k codes read from `next` free entries on are known in advance.
PNG_FN uint32_t lzw_width(uint32_t next) { return 9 + (next >= 511) + (next >= 1023) + (next >= 2047); }
PNG_FN uint32_t lzw_grown(uint32_t next, uint32_t k, uint32_t at)
{
    const uint32_t first = next >= at ? 0 : at - next; // the first of the k codes read at `at` entries or more
    return k > first ? k - first : 0;
}
PNG_FN uint32_t lzw_bits(uint32_t next, uint32_t k) { return 9 * k + lzw_grown(next, k, 511) + lzw_grown(next, k, 1023) + lzw_grown(next, k, 2047); }

constexpr uint32_t kNoLane = 64;

// TIFF's LZW as lzw_strip decodes it -- same strings, same refusals -- for a strip of any size.  After a ClearCode
// the first code, a literal, is read alone.  From then on a batch: lane j reads the j-th next code (batch code j
// is read with next + j free entries and defines entry next + j: where code j - 1 began, its length + 1; j = 0: the
// previous code's).  The batch ends ahead of the first ClearCode, EOI, code above its free entry or code past the
// strip's bytes (found by a ballot; met again as lane 0 of the next batch, it is acted on), where the table fills
// (a batch in a full table defines nothing, all its codes 12 bits), and ahead of the first code that does not fit
// the window or starts at `need`.  Lengths: 1 for a literal, the table's for a code below `next`; a code next + m
// names the entry batch code m defines, so its length is that of code m - 1 plus 1 -- a forest over earlier lanes,
// resolved in 6 rounds of pointer doubling.  An exclusive scan of the lengths gives the positions.  Bytes: first
// every byte of a literal or of a code below `next` (its source lies below the batch), lanes striding over the
// bytes, a byte's code found by bisection of the positions; then the codes that name the batch's own entries in
// lane order, each copied by all lanes.  A batch whose first code does not fit the window is that code alone,
// copied across the window's end.
PNG_FN bool lzw_large(LargeMem& M, const In& I, Out& O)
{
    const uint64_t total = (uint64_t)8 * I.n;
    const uint32_t need = O.need;
    uint64_t       bit = 0;
    uint32_t       next = 258, p = 0, prev_pos = 0, prev_len = 0;
    bool           fresh = true; // just cleared: the next code is a literal
    while (p < need) {
        if (fresh) {
            if (bit + 9 > total) return false;
            const uint32_t code = PNG_UNI(code_at(I, bit, 9));
            bit += 9;
            if (code == 256) continue;
            if (code == 257) break;
            if (code > 255) return false;
            PNG_SYNC();
            for (int l = PNG_LANE0; l < 1; l += PNG_LANE_STEP) M.chunk[p - O.base] = (uint8_t)code;
            prev_pos = p, prev_len = 1, p++, fresh = false;
            if (p == O.base + (uint32_t)kTiffChunk) flush_chunk(M, O, (uint32_t)kTiffChunk);
            continue;
        }
        const bool     full = next >= (uint32_t)kTiffLzwCodes;
        const uint32_t nb = full || (uint32_t)kTiffLzwCodes - next > 64 ? 64 : (uint32_t)kTiffLzwCodes - next;
        const uint32_t wend = O.base + (uint32_t)kTiffChunk;
        PNG_SYNC();
        // each lane its code: what it is, its length or the lane its length hangs on
        for (uint32_t j = PNG_LANE0; j < 64; j += PNG_LANE_STEP) {
            const uint32_t nj = full ? next : next + j, w = lzw_width(nj);
            const uint64_t at = bit + lzw_bits(next, j);
            uint32_t       code = 257, stop = 1, len = 0, ptr = kNoLane;
            if (j < nb && at + w <= total) {
                code = code_at(I, at, w);
                stop = code == 256 || code == 257 || code > nj; // (a full table: nj is 4096, above every code)
            }
            if (!stop) {
                if (code < 256) len = 1;
                else if (code < next) len = M.len[code];
                else if (code == next) len = prev_len + 1;
                else len = 1, ptr = code - next - 1;
            }
            M.b_code[j] = code, M.b_flag[j] = stop, M.b_len[j] = len, M.b_ptr[j] = ptr;
        }
        PNG_SYNC();
        const uint32_t c = first_lane(wave_mask(M.b_flag));
        if (c == 0) { // a ClearCode; anything else ends the strip short of its rows, or is corrupt
            if (PNG_UNI(M.b_code[0]) != 256) return false; // (a code past the strip's bytes was noted as EOI)
            bit += lzw_width(next), next = 258, fresh = true;
            continue;
        }
        // len[j] += len[ptr[j]], ptr[j] = ptr[ptr[j]]: a lane hangs on an earlier one, so 6 rounds reach every root
        for (int r = 0; r < 6; r++) {
            for (uint32_t j = PNG_LANE0; j < 64; j += PNG_LANE_STEP) {
                const uint32_t q = M.b_ptr[j], add = q < kNoLane ? M.b_len[q] : 0, up = q < kNoLane ? M.b_ptr[q] : kNoLane;
                PNG_SYNC();
                if (q < kNoLane) M.b_len[j] += add, M.b_ptr[j] = up;
            }
            PNG_SYNC();
        }
        wave_exscan(M.b_len, M.b_pos);
        PNG_SYNC();
        // the codes of this step: those that start below `need` and end (cut at `need`) inside the window
        for (uint32_t j = PNG_LANE0; j < 64; j += PNG_LANE_STEP) {
            const uint32_t at = p + M.b_pos[j], len = M.b_len[j];
            const uint32_t end = at < need ? (len < need - at ? at + len : need) : at;
            M.b_pos[j] = at, M.b_flag[j] = !(j < c && at < need && end <= wend);
        }
        PNG_SYNC();
        uint32_t   cn = first_lane(wave_mask(M.b_flag));
        const bool alone = cn == 0; // code 0 crosses the window's end (a literal never does)
        if (alone) cn = 1;
        const uint32_t last_pos = PNG_UNI(M.b_pos[cn - 1]), last_len = PNG_UNI(M.b_len[cn - 1]);
        const uint32_t pend = last_len < need - last_pos ? last_pos + last_len : need;
        PNG_SYNC();
        for (uint32_t j = PNG_LANE0; j < 64; j += PNG_LANE_STEP) {
            if (j < cn && !full) {
                M.pos[next + j] = j ? M.b_pos[j - 1] : prev_pos;
                M.len[next + j] = (uint16_t)((j ? M.b_len[j - 1] : prev_len) + 1);
            }
            M.b_flag[j] = j < cn && (alone || M.b_code[j] >= next);
        }
        if (!alone) {
            for (uint32_t q = p + PNG_LANE0; q < pend; q += PNG_LANE_STEP) {
                uint32_t j = 0;
                for (uint32_t step = 32; step; step >>= 1)
                    if (j + step < cn && M.b_pos[j + step] <= q) j += step;
                const uint32_t code = M.b_code[j];
                if (code < 256) M.chunk[q - O.base] = (uint8_t)code;
                else if (code < next) M.chunk[q - O.base] = (uint8_t)out_at(M, O, M.pos[code] + (q - M.b_pos[j]));
            }
        }
        PNG_SYNC();
        for (uint64_t todo = wave_mask(M.b_flag); todo; todo &= todo - 1) {
            const uint32_t j = (uint32_t)__builtin_ctzll(todo), code = PNG_UNI(M.b_code[j]);
            const uint32_t at = PNG_UNI(M.b_pos[j]), len = PNG_UNI(M.b_len[j]);
            const uint32_t src = code < next ? PNG_UNI(M.pos[code]) : code == next ? prev_pos : PNG_UNI(M.b_pos[code - next - 1]);
            emit_copy(M, O, at, src, len < need - at ? len : need - at);
        }
        bit += lzw_bits(next, cn);
        if (!full) next += cn;
        prev_pos = last_pos, prev_len = last_len, p = pend;
        if (p == O.base + (uint32_t)kTiffChunk) flush_chunk(M, O, (uint32_t)kTiffChunk);
    }
    if (p < need) return false;
    if (need > O.base) flush_chunk(M, O, need - O.base);
    return true;
}

// PackBits as packbits_strip walks it, the runs written through the window.
PNG_FN bool packbits_large(LargeMem& M, const In& I, Out& O)
{
    const PNG_GLOBAL uint8_t* bytes = (const PNG_GLOBAL uint8_t*)I.w + I.a;
    const uint32_t            need = O.need;
    uint32_t                  i = 0, p = 0;
    while (p < need) {
        if (i >= I.n) return false;
        const uint32_t c = in_byte(I, i++);
        if (c == 128) continue;
        const bool     lit = c < 128;
        const uint32_t cnt = lit ? c + 1 : 257 - c;
        if ((lit ? cnt > I.n - i : i >= I.n) || cnt > need - p) return false;
        const uint32_t v = lit ? 0 : in_byte(I, i);
        for (uint32_t k0 = 0; k0 < cnt;) {
            const uint32_t room = O.base + (uint32_t)kTiffChunk - (p + k0), m = cnt - k0 < room ? cnt - k0 : room;
            for (uint32_t k = k0 + PNG_LANE0; k < k0 + m; k += PNG_LANE_STEP) M.chunk[p + k - O.base] = lit ? bytes[i + k] : (uint8_t)v;
            k0 += m;
            if (m == room) flush_chunk(M, O, (uint32_t)kTiffChunk);
        }
        i += lit ? cnt : 1, p += cnt;
    }
    if (need > O.base) flush_chunk(M, O, need - O.base);
    return true;
}

// One strip of the call's table of large strips into its place in its file's scratch, as expand_strip does a small one.
PNG_FN bool expand_strip_large(const TiffJob& J, const TiffStrip& T, LargeMem& M)
{
    const uint64_t at = J.src + T.off;
    In             I;
    I.w = (const PNG_GLOBAL uint32_t*)(at & ~(uint64_t)3), I.a = (uint32_t)(at & 3), I.n = T.bytes;
    Out O;
    O.raw = (PNG_GLOBAL uint8_t*)(J.raw + T.soff), O.base = 0, O.need = T.need;
    if (T.comp == kTfLzw) return lzw_large(M, I, O);
    return T.comp == kTfPackBits && packbits_large(M, I, O);
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

// ---- tiff_convert_tiled: one band of a tiled file -----------------------------------------------------------
// A segment is one row of one tile: TileWidth pixels, a multiple of 16 bytes, so every segment of a tile lies at the
// tile's own offset mod 16 -- 0 in the scratch, anything for an uncompressed tile in the file.  A band is `rows`
// image rows times `nt` tiles across.  Its segments go into LDS side by side, segment (r, t) at (r * nt + t) * segment
// bytes with its first byte on a 16-byte boundary: the LDS then holds `rows` ordinary rows of nt * TileWidth pixels
// and the output pass needs no tile arithmetic at all.  The waves deal the segments out among themselves; the wave
// that staged a segment also finishes it (byte order, predictor), since the predictor restarts in every segment.

#if defined(__HIP_DEVICE_COMPILE__)
#define TT_WAVE ((int)threadIdx.x >> 6)
#define TT_WAVES (kTiffLanes / 64)
#define TT_LANE ((int)threadIdx.x & 63)
#define TT_LANES 64
#else
#define TT_WAVE 0
#define TT_WAVES 1
#define TT_LANE 0
#define TT_LANES 1
#endif

// Bytes sh.. of the 8 that lo and hi hold (sh 1..3)
PM_FN uint32_t bytes_from(uint32_t lo, uint32_t hi, uint32_t sh) { return lo >> (8 * sh) | hi << (32 - 8 * sh); }

// One segment from global memory into LDS: 16 bytes per lane and step where the source is 16-byte aligned, else
// dwords put together from the two aligned words that hold them (the last lane reads at most 4 bytes past the
// segment: inside the 16 bytes of padding behind every file and scratch).
PM_FN void stage_segment(uint64_t g, uint8_t* seg, uint32_t segb)
{
    if ((g & 15) == 0) {
        const PM_GLOBAL pngdev::u32x4* gq = (const PM_GLOBAL pngdev::u32x4*)g;
        pngdev::u32x4*                 lq = (pngdev::u32x4*)seg;
        for (uint32_t i = TT_LANE; i < segb / 16; i += TT_LANES) lq[i] = gq[i];
        return;
    }
    const uint32_t            sh = (uint32_t)(g & 3);
    const PM_GLOBAL uint32_t* gw = (const PM_GLOBAL uint32_t*)(g - sh);
    uint32_t*                 lw = (uint32_t*)seg;
    for (uint32_t i = TT_LANE; i < segb / 4; i += TT_LANES) lw[i] = sh ? bytes_from(gw[i], gw[i + 1], sh) : gw[i];
}

// A staged segment's samples made native and its predictor undone, in place: every sample the sum of the
// segment's samples of its channel up to it, from zero at the tile's left edge.
#if defined(__HIP_DEVICE_COMPILE__)
// The wave's lanes on 64 consecutive pixels: an inclusive scan across the lanes per channel, the running sums
// carried from chunk to chunk in registers.
__device__ __forceinline__ void finish_segment(uint8_t* seg, int tw, int spp, int bs, bool swap, bool pred)
{
    const int lane = TT_LANE;
    uint32_t  sum[4] = {0, 0, 0, 0};
    for (int x0 = 0; x0 < tw; x0 += 64) {
        const int  px = x0 + lane;
        const bool in = px < tw;
        uint8_t*   s  = seg + (size_t)px * spp * bs;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (c >= spp) continue;
            uint32_t v = 0;
            if (in) v = bs == 2 ? (uint32_t)s[2 * c + (swap ? 1 : 0)] | (uint32_t)s[2 * c + (swap ? 0 : 1)] << 8 : s[c];
            if (pred) {
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(v, d, 64);
                    if (lane >= d) v += up;
                }
                v += sum[c];
                sum[c] = __shfl(v, 63, 64); // (lanes past the segment hold zeros: lane 63 has the chunk's total)
            }
            if (in) {
                s[bs * c] = (uint8_t)v;
                if (bs == 2) s[2 * c + 1] = (uint8_t)(v >> 8);
            }
        }
    }
}
#else
inline void finish_segment(uint8_t* seg, int tw, int spp, int bs, bool swap, bool pred)
{
    uint32_t sum[4] = {0, 0, 0, 0};
    for (int px = 0; px < tw; px++)
        for (int c = 0; c < spp; c++) {
            uint8_t* s = seg + ((size_t)px * spp + c) * bs;
            uint32_t v = bs == 2 ? (uint32_t)s[swap ? 1 : 0] | (uint32_t)s[swap ? 0 : 1] << 8 : s[0];
            if (pred) v = sum[c] += v;
            s[0] = (uint8_t)v;
            if (bs == 2) s[1] = (uint8_t)(v >> 8);
        }
}
#endif

// One tiled band.  tile_src: the call's table of tile sources; tab: 256 words; lds: kTiffBandBytes bytes, 16-byte aligned.
PM_FN void convert_tiled_band(const TiffJob& J, const TiffTileBand& B, const uint32_t* tile_src, uint32_t* tab, uint8_t* lds)
{
    if (J.photo == 3)
        for (int i = PM_LANE0; i < 256; i += PM_LANE_STEP) tab[i] = J.table[i];
    const int      bs = J.bps >> 3, spp = J.spp, bpp = bs * spp, nt = B.nt, rows = B.rows;
    const uint32_t segb = (uint32_t)J.tw * bpp, nseg = (uint32_t)rows * nt, pitch = (uint32_t)nt * segb;
    const uint64_t base = J.comp == kTfNone ? J.src : J.raw;
    const bool     swap = bs == 2 && J.big, pred = J.pred == 2;
    const PM_GLOBAL uint32_t* from = (const PM_GLOBAL uint32_t*)tile_src + J.tile0 + B.tile;
    for (uint32_t s = TT_WAVE; s < nseg; s += TT_WAVES) {
        const uint32_t r = s / nt, t = s - r * nt;
        stage_segment(base + from[t] + (uint64_t)(B.r0 + r) * segb, lds + (size_t)s * segb, segb);
    }
    if (swap || pred) {
        PM_SYNC();
        for (uint32_t s = TT_WAVE; s < nseg; s += TT_WAVES) finish_segment(lds + (size_t)s * segb, J.tw, spp, bs, swap, pred);
    }
    PM_SYNC();
    // the rows of the band, clipped at the image's right edge (the band table clips at the bottom one): every lane
    // four consecutive output bytes of a row per step, as convert_piece writes them
    RowForm F;
    F.photo = J.photo, F.bs = bs, F.bpp = bpp, F.bgr = J.mode == AEON_DECODE_BGR8, F.out16 = J.elem_bytes == 2;
    const uint32_t opp = F.bgr ? 3 : F.out16 ? 2 : 1, p0 = (uint32_t)B.px0;
    const uint32_t p1 = p0 + (uint32_t)nt * J.tw < (uint32_t)J.w ? p0 + (uint32_t)nt * J.tw : (uint32_t)J.w;
    const uint32_t k0 = p0 * opp, n = (p1 - p0) * opp;
    const uint32_t G = n / 4 + 2, total = (uint32_t)rows * G; // groups of a row: the head, the aligned dwords, the tail
    for (uint32_t item = (uint32_t)PM_LANE0; item < total; item += PM_LANE_STEP) {
        const uint32_t r = item / G, g = item - r * G;
        const uint64_t da = J.out + (uint64_t)(B.y0 + (int64_t)r) * (uint64_t)J.stride + k0;
        const uint32_t head = (uint32_t)(-da) & 3;
        const uint32_t start = g ? head + 4 * (g - 1) : 0;
        uint32_t       end   = g ? start + 4 : head;
        if (end > n) end = n;
        if (start >= end) continue;
        const uint8_t* row = lds + (size_t)r * pitch;
        uint32_t       v   = 0;
        for (uint32_t j = start; j < end; j++) v |= out_byte(F, tab, row, p0, k0 + j) << (8 * (j - start));
        PM_GLOBAL uint8_t* d = (PM_GLOBAL uint8_t*)(da + start);
        if (end - start == 4 && g) *(PM_GLOBAL uint32_t*)d = v;
        else
            for (uint32_t j = 0; j < end - start; j++) d[j] = (uint8_t)(v >> (8 * j));
    }
}

} // namespace tiffdev
} // namespace aeon_hip
