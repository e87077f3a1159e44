// pixmap_rle.hpp -- bmp_rle_expand's per-wave logic (pixmap_kernels.hip), written once for the device and for the
// host: the kernel runs rle_expand on the 64 lanes of one wave, pixmap_host.cpp's pixmap_gpu_emulate runs the same
// code with every lane loop walked serially (the PNG_* lane macros of png_inflate.hpp; the ballot and the scan are
// tiff_strips.hpp's wave_mask / wave_exscan).  Everything outside a lane loop is wave-uniform.  DESIGN section 20.
//
// A BMP RLE stream is a sequence of 16-bit words and its position only moves forward, so the wave takes it 64
// words at a time, one word per lane: every lane reads its word as if a token started there, pointer doubling from
// the window's known first start marks the true starts, scans of the tokens' advances give each its (x, y), and
// all lanes then write the window's pixels, striding over pixel ordinals.  The stream is staged in LDS in blocks
// of kRleBlockWords words plus the kRleAheadWords a token starting in a block's last window can span (a literal is
// at most 129 words), so a token's payload is always read in the window the token starts in.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pixmap.hpp"
#include "png_inflate.hpp"
#include "tiff_strips.hpp"

namespace aeon_hip {
namespace pmdev {

using tiffdev::first_lane;
using tiffdev::wave_exscan;
using tiffdev::wave_mask;

enum RleToken : uint32_t { kRleRun = 0, kRleLiteral, kRleEol, kRleDelta, kRleEnd, kRleBad };

// The wave's LDS (bmp_rle_expand) or the emulation's heap block: the staged stream and the window's per-lane state
struct alignas(16) RleMem {
    uint8_t  stream[2 * (kRleBlockWords + kRleAheadWords) + 8];
    uint32_t kind[64], val[64], span[64], nxt[64], mark[64], flag[64];
    uint32_t dx[64], dy[64], npx[64]; // a token's advances: columns, rows, pixels written
    uint32_t sx[64], sy[64], pos[64]; // their exclusive scans
    uint32_t x[64], y[64], end[64];   // where a token's pixels start; pos + npx
};

PNG_FN uint32_t last_lane(uint64_t mask) { return mask ? 63u - (uint32_t)__builtin_clzll(mask) : 64u; }

// Pixel k of the token at lane j (a run or a literal); `pay` is the staged byte behind the token's own word.
PNG_FN uint32_t rle_pixel(const RleMem& M, int depth, uint32_t j, const uint8_t* pay, uint32_t k)
{
    const bool lit = M.kind[j] == kRleLiteral;
    if (depth == 8) return lit ? pay[k] : M.val[j];
    const uint32_t b = lit ? pay[k >> 1] : M.val[j];
    return (k & 1) ? b & 15 : b >> 4; // a run starts with its high nibble wherever it lies
}

// One file's stream into its index scratch.  False: the stream is refused (kPixmapCorruptBit) -- a run or literal
// past the row's end or at y >= h, or a token whose bytes pass the end of the data; nothing is written outside the
// scratch.  Data that ends between two tokens ends the stream as (0,1) does.
PNG_FN bool rle_expand(const PixmapRleJob& J, RleMem& M)
{
    const uint32_t nwords = J.bytes >> 1, sh = J.off & 3, W = (uint32_t)J.w, H = (uint32_t)J.h;
    const int      depth = J.depth;
    uint32_t       xc = 0, yc = 0; // the position in front of the window: saturated at (W, H), past which
    uint32_t       first = 0;      // nothing may be written; the window's lane of the first token start
    for (uint32_t base = 0;; base += 64) {
        const uint32_t bb = base / (uint32_t)kRleBlockWords * (uint32_t)kRleBlockWords;
        if (base == bb) { // the next block: aligned dwords, the stream's own offset mod 4 kept (J.src is 16-byte
            PNG_SYNC();   // aligned and 2 * bb a multiple of 4; the file has 16 zero bytes behind it)
            const PNG_GLOBAL uint32_t* gw = (const PNG_GLOBAL uint32_t*)(J.src + (uint64_t)(J.off - sh) + 2 * (uint64_t)bb);
            const uint32_t cap = 2u * (uint32_t)(kRleBlockWords + kRleAheadWords), have = J.bytes - 2 * bb;
            const int      nw = (int)((sh + (have < cap ? have : cap) + 3) >> 2);
            uint32_t*      lw = (uint32_t*)M.stream;
            for (int i = PNG_LANE0; i < nw; i += PNG_LANE_STEP) lw[i] = gw[i];
            PNG_SYNC();
        }
        if (first >= 64) { // the window lies inside a literal's payload
            first -= 64;
            continue;
        }
        const uint8_t* win = M.stream + sh + 2 * (size_t)(base - bb); // the window's first byte
        PNG_SYNC();
        // each lane its word, read as a token's first
        for (uint32_t l = PNG_LANE0; l < 64; l += PNG_LANE_STEP) {
            const uint32_t i = base + l;
            uint32_t       kind = kRleEnd, span = 1, dx = 0, dy = 0, npx = 0, val = 0;
            if (i < nwords) {
                const uint32_t a = win[2 * l], b = win[2 * l + 1];
                val = b;
                if (a) kind = kRleRun, npx = dx = a;
                else if (b == 0) kind = kRleEol, dy = 1;
                else if (b == 1) kind = kRleEnd;
                else if (b == 2) {
                    kind = kRleDelta, span = 2;
                    if (i + 1 < nwords) dx = win[2 * l + 2], dy = win[2 * l + 3];
                } else {
                    kind = kRleLiteral, npx = dx = b;
                    span = 1 + (depth == 8 ? (b + 1) >> 1 : (b + 3) >> 2); // the payload padded to a word
                }
                if (span > nwords - i) kind = kRleBad;
            } else if (2 * (uint64_t)i < J.bytes) {
                kind = kRleBad; // half a word left
            }
            M.kind[l] = kind, M.val[l] = val, M.span[l] = span, M.dx[l] = dx, M.dy[l] = dy, M.npx[l] = npx;
            M.nxt[l] = l + span < 64 ? l + span : 64, M.mark[l] = l == first;
        }
        PNG_SYNC();
        // the true starts: a marked lane marks its successor, every lane's successor doubles; 6 rounds reach 64
        for (int r = 0; r < 6; r++) {
            for (uint32_t l = PNG_LANE0; l < 64; l += PNG_LANE_STEP) {
                const uint32_t n = M.nxt[l], m = M.mark[l], nn = n < 64 ? M.nxt[n] : 64;
                PNG_SYNC();
                if (m && n < 64) M.mark[n] = 1;
                M.nxt[l] = nn;
            }
            PNG_SYNC();
        }
        const uint64_t starts = wave_mask(M.mark);
        for (uint32_t l = PNG_LANE0; l < 64; l += PNG_LANE_STEP) M.flag[l] = M.mark[l] && M.kind[l] >= kRleEnd;
        PNG_SYNC();
        const uint32_t c = first_lane(wave_mask(M.flag)); // the stream ends at lane c (64: not in this window)
        PNG_SYNC();
        for (uint32_t l = PNG_LANE0; l < 64; l += PNG_LANE_STEP) {
            const bool live = M.mark[l] && l < c;
            if (!live) M.dx[l] = 0, M.dy[l] = 0, M.npx[l] = 0;
            M.flag[l] = live && M.kind[l] == kRleEol;
        }
        PNG_SYNC();
        const uint64_t eol = wave_mask(M.flag);
        wave_exscan(M.dx, M.sx);
        wave_exscan(M.dy, M.sy);
        wave_exscan(M.npx, M.pos);
        PNG_SYNC();
        // x restarts at every EOL: the columns advanced since the last one below the lane
        for (uint32_t l = PNG_LANE0; l < 64; l += PNG_LANE_STEP) {
            const uint32_t e = last_lane(eol & (((uint64_t)1 << l) - 1));
            const uint32_t x = e < 64 ? M.sx[l] - M.sx[e] : xc + M.sx[l], y = yc + M.sy[l], n = M.npx[l];
            M.x[l] = x, M.y[l] = y, M.end[l] = M.pos[l] + n;
            M.flag[l] = n && (x + n > W || y >= H);
        }
        PNG_SYNC();
        if (wave_mask(M.flag)) return false;
        if (c < 64 && PNG_UNI(M.kind[c]) == kRleBad) return false;
        // the pixels: a lane takes four consecutive ordinals, finds the first one's token by bisection of the scanned
        // ends and stores a dword where the four lie in one token at an aligned address, else bytes
        const uint32_t total = PNG_UNI(M.end[63]);
        for (uint32_t q0 = 4 * PNG_LANE0; q0 < total; q0 += 4 * PNG_LANE_STEP) {
            uint32_t j = 0;
            for (uint32_t step = 32; step; step >>= 1)
                if (M.end[j + step - 1] <= q0) j += step;
            uint32_t       k = q0 - M.pos[j];
            const uint8_t* pay = win + 2 * (size_t)(j + 1);
            PNG_GLOBAL uint8_t* d = (PNG_GLOBAL uint8_t*)(J.idx + (uint64_t)M.y[j] * (uint64_t)J.pitch + M.x[j] + k);
            if (M.end[j] - q0 >= 4 && ((uint64_t)d & 3) == 0) {
                *(PNG_GLOBAL uint32_t*)d = rle_pixel(M, depth, j, pay, k) | rle_pixel(M, depth, j, pay, k + 1) << 8 |
                                           rle_pixel(M, depth, j, pay, k + 2) << 16 | rle_pixel(M, depth, j, pay, k + 3) << 24;
                continue;
            }
            for (uint32_t q = q0; q < q0 + 4 && q < total; q++, k++, d++) {
                if (q >= M.end[j]) { // the next token that holds pixels
                    do j++;
                    while (M.end[j] <= q);
                    k = 0, pay = win + 2 * (size_t)(j + 1);
                    d = (PNG_GLOBAL uint8_t*)(J.idx + (uint64_t)M.y[j] * (uint64_t)J.pitch + M.x[j]);
                }
                *d = (uint8_t)rle_pixel(M, depth, j, pay, k);
            }
        }
        if (c < 64) return true;
        const uint32_t e = last_lane(eol), adv = PNG_UNI(M.sx[63]) + PNG_UNI(M.dx[63]);
        xc = e < 64 ? adv - PNG_UNI(M.sx[e]) : xc + adv;
        yc += PNG_UNI(M.sy[63]) + PNG_UNI(M.dy[63]);
        xc = xc < W ? xc : W, yc = yc < H ? yc : H;
        const uint32_t last = last_lane(starts);
        first = last + PNG_UNI(M.span[last]) - 64;
    }
}

} // namespace pmdev
} // namespace aeon_hip
