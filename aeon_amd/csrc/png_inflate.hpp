// png_inflate.hpp -- the PNG stage's per-wave logic (png_kernels.hip), written once for the device and for
// the host: png_inflate and png_unfilter run it on the 64 lanes of one wave; png_host.cpp's png_gpu_emulate
// runs the same code with every lane loop walked serially, so the CPU tests and a sanitizer build cover what
// the kernels run.  A lane loop is `for (int l = PNG_LANE0; l < n; l += PNG_LANE_STEP)`: lane l, l + 64, ...
// on the device, 0, 1, 2, ... on the host.  Everything outside a lane loop is wave-uniform: what it loads
// (LDS tables, the compressed words) passes through PNG_UNI (readfirstlane on the device), so the bit reader
// and the symbol decode stay in scalar registers and their branches are scalar branches.  See DESIGN §19.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "png.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define PNG_FN __device__ __forceinline__
#define PNG_LANE0 ((int)threadIdx.x)
#define PNG_LANE_STEP 64
#define PNG_SLOT(l) 0 // a lane's own accumulators: one set in its registers
#define PNG_SLOTS 1
#define PNG_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define PNG_SYNC() __syncthreads() // (a workgroup of one wave: orders the lanes' LDS and scratch accesses)
#define PNG_GLOBAL __attribute__((address_space(1)))
#else
#if defined(__HIP__) // (the host pass over a .hip file: the kernels' calls of the templates must resolve there too)
#define PNG_FN __host__ __device__ inline
#else
#define PNG_FN inline
#endif
#define PNG_LANE0 0
#define PNG_LANE_STEP 1
#define PNG_SLOT(l) (l)
#define PNG_SLOTS 64
#define PNG_UNI(x) ((uint32_t)(x))
#define PNG_SYNC() ((void)0)
#define PNG_GLOBAL
#endif

namespace aeon_hip {
namespace pngdev {

constexpr int      kRing     = kPngWindow; // the window: a ring of the last 32 KiB produced
constexpr uint32_t kRingMask = kRing - 1;
constexpr int      kFlush    = 1024; // bytes a flush round stores: 64 lanes x 16
constexpr int      kLitBits  = 10;   // lookahead of the literal/length and distance tables
constexpr int      kMaxLit   = 288, kMaxDist = 32, kMaxSyms = kMaxLit + kMaxDist;
constexpr uint32_t kAdlerMod = 65521;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One code set's decode tables: a lookahead table (entry = symbol | length << 12, 0: no code that short)
// and puff's canonical walk for the longer codes (count of codes per length, symbols sorted by code).
struct Code {
    uint16_t fast[1 << kLitBits];
    uint16_t count[16];
    uint16_t first[16]; // first canonical code of each length
    uint16_t offs[16];  // index of its first symbol in `sorted`
    uint16_t sorted[kMaxLit];
};

// The wave's LDS (png_inflate) or the emulation's heap block: 32 KiB of window and ~7.5 KB of tables.
struct alignas(16) InflateMem {
    uint8_t  ring[kRing];
    Code     lit, dist;
    uint8_t  lens[kMaxSyms + 2];
    uint16_t rank[kMaxSyms];
    uint32_t red[2][64]; // the lanes' Adler sums
};

// Wave-uniform state: the bit reader over the file's compressed words, the output position, what is flushed.
struct Inflate {
    const PNG_GLOBAL uint32_t* in; // compressed stream, 4-byte aligned, readable to clen rounded up to 8
    PNG_GLOBAL uint8_t*        raw; // the file's scratch (16-byte aligned, capacity `need` rounded up to 16)
    uint32_t clen, need;
    uint64_t hold;
    uint32_t nbits, ip; // ip: bytes loaded so far
    uint32_t pos, fl;   // bytes produced / flushed
    uint32_t ad1[PNG_SLOTS], ad2[PNG_SLOTS];
};

PNG_FN uint32_t load_word(const Inflate& S, uint32_t byte)
{
    // past the stream: zeros (the consumed-bits check below then ends the decode)
    return byte < ((S.clen + 7) & ~7u) ? PNG_UNI(S.in[byte >> 2]) : 0u;
}
PNG_FN void refill(Inflate& S)
{
    if (S.nbits < 32) {
        S.hold |= (uint64_t)load_word(S, S.ip) << S.nbits;
        S.nbits += 32, S.ip += 4;
    }
}
PNG_FN void seek(Inflate& S, uint32_t byte)
{
    const uint32_t a = byte & ~3u, sh = 8 * (byte & 3);
    S.hold  = (uint64_t)(load_word(S, a) >> sh);
    S.nbits = 32 - sh, S.ip = a + 4;
    refill(S);
}
PNG_FN uint64_t bit_pos(const Inflate& S) { return (uint64_t)8 * S.ip - S.nbits; } // bits consumed
PNG_FN bool     overrun(const Inflate& S) { return bit_pos(S) > (uint64_t)8 * S.clen; }
PNG_FN uint32_t take(Inflate& S, uint32_t n) // n <= 16 bits of a refilled reader
{
    const uint32_t v = (uint32_t)S.hold & ((1u << n) - 1);
    S.hold >>= n, S.nbits -= n;
    return v;
}

// The tables of a code set from lens[0..n): counts and ranks by the lanes (one length each), the judgement
// zlib's inflate_table makes (over-subscribed: refused; incomplete: refused unless `lone_ok` and the set is a
// single code of one bit; no code at all: accepted, every lookup then fails), then codes and table entries by
// the lanes (one symbol each).  fbits: the lookahead (7 for the code-length code, whose codes are no longer).
PNG_FN bool build_code(InflateMem& M, Code& C, const uint8_t* lens, int n, int fbits, bool lone_ok, bool judge)
{
    PNG_SYNC();
    for (int l = PNG_LANE0; l < 64; l += PNG_LANE_STEP) {
        if (l < 16) {
            int c = 0;
            if (l > 0)
                for (int s = 0; s < n; s++)
                    if (lens[s] == l) M.rank[s] = (uint16_t)c++;
            C.count[l] = (uint16_t)c;
        }
    }
    for (int i = PNG_LANE0; i < (1 << fbits); i += PNG_LANE_STEP) C.fast[i] = 0;
    PNG_SYNC();
    int left = 1, max = 0, code = 0, off = 0;
    bool over = false;
    for (int len = 1; len <= 15; len++) {
        const int c = (int)PNG_UNI(C.count[len]);
        left        = (left << 1) - c;
        if (left < 0) over = true, left = 0;
        if (c) max = len;
        C.first[len] = (uint16_t)code, C.offs[len] = (uint16_t)off; // (every lane writes the same value)
        code = (code + c) << 1, off += c;
    }
    if (judge && (over || (max > 0 && left > 0 && !(lone_ok && max == 1)))) return false;
    PNG_SYNC();
    for (int s = PNG_LANE0; s < n; s += PNG_LANE_STEP) {
        const int len = lens[s];
        if (!len) continue;
        const uint32_t c = (uint32_t)C.first[len] + M.rank[s];
        C.sorted[C.offs[len] + M.rank[s]] = (uint16_t)s;
        if (len <= fbits) {
            uint32_t rev = 0;
            for (int k = 0; k < len; k++) rev |= ((c >> k) & 1u) << (len - 1 - k);
            for (uint32_t e = rev; e < (1u << fbits); e += 1u << len) C.fast[e] = (uint16_t)(s | len << 12);
        }
    }
    PNG_SYNC();
    return true;
}

// One symbol of code C off a refilled reader (15 bits at most); -1: no such code.
PNG_FN int decode_sym(Inflate& S, const Code& C, int fbits)
{
    const uint32_t e = PNG_UNI(C.fast[(uint32_t)S.hold & ((1u << fbits) - 1)]);
    if (e) {
        take(S, e >> 12);
        return (int)(e & 0xfff);
    }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; len++) {
        code |= (int)((S.hold >> (len - 1)) & 1);
        const int cnt = (int)PNG_UNI(C.count[len]);
        if (code - cnt < first) {
            take(S, len);
            return (int)PNG_UNI(C.sorted[index + (code - first)]);
        }
        index += cnt, first += cnt;
        first <<= 1, code <<= 1;
    }
    return -1;
}

// A lane's share of the Adler-32 sums: s1 = sum of bytes, s2 = sum of (index mod 65521) * byte, of what it flushed.
PNG_FN void adler_add(Inflate& S, int slot, uint32_t idx_mod, const uint32_t (&w)[4])
{
    uint32_t s1 = 0, s2 = 0; // 16 bytes: s2 <= 16 * 65536 * 255 < 2^32
    for (int k = 0; k < 16; k++) {
        const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xff;
        s1 += b, s2 += (idx_mod + k) * b;
    }
    S.ad1[slot] = (S.ad1[slot] + s1) % kAdlerMod;
    S.ad2[slot] = (S.ad2[slot] + s2 % kAdlerMod) % kAdlerMod;
}

// The ring's whole 1 KiB rounds leave for the scratch: 16 bytes per lane, one coalesced store round each.
PNG_FN void flush(InflateMem& M, Inflate& S)
{
    if (S.pos - S.fl < (uint32_t)kFlush) return;
    PNG_SYNC();
    while (S.pos - S.fl >= (uint32_t)kFlush) {
        for (int l = PNG_LANE0; l < 64; l += PNG_LANE_STEP) {
            const uint32_t  at = S.fl + 16 * l;
            const uint32_t* w  = (const uint32_t*)(M.ring + (at & kRingMask));
            const uint32_t  v[4] = {w[0], w[1], w[2], w[3]};
            *(PNG_GLOBAL u32x4*)(S.raw + at) = u32x4{v[0], v[1], v[2], v[3]};
            adler_add(S, PNG_SLOT(l), at % kAdlerMod, v);
        }
        S.fl += kFlush;
    }
}

// The last bytes (fewer than a round), then the lanes' sums reduced with the position weights:
// a = 1 + sum b[i], b = n + sum (n - i) b[i]  (mod 65521).  Returns the stream's Adler-32.
PNG_FN uint32_t flush_tail(InflateMem& M, Inflate& S)
{
    PNG_SYNC();
    for (uint32_t i = S.fl + PNG_LANE0; i < S.pos; i += PNG_LANE_STEP) {
        const uint32_t b = M.ring[i & kRingMask];
        S.raw[i]         = (uint8_t)b;
        const int slot   = PNG_SLOT((int)((i - S.fl) & 63));
        S.ad1[slot]      = (S.ad1[slot] + b) % kAdlerMod;
        S.ad2[slot]      = (S.ad2[slot] + (i % kAdlerMod) * b % kAdlerMod) % kAdlerMod;
    }
    S.fl = S.pos;
    for (int l = PNG_LANE0; l < 64; l += PNG_LANE_STEP) M.red[0][l] = S.ad1[PNG_SLOT(l)], M.red[1][l] = S.ad2[PNG_SLOT(l)];
    PNG_SYNC();
    uint64_t s1 = 0, s2 = 0;
    for (int l = 0; l < 64; l++) s1 += PNG_UNI(M.red[0][l]), s2 += PNG_UNI(M.red[1][l]);
    s1 %= kAdlerMod, s2 %= kAdlerMod;
    const uint64_t n = S.pos % kAdlerMod;
    const uint32_t a = (uint32_t)((1 + s1) % kAdlerMod);
    const uint32_t b = (uint32_t)((n + n * s1 + kAdlerMod - s2) % kAdlerMod);
    return b << 16 | a;
}

// `len` bytes `dist` back, by all lanes: out[p + i] = out[p - dist + i mod dist], every source below p, so a
// short distance is a periodic fill and never a chain through bytes this copy writes.
PNG_FN void copy_match(InflateMem& M, Inflate& S, uint32_t len, uint32_t dist)
{
    PNG_SYNC();
    const uint32_t p = S.pos;
    for (uint32_t i = PNG_LANE0; i < len; i += PNG_LANE_STEP) {
        const uint32_t k              = dist >= len ? i : i % dist;
        const uint8_t  v              = M.ring[(p - dist + k) & kRingMask];
        M.ring[(p + i) & kRingMask] = v;
    }
    S.pos = p + len;
}

constexpr uint16_t kLenBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                   31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t  kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t kDistBase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                    193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t  kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
// (the base / extra-bit tables as arithmetic: a constant array indexed by a run-time symbol is a memory load)
PNG_FN uint32_t len_extra(uint32_t s) { return s < 8 || s == 28 ? 0 : (s - 4) >> 2; }
PNG_FN uint32_t len_base(uint32_t s)
{
    if (s < 8) return 3 + s;
    if (s == 28) return 258;
    const uint32_t e = (s - 4) >> 2;
    return 3 + ((4 + (s & 3)) << e);
}
PNG_FN uint32_t dist_extra(uint32_t s) { return s < 4 ? 0 : (s - 2) >> 1; }
PNG_FN uint32_t dist_base(uint32_t s) { return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s - 2) >> 1)); }

// The code lengths of a dynamic block's two code sets, through its code-length code; then both tables.
PNG_FN bool dynamic_tables(InflateMem& M, Inflate& S)
{
    refill(S);
    const int nlen = (int)take(S, 5) + 257, ndist = (int)take(S, 5) + 1, ncode = (int)take(S, 4) + 4;
    if (nlen > 286 || ndist > 30) return false;
    PNG_SYNC();
    for (int i = PNG_LANE0; i < 19; i += PNG_LANE_STEP) M.lens[i] = 0;
    PNG_SYNC();
    for (int i = 0; i < ncode; i++) {
        refill(S);
        M.lens[kClOrder[i]] = (uint8_t)take(S, 3); // (every lane the same value)
    }
    if (!build_code(M, M.dist, M.lens, 19, 7, false, true)) return false; // (in the distance set's tables, rebuilt below)
    int i = 0, prev = 0;
    while (i < nlen + ndist) {
        refill(S);
        const int sym = decode_sym(S, M.dist, 7);
        if (sym < 0 || overrun(S)) return false;
        if (sym < 16) {
            M.lens[i++] = (uint8_t)sym, prev = sym;
            continue;
        }
        int rep, val = 0;
        if (sym == 16) {
            if (i == 0) return false;
            val = prev, rep = 3 + (int)take(S, 2);
        } else if (sym == 17) {
            rep = 3 + (int)take(S, 3);
        } else {
            rep = 11 + (int)take(S, 7);
        }
        if (i + rep > nlen + ndist) return false;
        for (int k = PNG_LANE0; k < rep; k += PNG_LANE_STEP) M.lens[i + k] = (uint8_t)val;
        i += rep, prev = val;
    }
    PNG_SYNC();
    if (PNG_UNI(M.lens[256]) == 0) return false; // no end-of-block code
    // the literal/length lengths stay where they are; the distance lengths behind them
    if (!build_code(M, M.lit, M.lens, nlen, kLitBits, true, true)) return false;
    return build_code(M, M.dist, M.lens + nlen, ndist, kLitBits, true, true);
}

PNG_FN void fixed_tables(InflateMem& M)
{
    PNG_SYNC();
    for (int s = PNG_LANE0; s < kMaxSyms; s += PNG_LANE_STEP)
        M.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    build_code(M, M.lit, M.lens, 288, kLitBits, true, false);
    build_code(M, M.dist, M.lens + 288, 32, kLitBits, true, false); // (30 and 31 decode, and are refused)
}

// What a failed step of a stream that may be cut (the TIFF stage's strips, kCut) comes to: where the bits the
// step took reach past the stream's end, the input ran out -- zlib, which judges nothing it has not all the bits
// of, then stops without an error -- and the stream counts if everything it is needed for is out.  A PNG's
// stream (kCut false) fails.
template <bool kCut>
PNG_FN bool ran_out(InflateMem& M, Inflate& S)
{
    if (!kCut || !overrun(S) || S.pos != S.need) return false;
    flush_tail(M, S);
    return true;
}

// The file's zlib stream inflated into its scratch.  False: the stream is one zlib refuses, or does not make
// exactly `need` bytes.  Every loop ends: a symbol consumes a bit at least, reading past the stream's end is
// an error, and nothing is written past `need`.
// kCut (a TIFF strip, tiff_strips.hpp): the stream may make more than `need` bytes; it is inflated as zlib's
// inflate(Z_FINISH) does into a buffer of `need` bytes: the symbol that would write past them is checked, copied as
// far as the room goes and ends the decode; what comes behind it is not looked at.  skip: bytes ahead of the
// stream at `in` (a strip starts at any byte of its file; `clen` counts them in).
template <bool kCut = false>
PNG_FN bool inflate_file(InflateMem& M, Inflate& S, uint32_t skip = 0)
{
    for (int l = 0; l < PNG_SLOTS; l++) S.ad1[l] = S.ad2[l] = 0;
    S.pos = S.fl = 0;
    if (S.clen < 6 + skip) return false;
    seek(S, 2 + skip); // (the host checked the two header bytes)
    for (bool last = false; !last;) {
        refill(S);
        last                = take(S, 1) != 0;
        const uint32_t type = take(S, 2);
        if (overrun(S)) return ran_out<kCut>(M, S);
        if (type == 0) {
            const uint32_t at = (uint32_t)((bit_pos(S) + 7) >> 3); // LEN, NLEN at the next byte
            if ((uint64_t)at + 4 > S.clen) return kCut && S.pos == S.need ? (flush_tail(M, S), true) : false;
            seek(S, at);
            uint32_t len = take(S, 16);
            refill(S);
            if ((take(S, 16) ^ 0xffff) != len) return false;
            bool cut = false;
            if (kCut && len > S.need - S.pos) len = S.need - S.pos, cut = true;
            if ((uint64_t)at + 4 + len > S.clen || len > S.need - S.pos) return false;
            const PNG_GLOBAL uint8_t* src = (const PNG_GLOBAL uint8_t*)S.in + at + 4;
            for (uint32_t done = 0; done < len;) {
                const uint32_t n = len - done < 4096 ? len - done : 4096;
                PNG_SYNC();
                for (uint32_t i = PNG_LANE0; i < n; i += PNG_LANE_STEP) M.ring[(S.pos + i) & kRingMask] = src[done + i];
                S.pos += n, done += n;
                flush(M, S);
            }
            if (kCut && cut) return flush_tail(M, S), true;
            seek(S, at + 4 + len);
            continue;
        }
        if (type == 3) return false;
        if (type == 1) fixed_tables(M);
        else if (!dynamic_tables(M, S)) return ran_out<kCut>(M, S);
        for (;;) {
            refill(S);
            int sym = decode_sym(S, M.lit, kLitBits);
            if (kCut && overrun(S)) return ran_out<kCut>(M, S);
            if (sym < 0 || overrun(S)) return false;
            if (sym < 256) {
                if (S.pos >= S.need) return kCut ? (flush_tail(M, S), true) : false;
                for (int l = PNG_LANE0; l < 1; l += PNG_LANE_STEP) M.ring[S.pos & kRingMask] = (uint8_t)sym;
                S.pos++;
            } else if (sym == 256) {
                break;
            } else {
                sym -= 257;
                if (sym >= 29) return false; // 286, 287
                uint32_t len = len_base((uint32_t)sym) + take(S, len_extra((uint32_t)sym));
                refill(S);
                const int ds = decode_sym(S, M.dist, kLitBits);
                if (kCut && overrun(S)) return ran_out<kCut>(M, S);
                if (ds < 0 || ds >= 30) return false;
                const uint32_t dist = dist_base((uint32_t)ds) + take(S, dist_extra((uint32_t)ds));
                if (kCut && overrun(S)) return ran_out<kCut>(M, S);
                if (overrun(S) || dist > S.pos) return false;
                if (len > S.need - S.pos) {
                    if (!kCut) return false;
                    copy_match(M, S, S.need - S.pos, dist);
                    return flush_tail(M, S), true;
                }
                copy_match(M, S, len, dist);
            }
            flush(M, S);
        }
    }
    if (S.pos != S.need) return false; // short output
    const uint32_t adler = flush_tail(M, S);
    const uint32_t at    = (uint32_t)((bit_pos(S) + 7) >> 3);
    if ((uint64_t)at + 4 > S.clen) return kCut;
    seek(S, at);
    const uint32_t t0 = take(S, 16);
    refill(S);
    const uint32_t t1 = take(S, 16), le = t0 | t1 << 16; // the trailer is big-endian
    return __builtin_bswap32(le) == adler;
}

// ---- row filters and conversion (png_unfilter) --------------------------------------------------------

// One byte: x = filtered, a = left, b = up, c = up-left (RFC 2083 section 6).
PNG_FN uint32_t unfilter_byte(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t pred = 0;
    if (ft == 1) pred = a;
    else if (ft == 2) pred = b;
    else if (ft == 3) pred = (a + b) >> 1;
    else if (ft == 4) {
        const int p = (int)a + (int)b - (int)c;
        const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p;
        const int pc = p > (int)c ? p - (int)c : (int)c - p;
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (x + pred) & 0xff;
}

// A band of `rows` consecutive rows in `band` (rows of pitch bytes: the filter byte, then rowb bytes), lane r
// its row r, one pixel behind row r - 1: at step t lane r undoes pixel t - r in place, reading the pixel above
// (written a step earlier by lane r - 1; row 0 reads `prev`, the last row of the band before) and keeping its
// own left pixel and the up-left one (the pixel above of its previous step).  False: a filter byte above 4.
PNG_FN bool unfilter_band(uint8_t* band, const uint8_t* prev, int rows, int rowb, int pitch, int bpp)
{
    const int units = rowb / bpp; // (rowb is a multiple of bpp: bpp > 1 only at 8 and 16 bits)
    uint64_t  la[PNG_SLOTS], lc[PNG_SLOTS]; // the left and up-left pixels, a byte each 8 bits
    bool      ok = true;
    PNG_SYNC();
    for (int r = PNG_LANE0; r < rows; r += PNG_LANE_STEP)
        if (band[(size_t)r * pitch] > 4) ok = false;
    for (int t = 0; t < units + rows - 1; t++) {
        for (int r = PNG_LANE0; r < rows; r += PNG_LANE_STEP) {
            const int x = t - r;
            if (x < 0 || x >= units) continue;
            uint8_t*       row = band + (size_t)r * pitch + 1;
            const uint8_t* up  = r ? row - pitch : prev;
            const uint32_t ft  = band[(size_t)r * pitch];
            const uint64_t a = x ? la[PNG_SLOT(r)] : 0, c = x ? lc[PNG_SLOT(r)] : 0;
            uint64_t       na = 0, nc = 0;
            for (int k = 0; k < bpp; k++) {
                const uint32_t av = (uint32_t)(a >> (8 * k)) & 0xff, cv = (uint32_t)(c >> (8 * k)) & 0xff;
                const uint32_t bv = up[x * bpp + k];
                const uint32_t v  = unfilter_byte(ft, row[x * bpp + k], av, bv, cv);
                row[x * bpp + k]  = (uint8_t)v;
                na |= (uint64_t)v << (8 * k), nc |= (uint64_t)bv << (8 * k);
            }
            la[PNG_SLOT(r)] = na, lc[PNG_SLOT(r)] = nc;
        }
        PNG_SYNC();
    }
    return ok;
}

PNG_FN uint32_t sample_at(const uint8_t* row, uint32_t s, int depth)
{
    if (depth == 16) return (uint32_t)row[2 * s] << 8 | row[2 * s + 1];
    if (depth == 8) return row[s];
    const uint32_t bit = s * depth;
    return (row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1u << depth) - 1);
}

// libpng 1.2's png_do_rgb_to_gray without gamma (png_host.cpp rgb_to_gray): 9797 / 19234 / 3737, truncating.
PNG_FN uint32_t to_gray(uint32_t r, uint32_t g, uint32_t b)
{
    return (r == g && r == b) ? r : (9797u * r + 19234u * g + 3737u * b) >> 15;
}

// Byte k of an output row (png_host.cpp's png_emit_row, per output byte) from the unfiltered row.
// *bad: a palette index past PLTE.
PNG_FN uint32_t out_byte(const PngJob& J, const uint8_t* pal, const uint8_t* row, uint32_t k, bool* bad)
{
    const int  depth = J.depth, ct = J.ctype;
    const bool bgr = J.mode == AEON_PNG_BGR8, out16 = J.elem_bytes == 2;
    const uint32_t px = bgr ? k / 3 : out16 ? k >> 1 : k;
    uint32_t r, g, b;
    bool     gray = false;
    if (ct == 3) {
        uint32_t idx = sample_at(row, px, depth);
        if ((int)idx >= J.npal) *bad = true, idx = 0;
        r = pal[3 * idx], g = pal[3 * idx + 1], b = pal[3 * idx + 2];
    } else if (ct == 0 || ct == 4) {
        uint32_t v = sample_at(row, px * J.samples, depth);
        if (depth < 8) v *= depth == 1 ? 255 : depth == 2 ? 85 : 17;
        r = g = b = v, gray = true;
    } else {
        r = sample_at(row, px * J.samples, depth), g = sample_at(row, px * J.samples + 1, depth);
        b = sample_at(row, px * J.samples + 2, depth);
    }
    const bool wide = depth == 16 && ct != 3;
    if (bgr) {
        const uint32_t ch = k - 3 * px, v = ch == 0 ? b : ch == 1 ? g : r;
        return (wide ? v >> 8 : v) & 0xff; // png_set_strip_16: the high byte
    }
    const uint32_t v = gray ? r : to_gray(r, g, b);
    if (out16) return (v >> (8 * (k & 1))) & 0xff; // native (little-endian) uint16
    return (wide ? v >> 8 : v) & 0xff;
}

// Rows of a band: how many the LDS of `lds` bytes holds beside the previous row and the palette.
PNG_FN int band_rows(int rowb, int lds)
{
    const int pitch = rowb + 1, room = (lds - kPngUnfilterFixed - ((rowb + 15) & ~15) - 16) / pitch;
    return room < 1 ? 0 : room > 64 ? 64 : room;
}

// The file's scratch unfiltered band by band and converted into its record.  mem: `lds` bytes, 16-byte
// aligned: the palette, the previous row, the band.  False: a filter byte above 4 or a palette index past PLTE.
PNG_FN bool unfilter_file(const PngJob& J, uint8_t* mem, int lds)
{
    const int rowb = J.rowb, pitch = rowb + 1, bpp = J.bpp, R = band_rows(rowb, lds);
    uint8_t*  pal  = mem;
    uint8_t*  prev = mem + kPngUnfilterFixed;
    uint8_t*  band = prev + ((rowb + 15) & ~15);
    const PNG_GLOBAL uint8_t* raw = (const PNG_GLOBAL uint8_t*)J.raw;
    PNG_GLOBAL uint8_t*       out = (PNG_GLOBAL uint8_t*)J.out;
    if (R < 1) return false;
    bool ok = true;
    PNG_SYNC();
    for (int i = PNG_LANE0; i < 768; i += PNG_LANE_STEP) pal[i] = J.pal[i];
    for (int i = PNG_LANE0; i < rowb; i += PNG_LANE_STEP) prev[i] = 0;
    for (int y0 = 0; y0 < J.h; y0 += R) {
        const int rows = J.h - y0 < R ? J.h - y0 : R;
        // the band's bytes are contiguous in the scratch: whole words, the band placed at its own offset mod 4
        const size_t   g0 = (size_t)y0 * pitch, g1 = g0 + (size_t)rows * pitch;
        const uint32_t sh = (uint32_t)(g0 & 3);
        PNG_SYNC();
        {
            const PNG_GLOBAL uint32_t* gw = (const PNG_GLOBAL uint32_t*)(raw + (g0 - sh));
            uint32_t*                  lw = (uint32_t*)band;
            const int                  nw = (int)((g1 - (g0 - sh) + 3) >> 2);
            for (int i = PNG_LANE0; i < nw; i += PNG_LANE_STEP) lw[i] = gw[i];
        }
        uint8_t* b0 = band + sh;
        if (!unfilter_band(b0, prev, rows, rowb, pitch, bpp)) ok = false;
        // the finished rows converted where they lie: four output bytes per lane and store
        const uint32_t ob = (uint32_t)J.out_row_bytes;
        bool           bad = false;
        for (int r = 0; r < rows; r++) {
            const uint8_t*      row = b0 + (size_t)r * pitch + 1;
            PNG_GLOBAL uint8_t* d   = out + (size_t)(y0 + r) * J.stride;
            const bool          al  = (((uint64_t)(size_t)d) & 3) == 0;
            for (uint32_t k = 4 * PNG_LANE0; k < ob; k += 4 * PNG_LANE_STEP) {
                uint32_t v = 0;
                const uint32_t n = ob - k < 4 ? ob - k : 4;
                for (uint32_t j = 0; j < n; j++) v |= out_byte(J, pal, row, k + j, &bad) << (8 * j);
                if (al && n == 4) *(PNG_GLOBAL uint32_t*)(d + k) = v;
                else
                    for (uint32_t j = 0; j < n; j++) d[k + j] = (uint8_t)(v >> (8 * j));
            }
        }
        if (bad) ok = false;
        PNG_SYNC();
        for (int i = PNG_LANE0; i < rowb; i += PNG_LANE_STEP) prev[i] = b0[(size_t)(rows - 1) * pitch + 1 + i];
    }
    return ok;
}

} // namespace pngdev
} // namespace aeon_hip
