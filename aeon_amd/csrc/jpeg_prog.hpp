// jpeg_prog.hpp -- one wave's decode of one unit of a progressive JPEG scan (jpeg_prog.hip), written once for the
// device and for the host: jpeg_prog_scan runs walk_unit on a wave; jpeg_host.cpp's jpeg_prog_emulate runs it one
// unit after another with the wave's lanes as arrays (the CPU tests compare it with the host entropy decoder).
// The symbol walk is the same on every lane (one bit reader, one block index, one zigzag position); what the lanes
// hold apart is in Wave: the 64 coefficients of the block in hand (AC refinement), one buffered store each (the
// first scans), one block each (DC refinement).  See jpeg_prog.hip for the design; the scans follow
// decode_progressive_scan (jpeg_host.cpp) line for line.
#pragma once
#include "jpeg_huff.hpp"

namespace aeon_hip {
namespace prog {

using huff::gmem;
using huff::imin;
using huff::kFast;
using huff::kKind;
using huff::kSym;
using huff::kTabs;
using huff::kValue;
using huff::pick4;
using huff::Tables;

typedef HUFF_GLOBAL int16_t* coef_ptr;

// What the lanes of a wave hold apart: per lane on the device, an array over the lanes on the host.
struct Wave {
#if defined(__HIP_DEVICE_COMPILE__)
    int      lane;
    int      c, c0; // zigzag coefficient `lane` of the block in hand, and as it was loaded
    coef_ptr ea;    // buffered store `lane`: where, what
    int      ev;
#else
    int16_t  c[64], c0[64];
    coef_ptr ea[64];
    int16_t  ev[64];
#endif
    int ne; // stores buffered (the same on every lane)
};

HUFF_FN void wave_start(Wave& W)
{
#if defined(__HIP_DEVICE_COMPILE__)
    W.lane = (int)__lane_id();
    W.c = W.c0 = 0, W.ea = nullptr, W.ev = 0;
#endif
    W.ne = 0;
}

// The buffered stores go out, one per lane.
HUFF_FN void ev_flush(Wave& W)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (W.lane < W.ne) *W.ea = (int16_t)W.ev;
#else
    for (int l = 0; l < W.ne; l++) *W.ea[l] = W.ev[l];
#endif
    W.ne = 0;
}

// One coefficient of a first scan: into the next lane's buffer; every lane stores when all 64 hold one.  (A first
// scan writes no coefficient twice, so the stores of one flush never meet.)
HUFF_FN void ev_push(Wave& W, coef_ptr a, int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (W.lane == W.ne) W.ea = a, W.ev = v;
#else
    W.ea[W.ne] = a, W.ev[W.ne] = (int16_t)v;
#endif
    if (++W.ne == 64) ev_flush(W);
}

// The block's row: lane z takes zigzag coefficient z (128 bytes, one load); returns the non-zero ones as a mask.
HUFF_FN uint64_t row_load(Wave& W, coef_ptr blk)
{
#if defined(__HIP_DEVICE_COMPILE__)
    W.c = W.c0 = blk[W.lane];
    return __ballot(W.c != 0);
#else
    uint64_t h = 0;
    for (int l = 0; l < 64; l++) W.c[l] = W.c0[l] = blk[l], h |= (uint64_t)(blk[l] != 0) << l;
    return h;
#endif
}

// Refinement of the history coefficients `span`: the one of rank j (from the lowest position) takes bit j of the
// n-bit field, first bit first (jdphuff.c: a set bit moves a coefficient whose bit p1 is clear away from zero).
HUFF_FN void row_refine(Wave& W, uint64_t span, uint64_t field, int n, int p1, int m1)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(span >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)span, 0u));
    if ((span >> W.lane & 1) && (field >> ((n - 1 - rank) & 63) & 1) && !(W.c & p1)) W.c = (int16_t)(W.c + (W.c >= 0 ? p1 : m1));
#else
    for (int l = 0, rank = 0; l < 64; l++) {
        if (!(span >> l & 1)) continue;
        if ((field >> (n - 1 - rank) & 1) && !(W.c[l] & p1)) W.c[l] = (int16_t)(W.c[l] + (W.c[l] >= 0 ? p1 : m1));
        rank++;
    }
#endif
}

HUFF_FN void row_set(Wave& W, int z, int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (W.lane == z) W.c = v;
#else
    W.c[z] = (int16_t)v;
#endif
}

// The changed coefficients go back, one store instruction.  Not the whole row: the units of a level hold other
// bands of the same block (DC refinement next to a component's AC refinement), whose stores a stale copy would undo.
HUFF_FN void row_store(Wave& W, coef_ptr blk)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (W.c != W.c0) blk[W.lane] = (int16_t)W.c;
#else
    for (int l = 0; l < 64; l++)
        if (W.c[l] != W.c0[l]) blk[l] = W.c[l];
#endif
}

// ---- tables: huff::Tables by the scan's slots ----

// huff::tables_codes over the file's pool (tables t0, t0 + dt, ...; symbols i0, i0 + di, ...); a slot without a
// table holds no code and no long-code prefix.
HUFF_FN void tables_codes(Tables& T, const JpegProgScan& S, int i0, int di)
{
    const HUFF_GLOBAL JpegHuffTab* pool = gmem<const JpegHuffTab>(S.pool);
    for (int i = i0; i < kTabs * 256; i += di) {
        const int id       = S.tab[i >> 8];
        T.vals[i >> 8][i & 255] = id >= 0 ? pool[id].symbols[i & 255] : 0;
    }
    for (int t = i0; t < kTabs; t += di) {
        const int id   = S.tab[t];
        int       code = 0, s = 0;
        T.long_first[t] = kFast;
        for (int l = 1; l <= 16; l++) {
            const int n     = id >= 0 ? pool[id].counts[l - 1] : 0;
            T.delta[t][l]   = s - code;
            T.maxcode[t][l] = n ? code + n - 1 : -1;
            code = (code + n) << 1;
            s += n;
            if (l == kHuffFastBits && id >= 0) T.long_first[t] = code >> 1;
        }
    }
}

// An AC table's entry of lookahead x: the symbol itself (kSym, run << 4 | size in bits 16-23), as huff::long_entry
// gives it for a slot below 2 -- a progressive scan reads a size-0 symbol's run as an EOB run, and a refinement
// scan takes one bit whatever the size says.
HUFF_FN uint32_t sym_entry(const Tables& T, int t, int x)
{
    for (int l = 1; l <= kHuffFastBits; l++) {
        const int code = x >> (kHuffFastBits - l);
        if (code <= T.maxcode[t][l]) return kSym | (uint32_t)l | ((uint32_t)T.vals[t][T.delta[t][l] + code] << 16);
    }
    return 0;
}

// After tables_codes: the fast entries of the slots in use -- a DC-first scan's as the sequential decoder's DC
// tables (huff::fast_entry: the difference decoded where it fits), an AC scan's as symbols.
HUFF_FN void tables_fast(Tables& T, const JpegProgScan& S, int i0, int di)
{
    for (int i = i0; i < S.ntab * kFast; i += di)
        T.fast[i / kFast][i % kFast] = S.Ss == 0 ? huff::fast_entry(T, i / kFast, i % kFast) : sym_entry(T, i / kFast, i % kFast);
}

// ---- the walk ----

// n bits (0..32) of a filled reader.
template <typename B>
HUFF_FN uint32_t take(B& b, int n)
{
    const uint32_t v = n ? (uint32_t)(b.buf >> (64 - n)) : 0u;
    b.skip(n);
    return v;
}

// n bits (0..63), as two reads of at most 32 (fill guarantees 32).
template <typename B>
HUFF_FN uint64_t take_field(B& b, int n)
{
    const int n1 = imin(n, 32), n2 = n - n1;
    b.fill();
    uint64_t f = take(b, n1);
    if (n2) {
        b.fill();
        f = (f << n2) | take(b, n2);
    }
    return f;
}

HUFF_FN uint64_t below(int k) { return k >= 64 ? ~0ull : (1ull << k) - 1; } // positions 0 .. k-1

// Block c of MCU m of the scan (scan order): its 64 coefficients.  m lies in the unit, so inside the component.
HUFF_FN coef_ptr block_at(const JpegProgScan& S, int m, int c)
{
    const int by = (int)(((c < 8 ? S.blk_tab[0] : S.blk_tab[1]) >> (8 * (c & 7))) & 0xff);
    const int i = by & 3, x = (by >> 2) & 3, y = (by >> 4) & 3;
    const int my = m / S.mcux, mx = m - my * S.mcux;
    const int bw = pick4(i, S.bw[0], S.bw[1], S.bw[2], S.bw[3]), hs = pick4(i, S.hs[0], S.hs[1], S.hs[2], S.hs[3]);
    const int vs = pick4(i, S.vs[0], S.vs[1], S.vs[2], S.vs[3]);
    return gmem<int16_t>(pick4(i, S.dvals[0], S.dvals[1], S.dvals[2], S.dvals[3])) + ((size_t)(my * vs + y) * bw + mx * hs + x) * 64;
}

// The next symbol of table slot t: its code's length skipped, the symbol (or for a DC-first table the entry) returned.
// ok = false: no code of <= 16 bits.
template <typename B>
HUFF_FN uint32_t next_entry(const Tables& T, int t, B& b, bool& ok)
{
    b.fill();
    uint32_t e = T.fast[t][(int)(b.buf >> (64 - kHuffFastBits))];
    ok         = true;
    if (!(e & kKind)) e = huff::long_entry(T, t, b.buf, ok);
    return e;
}

// DC first: one difference per block, MCU after MCU; pred << Al into coefficient 0 through the store buffer.
template <typename B>
HUFF_FN bool walk_dc_first(const Tables& T, const JpegProgScan& S, const JpegProgUnit& U, B& b, Wave& W)
{
    int pred0 = 0, pred1 = 0, pred2 = 0, pred3 = 0;
    for (int m = U.first_mcu; m < U.first_mcu + U.n_mcu; m++)
        for (int c = 0; c < S.bpm; c++) {
            const int by = (int)(((c < 8 ? S.blk_tab[0] : S.blk_tab[1]) >> (8 * (c & 7))) & 0xff), i = by & 3;
            bool      ok;
            const uint32_t e = next_entry(T, by >> 6, b, ok);
            if (!ok) return false;
            const int used = (int)(e & 31), z = (e & kKind) == kSym ? (int)((e >> 16) & 0xff) : 0;
            if (z > 15) return false; // (a DC size: the host decoder refuses it too)
            int v = (e & kKind) == kValue ? (int)(int16_t)(e >> 16) : 0;
            if (z) v = huff::extend((int)((b.buf << used) >> (64 - z)), z);
            b.skip(used + z);
            const int pr = pick4(i, pred0, pred1, pred2, pred3) + v;
            pred0 = i == 0 ? pr : pred0, pred1 = i == 1 ? pr : pred1, pred2 = i == 2 ? pr : pred2, pred3 = i == 3 ? pr : pred3;
            ev_push(W, block_at(S, m, c), (int16_t)(pr * (1 << S.Al)));
        }
    return true;
}

// DC refinement, block j of the unit (scan order): bit j of its data ORs 1 << Al into coefficient 0.
template <typename WP>
HUFF_FN void dc_refine_block(const JpegProgScan& S, const JpegProgUnit& U, WP words, int j)
{
    const uint32_t p = U.start_bit + (uint32_t)j;
    if (p >= U.end_bit) return; // (past the data: zeros)
    if (!(__builtin_bswap32(words[p >> 5]) >> (31 - (p & 31)) & 1)) return;
    const int m   = j / S.bpm;
    coef_ptr  blk = block_at(S, U.first_mcu + m, j - m * S.bpm);
    blk[0]        = (int16_t)(blk[0] | (1 << S.Al));
}

// AC first: runs and values of the band's new coefficients through the store buffer; an EOB run skips its blocks
// without touching memory.
template <typename B>
HUFF_FN bool walk_ac_first(const Tables& T, const JpegProgScan& S, const JpegProgUnit& U, B& b, Wave& W)
{
    int eobrun = 0;
    for (int j = 0; j < U.n_mcu; j++) {
        if (eobrun > 0) {
            const int skip = imin(eobrun, U.n_mcu - j);
            eobrun -= skip, j += skip - 1;
            continue;
        }
        coef_ptr blk = block_at(S, U.first_mcu + j, 0);
        for (int k = S.Ss; k <= S.Se; k++) {
            bool           ok;
            const uint32_t e = next_entry(T, 0, b, ok);
            if (!ok) return false;
            b.skip((int)(e & 31));
            const int r = (int)(e >> 20) & 15, z = (int)(e >> 16) & 15;
            if (z) {
                k += r;
                b.fill();
                // (a corrupt run past 63 is clamped to 63, as the host and libjpeg's natural-order table do)
                ev_push(W, blk + imin(k, 63), (int16_t)(huff::extend((int)take(b, z), z) * (1 << S.Al)));
            } else if (r == 15) {
                k += 15;
            } else {
                eobrun = (1 << r) - 1;
                if (r) b.fill(), eobrun += (int)take(b, r);
                break;
            }
        }
    }
    return true;
}

// AC refinement.  Lane z holds coefficient z of the block; H, the band's coefficients that earlier scans made non-zero,
// decides how the bits are read: a symbol (r, s) passes the history coefficients up to the (r+1)-th zero one at or
// after k -- found in ~H by clearing r low bits -- and each of the n passed takes one correction bit, read as one
// field and picked by rank.  Positions at or past k are untouched by this scan so far, so H serves the whole block.
template <typename B>
HUFF_FN bool walk_ac_refine(const Tables& T, const JpegProgScan& S, const JpegProgUnit& U, B& b, Wave& W)
{
    const int      p1 = 1 << S.Al, m1 = -p1;
    const uint64_t band = below(S.Se + 1) & ~below(S.Ss);
    int            eobrun = 0;
    for (int j = 0; j < U.n_mcu; j++) {
        coef_ptr       blk = block_at(S, U.first_mcu + j, 0);
        const uint64_t H   = row_load(W, blk) & band;
        int            k   = S.Ss;
        if (eobrun == 0) {
            for (; k <= S.Se; k++) {
                bool           ok;
                const uint32_t e = next_entry(T, 0, b, ok);
                if (!ok) return false;
                b.skip((int)(e & 31));
                int r = (int)(e >> 20) & 15, v = 0;
                if ((e >> 16) & 15) { // (size 1 by construction; libjpeg only warns otherwise)
                    b.fill();
                    v = take(b, 1) ? p1 : m1;
                } else if (r != 15) {
                    eobrun = 1 << r;
                    if (r) b.fill(), eobrun += (int)take(b, r);
                    break;
                }
                uint64_t Z = ~H & band & ~below(k); // the zero-history positions ahead
                for (; r > 0 && Z; r--) Z &= Z - 1;
                const int      pos  = Z && r == 0 ? __builtin_ctzll(Z) : S.Se + 1; // (run out: past the band)
                const uint64_t span = H & below(pos) & ~below(k);
                const int      n    = __builtin_popcountll(span);
                if (n) row_refine(W, span, take_field(b, n), n, p1, m1);
                k = pos;
                if (v) row_set(W, imin(k, 63), v);
            }
        }
        if (eobrun > 0) { // the band's remaining history coefficients take their bits
            const uint64_t span = H & ~below(k);
            const int      n    = __builtin_popcountll(span);
            if (n) row_refine(W, span, take_field(b, n), n, p1, m1);
            eobrun--;
        }
        row_store(W, blk);
    }
    return true;
}

// One unit.  Returns false on data the host decoder refuses (no code of <= 16 bits, a DC size above 15); the wave
// has then stopped storing.
template <typename WP>
HUFF_FN bool walk_unit(const Tables& T, const JpegProgScan& S, const JpegProgUnit& U, WP words, Wave& W)
{
    wave_start(W);
    if (S.Ss == 0 && S.Ah) { // no codes: the lanes stride over the unit's blocks
        const int total = U.n_mcu * S.bpm;
#if defined(__HIP_DEVICE_COMPILE__)
        for (int j = W.lane; j < total; j += 64) dc_refine_block(S, U, words, j);
#else
        for (int j = 0; j < total; j++) dc_refine_block(S, U, words, j);
#endif
        return true;
    }
    auto b  = huff::bits_from(words, JpegHuffSeg{U.start_bit, U.end_bit, 0, 1}, (int)U.start_bit);
    bool ok = S.Ss == 0 ? walk_dc_first(T, S, U, b, W) : S.Ah == 0 ? walk_ac_first(T, S, U, b, W) : walk_ac_refine(T, S, U, b, W);
    if (ok) ev_flush(W);
    return ok;
}

// The closing pass's mask of one block: its non-zero coefficients (lane z: coefficient z).
HUFF_FN uint64_t block_mask(Wave& W, coef_ptr blk) { return row_load(W, blk); }

} // namespace prog
} // namespace aeon_hip
