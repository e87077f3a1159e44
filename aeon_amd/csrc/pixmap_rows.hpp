// pixmap_rows.hpp -- the pixmap stage's per-band logic (pixmap_kernels.hip), written once for the device and
// for the host: pixmap_convert runs it on the 256 lanes of a workgroup; pixmap_host.cpp's pixmap_gpu_emulate
// runs the same code with every lane loop walked serially (`for (int l = PM_LANE0; l < n; l += PM_LANE_STEP)`:
// lane l, l + 256, ... on the device, 0, 1, 2, ... on the host), so the CPU tests and the sanitizer program
// cover what the kernel runs.  See DESIGN section 20.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pixmap.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define PM_FN __device__ __forceinline__
#define PM_LANE0 ((int)threadIdx.x)
#define PM_LANE_STEP kPixmapLanes
#define PM_SYNC() __syncthreads()
#define PM_GLOBAL __attribute__((address_space(1)))
#else
#define PM_FN inline
#define PM_LANE0 0
#define PM_LANE_STEP 1
#define PM_SYNC() ((void)0)
#define PM_GLOBAL
#endif

namespace aeon_hip {
namespace pmdev {

// What out_byte needs of a job, in registers
struct RowForm {
    int  kind, opp;   // source layout; output bytes per pixel
    bool bgr, out16;
};

// Byte k of an output row from the staged source row; `row` points at source byte `s0` of the row.
PM_FN uint32_t out_byte(const RowForm& F, const uint32_t* tab, const uint8_t* row, uint32_t s0, uint32_t k)
{
    const uint32_t px = F.bgr ? k / 3 : F.out16 ? k >> 1 : k;
    const uint32_t ch = F.bgr ? k - 3 * px : 0;
    if (F.kind <= kPmIndex8) { // through the table: the device only looks up
        uint32_t idx;
        if (F.kind == kPmBits1) idx = (row[(px >> 3) - s0] >> (7 - (px & 7))) & 1;
        else if (F.kind == kPmBits4) idx = (row[(px >> 1) - s0] >> ((px & 1) ? 0 : 4)) & 15;
        else idx = row[px - s0];
        const uint32_t e = tab[idx];
        return F.bgr ? (e >> (8 * ch)) & 0xff : e >> 24;
    }
    if (F.kind == kPmGray8) return row[px - s0];
    if (F.kind == kPmGray16) {
        const uint8_t* p = row + (2 * px - s0);
        return F.out16 ? p[1 - (k & 1)] : p[0]; // native (little-endian) uint16, or the high byte
    }
    if (F.kind == kPmRgb16) {
        const uint8_t* p = row + (6 * px - s0);
        if (F.bgr) return p[2 * (2 - ch)];
        if (!F.out16) return pixmap_gray(p[4], p[2], p[0]); // each sample's high byte, then gray
        const uint32_t r = (uint32_t)p[0] << 8 | p[1], g = (uint32_t)p[2] << 8 | p[3], b = (uint32_t)p[4] << 8 | p[5];
        return (pixmap_gray(b, g, r) >> (8 * (k & 1))) & 0xff;
    }
    const uint32_t spp = F.kind == kPmBgra8 ? 4 : 3;
    const uint8_t* p   = row + (spp * px - s0);
    if (F.kind == kPmRgb8) return F.bgr ? p[2 - ch] : pixmap_gray(p[2], p[1], p[0]);
    return F.bgr ? p[ch] : pixmap_gray(p[0], p[1], p[2]); // kPmBgr8, kPmBgra8
}

// One band: its source bytes -- contiguous in the file, whatever the row order -- into `lds` as aligned words,
// placed at their own offset mod 4; then every lane four consecutive output bytes of a row per step, stored
// as one dword where the destination is aligned and bytewise at a row's unaligned head and tail.
// tab: 256 words; lds: kPixmapBandBytes + 8 bytes, 4-byte aligned.
PM_FN void convert_band(const PixmapJob& J, const PixmapBand& B, uint32_t* tab, uint8_t* lds)
{
    const int     kind = J.kind, rows = B.rows;
    const int64_t pitch = J.pitch, ap = pitch < 0 ? -pitch : pitch;
    const int64_t sb0 = ((int64_t)B.p0 * J.sbits) >> 3, sb1 = (((int64_t)B.p0 + B.np) * J.sbits + 7) >> 3;
    const int64_t ylow = pitch < 0 ? (int64_t)B.y0 + rows - 1 : B.y0; // the band's row that lies lowest in the file
    const int64_t g0 = J.off + ylow * pitch + sb0, g1 = g0 + (int64_t)(rows - 1) * ap + (sb1 - sb0);
    const uint32_t sh = (uint32_t)(g0 & 3);
    {
        const PM_GLOBAL uint32_t* gw = (const PM_GLOBAL uint32_t*)(J.src + (uint64_t)(g0 - sh));
        uint32_t*                 lw = (uint32_t*)lds;
        const int                 nw = (int)((g1 - (g0 - sh) + 3) >> 2);
        for (int i = PM_LANE0; i < nw; i += PM_LANE_STEP) lw[i] = gw[i];
    }
    if (kind <= kPmIndex8)
        for (int i = PM_LANE0; i < 256; i += PM_LANE_STEP) tab[i] = J.table[i];
    PM_SYNC();
    RowForm F;
    F.kind = kind, F.bgr = J.mode == AEON_DECODE_BGR8, F.out16 = J.elem_bytes == 2;
    F.opp  = F.bgr ? 3 : F.out16 ? 2 : 1;
    const uint32_t k0 = (uint32_t)B.p0 * F.opp, n = (uint32_t)B.np * F.opp;
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
        const uint8_t* row = lds + sh + (size_t)(pitch < 0 ? rows - 1 - (int)r : (int)r) * ap;
        uint32_t       v   = 0;
        for (uint32_t j = start; j < end; j++) v |= out_byte(F, tab, row, (uint32_t)sb0, k0 + j) << (8 * (j - start));
        PM_GLOBAL uint8_t* d = (PM_GLOBAL uint8_t*)(da + start);
        if (end - start == 4 && g) *(PM_GLOBAL uint32_t*)d = v;
        else
            for (uint32_t j = 0; j < end - start; j++) d[j] = (uint8_t)(v >> (8 * j));
    }
}

} // namespace pmdev
} // namespace aeon_hip
