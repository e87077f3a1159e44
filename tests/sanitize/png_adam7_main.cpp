// png_adam7_main.cpp -- the opt-in interlaced PNG path's host half (aeon_png_interlaced_route: png_plan with
// png_route_adam7) and its kernels' code run on the host (aeon_png_gpu_emulate_interlaced: png_inflate and
// png_unfilter_adam7 as png_inflate.hpp has them) under AddressSanitizer + UndefinedBehaviorSanitizer (Makefile
// target sanitize_png_adam7; tests/test_sanitize_png_adam7.py runs it).  Arguments: interlaced PNG files.  Each
// file, truncations of it and single-byte mutations of it (the chunk's CRC mended, so the mutation reaches the
// inflate, the filters and the palette) go through both entries in the three modes.  Whatever the emulation
// decodes, aeon_decode_png must decode to the same bytes; what it refuses must be refused with a code of the C
// ABI.  Exit status 0 and a count on stdout, or 1 and the first disagreement.
#include <zlib.h>

#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"

namespace {

long g_runs = 0, g_decoded = 0, g_refused = 0;

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// The CRC of the chunk that holds byte `at` recomputed (a walk over well-formed chunk lengths only).
void mend_crc(std::vector<uint8_t>& f, size_t at)
{
    for (size_t p = 8; p + 12 <= f.size();) {
        const size_t len = be32(&f[p]);
        if (len > f.size() - p - 12) return;
        if (at >= p + 4 && at < p + 8 + len) {
            const uint32_t c = (uint32_t)crc32(0L, &f[p + 4], (uInt)(len + 4));
            f[p + 8 + len] = c >> 24, f[p + 9 + len] = c >> 16, f[p + 10 + len] = c >> 8, f[p + 11 + len] = c;
            return;
        }
        p += 12 + len;
    }
}

bool run(const std::vector<uint8_t>& f, const std::string& what)
{
    int w = 0, h = 0, depth = 0, ctype = 0, route = -1;
    const bool info = aeon_png_info(f.data(), f.size(), &w, &h, &depth, &ctype) == 0;
    const int  rr   = aeon_png_interlaced_route(f.data(), f.size(), &route);
    if (rr != 0 && rr != AEON_HIP_EINVAL) {
        std::printf("%s: the route returned %d (%s)\n", what.c_str(), rr, aeon_hip_last_error());
        return false;
    }
    if (!info || (size_t)w * h > (1u << 22)) return true;
    for (int mode = AEON_PNG_BGR8; mode <= AEON_PNG_ANYDEPTH; mode++) {
        g_runs++;
        const size_t eb = (mode == AEON_PNG_ANYDEPTH && depth == 16 && ctype != 3) ? 2 : 1;
        const size_t stride = (size_t)w * (mode == AEON_PNG_BGR8 ? 3 : 1) * eb;
        std::vector<uint8_t> a(stride * h, 0xA5), b(stride * h, 0x5A);
        const int re = aeon_png_gpu_emulate_interlaced(f.data(), f.size(), mode, a.data(), stride);
        if (re == 0) {
            g_decoded++;
            const int rd = aeon_decode_png(f.data(), f.size(), mode, b.data(), stride, nullptr);
            if (rr != 0 || route != 1 || rd != 0 || a != b) {
                std::printf("%s mode %d: the emulation decoded, route %d (%d), decoder %d, equal %d\n", what.c_str(), mode,
                            route, rr, rd, (int)(a == b));
                return false;
            }
        } else if (re == AEON_HIP_EINVAL || re == AEON_HIP_EDEVICE || re == AEON_HIP_EUNSUPPORTED) {
            g_refused++;
            if ((re == AEON_HIP_EINVAL) != (rr == AEON_HIP_EINVAL) || (re == AEON_HIP_EUNSUPPORTED) != (rr == 0 && route == 0)) {
                std::printf("%s mode %d: emulation %d, route %d (%d)\n", what.c_str(), mode, re, route, rr);
                return false;
            }
        } else {
            std::printf("%s mode %d: emulation returned %d\n", what.c_str(), mode, re);
            return false;
        }
    }
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    int files = 0;
    for (int i = 1; i < argc; i++) {
        std::ifstream              in(argv[i], std::ios::binary);
        const std::vector<uint8_t> f((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (f.size() < 33 || f[28] != 1) {
            std::printf("%s: not an interlaced PNG file\n", argv[i]);
            return 1;
        }
        files++;
        const std::string name = argv[i];
        if (!run(f, name)) return 1;
        const size_t tstep = f.size() / 64 + 1, mstep = f.size() / 256 + 1;
        for (size_t n = 0; n < f.size(); n += tstep)
            if (!run(std::vector<uint8_t>(f.begin(), f.begin() + n), name + " cut at " + std::to_string(n))) return 1;
        for (size_t at = 33; at < f.size(); at += mstep) { // (behind IHDR: its sizes would only ask for memory)
            static const uint8_t flips[3] = {0x01, 0x80, 0xFF};
            std::vector<uint8_t> m = f;
            m[at] ^= flips[(at / mstep) % 3];
            mend_crc(m, at);
            if (!run(m, name + " byte " + std::to_string(at))) return 1;
        }
    }
    std::printf("%d files, %ld runs: %ld decoded, %ld refused\n", files, g_runs, g_decoded, g_refused);
    return 0;
}
