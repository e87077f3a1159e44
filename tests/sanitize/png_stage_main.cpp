// png_stage_main.cpp -- the PNG stage's host half (aeon_png_host_stage) and its kernels' code run on the host
// (aeon_png_gpu_emulate: png_inflate.hpp, what png_inflate and png_unfilter compile) under AddressSanitizer +
// UndefinedBehaviorSanitizer (Makefile target sanitize_png; tests/test_png_stage.py runs it).  Arguments: PNG
// files.  Each file, every truncation of it and single-byte mutations of it (the chunk's CRC mended, so the
// mutation reaches the inflate and the filters) go through both entries in the three modes.  Whatever the
// emulation decodes, aeon_decode_png must decode to the same bytes; what it refuses must be refused with a
// code of the C ABI.  Exit status 0 and a count on stdout, or 1 and the first disagreement.
#include <zlib.h>

#include <cstdio>
#include <cstring>
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
    size_t p = 8;
    while (p + 12 <= f.size()) {
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
    int w = 0, h = 0, depth = 0, ctype = 0;
    const bool info = aeon_png_info(f.data(), f.size(), &w, &h, &depth, &ctype) == 0;
    for (int mode = AEON_PNG_BGR8; mode <= AEON_PNG_ANYDEPTH; mode++) {
        g_runs++;
        int     route = -1;
        int64_t staged = 0;
        const int rs = aeon_png_host_stage(f.data(), f.size(), mode, &route, &staged);
        if (rs != 0 && rs != AEON_HIP_EINVAL) {
            std::printf("%s mode %d: host stage returned %d (%s)\n", what.c_str(), mode, rs, aeon_hip_last_error());
            return false;
        }
        if (!info || (size_t)w * h > (1u << 22)) continue;
        const size_t eb = (mode == AEON_PNG_ANYDEPTH && depth == 16 && ctype != 3) ? 2 : 1;
        const size_t stride = (size_t)w * (mode == AEON_PNG_BGR8 ? 3 : 1) * eb;
        std::vector<uint8_t> a(stride * h, 0xA5), b(stride * h, 0x5A);
        const int re = aeon_png_gpu_emulate(f.data(), f.size(), mode, a.data(), stride);
        if (re == 0) {
            g_decoded++;
            const int rd = aeon_decode_png(f.data(), f.size(), mode, b.data(), stride, nullptr);
            if (rs != 0 || route != 1 || rd != 0 || a != b) {
                std::printf("%s mode %d: the emulation decoded, host stage %d route %d, decoder %d, equal %d\n", what.c_str(),
                            mode, rs, route, rd, (int)(a == b));
                return false;
            }
        } else if (re == AEON_HIP_EINVAL || re == AEON_HIP_EDEVICE || re == AEON_HIP_EUNSUPPORTED) {
            g_refused++;
            // parse-time refusals are the host half's too (a file left to the host decoder fails there, or not)
            if (re != AEON_HIP_EUNSUPPORTED && (re == AEON_HIP_EINVAL) != (rs == AEON_HIP_EINVAL)) {
                std::printf("%s mode %d: emulation %d, host stage %d\n", what.c_str(), mode, re, rs);
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
        if (f.empty()) {
            std::printf("%s: cannot read\n", argv[i]);
            return 1;
        }
        files++;
        const std::string name = argv[i];
        if (!run(f, name)) return 1;
        const size_t tstep = f.size() / 96 + 1, mstep = f.size() / 256 + 1;
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
