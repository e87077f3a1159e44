// pixmap_stage_main.cpp -- the pixmap decoder (aeon_decode_pixmap), the stage's host half (aeon_pixmap_host_stage)
// and its kernel's code run on the host (aeon_pixmap_gpu_emulate: pixmap_rows.hpp, what pixmap_convert compiles)
// under AddressSanitizer + UndefinedBehaviorSanitizer (Makefile target sanitize_pixmap; tests/test_pixmap_stage.py
// runs it).  No device, no preload.  Arguments: BMP / PNM files.  Each file, its truncation at every header byte
// (and at steps through the pixel data) and 64 single-byte mutations of it go through the three entries in the
// three modes.  Whatever the emulation decodes, aeon_decode_pixmap must decode to the same bytes; the host half
// must refuse exactly what the decoder refuses, with a code of the C ABI.  One line per input with its outcome,
// then a count; exit status 1 at the first disagreement.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"

namespace {

long g_runs = 0, g_decoded = 0, g_refused = 0;

// outcome letters per mode: D decoded on the device route, H decoded on the host route, r refused, - too large to run
bool run(const std::vector<uint8_t>& f, const std::string& what)
{
    int  w = 0, h = 0, depth = 0, cn = 0, format = 0;
    char out[4] = "???";
    const bool info = aeon_pixmap_info(f.data(), f.size(), &w, &h, &depth, &cn, &format) == 0;
    for (int mode = AEON_DECODE_BGR8; mode <= AEON_DECODE_ANYDEPTH; mode++) {
        g_runs++;
        if (info && (size_t)w * h > (1u << 22)) { // (a mutated header asking for memory: the parse is what ran)
            out[mode] = '-';
            continue;
        }
        int     route = -1;
        int64_t staged = 0;
        const int rs = aeon_pixmap_host_stage(f.data(), f.size(), mode, &route, &staged);
        if (rs != 0 && rs != AEON_HIP_EINVAL && rs != AEON_HIP_EUNSUPPORTED) {
            std::printf("%s mode %d: host stage returned %d (%s)\n", what.c_str(), mode, rs, aeon_hip_last_error());
            return false;
        }
        if (!info) { // (the info entry is header only: it may pass where the pixel data falls short, never the reverse)
            if (rs == 0) {
                std::printf("%s mode %d: the header is refused, the host stage is not\n", what.c_str(), mode);
                return false;
            }
            out[mode] = 'r', g_refused++;
            continue;
        }
        const size_t eb = (mode == AEON_DECODE_ANYDEPTH && depth == 16) ? 2 : 1;
        const size_t stride = (size_t)w * (mode == AEON_DECODE_BGR8 ? 3 : 1) * eb + 3; // (unaligned rows)
        std::vector<uint8_t> a(stride * h, 0xA5), b(stride * h, 0xA5);
        const int rd = aeon_decode_pixmap(f.data(), f.size(), mode, b.data(), stride, nullptr);
        const int re = aeon_pixmap_gpu_emulate(f.data(), f.size(), mode, a.data(), stride);
        if (rd != rs) {
            std::printf("%s mode %d: decoder %d, host stage %d\n", what.c_str(), mode, rd, rs);
            return false;
        }
        if (rd != 0) {
            // (an ASCII file is not the emulation's: it says so without reading the samples)
            if (re != rd && !(format >= 1 && format <= 3 && re == AEON_HIP_EUNSUPPORTED)) {
                std::printf("%s mode %d: decoder %d, emulation %d\n", what.c_str(), mode, rd, re);
                return false;
            }
            out[mode] = 'r', g_refused++;
            continue;
        }
        g_decoded++;
        if (route == 1 ? (re != 0 || a != b || staged != (int64_t)f.size()) : re != AEON_HIP_EUNSUPPORTED) {
            std::printf("%s mode %d: route %d, emulation %d, equal %d, staged %ld\n", what.c_str(), mode, route, re,
                        (int)(a == b), (long)staged);
            return false;
        }
        out[mode] = route == 1 ? 'D' : 'H';
    }
    std::printf("%s: %s\n", what.c_str(), out);
    return true;
}

// where the header ends: the pixel data's offset for a BMP (its bfOffBits, if sane), else the first 64 bytes
size_t header_bytes(const std::vector<uint8_t>& f)
{
    if (f.size() >= 14 && f[0] == 'B') {
        const size_t off = (size_t)f[10] | (size_t)f[11] << 8 | (size_t)f[12] << 16 | (size_t)f[13] << 24;
        if (off <= f.size()) return off;
    }
    return f.size() < 64 ? f.size() : 64;
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
        std::string name = argv[i];
        name             = name.substr(name.find_last_of('/') + 1);
        if (!run(f, name)) return 1;
        const size_t hb = header_bytes(f), tstep = (f.size() - hb) / 16 + 1;
        for (size_t n = 1; n < f.size(); n += n < hb ? 1 : tstep)
            if (!run(std::vector<uint8_t>(f.begin(), f.begin() + n), name + " cut at " + std::to_string(n))) return 1;
        // 64 single-byte mutations: the header's bytes first, the rest spread over the file
        for (int k = 0; k < 64; k++) {
            static const uint8_t flips[4] = {0x01, 0x80, 0xFF, 0x10};
            const size_t at = (size_t)k < hb && k < 48 ? (size_t)k : hb + (f.size() - hb) * (size_t)(k % 16) / 16;
            std::vector<uint8_t> m = f;
            m[at % f.size()] ^= flips[(k + k / 16) % 4];
            if (!run(m, name + " mutation " + std::to_string(k) + " at byte " + std::to_string(at % f.size()))) return 1;
        }
    }
    std::printf("%d files, %ld runs: %ld decoded, %ld refused\n", files, g_runs, g_decoded, g_refused);
    return 0;
}
