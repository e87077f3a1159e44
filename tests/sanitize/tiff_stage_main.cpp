// tiff_stage_main.cpp -- the TIFF decoder (aeon_decode_tiff), the stage's host half (aeon_tiff_host_stage) and its
// kernels' code run on the host (aeon_tiff_gpu_emulate: tiff_strips.hpp, what tiff_expand and tiff_convert compile)
// under AddressSanitizer + UndefinedBehaviorSanitizer (Makefile target sanitize_tiff; tests/test_tiff_stage.py runs
// it).  No device, no preload.  Arguments: TIFF files.  Each file, its truncation at every byte of its header and
// IFD (and at steps through the rest) and 64 single-byte mutations of it go through the three entries in the
// three modes.  Whatever the emulation decodes, aeon_decode_tiff must decode to the same bytes; what the decoder
// refuses for its strip data the emulation reports as a device error; the host half must refuse exactly what the
// header parse refuses.  One line per input with its outcome, then a count; exit status 1 at the first disagreement.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"

namespace {

long g_runs = 0, g_decoded = 0, g_refused = 0, g_corrupt = 0;

// outcome letters per mode: D decoded on the device route, H decoded on the host route, r refused from the header,
// c strip data corrupt (decoder: invalid; emulation: device error), - too large to run
bool run(const std::vector<uint8_t>& f, const std::string& what)
{
    int  w = 0, h = 0, cn = 0, eb2 = 0;
    char out[4] = "???";
    const bool info = aeon_tiff_info(f.data(), f.size(), &w, &h, &cn, &eb2) == 0;
    for (int mode = AEON_DECODE_BGR8; mode <= AEON_DECODE_ANYDEPTH; mode++) {
        g_runs++;
        if (info && (size_t)w * h > (1u << 22)) { // (a mutated header asking for memory: the parse is what ran)
            out[mode] = '-';
            continue;
        }
        int     route = -1;
        int64_t staged = 0;
        const int rs = aeon_tiff_host_stage(f.data(), f.size(), mode, &route, &staged);
        if (rs != 0 && rs != AEON_HIP_EINVAL && rs != AEON_HIP_EUNSUPPORTED) {
            std::printf("%s mode %d: host stage returned %d (%s)\n", what.c_str(), mode, rs, aeon_hip_last_error());
            return false;
        }
        if (!info) {
            if (rs == 0) {
                std::printf("%s mode %d: the header is refused, the host stage is not\n", what.c_str(), mode);
                return false;
            }
            out[mode] = 'r', g_refused++;
            continue;
        }
        const size_t eb = mode == AEON_DECODE_ANYDEPTH ? (size_t)eb2 : 1;
        const size_t stride = (size_t)w * (mode == AEON_DECODE_BGR8 ? 3 : 1) * eb + 3; // (unaligned rows)
        std::vector<uint8_t> a(stride * h, 0xA5), b(stride * h, 0xA5);
        const int rd = aeon_decode_tiff(f.data(), f.size(), mode, b.data(), stride, nullptr);
        const int re = aeon_tiff_gpu_emulate(f.data(), f.size(), mode, a.data(), stride);
        if (rs != 0) { // (a host-routed file with corrupt strips: the host half decodes it, and refuses as the decoder does)
            if (rd != rs) {
                std::printf("%s mode %d: decoder %d, host stage %d\n", what.c_str(), mode, rd, rs);
                return false;
            }
            out[mode] = 'c', g_corrupt++;
            continue;
        }
        if (route == 0) {
            if (rd != 0 || re != AEON_HIP_EUNSUPPORTED) {
                std::printf("%s mode %d: host route, decoder %d, emulation %d\n", what.c_str(), mode, rd, re);
                return false;
            }
            out[mode] = 'H', g_decoded++;
            continue;
        }
        // the device route: the decoder and the emulation accept the same strips
        if ((rd == 0) != (re == 0) || (rd != 0 && (rd != AEON_HIP_EINVAL || re != AEON_HIP_EDEVICE)) || staged != (int64_t)f.size()) {
            std::printf("%s mode %d: decoder %d, emulation %d, staged %ld (%s)\n", what.c_str(), mode, rd, re, (long)staged,
                        aeon_hip_last_error());
            return false;
        }
        if (rd != 0) {
            out[mode] = 'c', g_corrupt++;
            continue;
        }
        if (a != b) {
            std::printf("%s mode %d: the emulation's record differs from the decoder's\n", what.c_str(), mode);
            return false;
        }
        out[mode] = 'D', g_decoded++;
    }
    std::printf("%s: %s\n", what.c_str(), out);
    return true;
}

// where the header, the IFD and its out-of-line values lie: the writer's and Pillow's files keep them in one piece,
// from the IFD to the end of the file or from the header to the first strip
void ifd_range(const std::vector<uint8_t>& f, size_t* from, size_t* to)
{
    *from = 0, *to = f.size() < 8 ? f.size() : 8;
    if (f.size() < 8) return;
    const bool big = f[0] == 'M';
    const size_t ifd = big ? ((size_t)f[4] << 24 | (size_t)f[5] << 16 | (size_t)f[6] << 8 | f[7])
                           : ((size_t)f[7] << 24 | (size_t)f[6] << 16 | (size_t)f[5] << 8 | f[4]);
    if (ifd >= f.size()) return;
    *from = ifd > 64 ? ifd - 64 : 0;
    *to   = ifd + 400 < f.size() ? ifd + 400 : f.size();
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
        size_t from, to;
        ifd_range(f, &from, &to);
        const size_t tstep = f.size() / 24 + 1;
        for (size_t n = 1; n < f.size(); n += (n < 8 || (n >= from && n < to)) ? 1 : tstep)
            if (!run(std::vector<uint8_t>(f.begin(), f.begin() + n), name + " cut at " + std::to_string(n))) return 1;
        // 64 single-byte mutations: the header and the IFD's bytes first, the rest spread over the file
        for (int k = 0; k < 64; k++) {
            static const uint8_t flips[4] = {0x01, 0x80, 0xFF, 0x10};
            const size_t ifd0 = from + (from ? 64 : 0);
            const size_t at = k < 8 ? (size_t)k : k < 40 ? ifd0 + (size_t)(k - 8) * 5 : f.size() * (size_t)(k - 40) / 24;
            std::vector<uint8_t> m = f;
            m[at % f.size()] ^= flips[(k + k / 16) % 4];
            if (!run(m, name + " mutation " + std::to_string(k) + " at byte " + std::to_string(at % f.size()))) return 1;
        }
    }
    std::printf("%d files, %ld runs: %ld decoded, %ld refused, %ld corrupt\n", files, g_runs, g_decoded, g_refused, g_corrupt);
    return 0;
}
