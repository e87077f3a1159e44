// avi_driver.cpp -- aeon_avi_frames (aeon_amd/csrc/avi_host.cpp) over AVI files, and aeon_jpeg_info over
// every non-empty frame it returns, for the AddressSanitizer + UndefinedBehaviorSanitizer build
// `make -C aeon_amd/csrc sanitize_video`.
//   avi_driver <file>...
// Per file one line: "<path>\tok <width>x<height> frames <n> sizes <s0,s1,...> jpeg <w>x<h>x<components> bad <k>"
// (jpeg: the first frame's header; bad: kept frames whose header aeon_jpeg_info refuses) or
// "<path>\terror <code> <message>".  Each file is read into a heap buffer of its exact size (so a read past
// the end is a sanitizer report) and demuxed twice: with room for 2 frames and with room for all.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: avi_driver <file>...\n");
        return 2;
    }
    for (int a = 1; a < argc; a++) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) {
            std::printf("%s\terror io\n", argv[a]);
            continue;
        }
        std::fseek(f, 0, SEEK_END);
        const long size = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        char* data = size > 0 ? (char*)std::malloc((size_t)size) : nullptr;
        if (size > 0 && std::fread(data, 1, (size_t)size, f) != (size_t)size) {
            std::printf("%s\terror io\n", argv[a]);
            std::fclose(f);
            std::free(data);
            continue;
        }
        std::fclose(f);
        aeon_avi_frame two[2];
        int            n = 0, w = 0, h = 0;
        int            rc = aeon_avi_frames(data, (size_t)size, two, 2, &n, &w, &h);
        if (rc == 0) {
            std::vector<aeon_avi_frame> frames((size_t)n + 1);
            int                         n2 = 0;
            rc = aeon_avi_frames(data, (size_t)size, frames.data(), n, &n2, &w, &h);
            if (rc == 0 && n2 != n) rc = -100;
            if (rc == 0 && std::memcmp(frames.data(), two, sizeof(aeon_avi_frame) * (size_t)(n < 2 ? n : 2)) != 0) rc = -101;
            if (rc == 0) {
                std::string sizes;
                int         jw = 0, jh = 0, jc = 0, bad = 0;
                for (int i = 0; i < n; i++) {
                    const aeon_avi_frame& fr = frames[(size_t)i];
                    if (i < 16) sizes += (i ? "," : "") + std::to_string(fr.size);
                    if (fr.offset > (uint64_t)size || (uint64_t)size - fr.offset < fr.size) rc = -102; // inside the datum
                    if (rc != 0 || fr.size == 0) continue;
                    int fw = 0, fh = 0, fc = 0;
                    if (aeon_jpeg_info(data + fr.offset, fr.size, &fw, &fh, &fc) != 0) bad++;
                    else if (i == 0) jw = fw, jh = fh, jc = fc;
                }
                if (rc == 0)
                    std::printf("%s\tok %dx%d frames %d sizes %s jpeg %dx%dx%d bad %d\n", argv[a], w, h, n, sizes.c_str(), jw, jh,
                                jc, bad);
                else
                    std::printf("%s\terror %d frame outside the datum\n", argv[a], rc);
            } else if (rc <= -100) {
                std::printf("%s\terror %d demux calls disagree\n", argv[a], rc);
                rc = 0;
            }
        }
        if (rc != 0 && rc > -100) std::printf("%s\terror %d %s\n", argv[a], rc, aeon_avi_last_error());
        std::free(data);
    }
    return 0;
}
