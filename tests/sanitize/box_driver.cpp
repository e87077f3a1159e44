// box_driver.cpp -- aeon_box_extract (aeon_amd/csrc/box_host.cpp) over metadata files, for the
// AddressSanitizer + UndefinedBehaviorSanitizer build `make -C aeon_amd/csrc sanitize_boxes`.
//   box_driver <class names JSON> <file>...
// Per file one line: "<path>\tok <width>x<height>x<depth> boxes <n> sum <sum of coordinates> labels <...>"
// or "<path>\terror <code> <message>".  Each file is read into a heap buffer of its exact size (so a read
// past the end is a sanitizer report) and extracted twice: with room for 4 boxes and with room for all.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: box_driver <class names JSON> <file>...\n");
        return 2;
    }
    for (int a = 2; a < argc; a++) {
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
        int     w = 0, h = 0, d = 0, n = 0;
        float   small_boxes[16];
        int32_t small_labels[4], small_difficult[4];
        int     rc = aeon_box_extract(argv[1], data, (size_t)size, &w, &h, &d, small_boxes, small_labels,
                                      small_difficult, 4, &n);
        if (rc == 0) {
            std::vector<float>   boxes(4 * (size_t)n + 1);
            std::vector<int32_t> labels((size_t)n + 1), difficult((size_t)n + 1);
            int                  n2 = 0;
            rc = aeon_box_extract(argv[1], data, (size_t)size, &w, &h, &d, boxes.data(), labels.data(), difficult.data(),
                                  n, &n2);
            if (rc == 0 && n2 != n) rc = -100;
            if (rc == 0 && std::memcmp(boxes.data(), small_boxes, sizeof(float) * 4 * (size_t)(n < 4 ? n : 4)) != 0) rc = -101;
            if (rc == 0) {
                double      sum = 0;
                std::string ls;
                for (int i = 0; i < 4 * n; i++) sum += boxes[(size_t)i];
                for (int i = 0; i < n && i < 8; i++) ls += (i ? "," : "") + std::to_string(labels[(size_t)i]);
                std::printf("%s\tok %dx%dx%d boxes %d sum %.3f labels %s\n", argv[a], w, h, d, n, sum, ls.c_str());
            }
        }
        if (rc != 0) std::printf("%s\terror %d %s\n", argv[a], rc, aeon_box_last_error());
        std::free(data);
    }
    return 0;
}
