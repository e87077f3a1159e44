// rcnn_driver.cpp -- the host half of the localization_rcnn targets (aeon_amd/csrc/rcnn_host.cpp) and the
// shuffle header the device shares (aeon_amd/csrc/rcnn_shuffle.hpp, compiled here for the host), for the
// AddressSanitizer + UndefinedBehaviorSanitizer build `make -C aeon_amd/csrc sanitize_rcnn`.
//   rcnn_driver shuffle            rcnn_shuffle_prefix against std::shuffle over std::minstd_rand0: every n
//                                  from 0 to 300 and 46340, 46341, 60000 (either side of libstdc++'s switch
//                                  between its two forms), three seeds, the whole permutation, a prefix of
//                                  it and the engine's end state.  Prints "shuffle ok <cases>" or the
//                                  mismatches.  Then seven engine words, among them 0, 2^31 - 1 and 2^32 - 2,
//                                  against minstd_rand0::seed.
//   rcnn_driver config <json>...   per config: "ok <total_anchors> <num_fg> <first anchor> <last anchor>
//                                  <sum>" (anchors into a heap buffer of their exact size) or "error <code>
//                                  <message>"
//   rcnn_driver sample             aeon_rcnn_sample_anchors over label vectors in exact-size heap buffers,
//                                  checked against the list form of sample_anchors built here
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../aeon_amd/csrc/rcnn_host.hpp"
#include "../../aeon_amd/csrc/rcnn_shuffle.hpp"
#include "../../include/aeon_hip.h"

namespace {

using tracked = aeon_hip::tracked_engine;

int run_shuffle()
{
    std::vector<uint32_t> sizes;
    for (uint32_t n = 0; n <= 300; n++) sizes.push_back(n);
    for (uint32_t n : {46340u, 46341u, 60000u}) sizes.push_back(n);
    int cases = 0, bad = 0;
    for (uint32_t seed : {1u, 42u, 2147483646u})
        for (uint32_t n : sizes) {
            std::vector<int32_t> ref(n);
            std::iota(ref.begin(), ref.end(), 0);
            tracked g(seed);
            std::shuffle(ref.begin(), ref.end(), g);
            for (uint32_t keep : {n, std::min(n, 7u), 0u, n + 5}) {
                const uint32_t        m = std::min(n, keep);
                std::vector<int32_t>  out(m); // exact size: a write past the prefix is a sanitizer report
                aeon_hip::minstd0     h{seed};
                aeon_hip::rcnn_shuffle_prefix(n, keep, h, out.data());
                cases++;
                if (h.x != g.last || !std::equal(out.begin(), out.end(), ref.begin())) {
                    std::printf("mismatch seed %u n %u keep %u: state %u vs %u\n", seed, n, keep, h.x, (uint32_t)g.last);
                    bad++;
                }
            }
        }
    // engine words as minstd_rand0::seed takes them; a word congruent to 0 must not reach the engine as 0
    for (uint32_t word : {0u, 1u, 2147483646u, 2147483647u, 2147483648u, 4294967294u, 4294967295u}) {
        cases++;
        std::minstd_rand0 ref(word);
        aeon_hip::minstd0 h{aeon_hip::rcnn_engine_word(word)};
        if (h.x != tracked(word).last || h.x == 0 || h.next() != ref() || aeon_hip::minstd_state(ref) != h.x) {
            std::printf("mismatch engine word %u\n", word);
            bad++;
        }
    }
    if (!bad) std::printf("shuffle ok %d\n", cases);
    return bad ? 1 : 0;
}

int run_config(int argc, char** argv)
{
    for (int a = 2; a < argc; a++) {
        aeon_rcnn_info info{};
        int            n  = 0;
        int            rc = aeon_rcnn_config_info(argv[a], &info);
        if (rc == 0) rc = aeon_rcnn_anchors(argv[a], nullptr, 0, &n);
        if (rc != 0) {
            std::printf("error %d %s\n", rc, aeon_rcnn_last_error());
            continue;
        }
        std::vector<float> anchors(4 * (size_t)n);
        int                n2 = 0;
        rc = aeon_rcnn_anchors(argv[a], anchors.data(), n, &n2);
        if (rc != 0 || n2 != n || n != info.total_anchors) {
            std::printf("error %d inconsistent anchors\n", rc);
            continue;
        }
        double sum = 0;
        for (float v : anchors) sum += v;
        std::printf("ok %d %d (%g %g %g %g) (%g %g %g %g) %.3f\n", n, info.num_fg, anchors[0], anchors[1], anchors[2],
                    anchors[3], anchors[4 * (size_t)n - 4], anchors[4 * (size_t)n - 3], anchors[4 * (size_t)n - 2],
                    anchors[4 * (size_t)n - 1], sum);
    }
    return 0;
}

int run_sample()
{
    int bad = 0, cases = 0;
    for (int n : {0, 1, 5, 64, 300, 1000})
        for (int rois : {0, 4, 16, 256})
            for (int shuffle : {0, 1}) {
                std::vector<int32_t> labels((size_t)n);
                std::minstd_rand0    lg(7u + (uint32_t)n);
                for (auto& l : labels) l = (int32_t)(lg() % 4) - 1; // -1, 0, 1, 2
                const int            num_fg = rois / 2;
                std::vector<int32_t> fg, bg;
                for (int i = 0; i < n; i++) {
                    if (labels[(size_t)i] >= 1) fg.push_back(i);
                    else if (labels[(size_t)i] == 0) bg.push_back(i);
                }
                tracked g(99u);
                if (shuffle) {
                    std::shuffle(fg.begin(), fg.end(), g);
                    std::shuffle(bg.begin(), bg.end(), g);
                }
                if ((int)fg.size() > num_fg) fg.resize((size_t)num_fg);
                if ((int)bg.size() > rois - (int)fg.size()) bg.resize((size_t)(rois - (int)fg.size()));
                fg.insert(fg.end(), bg.begin(), bg.end());
                std::vector<int32_t> out((size_t)rois);
                uint32_t             state = 99u;
                int                  n_out = -1;
                const int rc = aeon_rcnn_sample_anchors(labels.data(), n, rois, num_fg, shuffle, &state, out.data(), &n_out);
                cases++;
                if (rc != 0 || n_out != (int)fg.size() || !std::equal(fg.begin(), fg.end(), out.begin()) ||
                    state != (uint32_t)g.last) {
                    std::printf("mismatch n %d rois %d shuffle %d rc %d\n", n, rois, shuffle, rc);
                    bad++;
                }
            }
    if (!bad) std::printf("sample ok %d\n", cases);
    return bad ? 1 : 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "shuffle")) return run_shuffle();
    if (argc >= 3 && !std::strcmp(argv[1], "config")) return run_config(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "sample")) return run_sample();
    std::fprintf(stderr, "usage: rcnn_driver shuffle | config <json>... | sample\n");
    return 2;
}
