// rcnn_host.hpp -- localization::rcnn::config, anchor::generate and transformer::sample_anchors
// (src/etl_localization_rcnn.{hpp,cpp}) on the host; no HIP dependency (tests/sanitize/rcnn_driver.cpp
// links rcnn_host.cpp alone).
#pragma once
#include <cstddef>
#include <cstdint>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "json.hpp"

namespace aeon_hip {

// a configuration or record this build refuses (AEON_HIP_EUNSUPPORTED at the C ABI)
struct unsupported_error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// std::minstd_rand0 whose state word can be read back (an LCG's state is its last output); a seed
// congruent to 0 mod 2^31 - 1 becomes 1, as minstd_rand0::seed makes it
struct tracked_engine {
    using result_type = std::minstd_rand0::result_type;
    std::minstd_rand0 e;
    result_type       last;
    static constexpr result_type min() { return std::minstd_rand0::min(); }
    static constexpr result_type max() { return std::minstd_rand0::max(); }
    explicit tracked_engine(uint32_t s) : e(s), last(s % 2147483647u == 0 ? 1 : s % 2147483647u) {}
    result_type operator()() { return last = e(); }
};

// the state word of a minstd_rand0: one step of a copy, undone (16807 * 1407677000 = 1 mod 2^31 - 1)
inline uint32_t minstd_state(std::minstd_rand0 e) { return (uint32_t)((uint64_t)e() * 1407677000u % 2147483647u); }

// localization::rcnn::config (etl_localization_rcnn.hpp:98-146): defaults, ranges, unknown keys refused
// (std::invalid_argument).  aeon's validate() is empty; values aeon would take but this stage cannot
// launch with are std::invalid_argument where they give no anchors at all (sizes, base_size, ratios or
// scales that are not positive, an empty ratios / scales list, a scaling_factor that is not a positive
// finite number) and unsupported_error where only this build's arithmetic stops (width, height or
// max_gt_boxes above 2^24, a feature grid side above 2^24)
struct rcnn_config {
    int64_t                  rois_per_image = 256, height = 0, width = 0, base_size = 16, max_gt_boxes = 64;
    float                    scaling_factor = 1.0 / 16.;
    std::vector<float>       ratios{0.5f, 1.f, 2.f}, scales{8.f, 16.f, 32.f};
    float                    negative_overlap = 0.3, positive_overlap = 0.7, foreground_fraction = 0.5;
    std::vector<std::string> class_names;
    std::string              name;

    rcnn_config() = default;
    explicit rcnn_config(const Json& js);
    int64_t conv_w() const;
    int64_t conv_h() const;
    int64_t total_anchors() const; // ratios x scales x conv_h x conv_w
    // int(foreground_fraction * rois_per_image): a float product (sample_anchors)
    int num_fg() const { return int(foreground_fraction * rois_per_image); }
};

// anchor::generate (etl_localization_rcnn.cpp:430-554): total_anchors() x (xmin, ymin, xmax, ymax), base
// anchors outermost, then shift rows, then shift columns
std::vector<float> rcnn_generate_anchors(const rcnn_config& cfg);

// transformer::sample_anchors over labels[n] (>= 1 foreground, 0 background) with the real
// std::shuffle over std::minstd_rand0 started from *engine_state (left at the state after the two
// shuffles); shuffle == false is aeon's debug_deterministic.  Foreground indices first.
std::vector<int32_t> rcnn_sample_anchors(const int32_t* labels, size_t n, int rois_per_image, int num_fg, bool shuffle,
                                         uint32_t* engine_state);

} // namespace aeon_hip
