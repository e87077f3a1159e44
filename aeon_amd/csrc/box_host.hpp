// box_host.hpp -- boundingbox::decoded (src/etl_boundingbox.hpp) as flat arrays, and its extractor.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace aeon_hip {

// one record's metadata: image size and its object boxes in file order
struct box_metadata {
    int                  width = 0, height = 0, depth = 0;
    std::vector<float>   boxes; // 4 per box: xmin, ymin, xmax, ymax (pixels, xmax / ymax inclusive)
    std::vector<int32_t> labels, difficult, truncated;
};

// boundingbox::config label_map: class name -> index
std::unordered_map<std::string, int> box_label_map(const std::vector<std::string>& class_names);
// boundingbox::extractor::extract; std::invalid_argument with aeon's texts
void box_extract(const std::unordered_map<std::string, int>& label_map, const void* data, size_t size,
                 box_metadata& out);

} // namespace aeon_hip
