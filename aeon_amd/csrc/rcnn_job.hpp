// rcnn_job.hpp -- what the host (targets.cpp, host.cpp) and the device (rcnn_kernels.hip) share about one
// localization_rcnn targets launch: the limits, what fills the per-record extension of the box table
// (box_job.hpp's RcnnRec) and the launch description.
//
// Limits (a config or record beyond them is AEON_HIP_EUNSUPPORTED, never a wrong answer).  The kernel
// keeps a record's state in LDS: three bits per anchor (foreground, background, sampled) and a running
// count per 64 anchors, the transformed gt boxes, and the sampled ranks.
//   total_anchors   <= kRcnnMaxAnchors (65 536; aeon's 1000 x 1000 default has 34 596)
//   boxes per record <= kRcnnMaxBoxes   (1024, before the crop drops any)
//   rois_per_image  <= kRcnnMaxRois    (1024; aeon's default is 256)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "box_job.hpp"
#include "rcnn_shuffle.hpp"

namespace aeon_hip {

constexpr int kRcnnMaxAnchors = 65536;
constexpr int kRcnnMaxBoxes   = 1024;
constexpr int kRcnnMaxRois    = 1024;

// host: transformer::transform's first lines for one record
int   unbiased_round(float x);                         // param_factory.cpp
float calculate_scale(int w, int h, int ow, int oh);   // param_factory.cpp
inline RcnnRec rcnn_rec(const aeon_aug_params& p, float fixed_scaling_factor, int width, int height, uint32_t engine)
{
    engine = rcnn_engine_word(engine);
    const float im_scale = fixed_scaling_factor > 0 ? fixed_scaling_factor : calculate_scale(p.crop_w, p.crop_h, width, height);
    return RcnnRec{im_scale, unbiased_round(p.crop_w * im_scale), unbiased_round(p.crop_h * im_scale), engine};
}

struct RcnnLaunch {
    BoxTableDev    t;          // with the extension
    const float*   anchors;    // 16-byte aligned, 4 floats per anchor (anchor::generate, uploaded once)
    uint32_t*      states_out; // n engine states after the shuffles, or null
    int32_t        n, total_anchors, max_gt_boxes, emit_type;
    float          emit_min_overlap;
    float          negative_overlap, positive_overlap;
    int32_t        rois_per_image, num_fg, shuffle;
    // bbtargets, bbtargets_mask, labels_flat, labels_mask, image_shape, gt_boxes, gt_box_count,
    // gt_class_count, image_scale, difficult_flag
    uint8_t*       buf[10];
    uint64_t       stride[10];
};

} // namespace aeon_hip
