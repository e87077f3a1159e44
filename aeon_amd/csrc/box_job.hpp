// box_job.hpp -- the device table of one aeon_hip_box_targets_batch call (stage.cpp writes it,
// box_kernels.hip reads it): n BoxRec, then the call's boxes (float4 each), labels and difficult flags.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/aeon_hip.h"

namespace aeon_hip {

// One record: where its boxes lie in the box table, and the fields of its augment::image::params
// that boundingbox::transformer::transform_box reads (etl_boundingbox.cpp:174-261).
struct BoxRec {
    uint32_t first;
    int32_t  count;
    int32_t  crop_x, crop_y, crop_w, crop_h;
    int32_t  out_w, out_h; // params.output_size: the rescale's numerators
    int32_t  flip;
    int32_t  expand;       // expand_ratio > 1
    int32_t  expand_x, expand_y;
};
static_assert(sizeof(BoxRec) == 48, "BoxRec is read as three 16-byte loads");

// table layout: BoxRec[n] padded to 16 bytes, float[4 * total], int32[total] labels, int32[total] difficult
inline size_t box_rec_bytes(int n) { return ((size_t)n * sizeof(BoxRec) + 15) & ~(size_t)15; }
inline size_t box_table_bytes(int n, size_t total) { return box_rec_bytes(n) + total * 24; }

inline BoxRec box_rec(uint32_t first, int32_t count, const aeon_aug_params& p)
{
    return BoxRec{first, count, p.crop_x, p.crop_y, p.crop_w, p.crop_h, p.out_w, p.out_h,
                  p.flip ? 1 : 0, p.expand_ratio > 1. ? 1 : 0, p.expand_x, p.expand_y};
}

// What the box transform refuses for one record (null = accepted): rotation -- aeon's transformer
// returns a null pointer there, which its loader dereferences (etl_boundingbox.cpp:281-284) --, an
// empty cropbox, and boundingbox::box::expand's precondition (boundingbox.cpp:92-102).
inline const char* box_refusal(const aeon_aug_params& p, const float* boxes, int count)
{
    if (p.angle != 0) return "boundingbox transform does not support rotation (angle != 0)";
    if (p.crop_w <= 0 || p.crop_h <= 0) return "empty cropbox";
    if (p.expand_ratio > 1.)
        for (int k = 0; k < count; k++) {
            const float* b = boxes + 4 * (size_t)k;
            if (b[2] + p.expand_x > p.expand_w || b[3] + p.expand_y > p.expand_h)
                return "Invalid parameters to expand boundingbox";
        }
    return nullptr;
}

struct BoxLaunch {
    const BoxRec*  recs;
    const float*   boxes; // 16-byte aligned, 4 floats per box
    const int32_t* labels;
    const int32_t* difficult;
    int32_t        n, kind, max_boxes, emit_type;
    float          emit_min_overlap;
    float          norm_w, norm_h; // SSD: config width / height
    int32_t        shape_w, shape_h;
    uint8_t*       buf[5];
    uint64_t       stride[5];
};

} // namespace aeon_hip
