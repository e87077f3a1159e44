// box_job.hpp -- the device table of one box targets call (aeon_hip_box_targets_batch, aeon_hip_rcnn_targets_batch
// or a decode window's box provider; targets.cpp and host.cpp write it, box_kernels.hip and rcnn_kernels.hip
// read it) and the box kernel's launch description.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

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

// Per record of a localization_rcnn table, next to its BoxRec: transformer::transform's image scale and
// scaled image size (etl_localization_rcnn.cpp:101-118), and the minstd_rand0 state its shuffles start from
// (rcnn_job.hpp's rcnn_rec fills it).
struct RcnnRec {
    float    im_scale;
    int32_t  im_w, im_h;
    uint32_t engine;
};
static_assert(sizeof(RcnnRec) == 16, "RcnnRec is read as one 16-byte load");

// The table of n records with `total` boxes between them: BoxRec[n] padded to 16 bytes, float[4 * total] boxes,
// int32[total] labels, int32[total] difficult flags and, for localization_rcnn, RcnnRec[n] after padding to 16
// bytes.  Byte offsets of the parts, and the table's size.
struct BoxTableLayout {
    size_t boxes, labels, difficult, ext, bytes;
};
inline BoxTableLayout box_table_layout(int n, size_t total, bool rcnn)
{
    BoxTableLayout l{};
    l.boxes     = ((size_t)n * sizeof(BoxRec) + 15) & ~(size_t)15;
    l.labels    = l.boxes + total * 16;
    l.difficult = l.labels + total * 4;
    l.ext = l.bytes = l.difficult + total * 4;
    if (rcnn) {
        l.ext   = (l.bytes + 15) & ~(size_t)15;
        l.bytes = l.ext + (size_t)n * sizeof(RcnnRec);
    }
    return l;
}
inline size_t box_table_bytes(int n, size_t total, bool rcnn) { return box_table_layout(n, total, rcnn).bytes; }

// The parts of a table at `base` (16-byte aligned).  Byte = uint8_t: the pinned table the host writes;
// const uint8_t: the device table a launch reads.
template <typename Byte>
struct BoxTable {
    template <typename T>
    using part = typename std::conditional<std::is_const<Byte>::value, const T, T>::type*;
    part<BoxRec>  recs;
    part<float>   boxes; // 16-byte aligned, 4 floats per box
    part<int32_t> labels, difficult;
    part<RcnnRec> ext; // null without the extension
    size_t        bytes;

    BoxTable() = default;
    BoxTable(Byte* base, int n, size_t total, bool rcnn)
    {
        const BoxTableLayout l = box_table_layout(n, total, rcnn);
        recs      = (part<BoxRec>)base;
        boxes     = (part<float>)(base + l.boxes);
        labels    = (part<int32_t>)(base + l.labels);
        difficult = (part<int32_t>)(base + l.difficult);
        ext       = rcnn ? (part<RcnnRec>)(base + l.ext) : nullptr;
        bytes     = l.bytes;
    }
};
using BoxTableHost = BoxTable<uint8_t>;
using BoxTableDev  = BoxTable<const uint8_t>;

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
    BoxTableDev    t;
    int32_t        n, kind, max_boxes, emit_type;
    float          emit_min_overlap;
    float          norm_w, norm_h; // SSD: config width / height
    int32_t        shape_w, shape_h;
    uint8_t*       buf[5];
    uint64_t       stride[5];
};

} // namespace aeon_hip
