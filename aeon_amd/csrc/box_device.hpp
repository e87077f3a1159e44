// box_device.hpp -- boundingbox::transformer::transform_box (src/etl_boundingbox.cpp:146-261) for one box on
// the device and a wave's loop over a record's boxes, shared by the box kernels (box_kernels.hip) and the
// localization_rcnn targets (rcnn_kernels.hip).  Float32, every operation rounded once and in aeon's order: the including file is
// built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aeon_hip.h"
#include "box_job.hpp"

namespace aeon_hip {

// box::size (box.hpp:58-69): inclusive, 0 when inverted
__device__ inline float box_size(float xmin, float ymin, float xmax, float ymax)
{
    if (xmax < xmin || ymax < ymin) return 0.0f;
    const float w = xmax - xmin + 1.0f;
    const float h = ymax - ymin + 1.0f;
    return w * h;
}

// transform_box for one box; false = dropped
__device__ inline bool transform_box(const BoxRec& r, int emit_type, float emit_min_overlap, float4& b)
{
    float xmin = b.x, ymin = b.y, xmax = b.z, ymax = b.w;
    if (r.expand) { // box::expand -> operator+(cv::Point)
        xmin = xmin + (float)r.expand_x;
        ymin = ymin + (float)r.expand_y;
        xmax = xmax + (float)r.expand_x;
        ymax = ymax + (float)r.expand_y;
    }
    if (emit_type != AEON_EMIT_NONE) { // meet_emit_constraint
        const float cx0 = (float)r.crop_x, cy0 = (float)r.crop_y;
        const float cx1 = (float)(r.crop_x + r.crop_w - 1), cy1 = (float)(r.crop_y + r.crop_h - 1);
        if (emit_type == AEON_EMIT_CENTER) {
            // box::xcenter (box.hpp:92): the float difference, halved and added in double, narrowed
            const float xc = (float)((double)xmin + (double)(xmax - xmin) / 2.);
            const float yc = (float)((double)ymin + (double)(ymax - ymin) / 2.);
            if (!(xc >= cx0 && xc <= cx1 && yc >= cy0 && yc <= cy1)) return false;
        } else { // input_bbox.coverage(crop_bbox) >= emit_min_overlap
            float isz = 0.0f;
            if (!(cx0 > xmax || cx1 < xmin || cy0 > ymax || cy1 < ymin)) {
                const float ix0 = xmin < cx0 ? cx0 : xmin, iy0 = ymin < cy0 ? cy0 : ymin; // std::max(a, b)
                const float ix1 = cx1 < xmax ? cx1 : xmax, iy1 = cy1 < ymax ? cy1 : ymax; // std::min(a, b)
                isz = box_size(ix0, iy0, ix1, iy1);
            }
            float coverage = 0.0f;
            if (isz > 0) coverage = isz / box_size(xmin, ymin, xmax, ymax);
            if (!(coverage >= emit_min_overlap)) return false;
        }
    }
    const float cx = (float)r.crop_x, cy = (float)r.crop_y;
    const float cxe = (float)(r.crop_x + r.crop_w), cye = (float)(r.crop_y + r.crop_h);
    const float cw = (float)r.crop_w, ch = (float)r.crop_h;
    if (xmax < cx || xmin >= cxe || ymax < cy || ymin >= cye) return false;
    xmin = xmin < cx ? 0.0f : xmin - cx;
    ymin = ymin < cy ? 0.0f : ymin - cy;
    xmax = xmax >= cxe ? (float)(r.crop_w - 1) : xmax - cx;
    ymax = ymax >= cye ? (float)(r.crop_h - 1) : ymax - cy;
    if (r.flip) {
        const float old_xmax = xmax;
        xmax = cw - xmin - 1.0f;
        xmin = cw - old_xmax - 1.0f;
    }
    const float xs = (float)r.out_w / cw;
    const float ys = (float)r.out_h / ch;
    b.x = xmin * xs;
    b.y = ymin * ys;
    b.z = (xmax + 1.0f) * xs - 1.0f;
    b.w = (ymax + 1.0f) * ys - 1.0f;
    return true;
}

// One wave (every lane calls this) over `count` boxes of record r, 64 at a time: each lane transforms its
// box, and the kept ones are numbered in input order with a ballot and the popcount of the lower lanes on top
// of a wave-uniform running count.  The lane of kept box i calls store(slot, i, b), whatever the slot; the
// slots from the kept count up to max_out get pad(slot).  Returns the number of boxes kept (wave-uniform).
template <typename Store, typename Pad>
__device__ __forceinline__ int compact_boxes(const BoxRec& r, const float4* boxes, int count, int emit_type,
                                             float emit_min_overlap, int max_out, int lane, Store store, Pad pad)
{
    int kept = 0;
    for (int base = 0; base < count; base += 64) {
        const int i    = base + lane;
        bool      keep = false;
        float4    b    = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < count) {
            b    = boxes[i];
            keep = transform_box(r, emit_type, emit_min_overlap, b);
        }
        const unsigned long long mask = __ballot(keep);
        const int slot = kept + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep) store(slot, i, b);
        kept += __popcll(mask);
    }
    for (int s = (kept < max_out ? kept : max_out) + lane; s < max_out; s += 64) pad(s);
    return kept;
}

} // namespace aeon_hip
