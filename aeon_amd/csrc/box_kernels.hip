// box_kernels.hip -- boundingbox / localization_ssd targets of a decode window in one launch.
//
// aeon transforms a record's object boxes with the params that cropped, expanded and flipped its
// image (boundingbox::transformer::transform_box, src/etl_boundingbox.cpp:146-261, with
// boundingbox::box::expand / rescale / coverage / normalize, src/boundingbox.cpp:78-163, box.hpp:51-93)
// and loads the survivors, in input order, into zero-padded fixed-size items:
//   provider::boundingbox        loader (etl_boundingbox.cpp:296-318): max_bbox_count x 4 floats
//   provider::localization::ssd  loader (etl_localization_ssd.cpp:116-150): image_shape, gt_boxes
//                                (normalized), gt_box_count, gt_class_count, difficult_flag
// One wave (64 lanes) per record, four records per 256-thread workgroup, no LDS: lanes take the
// record's boxes 64 at a time, each decides keep / drop, and the kept ones are compacted in order with
// a ballot and the popcount of the lower lanes on top of a wave-uniform running count.  Slots past
// max_boxes are not written (aeon's min(max, size)); the rest of every item is zero-filled.
//
// Arithmetic: float32, every operation rounded once and in aeon's order (-ffp-contract=off; the
// divisions are the correctly rounded ones), so the outputs equal aeon's bit for bit.  aeon's range
// check in normalized_box::box's constructor (normalized_box.cpp:90-107: a coordinate outside [0, 1]
// throws) is NOT reproduced: the normalized values are written as computed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aeon_hip.h"
#include "box_device.hpp"
#include "box_job.hpp"
#include "launch.hpp"

namespace aeon_hip {

namespace {

__global__ __launch_bounds__(256) void box_targets(BoxLaunch L)
{
    const int lane = threadIdx.x & 63;
    const int rec  = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rec >= L.n) return; // the whole wave leaves: no barrier anywhere below
    const BoxRec   r   = L.t.recs[rec];
    const int32_t* lab = L.t.labels + r.first;
    const int32_t* dif = L.t.difficult + r.first;
    const bool     ssd = L.kind == AEON_BOX_SSD;
    const int      bi  = ssd ? 1 : 0; // the boxes' buffer
    float4*  out_box = (float4*)(L.buf[bi] + (uint64_t)rec * L.stride[bi]);
    int32_t* out_cls = ssd ? (int32_t*)(L.buf[3] + (uint64_t)rec * L.stride[3]) : nullptr;
    int32_t* out_dif = ssd ? (int32_t*)(L.buf[4] + (uint64_t)rec * L.stride[4]) : nullptr;

    const int kept = compact_boxes(
        r, (const float4*)L.t.boxes + r.first, r.count, L.emit_type, L.emit_min_overlap, L.max_boxes, lane,
        [&](int slot, int i, float4 b) {
            if (slot >= L.max_boxes) return;
            if (ssd) { // bbox::normalize (boundingbox.cpp:150-156)
                b.x = b.x / L.norm_w;
                b.y = b.y / L.norm_h;
                b.z = (b.z + 1.0f) / L.norm_w;
                b.w = (b.w + 1.0f) / L.norm_h;
                out_cls[slot] = lab[i];
                out_dif[slot] = dif[i] != 0 ? 1 : 0;
            }
            out_box[slot] = b;
        },
        [&](int s) {
            out_box[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ssd) out_cls[s] = 0, out_dif[s] = 0;
        });
    if (ssd) {
        if (lane == 0) {
            int32_t* shape = (int32_t*)(L.buf[0] + (uint64_t)rec * L.stride[0]);
            shape[0] = L.shape_w;
            shape[1] = L.shape_h;
            *(int32_t*)(L.buf[2] + (uint64_t)rec * L.stride[2]) = kept < L.max_boxes ? kept : L.max_boxes;
        }
    } else {
        // aeon's item is max_bbox_count x 16 elements of output_type, of which the loader writes the
        // first max_bbox_count x 4 floats: the rest is zeroed here (16 bytes per lane and step)
        const int n16 = (int)(L.stride[0] / 16);
        for (int s = L.max_boxes + lane; s < n16; s += 64) out_box[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

} // namespace

hipError_t launch_box_targets(const BoxLaunch& L, hipStream_t stream)
{
    if (L.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(box_targets, dim3((unsigned)((L.n + 3) / 4)), dim3(256), 0, stream, L);
    return hipGetLastError();
}

} // namespace aeon_hip
