// targets.cpp -- the boundingbox, localization_ssd and localization_rcnn target calls of the device half: a
// call's box table through a ring slot (or already staged in a decode window's arena: box_targets_staged,
// rcnn_targets_staged), read by one launch of box_kernels.hip / rcnn_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/aeon_hip.h"
#include "box_job.hpp"
#include "context.hpp"
#include "host.hpp"
#include "launch.hpp"
#include "rcnn_job.hpp"

using namespace aeon_hip;

namespace {

// ---- boundingbox / localization_ssd / localization_rcnn targets ---------------------------------
// One output buffer of a targets call: n items of `stride` bytes, of which the kernel writes `need`.
bool out_buf_ok(const void* buf, uint64_t stride, uint64_t need, uintptr_t align)
{
    return buf && !((uintptr_t)buf & (align - 1)) && !(stride & (align - 1)) && stride >= need;
}

void check_emit(int emit_type)
{
    if (emit_type < AEON_EMIT_NONE || emit_type > AEON_EMIT_MIN_OVERLAP) fail(AEON_HIP_EINVAL, "Invalid emit constraint type");
}

// The output side of a box call: every buffer holds n items of its stride, and the kernel writes exactly
// max_boxes * 16 (boxes; boundingbox: the whole item), 8 (image_shape), 4 (count) or max_boxes * 4 bytes.
void check_box_out(const aeon_box_out& o)
{
    if (o.kind != AEON_BOX_BOUNDINGBOX && o.kind != AEON_BOX_SSD) fail(AEON_HIP_EINVAL, "unknown box target kind");
    if (o.max_boxes <= 0) fail(AEON_HIP_EINVAL, o.kind == AEON_BOX_SSD ? "invalid max_gt_boxes" : "invalid max_bbox_count");
    check_emit(o.emit_type);
    const bool ssd = o.kind == AEON_BOX_SSD;
    if (ssd && (o.out_w <= 0 || o.out_h <= 0)) fail(AEON_HIP_EINVAL, "invalid width / height of the box config");
    const uint64_t box_bytes = (uint64_t)o.max_boxes * 16, cls_bytes = (uint64_t)o.max_boxes * 4;
    const int      bi        = ssd ? 1 : 0;
    if (!out_buf_ok(o.buf[bi], o.item_stride[bi], box_bytes, 16))
        fail(AEON_HIP_EINVAL, "box buffer: 16-byte aligned items of at least max_boxes*16 bytes");
    if (ssd) {
        const uint64_t need[5] = {8, 0, 4, cls_bytes, cls_bytes};
        for (int k : {0, 2, 3, 4})
            if (!out_buf_ok(o.buf[k], o.item_stride[k], need[k], 4))
                fail(AEON_HIP_EINVAL, "box buffers: 4-byte aligned int32 items of the output's size");
    }
}

// The output side of an rcnn call: ten buffers of n items; the kernel writes 4A floats (bbtargets,
// bbtargets_mask), 2A int32 (labels_flat, labels_mask), 8 bytes (image_shape), max_gt_boxes * 16
// (gt_boxes), max_gt_boxes * 4 (gt_class_count, difficult_flag) and 4 bytes (gt_box_count, image_scale).
void check_rcnn_out(const aeon_rcnn_out& o)
{
    if (o.total_anchors <= 0) fail(AEON_HIP_EINVAL, "invalid total_anchors");
    if (o.total_anchors > kRcnnMaxAnchors)
        fail(AEON_HIP_EUNSUPPORTED, "localization_rcnn: total_anchors above 65536 (the per-record LDS state)");
    if (o.rois_per_image < 0 || o.num_fg < 0 || o.num_fg > o.rois_per_image)
        fail(AEON_HIP_EINVAL, "invalid rois_per_image / num_fg");
    if (o.rois_per_image > kRcnnMaxRois) fail(AEON_HIP_EUNSUPPORTED, "localization_rcnn: rois_per_image above 1024");
    if (o.max_gt_boxes <= 0) fail(AEON_HIP_EINVAL, "invalid max_gt_boxes");
    check_emit(o.emit_type);
    if (!o.anchors) fail(AEON_HIP_EINVAL, "null anchors");
    const uint64_t A = (uint64_t)o.total_anchors, m = (uint64_t)o.max_gt_boxes;
    const uint64_t need[10] = {16 * A, 16 * A, 8 * A, 8 * A, 8, 16 * m, 4, 4 * m, 4, 4 * m};
    for (int k = 0; k < 10; k++)
        if (!out_buf_ok(o.buf[k], o.item_stride[k], need[k], 4))
            fail(AEON_HIP_EINVAL, "rcnn buffers: 4-byte aligned items of the output's size");
    if (!out_buf_ok(o.buf[5], o.item_stride[5], need[5], 16)) fail(AEON_HIP_EINVAL, "gt_boxes buffer: 16-byte aligned items");
}

// The input side of a direct call (aeon_hip_box_targets_batch, aeon_hip_rcnn_targets_batch).
struct BoxCall {
    int                    n;
    const aeon_box_record* recs;
    const float*           boxes;
    const int32_t *        labels, *difficult;
    const aeon_aug_params* params;
};

// Validates a direct call in the order the C entries refuse in; check_out() is the entry's look at its
// output description.  max_count: the most boxes a record may have (0: no limit).  Returns false for a
// call of no records; else `total`, the box table's length.
template <typename CheckOut>
bool check_box_call(const aeon_hip_ctx* ctx, const void* out, const BoxCall& c, int max_count, CheckOut check_out, size_t& total)
{
    if (!ctx || !out) fail(AEON_HIP_EINVAL, "null argument");
    if (c.n < 0) fail(AEON_HIP_EINVAL, "negative record count");
    if (c.n == 0) return false;
    if (!c.recs || !c.params) fail(AEON_HIP_EINVAL, "null argument");
    check_out();
    total = 0;
    for (int i = 0; i < c.n; i++) {
        if (c.recs[i].count < 0) fail(AEON_HIP_EINVAL, "negative box count");
        if (max_count && c.recs[i].count > max_count)
            fail(AEON_HIP_EUNSUPPORTED, "localization_rcnn: more than 1024 boxes in a record");
        total = std::max(total, (size_t)c.recs[i].first + (size_t)c.recs[i].count);
    }
    if (total > 0 && (!c.boxes || !c.labels || !c.difficult)) fail(AEON_HIP_EINVAL, "null box table");
    if (total > ((size_t)1 << 26)) fail(AEON_HIP_EINVAL, "box table too large");
    for (int i = 0; i < c.n; i++)
        if (const char* why = box_refusal(c.params[i], c.recs[i].count ? c.boxes + 4 * (size_t)c.recs[i].first : nullptr,
                                          c.recs[i].count))
            fail(AEON_HIP_EINVAL, why);
    return true;
}

// A checked call's table (box_job.hpp) written into its ring slot's pinned buffer -- the extension, when the
// call has one, by fill_ext(RcnnRec*) -- and copied to the slot's device table on `stream`.  The caller
// holds ctx->mu and the slot's lease, which it releases after its launch over the device table, which is
// returned.
template <typename FillExt>
BoxTableDev stage_box_call(aeon_hip_ctx* ctx, const BoxCall& c, size_t total, bool rcnn, hipStream_t stream, Slot& s,
                           FillExt fill_ext)
{
    ensure_ring(ctx, box_table_bytes(c.n, total, rcnn), 0, 0);
    const BoxTableHost t(s.host, c.n, total, rcnn);
    for (int i = 0; i < c.n; i++) t.recs[i] = box_rec(c.recs[i].first, c.recs[i].count, c.params[i]);
    if (rcnn) fill_ext(t.ext);
    if (total) {
        std::memcpy(t.boxes, c.boxes, total * sizeof(float) * 4);
        std::memcpy(t.labels, c.labels, total * sizeof(int32_t));
        std::memcpy(t.difficult, c.difficult, total * sizeof(int32_t));
    }
    HIP_OK(hipMemcpyAsync(s.dev, s.host, t.bytes, hipMemcpyHostToDevice, stream));
    return BoxTableDev(s.dev, c.n, total, rcnn);
}

// One launch over a box table in device memory.
void launch_box_table(int n, const BoxTableDev& t, const aeon_box_out& o, hipStream_t stream)
{
    BoxLaunch L{};
    L.t = t;
    L.n = n, L.kind = o.kind, L.max_boxes = o.max_boxes, L.emit_type = o.emit_type;
    L.emit_min_overlap = o.emit_min_overlap;
    L.norm_w = (float)o.out_w, L.norm_h = (float)o.out_h;
    L.shape_w = o.out_w, L.shape_h = o.out_h;
    for (int k = 0; k < 5; k++) L.buf[k] = (uint8_t*)o.buf[k], L.stride[k] = o.item_stride[k];
    HIP_OK(launch_box_targets(L, stream));
}

// aeon_hip_box_targets_batch: the call's table through a ring slot, read by one launch.
int run_box_targets(aeon_hip_ctx* ctx, int n, const aeon_box_record* recs, const float* boxes, const int32_t* labels,
                    const int32_t* difficult, const aeon_aug_params* params, const aeon_box_out* out, void* stream_)
{
    const BoxCall c{n, recs, boxes, labels, difficult, params};
    size_t        total;
    if (!check_box_call(ctx, out, c, 0, [&] { check_box_out(*out); }, total)) return 0;
    hipStream_t stream = (hipStream_t)stream_;

    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_OK(hipSetDevice(ctx->device));
    SlotLease         lease(ctx, stream);
    const BoxTableDev t = stage_box_call(ctx, c, total, false, stream, lease.slot(), [](RcnnRec*) {});
    launch_box_table(n, t, *out, stream);
    lease.release();
    return 0;
}

// The config's anchor table on the device: uploaded when it differs from the resident one.  A caller that
// keeps one table per key (aeon_rcnn_out::anchors_key != 0: the decoder's provider) is believed on the key;
// without a key the table's content is compared.
const float* resident_anchors(aeon_hip_ctx* ctx, const aeon_rcnn_out& o)
{
    const size_t words = 4 * (size_t)o.total_anchors;
    if (ctx->rcnn_anchors_dev && ctx->rcnn_anchors_host.size() == words) {
        if (o.anchors_key != 0 ? ctx->rcnn_anchors_key == o.anchors_key
                               : std::memcmp(ctx->rcnn_anchors_host.data(), o.anchors, words * sizeof(float)) == 0)
            return ctx->rcnn_anchors_dev;
    }
    HIP_OK(hipDeviceSynchronize()); // launches that read the resident table
    if (ctx->rcnn_anchors_dev) HIP_OK(hipFree(ctx->rcnn_anchors_dev));
    ctx->rcnn_anchors_dev = nullptr;
    ctx->rcnn_anchors_host.assign(o.anchors, o.anchors + words);
    ctx->rcnn_anchors_key = 0;
    HIP_OK(hipMalloc((void**)&ctx->rcnn_anchors_dev, words * sizeof(float)));
    HIP_OK(hipMemcpy(ctx->rcnn_anchors_dev, o.anchors, words * sizeof(float), hipMemcpyHostToDevice));
    ctx->rcnn_anchors_key = o.anchors_key;
    return ctx->rcnn_anchors_dev;
}

// One launch over an rcnn table (a box table with the extension) in device memory.
void launch_rcnn_table(aeon_hip_ctx* ctx, int n, const BoxTableDev& t, const aeon_rcnn_out& o, int shuffle,
                       uint32_t* states_dev, hipStream_t stream)
{
    RcnnLaunch L{};
    L.t          = t;
    L.anchors    = resident_anchors(ctx, o);
    L.states_out = states_dev;
    L.n = n, L.total_anchors = o.total_anchors, L.max_gt_boxes = o.max_gt_boxes, L.emit_type = o.emit_type;
    L.emit_min_overlap = o.emit_min_overlap;
    L.negative_overlap = o.negative_overlap, L.positive_overlap = o.positive_overlap;
    L.rois_per_image = o.rois_per_image, L.num_fg = o.num_fg, L.shuffle = shuffle ? 1 : 0;
    for (int k = 0; k < 10; k++) L.buf[k] = (uint8_t*)o.buf[k], L.stride[k] = o.item_stride[k];
    HIP_OK(launch_rcnn_targets(L, stream));
}

// aeon_hip_rcnn_targets_batch: the call's table goes through a ring slot like a box call's; with engine
// states the end states come back (one small D2H behind the kernel, then the stream is synchronized).
int run_rcnn_targets(aeon_hip_ctx* ctx, int n, const aeon_box_record* recs, const float* boxes, const int32_t* labels,
                     const int32_t* difficult, const aeon_aug_params* params, uint32_t* engine_states, int shuffle,
                     const aeon_rcnn_out* out, void* stream_)
{
    const BoxCall c{n, recs, boxes, labels, difficult, params};
    size_t        total;
    auto          check_out = [&] {
        if (shuffle && !engine_states) fail(AEON_HIP_EINVAL, "shuffle needs the records' engine states");
        check_rcnn_out(*out);
    };
    if (!check_box_call(ctx, out, c, kRcnnMaxBoxes, check_out, total)) return 0;
    hipStream_t stream = (hipStream_t)stream_;

    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_OK(hipSetDevice(ctx->device));
    SlotLease         lease(ctx, stream);
    const BoxTableDev t = stage_box_call(ctx, c, total, true, stream, lease.slot(), [&](RcnnRec* X) {
        for (int i = 0; i < n; i++)
            X[i] = rcnn_rec(params[i], out->fixed_scaling_factor, out->width, out->height, engine_states ? engine_states[i] : 1u);
    });
    uint32_t* states_dev = nullptr;
    if (engine_states) {
        if ((size_t)n > ctx->rcnn_states_cap) {
            HIP_OK(hipDeviceSynchronize());
            if (ctx->rcnn_states_dev) HIP_OK(hipFree(ctx->rcnn_states_dev));
            ctx->rcnn_states_dev = nullptr, ctx->rcnn_states_cap = 0;
            HIP_OK(hipMalloc((void**)&ctx->rcnn_states_dev, (size_t)n * 2 * sizeof(uint32_t)));
            ctx->rcnn_states_cap = (size_t)n * 2;
        }
        states_dev = ctx->rcnn_states_dev;
    }
    launch_rcnn_table(ctx, n, t, *out, shuffle, states_dev, stream);
    lease.release();
    if (engine_states) {
        HIP_OK(hipMemcpyAsync(engine_states, states_dev, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
    }
    return 0;
}

} // namespace

namespace aeon_hip {
// What the two staged entries share: the table's and the outputs' checks, then launch() under the context's lock.
template <typename CheckOut, typename Launch>
static int table_targets_staged(aeon_hip_ctx* ctx, int n, const void* dev_table, const char* misaligned, CheckOut check_out,
                                Launch launch)
{
    return guarded([&] {
        if (!ctx || (n > 0 && !dev_table)) fail(AEON_HIP_EINVAL, "null argument");
        if (n <= 0) return 0;
        if ((uintptr_t)dev_table & 15) fail(AEON_HIP_EINVAL, misaligned);
        check_out();
        std::lock_guard<std::mutex> lock(ctx->mu);
        HIP_OK(hipSetDevice(ctx->device));
        launch();
        return 0;
    });
}
int box_targets_staged(aeon_hip_ctx* ctx, int n, const void* dev_table, size_t total, const aeon_box_out& out,
                       void* stream)
{
    return table_targets_staged(ctx, n, dev_table, "box table not 16-byte aligned", [&] { check_box_out(out); }, [&] {
        launch_box_table(n, BoxTableDev((const uint8_t*)dev_table, n, total, false), out, (hipStream_t)stream);
    });
}
int rcnn_targets_staged(aeon_hip_ctx* ctx, int n, const void* dev_table, size_t total, const aeon_rcnn_out& out,
                        int shuffle, uint32_t* states_dev, void* stream)
{
    return table_targets_staged(ctx, n, dev_table, "rcnn table not 16-byte aligned", [&] { check_rcnn_out(out); }, [&] {
        launch_rcnn_table(ctx, n, BoxTableDev((const uint8_t*)dev_table, n, total, true), out, shuffle, states_dev,
                          (hipStream_t)stream);
    });
}
} // namespace aeon_hip

extern "C" {

int aeon_hip_rcnn_targets_batch(aeon_hip_ctx* ctx, int n, const aeon_box_record* recs, const float* boxes,
                                const int32_t* labels, const int32_t* difficult, const aeon_aug_params* params,
                                uint32_t* engine_states, int shuffle, const aeon_rcnn_out* out, void* stream)
{
    return guarded([&] {
        return run_rcnn_targets(ctx, n, recs, boxes, labels, difficult, params, engine_states, shuffle, out, stream);
    });
}

int aeon_hip_box_targets_batch(aeon_hip_ctx* ctx, int n, const aeon_box_record* recs, const float* boxes,
                               const int32_t* labels, const int32_t* difficult, const aeon_aug_params* params,
                               const aeon_box_out* out, void* stream)
{
    return guarded([&] { return run_box_targets(ctx, n, recs, boxes, labels, difficult, params, out, stream); });
}

} // extern "C"
