// image_path.cpp -- the image path of the device half: a call's records through run_direct (one launch),
// run_records (contrast records in one launch) or run_batch's multi-pass launches over the CallPlan that
// plan.cpp returns, run_video on top of them, and the C entries for augment, mask, pair, depthmap, video,
// transpose, the JPEG batch, the PNG batch, the pixmap batch and the TIFF batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"
#include "aug_job.hpp"
#include "context.hpp"
#include "host.hpp"
#include "jpeg.hpp"
#include "launch.hpp"
#include "mask16.hpp"
#include "param_factory.hpp"
#include "pixmap.hpp"
#include "tiff.hpp"
#include "plan.hpp"
#include "plan_record.hpp"
#include "png.hpp"
#include "video_job.hpp"

using namespace aeon_hip;

namespace {

#ifndef AEON_HIP_UPLOAD_KERNEL_MAX_KB
#define AEON_HIP_UPLOAD_KERNEL_MAX_KB 128
#endif
constexpr size_t kUploadKernelMax = AEON_HIP_UPLOAD_KERNEL_MAX_KB * 1024; // job tables above this go up by SDMA (run_batch)
constexpr size_t kDirectFetchMax  = 512 * 1024; // run_direct: most job bytes a launch's tiles read over PCIe

// Persistent grid: as many workgroups as the CUs hold at once, never more than the tiles.
int grid_for(aeon_hip_ctx* ctx, int mode, const LaunchPlan& P, const LaunchArgs& a)
{
    int per_cu = 0;
    {
        const std::vector<int> key = {mode, P.rm, (int)P.tail, (int)P.photo, a.threads, a.lds_bytes, a.vec_ok, a.has_rtab,
                                      a.out_dtype, a.channel_major, a.m_blocks > 0};
        for (auto& e : ctx->occ)
            if (e.first == key) per_cu = e.second;
        if (per_cu <= 0) {
            HIP_OK(kernel_occupancy(mode, P.rm, P.tail, P.photo, a, &per_cu));
            per_cu = std::max(per_cu, 1);
            ctx->occ.push_back({key, per_cu});
            if (ctx->host_profile)
                std::fprintf(stderr, "[aeon_hip] kernel km=%d rm=%d tail=%d photo=%d: %d threads, %d B LDS, TR %d, "
                                     "%d workgroups/CU x %d CUs, %d tiles\n",
                             mode, P.rm, (int)P.tail, (int)P.photo, a.threads, a.lds_bytes, a.rows_per_tile, per_cu,
                             ctx->n_cu, a.total_tiles);
        }
    }
    return (int)std::min<long>((long)a.total_tiles, (long)per_cu * ctx->n_cu);
}

void timed_launch(aeon_hip_ctx* ctx, int mode, const LaunchPlan& P, const LaunchArgs& a, hipStream_t stream,
                  double bytes, bool timed)
{
    KernelTimer t{};
    if (timed) t = take_timer(ctx, mode, bytes);
    const int grid = grid_for(ctx, mode, P, a);
    HIP_OK(launch_tiles(mode, P.rm, P.tail, P.photo, a, grid, stream, timed ? t.start : nullptr,
                        timed ? t.stop : nullptr));
    if (timed) ctx->timers.push_back(t);
}

// fixed_aspect_ratio: std::fill_n of each item's canvas, its whole byte size as declared (etl_image.cpp:263)
void clear_canvases(const aeon_out_desc& od, void* out_dev, int n, hipStream_t stream)
{
    if (od.fixed_aspect_ratio)
        HIP_OK(hipMemset2DAsync(out_dev, od.item_stride, 0,
                                (size_t)od.canvas_w * od.canvas_h * od.channels * out_elem_bytes(od.dtype), n, stream));
}

LaunchArgs launch_args(aeon_hip_ctx* ctx, const Slot& s, const uint8_t* table, const LaunchPlan& L, int n_jobs,
                       const aeon_out_desc& o, const float* d_lut, int partial_stride, bool u8_map = false)
{
    LaunchArgs a{};
    // dynamic tail: the partial last round plus two full rounds before it drawn from a counter (one
    // or four full rounds measured within noise or slower), the slot's own counter so
    // launches of calls in flight never share one
    a.tail_ctr    = ctx->d_tail + (&s - ctx->slots);
#ifndef AEON_HIP_TAIL_ROUNDS
#define AEON_HIP_TAIL_ROUNDS 2
#endif
    a.tail_rounds = AEON_HIP_TAIL_ROUNDS;
    a.jobs           = (const AugJob*)(table + L.blob_off);
    a.job_bytes      = L.photo ? (int)sizeof(AugJob) : kJobHotBytes;
    a.job_stride     = (int)sizeof(AugJob);
    a.lut            = d_lut; // [3][256]: standardized, or (float)x without mean
    a.hsv_tables     = ctx->d_hsv;
    a.partials       = s.partials;
    a.shifts         = s.shifts;
    a.partial_stride = partial_stride;
    a.error          = ctx->call_error;
#ifdef AEON_HIP_TRACE
    a.trace = ctx->trace; // development builds only (tools/build_variants.sh trace)
#endif
    a.rows_per_tile = L.tr;
    a.max_tiles     = L.max_tiles;
    a.total_tiles   = L.max_tiles * n_jobs;
    a.stage_bytes   = L.stage_bytes;
    a.max_win_w     = L.max_win_w;
    a.out_dtype     = o.dtype;
    a.u8_map        = u8_map;
    a.has_mean      = o.has_mean;
    for (int c = 0; c < 3; c++) { // by source channel (mixChannels from_to {0,2,1,1,2,0} with bgr_to_rgb)
        const int oc = (o.bgr_to_rgb && o.channels == 3) ? 2 - c : c;
        a.smean[c]   = oc < o.channels ? o.mean[oc] : 0;
        a.sinv[c]    = oc < o.channels && o.stddev[oc] != 0 ? 1. / o.stddev[oc] : 0;
    }
    a.channel_major = o.channel_major;
    a.bgr_to_rgb    = o.bgr_to_rgb;
    a.vec_ok        = L.vec_ok && o.channel_major;
    a.lds_bytes     = L.lds;
    a.has_hue       = L.has_hue;
    a.threads       = L.threads;
    a.has_rtab      = L.rtab;
    return a;
}

// Direct call (the common case: C2, C5's image, every record transformed straight from its source in
// one launch group): one launch and nothing else on the stream.  The host checks the records, sizes
// the launch from their geometry and writes each record's AugJob (plan_direct) into the slot's
// pinned table; the tile kernel reads the jobs from there itself (an LDS-DMA of one job per tile,
// a tile ahead, over PCIe) -- no planner or upload launch ahead of it.  Returns false (nothing done)
// when some record needs the multi-pass planner: rotation, resize_short, contrast's two passes,
// 2x-area + photometric, the mask gather pass, or records of several launch groups.
template <typename Phase>
bool run_direct(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs, const void* src_base,
                const aeon_aug_params* params, const aeon_out_desc& od, void* out_dev, hipStream_t stream,
                bool is_mask, Phase&& phase, const ItemMap* im = nullptr)
{
    const OutView        ov = out_view(od);
    const aeon_out_desc& o  = ov.ko; // what the kernels write
    std::vector<JobGeom>& geo = ctx->geoms;
    geo.resize(n);
    std::vector<AugJob>& jobs = ctx->direct_jobs; // each record planned once, copied into the slot below
    if (jobs.size() < (size_t)n) jobs.resize(n);
    int  key = -1, max_h = 0;
    bool vec_ok = !o.fixed_aspect_ratio;
    const OutGeom og = out_geom(o, im);
    for (int i = 0; i < n; i++) {
        const aeon_img_desc&   d = descs[i];
        const aeon_aug_params& p = params[i];
        if (d.elem_bytes != 0 && d.elem_bytes != 1) return false;
        if (is_mask && d.channels == 1 && o.channels == 1 && p.angle == 0) return false; // mask gather pass
        if (p.angle != 0 || (!is_mask && (p.resize_short_size > 0 || expands(p)))) return false;
        if (!is_mask && p.interp > AEON_INTERP_NEAREST) return false; // CUBIC / AREA / LANCZOS4 (CallPlan::add)
        validate_record(d, p, o, is_mask);
        AugJob& J = jobs[i];
        const uint64_t item = item_of(im, out_dev, o, i);
        plan_direct(d, (uint64_t)src_base, p, og, item, is_mask, J);
        const int photo = J.photo, mode = J.mode; // (plan_direct: the cv::resize dispatch, photometric flags)
        if ((photo & PHOTO_CONTRAST) || (photo && mode == RESIZE_AREA2X)) return false;
        const bool tail = mode == RESIZE_LINEAR && J.xv < p.out_w * d.channels;
        const int  k    = mode * 4 + (tail ? 2 : 0) + (photo ? 1 : 0);
        if (key < 0) key = k;
        else if (k != key) return false;
        if ((item & 15) != 0 || (p.out_w & 3) != 0) vec_ok = false;
        JobGeom& g = geo[i];
        g.mode = mode, g.cn = d.channels, g.crop_w = p.crop_w, g.crop_h = p.crop_h;
        g.win_w = g.dst_w = p.out_w, g.win_h = g.dst_h = p.out_h, g.photo = photo, g.stats_slot = -1;
        g.scale_x = J.scale_x, g.scale_y = J.scale_y;
        max_h     = std::max(max_h, p.out_h);
    }
    LaunchPlan P;
    P.rm     = key >> 2;
    P.tail   = (key & 2) != 0;
    P.photo  = (key & 1) != 0;
    P.vec_ok = vec_ok;
    P.rtab   = P.photo && (o.dtype == AEON_DTYPE_F32 || out_is_half(o.dtype));
    P.shape(geo);
    P.max_tiles = (max_h + P.tr - 1) / P.tr;
    // every tile reads its job over PCIe: past ~512 KB of such reads per launch the multi-pass path's
    // device table wins (C5's image launch, 4,096 tiles of 256 B: 98 vs 90 us of kernels per step;
    // C2, 1,792 tiles: direct 3 us faster; a job table the kernel imports itself -- one PCIe read per
    // job into device memory, flags, tiles fetching through L2 -- measured no faster, profiles/r03)
    // (C5's image launch with 128-B hot-half fetches, 512 KB: 112.5 vs 95.5 us per step)
    if ((size_t)P.max_tiles * n * sizeof(AugJob) > kDirectFetchMax) return false;
    phase(2);
    SlotLease   lease(ctx, stream);
    Slot&       s     = lease.slot();
    phase(3);
    const float* d_lut = resident_lut(ctx, od, ov.u8_map);
    ensure_ring(ctx, (size_t)n * sizeof(AugJob), 16, 32);
    // without photometric stages the tiles read only each job's hot half: the table holds just those
    // (half the bytes the host writes and publishes)
    const size_t stride = P.photo ? sizeof(AugJob) : (size_t)kJobHotBytes;
    const size_t tbytes = (size_t)n * stride;
    // the jobs go straight into the slot's HBM table when it has one (no pinned copy first), else
    // into the pinned slot the tiles read over PCIe
    const bool vram = ctx->vram_jobs && tbytes > 0 && tbytes <= kVramTableMax && tbytes <= s.vram_cap;
    uint8_t*   dstt = vram ? s.vram : s.host;
    // largest crop first: the first round's workgroups take the first jobs' tiles and the dynamic tail
    // hands out the rest in table order, so the cheapest tiles come last and the launch's tail is
    // theirs (each job carries its own source and output: the order changes nothing else)
    // (a counting sort into 32 area classes: two passes, ~1 us for 256 records, where a comparison sort
    // cost the host several)
    std::vector<int>& order = ctx->direct_order;
    order.resize(n);
    {
        int64_t amax = 1;
        for (int i = 0; i < n; i++) amax = std::max(amax, (int64_t)geo[i].crop_w * geo[i].crop_h);
        int  cnt[33] = {0};
        auto cls     = [&](int i) { return 31 - (int)((int64_t)geo[i].crop_w * geo[i].crop_h * 31 / amax); };
        for (int i = 0; i < n; i++) cnt[cls(i) + 1]++;
        for (int c = 0; c < 32; c++) cnt[c + 1] += cnt[c];
        for (int i = 0; i < n; i++) order[cnt[cls(i)]++] = i;
    }
    for (int i = 0; i < n; i++) {
        AugJob& J = jobs[order[i]];
        J.tiles   = (J.win_h + P.tr - 1) / P.tr;
        std::memcpy(dstt + i * stride, &J, stride);
    }
    phase(4);
    const bool timed = take_timing(ctx);
    clear_canvases(od, out_dev, n, stream);
    const uint8_t* vt = vram ? publish_written(s, tbytes) : nullptr;
    phase(5);
    LaunchArgs     a  = launch_args(ctx, s, vt ? vt : s.host_dev, P, n, o, d_lut, 1, ov.u8_map);
    a.job_stride      = (int)stride;
    a.jobs_host       = 1; // (read-through loads: pinned host memory, or the uncached HBM copy)
    // (the algorithmic bytes only for a timed launch: a pass over the records the call does not need)
    const double lbytes = timed ? launch_bytes(geo, KM_FINAL, out_elem_bytes(o.dtype)) : 0;
    timed_launch(ctx, KM_FINAL, P, a, stream, lbytes, timed);
    phase(6);
    lease.release();
    phase(7);
    return true;
}

// Contrast records in ONE launch (record_kernels.hip): every record 3-channel, INTER_LINEAR with no
// OpenCV scalar-tail columns, no rotation / resize_short / expand, one output size that the lanes'
// registers hold (win_w <= 256, a multiple of 4; win_h <= 224), float32 CHW out; some record with
// contrast (else the single-pass direct call is the better one).  The post-hue record stays on chip:
// no u8 intermediate written and read back, no contrast_reduce launch.  Returns false (nothing done)
// for any other call.  AEON_HIP_RECORDS=0 sends such calls through the two-launch path.
template <typename Phase>
bool run_records(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs, const void* src_base,
                 const aeon_aug_params* params, const aeon_out_desc& od, void* out_dev, hipStream_t stream,
                 bool is_mask, Phase&& phase, const ItemMap* im = nullptr)
{
    if (is_mask || n <= 0 || !ctx->records) return false;
    const OutView        ov = out_view(od);
    const aeon_out_desc& o  = ov.ko;
    if (o.dtype != AEON_DTYPE_F32 || !o.channel_major || o.fixed_aspect_ratio || o.channels != 3) return false;
    if ((((uint64_t)out_dev) & 15) != 0 || (o.item_stride & 15) != 0) return false;
    for (int i = 0; im && i < n; i++)
        if ((im->item[i] & 15) != 0) return false;
    const int W = params[0].out_w, H = params[0].out_h;
    const int nph = rec_phases(W, H);
    if (W <= 0 || (W & 3) != 0 || W > 4 * 256 || H <= 0 || nph <= 0) return false;
    if (simd_boundary(W * 3) < W * 3) return false; // OpenCV's scalar row tail
    bool      contrast = false;
    long      stage    = 0;
    JobGeom   g{};
    for (int i = 0; i < n; i++) {
        const aeon_img_desc&   d = descs[i];
        const aeon_aug_params& p = params[i];
        if (d.channels != 3 || (d.elem_bytes != 0 && d.elem_bytes != 1)) return false;
        if (p.angle != 0 || p.resize_short_size > 0 || expands(p) || p.interp != AEON_INTERP_LINEAR) return false;
        if (p.out_w != W || p.out_h != H || p.crop_w <= 0 || p.crop_h <= 0) return false;
        if (choose_mode(p.crop_w, p.crop_h, W, H, AEON_INTERP_LINEAR, 3) != RESIZE_LINEAR) return false;
        contrast |= (photo_flags(p) & PHOTO_CONTRAST) != 0;
        g.mode = RESIZE_LINEAR, g.cn = 3, g.crop_w = p.crop_w, g.crop_h = p.crop_h, g.win_w = W, g.win_h = H;
        g.scale_x = 1. / ((double)W / p.crop_w);
        g.scale_y = 1. / ((double)H / p.crop_h);
        stage     = std::max(stage, stage_bytes_for(3, stage_rows_for(g, nph * kRecTileRows), stage_cols(g)));
    }
    if (!contrast) return false;
    stage         = (stage + 1023) / 1024 * 1024;
    const int lds = rec_lds_layout(W, (int)stage).total;
    if (lds > kMaxLds) return false;
    for (int i = 0; i < n; i++) validate_record(descs[i], params[i], o, false);
    phase(2);
    SlotLease lease(ctx, stream);
    Slot&     s = lease.slot();
    phase(3);
    const float* d_lut = resident_lut(ctx, od, false);
    ensure_ring(ctx, (size_t)n * sizeof(AugJob), 16, 32);
    AugJob*       jt   = (AugJob*)s.host;
    const OutGeom og   = out_geom(o, im);
    bool          fast = true;
    double        bytes = 0;
    for (int i = 0; i < n; i++) {
        plan_direct(descs[i], (uint64_t)src_base, params[i], og, item_of(im, out_dev, o, i), false, jt[i]);
        if ((jt[i].photo & PHOTO_BS) && jt[i].bs_kind != BS_FIXPT) fast = false;
        // algorithmic bytes: the crop read once + the float32 output written once
        bytes += (double)params[i].crop_w * params[i].crop_h * 3 + (double)W * H * 3 * 4;
    }
    phase(4);
    const uint8_t* vt = publish_table(ctx, s, (size_t)n * sizeof(AugJob));
    phase(5);
    LaunchArgs a{};
    a.jobs        = (const AugJob*)(vt ? vt : s.host_dev);
    a.jobs_host   = 1; // (read-through loads: pinned host memory, or the uncached HBM copy)
    a.job_bytes   = (int)sizeof(AugJob);
    a.lut         = d_lut;
    a.hsv_tables  = ctx->d_hsv;
    a.error       = ctx->call_error;
    a.stage_bytes = (int)stage;
    a.max_win_w   = W;
    a.out_dtype   = AEON_DTYPE_F32;
    a.channel_major = 1;
    a.bgr_to_rgb  = o.bgr_to_rgb && o.channels == 3;
    a.threads     = (nph * (W / 4) + 63) / 64 * 64;
    // helper waves (record_kernels.hip: staging only) when the workgroup has room for them
    constexpr int kRecHelpers = 2;
    const bool    split       = a.threads + 64 * kRecHelpers <= 1024;
    if (split) a.threads += 64 * kRecHelpers;
    a.lds_bytes   = lds;
#ifdef AEON_HIP_TRACE
    a.trace = ctx->trace; // development builds only (tools/trace_records.py)
#endif
    const RecArgs r{n, nph, W, H, ((H + nph - 1) / nph + kRecTileRows - 1) / kRecTileRows};
    const int     grid  = std::min(n, ctx->n_cu); // one workgroup per CU (LDS, 14-16 waves at <= 128 VGPRs)
    const bool    timed = take_timing(ctx);
    KernelTimer   t{};
    if (timed) t = take_timer(ctx, KM_FINAL, bytes);
    HIP_OK(launch_contrast_records(fast, split, a, r, grid, stream, timed ? t.start : nullptr, timed ? t.stop : nullptr));
    if (timed) ctx->timers.push_back(t);
    phase(6);
    lease.release();
    phase(7);
    return true;
}

// A pair call whose images are one final tile launch: the masks' row blocks go into that launch (its
// workgroups take them after their tiles, augment_kernels.hip mask_blocks) -- no gather launch.
// into = that launch's group (null: the gather launch), then nearest_staged's geometry inside it.
struct MaskFuse {
    const LaunchPlan* into = nullptr;
    int               rows = 0, pitch = 0, slots = 0, base = 0, lds = 0;
};
MaskFuse fuse_masks(const CallPlan& plan)
{
    MaskFuse f;
    if (plan.m16.empty() || !plan.rot.empty() || !plan.exp.empty() || !plan.gr_short.jobs.empty() || !plan.gr_main.jobs.empty())
        return f;
    int groups = 0;
    for (const LaunchPlan& P : plan.tiles)
        if (!P.jobs.empty()) groups++, f.into = &P;
#ifndef AEON_HIP_FUSED_MASK_ROWS
#define AEON_HIP_FUSED_MASK_ROWS 64
#endif
    f.rows = std::min(mask16_rows(plan.m16_max_w, plan.m16_max_seg), AEON_HIP_FUSED_MASK_ROWS);
    if (groups != 1 || f.into < plan.tiles + CallPlan::kMain || f.into >= plan.tiles + CallPlan::kWide || f.rows < 1 || f.into->has_contrast) return MaskFuse{};
    const LaunchPlan& P = *f.into;
    f.pitch = mask16_pitch(plan.m16_max_seg);
    f.slots = std::max(1, std::min(plan.m16_max_slots, f.rows));
    f.base  = lds_layout(P.max_win_w, P.tr, P.stage_bytes, P.photo && P.has_hue, P.rtab).stage;
    f.lds   = std::max(P.lds, f.base + kMaskBlockHdrBytes + f.slots * f.pitch);
    return f.lds > kMaxLds ? MaskFuse{} : f;
}

// Job-table transport: where the call's kernels read the table that plan.write left in the pinned slot.
// Tables up to kUploadKernelMax go up by a small kernel on the launch
// stream that reads the pinned slot over PCIe (kernel-to-kernel order, no cross-queue wait:
// 43.5 vs 44.2 us per C2 step against an SDMA copy + event, which costs a ~6.6 us dispatch gap);
// larger ones by SDMA on copy_stream, which overlaps the previous call's kernels while the
// upload kernel would read PCIe at ~34 GB/s (C3, 512 KB: 347 vs 357 us per step).
// A call of pixel-mask gather jobs only (C5's masks): the gather reads its few jobs (one per
// workgroup) from the pinned slot itself, no upload launch ahead of it.
// (A pair call's tables go up together by the upload kernel, and its gather launch reads the device
// copy: C5 93-94 us per step against 96-98 for the image and mask calls, whose gather reads the
// pinned slot -- 4.5 us more kernel time -- and 97-98 for the masks first on the pinned slot while
// SDMA uploads the images' table; tools/c5_ab.sh)
const uint8_t* transport_table(aeon_hip_ctx* ctx, Slot& s, const CallPlan& plan, hipStream_t stream)
{
    // the tables in HBM written by the host (no upload launch) unless a LANCZOS4 tap table is among
    // them (read per output pixel: the cached device copy)
    const bool     vram_ok = plan.gr_short.n_taps == 0 && plan.gr_main.n_taps == 0;
    const uint8_t* vt      = vram_ok ? publish_table(ctx, s, plan.blob) : nullptr;
    const uint8_t* table   = vt ? vt : plan.mask_only ? s.host_dev : s.dev;
    if (plan.mask_only || vt) {
    } else if (plan.blob > kUploadKernelMax) {
        HIP_OK(hipMemcpyAsync(s.dev, s.host, plan.blob, hipMemcpyHostToDevice, ctx->copy_stream));
        HIP_OK(hipEventRecord(s.copied, ctx->copy_stream));
        HIP_OK(hipStreamWaitEvent(stream, s.copied, 0));
    } else {
        HIP_OK(launch_upload_table(s.host_dev, s.dev, plan.blob, stream));
    }
    for (const GrPlan* g : {&plan.gr_short, &plan.gr_main}) // the Lanczos4 taps from their host-computed inputs
        if (g->n_taps)
            HIP_OK(launch_lanczos4_taps((const LzIn*)(table + g->lz_off), (GrTap*)(table + g->taps_off), (int)g->n_taps,
                                        stream));
    return table;
}

// The launches of one GrPlan: resize_sep bands or resize_generic tiles per method class.
void launch_generic(aeon_hip_ctx* ctx, const GrPlan& g, const uint8_t* table, const aeon_out_desc& o, const float* d_lut,
                    hipStream_t stream, bool timed)
{
    if (g.jobs.empty()) return;
    KernelTimer t{};
    if (timed) t = take_timer(ctx, KM_RAW, g.bytes);
    if (timed) HIP_OK(hipEventRecord(t.start, stream));
    const int gbgr = o.bgr_to_rgb && o.channels == 3, gchm = o.channel_major;
    for (const GrPlan::Sub& u : g.subs) {
        const ResizeJob* gj   = (const ResizeJob*)(table + g.off) + u.first;
        const float*     glut = u.any_final ? d_lut : nullptr;
        if (u.sep)
            HIP_OK(launch_resize_sep(u.sep, u.area, gj, table, u.count, u.max_tiles, u.TR, u.CW, u.NR, u.SW, u.cn_max, glut, gbgr,
                                     gchm, ctx->call_error, stream));
        else
            HIP_OK(launch_resize_generic(gj, table, u.count, u.max_tiles, u.TR, u.CW, u.NR, u.xs, u.amax, u.cn_max, u.SW,
                                         glut, gbgr, gchm, ctx->call_error, stream));
    }
    if (timed) {
        HIP_OK(hipEventRecord(t.stop, stream));
        ctx->timers.push_back(t);
    }
}

std::string half_refusal(int dtype, const char* what)
{
    return std::string(dtype == AEON_DTYPE_BF16 ? "bfloat16" : "float16") + " output is implemented for images only, not for " + what;
}

int run_batch(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs, const void* src_base,
              const aeon_aug_params* params, const aeon_out_desc* out, void* out_dev, void* stream_,
              bool is_mask, const MaskSet* ms = nullptr, const ItemMap* im = nullptr)
{
    if (!ctx || n < 0 || (n > 0 && (!descs || !params || !out || !out_dev || !src_base)))
        fail(AEON_HIP_EINVAL, "null argument");
    if (n == 0) return 0;
    if (n > 65535) fail(AEON_HIP_EINVAL, "at most 65535 records per call");
    const aeon_out_desc& od = *out; // as declared; `o` below is what the kernels write (out_view)
    if (od.dtype < AEON_DTYPE_U8 || od.dtype > AEON_DTYPE_BF16) fail(AEON_HIP_EUNSUPPORTED, "unknown output dtype");
    const bool half = out_is_half(od.dtype);
    // float16 / bfloat16 are image outputs of the tile kernel only: refused here, before any launch (the
    // gather kernels' and the uint8 canvas view's stores know nothing of them)
    if (half && is_mask) fail(AEON_HIP_EUNSUPPORTED, half_refusal(od.dtype, "pixel masks / depth maps"));
    if (half && od.fixed_aspect_ratio) fail(AEON_HIP_EUNSUPPORTED, half_refusal(od.dtype, "fixed_aspect_ratio"));
    if (od.has_mean && od.dtype != AEON_DTYPE_F32 && od.dtype != AEON_DTYPE_F64 && !half)
        fail(AEON_HIP_EINVAL,
             "Standardization (mean, stddev) is supported only for float or double 'output_type'.");
    const OutView        ov = out_view(od);
    const aeon_out_desc& o  = ov.ko;
    if (o.bgr_to_rgb && o.channels != 3)
        fail(AEON_HIP_EINVAL, "invalid config: bgr_to_rgb can be 'true' only for channels set to '3'");
    // pixel_mask / depthmap loaders never standardize or swap channels (etl_pixel_mask.cpp:94-105,
    // etl_depthmap.cpp:98-134): refuse both, so rotated and unrotated masks agree
    if (is_mask && (od.has_mean || od.bgr_to_rgb))
        fail(AEON_HIP_EINVAL, "pixel masks / depth maps take no mean/stddev and no bgr_to_rgb");
    if (od.fixed_aspect_ratio) {
        // aeon's fixed-aspect loader zeroes the item's whole byte size and views the canvas as
        // CV_8U planes whatever the output type (etl_image.cpp:263-305): out_view
        if (od.canvas_w <= 0 || od.canvas_h <= 0 ||
            (size_t)od.canvas_w * od.canvas_h * od.channels * out_elem_bytes(od.dtype) > od.item_stride)
            fail(AEON_HIP_EINVAL, "fixed_aspect_ratio: canvas does not fit item_stride");
    }
    hipStream_t stream = (hipStream_t)stream_;

    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->call_error = stream_error(ctx, stream);
    using clk = std::chrono::steady_clock;
    auto t_prev = clk::now();
    auto phase  = [&](int k) {
        if (!ctx->host_profile) return;
        auto t = clk::now();
        ctx->host_ns[k].push_back(std::chrono::duration<double, std::nano>(t - t_prev).count());
        t_prev = t;
    };
    HIP_OK(hipSetDevice(ctx->device));
    phase(0);
    // (a pair call goes through the planner: its masks join the images' launch)
    if (!ms && ctx->direct && run_direct(ctx, n, descs, src_base, params, od, out_dev, stream, is_mask, phase, im))
        return 0;
    if (!ms && run_records(ctx, n, descs, src_base, params, od, out_dev, stream, is_mask, phase, im)) return 0;

    CallPlan& plan = ctx->plan;
    plan.clear();
    plan.add_records(n, descs, src_base, params, o, out_dev, is_mask, ms, im);
    phase(1);
    plan.finalize(o);
    if (std::max(plan.gr_short.n_taps, plan.gr_main.n_taps) > 4096 && !ctx->plan_pool)
        ctx->plan_pool.reset(new thread_pool(thread_affinity_map("")));
    phase(2);
    SlotLease lease(ctx, stream);
    Slot&     s = lease.slot();
    phase(3);
    const float* d_lut = resident_lut(ctx, od, ov.u8_map);
    // job tables, contrast sums and shifts: one capacity for every slot of the ring (a call never
    // allocates unless it needs more than any call before it); scratch per slot, on demand
    ensure_ring(ctx, plan.ring_need, plan.partial_words * 4, std::max(1, plan.n_stats) * 4 * sizeof(double));
    if (plan.scratch_bytes > s.scratch_cap) // (slack as ensure_ring)
        grow(s.scratch, s.scratch_cap, plan.scratch_bytes + plan.scratch_bytes / 4, false);
    plan.write(s.host, (uint64_t)s.scratch, [&](int k, const std::function<void(int)>& f) { ctx->plan_pool->run(k, f); });
    phase(4);
    const uint8_t* table = transport_table(ctx, s, plan, stream);
    const bool     timed = take_timing(ctx);
    phase(5);

    clear_canvases(od, out_dev, n, stream);
    if (!plan.rot.empty()) { // image::rotate pre-pass first: the gather and tile passes read its output
        int words = 0;       // (the launch's LDS source box, rotate_kernels.hip)
        for (const RotJob& R : plan.rot) words = std::max(words, rot_box_words(R.angle));
        HIP_OK(launch_rotate((const RotJob*)(table + plan.rot_off), (int)plan.rot.size(), plan.rot_max_tiles, words, plan.rot_cn,
                             ctx->call_error, stream));
    }
    if (!plan.exp.empty()) // then image::expand (etl_image.cpp:155-159)
        HIP_OK(launch_expand((const ExpandJob*)(table + plan.exp_off), (int)plan.exp.size(), plan.exp_max_px, stream));
    const MaskFuse mf = ms && ctx->fuse_masks ? fuse_masks(plan) : MaskFuse{};
    if (!plan.m16.empty() && !mf.into) { // the gather pass
        KernelTimer t{};
        if (timed) t = take_timer(ctx, KM_FINAL, plan.m16_bytes);
        HIP_OK(launch_nearest((const Mask16Job*)(table + plan.m16_off), (int)plan.m16.size(), plan.m16_max_h, plan.m16_max_w,
                              plan.m16_max_seg, plan.m16_max_slots, stream, timed ? t.start : nullptr, timed ? t.stop : nullptr));
        if (timed) ctx->timers.push_back(t);
    }
    const size_t oelem = out_elem_bytes(o.dtype);
    const auto   args  = [&](const LaunchPlan& L) {
        return launch_args(ctx, s, table, L, (int)L.jobs.size(), o, d_lut, plan.partial_stride, ov.u8_map);
    };
    const auto pass = [&](int first, int end, int km) { // the tile launches of one pass
        for (int g = first; g < end; g++) {
            const LaunchPlan& P = plan.tiles[g];
            if (P.jobs.empty()) continue;
            double bytes = launch_bytes(P.jobs, km, km == KM_RAW ? 1 : oelem);
            if (km != KM_FINAL) {
                timed_launch(ctx, km, P, args(P), stream, bytes, timed);
                continue;
            }
            if (P.has_contrast) HIP_OK(launch_contrast_reduce(args(P), (int)P.jobs.size(), stream));
            LaunchArgs a = args(P);
            if (&P == mf.into) {
                a.mjobs    = (const Mask16Job*)(table + plan.m16_off);
                a.m_ctr    = ctx->d_tail + aeon_hip_ctx::kSlots + lease.index;
                a.m_bpj    = (plan.m16_max_h + mf.rows - 1) / mf.rows;
                a.m_blocks = (int)plan.m16.size() * a.m_bpj;
                a.m_rows = mf.rows, a.m_pitch = mf.pitch, a.m_perm = 1, a.m_slots = mf.slots, a.m_lds = mf.base;
                a.lds_bytes = mf.lds;
                bytes += plan.m16_bytes;
            }
            timed_launch(ctx, KM_FINAL, P, a, stream, bytes, timed);
        }
    };
    launch_generic(ctx, plan.gr_short, table, o, d_lut, stream, timed);
    pass(CallPlan::kPre, CallPlan::kPre2, KM_RAW);
    pass(CallPlan::kWide, CallPlan::kGroups, KM_RAW);
    launch_generic(ctx, plan.gr_main, table, o, d_lut, stream, timed);
    pass(CallPlan::kPre2, CallPlan::kPass1, KM_RAW);
    pass(CallPlan::kPass1, CallPlan::kMain, KM_STATS);
    pass(CallPlan::kMain, CallPlan::kWide, KM_FINAL);
    phase(6);
    lease.release();
    phase(7);
    return 0;
}

// ---- video ---------------------------------------------------------------------------------------
// aeon_hip_video_batch: video::transformer + video::loader (src/etl_video.cpp:49-107).  Every kept frame
// is one record of a run_batch call with its clip's params -- so every pass of the image path takes
// clips as it takes images -- writing uint8 planes, no channel swap, at item + d * H * W with the planes
// D * H * W apart (ItemMap); the pad frames of the short clips are one clip_pad launch behind it.
int run_video(aeon_hip_ctx* ctx, int n, const int32_t* frame_counts, const aeon_img_desc* descs, const void* src_base,
              const aeon_aug_params* params, int D, int out_w, int out_h, void* out_dev, uint64_t item_stride,
              void* stream_)
{
    if (!ctx || n < 0 || (n > 0 && (!frame_counts || !descs || !params || !out_dev || !src_base)))
        fail(AEON_HIP_EINVAL, "null argument");
    if (n == 0) return 0;
    if (D <= 0 || out_w <= 0 || out_h <= 0) fail(AEON_HIP_EINVAL, "video: invalid max_frame_count or frame size");
    const uint64_t hw = (uint64_t)out_w * (uint64_t)out_h;
    if (hw > INT32_MAX || 3 * (uint64_t)D * hw > (uint64_t)INT32_MAX)
        fail(AEON_HIP_EUNSUPPORTED, "video: a clip item above 2^31 - 1 bytes");
    const uint64_t item_bytes = 3 * (uint64_t)D * hw;
    if (item_stride < item_bytes) fail(AEON_HIP_EINVAL, "video: output item does not fit item_stride");
    uint64_t total = 0;
    for (int i = 0; i < n; i++) {
        if (frame_counts[i] < 0 || frame_counts[i] > D)
            fail(AEON_HIP_EINVAL, "video: frame count of clip " + std::to_string(i) + " outside [0, max_frame_count]");
        if (params[i].out_w != out_w || params[i].out_h != out_h)
            fail(AEON_HIP_EINVAL, "video: output_size of clip " + std::to_string(i) + " differs from the frame size");
        total += (uint64_t)frame_counts[i];
    }
    // (run_batch's own limit, with the clip in the message: a job table of n * D entries)
    if (total > 65535) fail(AEON_HIP_EINVAL, "video: at most 65535 frames per call");
    // (kept between calls: a C3D window's 2,048 frames make these ~300 KB, which allocated per call come
    // from mmap and cost their page faults again each time)
    static thread_local std::vector<aeon_img_desc>   fd;
    static thread_local std::vector<aeon_aug_params> fp;
    static thread_local std::vector<uint64_t>        items;
    static thread_local std::vector<PadRegion>       pads;
    fd.clear(), fp.clear(), items.clear(), pads.clear();
    fd.reserve(total), fp.reserve(total), items.reserve(total);
    uint64_t max_pad = 0;
    for (int i = 0; i < n; i++) {
        const uint64_t item = (uint64_t)out_dev + (uint64_t)i * item_stride;
        const int      fc   = frame_counts[i];
        for (int d = 0; d < fc; d++) {
            const aeon_img_desc& f = descs[(size_t)i * D + d];
            // imdecode(ANYDEPTH | COLOR): three channels, also for grayscale files (cap_mjpeg_decoder.cpp:140)
            if (f.channels != 3 || (f.elem_bytes != 0 && f.elem_bytes != 1))
                fail(AEON_HIP_EINVAL, "video: frames are 3-channel 8-bit records");
            fd.push_back(f), fp.push_back(params[i]), items.push_back(item + (uint64_t)d * hw);
        }
        if (fc < D) { // the pad frames of one plane are contiguous
            const uint64_t bytes = (uint64_t)(D - fc) * hw;
            for (int c = 0; c < 3; c++) pads.push_back(PadRegion{item + ((uint64_t)c * D + (uint64_t)fc) * hw, bytes});
            max_pad = std::max(max_pad, bytes);
        }
    }
    if (total) {
        aeon_out_desc o{};
        o.dtype = AEON_DTYPE_U8, o.channels = 3, o.channel_major = 1;
        o.item_stride = item_stride; // (validate_record: a frame fits its clip's item)
        const ItemMap im{items.data(), (int32_t)((uint64_t)D * hw)};
        run_batch(ctx, (int)total, fd.data(), src_base, fp.data(), &o, out_dev, stream_, false, nullptr, &im);
    }
    if (pads.empty()) return 0; // no clip is short: no launch
    hipStream_t                 stream = (hipStream_t)stream_;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_OK(hipSetDevice(ctx->device));
    SlotLease lease(ctx, stream);
    Slot&     s = lease.slot();
    const size_t tbytes = pads.size() * sizeof(PadRegion);
    ensure_ring(ctx, tbytes, 0, 0);
    std::memcpy(s.host, pads.data(), tbytes);
    // the table goes to the slot's device copy first, as the planner's job tables do (run_batch): read from the
    // pinned slot by every work item, its ~4,600 16-byte PCIe reads held the C3D half-short window's launch
    // at 62 us for 19 MB of zeros
    if (tbytes > kUploadKernelMax) HIP_OK(hipMemcpyAsync(s.dev, s.host, tbytes, hipMemcpyHostToDevice, stream));
    else HIP_OK(launch_upload_table(s.host_dev, s.dev, tbytes, stream));
    HIP_OK(launch_clip_pad((const PadRegion*)s.dev, (int)pads.size(), max_pad, stream));
    lease.release();
    return 0;
}

} // namespace

// ---- PNG stage ------------------------------------------------------------------------------------
// Per-context state of aeon_hip_decode_png_batch: a two-deep ring of pinned staging, its device copy and the
// device scratch of the inflated scanlines (a call reuses a set once the call before last is done with it).
struct aeon_hip::PngStage {
    struct Set {
        hipEvent_t done    = nullptr;
        bool       pending = false;
        uint8_t *  pinned = nullptr, *dev = nullptr, *scratch = nullptr;
        size_t     pinned_cap = 0, dev_cap = 0, scratch_cap = 0;
    } sets[2];
    int        next = 0;
    std::mutex mu;
};

void aeon_hip::png_stage_destroy(PngStage* s)
{
    if (!s) return;
    for (auto& st : s->sets) {
        if (st.pending) (void)hipEventSynchronize(st.done);
        if (st.done) (void)hipEventDestroy(st.done);
        if (st.pinned) (void)hipHostFree(st.pinned);
        if (st.dev) (void)hipFree(st.dev);
        if (st.scratch) (void)hipFree(st.scratch);
    }
    delete s;
}

namespace {

// The decode call: each file's chunk walk (png_plan) on the pool, the layout of the call's staging -- the jobs,
// the routed files' zlib streams, the host-decoded files' pixels -- filled on the pool, one H2D, then
// png_inflate and png_unfilter over the jobs and a strided device copy per host-decoded file, all on `stream`.
int run_png(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes, const int* modes,
            const aeon_img_desc* descs, void* dst_base, hipStream_t stream)
{
    if (!ctx || n < 0 || (n > 0 && (!data || !sizes || !modes || !descs || !dst_base))) fail(AEON_HIP_EINVAL, "null argument");
    if (n == 0) return 0;
    HIP_OK(hipSetDevice(ctx->device));
    if (!ctx->png) ctx->png = new PngStage();
    PngStage&                   S = *ctx->png;
    std::lock_guard<std::mutex> lock(S.mu);
    const auto each = [&](const std::function<void(int)>& f) {
        if (ctx->host_pool) ctx->host_pool->run(n, f);
        else
            for (int i = 0; i < n; i++) f(i);
    };
    std::vector<PngPlan> plans(n);
    each([&](int i) {
        if (!data[i] || !sizes[i]) fail(AEON_HIP_EINVAL, "PNG: empty file");
        if (modes[i] < AEON_PNG_BGR8 || modes[i] > AEON_PNG_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown PNG decode mode");
        PngPlan& P = plans[i];
        png_plan(data[i], sizes[i], modes[i], P);
        const aeon_img_desc& d = descs[i];
        if (d.width != P.w || d.height != P.h)
            fail(AEON_HIP_EINVAL, "PNG: record " + std::to_string(i) + " is " + std::to_string(P.w) + "x" + std::to_string(P.h) +
                                      ", its descriptor says " + std::to_string(d.width) + "x" + std::to_string(d.height));
        if (d.stride < 0 || (size_t)d.stride < (size_t)P.w * P.channels * P.elem_bytes) fail(AEON_HIP_EINVAL, "stride too small");
    });
    // layout: the jobs, then per file its stream (8-byte aligned and padded) or its pixels (16-byte aligned)
    std::vector<size_t> at(n), raw_at(n);
    std::vector<int>    job_of(n, -1);
    int                 n_gpu = 0, lds = 0;
    for (int i = 0; i < n; i++)
        if (plans[i].route) job_of[i] = n_gpu++;
    size_t total = (size_t)n_gpu * sizeof(PngJob), scratch = 0;
    for (int i = 0; i < n; i++) {
        const PngPlan& P = plans[i];
        total            = (total + 15) & ~(size_t)15;
        at[i]            = total;
        if (P.route) {
            total += ((P.clen + 7) & ~(size_t)7) + 8;
            raw_at[i] = scratch;
            scratch += ((P.need + 15) & ~(size_t)15) + 16;
        } else {
            total += (size_t)P.w * P.channels * P.elem_bytes * P.h;
        }
    }
    PngStage::Set& st = S.sets[S.next];
    S.next ^= 1;
    if (!st.done) HIP_OK(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    if (st.pending) HIP_OK(hipEventSynchronize(st.done));
    st.pending = false;
    if (total > st.pinned_cap) grow(st.pinned, st.pinned_cap, total + total / 4, true);
    if (total > st.dev_cap) grow(st.dev, st.dev_cap, total + total / 4, false);
    if (scratch > st.scratch_cap) grow(st.scratch, st.scratch_cap, scratch + scratch / 4, false);
    PngJob* jobs = (PngJob*)st.pinned;
    each([&](int i) {
        const PngPlan& P = plans[i];
        uint8_t*       p = st.pinned + at[i];
        if (!P.route) {
            png_decode(data[i], sizes[i], modes[i], p, (size_t)P.w * P.channels * P.elem_bytes, nullptr);
            return;
        }
        PngJob& J = jobs[job_of[i]];
        png_stage(data[i], sizes[i], modes[i], P, J, p);
        std::memset(p + P.clen, 0, ((P.clen + 7) & ~(size_t)7) + 8 - P.clen);
        J.comp   = (uint64_t)(st.dev + at[i]);
        J.raw    = (uint64_t)(st.scratch + raw_at[i]);
        J.out    = (uint64_t)dst_base + descs[i].offset;
        J.stride = descs[i].stride;
    });
    for (int i = 0; i < n; i++)
        if (plans[i].route) lds = std::max(lds, png_unfilter_lds(jobs[job_of[i]].rowb));
    KernelTimer t{};
    bool        timed = false;
    if (ctx->timing && n_gpu) {
        std::lock_guard<std::mutex> tl(ctx->mu);
        if ((timed = take_timing(ctx))) t = take_timer(ctx, kTimerPng, (double)scratch);
    }
    HIP_OK(hipMemcpyAsync(st.dev, st.pinned, total, hipMemcpyHostToDevice, stream));
    if (timed) HIP_OK(hipEventRecord(t.start, stream));
    HIP_OK(launch_png((const PngJob*)st.dev, n_gpu, lds, stream_error(ctx, stream), stream));
    if (timed) {
        HIP_OK(hipEventRecord(t.stop, stream));
        std::lock_guard<std::mutex> tl(ctx->mu);
        ctx->timers.push_back(t);
    }
    for (int i = 0; i < n; i++) {
        const PngPlan& P = plans[i];
        if (P.route) continue;
        const size_t rowb = (size_t)P.w * P.channels * P.elem_bytes;
        HIP_OK(hipMemcpy2DAsync((uint8_t*)dst_base + descs[i].offset, (size_t)descs[i].stride, st.dev + at[i], rowb, rowb,
                                (size_t)P.h, hipMemcpyDeviceToDevice, stream));
    }
    HIP_OK(hipEventRecord(st.done, stream));
    st.pending = true;
    return 0;
}

// ---- pixmap stage (BMP, PNM) ------------------------------------------------------------------------
// The decode call: each file's header parse (pixmap_plan) on the pool, the layout of the call's staging -- the
// jobs, the band table, the routed files as they are (each at a 16-byte-aligned offset, at least 16 zero bytes
// behind it, so the kernel's aligned over-reads stay inside the buffer), the host-decoded ASCII files' pixels --
// filled on the pool, one H2D, then pixmap_convert over the bands and a strided device copy per host-decoded
// file, all on `stream`.  The staging ring is a PngStage of the stage's own (its scratch unused).
int run_pixmap(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes, const int* modes,
               const aeon_img_desc* descs, void* dst_base, hipStream_t stream)
{
    if (!ctx || n < 0 || (n > 0 && (!data || !sizes || !modes || !descs || !dst_base))) fail(AEON_HIP_EINVAL, "null argument");
    if (n == 0) return 0;
    HIP_OK(hipSetDevice(ctx->device));
    if (!ctx->pixmap) ctx->pixmap = new PngStage();
    PngStage&                   S = *ctx->pixmap;
    std::lock_guard<std::mutex> lock(S.mu);
    const auto each = [&](const std::function<void(int)>& f) {
        if (ctx->host_pool) ctx->host_pool->run(n, f);
        else
            for (int i = 0; i < n; i++) f(i);
    };
    std::vector<PixmapPlan> plans(n);
    each([&](int i) {
        if (!data[i] || !sizes[i]) fail(AEON_HIP_EINVAL, "BMP / PNM: empty file");
        if (modes[i] < AEON_DECODE_BGR8 || modes[i] > AEON_DECODE_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown pixmap decode mode");
        PixmapPlan& P = plans[i];
        pixmap_plan(data[i], sizes[i], modes[i], P);
        const aeon_img_desc& d = descs[i];
        if (d.width != P.w || d.height != P.h)
            fail(AEON_HIP_EINVAL, "BMP / PNM: record " + std::to_string(i) + " is " + std::to_string(P.w) + "x" +
                                      std::to_string(P.h) + ", its descriptor says " + std::to_string(d.width) + "x" +
                                      std::to_string(d.height));
        if (d.stride < 0 || (size_t)d.stride < (size_t)P.w * P.channels * P.elem_bytes) fail(AEON_HIP_EINVAL, "stride too small");
    });
    // the band table needs the geometry only: built before the staging is laid out
    std::vector<int>        job_of(n, -1);
    std::vector<PixmapBand> bands;
    int                     n_gpu = 0;
    double                  bytes = 0;
    for (int i = 0; i < n; i++) {
        const PixmapPlan& P = plans[i];
        if (!P.route) continue;
        job_of[i] = n_gpu++;
        PixmapJob g{};
        g.pitch = P.pitch, g.w = P.w, g.h = P.h, g.sbits = P.sbits;
        pixmap_bands(g, job_of[i], bands);
        bytes += (double)P.h * (((double)P.w * P.sbits + 7) / 8 + (double)P.w * P.channels * P.elem_bytes);
    }
    if (bands.size() > (size_t)INT32_MAX) fail(AEON_HIP_EUNSUPPORTED, "BMP / PNM: too many bands for one call");
    // layout: the jobs, the bands, then per file the file itself or its pixels (16-byte aligned)
    std::vector<size_t> at(n);
    const size_t        bands_at = (size_t)n_gpu * sizeof(PixmapJob);
    size_t              total    = bands_at + bands.size() * sizeof(PixmapBand);
    for (int i = 0; i < n; i++) {
        const PixmapPlan& P = plans[i];
        total               = (total + 15) & ~(size_t)15;
        at[i]               = total;
        total += P.route ? sizes[i] + 16 : (size_t)P.w * P.channels * P.elem_bytes * P.h;
    }
    PngStage::Set& st = S.sets[S.next];
    S.next ^= 1;
    if (!st.done) HIP_OK(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    if (st.pending) HIP_OK(hipEventSynchronize(st.done));
    st.pending = false;
    if (total > st.pinned_cap) grow(st.pinned, st.pinned_cap, total + total / 4, true);
    if (total > st.dev_cap) grow(st.dev, st.dev_cap, total + total / 4, false);
    PixmapJob* jobs = (PixmapJob*)st.pinned;
    if (!bands.empty()) std::memcpy(st.pinned + bands_at, bands.data(), bands.size() * sizeof(PixmapBand));
    each([&](int i) {
        const PixmapPlan& P = plans[i];
        uint8_t*          p = st.pinned + at[i];
        if (!P.route) {
            pixmap_decode(data[i], sizes[i], modes[i], p, (size_t)P.w * P.channels * P.elem_bytes, nullptr);
            return;
        }
        PixmapJob& J = jobs[job_of[i]];
        pixmap_stage(data[i], sizes[i], modes[i], P, J, p);
        std::memset(p + sizes[i], 0, 16);
        J.src    = (uint64_t)(st.dev + at[i]);
        J.out    = (uint64_t)dst_base + descs[i].offset;
        J.stride = descs[i].stride;
    });
    KernelTimer t{};
    bool        timed = false;
    if (ctx->timing && n_gpu) {
        std::lock_guard<std::mutex> tl(ctx->mu);
        if ((timed = take_timing(ctx))) t = take_timer(ctx, kTimerPng, bytes);
    }
    HIP_OK(hipMemcpyAsync(st.dev, st.pinned, total, hipMemcpyHostToDevice, stream));
    if (timed) HIP_OK(hipEventRecord(t.start, stream));
    HIP_OK(launch_pixmap((const PixmapJob*)st.dev, (const PixmapBand*)(st.dev + bands_at), (int)bands.size(), stream));
    if (timed) {
        HIP_OK(hipEventRecord(t.stop, stream));
        std::lock_guard<std::mutex> tl(ctx->mu);
        ctx->timers.push_back(t);
    }
    for (int i = 0; i < n; i++) {
        const PixmapPlan& P = plans[i];
        if (P.route) continue;
        const size_t rowb = (size_t)P.w * P.channels * P.elem_bytes;
        HIP_OK(hipMemcpy2DAsync((uint8_t*)dst_base + descs[i].offset, (size_t)descs[i].stride, st.dev + at[i], rowb, rowb,
                                (size_t)P.h, hipMemcpyDeviceToDevice, stream));
    }
    HIP_OK(hipEventRecord(st.done, stream));
    st.pending = true;
    return 0;
}

// ---- TIFF stage ---------------------------------------------------------------------------------------
// The decode call: each file's IFD parse (tiff_plan) on the pool, the call's tables -- jobs, compressed strips
// (sorted by compressed size, largest first: the long waves start first), bands -- then the layout
// of the staging: the tables, the routed files as they are (each at a 16-byte-aligned offset, 16 zero bytes
// behind it, so the kernels' aligned over-reads stay inside the buffer), the host-decoded files' pixels -- filled on
// the pool, one H2D, then tiff_expand over the strips into the files' scratch, tiff_convert over the bands and a
// strided device copy per host-decoded file, all on `stream`.
int run_tiff(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes, const int* modes,
             const aeon_img_desc* descs, void* dst_base, hipStream_t stream)
{
    if (!ctx || n < 0 || (n > 0 && (!data || !sizes || !modes || !descs || !dst_base))) fail(AEON_HIP_EINVAL, "null argument");
    if (n == 0) return 0;
    HIP_OK(hipSetDevice(ctx->device));
    if (!ctx->tiff) ctx->tiff = new PngStage();
    PngStage&                   S = *ctx->tiff;
    std::lock_guard<std::mutex> lock(S.mu);
    const auto each = [&](const std::function<void(int)>& f) {
        if (ctx->host_pool) ctx->host_pool->run(n, f);
        else
            for (int i = 0; i < n; i++) f(i);
    };
    std::vector<TiffPlan> plans(n);
    each([&](int i) {
        if (!data[i] || !sizes[i]) fail(AEON_HIP_EINVAL, "TIFF: empty file");
        if (modes[i] < AEON_DECODE_BGR8 || modes[i] > AEON_DECODE_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown TIFF decode mode");
        TiffPlan& P = plans[i];
        tiff_plan(data[i], sizes[i], modes[i], P);
        const aeon_img_desc& d = descs[i];
        if (d.width != P.w || d.height != P.h)
            fail(AEON_HIP_EINVAL, "TIFF: record " + std::to_string(i) + " is " + std::to_string(P.w) + "x" + std::to_string(P.h) +
                                      ", its descriptor says " + std::to_string(d.width) + "x" + std::to_string(d.height));
        if (d.stride < 0 || (size_t)d.stride < (size_t)P.w * P.channels * P.elem_bytes) fail(AEON_HIP_EINVAL, "stride too small");
    });
    // the tables need the headers only: built before the staging is laid out
    std::vector<int>       job_of(n, -1);
    std::vector<TiffJob>   jobs_host;
    std::vector<TiffStrip> strips;
    std::vector<TiffBand>  bands;
    std::vector<size_t>    raw_at(n, 0);
    size_t                 scratch = 0;
    double                 bytes = 0;
    for (int i = 0; i < n; i++) {
        const TiffPlan& P = plans[i];
        if (!P.route) continue;
        job_of[i] = (int)jobs_host.size();
        jobs_host.emplace_back();
        tiff_stage(data[i], sizes[i], modes[i], P, job_of[i], jobs_host.back(), strips, bands, nullptr);
        raw_at[i] = scratch;
        scratch += (tiff_scratch_bytes(P) + 15) & ~(size_t)15;
        bytes += (double)P.h * ((double)P.rowb + (double)P.w * P.channels * P.elem_bytes);
    }
    const int n_gpu = (int)jobs_host.size();
    if (bands.size() > (size_t)INT32_MAX || strips.size() > (size_t)INT32_MAX) fail(AEON_HIP_EUNSUPPORTED, "TIFF: too many strips for one call");
    std::stable_sort(strips.begin(), strips.end(), [](const TiffStrip& a, const TiffStrip& b) { return a.bytes > b.bytes; });
    // layout: the jobs, the strips, the bands, then per file the file itself or its pixels (16-byte aligned)
    std::vector<size_t> at(n);
    const size_t        strips_at = (size_t)n_gpu * sizeof(TiffJob);
    const size_t        bands_at  = strips_at + strips.size() * sizeof(TiffStrip);
    size_t              total     = bands_at + bands.size() * sizeof(TiffBand);
    for (int i = 0; i < n; i++) {
        const TiffPlan& P = plans[i];
        total             = (total + 15) & ~(size_t)15;
        at[i]             = total;
        total += P.route ? sizes[i] + 16 : (size_t)P.w * P.channels * P.elem_bytes * P.h;
    }
    PngStage::Set& st = S.sets[S.next];
    S.next ^= 1;
    if (!st.done) HIP_OK(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    if (st.pending) HIP_OK(hipEventSynchronize(st.done));
    st.pending = false;
    if (total > st.pinned_cap) grow(st.pinned, st.pinned_cap, total + total / 4, true);
    if (total > st.dev_cap) grow(st.dev, st.dev_cap, total + total / 4, false);
    if (scratch > st.scratch_cap) grow(st.scratch, st.scratch_cap, scratch + scratch / 4, false);
    TiffJob* jobs = (TiffJob*)st.pinned;
    if (!strips.empty()) std::memcpy(st.pinned + strips_at, strips.data(), strips.size() * sizeof(TiffStrip));
    if (!bands.empty()) std::memcpy(st.pinned + bands_at, bands.data(), bands.size() * sizeof(TiffBand));
    each([&](int i) {
        const TiffPlan& P = plans[i];
        uint8_t*        p = st.pinned + at[i];
        if (!P.route) {
            tiff_decode(data[i], sizes[i], modes[i], p, (size_t)P.w * P.channels * P.elem_bytes, nullptr);
            return;
        }
        TiffJob& J = jobs[job_of[i]];
        J          = jobs_host[job_of[i]];
        std::memcpy(p, data[i], sizes[i]);
        std::memset(p + sizes[i], 0, 16);
        J.src    = (uint64_t)(st.dev + at[i]);
        J.raw    = (uint64_t)(st.scratch + raw_at[i]);
        J.out    = (uint64_t)dst_base + descs[i].offset;
        J.stride = descs[i].stride;
    });
    KernelTimer t{};
    bool        timed = false;
    if (ctx->timing && n_gpu) {
        std::lock_guard<std::mutex> tl(ctx->mu);
        if ((timed = take_timing(ctx))) t = take_timer(ctx, kTimerPng, bytes);
    }
    HIP_OK(hipMemcpyAsync(st.dev, st.pinned, total, hipMemcpyHostToDevice, stream));
    if (timed) HIP_OK(hipEventRecord(t.start, stream));
    HIP_OK(launch_tiff((const TiffJob*)st.dev, (const TiffStrip*)(st.dev + strips_at), (int)strips.size(),
                       (const TiffBand*)(st.dev + bands_at), (int)bands.size(), stream_error(ctx, stream), stream));
    if (timed) {
        HIP_OK(hipEventRecord(t.stop, stream));
        std::lock_guard<std::mutex> tl(ctx->mu);
        ctx->timers.push_back(t);
    }
    for (int i = 0; i < n; i++) {
        const TiffPlan& P = plans[i];
        if (P.route) continue;
        const size_t rowb = (size_t)P.w * P.channels * P.elem_bytes;
        HIP_OK(hipMemcpy2DAsync((uint8_t*)dst_base + descs[i].offset, (size_t)descs[i].stride, st.dev + at[i], rowb, rowb,
                                (size_t)P.h, hipMemcpyDeviceToDevice, stream));
    }
    HIP_OK(hipEventRecord(st.done, stream));
    st.pending = true;
    return 0;
}

} // namespace

extern "C" {

int aeon_hip_decode_tiff_batch(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes, const int* modes,
                               const aeon_img_desc* descs, void* dst_base, void* stream)
{
    return guarded([&] { return run_tiff(ctx, n, data, sizes, modes, descs, dst_base, (hipStream_t)stream); });
}

int aeon_hip_decode_pixmap_batch(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes, const int* modes,
                                 const aeon_img_desc* descs, void* dst_base, void* stream)
{
    return guarded([&] { return run_pixmap(ctx, n, data, sizes, modes, descs, dst_base, (hipStream_t)stream); });
}

int aeon_hip_decode_png_batch(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes, const int* modes,
                              const aeon_img_desc* descs, void* dst_base, void* stream)
{
    return guarded([&] { return run_png(ctx, n, data, sizes, modes, descs, dst_base, (hipStream_t)stream); });
}

int aeon_hip_transpose_batch(aeon_hip_ctx* ctx, const void* src_dev, void* dst_dev, int64_t rows, int64_t cols,
                             int element_size, void* stream)
{
    return guarded([&] {
        if (!ctx || !src_dev || !dst_dev) fail(AEON_HIP_EINVAL, "null argument");
        if (rows < 0 || cols < 0) fail(AEON_HIP_EINVAL, "negative matrix size");
        if (element_size != 1 && element_size != 2 && element_size != 4 && element_size != 8)
            fail(AEON_HIP_EINVAL, "unsupported datatype for transpose");
        if (rows / 64 >= 65535) fail(AEON_HIP_EINVAL, "too many rows for one transpose");
        if (rows == 0 || cols == 0) return 0;
        const uint8_t* s = (const uint8_t*)src_dev;
        uint8_t*       d = (uint8_t*)dst_dev;
        const size_t   bytes = (size_t)rows * cols * element_size;
        if (s < d + bytes && d < s + bytes) fail(AEON_HIP_EINVAL, "transpose buffers overlap");
        std::lock_guard<std::mutex> lock(ctx->mu);
        HIP_OK(hipSetDevice(ctx->device));
        HIP_OK(launch_transpose(src_dev, dst_dev, rows, cols, element_size, (hipStream_t)stream));
        return 0;
    });
}

int aeon_hip_augment_batch(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs, const void* src_base,
                           const aeon_aug_params* params, const aeon_out_desc* out, void* out_dev,
                           void* stream)
{
    return guarded([&] { return run_batch(ctx, n, descs, src_base, params, out, out_dev, stream, false); });
}

int aeon_hip_mask_batch(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs, const void* src_base,
                        const aeon_aug_params* params, const aeon_out_desc* out, void* out_dev,
                        void* stream)
{
    return guarded([&] { return run_batch(ctx, n, descs, src_base, params, out, out_dev, stream, true); });
}

int aeon_hip_augment_pair_batch(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs, const void* src_base,
                                const aeon_img_desc* mask_descs, const void* mask_src_base,
                                const aeon_aug_params* params, const aeon_out_desc* out, void* out_dev,
                                const aeon_out_desc* mask_out, void* mask_out_dev, void* stream)
{
    return guarded([&] {
        if (!ctx || n < 0 || (n > 0 && (!mask_descs || !mask_src_base || !mask_out || !mask_out_dev)))
            fail(AEON_HIP_EINVAL, "null argument");
        if (n == 0) return 0;
        // (before the images' launches: a refused pair call writes nothing)
        if (out_is_half(mask_out->dtype)) fail(AEON_HIP_EUNSUPPORTED, half_refusal(mask_out->dtype, "pixel masks / depth maps"));
        // one launch when every mask is an 8-bit single-channel record without rotation into plain
        // uint8 items (the gather pass the launch's workgroups take after the image tiles); otherwise
        // exactly aeon_hip_augment_batch then aeon_hip_mask_batch
        bool fuse = mask_out->dtype == AEON_DTYPE_U8 && mask_out->channels == 1 && !mask_out->fixed_aspect_ratio &&
                    !mask_out->has_mean && !mask_out->bgr_to_rgb && params;
        for (int i = 0; fuse && i < n; i++)
            fuse = (mask_descs[i].elem_bytes == 0 || mask_descs[i].elem_bytes == 1) && mask_descs[i].channels == 1 &&
                   params[i].angle == 0;
        if (!fuse) {
            run_batch(ctx, n, descs, src_base, params, out, out_dev, stream, false);
            return run_batch(ctx, n, mask_descs, mask_src_base, params, mask_out, mask_out_dev, stream, true);
        }
        const MaskSet ms{mask_descs, mask_src_base, *mask_out, mask_out_dev};
        return run_batch(ctx, n, descs, src_base, params, out, out_dev, stream, false, &ms);
    });
}

int aeon_hip_depthmap_batch(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs, const void* src_base,
                            const aeon_aug_params* params, const aeon_out_desc* out, void* out_dev, void* stream)
{
    return guarded([&] {
        if (out && out->fixed_aspect_ratio)
            fail(AEON_HIP_EINVAL, "depthmap::loader has no fixed_aspect_ratio canvas (etl_depthmap.cpp:98-134)");
        return run_batch(ctx, n, descs, src_base, params, out, out_dev, stream, true);
    });
}

int aeon_hip_video_batch(aeon_hip_ctx* ctx, int n, const int32_t* frame_counts, const aeon_img_desc* descs,
                         const void* src_base, const aeon_aug_params* params, int max_frames, int out_w, int out_h,
                         void* out_dev, uint64_t item_stride, void* stream)
{
    return guarded([&] {
        return run_video(ctx, n, frame_counts, descs, src_base, params, max_frames, out_w, out_h, out_dev, item_stride,
                         stream);
    });
}

int aeon_hip_decode_jpeg_batch(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes,
                               const aeon_img_desc* descs, void* dst_base, void* stream)
{
    return guarded([&] {
        if (!ctx || n < 0 || (n > 0 && (!data || !sizes || !descs || !dst_base))) fail(AEON_HIP_EINVAL, "null argument");
        if (n == 0) return 0;
        HIP_OK(hipSetDevice(ctx->device));
        if (!ctx->jpeg) ctx->jpeg = jpeg_state_create(ctx->host_pool, ctx->jpeg_gpu_huff, ctx->jpeg_huff_lanes);
        KernelTimer t{};
        bool        timed = false;
        if (ctx->timing) {
            std::lock_guard<std::mutex> lock(ctx->mu);
            timed = take_timing(ctx);
            if (timed) {
                double px = 0;
                for (int i = 0; i < n; i++) px += (double)descs[i].width * descs[i].height * descs[i].channels;
                t = take_timer(ctx, kTimerJpeg, px);
            }
        }
        jpeg_decode_batch(ctx->jpeg, n, data, sizes, descs, dst_base, stream_error(ctx, (hipStream_t)stream), (hipStream_t)stream,
                          timed ? t.start : nullptr,
                          timed ? t.stop : nullptr);
        if (timed) {
            std::lock_guard<std::mutex> lock(ctx->mu);
            ctx->timers.push_back(t);
        }
        return 0;
    });
}

int aeon_hip_jpeg_huff_lanes(aeon_hip_ctx* ctx, int* lanes)
{
    return guarded([&] {
        if (!ctx || !lanes) fail(AEON_HIP_EINVAL, "null argument");
        *lanes = ctx->jpeg_huff_lanes ? ctx->jpeg_huff_lanes : kHuffLanes;
        return 0;
    });
}

int aeon_hip_jpeg_huff_stage_cap(int lanes, int* bytes)
{
    return guarded([&] {
        if (!bytes) fail(AEON_HIP_EINVAL, "null argument");
        if (lanes != 256 && lanes != 512 && lanes != 1024) fail(AEON_HIP_EINVAL, "jpeg_huff runs 256, 512 or 1024 lanes");
        *bytes = jpeg_huff_stage_cap(lanes);
        return 0;
    });
}

} // extern "C"
