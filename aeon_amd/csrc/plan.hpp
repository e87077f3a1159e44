// plan.hpp -- the image path's planner: the host-side arithmetic aeon does per record before touching
// pixels, and where every byte of a call's job table and scratch goes.  Host-only (no HIP runtime):
// image_path.cpp acts on a finished CallPlan, tests/sanitize/callplan_driver.cpp checks one on a CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/aeon_hip.h"
#include "aug_job.hpp"
#include "error.hpp"
#include "mask16.hpp"
#include "plan_record.hpp"

namespace aeon_hip {

constexpr int kMaxLds = 160 * 1024;

// What the launch planner needs to know of a job (the fields share AugJob's names, so the
// templates below take either).
struct JobGeom {
    int32_t mode, cn, crop_w, crop_h, win_w, win_h, dst_w, dst_h, photo, stats_slot;
    double  scale_x, scale_y;
};

// source-footprint bounds used to size the LDS staging area
template <typename J_>
int stage_cols(const J_& J)
{
    switch (J.mode) {
    // +1: the second tap column is staged even where its weight is 0
    case RESIZE_LINEAR: return std::min(J.crop_w + 1, (int)std::ceil((J.win_w - 1) * J.scale_x) + 4);
    case RESIZE_NEAREST: return std::min(J.crop_w, (int)std::ceil((J.win_w - 1) * J.scale_x) + 3);
    case RESIZE_AREA2X: return 2 * J.win_w;
    default: return J.win_w;
    }
}
template <typename J_>
int stage_rows_for(const J_& J, int tr)
{
    int rows = std::min(tr, J.win_h);
    switch (J.mode) {
    case RESIZE_LINEAR: return std::min(J.crop_h, (int)std::ceil((rows - 1) * J.scale_y) + 3);
    case RESIZE_NEAREST: return std::min(J.crop_h, (int)std::ceil((rows - 1) * J.scale_y) + 2);
    case RESIZE_AREA2X: return 2 * rows;
    default: return rows;
    }
}

struct LaunchPlan {
    int                 rm = RESIZE_LINEAR;
    bool                photo = false;
    bool                tail  = false; // LINEAR jobs with OpenCV scalar-tail columns
    size_t              blob_off = 0;     // byte offset of this group's jobs in the slot blob
    std::vector<AugJob> jobs;
    int                 tr = 1, stage_bytes = 0, max_win_w = 0, max_tiles = 0;
    int                 lds = 0, threads = kBlockMax;
    bool                vec_ok = true;
    bool                has_hue = false, has_contrast = false;
    bool                rtab    = false; // final f32 / f16 / bf16 launch with contrast / lighting: per-record LDS table (f32)
    bool                out_scratch = false; // the jobs write scratch (out_ptr an offset until relocated)

    // launch shape for this->jobs, and each job's tile count
    void finalize()
    {
        if (jobs.empty()) return;
        shape(jobs);
        max_tiles = 0;
        for (AugJob& J : jobs) {
            J.tiles   = (J.win_h + tr - 1) / tr;
            max_tiles = std::max(max_tiles, J.tiles);
        }
    }

    // workgroup size, rows per tile, LDS staging size for a set of jobs (AugJob or JobGeom)
    template <typename J_>
    void shape(const std::vector<J_>& jobs);
};

// Checks of one 8-bit record aeon's transformer would throw on (or that this stage refuses).
void validate_record(const aeon_img_desc& d, const aeon_aug_params& p, const aeon_out_desc& o, bool is_mask);

// Where a call's records go when not to out_dev + i * item_stride as planes of their own size: the video
// call's frames (run_video), frame d of a clip at its item + d * H * W with planes D * H * W apart.
struct ItemMap {
    const uint64_t* item;  // record i's output address
    int32_t         plane; // plane stride (elements)
};
inline uint64_t item_of(const ItemMap* im, const void* out_dev, const aeon_out_desc& o, int i)
{
    return im ? im->item[i] : (uint64_t)out_dev + (uint64_t)i * o.item_stride;
}

inline OutGeom out_geom(const aeon_out_desc& o, const ItemMap* im = nullptr)
{
    return OutGeom{o.fixed_aspect_ratio, o.canvas_w, o.canvas_h, im ? im->plane : 0};
}

// The loader side of a launch: ko = what the kernels write (fixed_aspect_ratio writes its uint8
// canvas whatever the declared type, u8_map = standardized through the LUT); double output
// standardizes in the kernel with the declared mean / stddev by source channel.
struct OutView {
    aeon_out_desc ko;
    bool          u8_map = false;
};
OutView out_view(const aeon_out_desc& o);

// fn(0) .. fn(n - 1), each once, in any order and on any threads (thread_pool::run, or none: in order here)
using ParallelFor = std::function<void(int, const std::function<void(int)>&)>;

// One resize_generic launch: its jobs, the Lanczos tap tables, and the tile shape every job of it
// shares (rows x columns of a tile sized so the taps and the horizontal sums fit 64 KiB of LDS).
struct GrPlan {
    std::vector<ResizeJob> jobs;
    size_t                 off = 0, lz_off = 0, taps_off = 0; // byte offsets in the call's table
    // One launch per method class (finalize sorts the jobs so each class is contiguous): the
    // fixed-K methods as resize_sep bands, the rest (INTER_AREA's float taps, integer boxes, jobs
    // whose bands do not fit) as resize_generic tiles.
    struct Sub {
        int  first = 0, count = 0;
        int  TR = 16, CW = 128, NR = 1, xs = 3, amax = 1, cn_max = 1, max_tiles = 0, SW = 4;
        int  sep = 0;           // K of resize_sep, or 0: resize_generic
        bool area = false;      // resize_sep's INTER_AREA form (resizeArea_ jobs, sep = their most taps)
        bool any_final = false; // some job writes the loader's output itself (its LUT in the launch's LDS)
    };
    std::vector<Sub> subs;
    double bytes = 0; // algorithmic: the source region read once + the window written

    size_t n_taps = 0;     // Lanczos4 taps reserved by add(), their inputs computed by fill_taps()
    size_t n_taps_max = 0; // ... and what the jobs would need with no axis shared (the ring's sizing bound)
    // One tap array per distinct axis (source size, scale, first destination index, count, column clamp):
    // a batch of random crops over one output size repeats them (C2: ~76 crop widths, ~76 heights for 512
    // axes of 256 records), and equal inputs give equal taps.
    struct LzAxis {
        int      ssize, d0, n, clamp;
        uint64_t scale_bits;
        bool     operator==(const LzAxis& o) const
        {
            return ssize == o.ssize && d0 == o.d0 && n == o.n && clamp == o.clamp && scale_bits == o.scale_bits;
        }
    };
    struct LzAxisHash {
        size_t operator()(const LzAxis& a) const
        {
            uint64_t h = a.scale_bits * 0x9E3779B97F4A7C15ull;
            for (int v : {a.ssize, a.d0, a.n, a.clamp}) h = (h ^ (uint32_t)v) * 0x100000001B3ull;
            return (size_t)h;
        }
    };
    std::unordered_map<LzAxis, size_t, LzAxisHash> lz_index; // axis -> its first tap
    std::vector<std::pair<LzAxis, size_t>>          lz_axes;  // (axis, first tap), in reservation order
    int32_t axis_taps(int ssize, double scale, int d0, int n, bool clamp);
    void    add(ResizeJob R);
    // The Lanczos4 tap inputs (a sin and a cos per destination column and row), on `pool` when there
    // are enough jobs to pay for it; the device turns them into the taps (the whole taps computed here
    // cost ~75 us per 224x224 record of libm, divisions and rounding: ~1.1 ms per 256-record call on
    // 14 threads, and the LANCZOS4 step was host-bound).
    // They go straight into the call's pinned table (`lz`: n_taps entries; a per-call vector of ~2.8 MB
    // and its copy into the table cost page faults under 14 writers and ~0.1 ms of memcpy).
    void fill_taps(const ParallelFor& pool, LzIn* lz) const;
    static int ksize(int m) { return m == GR_CUBIC ? 4 : (m == GR_LANCZOS4 ? 8 : 2); }
    static int sep_k(int m) { return m == GR_CUBIC ? 4 : m == GR_LANCZOS4 ? 8 : m == GR_LINEAR_AREA ? 2 : 0; }
    // launch classes: the fixed-K methods by K, resizeArea_ jobs, the rest
    static int cls(int m) { return sep_k(m) ? sep_k(m) : m == GR_AREA ? 50 : 99; }
    int  rows_for(int f, int n, int tr) const;
    int  bytes_for(int f, int n, int cw) const;
    Sub  shape(int f, int n) const;
    void finalize();
    static constexpr size_t kGenericLds = 64 * 1024;
    static constexpr size_t kSepLds     = 40 * 1024; // (four bands per CU)
};

// Algorithmic bytes of one launch: the resampled u8 source footprint plus
// the bytes written (KM_STATS / KM_RAW write an HWC uint8 intermediate).
template <typename J_>
double launch_bytes(const std::vector<J_>& jobs, int mode, size_t out_elem);

// The masks of an image + mask call (aeon_hip_augment_pair_batch): 8-bit single-channel records
// without rotation into uint8 items, sharing the images' params.
struct MaskSet {
    const aeon_img_desc* descs;
    const void*          src_base;
    aeon_out_desc        out;
    void*                out_dev;
};

// One run_batch call's plan: its launches in launch order -- rot (image::rotate) -> exp (image::expand) ->
// m16 (the mask gather) -> gr_short / kPre, kWide (resize_short, generic or tile) -> gr_main (CUBIC / LANCZOS4 / AREA
// resize of the crop) -> kPre2 (2x-area resize ahead of photometric stages) -> kPass1 (contrast statistics) ->
// kMain; each reads only what an earlier one wrote -- and, after finalize(), where each one's jobs lie in
// the call's table and what its launch needs.  Reused from call to call (clear() keeps the vectors' memory).
struct CallPlan {
    std::vector<RotJob>    rot;
    std::vector<ExpandJob> exp;
    std::vector<Mask16Job> m16;
    GrPlan                 gr_short, gr_main;
    // the tile launches, one per (resize mode, scalar tail) and for kMain (resize mode, scalar tail,
    // photometric) group: the kernels are specialised on all three
    // kWide: resize_short pre-pass jobs whose window is wider than kWideCols, launched right after kPre's, apart
    // from them: a window's column taps take 8 bytes of LDS a column, and in one launch with records whose
    // staged rows are large the two maxima together passed the workgroup's LDS
    enum { kPre = 0, kPre2 = 8, kPass1 = 16, kMain = 24, kWide = 40, kGroups = 48 };
    static constexpr int kWideCols = 8192;
    LaunchPlan tiles[kGroups];
    size_t     scratch_bytes = 0; // of the slot's scratch, every region 16-aligned with 16 bytes of slack
    int        n_stats       = 0; // contrast records: pass-1 jobs, stats slots

    // -- set by finalize()
    size_t rot_off = 0, m16_off = 0, exp_off = 0; // byte offsets of the job arrays in the table
    size_t blob = 0;      // bytes the host writes (and uploads)
    size_t table_cap = 0; // ... plus the Lanczos4 taps the device builds behind them
    size_t ring_need = 0; // ... plus room for the taps of a call that shares no axis (ensure_ring's sizing)
    int    exp_max_px = 0, m16_max_h = 0, m16_max_w = 0, m16_max_seg = 0, m16_max_slots = 1;
    double m16_bytes = 0; // algorithmic: crop read once + output written once
    int    rot_max_tiles = 0, rot_cn = 0; // (rot_cn: the jobs' common bytes per pixel, or 0)
    int    partial_stride = 1; // (tile, wave) sums per stats slot
    size_t partial_words = 4;
    bool   mask_only = false;  // gather jobs and nothing else (read from the pinned slot, no upload)

    CallPlan();
    void clear(); // for the next call (keeps the vectors' memory)
    // One record: the gather pass (pixel masks without rotation, every 16-bit record), the image path, or
    // refused.  add_records: a call's records, then the masks of a pair call as gather jobs.
    void add(const aeon_img_desc& d, const void* src_base, const aeon_aug_params& p, const aeon_out_desc& o, uint64_t item,
             bool is_mask, const ItemMap* im = nullptr);
    void add_gather(const aeon_img_desc& d, const void* src_base, const aeon_aug_params& p, const aeon_out_desc& o,
                    uint64_t item, bool is_mask);
    void add_records(int n, const aeon_img_desc* descs, const void* src_base, const aeon_aug_params* params,
                     const aeon_out_desc& o, void* out_dev, bool is_mask, const MaskSet* ms, const ItemMap* im);
    // Launch shapes, tile counts, table offsets (tap offsets made absolute) and the launch maxima; `o` is
    // what the kernels write (out_view).
    void finalize(const aeon_out_desc& o);
    // The table's host-written bytes [0, blob) into `table`, scratch offsets relocated to `scratch`, the
    // Lanczos4 tap inputs computed (on `pool` when it pays).
    void write(uint8_t* table, uint64_t scratch, const ParallelFor& pool);

private:
    size_t        reserve(size_t bytes); // a scratch region: its offset
    const RotJob& rotate(const aeon_img_desc& d, uint64_t src, const aeon_aug_params& p, int cn, int interp, bool window);
    void          push(int pass, const AugJob& J);
    bool             vec_ok = true; // every final output 16-byte aligned, win_w % 4 == 0, no canvas
    std::vector<int> slot_tiles;    // tiles of each stats slot's pass-1 job
};

} // namespace aeon_hip
