// context.hpp -- the per-GPU context (aeon_hip_ctx) behind the device half of the C ABI: its staging ring
// and the scoped lease a call holds on one slot of it, timers, per-stream error words, and the services
// context.cpp implements for the image path (image_path.cpp) and the target calls (targets.cpp).  Private to
// the library, not installed.  The small per-call helpers are inline here: they sit on the host path of every
// call (a C2 step's submit is ~14 us).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/aeon_hip.h"
#include "aug_job.hpp"
#include "error.hpp"
#include "host.hpp"
#include "jpeg.hpp"
#include "plan.hpp"

#define HIP_OK(expr)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) fail(AEON_HIP_ERUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace aeon_hip {

// ---------------------------------------------------------------------------------------------
// Context: per-GPU state and a 16-deep staging ring (pinned host blob -> device blob per call)
// ---------------------------------------------------------------------------------------------
struct Slot {
    hipEvent_t done     = nullptr; // the slot's kernels finished (host reuses the slot after it)
    hipEvent_t copied   = nullptr; // the slot's job table reached the device
    bool       pending  = false; // the slot's kernels may still run: wait for slots[cover].done
    int        cover    = -1;
    uint8_t*   host     = nullptr;
    size_t     host_cap = 0;
    uint8_t*   host_dev = nullptr; // device view of `host` (zero-copy job tables)
    uint8_t*   dev      = nullptr;
    size_t     dev_cap  = 0;
    uint8_t*   vram     = nullptr; // job tables the host writes straight into HBM (uncached, through the BAR)
    size_t     vram_cap = 0;
    uint8_t*   scratch  = nullptr;
    size_t     scratch_cap = 0;
    uint32_t*  partials = nullptr;
    size_t     partials_cap = 0;
    double*    shifts = nullptr; // contrast (1-c)*mean per stats slot (contrast_reduce)
    size_t     shifts_cap = 0;
};

struct PngStage; // image_path.cpp
void png_stage_destroy(PngStage* s);

constexpr int kTimerJpeg = 3; // KernelTimer kind of the JPEG kernels (after the KernelMode kinds)
constexpr int kTimerPng  = 4; // ... of the PNG and pixmap decode kernels
struct KernelTimer {
    hipEvent_t start, stop;
    int        kind;   // KernelMode, kTimerJpeg or kTimerPng
    double     bytes;  // algorithmic bytes of the launch
};

} // namespace aeon_hip

// Owns everything it allocates: the destructor (context.cpp) is aeon_hip_ctx_destroy's teardown, and
// tolerates a context that aeon_hip_ctx_create gave up on half-way.
struct aeon_hip_ctx {
    using Slot        = aeon_hip::Slot;
    using KernelTimer = aeon_hip::KernelTimer;
    aeon_hip_ctx()    = default;
    ~aeon_hip_ctx();
    aeon_hip_ctx(const aeon_hip_ctx&)            = delete;
    aeon_hip_ctx& operator=(const aeon_hip_ctx&) = delete;

    int        device = 0;
    int32_t*   d_error = nullptr; // kErrWords device error words: [0] the null stream's (and overflow),
                                  // [i] the i-th stream's (stream_error)
    static constexpr int kErrWords = 64;
    hipStream_t err_stream[kErrWords] = {};
    bool        err_unread[kErrWords] = {}; // handed back without having been read: cleared for its next owner
    std::mutex  err_mu;
    int32_t*    call_error = nullptr; // the word of the call in progress (run_batch, under mu)
    uint32_t*  d_tail  = nullptr; // per ring slot: dynamic-tail tile counters (zero between launches)
    int32_t*   d_hsv   = nullptr;
    // staging ring: a slot (job table, scratch) is reused only after the kernels that read it
    // finished.  A completion event is recorded once per `done_every` calls on a stream and
    // covers the calls since the previous one (each event costs GPU time between launches).
    static constexpr int kSlots = 16;
    Slot       slots[kSlots];
    int        next = 0;
    int        done_every = 8;
    size_t     table_cap = 0, partials_cap = 0, shifts_cap = 0; // per-slot capacities (ensure_ring)
    // direct calls (run_direct): records of one job each, one launch group: the tile kernel reads
    // the jobs from the pinned slot itself
    bool                 direct = true; // AEON_HIP_DIRECT=0: the multi-pass path (device job table) for every call
    bool                 records = true; // AEON_HIP_RECORDS=0: contrast calls through the two-launch path
    bool                 fuse_masks = false; // AEON_HIP_FUSE_MASKS=1: a pair call's masks inside the image launch
    bool                 vram_jobs = false; // job tables written by the host into device memory (large-BAR GPUs;
                                            // AEON_HIP_VRAM_JOBS=0: pinned host tables)
    bool                 jpeg_gpu_huff = true; // AEON_HIP_JPEG_HUFF=host: every JPEG through the host entropy decoder
    int                  jpeg_huff_lanes = 0;  // AEON_HIP_JPEG_HUFF_LANES=256 / 512 / 1024 (0: jpeg.hpp's kHuffLanes)
    std::vector<aeon_hip::JobGeom> geoms;        // reused per call
    std::vector<aeon_hip::AugJob>  direct_jobs;  // (run_direct) the call's jobs before they go into the slot
    std::vector<int>     direct_order;       // (run_direct) their table order: largest crop first
    aeon_hip::CallPlan   plan;               // (run_batch) the call's plan
    aeon_hip::JpegState* jpeg = nullptr;     // JPEG decode stage (pool, staging ring), on first use
    aeon_hip::PngStage*  png  = nullptr;     // PNG decode stage (staging ring, scratch), on first use
    aeon_hip::PngStage*  pixmap = nullptr;   // pixmap decode stage: a staging ring of its own (no scratch), on first use
    aeon_hip::PngStage*  tiff = nullptr;     // TIFF decode stage (staging ring, scratch of the decoded strips), on first use
    aeon_hip::thread_pool* host_pool = nullptr; // the owning decoder's pool (ctx_share_pool), for the JPEG stage
    // localization_rcnn: the anchor table of the last config seen stays resident (uploaded once), and the
    // direct call's engine end states pass through a small device array
    std::vector<float>   rcnn_anchors_host;
    float*               rcnn_anchors_dev = nullptr;
    uint64_t             rcnn_anchors_key = 0; // aeon_rcnn_out::anchors_key of the resident table (0: none given)
    uint32_t*            rcnn_states_dev  = nullptr;
    size_t               rcnn_states_cap  = 0;
    std::unique_ptr<aeon_hip::thread_pool> plan_pool; // the context's own, made for the first call with many Lanczos4 taps
    std::vector<int> open_slots; // used since the last completion event, on open_stream
    hipStream_t      open_stream = nullptr;
    // job tables go up on their own stream, so a call's H2D overlaps the previous call's kernels
    // instead of queueing between them on the caller's stream
    hipStream_t copy_stream = nullptr;
    int         n_cu      = 0;
    std::vector<std::pair<std::vector<int>, int>> occ; // launch shape -> workgroups per CU
    // standardize LUTs stay resident per distinct output config (a new one is uploaded once)
    struct Lut {
        float  host[768];
        float* dev = nullptr;
    };
    std::vector<Lut> luts;
    aeon_out_desc    lut_memo_od{}; // the last resident_lut call: its config and LUT
    bool             lut_memo_u8  = false;
    const float*     lut_memo_dev = nullptr;
    // per-launch timing events on every `timing_every`-th call only (they cost GPU time)
    int         timing_every = 1;
    long        timing_calls = 0;
    std::mutex mu;
    // optional per-launch timing (aeon_hip_set_timing): events recorded on the launch stream
    bool                     timing = false;
    std::vector<KernelTimer> timers, free_timers;
    double                   ms[AEON_HIP_TIMER_KINDS]    = {};
    // AEON_HIP_HOST_PROFILE=1: host time per run_batch phase, printed when the context is destroyed
    bool                     host_profile = false;
    std::vector<double>      host_ns[8];  // per call, per phase
    long                     host_calls   = 0;
    double                   bytes[AEON_HIP_TIMER_KINDS] = {};
    long                     count[AEON_HIP_TIMER_KINDS] = {};
#ifdef AEON_HIP_TRACE
    uint32_t*                trace = nullptr; // AEON_HIP_TRACE_PTR, read once at ctx_create
#endif
};

namespace aeon_hip {

// ---- services of context.cpp ----------------------------------------------------------------
// p regrown to at least `need` bytes of pinned host or device memory (its content is not kept).
void grow(uint8_t*& p, size_t& cap, size_t need, bool pinned);
// Wait until no kernel of any ring slot can still be running.
void drain_ring(aeon_hip_ctx* ctx);
// Every slot's job table, contrast sums and shifts at these capacities at least.
void ensure_ring(aeon_hip_ctx* ctx, size_t table, size_t partials, size_t shifts);
// Device copy of the standardize LUT of output config `o` (uploaded the first time it is seen).
const float* resident_lut(aeon_hip_ctx* ctx, const aeon_out_desc& o, bool u8_map = false);

constexpr size_t kVramTableMax = 1 << 20; // the most a slot's HBM table holds (publish_table)

// One completion event after the open slots' kernels (on their stream) covers all of them.
inline void close_slots(aeon_hip_ctx* ctx)
{
    if (ctx->open_slots.empty()) return;
    const int last = ctx->open_slots.back();
    HIP_OK(hipEventRecord(ctx->slots[last].done, ctx->open_stream));
    for (int i : ctx->open_slots) ctx->slots[i].pending = true, ctx->slots[i].cover = last;
    ctx->open_slots.clear();
}

// A call's hold on the next ring slot for its launches on `stream`, taken under ctx->mu once the kernels that
// last used the slot are done.  release(), after the call's launches are enqueued, leaves the slot busy until a
// completion event covers it.  A call that throws in between unwinds through the destructor, which only
// lists the slot as open on `stream` -- kernels of the call may already be enqueued, so the next completion
// event there has to cover it before the slot's table is written again -- and makes no runtime call.
struct SlotLease {
    aeon_hip_ctx* ctx;
    hipStream_t   stream;
    int           index;
    bool          held = true;

    SlotLease(aeon_hip_ctx* c, hipStream_t st) : ctx(c), stream(st)
    {
        // calls on another stream than the open ones: close those with an event on their stream
        if (!ctx->open_slots.empty() && ctx->open_stream != stream) close_slots(ctx);
        index     = ctx->next;
        Slot& s   = ctx->slots[index];
        ctx->next = (ctx->next + 1) % aeon_hip_ctx::kSlots;
        if (s.pending) {
            HIP_OK(hipEventSynchronize(ctx->slots[s.cover].done));
            s.pending = false;
        }
    }
    SlotLease(const SlotLease&)            = delete;
    SlotLease& operator=(const SlotLease&) = delete;
    Slot& slot() const { return ctx->slots[index]; }
    void  release()
    {
        held = false;
        ctx->open_slots.push_back(index);
        ctx->open_stream = stream;
        if ((int)ctx->open_slots.size() >= ctx->done_every) close_slots(ctx);
        ctx->host_calls++;
    }
    ~SlotLease()
    {
        if (!held) return;
        try {
            ctx->open_slots.push_back(index);
            ctx->open_stream = stream;
        } catch (...) { // (out of memory for the list: nothing more to do while unwinding)
        }
    }
};

inline KernelTimer take_timer(aeon_hip_ctx* ctx, int kind, double bytes)
{
    KernelTimer t{};
    if (!ctx->free_timers.empty()) {
        t = ctx->free_timers.back();
        ctx->free_timers.pop_back();
    } else {
        // timing only: no system-scope fence (cache writeback + invalidate) when they complete,
        // which cost the stream ~11 us of idle GPU per timed launch
        HIP_OK(hipEventCreateWithFlags(&t.start, hipEventDisableSystemFence));
        HIP_OK(hipEventCreateWithFlags(&t.stop, hipEventDisableSystemFence));
    }
    t.kind  = kind;
    t.bytes = bytes;
    return t;
}

// Per-launch timing events on one call in timing_every (each event pair costs GPU time between launches).
inline bool take_timing(aeon_hip_ctx* ctx)
{
    return ctx->timing && (ctx->timing_calls++ % ctx->timing_every) == ctx->timing_every - 1;
}

// The device error word of the calls on `stream`: each stream its own (so that aeon_hip_synchronize of
// one stream -- a decode window -- never reads or clears a bit another stream's kernels set meanwhile),
// the null stream and streams beyond the table's size share word 0.  A stream keeps its word until
// aeon_hip_synchronize has read it or aeon_hip_release_stream gives the stream up
// (release_stream_error).  A word that was given up unread may hold bits: it is cleared on its new
// owner's stream ahead of that stream's first kernel -- the old owner's work is complete by then (the
// contract of aeon_hip_release_stream), so no old bit arrives after the clear, and the clear is ordered
// before every kernel of the new owner, so none of theirs is lost.
inline int32_t* stream_error(aeon_hip_ctx* ctx, hipStream_t stream)
{
    if (!stream) return ctx->d_error;
    std::lock_guard<std::mutex> lock(ctx->err_mu);
    int free_i = 0;
    for (int i = 1; i < aeon_hip_ctx::kErrWords; i++) {
        if (ctx->err_stream[i] == stream) return ctx->d_error + i;
        if (!free_i && !ctx->err_stream[i]) free_i = i;
    }
    if (!free_i) return ctx->d_error;
    if (ctx->err_unread[free_i]) {
        HIP_OK(hipMemsetAsync(ctx->d_error + free_i, 0, sizeof(int32_t), stream));
        ctx->err_unread[free_i] = false;
    }
    ctx->err_stream[free_i] = stream;
    return ctx->d_error + free_i;
}

// `stream` gives its word (if it has one) back to the table.  unread: nobody looked at the word, so it
// may hold bits (see above); else aeon_hip_synchronize has read it and left it zero.
inline void release_stream_error(aeon_hip_ctx* ctx, hipStream_t stream, bool unread)
{
    if (!stream) return;
    std::lock_guard<std::mutex> lock(ctx->err_mu);
    for (int i = 1; i < aeon_hip_ctx::kErrWords; i++)
        if (ctx->err_stream[i] == stream) {
            ctx->err_stream[i] = nullptr;
            ctx->err_unread[i] = unread;
        }
}

// A table the host wrote into s.vram is published to the launches behind it: a full fence so the
// write-combined writes reach the device ahead of the launch's doorbell, then a read back through the BAR
// -- PCIe does not let a read pass the posted writes ahead of it, so the table is in HBM when it returns
// (~1 us of host time; the host runs ahead of the GPU).
inline const uint8_t* publish_written(Slot& s, size_t bytes)
{
    std::atomic_thread_fence(std::memory_order_seq_cst);
    (void)*(volatile const uint32_t*)(s.vram + ((bytes - 1) & ~(size_t)3));
    return s.vram;
}

// A call's job table (written in the slot's pinned `host` buffer) published where its kernels read it
// with device-memory latency: copied by the host into the slot's HBM table through the PCIe BAR (one
// contiguous copy), then publish_written.  Null when the context has no such tables.  (C2: the workgroups'
// first job fetch waited 3.7 us over PCIe from pinned memory, 0.3 us from HBM; tools/trace_kernel.py.)
inline const uint8_t* publish_table(aeon_hip_ctx* ctx, Slot& s, size_t bytes)
{
    if (!ctx->vram_jobs || bytes == 0 || bytes > kVramTableMax || bytes > s.vram_cap) return nullptr;
    std::memcpy(s.vram, s.host, bytes);
    return publish_written(s, bytes);
}

} // namespace aeon_hip
