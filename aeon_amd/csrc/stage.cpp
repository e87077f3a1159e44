// stage.cpp -- device side of the HIP augmentation stage's host code: the per-GPU context with its
// pinned/device staging ring, kernel launches and the extern "C" boundary (include/aeon_hip.h).  The
// image path's per-record planning and table layout are plan.cpp's (host arithmetic only); run_batch
// acts on the CallPlan it returns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"
#include "aug_job.hpp"
#include "box_job.hpp"
#include "rcnn_job.hpp"
#include "host.hpp"
#include "jpeg.hpp"
#include "mask16.hpp"
#include "json.hpp"
#include "param_factory.hpp"
#include "plan.hpp"
#include "plan_record.hpp"
#include "video_job.hpp"

namespace aeon_hip {
hipError_t launch_tiles(int km, int rm, bool tail, bool photo, const LaunchArgs& a, int grid, hipStream_t stream,
                        hipEvent_t start, hipEvent_t stop);
hipError_t launch_contrast_reduce(const LaunchArgs& a, int n_jobs, hipStream_t stream);
hipError_t kernel_occupancy(int km, int rm, bool tail, bool photo, const LaunchArgs& a, int* blocks);
hipError_t set_kernel_lds_limit(int bytes);
hipError_t launch_transpose(const void* src, void* dst, int64_t rows, int64_t cols, int element_size,
                            hipStream_t stream);
hipError_t launch_rotate(const RotJob* jobs, int n_jobs, int max_tiles, int words, int cn, int32_t* error,
                         hipStream_t stream);
int        rot_box_words(int angle);
hipError_t launch_expand(const ExpandJob* jobs, int n_jobs, int max_pixels, hipStream_t stream);
hipError_t launch_nearest(const Mask16Job* jobs, int n_jobs, int max_h, int max_w, int max_seg_bytes, int max_slots, hipStream_t stream,
                          hipEvent_t start, hipEvent_t stop);
hipError_t launch_upload_table(const void* host_dev, void* dst, size_t bytes, hipStream_t stream);
hipError_t launch_contrast_records(bool fast, bool split, const LaunchArgs& a, const RecArgs& r, int grid, hipStream_t stream,
                                   hipEvent_t start, hipEvent_t stop);
hipError_t contrast_records_lds_limit(int bytes);
hipError_t launch_box_targets(const BoxLaunch& L, hipStream_t stream);
hipError_t launch_rcnn_targets(const RcnnLaunch& L, hipStream_t stream);
hipError_t launch_clip_pad(const PadRegion* regions, int n_regions, uint64_t max_bytes, hipStream_t stream);
hipError_t launch_resize_generic(const ResizeJob* jobs, const uint8_t* table, int n_jobs, int max_tiles, int TR, int CW,
                                 int NR, int xs, int amax, int cn_max, int SW, const float* lut, int bgr, int chm,
                                 int32_t* error, hipStream_t stream);
hipError_t launch_lanczos4_taps(const LzIn* in, GrTap* out, int n, hipStream_t stream);
hipError_t launch_resize_sep(int K, bool area, const ResizeJob* jobs, const uint8_t* table, int n_jobs, int max_tiles, int TR, int CW,
                             int NR, int SW, int cn, const float* lut, int bgr, int chm, int32_t* error, hipStream_t stream);
void       jpeg_decode_batch(JpegState* S, int n, const void* const* data, const size_t* sizes,
                             const aeon_img_desc* descs, void* dst_base, int32_t* error, hipStream_t stream,
                             hipEvent_t start, hipEvent_t stop);
void       jpeg_info(const void* data, size_t size, int* w, int* h, int* ncomp);
void       jpeg_entropy_only(const void* data, size_t size, int* w, int* h, int* ncomp, int64_t* n_blocks,
                             int64_t* n_values, uint64_t* hash);
void       jpeg_host_stage(const void* data, size_t size, int* gpu_entropy, int64_t* staged_bytes);
void       png_header(const void* data, size_t size, int* w, int* h, int* depth, int* ctype);
void       png_decode(const void* data, size_t size, int mode, void* dst, size_t stride, int* out_elem_bytes);
} // namespace aeon_hip

using namespace aeon_hip;

namespace {

thread_local std::string g_err;

// The device error word's bits (kernels atomicOr them; aeon_hip_synchronize reports and clears).
std::string device_error_text(int err)
{
    static const struct {
        int         bit;
        const char* what;
    } bits[] = {{2, "LDS staging footprint exceeded"},
                {4, "dynamic LDS not at address 0"},
                {16, "hue table without a t1 channel"},
                {32, "dynamic-tail counter left over by an earlier launch"},
                {64, "rotation source box exceeds the launch's LDS"},
                {128, "generic resize footprint exceeds the launch's LDS"},
                {256, "JPEG entropy-coded data corrupt or truncated (GPU Huffman decoder)"},
                {512, "separable resize band wider than its workgroup"}};
    std::string s;
    for (const auto& b : bits)
        if (err & b.bit) s += (s.empty() ? "" : "; ") + std::string(b.what);
    return s.empty() ? "unknown" : s;
}

#define HIP_OK(expr)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) fail(AEON_HIP_ERUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#ifndef AEON_HIP_UPLOAD_KERNEL_MAX_KB
#define AEON_HIP_UPLOAD_KERNEL_MAX_KB 128
#endif
constexpr size_t kUploadKernelMax = AEON_HIP_UPLOAD_KERNEL_MAX_KB * 1024; // job tables above this go up by SDMA (run_batch)
constexpr size_t kDirectFetchMax  = 512 * 1024; // run_direct: most job bytes a launch's tiles read over PCIe

// ---------------------------------------------------------------------------------------------
// Per-image constants (aeon computes these on the host per record, too)
// ---------------------------------------------------------------------------------------------

// image::standardize arithmetic (src/image.cpp:129-174 over OpenCV 2.4 arithm_op: f64 work
// type per op, rounded to f32 after each op) tabulated per channel and input value.
void build_lut(const aeon_out_desc& o, float* lut, bool u8_map = false)
{
    if (u8_map) {
        // fixed_aspect_ratio's in-place standardize of its uint8 canvas (etl_image.cpp:263-300 ->
        // image.cpp:129-174 on CV_8U planes): OpenCV 2.4 arithm_op on 8U -- multiply(1/255.) in
        // double, subtract the mean converted to int (cvRound, add/sub rule), multiply(1/stddev)
        // in double -- each saturated to uint8
        for (int c = 0; c < 3; c++) {
            const int oc = (o.bgr_to_rgb && o.channels == 3) ? 2 - c : c;
            for (int x = 0; x < 256; x++) {
                if (oc >= o.channels) {
                    lut[c * 256 + x] = (float)x;
                    continue;
                }
                auto sat = [](int v) { return std::min(std::max(v, 0), 255); };
                int  a   = sat(cv_round((double)x * (1. / 255.)));
                a        = sat(a - cv_round(o.mean[oc]));
                if (o.stddev[oc] != 0) a = sat(cv_round((double)a * (1. / o.stddev[oc])));
                lut[c * 256 + x] = (float)a;
            }
        }
        return;
    }
    // indexed by SOURCE channel c; its value lands in output channel oc (mixChannels
    // from_to {0,2,1,1,2,0} when bgr_to_rgb), standardized with that channel's mean/stddev
    for (int c = 0; c < 3; c++) {
        const int oc = (o.bgr_to_rgb && o.channels == 3) ? 2 - c : c;
        for (int x = 0; x < 256; x++) {
            if (!o.has_mean || oc >= o.channels) {
                lut[c * 256 + x] = (float)x;
                continue;
            }
            float t1 = (float)((double)(float)x * (1. / 255.));
            float t2 = (float)((double)t1 - o.mean[oc]);
            lut[c * 256 + x] = o.stddev[oc] != 0 ? (float)((double)t2 * (1. / o.stddev[oc])) : t2;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Context: per-GPU state and a 4-deep staging ring (pinned host blob -> device blob per call)
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

} // namespace

constexpr int kTimerJpeg = 3; // KernelTimer kind of the JPEG kernels (after the KernelMode kinds)
struct KernelTimer {
    hipEvent_t start, stop;
    int        kind;   // KernelMode, or kTimerJpeg
    double     bytes;  // algorithmic bytes of the launch
};

struct aeon_hip_ctx {
    int        device = 0;
    int32_t*   d_error = nullptr; // kErrWords device error words: [0] the null stream's (and overflow),
                                  // [i] the i-th stream's (stream_error)
    static constexpr int kErrWords = 64;
    hipStream_t err_stream[kErrWords] = {};
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
    std::vector<JobGeom> geoms;              // reused per call
    std::vector<AugJob>  direct_jobs;        // (run_direct) the call's jobs before they go into the slot
    std::vector<int>     direct_order;       // (run_direct) their table order: largest crop first
    CallPlan             plan;               // (run_batch) the call's plan
    JpegState*           jpeg = nullptr;     // JPEG decode stage (pool, staging ring), on first use
    thread_pool*         host_pool = nullptr; // the owning decoder's pool (ctx_share_pool), for the JPEG stage
    // localization_rcnn: the anchor table of the last config seen stays resident (uploaded once), and the
    // direct call's engine end states pass through a small device array
    std::vector<float>   rcnn_anchors_host;
    float*               rcnn_anchors_dev = nullptr;
    uint64_t             rcnn_anchors_key = 0; // aeon_rcnn_out::anchors_key of the resident table (0: none given)
    uint32_t*            rcnn_states_dev  = nullptr;
    size_t               rcnn_states_cap  = 0;
    std::unique_ptr<thread_pool> plan_pool;        // the context's own, made for the first call with many Lanczos4 taps
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
    double                   ms[4]    = {0, 0, 0, 0};
    // AEON_HIP_HOST_PROFILE=1: host time per run_batch phase, printed when the context is destroyed
    bool                     host_profile = false;
    std::vector<double>      host_ns[8];  // per call, per phase
    long                     host_calls   = 0;
    double                   bytes[4] = {0, 0, 0, 0};
    long                     count[4] = {0, 0, 0, 0};
#ifdef AEON_HIP_TRACE
    uint32_t*                trace = nullptr; // AEON_HIP_TRACE_PTR, read once at ctx_create
#endif
};

struct aeon_param_factory {
    param_factory f;
    std::mutex    mu; // make_params calls are serialised (the lighting normal_distribution caches a draw)
    explicit aeon_param_factory(const Json& j) : f(j) {}
};

namespace {

void grow(uint8_t*& p, size_t& cap, size_t need, bool pinned)
{
    if (need <= cap) return;
    size_t n = std::max(need, cap * 2);
    if (p) HIP_OK(pinned ? hipHostFree(p) : hipFree(p));
    p   = nullptr;
    cap = 0;
    if (pinned) HIP_OK(hipHostMalloc((void**)&p, n, hipHostMallocDefault));
    else HIP_OK(hipMalloc((void**)&p, n));
    cap = n;
}

void close_slots(aeon_hip_ctx* ctx);

// Device memory the host writes directly (a large-BAR GPU maps all of it): uncached, so every GPU read
// of it -- a kernel's job fetch -- goes to HBM and never meets a stale cache line of the slot's
// previous call.
// The host may write through p when the page holding it is mapped read-write into this process (on a
// large-BAR GPU the driver maps host-visible VRAM at the allocation's own address; a restricted or
// virtualised BAR can allocate device memory without mapping it for the CPU, and the runtime reports no
// host pointer for device memory either way).  Checked in /proc/self/maps -- no signal handlers, nothing
// process-wide touched, safe next to other threads -- then one write + read-back through p.
bool host_mapped_rw(const void* p, size_t bytes)
{
    std::FILE* f = std::fopen("/proc/self/maps", "r");
    if (!f) return false;
    const unsigned long a  = (unsigned long)(uintptr_t)p;
    bool                ok = false;
    char                line[512];
    while (std::fgets(line, sizeof line, f)) {
        unsigned long lo = 0, hi = 0;
        char          perms[8] = {0};
        if (std::sscanf(line, "%lx-%lx %7s", &lo, &hi, perms) != 3) continue;
        if (a >= lo && a < hi) {
            ok = a + bytes <= hi && perms[0] == 'r' && perms[1] == 'w';
            break;
        }
    }
    std::fclose(f);
    return ok;
}
bool host_can_write(void* p)
{
    if (!host_mapped_rw(p, sizeof(uint32_t))) return false;
    volatile uint32_t* q = (volatile uint32_t*)p;
    q[0]                 = 0xA5C3E1F7u;
    return q[0] == 0xA5C3E1F7u;
}

// The uncached HBM tables are never handed back to the driver: a context's tables go into a process-wide
// pool when it is destroyed (or grows them) and the next context takes them from there.  Measured on the
// MI355X boxes: once an uncached block had been freed, a later ordinary device allocation that reused its
// memory lost writes -- 128-byte lines of a kernel's output read back as zeros by the next kernel on the
// stream (tests/test_decoder.py after the stager and JPEG tests: 1-2.7 KB of one record, in 3 of 3
// runs; with the pool, 0 of 2; with cached tables, or pinned ones, 0 of 4).
std::mutex                               g_vram_pool_mu;
std::vector<std::pair<uint8_t*, size_t>> g_vram_pool;   // released tables, still allocated and mapped
std::vector<uint8_t*>                    g_vram_unused; // blocks whose probe failed (kept, never used)
std::vector<std::pair<uint8_t*, size_t>> g_vram_all;    // every uncached block of the process (diagnostics)
void free_vram(uint8_t*& p, size_t& cap)
{
    if (p) {
        std::lock_guard<std::mutex> lock(g_vram_pool_mu);
        g_vram_pool.emplace_back(p, cap);
    }
    p = nullptr, cap = 0;
}

bool grow_vram(int device, uint8_t*& p, size_t& cap, size_t need) // false: no table (p released)
{
    if (need <= cap) return true;
    const size_t n = std::max(need, cap * 2);
    free_vram(p, cap);
    {
        std::lock_guard<std::mutex> lock(g_vram_pool_mu); // the smallest pooled block of this device that fits
        size_t best = g_vram_pool.size();
        for (size_t i = 0; i < g_vram_pool.size(); i++) {
            hipPointerAttribute_t at{};
            if (g_vram_pool[i].second < n || hipPointerGetAttributes(&at, g_vram_pool[i].first) != hipSuccess ||
                at.device != device)
                continue;
            if (best == g_vram_pool.size() || g_vram_pool[i].second < g_vram_pool[best].second) best = i;
        }
        (void)hipGetLastError();
        if (best < g_vram_pool.size()) {
            p = g_vram_pool[best].first, cap = g_vram_pool[best].second;
            g_vram_pool.erase(g_vram_pool.begin() + (long)best);
            return true;
        }
    }
    if (hipExtMallocWithFlags((void**)&p, n, hipDeviceMallocUncached) != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        return false;
    }
    {
        std::lock_guard<std::mutex> lock(g_vram_pool_mu);
        g_vram_all.emplace_back(p, n);
    }
    // the host writes these tables through p itself: only when p's page is mapped read-write for the
    // host and a write + read-back through p works (a restricted BAR or a virtualised GPU can allocate it without mapping it for the
    // CPU; the runtime reports no host pointer for device memory either way) -- the pinned paths then
    if (!host_can_write(p)) {
        (void)hipGetLastError();
        if (std::getenv("AEON_HIP_HOST_PROFILE"))
            std::fprintf(stderr, "[aeon_hip] uncached HBM block not host-writable: pinned job tables\n");
        std::lock_guard<std::mutex> lock(g_vram_pool_mu);
        g_vram_unused.push_back(p); // (not freed either: see above)
        p = nullptr;
        return false;
    }
    cap = n;
    return true;
}

// A call's job table (written in the slot's pinned `host` buffer) published where its kernels read it
// with device-memory latency: copied by the host into the slot's HBM table through the PCIe BAR
// (write-combined: one contiguous copy, then a full fence so the writes reach the device ahead of the
// launch's doorbell).  Null when the context has no such tables.  (C2: the workgroups' first job
// fetch waited 3.7 us over PCIe from pinned memory, 0.3 us from HBM; tools/trace_kernel.py.)
constexpr size_t kVramTableMax = 1 << 20;
const uint8_t* publish_table(aeon_hip_ctx* ctx, Slot& s, size_t bytes)
{
    if (!ctx->vram_jobs || bytes == 0 || bytes > kVramTableMax || bytes > s.vram_cap) return nullptr;
    std::memcpy(s.vram, s.host, bytes);
    std::atomic_thread_fence(std::memory_order_seq_cst);
    // a read back through the BAR: PCIe does not let a read pass the posted writes ahead of it, so
    // the table is in HBM when it returns (~1 us of host time; the host runs ahead of the GPU)
    (void)*(volatile const uint32_t*)(s.vram + ((bytes - 1) & ~(size_t)3));
    return s.vram;
}

// publish_table for a table the host wrote into s.vram itself: the fence and the read-back only.
const uint8_t* publish_written(Slot& s, size_t bytes)
{
    std::atomic_thread_fence(std::memory_order_seq_cst);
    (void)*(volatile const uint32_t*)(s.vram + ((bytes - 1) & ~(size_t)3));
    return s.vram;
}

// Wait until no kernel of any ring slot can still be running.
void drain_ring(aeon_hip_ctx* ctx)
{
    close_slots(ctx);
    for (Slot& q : ctx->slots)
        if (q.pending) {
            HIP_OK(hipEventSynchronize(ctx->slots[q.cover].done));
            q.pending = false;
        }
}

// Ring capacities are shared by all slots and grown for all of them at once (after draining the
// ring), so the first call -- a warmup -- allocates everything the steady state needs and later
// calls never pay an allocation when they rotate onto a slot they have not used before.
void ensure_ring(aeon_hip_ctx* ctx, size_t table, size_t partials, size_t shifts)
{
    table = std::max<size_t>(table, 16);
    if (table <= ctx->table_cap && partials <= ctx->partials_cap && shifts <= ctx->shifts_cap) return;
    drain_ring(ctx);
    // (a quarter over the first need: a call's tables vary with its records' crops, and a later call
    // needing a few bytes more would otherwise reallocate every slot inside a loader's steady state --
    // ~10-20 ms of pinned and device allocations, seen as one-off stalls of the LANCZOS4 step)
    const size_t tc = table > ctx->table_cap ? std::max(table + table / 4, ctx->table_cap * 2) : ctx->table_cap;
    const size_t pc = partials > ctx->partials_cap ? std::max(partials + partials / 4, ctx->partials_cap * 2) : ctx->partials_cap;
    const size_t sc = shifts > ctx->shifts_cap ? std::max(shifts + shifts / 4, ctx->shifts_cap * 2) : ctx->shifts_cap;
    for (Slot& q : ctx->slots) {
        grow(q.host, q.host_cap, tc, true);
        HIP_OK(hipHostGetDevicePointer((void**)&q.host_dev, q.host, 0));
        grow(q.dev, q.dev_cap, tc, false);
        if (ctx->vram_jobs && !grow_vram(ctx->device, q.vram, q.vram_cap, std::min(tc, kVramTableMax))) {
            ctx->vram_jobs = false; // (no HBM tables on this device: the pinned paths)
            for (Slot& v : ctx->slots)
                free_vram(v.vram, v.vram_cap);
        }
        uint8_t* p = (uint8_t*)q.partials;
        grow(p, q.partials_cap, pc, false);
        q.partials = (uint32_t*)p;
        uint8_t* r = (uint8_t*)q.shifts;
        grow(r, q.shifts_cap, sc, false);
        q.shifts = (double*)r;
    }
    ctx->table_cap = tc, ctx->partials_cap = pc, ctx->shifts_cap = sc;
}

// Device copy of the standardize LUT of output config `o` (uploaded the first time it is seen).
const float* resident_lut(aeon_hip_ctx* ctx, const aeon_out_desc& o, bool u8_map = false)
{
    // the last call's output config again (a loader's steady state): its LUT without rebuilding it
    if (ctx->lut_memo_dev && ctx->lut_memo_u8 == u8_map && std::memcmp(&ctx->lut_memo_od, &o, sizeof(o)) == 0)
        return ctx->lut_memo_dev;
    float lut[768];
    build_lut(o, lut, u8_map);
    const float* dev = nullptr;
    for (auto& L : ctx->luts)
        if (std::memcmp(L.host, lut, sizeof(lut)) == 0) dev = L.dev;
    if (!dev) {
        if (ctx->luts.size() >= 16) { // many configs on one context: start over once the device is idle
            HIP_OK(hipDeviceSynchronize());
            for (auto& L : ctx->luts) HIP_OK(hipFree(L.dev));
            ctx->luts.clear();
        }
        aeon_hip_ctx::Lut L;
        std::memcpy(L.host, lut, sizeof(lut));
        HIP_OK(hipMalloc((void**)&L.dev, sizeof(lut)));
        HIP_OK(hipMemcpy(L.dev, lut, sizeof(lut), hipMemcpyHostToDevice));
        ctx->luts.push_back(L);
        dev = L.dev;
    }
    ctx->lut_memo_od  = o;
    ctx->lut_memo_u8  = u8_map;
    ctx->lut_memo_dev = dev;
    return dev;
}

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

// One completion event after the open slots' kernels (on their stream) covers all of them.
void close_slots(aeon_hip_ctx* ctx)
{
    if (ctx->open_slots.empty()) return;
    const int last = ctx->open_slots.back();
    HIP_OK(hipEventRecord(ctx->slots[last].done, ctx->open_stream));
    for (int i : ctx->open_slots) ctx->slots[i].pending = true, ctx->slots[i].cover = last;
    ctx->open_slots.clear();
}

KernelTimer take_timer(aeon_hip_ctx* ctx, int kind, double bytes)
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

// Per-launch timing events on one call in timing_every (each event pair costs GPU time between launches).
bool take_timing(aeon_hip_ctx* ctx)
{
    return ctx->timing && (ctx->timing_calls++ % ctx->timing_every) == ctx->timing_every - 1;
}

// fixed_aspect_ratio: std::fill_n of each item's canvas, its whole byte size as declared (etl_image.cpp:263)
void clear_canvases(const aeon_out_desc& od, void* out_dev, int n, hipStream_t stream)
{
    if (od.fixed_aspect_ratio)
        HIP_OK(hipMemset2DAsync(out_dev, od.item_stride, 0,
                                (size_t)od.canvas_w * od.canvas_h * od.channels * out_elem_bytes(od.dtype), n, stream));
}

// The next ring slot for a call on `stream`, once the kernels that last used it are done.
Slot& take_slot(aeon_hip_ctx* ctx, hipStream_t stream, int& index)
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
    return s;
}

// The call's launches are enqueued: its slot stays busy until a completion event covers it.
void release_slot(aeon_hip_ctx* ctx, int index, hipStream_t stream)
{
    ctx->open_slots.push_back(index);
    ctx->open_stream = stream;
    if ((int)ctx->open_slots.size() >= ctx->done_every) close_slots(ctx);
    ctx->host_calls++;
}

// The device error word of the calls on `stream`: each stream its own (so that aeon_hip_synchronize of
// one stream -- a decode window -- never reads or clears a bit another stream's kernels set meanwhile),
// the null stream and streams beyond the table's size share word 0.  A stream keeps its word until
// aeon_hip_synchronize has read it.
int32_t* stream_error(aeon_hip_ctx* ctx, hipStream_t stream, bool release = false)
{
    if (!stream) return ctx->d_error;
    std::lock_guard<std::mutex> lock(ctx->err_mu);
    int free_i = 0;
    for (int i = 1; i < aeon_hip_ctx::kErrWords; i++) {
        if (ctx->err_stream[i] == stream) {
            if (release) ctx->err_stream[i] = nullptr;
            return ctx->d_error + i;
        }
        if (!free_i && !ctx->err_stream[i]) free_i = i;
    }
    if (release || !free_i) return ctx->d_error;
    ctx->err_stream[free_i] = stream;
    return ctx->d_error + free_i;
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
        if (!is_mask && p.interp > AEON_INTERP_NEAREST) return false; // CUBIC / AREA / LANCZOS4 (plan_image)
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
    int         slot;
    Slot&       s     = take_slot(ctx, stream, slot);
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
    release_slot(ctx, slot, stream);
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
    int   slot;
    Slot& s = take_slot(ctx, stream, slot);
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
    release_slot(ctx, slot, stream);
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
    if (groups != 1 || f.into < plan.tiles + CallPlan::kMain || f.rows < 1 || f.into->has_contrast) return MaskFuse{};
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
    int   slot;
    Slot& s = take_slot(ctx, stream, slot);
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
                a.m_ctr    = ctx->d_tail + aeon_hip_ctx::kSlots + slot;
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
    launch_generic(ctx, plan.gr_main, table, o, d_lut, stream, timed);
    pass(CallPlan::kPre2, CallPlan::kPass1, KM_RAW);
    pass(CallPlan::kPass1, CallPlan::kMain, KM_STATS);
    pass(CallPlan::kMain, CallPlan::kGroups, KM_FINAL);
    phase(6);
    release_slot(ctx, slot, stream);
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
    int   slot;
    Slot& s = take_slot(ctx, stream, slot);
    const size_t tbytes = pads.size() * sizeof(PadRegion);
    ensure_ring(ctx, tbytes, 0, 0);
    std::memcpy(s.host, pads.data(), tbytes);
    // the table goes to the slot's device copy first, as the planner's job tables do (run_batch): read from the
    // pinned slot by every work item, its ~4,600 16-byte PCIe reads held the C3D half-short window's launch
    // at 62 us for 19 MB of zeros
    if (tbytes > kUploadKernelMax) HIP_OK(hipMemcpyAsync(s.dev, s.host, tbytes, hipMemcpyHostToDevice, stream));
    else HIP_OK(launch_upload_table(s.host_dev, s.dev, tbytes, stream));
    HIP_OK(launch_clip_pad((const PadRegion*)s.dev, (int)pads.size(), max_pad, stream));
    release_slot(ctx, slot, stream);
    return 0;
}

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

// A checked call's table (box_job.hpp) written into a ring slot's pinned buffer -- the extension, when the
// call has one, by fill_ext(RcnnRec*) -- and copied to the slot's device table on `stream`.  The caller
// holds ctx->mu and releases the slot after its launch over the device table, which is returned.
template <typename FillExt>
BoxTableDev stage_box_call(aeon_hip_ctx* ctx, const BoxCall& c, size_t total, bool rcnn, hipStream_t stream, int& slot,
                           FillExt fill_ext)
{
    Slot& s = take_slot(ctx, stream, slot);
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
    int               slot;
    const BoxTableDev t = stage_box_call(ctx, c, total, false, stream, slot, [](RcnnRec*) {});
    launch_box_table(n, t, *out, stream);
    release_slot(ctx, slot, stream);
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
    int               slot;
    const BoxTableDev t = stage_box_call(ctx, c, total, true, stream, slot, [&](RcnnRec* X) {
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
    release_slot(ctx, slot, stream);
    if (engine_states) {
        HIP_OK(hipMemcpyAsync(engine_states, states_dev, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
    }
    return 0;
}

using TrackedEngine = tracked_engine; // rcnn_host.hpp

template <typename F>
int guarded(F&& f)
{
    try {
        return f();
    } catch (const aeon_error& e) {
        g_err = e.what();
        return e.code;
    } catch (const jpeg_error& e) {
        g_err = e.what();
        return e.code;
    } catch (const std::invalid_argument& e) {
        g_err = e.what();
        return AEON_HIP_EINVAL;
    } catch (const std::exception& e) {
        g_err = e.what();
        return AEON_HIP_ERUNTIME;
    }
}

} // namespace

namespace aeon_hip {
// The owning decoder's pool runs the context's JPEG entropy decoding (set before the first JPEG call).
void ctx_share_pool(aeon_hip_ctx* ctx, thread_pool* pool)
{
    if (ctx && !ctx->jpeg) ctx->host_pool = pool;
}

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

int aeon_hip_ctx_create(int device, aeon_hip_ctx** out)
{
    return guarded([&] {
        if (!out) fail(AEON_HIP_EINVAL, "null out");
        auto* c   = new aeon_hip_ctx();
        c->device = device;
        try {
            HIP_OK(hipSetDevice(device));
            HIP_OK(set_kernel_lds_limit(kMaxLds));
            HIP_OK(contrast_records_lds_limit(kMaxLds));
            HIP_OK(hipMalloc((void**)&c->d_error, sizeof(int32_t) * aeon_hip_ctx::kErrWords));
            HIP_OK(hipMemset(c->d_error, 0, sizeof(int32_t) * aeon_hip_ctx::kErrWords));
            // per slot: the dynamic-tail counter, then (kSlots on) the mask-block counter of pair calls
            HIP_OK(hipMalloc((void**)&c->d_tail, 2 * aeon_hip_ctx::kSlots * sizeof(uint32_t)));
            HIP_OK(hipMemset(c->d_tail, 0, 2 * aeon_hip_ctx::kSlots * sizeof(uint32_t)));
            HIP_OK(hipDeviceSynchronize());
            // RGB2HSV_b division tables (hsv_shift = 12), as OpenCV builds them, then per uchar H
            // HSV2RGB_f's sector fraction f (its own float operations) turned into the weight w of
            // each output channel in t = v*(1 - s*w): t0 w=0, t1 w=1, t2 w=f, t3 w=1-f
            int32_t tab[kHsvWords];
            tab[0] = tab[256] = 0;
            for (int i = 1; i < 256; i++) {
                tab[i]       = cv_round((255 << 12) / (1. * i));
                tab[256 + i] = cv_round((180 << 12) / (6. * i));
            }
            static const int sector_data[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};
            for (int H = 0; H < 256; H++) {
                volatile float hf = (float)H;
                hf = hf * (6.f / 180.f);
                while (hf >= 6.f) hf = hf - 6.f;
                int sector = (int)std::floor((float)hf);
                hf         = hf - (float)sector;
                if ((unsigned)sector >= 6u) sector = 0, hf = 0.f;
                const float f      = hf;
                const float wt[4]  = {0.f, 1.f, f, 1.f - f};
                const float w[4]   = {wt[sector_data[sector][0]], wt[sector_data[sector][1]], wt[sector_data[sector][2]], 0.f};
                std::memcpy(&tab[512 + 4 * H], w, sizeof(w));
            }
            HIP_OK(hipMalloc((void**)&c->d_hsv, sizeof(tab)));
            HIP_OK(hipMemcpy(c->d_hsv, tab, sizeof(tab), hipMemcpyHostToDevice));
            for (Slot& s : c->slots) {
                // the ring's completion events only tell the host that the GPU is done reading a
                // slot: no system-scope fence needed (each one idled the GPU ~6 us between launches)
                HIP_OK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming | hipEventDisableSystemFence));
                // s.copied orders the SDMA job-table upload (copy_stream) before the kernels that read
                // it on the launch stream: it keeps the system-scope release
                HIP_OK(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
            }
            HIP_OK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
            // job tables in HBM written by the host when the GPU exposes all of its memory through
            // the PCIe BAR (else pinned host tables, read over PCIe)
            int large_bar = 0;
            if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, device) != hipSuccess) large_bar = 0;
            c->vram_jobs = large_bar != 0;
            if (const char* e = std::getenv("AEON_HIP_VRAM_JOBS")) c->vram_jobs = c->vram_jobs && std::atoi(e) != 0;
            // the ring at the size a 512-record call needs (job tables of 128 KB), so steady-state
            // calls of that size never allocate
            ensure_ring(c, 128 * 1024, 64 * 1024, 8 * 1024);
            // diagnostics: host time per phase (printed at destroy); the multi-pass path for every call
            if (const char* e = std::getenv("AEON_HIP_HOST_PROFILE")) c->host_profile = std::atoi(e) != 0;
            if (c->host_profile) std::fprintf(stderr, "[aeon_hip] job tables in HBM (BAR writes): %d\n", (int)c->vram_jobs);
            if (const char* e = std::getenv("AEON_HIP_DIRECT")) c->direct = std::atoi(e) != 0;
            if (const char* e = std::getenv("AEON_HIP_RECORDS")) c->records = std::atoi(e) != 0;
            if (const char* e = std::getenv("AEON_HIP_JPEG_HUFF")) c->jpeg_gpu_huff = std::strcmp(e, "host") != 0;
            if (const char* e = std::getenv("AEON_HIP_FUSE_MASKS")) c->fuse_masks = std::atoi(e) != 0;
#ifdef AEON_HIP_TRACE
            // development builds only: s_memtime phase stamps of the tile kernel into this device buffer
            if (const char* e = std::getenv("AEON_HIP_TRACE_PTR")) c->trace = (uint32_t*)std::strtoull(e, nullptr, 0);
#endif
            HIP_OK(hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device));
        } catch (...) {
            delete c;
            throw;
        }
        *out = c;
        return 0;
    });
}

int aeon_hip_ctx_destroy(aeon_hip_ctx* c)
{
    return guarded([&] {
        if (!c) return 0;
        if (c->host_profile && c->host_calls) {
            static const char* names[8] = {"set_device", "plan", "group+finalize", "slot_wait",
                                           "blob_fill", "h2d+wait_event (direct: table publish)", "launches",
                                           "done_event"};
            std::fprintf(stderr, "[aeon_hip host profile] %ld calls, us per call (median/mean/p90):", c->host_calls);
            double total = 0;
            for (int k = 0; k < 8; k++) {
                std::vector<double> v = c->host_ns[k];
                if (v.empty()) continue;
                double sum = 0;
                for (double x : v) sum += x;
                total += sum / v.size();
                std::sort(v.begin(), v.end());
                std::fprintf(stderr, " %s=%.1f/%.1f/%.1f", names[k], v[v.size() / 2] / 1e3, sum / v.size() / 1e3,
                             v[v.size() * 9 / 10] / 1e3);
            }
            std::fprintf(stderr, "; mean total %.1f us\n", total / 1e3);
        }
        (void)hipSetDevice(c->device);
        jpeg_state_destroy(c->jpeg);
        if (!c->open_slots.empty()) (void)hipStreamSynchronize(c->open_stream);
        for (Slot& s : c->slots)
            if (s.pending) (void)hipEventSynchronize(c->slots[s.cover].done);
        for (Slot& s : c->slots) {
            if (s.done) (void)hipEventDestroy(s.done);
            if (s.copied) (void)hipEventDestroy(s.copied);
            if (s.host) (void)hipHostFree(s.host);
            if (s.dev) (void)hipFree(s.dev);
            if (s.vram) free_vram(s.vram, s.vram_cap);
            if (s.scratch) (void)hipFree(s.scratch);
            if (s.partials) (void)hipFree(s.partials);
            if (s.shifts) (void)hipFree(s.shifts);
        }
        for (auto* v : {&c->timers, &c->free_timers})
            for (KernelTimer& t : *v) (void)hipEventDestroy(t.start), (void)hipEventDestroy(t.stop);
        if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
        for (auto& L : c->luts) (void)hipFree(L.dev);
        if (c->d_error) (void)hipFree(c->d_error);
        if (c->d_tail) (void)hipFree(c->d_tail);
        if (c->d_hsv) (void)hipFree(c->d_hsv);
        if (c->rcnn_anchors_dev) (void)hipFree(c->rcnn_anchors_dev);
        if (c->rcnn_states_dev) (void)hipFree(c->rcnn_states_dev);
        delete c;
        return 0;
    });
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

int aeon_hip_release_stream(aeon_hip_ctx* ctx, void* stream)
{
    return guarded([&] {
        if (!ctx) fail(AEON_HIP_EINVAL, "null ctx");
        std::lock_guard<std::mutex> lock(ctx->mu);
        HIP_OK(hipSetDevice(ctx->device));
        // the ring slots of the calls still open on this stream get their completion event now, while
        // the stream exists (the next call on another stream would record it there -- on a destroyed
        // stream by then); the context then holds no reference to the stream
        if (ctx->open_stream == (hipStream_t)stream) {
            close_slots(ctx);
            ctx->open_stream = nullptr;
        }
        return 0;
    });
}

int aeon_hip_synchronize(aeon_hip_ctx* ctx, void* stream)
{
    return guarded([&] {
        if (!ctx) fail(AEON_HIP_EINVAL, "null ctx");
        if (const int rc = aeon_hip_release_stream(ctx, stream)) return rc;
        HIP_OK(hipSetDevice(ctx->device));
        HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        // this stream's word (its calls' kernels are done): read and cleared on the stream itself, the
        // word then handed back (a stream that is reused gets a word again at its next call)
        int32_t* word = stream_error(ctx, (hipStream_t)stream);
        int32_t  err  = 0;
        HIP_OK(hipMemcpyAsync(&err, word, sizeof(err), hipMemcpyDeviceToHost, (hipStream_t)stream));
        if (err != 0) HIP_OK(hipMemsetAsync(word, 0, sizeof(int32_t), (hipStream_t)stream));
        HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        (void)stream_error(ctx, (hipStream_t)stream, true);
        if (err != 0) {
            fail(AEON_HIP_EDEVICE, "device error word " + std::to_string(err) + " (" + device_error_text(err) + ")");
        }
        return 0;
    });
}

int aeon_hip_set_timing(aeon_hip_ctx* ctx, int enable)
{
    return guarded([&] {
        if (!ctx) fail(AEON_HIP_EINVAL, "null ctx");
        std::lock_guard<std::mutex> lock(ctx->mu);
        ctx->timing       = enable > 0;
        ctx->timing_every = std::max(1, enable);
        ctx->timing_calls = 0;
        return 0;
    });
}

int aeon_hip_kernel_times(aeon_hip_ctx* ctx, int kinds, double* ms, double* bytes, long* count)
{
    return guarded([&] {
        if (!ctx || !ms || !bytes || !count) fail(AEON_HIP_EINVAL, "null argument");
        if (kinds < 0) fail(AEON_HIP_EINVAL, "negative kinds");
        std::lock_guard<std::mutex> lock(ctx->mu);
        HIP_OK(hipSetDevice(ctx->device));
        for (KernelTimer& t : ctx->timers) {
            HIP_OK(hipEventSynchronize(t.stop));
            float e = 0;
            HIP_OK(hipEventElapsedTime(&e, t.start, t.stop));
            ctx->ms[t.kind] += e;
            ctx->bytes[t.kind] += t.bytes;
            ctx->count[t.kind] += 1;
            ctx->free_timers.push_back(t);
        }
        ctx->timers.clear();
        for (int k = 0; k < 4; k++) {
            if (k < kinds) ms[k] = ctx->ms[k], bytes[k] = ctx->bytes[k], count[k] = ctx->count[k];
            ctx->ms[k] = ctx->bytes[k] = 0, ctx->count[k] = 0;
        }
        return 0;
    });
}

int aeon_param_factory_create(const char* aug_json, aeon_param_factory** out)
{
    return guarded([&] {
        if (!out) fail(AEON_HIP_EINVAL, "null out");
        Json j = aug_json && *aug_json ? Json::parse(aug_json) : Json();
        *out   = new aeon_param_factory(j);
        return 0;
    });
}

int aeon_param_factory_destroy(aeon_param_factory* f)
{
    delete f;
    return 0;
}

int aeon_make_params(aeon_param_factory* f, uint32_t* state, int in_w, int in_h, int out_w, int out_h,
                     aeon_aug_params* out)
{
    return guarded([&] {
        if (!f || !state || !out) fail(AEON_HIP_EINVAL, "null argument");
        std::lock_guard<std::mutex> lock(f->mu);
        TrackedEngine eng(*state);
        f->f.make_params(eng, in_w, in_h, out_w, out_h, out);
        *state = eng.last;
        return 0;
    });
}

int aeon_make_ssd_params(aeon_param_factory* f, uint32_t* state, int in_w, int in_h, int out_w, int out_h,
                         const float* boxes, int n_boxes, aeon_aug_params* out)
{
    return guarded([&] {
        if (!f || !state || !out || n_boxes < 0 || (n_boxes > 0 && !boxes)) fail(AEON_HIP_EINVAL, "null argument");
        std::lock_guard<std::mutex> lock(f->mu);
        TrackedEngine eng(*state);
        f->f.make_ssd_params(eng, in_w, in_h, out_w, out_h, boxes, n_boxes, out);
        *state = eng.last;
        return 0;
    });
}

int aeon_param_factory_emit(aeon_param_factory* f, int* type, float* min_overlap)
{
    return guarded([&] {
        if (!f || !type || !min_overlap) fail(AEON_HIP_EINVAL, "null argument");
        *type        = f->f.emit_type();
        *min_overlap = f->f.emit_constraint_min_overlap;
        return 0;
    });
}

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

int aeon_png_info(const void* data, size_t size, int* width, int* height, int* bit_depth, int* color_type)
{
    return guarded([&] {
        if (!data || !width || !height || !bit_depth || !color_type) fail(AEON_HIP_EINVAL, "null argument");
        png_header(data, size, width, height, bit_depth, color_type);
        return 0;
    });
}

int aeon_decode_png(const void* data, size_t size, int mode, void* dst, size_t stride, int* elem_bytes)
{
    return guarded([&] {
        if (!data || !dst) fail(AEON_HIP_EINVAL, "null argument");
        if (mode < AEON_PNG_BGR8 || mode > AEON_PNG_ANYDEPTH) fail(AEON_HIP_EINVAL, "unknown PNG decode mode");
        int w, h, depth, ctype;
        png_header(data, size, &w, &h, &depth, &ctype);
        const size_t eb = (mode == AEON_PNG_ANYDEPTH && depth == 16 && ctype != 3) ? 2 : 1;
        if (stride < (size_t)w * (mode == AEON_PNG_BGR8 ? 3 : 1) * eb) fail(AEON_HIP_EINVAL, "stride too small");
        png_decode(data, size, mode, dst, stride, elem_bytes);
        return 0;
    });
}

int aeon_batch_sample_patches(aeon_param_factory* f, int sampler, uint32_t* state, const float* nboxes, int n,
                              float* out, int cap, int* n_out)
{
    return guarded([&] {
        if (!f || !state || !n_out || n < 0 || (n > 0 && !nboxes) || cap < 0 || (cap > 0 && !out))
            fail(AEON_HIP_EINVAL, "null argument");
        std::lock_guard<std::mutex> lock(f->mu);
        if (sampler < 0 || sampler >= (int)f->f.batch_samplers.size()) fail(AEON_HIP_EINVAL, "sampler index out of range");
        TrackedEngine     eng(*state);
        std::vector<nbox> objects, samples;
        for (int i = 0; i < n; i++)
            objects.emplace_back(nboxes[4 * i], nboxes[4 * i + 1], nboxes[4 * i + 2], nboxes[4 * i + 3]);
        f->f.batch_samplers[sampler].sample_patches(eng, objects, samples);
        *n_out = (int)samples.size();
        for (int i = 0; i < (int)samples.size() && i < cap; i++) {
            out[4 * i] = samples[i].xmin, out[4 * i + 1] = samples[i].ymin;
            out[4 * i + 2] = samples[i].xmax, out[4 * i + 3] = samples[i].ymax;
        }
        *state = eng.last;
        return 0;
    });
}

int aeon_seed_slots(uint32_t seed, int n, uint32_t* states)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && !states)) fail(AEON_HIP_EINVAL, "bad arguments");
        std::minstd_rand0 g(seed);
        for (int i = 0; i < n; i++) {
            uint32_t s = g() % 2147483647u;
            states[i]  = s == 0 ? 1 : s;
        }
        return 0;
    });
}

int aeon_jpeg_info(const void* data, size_t size, int* width, int* height, int* components)
{
    return guarded([&] {
        if (!data || !width || !height || !components) fail(AEON_HIP_EINVAL, "null argument");
        jpeg_info(data, size, width, height, components);
        return 0;
    });
}

int aeon_jpeg_entropy_decode(const void* data, size_t size, int* width, int* height, int* components,
                             int64_t* n_blocks, int64_t* n_values, uint64_t* hash)
{
    return guarded([&] {
        if (!data || !width || !height || !components || !n_blocks || !n_values || !hash)
            fail(AEON_HIP_EINVAL, "null argument");
        jpeg_entropy_only(data, size, width, height, components, n_blocks, n_values, hash);
        return 0;
    });
}

int aeon_jpeg_host_stage(const void* data, size_t size, int* gpu_entropy, int64_t* staged_bytes)
{
    return guarded([&] {
        if (!data || !gpu_entropy || !staged_bytes) fail(AEON_HIP_EINVAL, "null argument");
        jpeg_host_stage(data, size, gpu_entropy, staged_bytes);
        return 0;
    });
}

int aeon_hip_decode_jpeg_batch(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes,
                               const aeon_img_desc* descs, void* dst_base, void* stream)
{
    return guarded([&] {
        if (!ctx || n < 0 || (n > 0 && (!data || !sizes || !descs || !dst_base))) fail(AEON_HIP_EINVAL, "null argument");
        if (n == 0) return 0;
        HIP_OK(hipSetDevice(ctx->device));
        if (!ctx->jpeg) ctx->jpeg = jpeg_state_create(ctx->host_pool, ctx->jpeg_gpu_huff);
        KernelTimer t{};
        bool        timed = false;
        if (ctx->timing) {
            std::lock_guard<std::mutex> lock(ctx->mu);
            timed = (ctx->timing_calls++ % ctx->timing_every) == ctx->timing_every - 1;
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

int aeon_unbiased_round(float x, int64_t* out)
{
    return guarded([&] {
        if (!out) fail(AEON_HIP_EINVAL, "null out");
        *out = unbiased_round(x);
        return 0;
    });
}

int aeon_calculate_scale(int width, int height, int output_width, int output_height, float* scale)
{
    return guarded([&] {
        if (!scale) fail(AEON_HIP_EINVAL, "null out");
        *scale = calculate_scale(width, height, output_width, output_height);
        return 0;
    });
}

int aeon_cropbox_max_proportional(float in_w, float in_h, float out_w, float out_h, float* res_w, float* res_h)
{
    return guarded([&] {
        if (!res_w || !res_h) fail(AEON_HIP_EINVAL, "null out");
        cropbox_max_proportional(in_w, in_h, out_w, out_h, res_w, res_h);
        return 0;
    });
}

int aeon_hip_host_alloc(size_t bytes, void** out)
{
    return guarded([&] {
        if (!out) fail(AEON_HIP_EINVAL, "null out");
        HIP_OK(hipHostMalloc(out, bytes, hipHostMallocDefault));
        return 0;
    });
}

int aeon_hip_host_free(void* p)
{
    return guarded([&] {
        if (p) HIP_OK(hipHostFree(p));
        return 0;
    });
}

const char* aeon_hip_last_error(void) { return g_err.c_str(); }
int aeon_hip_debug_uncached_blocks(uint64_t* ranges, int cap, int* n)
{
    return guarded([&] {
        if (!n || (cap > 0 && !ranges)) fail(AEON_HIP_EINVAL, "null argument");
        std::lock_guard<std::mutex> lock(g_vram_pool_mu);
        *n = (int)g_vram_all.size();
        for (int i = 0; i < cap && i < *n; i++) {
            ranges[2 * i]     = (uint64_t)(uintptr_t)g_vram_all[i].first;
            ranges[2 * i + 1] = (uint64_t)(uintptr_t)g_vram_all[i].first + g_vram_all[i].second;
        }
        return 0;
    });
}

const char* aeon_hip_version(void) { return "aeon-hip 0.1 (gfx950)"; }

} // extern "C"
