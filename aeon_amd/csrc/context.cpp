// context.cpp -- the per-GPU context of the device half (context.hpp): create and destroy, the staging ring
// and its capacities, the process-wide pool of uncached HBM blocks, the standardize LUT cache, and the C
// entries that concern the context alone (streams, synchronize with its error words, timing, pinned host
// memory).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"
#include "context.hpp"
#include "launch.hpp"
#include "param_factory.hpp"

namespace aeon_hip {
namespace {

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
                {512, "separable resize band wider than its workgroup"},
                {1024, "PNG image data corrupt or truncated (GPU inflate / unfilter)"},
                {2048, "TIFF strip data corrupt or truncated (GPU LZW / PackBits / Deflate decoder)"}};
    std::string s;
    for (const auto& b : bits)
        if (err & b.bit) s += (s.empty() ? "" : "; ") + std::string(b.what);
    return s.empty() ? "unknown" : s;
}

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

} // namespace

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
const float* resident_lut(aeon_hip_ctx* ctx, const aeon_out_desc& o, bool u8_map)
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

// The owning decoder's pool runs the context's JPEG entropy decoding (set before the first JPEG call).
void ctx_share_pool(aeon_hip_ctx* ctx, thread_pool* pool)
{
    if (ctx && !ctx->jpeg) ctx->host_pool = pool;
}

} // namespace aeon_hip

using namespace aeon_hip;

// The context's teardown (aeon_hip_ctx_destroy, and aeon_hip_ctx_create when it fails half-way: every
// handle and pointer is checked before it is destroyed or freed, and no call here throws).
aeon_hip_ctx::~aeon_hip_ctx()
{
    if (host_profile && host_calls) {
        static const char* names[8] = {"set_device", "plan", "group+finalize", "slot_wait",
                                       "blob_fill", "h2d+wait_event (direct: table publish)", "launches",
                                       "done_event"};
        std::fprintf(stderr, "[aeon_hip host profile] %ld calls, us per call (median/mean/p90):", host_calls);
        double total = 0;
        for (int k = 0; k < 8; k++) {
            std::vector<double> v = host_ns[k];
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
    (void)hipSetDevice(device);
    jpeg_state_destroy(jpeg);
    png_stage_destroy(png);
    png_stage_destroy(pixmap);
    png_stage_destroy(tiff);
    if (!open_slots.empty()) (void)hipStreamSynchronize(open_stream);
    for (Slot& s : slots)
        if (s.pending) (void)hipEventSynchronize(slots[s.cover].done);
    for (Slot& s : slots) {
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.copied) (void)hipEventDestroy(s.copied);
        if (s.host) (void)hipHostFree(s.host);
        if (s.dev) (void)hipFree(s.dev);
        if (s.vram) free_vram(s.vram, s.vram_cap);
        if (s.scratch) (void)hipFree(s.scratch);
        if (s.partials) (void)hipFree(s.partials);
        if (s.shifts) (void)hipFree(s.shifts);
    }
    for (auto* v : {&timers, &free_timers})
        for (KernelTimer& t : *v) (void)hipEventDestroy(t.start), (void)hipEventDestroy(t.stop);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    for (auto& L : luts) (void)hipFree(L.dev);
    if (d_error) (void)hipFree(d_error);
    if (d_tail) (void)hipFree(d_tail);
    if (d_hsv) (void)hipFree(d_hsv);
    if (rcnn_anchors_dev) (void)hipFree(rcnn_anchors_dev);
    if (rcnn_states_dev) (void)hipFree(rcnn_states_dev);
}

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
            // (read here like the flag above: the JPEG state itself is made by the context's first decode call)
            if (const char* e = std::getenv("AEON_HIP_JPEG_HUFF_LANES")) {
                const int l        = std::atoi(e);
                c->jpeg_huff_lanes = l == 256 || l == 512 || l == 1024 ? l : 0;
            }
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
        delete c;
        return 0;
    });
}

} // extern "C"

namespace {
// The ring slots of the calls still open on this stream get their completion event now, while the
// stream exists (the next call on another stream would record it there -- on a destroyed stream by
// then); the context then holds no reference to the stream through its ring.
void close_stream_slots(aeon_hip_ctx* ctx, hipStream_t stream)
{
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_OK(hipSetDevice(ctx->device));
    if (ctx->open_stream == stream) {
        close_slots(ctx);
        ctx->open_stream = nullptr;
    }
}
} // namespace

extern "C" {

int aeon_hip_release_stream(aeon_hip_ctx* ctx, void* stream)
{
    return guarded([&] {
        if (!ctx) fail(AEON_HIP_EINVAL, "null ctx");
        close_stream_slots(ctx, (hipStream_t)stream);
        // its error word goes back to the table unread: whatever bits it holds are cleared ahead of its
        // next owner's first kernel (stream_error)
        release_stream_error(ctx, (hipStream_t)stream, /*unread=*/true);
        return 0;
    });
}

int aeon_hip_synchronize(aeon_hip_ctx* ctx, void* stream)
{
    return guarded([&] {
        if (!ctx) fail(AEON_HIP_EINVAL, "null ctx");
        close_stream_slots(ctx, (hipStream_t)stream);
        HIP_OK(hipSetDevice(ctx->device));
        // this stream's word: copied out behind the stream's calls and looked at only once the stream has
        // been waited for (the copy has landed by then, whether or not the runtime held this thread for
        // it), cleared on the stream itself when it holds a bit, and handed back only after the clear is
        // complete (a stream that is reused gets a word again at its next call)
        int32_t* word = stream_error(ctx, (hipStream_t)stream);
        int32_t  err  = 0;
        HIP_OK(hipMemcpyAsync(&err, word, sizeof(err), hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        if (err != 0) {
            HIP_OK(hipMemsetAsync(word, 0, sizeof(int32_t), (hipStream_t)stream));
            HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        }
        release_stream_error(ctx, (hipStream_t)stream, /*unread=*/false);
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
        for (int k = 0; k < AEON_HIP_TIMER_KINDS; k++) {
            if (k < kinds) ms[k] = ctx->ms[k], bytes[k] = ctx->bytes[k], count[k] = ctx->count[k];
            ctx->ms[k] = ctx->bytes[k] = 0, ctx->count[k] = 0;
        }
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

} // extern "C"
