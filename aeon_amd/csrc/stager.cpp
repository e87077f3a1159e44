// stager.cpp -- the aeon-side drop-in's staging + window launch (aeon_hip_stager_*, include/aeon_hip.h).
//
// aeon runs provide(idx, record, out_buf) for every record of a decode window on its pool and then
// (the one-line change) post_process(out_buf) once per batch of the window
// (src/batch_decoder.cpp:62-99).  A stager is what provider::image / provider::pixelmask hold to make
// those calls the GPU path:
//   stage(batch_out, idx, pixels, params)  -- provide(): the decoded record's bytes into pinned memory
//                                            (lock-free bump allocation in pinned chunks; concurrent)
//   stage_encoded(batch_out, idx, file, params) -- provide() with the record still encoded (stager_encoded.cpp,
//                                            through stager_encoded.hpp): decoded into pinned memory right there,
//                                            or kept as a file that the window's launch decodes on the device
//                                            into a slot behind the staged pixels, ahead of the augment launch
//   stage_clip / stage_frames (stager_clip.cpp, through stager_clip.hpp) -- provider::video's provide(): a clip of
//                                            at most max_frames frames per idx, its frames still MJPEG (a slot each,
//                                            decoded by the window's launch) or decoded (pinned staging); the
//                                            window's launch then makes one video call per batch, not an augment one
//   launch(batch_out)                      -- post_process(): the FIRST call after a window's stages
//                                            launches the whole window -- one H2D per pinned chunk, ONE
//                                            augment (or mask) launch over every staged record of every
//                                            batch, one D2H per batch buffer (or, for pinned batch
//                                            buffers, the kernels store into them directly) -- on the
//                                            window's own stream, and returns
//   wait(batch_out)                        -- the consumer (batch_iterator_fbm::filler) before it swaps
//                                            or copies the batch: blocks until that batch is complete
//   flush(batch_out)                       -- launch + wait (post_process that returns a finished batch)
// Two windows are kept, as aeon's async_manager keeps two containers (src/async_manager.hpp:162-204):
// while window k's copies and kernels run, window k+1 stages into the other one.
// The batch buffer's own address (out_buf[name]->get_item(0)) is the staging key: batches of one
// window never share it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/aeon_hip.h"
#include "stager_clip.hpp"
#include "stager_encoded.hpp"

namespace {

thread_local std::string g_stager_err;

struct stager_error : std::runtime_error {
    int code;
    stager_error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

[[noreturn]] void fail(int code, const std::string& m) { throw stager_error(code, m); }

void hip_ok(hipError_t e, const char* what)
{
    if (e != hipSuccess) fail(AEON_HIP_ERUNTIME, std::string(what) + ": " + hipGetErrorString(e));
}

void abi_ok(int rc)
{
    if (rc != 0) fail(rc, aeon_hip_last_error());
}

// Device address of pinned, device-mapped host memory p (hipHostMalloc / hipHostRegister), or null.
void* mapped_view(void* p)
{
    static const bool on = [] {
        const char* e = std::getenv("AEON_HIP_ZERO_COPY");
        return !(e && std::atoi(e) == 0);
    }();
    if (!on || !p) return nullptr;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); // pageable memory
        return nullptr;
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer || !a.hostPointer) return nullptr;
    return (uint8_t*)a.devicePointer + ((uint8_t*)p - (uint8_t*)a.hostPointer);
}

constexpr size_t kChunkBytes = 64u << 20; // pinned staging chunk (a window usually fits in one or two)
// the "chunk" of a desc tag whose offset is a slot of the device-decoded records, behind every chunk's bytes
constexpr uint64_t kSlotChunk  = 0xFFFF;
constexpr uint64_t kOffsetMask = (1ull << 48) - 1;

// The decode stages, for windows with device-decoded records (installed by aeon_hip_stager_stage_encoded).
std::atomic<aeon_hip::stager_decode_fn> g_decode{nullptr};
// The same for the clips of a video stager, with the video call (installed by aeon_hip_stager_stage_clip /
// _stage_frames): this file names neither.
std::atomic<aeon_hip::stager_decode_fn> g_clip_decode{nullptr};
std::atomic<aeon_hip::stager_video_fn>  g_video{nullptr};
// (the video call's own limit: a window with more frames goes in several calls)
constexpr int64_t kVideoCallFrames = 65535;

// Where a staged record's pixels come from, for last_decode: kPixels, kHostDecoded + format or
// kDeviceDecoded + format.
constexpr uint8_t kPixels = 0, kHostDecoded = 1, kDeviceDecoded = 1 + AEON_FORMAT_COUNT;

struct Chunk {
    uint8_t* host = nullptr;
    size_t   cap  = 0;
    size_t   used = 0; // bump offset (under the stager's mutex)
    size_t   base = 0; // its offset in the device arena of the launched window
};

// One batch buffer of the window: per idx, where its pixels are and its params.
struct Batch {
    void*                        out = nullptr; // the batch buffer (host, or device memory)
    std::vector<aeon_img_desc>   descs;         // offset = (chunk << 48) | offset in chunk until launch; a video
                                                // stager's: max_frames per idx, row-major
    std::vector<aeon_aug_params> params;
    std::vector<uint8_t>         origin;        // kPixels, kHostDecoded + format, kDeviceDecoded + format
    std::vector<int32_t>         counts;        // video: the clip's frames, and how many of them are distinct (have
    std::vector<int32_t>         distinct;      // a slot or staging of their own: the others repeat a frame)
    std::unique_ptr<std::atomic<uint8_t>[]> have;
    int        first = 0;     // its first record in the window's launch order
    int        n     = 0;     // records staged (idx 0..n-1)
    hipEvent_t done  = nullptr;
    bool       d2h   = false; // pageable batch: its wait copies it out of the window's device outputs
    bool       launched = false; // a flush / launch named this batch buffer
    bool       waited   = false; // a flush / wait returned (or is returning) its completion
};

// A decode window: its pinned staging, its batches, its own stream and device buffers, so that window
// k's copies and kernels run while window k+1 is staged (aeon's async_manager keeps two containers in
// flight, src/async_manager.hpp:162-204).
// A file the window's launch decodes on the device into the slot its record's desc names.
struct File {
    std::unique_ptr<uint8_t[]> bytes;
    size_t                     size = 0;
    int                        format = 0, mode = 0;
    Batch*                     batch = nullptr;
    int                        idx = 0, frame = 0; // (frame: of a clip)
};

struct Window {
    enum State { IDLE, STAGING, LAUNCHED };
    State                               state = IDLE;
    uint64_t                            gen   = 0; // launch generation (a retire checks it)
    std::vector<Chunk>                  chunks;
    int                                 cur = 0; // chunk being filled
    std::vector<std::unique_ptr<Batch>> batches; // in first-stage order
    std::vector<File>                   files;   // records still encoded (under the stager's mutex)
    size_t                              slot_bytes = 0; // their slots' bump offset
    int                                 unwaited = 0;
    hipStream_t                         stream  = nullptr;
    hipEvent_t                          done    = nullptr;
    uint8_t*                            dev_src = nullptr;
    size_t                              dev_src_cap = 0;
    uint8_t*                            dev_out = nullptr;
    size_t                              dev_out_cap = 0;
    std::atomic<int>                    copying{0}; // waits copying a pageable batch out of dev_out
};

// A wait's hold on its window's `copying` count, taken under s->mu and given back on every way out of
// the wait -- a runtime call that fails ahead of the copy included: the window's last wait and
// staging_window spin until the count is 0.
struct CopyHold {
    Window* w = nullptr;
    CopyHold() = default;
    CopyHold(const CopyHold&)            = delete;
    CopyHold& operator=(const CopyHold&) = delete;
    void take(Window& win)
    {
        win.copying.fetch_add(1, std::memory_order_acq_rel);
        w = &win;
    }
    void drop()
    {
        if (w) w->copying.fetch_sub(1, std::memory_order_acq_rel);
        w = nullptr;
    }
    ~CopyHold() { drop(); }
};

} // namespace

struct aeon_hip_stager {
    aeon_hip_ctx* ctx   = nullptr;
    int           kind  = AEON_STAGER_IMAGE;
    aeon_out_desc out{};
    int           batch = 0;
    int           frames = 1;           // descs per idx: a video stager's max_frames
    int           out_w = 0, out_h = 0; // video: the frame's output size
    size_t        item_bytes = 0;       // video: a clip's bytes (copy_out); 0: items are copied strides whole
    int           device = 0;
    std::mutex    mu;
    Window        win[2];
    int           cur = 0; // the window stages go to
    uint64_t      gens = 0;
    std::vector<hipEvent_t> spare_events;
    aeon_stager_launch_info last{}; // the last window launched (launch_window, under mu)
    aeon_stager_decode_info last_decode{};
    std::atomic<int>        waiters{0}; // aeon_hip_stager_wait(NULL, ...) calls inside this stager (destroy waits)
};

namespace {

// Batch buffers of launched windows -> their stager, for aeon_hip_stager_wait(NULL, buffer) (the
// consumer, batch_iterator_fbm::filler, knows the buffers but not the providers).  Lock order: a
// stager's mu may be held when g_reg_mu is taken, never the reverse.
// An entry is (stager, window generation): a buffer address that appears in both windows keeps the
// newer window's entry, and retiring the older window erases only its own.
struct Pending {
    aeon_hip_stager* s;
    uint64_t         gen;
};
std::mutex                        g_reg_mu;
std::unordered_map<void*, Pending> g_pending;

template <typename F>
int stager_guarded(F&& f)
{
    try {
        f();
        return 0;
    } catch (const stager_error& e) {
        g_stager_err = e.what();
        return e.code;
    } catch (const std::exception& e) {
        g_stager_err = e.what();
        return AEON_HIP_ERUNTIME;
    }
}

void grow(uint8_t*& p, size_t& cap, size_t need)
{
    if (need <= cap) return;
    const size_t n = std::max(need, cap + cap / 2);
    if (p) hip_ok(hipFree(p), "hipFree");
    p = nullptr, cap = 0;
    hip_ok(hipMalloc((void**)&p, n), "hipMalloc");
    cap = n;
}

// A pageable batch's D2H out of the window's device output: n items in one copy, strides whole -- or, for clips
// whose item_stride is wider than the clip (aeon's buffers have none that are), clip by clip, so that no byte
// between the host items is written.
hipError_t copy_out(const aeon_hip_stager* s, void* dst, const uint8_t* src, int n)
{
    const size_t stride = s->out.item_stride;
    if (s->item_bytes == 0 || s->item_bytes == stride) return hipMemcpy(dst, src, (size_t)n * stride, hipMemcpyDeviceToHost);
    for (int i = 0; i < n; i++)
        if (const hipError_t e = hipMemcpy((uint8_t*)dst + i * stride, src + i * stride, s->item_bytes, hipMemcpyDeviceToHost))
            return e;
    return hipSuccess;
}

// Forget a completed (or dropped) window: batches gone, chunks empty (their memory is kept).  Caller
// holds s->mu.
void reset_window(aeon_hip_stager* s, Window& w)
{
    if (w.state == Window::LAUNCHED) {
        std::lock_guard<std::mutex> r(g_reg_mu);
        for (auto& b : w.batches) {
            auto it = g_pending.find(b->out);
            if (it != g_pending.end() && it->second.s == s && it->second.gen == w.gen) g_pending.erase(it);
        }
    }
    for (auto& b : w.batches)
        if (b->done) s->spare_events.push_back(b->done);
    w.batches.clear();
    w.files.clear();
    w.slot_bytes = 0;
    for (Chunk& c : w.chunks) c.used = 0;
    w.cur      = 0;
    w.state    = Window::IDLE;
    w.unwaited = 0;
}

// The window stages go to, under s->mu: the current one unless it was launched, else the other one --
// which, if it is still in flight (its consumer never waited for it), is completed and dropped first.
Window& staging_window(aeon_hip_stager* s)
{
    if (s->win[s->cur].state != Window::LAUNCHED) return s->win[s->cur];
    s->cur    = 1 - s->cur;
    Window& w = s->win[s->cur];
    if (w.state == Window::LAUNCHED) {
        hip_ok(hipSetDevice(s->device), "hipSetDevice");
        hip_ok(hipEventSynchronize(w.done), "hipEventSynchronize");
        // its pageable batches nobody waited for: their D2H now, so they are complete when this returns
        for (auto& b : w.batches)
            if (b->d2h && !b->waited) {
                b->waited = true;
                hip_ok(copy_out(s, b->out, w.dev_out + (size_t)b->first * s->out.item_stride, b->n), "hipMemcpy");
            }
        while (w.copying.load(std::memory_order_acquire) != 0) std::this_thread::yield();
        reset_window(s, w);
    }
    return w;
}

// Reserve `bytes` (16-aligned) of pinned staging: returns (chunk, offset).  Caller holds s->mu.
std::pair<int, size_t> reserve(Window& w, size_t bytes)
{
    bytes = (bytes + 15) & ~(size_t)15;
    for (;; w.cur++) {
        if (w.cur == (int)w.chunks.size()) {
            Chunk c;
            c.cap = std::max(kChunkBytes, bytes);
            hip_ok(hipHostMalloc((void**)&c.host, c.cap, hipHostMallocDefault), "hipHostMalloc");
            w.chunks.push_back(c);
        }
        Chunk& c = w.chunks[w.cur];
        if (c.used + bytes <= c.cap) {
            const size_t off = c.used;
            c.used += bytes;
            return {w.cur, off};
        }
    }
}

Batch& batch_for(aeon_hip_stager* s, Window& w, void* out)
{
    for (auto& b : w.batches)
        if (b->out == out) return *b;
    auto b  = std::make_unique<Batch>();
    b->out  = out;
    b->descs.resize((size_t)s->batch * s->frames);
    b->params.resize(s->batch);
    b->origin.assign(s->batch, kPixels);
    if ((s->kind & ~AEON_STAGER_DEVICE_OUT) == AEON_STAGER_VIDEO) {
        b->counts.assign(s->batch, 0);
        b->distinct.assign(s->batch, 0);
    }
    b->have.reset(new std::atomic<uint8_t>[s->batch]);
    for (int i = 0; i < s->batch; i++) b->have[i] = 0;
    w.batches.push_back(std::move(b));
    return *w.batches.back();
}

// The window's launch (the first flush / launch): H2D of the pinned chunks, one kernel launch over every
// staged record, then per batch buffer its D2H (or zero-copy stores) and completion event, all on the
// window's stream.  Caller holds s->mu.
void launch_window(aeon_hip_stager* s, Window& w)
{
    size_t total = 0;
    for (Chunk& c : w.chunks) {
        c.base = total;
        total += c.used;
    }
    const bool                   video = (s->kind & ~AEON_STAGER_DEVICE_OUT) == AEON_STAGER_VIDEO;
    const size_t                 D     = (size_t)s->frames; // descs per record (a clip's row)
    std::vector<aeon_img_desc>   descs;
    std::vector<aeon_aug_params> params; // one per record: params.size() is the window's records
    std::vector<int32_t>         counts; // video: one per clip
    std::vector<void*>           views;
    bool                         all_mapped = true;
    aeon_stager_decode_info      decoded{};
    for (auto& bp : w.batches) {
        Batch& b = *bp;
        b.n = 0;
        while (b.n < s->batch && b.have[b.n]) b.n++;
        for (int i = b.n; i < s->batch; i++)
            if (b.have[i]) fail(AEON_HIP_EINVAL, "batch staged with a hole: idx " + std::to_string(b.n) + " missing");
        b.first = (int)params.size();
        for (int i = 0; i < b.n; i++) {
            const size_t kept = video ? (size_t)b.counts[i] : 1;
            for (size_t f = 0; f < D; f++) {
                aeon_img_desc d{}; // (the rest of a short clip's row is not read)
                if (f < kept) {
                    d = b.descs[(size_t)i * D + f];
                    // (a device-decoded record's slot lies behind every chunk's bytes)
                    d.offset =
                        ((d.offset >> 48) == kSlotChunk ? total : w.chunks[d.offset >> 48].base) + (d.offset & kOffsetMask);
                }
                descs.push_back(d);
            }
            params.push_back(b.params[i]);
            if (video) counts.push_back(b.counts[i]);
            const uint8_t o = b.origin[i];
            const int32_t k = video ? b.distinct[i] : 1; // (a clip counts by its frames)
            if (o == kPixels) decoded.pixels += k;
            else if (o < kDeviceDecoded) decoded.host[o - kHostDecoded] += k;
            else decoded.device[o - kDeviceDecoded] += k;
        }
        void* v = (s->kind & AEON_STAGER_DEVICE_OUT) ? nullptr : mapped_view(b.out);
        views.push_back(v);
        all_mapped = all_mapped && v;
    }
    // The window's sources: read by the kernels straight from its pinned chunk over PCIe when the outputs
    // go to pinned host buffers too and the window fits one chunk -- no H2D ahead of the kernels (the
    // runtime may run that copy as a blit kernel, which then cannot overlap the previous window's
    // persistent grid: C2 60 K vs ~80 K records/s, tools/aeon_path_cpp.cpp) -- else one H2D per chunk into
    // the window's device arena.
    const bool on_device = (s->kind & AEON_STAGER_DEVICE_OUT) != 0;
    bool       all_out_mapped = !on_device;
    for (auto& bp : w.batches) all_out_mapped = all_out_mapped && mapped_view(bp->out);
    int         used_chunks = 0;
    const Chunk* used = nullptr; // (its base is 0: the chunks before it hold nothing)
    for (const Chunk& c : w.chunks)
        if (c.used) used_chunks++, used = used ? used : &c;
    static const bool src_copy = [] {
        const char* e = std::getenv("AEON_HIP_STAGER_SRC_COPY");
        return e && std::atoi(e) != 0;
    }();
    const uint8_t* src_base = nullptr;
    if (all_out_mapped && used_chunks == 1 && !src_copy && w.files.empty()) src_base = (const uint8_t*)mapped_view(used->host);
    const bool zero_copy = src_base != nullptr;
    if (!src_base) {
        grow(w.dev_src, w.dev_src_cap, std::max<size_t>(total + w.slot_bytes, 16));
        for (const Chunk& c : w.chunks)
            if (c.used)
                hip_ok(hipMemcpyAsync(w.dev_src + c.base, c.host, c.used, hipMemcpyHostToDevice, w.stream),
                       "hipMemcpyAsync");
        src_base = w.dev_src;
    }
    // The records still encoded: decoded into their slots by the stages, which upload the files themselves (no
    // encoded byte is in a chunk), on the window's stream ahead of the kernels that read the slots.  The stages
    // are done with the files when they return.
    if (!w.files.empty()) {
        const aeon_hip::stager_decode_fn decode = (video ? g_clip_decode : g_decode).load(std::memory_order_acquire);
        if (!decode) fail(AEON_HIP_ERUNTIME, "encoded records staged without the decode stages");
        std::vector<aeon_hip::stager_file> files;
        files.reserve(w.files.size());
        for (const File& f : w.files)
            files.push_back(
                {f.bytes.get(), f.size, f.format, f.mode, descs[((size_t)f.batch->first + f.idx) * D + f.frame]});
        abi_ok(decode(s->ctx, files.data(), files.size(), w.dev_src, w.stream));
        w.files.clear();
    }
    const size_t item = s->out.item_stride;
    auto run = [&](int first, int n, void* dst) {
        if (n == 0) return;
        if (video) {
            const aeon_hip::stager_video_fn call = g_video.load(std::memory_order_acquire);
            if (!call) fail(AEON_HIP_ERUNTIME, "clips staged without the video call");
            // clips [a, e): as many as the video call takes frames (a clip has at most 65,535 of them: create)
            for (int a = first, e; a < first + n; a = e) {
                int64_t fr = 0;
                for (e = a; e < first + n && fr + counts[e] <= kVideoCallFrames; e++) fr += counts[e];
                abi_ok(call(s->ctx, e - a, counts.data() + a, descs.data() + (size_t)a * D, src_base, params.data() + a,
                            s->frames, s->out_w, s->out_h, (uint8_t*)dst + (size_t)(a - first) * item, item, w.stream));
            }
        } else if ((s->kind & ~AEON_STAGER_DEVICE_OUT) == AEON_STAGER_MASK)
            abi_ok(aeon_hip_mask_batch(s->ctx, n, descs.data() + first, src_base, params.data() + first, &s->out,
                                       dst, w.stream));
        else
            abi_ok(aeon_hip_augment_batch(s->ctx, n, descs.data() + first, src_base, params.data() + first, &s->out,
                                          dst, w.stream));
    };
    if (on_device || all_mapped) {
        // outputs the kernels can store into directly (device batch buffers, or pinned host ones over
        // PCIe): one launch per batch, queued back to back
        for (size_t k = 0; k < w.batches.size(); k++) {
            Batch& b = *w.batches[k];
            run(b.first, b.n, on_device ? b.out : views[k]);
            hip_ok(hipEventRecord(b.done, w.stream), "hipEventRecord");
        }
    } else {
        // pageable host batches: the whole window in ONE launch into device memory; each batch's D2H is
        // made by its wait (the consumer's thread): a copy into pageable memory holds the calling thread
        // until the data is out (the runtime stages it), and on the decode thread that made the
        // launch-only post_process wait for the window's kernels (overlap measured below flush)
        grow(w.dev_out, w.dev_out_cap, std::max<size_t>(params.size() * item, 16));
        run(0, (int)params.size(), w.dev_out);
        hip_ok(hipEventRecord(w.batches.front()->done, w.stream), "hipEventRecord");
        for (auto& bp : w.batches) {
            Batch& b = *bp;
            if (&b != w.batches.front().get()) hip_ok(hipEventRecord(b.done, w.stream), "hipEventRecord");
            b.d2h = b.n > 0;
        }
    }
    hip_ok(hipEventRecord(w.done, w.stream), "hipEventRecord");
    w.state    = Window::LAUNCHED;
    w.gen      = ++s->gens;
    w.unwaited = (int)w.batches.size();
    s->last    = aeon_stager_launch_info{s->last.launches + 1, zero_copy ? 1 : 0, (on_device || all_mapped) ? 1 : 0,
                                         used_chunks, (int32_t)params.size()};
    decoded.launches = s->last.launches;
    s->last_decode   = decoded;
    std::lock_guard<std::mutex> r(g_reg_mu);
    for (auto& b : w.batches) g_pending[b->out] = Pending{s, w.gen};
}

// Launch the staging window if batch_out belongs to it (the first post_process of a window); mark
// batch_out launched.  Caller holds s->mu.
void launch_for(aeon_hip_stager* s, void* batch_out)
{
    hip_ok(hipSetDevice(s->device), "hipSetDevice");
    Window& sw = s->win[s->cur];
    if (sw.state == Window::STAGING) {
        bool mine = false;
        for (auto& b : sw.batches) mine = mine || b->out == batch_out;
        if (mine) {
            try {
                launch_window(s, sw);
            } catch (...) { // nothing of this window is delivered: drop it whole
                (void)hipStreamSynchronize(sw.stream);
                sw.state = Window::STAGING; // (never registered)
                reset_window(s, sw);
                throw;
            }
        }
    }
    for (Window& w : s->win) {
        if (w.state != Window::LAUNCHED) continue;
        for (auto& b : w.batches)
            if (b->out == batch_out && !b->waited) {
                if (b->launched) fail(AEON_HIP_EINVAL, "batch buffer flushed twice in one window");
                b->launched = true;
                return;
            }
    }
    fail(AEON_HIP_EINVAL, "no records of this window were staged for this batch buffer");
}

// Wait until batch_out's outputs are complete.  found = false: no launched window holds it (nothing to
// wait for).  The window's last wait checks the device error word and retires the window -- unless it
// was dropped and reused meanwhile (its generation changed).
void wait_batch(aeon_hip_stager* s, void* batch_out, bool& found)
{
    hipEvent_t ev = nullptr, wdone = nullptr;
    hipStream_t wstream = nullptr;
    Window*     wp  = nullptr;
    uint64_t    gen = 0;
    bool        last = false;
    void*       copy_dst = nullptr; // pageable batch: its D2H, made here
    const void* copy_src = nullptr;
    int         copy_n = 0;
    CopyHold    hold;
    {
        std::lock_guard<std::mutex> l(s->mu);
        for (Window& w : s->win) {
            if (w.state != Window::LAUNCHED || ev) continue;
            for (auto& b : w.batches)
                if (b->out == batch_out && !b->waited) {
                    b->waited = true;
                    ev        = b->done;
                    wp = &w, gen = w.gen, wdone = w.done, wstream = w.stream;
                    last = --w.unwaited == 0;
                    if (b->d2h) {
                        hold.take(w);
                        copy_dst   = b->out;
                        copy_src   = w.dev_out + (size_t)b->first * s->out.item_stride;
                        copy_n     = b->n;
                    }
                    break;
                }
        }
    }
    found = ev != nullptr;
    if (!found) return;
    hip_ok(hipSetDevice(s->device), "hipSetDevice");
    hip_ok(hipEventSynchronize(ev), "hipEventSynchronize");
    // (the window's device outputs stay until its last wait has returned: reset_window runs after it)
    if (copy_n) {
        const hipError_t e = copy_out(s, copy_dst, (const uint8_t*)copy_src, copy_n);
        hold.drop();
        hip_ok(e, "hipMemcpy");
    }
    if (!last) return;
    while (wp->copying.load(std::memory_order_acquire) != 0) std::this_thread::yield(); // (other batches' copies)
    // the window is complete: surface a device error word, then free it for the window after next
    hip_ok(hipEventSynchronize(wdone), "hipEventSynchronize");
    const int rc = aeon_hip_synchronize(s->ctx, wstream);
    {
        std::lock_guard<std::mutex> l(s->mu);
        if (wp->state == Window::LAUNCHED && wp->gen == gen) reset_window(s, *wp);
    }
    abi_ok(rc);
}

// What every staged record is checked for, however its pixels arrive.
void check_record(aeon_hip_stager* s, int idx, int width, int height, int channels, int elem_bytes)
{
    if (idx < 0 || idx >= s->batch) fail(AEON_HIP_EINVAL, "idx out of range of the batch");
    if (width <= 0 || height <= 0) fail(AEON_HIP_EINVAL, "received an image with size 0, at idx " + std::to_string(idx));
    if (channels != 1 && channels != 3) fail(AEON_HIP_EINVAL, "channels must be 1 or 3");
    if (elem_bytes != 1 && elem_bytes != 2) fail(AEON_HIP_EINVAL, "elem_bytes must be 1 or 2");
}

// batch_out's batch of the staging window w, made on its first stage and given its completion event, for a
// stage of idx, which must be its first.  Caller holds s->mu.
Batch& open_batch(aeon_hip_stager* s, Window& w, void* batch_out, int idx)
{
    w.state  = Window::STAGING;
    Batch& b = batch_for(s, w, batch_out);
    if (!b.done) {
        if (!s->spare_events.empty()) {
            b.done = s->spare_events.back();
            s->spare_events.pop_back();
        } else {
            hip_ok(hipSetDevice(s->device), "hipSetDevice");
            hip_ok(hipEventCreateWithFlags(&b.done, hipEventDisableTiming), "hipEventCreate");
        }
    }
    if (b.have[idx]) fail(AEON_HIP_EINVAL, "idx " + std::to_string(idx) + " staged twice for one batch");
    return b;
}

// Record idx of batch_out into the staging window.  file == nullptr: its pixels go into pinned staging, written
// by fill(dst) on the calling thread.  Else the record is still encoded: *file is kept for the window's launch
// and the record gets a slot behind the staged pixels (fill is not called).
template <typename Fill>
void stage_record(aeon_hip_stager* s, void* batch_out, int idx, int width, int height, int channels, int elem_bytes,
                  const aeon_aug_params* params, uint8_t origin, File* file, Fill&& fill)
{
    const size_t row = (size_t)width * channels * elem_bytes;
    Batch*       b;
    uint8_t*     dst = nullptr;
    size_t       tag;
    {
        std::lock_guard<std::mutex> l(s->mu);
        Window& w = staging_window(s);
        b         = &open_batch(s, w, batch_out, idx);
        if (file) {
            if (w.slot_bytes + row * height > kOffsetMask) fail(AEON_HIP_EINVAL, "window too large");
            file->batch = b, file->idx = idx;
            w.files.push_back(std::move(*file));
            tag = (size_t)(kSlotChunk << 48) | w.slot_bytes;
            w.slot_bytes += (row * height + 15) & ~(size_t)15;
        } else {
            const auto r = reserve(w, row * height);
            dst          = w.chunks[r.first].host + r.second;
            tag          = ((size_t)r.first << 48) | r.second;
        }
    }
    // the copy (or decode) itself runs unlocked, on the calling pool thread (the window cannot launch before
    // this provide() returns: aeon flushes after its pool run)
    if (dst) fill(dst);
    b->descs[idx]  = aeon_img_desc{tag, width, height, (int32_t)row, channels, elem_bytes, 0};
    b->params[idx] = *params;
    b->origin[idx] = origin;
    b->have[idx].store(1, std::memory_order_release);
}

// Clip idx of batch_out into the staging window: n_frames frames of width x height BGR, each with data either
// its JPEG file (encoded: copied and kept for the window's launch, a slot behind the staged pixels each) or its
// pixels (copied into pinned staging), or without data: the frame before it again.
void stage_clip(aeon_hip_stager* s, void* batch_out, int idx, int n_frames, const aeon_hip::stager_clip_frame* frames,
                bool encoded, int width, int height, int stride, const aeon_aug_params* params)
{
    const size_t row = (size_t)width * 3, bytes = row * height, slot = (bytes + 15) & ~(size_t)15;
    const size_t D   = (size_t)s->frames;
    // aeon's datum dies with provide(): the window's launch reads these copies (made unlocked)
    std::vector<File> files;
    int32_t           distinct = 0;
    for (int d = 0; d < n_frames; d++) {
        if (!frames[d].data) continue;
        distinct++;
        if (!encoded) continue;
        File f;
        f.bytes.reset(new uint8_t[frames[d].size]);
        std::memcpy(f.bytes.get(), frames[d].data, frames[d].size);
        f.size = frames[d].size, f.format = AEON_FORMAT_JPEG, f.mode = AEON_DECODE_BGR8, f.idx = idx, f.frame = d;
        files.push_back(std::move(f));
    }
    std::vector<size_t>   tags((size_t)n_frames, 0);
    std::vector<uint8_t*> dsts((size_t)n_frames, nullptr);
    Batch*                b;
    {
        std::lock_guard<std::mutex> l(s->mu);
        Window& w = staging_window(s);
        b         = &open_batch(s, w, batch_out, idx);
        if (encoded && w.slot_bytes + (size_t)distinct * slot > kOffsetMask) fail(AEON_HIP_EINVAL, "window too large");
        size_t k = 0;
        for (int d = 0; d < n_frames; d++) {
            if (!frames[d].data) {
                tags[d] = tags[d - 1]; // (the first frame has data: the entries check it)
            } else if (encoded) {
                files[k].batch = b;
                w.files.push_back(std::move(files[k++]));
                tags[d] = (size_t)(kSlotChunk << 48) | w.slot_bytes;
                w.slot_bytes += slot;
            } else {
                const auto r = reserve(w, bytes);
                dsts[d]      = w.chunks[r.first].host + r.second;
                tags[d]      = ((size_t)r.first << 48) | r.second;
            }
        }
    }
    // the pixels' copy runs unlocked, on the calling pool thread, as a record's
    for (int d = 0; d < n_frames; d++) {
        if (dsts[d]) {
            if ((size_t)stride == row) std::memcpy(dsts[d], frames[d].data, bytes);
            else
                for (int y = 0; y < height; y++)
                    std::memcpy(dsts[d] + y * row, (const uint8_t*)frames[d].data + (size_t)y * stride, row);
        }
        b->descs[(size_t)idx * D + d] = aeon_img_desc{tags[d], width, height, (int32_t)row, 3, 1, 0};
    }
    b->counts[idx]   = n_frames;
    b->distinct[idx] = distinct;
    b->params[idx]   = *params;
    b->origin[idx]   = encoded ? (uint8_t)(kDeviceDecoded + AEON_FORMAT_JPEG) : kPixels;
    b->have[idx].store(1, std::memory_order_release);
}

// What the two create entries share.
aeon_hip_stager* make_stager(aeon_hip_ctx* ctx, int kind, const aeon_out_desc& out, int batch_size)
{
    auto s   = std::make_unique<aeon_hip_stager>();
    s->ctx   = ctx;
    s->kind  = kind;
    s->out   = out;
    s->batch = batch_size;
    hip_ok(hipGetDevice(&s->device), "hipGetDevice");
    for (Window& w : s->win) {
        hip_ok(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking), "hipStreamCreate");
        hip_ok(hipEventCreateWithFlags(&w.done, hipEventDisableTiming), "hipEventCreate");
    }
    return s.release();
}

} // namespace

extern "C" {

int aeon_hip_stager_create(aeon_hip_ctx* ctx, int kind, const aeon_out_desc* out, int batch_size,
                           aeon_hip_stager** result)
{
    return stager_guarded([&] {
        if (!ctx || !out || !result) fail(AEON_HIP_EINVAL, "null argument");
        if (batch_size <= 0) fail(AEON_HIP_EINVAL, "batch_size must be > 0");
        const int base = kind & ~AEON_STAGER_DEVICE_OUT;
        if (base != AEON_STAGER_IMAGE && base != AEON_STAGER_MASK) fail(AEON_HIP_EINVAL, "unknown stager kind");
        if (base == AEON_STAGER_MASK && (out->dtype == AEON_DTYPE_F16 || out->dtype == AEON_DTYPE_BF16))
            fail(AEON_HIP_EUNSUPPORTED, std::string(out->dtype == AEON_DTYPE_BF16 ? "bfloat16" : "float16") +
                                            " output is implemented for images only, not for pixel masks / depth maps");
        if (out->item_stride == 0) fail(AEON_HIP_EINVAL, "out->item_stride is 0");
        *result = make_stager(ctx, kind, *out, batch_size);
    });
}

int aeon_hip_stager_create_video(aeon_hip_ctx* ctx, int flags, int max_frames, int out_w, int out_h, uint64_t item_stride,
                                 int batch_size, aeon_hip_stager** result)
{
    return stager_guarded([&] {
        if (!ctx || !result) fail(AEON_HIP_EINVAL, "null argument");
        if (batch_size <= 0) fail(AEON_HIP_EINVAL, "batch_size must be > 0");
        if (flags != 0 && flags != AEON_STAGER_DEVICE_OUT) fail(AEON_HIP_EINVAL, "flags must be 0 or AEON_STAGER_DEVICE_OUT");
        // (the decoder's video config refuses the same: one clip must fit one video call)
        if (max_frames <= 0 || max_frames > kVideoCallFrames) fail(AEON_HIP_EINVAL, "invalid max_frame_count");
        if (out_w <= 0 || out_h <= 0) fail(AEON_HIP_EINVAL, "video: invalid max_frame_count or frame size");
        // the video call's own refusal and text (aeon_hip_video_batch), at create time
        const uint64_t hw = (uint64_t)out_w * (uint64_t)out_h;
        if (hw > INT32_MAX || 3 * (uint64_t)max_frames * hw > (uint64_t)INT32_MAX)
            fail(AEON_HIP_EUNSUPPORTED, "video: a clip item above 2^31 - 1 bytes");
        if (item_stride < 3 * (uint64_t)max_frames * hw) fail(AEON_HIP_EINVAL, "video: output item does not fit item_stride");
        aeon_out_desc out{}; // what the video call writes: uint8 planes, channel x frame x height x width
        out.dtype = AEON_DTYPE_U8, out.channels = 3, out.channel_major = 1, out.item_stride = item_stride;
        aeon_hip_stager* s = make_stager(ctx, AEON_STAGER_VIDEO | flags, out, batch_size);
        s->frames = max_frames, s->out_w = out_w, s->out_h = out_h, s->item_bytes = (size_t)(3 * (uint64_t)max_frames * hw);
        *result = s;
    });
}

int aeon_hip_stager_destroy(aeon_hip_stager* s)
{
    if (!s) return 0;
    {
        // no new consumer wait can find this stager once its buffers are unregistered; the ones already
        // inside it finish first
        std::lock_guard<std::mutex> r(g_reg_mu);
        for (auto it = g_pending.begin(); it != g_pending.end();)
            it = it->second.s == s ? g_pending.erase(it) : std::next(it);
    }
    while (s->waiters.load(std::memory_order_acquire) != 0) std::this_thread::yield();
    (void)hipSetDevice(s->device);
    {
        std::lock_guard<std::mutex> l(s->mu);
        for (Window& w : s->win) {
            if (w.state == Window::LAUNCHED) (void)hipEventSynchronize(w.done);
            if (w.stream) (void)aeon_hip_release_stream(s->ctx, w.stream); // (before the stream goes)
            reset_window(s, w);
            for (Chunk& c : w.chunks) (void)hipHostFree(c.host);
            if (w.dev_src) (void)hipFree(w.dev_src);
            if (w.dev_out) (void)hipFree(w.dev_out);
            if (w.done) (void)hipEventDestroy(w.done);
            if (w.stream) (void)hipStreamDestroy(w.stream);
        }
        for (hipEvent_t e : s->spare_events) (void)hipEventDestroy(e);
        s->spare_events.clear();
    }
    delete s;
    return 0;
}

int aeon_hip_stager_stage(aeon_hip_stager* s, void* batch_out, int idx, const void* pixels, int width, int height,
                          int stride, int channels, int elem_bytes, const aeon_aug_params* params)
{
    return stager_guarded([&] {
        if (!s || !batch_out || !pixels || !params) fail(AEON_HIP_EINVAL, "null argument");
        if ((s->kind & ~AEON_STAGER_DEVICE_OUT) == AEON_STAGER_VIDEO)
            fail(AEON_HIP_EINVAL, "aeon_hip_stager_stage on a video stager, which takes clips (aeon_hip_stager_stage_clip / "
                                  "_stage_frames), at idx " + std::to_string(idx));
        if (elem_bytes == 0) elem_bytes = 1;
        check_record(s, idx, width, height, channels, elem_bytes);
        const size_t row = (size_t)width * channels * elem_bytes;
        if (stride == 0) stride = (int)row;
        if ((size_t)stride < row) fail(AEON_HIP_EINVAL, "stride < width * channels * elem_bytes");
        stage_record(s, batch_out, idx, width, height, channels, elem_bytes, params, kPixels, nullptr, [&](uint8_t* dst) {
            if ((size_t)stride == row) std::memcpy(dst, pixels, row * height);
            else
                for (int y = 0; y < height; y++) std::memcpy(dst + y * row, (const uint8_t*)pixels + (size_t)y * stride, row);
        });
    });
}

int aeon_hip_stager_launch(aeon_hip_stager* s, void* batch_out)
{
    return stager_guarded([&] {
        if (!s || !batch_out) fail(AEON_HIP_EINVAL, "null argument");
        std::lock_guard<std::mutex> l(s->mu);
        launch_for(s, batch_out);
    });
}

int aeon_hip_stager_wait(aeon_hip_stager* s, void* batch_out)
{
    return stager_guarded([&] {
        if (!batch_out) fail(AEON_HIP_EINVAL, "null argument");
        if (!s) { // the consumer's form: whichever stager launched this buffer, if any
            {
                // the stager is pinned (waiters) under the registry lock, which its destroy takes to
                // unregister: it cannot go away between the lookup and the wait
                std::lock_guard<std::mutex> r(g_reg_mu);
                auto it = g_pending.find(batch_out);
                if (it == g_pending.end()) return;
                s = it->second.s;
                s->waiters.fetch_add(1, std::memory_order_acq_rel);
            }
            struct Unpin {
                aeon_hip_stager* s;
                ~Unpin() { s->waiters.fetch_sub(1, std::memory_order_acq_rel); }
            } unpin{s};
            bool found = false;
            wait_batch(s, batch_out, found);
            return;
        }
        bool found = false;
        wait_batch(s, batch_out, found);
    });
}

int aeon_hip_stager_flush(aeon_hip_stager* s, void* batch_out)
{
    return stager_guarded([&] {
        if (!s || !batch_out) fail(AEON_HIP_EINVAL, "null argument");
        {
            std::lock_guard<std::mutex> l(s->mu);
            launch_for(s, batch_out);
        }
        bool found = false;
        wait_batch(s, batch_out, found);
        if (!found) fail(AEON_HIP_EINVAL, "batch buffer completed by another thread's wait");
    });
}

int aeon_hip_stager_last_launch(aeon_hip_stager* s, aeon_stager_launch_info* info)
{
    return stager_guarded([&] {
        if (!s || !info) fail(AEON_HIP_EINVAL, "null argument");
        std::lock_guard<std::mutex> l(s->mu);
        *info = s->last;
    });
}

int aeon_hip_stager_last_decode(aeon_hip_stager* s, aeon_stager_decode_info* info)
{
    return stager_guarded([&] {
        if (!s || !info) fail(AEON_HIP_EINVAL, "null argument");
        std::lock_guard<std::mutex> l(s->mu);
        *info = s->last_decode;
    });
}

const char* aeon_hip_stager_last_error(void) { return g_stager_err.c_str(); }

} // extern "C"

// ---- for stager_encoded.cpp (stager_encoded.hpp) ----
namespace aeon_hip {

void stager_set_decode(stager_decode_fn fn) { g_decode.store(fn, std::memory_order_release); }

void stager_describe(const aeon_hip_stager* s, int* base_kind, int* out_channels)
{
    *base_kind    = s->kind & ~AEON_STAGER_DEVICE_OUT;
    *out_channels = s->out.channels;
}

void stager_set_error(const std::string& what) { g_stager_err = what; }

int stager_stage_decoded(aeon_hip_stager* s, void* batch_out, int idx, int width, int height, int channels, int elem_bytes,
                         const aeon_aug_params* params, int format, stager_fill_fn fill_fn, void* arg)
{
    int rc = 0;
    const int guard = stager_guarded([&] {
        check_record(s, idx, width, height, channels, elem_bytes);
        const size_t row = (size_t)width * channels * elem_bytes;
        stage_record(s, batch_out, idx, width, height, channels, elem_bytes, params, (uint8_t)(kHostDecoded + format),
                     nullptr, [&](uint8_t* dst) {
                         rc = fill_fn(arg, dst, row);
                         if (rc != 0) throw stager_error(rc, g_stager_err); // (the text is fill's)
                     });
    });
    return guard;
}

int stager_stage_file(aeon_hip_stager* s, void* batch_out, int idx, int width, int height, int channels, int elem_bytes,
                      const aeon_aug_params* params, int format, int mode, std::unique_ptr<uint8_t[]> bytes, size_t size)
{
    return stager_guarded([&] {
        check_record(s, idx, width, height, channels, elem_bytes);
        File f;
        f.bytes = std::move(bytes), f.size = size, f.format = format, f.mode = mode;
        stage_record(s, batch_out, idx, width, height, channels, elem_bytes, params, (uint8_t)(kDeviceDecoded + format), &f,
                     [](uint8_t*) {});
    });
}

// ---- for stager_clip.cpp (stager_clip.hpp) ----
void stager_set_clip_hooks(stager_decode_fn decode, stager_video_fn video)
{
    g_clip_decode.store(decode, std::memory_order_release);
    g_video.store(video, std::memory_order_release);
}

void stager_clip_describe(const aeon_hip_stager* s, stager_clip_shape* shape)
{
    *shape = stager_clip_shape{s->kind & ~AEON_STAGER_DEVICE_OUT, s->frames, s->out_w, s->out_h};
}

int stager_stage_clip_frames(aeon_hip_stager* s, void* batch_out, int idx, int n_frames, const stager_clip_frame* frames,
                             int encoded, int width, int height, int stride, const aeon_aug_params* params)
{
    return stager_guarded([&] {
        const std::string at = ", at idx " + std::to_string(idx);
        if ((s->kind & ~AEON_STAGER_DEVICE_OUT) != AEON_STAGER_VIDEO) fail(AEON_HIP_EINVAL, "not a video stager" + at);
        if (idx < 0 || idx >= s->batch) fail(AEON_HIP_EINVAL, "idx out of range of the batch");
        if (n_frames < 1 || n_frames > s->frames)
            fail(AEON_HIP_EINVAL, "n_frames " + std::to_string(n_frames) + " outside [1, max_frames " +
                                      std::to_string(s->frames) + "]" + at);
        if (!frames[0].data) fail(AEON_HIP_EINVAL, "the first frame of a clip has no data" + at);
        if (width <= 0 || height <= 0) fail(AEON_HIP_EINVAL, "received encoded video with size 0" + at);
        if (params->out_w != s->out_w || params->out_h != s->out_h)
            fail(AEON_HIP_EINVAL, "params' output size " + std::to_string(params->out_w) + "x" + std::to_string(params->out_h) +
                                      " is not the stager's " + std::to_string(s->out_w) + "x" + std::to_string(s->out_h) + at);
        if (!encoded && (size_t)stride < (size_t)width * 3) fail(AEON_HIP_EINVAL, "stride < width * 3" + at);
        stage_clip(s, batch_out, idx, n_frames, frames, encoded != 0, width, height, stride, params);
    });
}

} // namespace aeon_hip
