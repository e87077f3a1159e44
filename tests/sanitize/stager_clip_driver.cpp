// stager_clip_driver.cpp -- the stager's video half (aeon_amd/csrc/stager.cpp + stager_clip.cpp, with the demux,
// the JPEG header parser and abi_host.cpp as they are) over the decoding model device (model_decode.cpp) and the
// model of the video call (model_video.cpp), as a stand-alone program for the sanitizer builds (Makefile targets
// sanitize_stager_clip: ASan + UBSan, tsan_stager_clip: ThreadSanitizer; tests/test_stager_clip.py runs both).
// Each scenario prints one line, "name\tok" or "name\tFAIL what", and the program exits non-zero when any failed.
// argv[1] is the time limit in seconds (alarm() ends a scenario that spins).
//   stager_clip_driver [seconds [scenario ...]]
// The clips: every frame is a header the library's JPEG parser accepts around arbitrary bytes, which the model's
// JPEG stage "decodes" to a pattern of the file's hash; the driver writes the frames into an MJPEG AVI of its own
// (second form) or hands the patterns over as decoded frames (first form), and expects the model's per-clip
// checksum over those patterns either way.  Every item of every batch buffer is compared, with the bytes between
// the items, and the counts are read from aeon_hip_stager_last_launch / _last_decode.
#include <hip/hip_runtime_api.h>
#include <signal.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/aeon_hip.h"
#include "model_decode.hpp"
#include "model_video.hpp"

namespace {

char          g_ctx_storage; // the stager only passes its context on to the (model's) entries
aeon_hip_ctx* ctx() { return reinterpret_cast<aeon_hip_ctx*>(&g_ctx_storage); }

struct Failure {
    std::string what;
};
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            char m_[512];                                  \
            std::snprintf(m_, sizeof(m_), __VA_ARGS__);    \
            throw Failure{std::string(#cond) + ": " + m_}; \
        }                                                  \
    } while (0)
#define OK(call)                                                                              \
    do {                                                                                      \
        const int rc_ = (call);                                                               \
        if (rc_ != 0) throw Failure{std::string(#call) + " -> " + std::to_string(rc_) + " " + \
                                    aeon_hip_stager_last_error()};                            \
    } while (0)

using Bytes = std::vector<uint8_t>;
constexpr uint8_t kFill = 0xEE;
constexpr size_t  kGap  = 5; // bytes between the items of a batch buffer

uint64_t next(uint64_t& x)
{
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x;
}

void fill(uint8_t* p, size_t n, uint64_t seed)
{
    uint64_t x = seed * 0x9e3779b97f4a7c15ull + 0x2545f4914f6cdd1dull;
    for (size_t k = 0; k < n; k++) p[k] = (uint8_t)(next(x) >> 32);
}

void put16(Bytes& b, unsigned v, bool big = false)
{
    if (big) b.push_back((uint8_t)(v >> 8)), b.push_back((uint8_t)v);
    else b.push_back((uint8_t)v), b.push_back((uint8_t)(v >> 8));
}
void put32(Bytes& b, uint32_t v)
{
    for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * k)));
}
void append(Bytes& b, const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); }
void append(Bytes& b, const Bytes& o) { b.insert(b.end(), o.begin(), o.end()); }

// A frame header the library's JPEG parser accepts (SOI, SOF0 of three 1x1-sampled components) around bytes of the
// frame's own; the model "decodes" it to a pattern of the whole file's hash.
Bytes write_jpeg(int w, int h, uint64_t seed)
{
    Bytes f{0xFF, 0xD8, 0xFF, 0xC0};
    put16(f, 17, true);
    f.push_back(8), put16(f, (unsigned)h, true), put16(f, (unsigned)w, true), f.push_back(3);
    for (uint8_t id = 1; id <= 3; id++) f.push_back(id), f.push_back(0x11), f.push_back(0);
    const size_t at = f.size();
    f.resize(at + 60 + seed % 41);
    fill(f.data() + at, f.size() - at, seed);
    f.push_back(0xFF), f.push_back(0xD9);
    return f;
}

Bytes chunk(const char* cc, const Bytes& payload)
{
    Bytes c;
    append(c, cc, 4), put32(c, (uint32_t)payload.size()), append(c, payload);
    if (payload.size() & 1) c.push_back(0);
    return c;
}
Bytes list(const char* kind, const Bytes& payload)
{
    Bytes c;
    append(c, "LIST", 4), put32(c, (uint32_t)(4 + payload.size())), append(c, kind, 4), append(c, payload);
    return c;
}

// An MJPEG AVI over `frames` (an empty one: an empty chunk): hdrl / avih with the index flag, one vids / MJPG strl,
// a JUNK chunk, movi with 00dc chunks, idx1 with offsets from the movi fourcc.
Bytes write_avi(const std::vector<Bytes>& frames, int w, int h, uint32_t flags = 0x10)
{
    const uint32_t n = (uint32_t)frames.size();
    Bytes          avih, strh, strf;
    for (uint32_t v : {40000u, 0u, 0u, flags, n, 0u, 1u, 0u, (uint32_t)w, (uint32_t)h, 0u, 0u, 0u, 0u}) put32(avih, v);
    append(strh, "vidsMJPG", 8);
    for (uint32_t v : {0u, 0u, 0u, 1u, 25u, 0u, n, 0u, 0u, 0u}) put32(strh, v);
    put16(strh, 0), put16(strh, 0), put16(strh, (unsigned)w), put16(strh, (unsigned)h);
    put32(strf, 40), put32(strf, (uint32_t)w), put32(strf, (uint32_t)h), put16(strf, 1), put16(strf, 24);
    append(strf, "MJPG", 4);
    for (uint32_t v : {(uint32_t)(w * h * 3), 0u, 0u, 0u, 0u}) put32(strf, v);
    Bytes strl = chunk("strh", strh);
    append(strl, chunk("strf", strf));
    Bytes hdrl = chunk("avih", avih);
    append(hdrl, list("strl", strl));
    Bytes movi, idx;
    for (const Bytes& f : frames) {
        append(idx, "00dc", 4), put32(idx, 0x10), put32(idx, (uint32_t)(4 + movi.size())), put32(idx, (uint32_t)f.size());
        append(movi, chunk("00dc", f));
    }
    Bytes body = list("hdrl", hdrl);
    append(body, chunk("JUNK", Bytes(12, 0)));
    append(body, list("movi", movi));
    append(body, chunk("idx1", idx));
    Bytes avi;
    append(avi, "RIFF", 4), put32(avi, (uint32_t)(4 + body.size())), append(avi, "AVI ", 4), append(avi, body);
    return avi;
}

// ---- clips: the geometry of clip (b, i) is the same in every window, its frames differ ----
struct Shape {
    int nb, nr;       // batches per window, clips per batch
    int D, ow, oh;    // the stager's max_frames and output size
    int form;         // 1: every clip as its AVI; 0: as decoded frames; -1: alternating
    size_t item() const { return 3 * (size_t)D * oh * ow; }
    size_t stride() const { return item() + kGap; }
};

struct Clip {
    int                w, h, kept, distinct;
    bool               encoded;
    std::vector<Bytes> frames; // the AVI's frames, JPEG files; empty: repeats the one before
    std::vector<Bytes> px;     // the kept frames' patterns (empty where the frame repeats)
    Bytes              avi;
    aeon_aug_params    p;
    Bytes              want;   // the model's clip
};

Clip make_clip(const Shape& sh, int win, int b, int i)
{
    Clip c;
    c.w = 6 + 3 * i + b, c.h = 4 + 2 * ((i + b) % 3);
    c.kept           = 1 + (2 * i + b) % sh.D;
    const int in_avi = c.kept == sh.D && i % 2 ? c.kept + 2 : c.kept; // (some files hold more frames than are kept)
    c.encoded        = sh.form < 0 ? ((b * sh.nr + i + win) & 1) != 0 : sh.form != 0;
    const uint64_t seed = ((uint64_t)(win + 1) << 32) ^ (uint64_t)(b * 131 + i + 1);
    for (int d = 0; d < in_avi; d++)
        c.frames.push_back(d > 0 && (d + i) % 3 == 2 ? Bytes() : write_jpeg(c.w, c.h, seed * 64 + d));
    c.avi = write_avi(c.frames, c.w + 1, c.h + 1); // (avih's size is not the frames': the stager must not use it)
    std::memset(&c.p, 0, sizeof(c.p));
    c.p.crop_x = win, c.p.crop_y = b, c.p.crop_w = c.w - win % 3, c.p.crop_h = c.h - 1;
    c.p.out_w = sh.ow, c.p.out_h = sh.oh, c.p.flip = (win + i) & 1;
    // the expected clip: the kept frames' patterns in an arena of the driver's own
    Bytes                      arena;
    std::vector<aeon_img_desc> row;
    c.distinct = 0;
    for (int d = 0; d < c.kept; d++) {
        if (c.frames[d].empty()) {
            row.push_back(row.back());
            c.px.push_back(Bytes());
            continue;
        }
        const aeon_img_desc desc{arena.size(), c.w, c.h, c.w * 3, 3, 1, 0};
        Bytes               px((size_t)c.w * c.h * 3);
        model_jpeg_pattern(c.frames[d].data(), c.frames[d].size(), desc, px.data());
        append(arena, px);
        c.px.push_back(std::move(px));
        row.push_back(desc);
        c.distinct++;
    }
    c.want.assign(sh.item(), 0);
    model_clip_output(arena.data(), row.data(), c.kept, sh.D, sh.ow, sh.oh, c.p, c.want.data());
    return c;
}

int stage_clip(aeon_hip_stager* s, uint8_t* buf, int i, const Clip& c)
{
    if (c.encoded) {
        // aeon's datum dies with provide(): the stager must have copied what it needs
        Bytes     gone(c.avi);
        const int rc = aeon_hip_stager_stage_clip(s, buf, i, gone.data(), gone.size(), &c.p);
        std::memset(gone.data(), 0xDD, gone.size());
        return rc;
    }
    std::vector<Bytes>       gone(c.px);
    std::vector<const void*> ptrs;
    for (const Bytes& f : gone) ptrs.push_back(f.empty() ? nullptr : f.data());
    const int rc = aeon_hip_stager_stage_frames(s, buf, i, c.kept, ptrs.data(), c.w, c.h, 0, &c.p);
    for (Bytes& f : gone)
        if (!f.empty()) std::memset(f.data(), 0xDD, f.size());
    return rc;
}

struct Buffers { // the batch buffers of one container: pageable, or the model's mapped host memory
    std::vector<uint8_t*> p;
    size_t                bytes;
    bool                  mapped;
    Buffers(const Shape& sh, bool mapped_) : bytes(sh.nr * sh.stride()), mapped(mapped_)
    {
        for (int b = 0; b < sh.nb; b++) {
            void* q = nullptr;
            if (mapped) {
                if (hipHostMalloc(&q, bytes, 0) != hipSuccess) std::abort();
            } else {
                q = std::malloc(bytes);
            }
            std::memset(q, kFill, bytes);
            p.push_back((uint8_t*)q);
        }
    }
    Buffers(const Buffers&)            = delete;
    Buffers& operator=(const Buffers&) = delete;
    ~Buffers()
    {
        for (uint8_t* q : p) mapped ? (void)hipHostFree(q) : std::free(q);
    }
};

struct StagerHandle {
    aeon_hip_stager* s = nullptr;
    explicit StagerHandle(const Shape& sh) { OK(aeon_hip_stager_create_video(ctx(), 0, sh.D, sh.ow, sh.oh, sh.stride(), sh.nr, &s)); }
    StagerHandle(const StagerHandle&)            = delete;
    StagerHandle& operator=(const StagerHandle&) = delete;
    void destroy()
    {
        if (s) OK(aeon_hip_stager_destroy(s));
        s = nullptr;
    }
    ~StagerHandle()
    {
        if (s) (void)aeon_hip_stager_destroy(s);
    }
};

// provide() for every clip of window `win` into `bufs`, from `threads` threads (clips dealt round robin, so both
// forms of one batch are staged concurrently).  skip: a clip left out (-1: none).
void stage_window(aeon_hip_stager* s, const Shape& sh, Buffers& bufs, int win, int threads, int skip = -1)
{
    std::mutex  mu;
    std::string err;
    auto        work = [&](int t) {
        for (int k = t; k < sh.nb * sh.nr; k += threads) {
            if (k == skip) continue;
            const Clip c  = make_clip(sh, win, k / sh.nr, k % sh.nr);
            const int  rc = stage_clip(s, bufs.p[k / sh.nr], k % sh.nr, c);
            if (rc != 0) {
                std::lock_guard<std::mutex> l(mu);
                err = std::string("stage ") + (c.encoded ? "clip" : "frames") + " -> " + std::to_string(rc) + " " +
                      aeon_hip_stager_last_error();
            }
        }
    };
    if (threads <= 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++) pool.emplace_back(work, t);
        for (auto& t : pool) t.join();
    }
    if (!err.empty()) throw Failure{err};
}

void verify_batch(const Shape& sh, const uint8_t* buf, int win, int b, int n = -1)
{
    for (int i = 0; i < (n < 0 ? sh.nr : n); i++) {
        const Clip c = make_clip(sh, win, b, i);
        CHECK(std::memcmp(buf + i * sh.stride(), c.want.data(), sh.item()) == 0, "window %d batch %d clip %d (%s) differs", win, b, i,
              c.encoded ? "clip" : "frames");
        for (size_t g = 0; g < kGap; g++)
            CHECK(buf[i * sh.stride() + sh.item() + g] == kFill, "window %d batch %d: the bytes behind clip %d were written", win, b, i);
    }
}

void expect_untouched(const Buffers& bufs)
{
    for (size_t b = 0; b < bufs.p.size(); b++)
        for (size_t i = 0; i < bufs.bytes; i++) CHECK(bufs.p[b][i] == kFill, "a dropped window wrote batch %zu", b);
}

// The counts a whole window must report: clips as records, frames by where they were decoded.
void expect_window(aeon_hip_stager* s, const Shape& sh, int win, uint64_t launches, int direct)
{
    int files = 0, pixels = 0;
    for (int b = 0; b < sh.nb; b++)
        for (int i = 0; i < sh.nr; i++) {
            const Clip c = make_clip(sh, win, b, i);
            (c.encoded ? files : pixels) += c.distinct;
        }
    aeon_stager_decode_info d;
    OK(aeon_hip_stager_last_decode(s, &d));
    CHECK(d.launches == launches && d.device[AEON_FORMAT_JPEG] == files && d.pixels == pixels && d.device[1] + d.device[2] + d.device[3] == 0 &&
              d.host[0] + d.host[1] + d.host[2] + d.host[3] == 0,
          "last_decode {launches %llu, jpeg %d, pixels %d}, expected {%llu, %d, %d}", (unsigned long long)d.launches,
          d.device[AEON_FORMAT_JPEG], d.pixels, (unsigned long long)launches, files, pixels);
    aeon_stager_launch_info i;
    OK(aeon_hip_stager_last_launch(s, &i));
    const int zero_copy = direct && files == 0;
    CHECK(i.launches == launches && i.src_zero_copy == zero_copy && i.out_direct == direct && i.records == sh.nb * sh.nr,
          "launch info {launches %llu, zero_copy %d, direct %d, records %d}, expected {%llu, %d, %d, %d}",
          (unsigned long long)i.launches, i.src_zero_copy, i.out_direct, i.records, (unsigned long long)launches, zero_copy, direct,
          sh.nb * sh.nr);
}

void expect_single_upload()
{
    CHECK(model_double_uploads() == 0, "%ld encoded frames lay in a range a host-to-device copy carried as well",
          model_double_uploads());
}

const Shape kMixed{2, 8, 5, 7, 5, -1};

// ---- scenarios ----
// Eight threads staging both forms of one window concurrently; then a window of each form alone.
void both_forms_8_threads()
{
    for (int form : {-1, 1, 0}) {
        Shape sh = kMixed;
        sh.form  = form;
        StagerHandle st(sh);
        Buffers      bufs(sh, true);
        stage_window(st.s, sh, bufs, 0, 8);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
        expect_window(st.s, sh, 0, 1, 1);
        for (int b = 0; b < sh.nb; b++) verify_batch(sh, bufs.p[b], 0, b);
        CHECK(model_video_calls() > 0 && model_video_max_frames() <= sh.nr * sh.D, "%ld video calls", model_video_calls());
        expect_single_upload();
        st.destroy();
    }
    CHECK(model_video_calls() == 3 * kMixed.nb, "%ld video calls for 3 windows of %d batches", model_video_calls(), kMixed.nb);
}

// Two windows in flight over two containers, and a third staged over a first nobody waited for.
void two_windows_and_a_third()
{
    const Shape  sh = kMixed;
    StagerHandle st(sh);
    Buffers      w0(sh, false), w1(sh, false), w2(sh, false);
    Buffers*     wins[3] = {&w0, &w1, &w2};
    for (int win = 0; win < 3; win++) {
        stage_window(st.s, sh, *wins[win], win, 4);
        if (win == 2) // staging window 2 completed window 0 and dropped it: its buffers are filled
            for (int b = 0; b < sh.nb; b++) verify_batch(sh, w0.p[b], 0, b);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_launch(st.s, wins[win]->p[b]));
        expect_window(st.s, sh, win, win + 1, 0);
    }
    for (int win = 1; win < 3; win++)
        for (int b = 0; b < sh.nb; b++) {
            OK(aeon_hip_stager_wait(st.s, wins[win]->p[b]));
            verify_batch(sh, wins[win]->p[b], win, b);
        }
    expect_single_upload();
    st.destroy();
}

// A batch staged with a hole: the launch refuses, the window is dropped whole, the next one is right.
void hole_in_a_batch()
{
    const Shape  sh = kMixed;
    StagerHandle st(sh);
    Buffers      bufs(sh, false);
    stage_window(st.s, sh, bufs, 0, 4, 1 * sh.nr + 2);
    const int rc = aeon_hip_stager_launch(st.s, bufs.p[0]);
    CHECK(rc == AEON_HIP_EINVAL && std::strstr(aeon_hip_stager_last_error(), "hole"), "launch returned %d '%s'", rc,
          aeon_hip_stager_last_error());
    for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_wait(st.s, bufs.p[b])); // nothing to wait for
    expect_untouched(bufs);
    stage_window(st.s, sh, bufs, 1, 4);
    for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
    expect_window(st.s, sh, 1, 1, 0);
    for (int b = 0; b < sh.nb; b++) verify_batch(sh, bufs.p[b], 1, b);
    st.destroy();
}

// Clips refused in mid-window: the code and text with the idx, the window usable, the idx staged again.
void refused_clip_restaged()
{
    const Shape  sh = kMixed;
    StagerHandle st(sh);
    Buffers      bufs(sh, true);
    const int    bad_k = 1 * sh.nr + 3; // batch 1, idx 3
    stage_window(st.s, sh, bufs, 0, 4, bad_k);
    const Clip c = make_clip(sh, 0, 1, 3);
    struct Case {
        Bytes       avi;
        int         code;
        const char* text;
    };
    std::vector<Bytes> other_size{write_jpeg(c.w, c.h, 1), write_jpeg(c.w, c.h, 2), write_jpeg(c.w + 1, c.h, 3)};
    std::vector<Bytes> bad_header{write_jpeg(c.w, c.h, 1), Bytes{0xFF, 0xD8, 0xFF, 0xC0, 0x00}};
    Bytes              cut = c.avi;
    cut.resize(cut.size() / 2); // (the index is gone)
    Bytes not_avi = c.avi;
    not_avi[3]    = 'X';
    char size_text[96];
    std::snprintf(size_text, sizeof(size_text), "video: frame 2 is %dx%d, the first frame %dx%d, at idx 3", c.w + 1, c.h, c.w, c.h);
    const Case cases[] = {{write_avi(other_size, c.w, c.h), AEON_HIP_EINVAL, size_text},
                          {write_avi(bad_header, c.w, c.h), AEON_HIP_EINVAL, "JPEG: truncated marker segment, at idx 3"},
                          {write_avi(c.frames, c.w, c.h, 0), AEON_HIP_EINVAL, "Not a valid AVI file type, at idx 3"},
                          {cut, AEON_HIP_EINVAL, ", at idx 3"},
                          {not_avi, AEON_HIP_EINVAL, "avi: not a RIFF AVI file, at idx 3"},
                          {Bytes(), AEON_HIP_EINVAL, "received encoded video with size 0, at idx 3"}};
    for (const Case& k : cases) {
        const int rc = aeon_hip_stager_stage_clip(st.s, bufs.p[1], 3, k.avi.data(), k.avi.size(), &c.p);
        CHECK(rc == k.code && std::strstr(aeon_hip_stager_last_error(), k.text), "a refused clip returned %d '%s', expected '%s'", rc,
              aeon_hip_stager_last_error(), k.text);
    }
    // the first form's refusals
    std::vector<const void*> ptrs((size_t)sh.D + 1, c.px[0].data());
    int rc = aeon_hip_stager_stage_frames(st.s, bufs.p[1], 3, sh.D + 1, ptrs.data(), c.w, c.h, 0, &c.p);
    CHECK(rc == AEON_HIP_EINVAL && std::strstr(aeon_hip_stager_last_error(), "n_frames") && std::strstr(aeon_hip_stager_last_error(), ", at idx 3"),
          "n_frames above max_frames returned %d '%s'", rc, aeon_hip_stager_last_error());
    ptrs[0] = nullptr;
    rc      = aeon_hip_stager_stage_frames(st.s, bufs.p[1], 3, 2, ptrs.data(), c.w, c.h, 0, &c.p);
    CHECK(rc == AEON_HIP_EINVAL, "a clip without a first frame returned %d", rc);
    aeon_aug_params other = c.p;
    other.out_w++;
    rc = aeon_hip_stager_stage_clip(st.s, bufs.p[1], 3, c.avi.data(), c.avi.size(), &other);
    CHECK(rc == AEON_HIP_EINVAL && std::strstr(aeon_hip_stager_last_error(), "output size"), "other params returned %d '%s'", rc,
          aeon_hip_stager_last_error());
    rc = aeon_hip_stager_stage(st.s, bufs.p[1], 3, c.px[0].data(), c.w, c.h, 0, 3, 1, &c.p);
    CHECK(rc == AEON_HIP_EINVAL && std::strstr(aeon_hip_stager_last_error(), "video stager"), "stage returned %d '%s'", rc,
          aeon_hip_stager_last_error());
    OK(stage_clip(st.s, bufs.p[1], 3, c));
    const int twice = stage_clip(st.s, bufs.p[1], 3, c);
    CHECK(twice == AEON_HIP_EINVAL && std::strstr(aeon_hip_stager_last_error(), "staged twice"), "a second stage returned %d '%s'", twice,
          aeon_hip_stager_last_error());
    for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
    expect_window(st.s, sh, 0, 1, 1);
    for (int b = 0; b < sh.nb; b++) verify_batch(sh, bufs.p[b], 0, b);
    expect_single_upload();
    // aeon_clip_info: kept, and the first frame's size -- not avih's
    int kept = 0, w = 0, h = 0;
    CHECK(aeon_clip_info(c.avi.data(), c.avi.size(), sh.D, &kept, &w, &h) == 0 && kept == c.kept && w == c.w && h == c.h,
          "aeon_clip_info: %d frames of %dx%d, expected %d of %dx%d", kept, w, h, c.kept, c.w, c.h);
    st.destroy();
}

// The JPEG call, then the video call, fails at launch: the window is dropped whole, nothing is written, the next
// window is right.
void batch_call_fails()
{
    Shape sh = kMixed;
    sh.form  = 1;
    StagerHandle st(sh);
    Buffers      bufs(sh, false);
    uint64_t     launches = 0;
    for (int k = 0; k < 2; k++) {
        stage_window(st.s, sh, bufs, 2 * k, 4);
        if (k == 0) model_fail_call("aeon_hip_decode_jpeg_batch", 1, AEON_HIP_ERUNTIME);
        else model_video_fail_call(1, AEON_HIP_EDEVICE);
        int rc = aeon_hip_stager_launch(st.s, bufs.p[0]);
        CHECK(rc == (k == 0 ? AEON_HIP_ERUNTIME : AEON_HIP_EDEVICE) &&
                  std::strstr(aeon_hip_stager_last_error(), k == 0 ? "aeon_hip_decode_jpeg_batch" : "aeon_hip_video_batch"),
              "launch returned %d '%s'", rc, aeon_hip_stager_last_error());
        rc = aeon_hip_stager_launch(st.s, bufs.p[1]);
        CHECK(rc == AEON_HIP_EINVAL, "the dropped window's other batch launched: %d", rc);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_wait(st.s, bufs.p[b])); // nothing to wait for
        expect_untouched(bufs);
        stage_window(st.s, sh, bufs, 2 * k + 1, 4);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
        expect_window(st.s, sh, 2 * k + 1, ++launches, 0);
        for (int b = 0; b < sh.nb; b++) {
            verify_batch(sh, bufs.p[b], 2 * k + 1, b);
            std::memset(bufs.p[b], kFill, bufs.bytes);
        }
    }
    expect_single_upload();
    st.destroy();
}

// The consumer's wait: by buffer alone, from threads of its own, with a short last batch.
void wait_by_buffer()
{
    const Shape  sh = kMixed;
    StagerHandle st(sh);
    Buffers      c0(sh, false), c1(sh, true);
    Buffers*     cont[2] = {&c0, &c1};
    for (int win = 0; win < 4; win++) {
        Buffers& bufs = *cont[win % 2];
        stage_window(st.s, sh, bufs, win, 4, win == 3 ? sh.nb * sh.nr - 1 : -1); // (window 3: its last batch is one short)
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_launch(st.s, bufs.p[b]));
        std::vector<std::thread> consumers;
        std::vector<int>         rcs(sh.nb, -99);
        for (int b = 0; b < sh.nb; b++)
            consumers.emplace_back([&, b] { rcs[b] = aeon_hip_stager_wait(nullptr, bufs.p[b]); });
        for (auto& t : consumers) t.join();
        for (int b = 0; b < sh.nb; b++) {
            CHECK(rcs[b] == 0, "wait(NULL, batch %d) of window %d returned %d", b, win, rcs[b]);
            verify_batch(sh, bufs.p[b], win, b, win == 3 && b == sh.nb - 1 ? sh.nr - 1 : -1);
            std::memset(bufs.p[b], kFill, bufs.bytes);
        }
        OK(aeon_hip_stager_wait(nullptr, bufs.p[0])); // already waited for: returns at once
    }
    st.destroy();
}

// Destroy with a window launched and never waited for, and another one half staged.
void destroy_with_window_launched()
{
    const Shape  sh = kMixed;
    StagerHandle st(sh);
    Buffers      w0(sh, false), w1(sh, true);
    stage_window(st.s, sh, w0, 0, 4);
    for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_launch(st.s, w0.p[b]));
    stage_window(st.s, sh, w1, 1, 4, 3);
    st.destroy();
    OK(aeon_hip_stager_wait(nullptr, w0.p[0])); // no stager holds the buffer any more
}

// A batch of more frames than one video call takes: 70 clips of 1,000 frames (one picture and its repeats).
void split_above_65535_frames()
{
    const int        n = 70, D = 1000, ow = 2, oh = 2;
    const size_t     item = 3 * (size_t)D * oh * ow, stride = item + kGap;
    aeon_hip_stager* s = nullptr;
    OK(aeon_hip_stager_create_video(ctx(), 0, D, ow, oh, stride, n, &s));
    Bytes           buf(n * stride, kFill), px(3 * 2 * 3);
    aeon_aug_params p;
    std::memset(&p, 0, sizeof(p));
    p.crop_w = 3, p.crop_h = 2, p.out_w = ow, p.out_h = oh;
    std::vector<const void*>   ptrs((size_t)D, nullptr);
    std::vector<aeon_img_desc> row((size_t)D, aeon_img_desc{0, 3, 2, 9, 3, 1, 0});
    for (int i = 0; i < n; i++) {
        fill(px.data(), px.size(), 77 + i);
        ptrs[0] = px.data();
        OK(aeon_hip_stager_stage_frames(s, buf.data(), i, D, ptrs.data(), 3, 2, 0, &p));
    }
    OK(aeon_hip_stager_flush(s, buf.data()));
    CHECK(model_video_calls() == 2 && model_video_max_frames() == 65000, "%ld video calls, the largest of %ld frames",
          model_video_calls(), model_video_max_frames());
    Bytes want(item);
    for (int i = 0; i < n; i++) {
        fill(px.data(), px.size(), 77 + i);
        model_clip_output(px.data(), row.data(), D, D, ow, oh, p, want.data());
        CHECK(std::memcmp(buf.data() + i * stride, want.data(), item) == 0, "clip %d differs", i);
        CHECK(buf[i * stride + item] == kFill, "the bytes behind clip %d were written", i);
    }
    aeon_stager_decode_info d;
    OK(aeon_hip_stager_last_decode(s, &d));
    CHECK(d.pixels == n && d.device[AEON_FORMAT_JPEG] == 0, "pixels %d", d.pixels);
    OK(aeon_hip_stager_destroy(s));
}

// ---- the program ----
const char* g_running = "";

void on_alarm(int)
{
    char          line[160];
    const int     n = std::snprintf(line, sizeof(line), "%s\tFAIL time limit: the scenario did not return\n", g_running);
    const ssize_t r = write(1, line, n > 0 ? (size_t)n : 0);
    (void)r;
    _exit(3);
}

} // namespace

int main(int argc, char** argv)
{
    const int seconds = argc > 1 ? std::atoi(argv[1]) : 120;
    signal(SIGALRM, on_alarm);
    alarm(seconds > 0 ? seconds : 120);
    const std::vector<std::pair<std::string, std::function<void()>>> scenarios = {
        {"both_forms_8_threads", both_forms_8_threads},
        {"two_windows_and_a_third", two_windows_and_a_third},
        {"hole_in_a_batch", hole_in_a_batch},
        {"refused_clip_restaged", refused_clip_restaged},
        {"batch_call_fails", batch_call_fails},
        {"wait_by_buffer", wait_by_buffer},
        {"destroy_with_window_launched", destroy_with_window_launched},
        {"split_above_65535_frames", split_above_65535_frames},
    };
    int failed = 0;
    for (const auto& sc : scenarios) {
        bool wanted = argc <= 2;
        for (int k = 2; k < argc; k++) wanted = wanted || sc.first == argv[k];
        if (!wanted) continue;
        g_running = sc.first.c_str();
        model_reset();
        model_video_reset();
        std::string res = "ok";
        try {
            sc.second();
        } catch (const Failure& f) {
            res = "FAIL " + f.what;
            failed++;
        }
        std::printf("%s\t%s\n", sc.first.c_str(), res.c_str());
        std::fflush(stdout);
    }
    return failed ? 1 : 0;
}
