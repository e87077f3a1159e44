// stager_driver.cpp -- the stager (aeon_amd/csrc/stager.cpp) over the model device (model_device.cpp), as a
// stand-alone program for the sanitizer builds (Makefile targets sanitize_stager: ASan + UBSan, tsan_stager:
// ThreadSanitizer; tests/test_sanitize_stager.py runs both).  Each scenario prints one line,
// "name\tok" or "name\tFAIL what", and the program exits non-zero when any failed.  argv[1] is the time limit
// in seconds: alarm() ends a scenario that spins (the `copying` count left raised did) with a FAIL line.
//   stager_driver [seconds [scenario ...]]
#include <hip/hip_runtime_api.h>
#include <signal.h>
#include <unistd.h>

#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/aeon_hip.h"
#include "model_device.hpp"

namespace {

char          g_ctx_storage; // the stager only passes its context on to the (model's) batch entries
aeon_hip_ctx* ctx() { return reinterpret_cast<aeon_hip_ctx*>(&g_ctx_storage); }

struct Failure {
    std::string what;
};
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            char m_[512];                                                 \
            std::snprintf(m_, sizeof(m_), __VA_ARGS__);                   \
            throw Failure{std::string(#cond) + ": " + m_};                \
        }                                                                 \
    } while (0)
#define OK(call)                                                                             \
    do {                                                                                     \
        const int rc_ = (call);                                                              \
        if (rc_ != 0) throw Failure{std::string(#call) + " -> " + std::to_string(rc_) + " " + \
                                    aeon_hip_stager_last_error()};                           \
    } while (0)

// ---- records: the size of record (b, i) is the same in every window, its pixels differ per window ----
struct Shape {
    int    nb, nr;    // batches per window, records per batch
    size_t item;      // out.item_stride
    int    kind;      // AEON_STAGER_IMAGE / AEON_STAGER_MASK
};

void record_size(int b, int i, int kind, int& w, int& h, int& c)
{
    w = 9 + 5 * i + 2 * b; // odd and even widths
    h = 6 + 3 * ((i + b) % 3);
    c = kind == AEON_STAGER_MASK ? 1 : 3;
}

void fill(uint8_t* p, size_t n, uint64_t seed)
{
    uint64_t x = seed * 0x9e3779b97f4a7c15ull + 0x2545f4914f6cdd1dull;
    size_t   k = 0;
    for (; k + 8 <= n; k += 8) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        std::memcpy(p + k, &x, 8);
    }
    for (; k < n; k++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        p[k] = (uint8_t)x;
    }
}

aeon_aug_params params_of(int win, int b, int i, int w, int h)
{
    aeon_aug_params p;
    std::memset(&p, 0, sizeof(p));
    p.crop_x = win, p.crop_y = b, p.crop_w = w - win % 3, p.crop_h = h - 1;
    p.out_w = 7 + i, p.out_h = 5 + b;
    p.flip = (win + i) & 1;
    return p;
}

uint64_t model_kind(int kind) { return kind == AEON_STAGER_MASK ? MODEL_KIND_MASK : MODEL_KIND_AUGMENT; }

// The record's pixels and what the model writes for it.
void make_record(const Shape& sh, int win, int b, int i, std::vector<uint8_t>& px, int& w, int& h, int& c,
                 aeon_aug_params& p, std::vector<uint8_t>& want)
{
    record_size(b, i, sh.kind, w, h, c);
    px.resize((size_t)w * h * c);
    fill(px.data(), px.size(), ((uint64_t)win << 32) ^ (uint64_t)(b * 131 + i + 1));
    p = params_of(win, b, i, w, h);
    want.resize(sh.item);
    model_record_output(model_kind(sh.kind), px.data(), aeon_img_desc{0, w, h, w * c, c, 1, 0}, p, want.data(), sh.item);
}

struct Buffers { // the batch buffers of one container: pageable, or the model's mapped host memory
    std::vector<uint8_t*> p;
    size_t                bytes;
    bool                  mapped;
    Buffers(const Shape& sh, bool mapped_) : bytes(sh.nr * sh.item), mapped(mapped_)
    {
        for (int b = 0; b < sh.nb; b++) {
            void* q = nullptr;
            if (mapped) {
                if (hipHostMalloc(&q, bytes, 0) != hipSuccess) std::abort();
            } else {
                q = std::malloc(bytes);
            }
            std::memset(q, 0xEE, bytes);
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
    StagerHandle(const Shape& sh)
    {
        aeon_out_desc od;
        std::memset(&od, 0, sizeof(od));
        od.dtype = AEON_DTYPE_U8, od.channels = sh.kind == AEON_STAGER_MASK ? 1 : 3, od.item_stride = sh.item;
        OK(aeon_hip_stager_create(ctx(), sh.kind, &od, sh.nr, &s));
    }
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

// provide() for every record of window `win` into `bufs`, from `threads` threads (records dealt round robin).
void stage_window(aeon_hip_stager* s, const Shape& sh, Buffers& bufs, int win, int threads)
{
    std::mutex  mu;
    std::string err;
    auto        work = [&](int t) {
        for (int k = t; k < sh.nb * sh.nr; k += threads) {
            const int            b = k / sh.nr, i = k % sh.nr;
            std::vector<uint8_t> px, want;
            int                  w, h, c;
            aeon_aug_params      p;
            make_record(sh, win, b, i, px, w, h, c, p, want);
            const int rc = aeon_hip_stager_stage(s, bufs.p[b], i, px.data(), w, h, 0, c, 1, &p);
            if (rc != 0) {
                std::lock_guard<std::mutex> l(mu);
                err = "stage -> " + std::to_string(rc) + " " + aeon_hip_stager_last_error();
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

void verify_batch(const Shape& sh, const uint8_t* buf, int win, int b)
{
    for (int i = 0; i < sh.nr; i++) {
        std::vector<uint8_t> px, want;
        int                  w, h, c;
        aeon_aug_params      p;
        make_record(sh, win, b, i, px, w, h, c, p, want);
        CHECK(std::memcmp(buf + i * sh.item, want.data(), sh.item) == 0, "window %d batch %d record %d differs", win, b, i);
    }
}

aeon_stager_launch_info info_of(aeon_hip_stager* s)
{
    aeon_stager_launch_info info;
    OK(aeon_hip_stager_last_launch(s, &info));
    return info;
}

void expect_info(aeon_hip_stager* s, uint64_t launches, int zero_copy, int direct, int chunks, int records)
{
    const aeon_stager_launch_info i = info_of(s);
    CHECK(i.launches == launches && i.src_zero_copy == zero_copy && i.out_direct == direct && i.chunks == chunks &&
              i.records == records,
          "launch info {launches %llu, zero_copy %d, direct %d, chunks %d, records %d}, expected {%llu, %d, %d, %d, %d}",
          (unsigned long long)i.launches, i.src_zero_copy, i.out_direct, i.chunks, i.records,
          (unsigned long long)launches, zero_copy, direct, chunks, records);
}

// ---- scenarios ----
void pageable_flush()
{
    const Shape  sh{2, 4, 256, AEON_STAGER_IMAGE};
    StagerHandle st(sh);
    Buffers      bufs(sh, false);
    expect_info(st.s, 0, 0, 0, 0, 0);
    for (int win = 0; win < 3; win++) {
        stage_window(st.s, sh, bufs, win, 1);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
        expect_info(st.s, win + 1, 0, 0, 1, sh.nb * sh.nr);
        for (int b = 0; b < sh.nb; b++) verify_batch(sh, bufs.p[b], win, b);
    }
    // flushing windows all go through one window object: its chunk and device buffers were made once
    CHECK(model_calls("hipHostMalloc") == 1, "%ld pinned chunks allocated", model_calls("hipHostMalloc"));
    CHECK(model_calls("hipMalloc") == 2, "%ld device allocations (the sources' and the outputs', once)",
          model_calls("hipMalloc"));
    st.destroy();
}

void overlap_wait_null(bool mapped)
{
    const Shape  sh{2, 4, 256, AEON_STAGER_IMAGE};
    const int    nwin = 6;
    StagerHandle st(sh);
    Buffers      c0(sh, mapped), c1(sh, mapped);
    Buffers*     containers[2] = {&c0, &c1};
    std::mutex              mu;
    std::condition_variable cv;
    std::deque<int>                 free_q{0, 1};
    std::deque<std::pair<int, int>> full_q; // (window, container); window -1: the decode stage gave up
    std::string                     consumer_err;
    bool                            stop = false; // the consumer gave up

    std::thread consumer([&] { // batch_iterator_fbm::filler
        try {
            for (int k = 0; k < nwin; k++) {
                std::pair<int, int> item;
                {
                    std::unique_lock<std::mutex> l(mu);
                    cv.wait(l, [&] { return !full_q.empty(); });
                    item = full_q.front();
                    full_q.pop_front();
                }
                if (item.first < 0) return;
                Buffers& bufs = *containers[item.second];
                for (int b = 0; b < sh.nb; b++) {
                    OK(aeon_hip_stager_wait(nullptr, bufs.p[b]));
                    verify_batch(sh, bufs.p[b], item.first, b);
                    std::memset(bufs.p[b], 0xEE, bufs.bytes); // (the batch is taken out of the container)
                }
                {
                    std::lock_guard<std::mutex> l(mu);
                    free_q.push_back(item.second);
                }
                cv.notify_all();
            }
        } catch (const Failure& f) {
            std::lock_guard<std::mutex> l(mu);
            consumer_err = f.what;
            stop         = true; // (the decode stage is not left waiting for a container)
            cv.notify_all();
        }
    });
    std::string decode_err;
    try { // async_manager::run_filler over batch_decoder::filler
        for (int win = 0; win < nwin; win++) {
            int c;
            {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return stop || !free_q.empty(); });
                if (stop) break;
                c = free_q.front();
                free_q.pop_front();
            }
            stage_window(st.s, sh, *containers[c], win, 8);
            for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_launch(st.s, containers[c]->p[b]));
            expect_info(st.s, win + 1, mapped ? 1 : 0, mapped ? 1 : 0, 1, sh.nb * sh.nr);
            {
                std::lock_guard<std::mutex> l(mu);
                full_q.emplace_back(win, c);
            }
            cv.notify_all();
        }
    } catch (const Failure& f) {
        decode_err = f.what;
        {
            std::lock_guard<std::mutex> l(mu);
            full_q.emplace_back(-1, 0);
        }
        cv.notify_all();
    }
    consumer.join();
    if (!decode_err.empty()) throw Failure{"decode stage: " + decode_err};
    if (!consumer_err.empty()) throw Failure{"consumer: " + consumer_err};
    st.destroy();
}

void dropped_window()
{
    const Shape  sh{2, 4, 256, AEON_STAGER_IMAGE};
    StagerHandle st(sh);
    Buffers      w0(sh, false), w1(sh, false), w2(sh, false);
    Buffers*     wins[3] = {&w0, &w1, &w2};
    for (int win = 0; win < 3; win++) { // nobody waits for windows 0 and 1
        stage_window(st.s, sh, *wins[win], win, 1);
        if (win == 2) // staging window 2 completed window 0 and dropped it: its buffers are filled
            for (int b = 0; b < sh.nb; b++) verify_batch(sh, w0.p[b], 0, b);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_launch(st.s, wins[win]->p[b]));
    }
    for (int win = 1; win < 3; win++)
        for (int b = 0; b < sh.nb; b++) {
            OK(aeon_hip_stager_wait(win == 1 ? nullptr : st.s, wins[win]->p[b]));
            verify_batch(sh, wins[win]->p[b], win, b);
        }
    const long syncs = model_calls("hipEventSynchronize"), copies = model_calls("hipMemcpy");
    for (int b = 0; b < sh.nb; b++) { // a late wait for window 0: nothing to wait for
        OK(aeon_hip_stager_wait(st.s, w0.p[b]));
        OK(aeon_hip_stager_wait(nullptr, w0.p[b]));
        verify_batch(sh, w0.p[b], 0, b);
    }
    CHECK(model_calls("hipEventSynchronize") == syncs && model_calls("hipMemcpy") == copies,
          "the late waits made runtime calls");
    st.destroy();
}

void zero_copy_reuse()
{
    const Shape  sh{2, 4, 512, AEON_STAGER_MASK};
    StagerHandle st(sh);
    Buffers      bufs(sh, true);
    for (int win = 0; win < 5; win++) {
        stage_window(st.s, sh, bufs, win, 4);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
        expect_info(st.s, win + 1, 1, 1, 1, sh.nb * sh.nr);
        for (int b = 0; b < sh.nb; b++) verify_batch(sh, bufs.p[b], win, b);
    }
    CHECK(model_calls("hipHostMalloc") == 1 + sh.nb, "%ld pinned allocations (one chunk, the batch buffers)",
          model_calls("hipHostMalloc"));
    CHECK(model_calls("hipMemcpyAsync") == 0 && model_calls("hipMemcpy") == 0 && model_calls("hipMalloc") == 0,
          "a zero-copy window made a copy or a device allocation");
    st.destroy();
}

void two_chunks()
{
    const Shape  big{1, 2, 256, AEON_STAGER_IMAGE};
    StagerHandle st(big);
    Buffers      bufs(big, true);
    const int    W = 3400, H = 3432; // 35 006 400 bytes each: the second record does not fit the first 64 MB chunk
    std::vector<uint8_t> want[2];
    for (int pass = 0; pass < 3; pass++) {
        if (pass == 1) { // a small window between the large ones: chunk 0 alone
            for (int i = 0; i < 2; i++) {
                std::vector<uint8_t> px, w;
                int                  ww, hh, c;
                aeon_aug_params      p;
                make_record(big, 7, 0, i, px, ww, hh, c, p, w);
                OK(aeon_hip_stager_stage(st.s, bufs.p[0], i, px.data(), ww, hh, 0, c, 1, &p));
            }
            OK(aeon_hip_stager_flush(st.s, bufs.p[0]));
            expect_info(st.s, 2, 1, 1, 1, 2);
            verify_batch(big, bufs.p[0], 7, 0);
            continue;
        }
        for (int i = 0; i < 2; i++) {
            std::vector<uint8_t> px((size_t)W * H * 3);
            fill(px.data(), px.size(), 1000 + 10 * pass + i);
            const aeon_aug_params p = params_of(pass, 0, i, W, H);
            want[i].resize(big.item);
            model_record_output(MODEL_KIND_AUGMENT, px.data(), aeon_img_desc{0, W, H, W * 3, 3, 1, 0}, p, want[i].data(),
                                big.item);
            OK(aeon_hip_stager_stage(st.s, bufs.p[0], i, px.data(), W, H, 0, 3, 1, &p));
        }
        OK(aeon_hip_stager_flush(st.s, bufs.p[0]));
        expect_info(st.s, pass + 1, 0, 1, 2, 2);
        for (int i = 0; i < 2; i++)
            CHECK(std::memcmp(bufs.p[0] + i * big.item, want[i].data(), big.item) == 0, "pass %d record %d differs", pass, i);
    }
    st.destroy();
}

void wait_sync_fails()
{
    const Shape  sh{2, 4, 256, AEON_STAGER_IMAGE};
    StagerHandle st(sh);
    Buffers      bufs(sh, false);
    stage_window(st.s, sh, bufs, 0, 1);
    for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_launch(st.s, bufs.p[b]));
    model_fail_call("hipEventSynchronize", 1, hipErrorLaunchFailure);
    const int rc = aeon_hip_stager_wait(st.s, bufs.p[0]);
    CHECK(rc == AEON_HIP_ERUNTIME, "the wait whose event synchronize failed returned %d", rc);
    CHECK(std::strstr(aeon_hip_stager_last_error(), "hipEventSynchronize") != nullptr, "its message: '%s'",
          aeon_hip_stager_last_error());
    OK(aeon_hip_stager_wait(st.s, bufs.p[1])); // the window's last wait: spun on the count the failed one left raised
    verify_batch(sh, bufs.p[1], 0, 1);
    for (int win = 1; win < 4; win++) { // whole new windows on the window object whose count was left raised
        stage_window(st.s, sh, bufs, win, 1);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
        for (int b = 0; b < sh.nb; b++) verify_batch(sh, bufs.p[b], win, b);
    }
    st.destroy();
}

void launch_copy_fails()
{
    const Shape  sh{2, 4, 256, AEON_STAGER_IMAGE};
    StagerHandle st(sh);
    Buffers      bufs(sh, false);
    stage_window(st.s, sh, bufs, 0, 1);
    model_fail_call("hipMemcpyAsync", 1, hipErrorInvalidValue);
    int rc = aeon_hip_stager_launch(st.s, bufs.p[0]);
    CHECK(rc == AEON_HIP_ERUNTIME && std::strstr(aeon_hip_stager_last_error(), "hipMemcpyAsync"), "launch returned %d '%s'",
          rc, aeon_hip_stager_last_error());
    expect_info(st.s, 0, 0, 0, 0, 0); // nothing was launched
    rc = aeon_hip_stager_launch(st.s, bufs.p[1]);
    CHECK(rc == AEON_HIP_EINVAL, "the dropped window's other batch launched: %d", rc);
    for (int b = 0; b < sh.nb; b++) {
        OK(aeon_hip_stager_wait(st.s, bufs.p[b])); // nothing to wait for
        for (size_t k = 0; k < bufs.bytes; k++) CHECK(bufs.p[b][k] == 0xEE, "a dropped window wrote batch %d", b);
    }
    stage_window(st.s, sh, bufs, 1, 1);
    for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
    expect_info(st.s, 1, 0, 0, 1, sh.nb * sh.nr);
    for (int b = 0; b < sh.nb; b++) verify_batch(sh, bufs.p[b], 1, b);
    st.destroy();
}

// ---- the program ----
const char* g_running = "";

void on_alarm(int)
{
    char         line[160];
    const int    n = std::snprintf(line, sizeof(line), "%s\tFAIL time limit: the scenario did not return\n", g_running);
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
        {"pageable_flush", pageable_flush},
        {"overlap_wait_null[pageable]", [] { overlap_wait_null(false); }},
        {"overlap_wait_null[mapped]", [] { overlap_wait_null(true); }},
        {"dropped_window", dropped_window},
        {"zero_copy_reuse", zero_copy_reuse},
        {"two_chunks", two_chunks},
        {"wait_sync_fails", wait_sync_fails},
        {"launch_copy_fails", launch_copy_fails},
    };
    int failed = 0;
    for (const auto& sc : scenarios) {
        bool wanted = argc <= 2;
        for (int k = 2; k < argc; k++) wanted = wanted || sc.first == argv[k];
        if (!wanted) continue;
        g_running = sc.first.c_str();
        model_reset();
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
