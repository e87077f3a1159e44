// stager_encoded_driver.cpp -- the stager's encoded half (aeon_amd/csrc/stager.cpp + stager_encoded.cpp, with the
// library's host decoders and abi_host.cpp as they are) over the decoding model device (model_decode.cpp), as a
// stand-alone program for the sanitizer builds (Makefile targets sanitize_stager_encoded: ASan + UBSan,
// tsan_stager_encoded: ThreadSanitizer; tests/test_stager_encoded.py runs both).  Each scenario prints one line,
// "name\tok" or "name\tFAIL what", and the program exits non-zero when any failed.  argv[1] is the time limit in
// seconds (alarm() ends a scenario that spins).
//   stager_encoded_driver [seconds [scenario ...]]
// The records: the driver makes BGR pixels, writes them as a file of the record's kind with encoders of its own
// (lossless formats: the decode must give the pixels back) and expects the model's "kernel" output of those
// pixels; a JPEG record is a header the library's parser accepts around arbitrary bytes, and decodes to the
// model's pattern for those bytes.  Every slot of every batch buffer is compared, the routes are asked of
// aeon_encoded_info, the counts read from aeon_hip_stager_last_decode, and no scenario may end with an encoded
// file that a host-to-device copy carried as well (model_double_uploads).
#include <hip/hip_runtime_api.h>
#include <signal.h>
#include <unistd.h>
#include <zlib.h>

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

namespace {

char          g_ctx_storage; // the stager only passes its context on to the (model's) batch entries
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

// ---- the record kinds ----
enum Kind { PIXELS, JPEG, PNG_FLAT, PNG_NOISE, PPM_P6, PPM_P3, BMP24, TIFF_RAW, NKINDS };
struct KindInfo {
    const char* name;
    int         format; // AEON_FORMAT_*, -1: staged decoded
    int         device; // the route the kind is made for
};
const KindInfo kKinds[NKINDS] = {{"pixels", -1, 0},
                                 {"jpeg", AEON_FORMAT_JPEG, 1},
                                 {"png_flat", AEON_FORMAT_PNG, 1},
                                 {"png_noise", AEON_FORMAT_PNG, 0},
                                 {"ppm_p6", AEON_FORMAT_PIXMAP, 1},
                                 {"ppm_p3", AEON_FORMAT_PIXMAP, 0},
                                 {"bmp24", AEON_FORMAT_PIXMAP, 1},
                                 {"tiff_raw", AEON_FORMAT_TIFF, 1}};

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
void put32(Bytes& b, uint32_t v, bool big = false)
{
    for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (big ? 24 - 8 * k : 8 * k)));
}
void append(Bytes& b, const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); }

Bytes rgb_of(const Bytes& bgr)
{
    Bytes rgb(bgr);
    for (size_t k = 0; k + 2 < rgb.size(); k += 3) std::swap(rgb[k], rgb[k + 2]);
    return rgb;
}

Bytes write_pnm(const Bytes& bgr, int w, int h, bool ascii)
{
    const Bytes rgb = rgb_of(bgr);
    char        head[64];
    const int   n = std::snprintf(head, sizeof(head), "P%d\n%d %d\n255\n", ascii ? 3 : 6, w, h);
    Bytes       f((const uint8_t*)head, (const uint8_t*)head + n);
    if (!ascii) {
        append(f, rgb.data(), rgb.size());
        return f;
    }
    for (size_t k = 0; k < rgb.size(); k++) {
        char      v[8];
        const int m = std::snprintf(v, sizeof(v), "%d%c", rgb[k], (k + 1) % 12 ? ' ' : '\n');
        append(f, v, (size_t)m);
    }
    return f;
}

Bytes write_bmp24(const Bytes& bgr, int w, int h)
{
    const size_t pitch = ((size_t)w * 3 + 3) & ~(size_t)3;
    Bytes        f{'B', 'M'};
    put32(f, (uint32_t)(54 + pitch * h)), put32(f, 0), put32(f, 54);
    put32(f, 40), put32(f, (uint32_t)w), put32(f, (uint32_t)h), put16(f, 1), put16(f, 24), put32(f, 0);
    put32(f, (uint32_t)(pitch * h)), put32(f, 2835), put32(f, 2835), put32(f, 0), put32(f, 0);
    for (int y = h - 1; y >= 0; y--) { // bottom-up
        append(f, bgr.data() + (size_t)y * w * 3, (size_t)w * 3);
        f.resize(f.size() + (pitch - (size_t)w * 3), 0);
    }
    return f;
}

void png_chunk(Bytes& f, const char* tag, const Bytes& data)
{
    put32(f, (uint32_t)data.size(), true);
    const size_t at = f.size();
    append(f, tag, 4);
    append(f, data.data(), data.size());
    put32(f, (uint32_t)crc32(0, f.data() + at, (uInt)(f.size() - at)), true);
}

Bytes write_png(const Bytes& bgr, int w, int h)
{
    const Bytes rgb = rgb_of(bgr);
    Bytes       lines;
    for (int y = 0; y < h; y++) {
        lines.push_back(0); // filter None
        append(lines, rgb.data() + (size_t)y * w * 3, (size_t)w * 3);
    }
    uLongf zn = compressBound((uLong)lines.size());
    Bytes  z(zn);
    if (compress2(z.data(), &zn, lines.data(), (uLong)lines.size(), 6) != Z_OK) std::abort();
    z.resize(zn);
    Bytes f{0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    Bytes ihdr;
    put32(ihdr, (uint32_t)w, true), put32(ihdr, (uint32_t)h, true);
    for (uint8_t v : {8, 2, 0, 0, 0}) ihdr.push_back(v); // 8-bit RGB, no interlace
    png_chunk(f, "IHDR", ihdr);
    png_chunk(f, "IDAT", z);
    png_chunk(f, "IEND", Bytes());
    return f;
}

Bytes write_tiff_raw(const Bytes& bgr, int w, int h)
{
    const Bytes rgb = rgb_of(bgr);
    Bytes       f{'I', 'I', 42, 0};
    put32(f, (uint32_t)(8 + rgb.size() + (rgb.size() & 1))); // the IFD follows the one strip
    append(f, rgb.data(), rgb.size());
    if (rgb.size() & 1) f.push_back(0);
    const uint32_t ifd = (uint32_t)f.size(), bps_at = ifd + 2 + 9 * 12 + 4;
    put16(f, 9);
    auto tag = [&](unsigned t, unsigned type, uint32_t count, uint32_t value) {
        put16(f, t), put16(f, type), put32(f, count);
        if (type == 3 && count == 1) put16(f, value), put16(f, 0);
        else put32(f, value);
    };
    tag(256, 4, 1, (uint32_t)w), tag(257, 4, 1, (uint32_t)h), tag(258, 3, 3, bps_at), tag(259, 3, 1, 1), tag(262, 3, 1, 2);
    tag(273, 4, 1, 8), tag(277, 3, 1, 3), tag(278, 4, 1, (uint32_t)h), tag(279, 4, 1, (uint32_t)rgb.size());
    put32(f, 0);
    put16(f, 8), put16(f, 8), put16(f, 8);
    return f;
}

// A frame header the library's JPEG parser accepts (SOI, SOF0 of three 1x1-sampled components) around bytes of
// the record's own; the model "decodes" it to a pattern of the whole file's hash.
Bytes write_jpeg(int w, int h, uint64_t seed)
{
    Bytes f{0xFF, 0xD8, 0xFF, 0xC0};
    put16(f, 17, true);
    f.push_back(8), put16(f, (unsigned)h, true), put16(f, (unsigned)w, true), f.push_back(3);
    for (uint8_t id = 1; id <= 3; id++) f.push_back(id), f.push_back(0x11), f.push_back(0);
    const size_t at = f.size();
    f.resize(at + 200 + seed % 97);
    fill(f.data() + at, f.size() - at, seed);
    f.push_back(0xFF), f.push_back(0xD9);
    return f;
}

// ---- records: the size and kind of record (b, i) are the same in every window, its pixels differ ----
struct Shape {
    int    nb, nr; // batches per window, records per batch
    size_t item;   // out.item_stride
    int    only;   // -1: kinds dealt round robin; else every record is of this kind
};

struct Record {
    int             kind, w, h;
    Bytes           px;   // what the decode must give (PIXELS: what is staged)
    Bytes           file; // encoded kinds
    aeon_aug_params p;
    Bytes           want; // the model's output for px
};

int kind_of(const Shape& sh, int b, int i) { return sh.only >= 0 ? sh.only : (b * sh.nr + i + b) % NKINDS; }

Record make_record(const Shape& sh, int win, int b, int i)
{
    Record r;
    r.kind = kind_of(sh, b, i);
    r.w = 9 + 5 * i + 2 * b, r.h = 6 + 3 * ((i + b) % 3);
    const uint64_t seed = ((uint64_t)(win + 1) << 32) ^ (uint64_t)(b * 131 + i + 1);
    r.px.resize((size_t)r.w * r.h * 3);
    if (r.kind == PNG_FLAT) { // bands of one colour: a zlib stream far below an eighth of the scanlines
        for (int y = 0; y < r.h; y++)
            for (int x = 0; x < r.w * 3; x++) r.px[(size_t)y * r.w * 3 + x] = (uint8_t)(seed * 37 + (y / 4) * 50 + x % 3);
    } else {
        fill(r.px.data(), r.px.size(), seed);
    }
    switch (r.kind) {
    case JPEG: r.file = write_jpeg(r.w, r.h, seed); break;
    case PNG_FLAT:
    case PNG_NOISE: r.file = write_png(r.px, r.w, r.h); break;
    case PPM_P6: r.file = write_pnm(r.px, r.w, r.h, false); break;
    case PPM_P3: r.file = write_pnm(r.px, r.w, r.h, true); break;
    case BMP24: r.file = write_bmp24(r.px, r.w, r.h); break;
    case TIFF_RAW: r.file = write_tiff_raw(r.px, r.w, r.h); break;
    default: break;
    }
    const aeon_img_desc d{0, r.w, r.h, r.w * 3, 3, 1, 0};
    if (r.kind == JPEG) model_jpeg_pattern(r.file.data(), r.file.size(), d, r.px.data());
    std::memset(&r.p, 0, sizeof(r.p));
    r.p.crop_x = win, r.p.crop_y = b, r.p.crop_w = r.w - win % 3, r.p.crop_h = r.h - 1;
    r.p.out_w = 7 + i, r.p.out_h = 5 + b, r.p.flip = (win + i) & 1;
    r.want.resize(sh.item);
    model_record_output(MODEL_KIND_AUGMENT, r.px.data(), d, r.p, r.want.data(), sh.item);
    return r;
}

int stage_record(aeon_hip_stager* s, uint8_t* buf, int i, const Record& r)
{
    if (r.kind == PIXELS) return aeon_hip_stager_stage(s, buf, i, r.px.data(), r.w, r.h, 0, 3, 1, &r.p);
    // aeon's datum dies with provide(): the stager must have copied what it needs
    Bytes     gone(r.file);
    const int rc = aeon_hip_stager_stage_encoded(s, buf, i, gone.data(), gone.size(), &r.p);
    std::memset(gone.data(), 0xDD, gone.size());
    return rc;
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
    explicit StagerHandle(const Shape& sh)
    {
        aeon_out_desc od;
        std::memset(&od, 0, sizeof(od));
        od.dtype = AEON_DTYPE_U8, od.channels = 3, od.item_stride = sh.item;
        OK(aeon_hip_stager_create(ctx(), AEON_STAGER_IMAGE, &od, sh.nr, &s));
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

// provide() for every record of window `win` into `bufs`, from `threads` threads (records dealt round robin, so
// encoded and decoded records of one batch are staged concurrently).  skip: a record left out (-1: none).
void stage_window(aeon_hip_stager* s, const Shape& sh, Buffers& bufs, int win, int threads, int skip = -1)
{
    std::mutex  mu;
    std::string err;
    auto        work = [&](int t) {
        for (int k = t; k < sh.nb * sh.nr; k += threads) {
            if (k == skip) continue;
            const Record r  = make_record(sh, win, k / sh.nr, k % sh.nr);
            const int    rc = stage_record(s, bufs.p[k / sh.nr], k % sh.nr, r);
            if (rc != 0) {
                std::lock_guard<std::mutex> l(mu);
                err = std::string("stage ") + kKinds[r.kind].name + " -> " + std::to_string(rc) + " " + aeon_hip_stager_last_error();
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
        const Record r = make_record(sh, win, b, i);
        CHECK(std::memcmp(buf + i * sh.item, r.want.data(), sh.item) == 0, "window %d batch %d record %d (%s) differs", win, b,
              i, kKinds[r.kind].name);
    }
}

// The routes the kinds are made for, asked of the library; and the counts a whole window must report.
void expect_decode(aeon_hip_stager* s, const Shape& sh, uint64_t launches)
{
    aeon_stager_decode_info want;
    std::memset(&want, 0, sizeof(want));
    want.launches = launches;
    for (int b = 0; b < sh.nb; b++)
        for (int i = 0; i < sh.nr; i++) {
            const Record r = make_record(sh, 0, b, i);
            if (r.kind == PIXELS) {
                want.pixels++;
                continue;
            }
            int format = -1, w = 0, h = 0, route = -1;
            CHECK(aeon_encoded_info(r.file.data(), r.file.size(), 0, &format, &w, &h, nullptr, nullptr, &route) == 0,
                  "aeon_encoded_info(%s): %s", kKinds[r.kind].name, aeon_hip_last_error());
            CHECK(format == kKinds[r.kind].format && w == r.w && h == r.h && route == kKinds[r.kind].device,
                  "%s %dx%d: format %d, %dx%d, device_route %d", kKinds[r.kind].name, r.w, r.h, format, w, h, route);
            (route ? want.device : want.host)[format]++;
        }
    aeon_stager_decode_info got;
    OK(aeon_hip_stager_last_decode(s, &got));
    CHECK(std::memcmp(&got, &want, sizeof(got)) == 0,
          "last_decode {launches %llu, device %d %d %d %d, host %d %d %d %d, pixels %d}, expected {%llu, %d %d %d %d, %d %d %d "
          "%d, %d}",
          (unsigned long long)got.launches, got.device[0], got.device[1], got.device[2], got.device[3], got.host[0],
          got.host[1], got.host[2], got.host[3], got.pixels, (unsigned long long)want.launches, want.device[0], want.device[1],
          want.device[2], want.device[3], want.host[0], want.host[1], want.host[2], want.host[3], want.pixels);
}

void expect_launch(aeon_hip_stager* s, uint64_t launches, int zero_copy, int direct, int records)
{
    aeon_stager_launch_info i;
    OK(aeon_hip_stager_last_launch(s, &i));
    CHECK(i.launches == launches && i.src_zero_copy == zero_copy && i.out_direct == direct && i.records == records,
          "launch info {launches %llu, zero_copy %d, direct %d, records %d}, expected {%llu, %d, %d, %d}",
          (unsigned long long)i.launches, i.src_zero_copy, i.out_direct, i.records, (unsigned long long)launches, zero_copy,
          direct, records);
}

void expect_single_upload()
{
    CHECK(model_double_uploads() == 0, "%ld encoded files lay in a range a host-to-device copy carried as well",
          model_double_uploads());
}

// ---- scenarios ----
// Eight threads staging the encoded and decoded records of one window concurrently.
void concurrent_mixed()
{
    const Shape  sh{2, 8, 1024, -1};
    StagerHandle st(sh);
    Buffers      bufs(sh, true);
    stage_window(st.s, sh, bufs, 0, 8);
    for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
    expect_launch(st.s, 1, 0, 1, sh.nb * sh.nr); // (mapped outputs, yet no zero-copy sources: files to decode)
    expect_decode(st.s, sh, 1);
    for (int b = 0; b < sh.nb; b++) verify_batch(sh, bufs.p[b], 0, b);
    // the files went up once, through the decode entries; the copies carried staged pixels only
    CHECK(model_file_bytes() > 0 && model_copied_bytes() > 0, "%ld file bytes, %ld copied bytes", model_file_bytes(),
          model_copied_bytes());
    expect_single_upload();
    st.destroy();
}

// Three windows over two containers: window k+1 staged and launched before window k is waited for.
void three_windows_two_containers()
{
    const Shape  sh{2, 8, 1024, -1};
    StagerHandle st(sh);
    Buffers      c0(sh, false), c1(sh, false);
    Buffers*     cont[2] = {&c0, &c1};
    for (int win = 0; win < 3; win++) {
        stage_window(st.s, sh, *cont[win % 2], win, 4);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_launch(st.s, cont[win % 2]->p[b]));
        expect_launch(st.s, win + 1, 0, 0, sh.nb * sh.nr);
        expect_decode(st.s, sh, win + 1);
        if (win == 0) continue;
        Buffers& prev = *cont[(win - 1) % 2]; // the consumer takes the window before
        for (int b = 0; b < sh.nb; b++) {
            OK(aeon_hip_stager_wait(nullptr, prev.p[b]));
            verify_batch(sh, prev.p[b], win - 1, b);
            std::memset(prev.p[b], 0xEE, prev.bytes);
        }
    }
    for (int b = 0; b < sh.nb; b++) {
        OK(aeon_hip_stager_wait(st.s, c0.p[b]));
        verify_batch(sh, c0.p[b], 2, b);
    }
    expect_single_upload();
    st.destroy();
}

// A window of encoded, device-decoded records only: no pinned chunk is touched, nothing is copied host to device.
void encoded_only()
{
    for (int kind : {(int)JPEG, (int)PPM_P6, (int)TIFF_RAW}) {
        model_reset();
        const Shape  sh{2, 4, 512, kind};
        StagerHandle st(sh);
        Buffers      bufs(sh, true);
        for (int win = 0; win < 2; win++) {
            stage_window(st.s, sh, bufs, win, 4);
            for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
            expect_launch(st.s, win + 1, 0, 1, sh.nb * sh.nr);
            expect_decode(st.s, sh, win + 1);
            for (int b = 0; b < sh.nb; b++) verify_batch(sh, bufs.p[b], win, b);
        }
        CHECK(model_calls("hipMemcpyAsync") == 0 && model_copied_bytes() == 0, "a window of files alone copied %ld bytes",
              model_copied_bytes());
        CHECK(model_calls("hipHostMalloc") == sh.nb, "%ld pinned allocations (the batch buffers alone)",
              model_calls("hipHostMalloc"));
        st.destroy();
    }
}

// A header error in mid-window: the stage's code and message with the idx, the window usable, the idx staged again.
void header_error_restage()
{
    const Shape  sh{2, 8, 1024, -1};
    StagerHandle st(sh);
    Buffers      bufs(sh, false);
    const int    bad_k = 1 * sh.nr + 3; // batch 1, idx 3
    stage_window(st.s, sh, bufs, 0, 4, bad_k);
    const Record r = make_record(sh, 0, 1, 3);
    CHECK(r.kind != PIXELS, "record (1, 3) is staged decoded");
    struct Case {
        Bytes       file;
        int         code;
        const char* text;
    };
    Bytes bad_tiff = make_record(sh, 0, 0, 7).file; // (kind TIFF_RAW)
    CHECK(make_record(sh, 0, 0, 7).kind == TIFF_RAW, "record (0, 7) is no TIFF");
    bad_tiff.resize(12);
    const Case cases[] = {{Bytes{0xFF, 0xD8, 0xFF, 0xC0, 0x00}, AEON_HIP_EINVAL, "JPEG: truncated marker segment, at idx 3"},
                          {Bytes{0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0}, AEON_HIP_EINVAL, ", at idx 3"},
                          {Bytes{'P', '6', '\n', '7'}, AEON_HIP_EINVAL, ", at idx 3"},
                          {bad_tiff, AEON_HIP_EINVAL, ", at idx 3"}};
    for (const Case& c : cases) {
        const int rc = aeon_hip_stager_stage_encoded(st.s, bufs.p[1], 3, c.file.data(), c.file.size(), &r.p);
        CHECK(rc == c.code && std::strstr(aeon_hip_stager_last_error(), c.text), "a broken header returned %d '%s'", rc,
              aeon_hip_stager_last_error());
    }
    OK(stage_record(st.s, bufs.p[1], 3, r));
    const int twice = stage_record(st.s, bufs.p[1], 3, r);
    CHECK(twice == AEON_HIP_EINVAL && std::strstr(aeon_hip_stager_last_error(), "staged twice"), "a second stage returned %d '%s'",
          twice, aeon_hip_stager_last_error());
    for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
    expect_decode(st.s, sh, 1);
    for (int b = 0; b < sh.nb; b++) verify_batch(sh, bufs.p[b], 0, b);
    expect_single_upload();
    st.destroy();
}

// A decode entry fails at launch: the window is dropped whole, nothing is written, the next window is right.
void batch_call_fails()
{
    const Shape  sh{2, 8, 1024, -1};
    StagerHandle st(sh);
    Buffers      bufs(sh, false);
    const char*  entries[] = {"aeon_hip_decode_jpeg_batch", "aeon_hip_decode_png_batch", "aeon_hip_decode_pixmap_batch",
                              "aeon_hip_decode_tiff_batch"};
    uint64_t     launches  = 0;
    for (int k = 0; k < 4; k++) {
        stage_window(st.s, sh, bufs, 2 * k, 4);
        model_fail_call(entries[k], 1, AEON_HIP_ERUNTIME);
        int rc = aeon_hip_stager_launch(st.s, bufs.p[0]);
        CHECK(rc == AEON_HIP_ERUNTIME && std::strstr(aeon_hip_stager_last_error(), entries[k]), "launch returned %d '%s'", rc,
              aeon_hip_stager_last_error());
        rc = aeon_hip_stager_launch(st.s, bufs.p[1]);
        CHECK(rc == AEON_HIP_EINVAL, "the dropped window's other batch launched: %d", rc);
        for (int b = 0; b < sh.nb; b++) {
            OK(aeon_hip_stager_wait(st.s, bufs.p[b])); // nothing to wait for
            for (size_t i = 0; i < bufs.bytes; i++) CHECK(bufs.p[b][i] == 0xEE, "a dropped window wrote batch %d", b);
        }
        expect_launch(st.s, launches, 0, 0, launches ? sh.nb * sh.nr : 0); // (the report of the window before)
        stage_window(st.s, sh, bufs, 2 * k + 1, 4);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_flush(st.s, bufs.p[b]));
        expect_decode(st.s, sh, ++launches);
        for (int b = 0; b < sh.nb; b++) {
            verify_batch(sh, bufs.p[b], 2 * k + 1, b);
            std::memset(bufs.p[b], 0xEE, bufs.bytes);
        }
    }
    expect_single_upload();
    st.destroy();
}

// A third window staged while the first was never waited for: the first is completed and dropped.
void third_window_unwaited()
{
    const Shape  sh{2, 8, 1024, -1};
    StagerHandle st(sh);
    Buffers      w0(sh, false), w1(sh, false), w2(sh, false);
    Buffers*     wins[3] = {&w0, &w1, &w2};
    for (int win = 0; win < 3; win++) {
        stage_window(st.s, sh, *wins[win], win, 4);
        if (win == 2) // staging window 2 completed window 0 and dropped it: its buffers are filled
            for (int b = 0; b < sh.nb; b++) verify_batch(sh, w0.p[b], 0, b);
        for (int b = 0; b < sh.nb; b++) OK(aeon_hip_stager_launch(st.s, wins[win]->p[b]));
        expect_decode(st.s, sh, win + 1);
    }
    for (int win = 1; win < 3; win++)
        for (int b = 0; b < sh.nb; b++) {
            OK(aeon_hip_stager_wait(win == 1 ? nullptr : st.s, wins[win]->p[b]));
            verify_batch(sh, wins[win]->p[b], win, b);
        }
    expect_single_upload();
    st.destroy();
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
        {"concurrent_mixed", concurrent_mixed},
        {"three_windows_two_containers", three_windows_two_containers},
        {"encoded_only", encoded_only},
        {"header_error_restage", header_error_restage},
        {"batch_call_fails", batch_call_fails},
        {"third_window_unwaited", third_window_unwaited},
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
