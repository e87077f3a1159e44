// host_driver.cpp -- the decoder's host layer (aeon_amd/csrc/host.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer and under ThreadSanitizer (aeon's SANITIZER_TYPE builds,
// /root/reference/CMakeLists.txt:80-101), linked against aeon_amd/csrc/sanitize/no_device.cpp instead of the
// HIP runtime.  What runs: loader-config parsing and verify_config (valid and malformed configs),
// provider_factory, the pinned thread_pool (creation, pinning, teardown, first-exception rethrow), the
// window draws on the pool (draw_window: every record on the pool with its slot engine, the lighting
// cache fixed up in order) against the serial draws over odd and even windows, a window that throws
// (an element of size 0) and the windows after it, the node slicing, and cpu lists; and the host half of a
// decode window (batch_decoder::plan: inspect, draw and the arena layout, which needs no device) for images
// (decoded, JPEG, PNG), label + image, image + boundingbox, localization_rcnn + boundingbox and video windows,
// each checked against the arena's rule as the driver restates it; and the refusals of the host-only C entries
// (aeon_amd/csrc/abi_host.cpp, linked as the library links it).
//
// Usage: host_driver [rounds]   One line per case, "name<TAB>ok ..." or "name<TAB>FAIL ..."; exit 1 if
// any case failed (a sanitizer finding aborts the run with its own exit status).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <zlib.h>

#include "../../aeon_amd/csrc/box_job.hpp"
#include "../../aeon_amd/csrc/host.hpp"
#include "../../include/aeon_hip.h"

namespace {

int failures = 0;

void report(const std::string& name, bool ok, const std::string& what)
{
    std::printf("%s\t%s %s\n", name.c_str(), ok ? "ok" : "FAIL", what.c_str());
    if (!ok) failures++;
}

const char* kImage224 =
    R"({"type": "image", "height": 224, "width": 224, "channels": 3, "output_type": "float", "channel_major": true, "bgr_to_rgb": true})";
const char* kC2Aug =
    R"({"type": "image", "scale": [0.5, 1.0], "flip_enable": true, "mean": [0.485, 0.456, 0.406], "stddev": [0.229, 0.224, 0.225]})";
const char* kC3Aug =
    R"({"type": "image", "scale": [0.5, 1.0], "flip_enable": true, "mean": [0.485, 0.456, 0.406], "stddev": [0.229, 0.224, 0.225], "brightness": [0.5, 1.0], "contrast": [0.5, 1.0], "saturation": [0.5, 2.0], "hue": [-18, 18], "lighting": [0.0, 0.1]})";
const char* kMask512 = R"({"type": "pixelmask", "height": 512, "width": 512, "channels": 1, "output_type": "uint8_t"})";
const char* kImage512 =
    R"({"type": "image", "height": 512, "width": 512, "channels": 3, "output_type": "float", "channel_major": true, "bgr_to_rgb": true})";

std::string loader(const std::string& etl, const std::string& aug, const std::string& extra)
{
    return R"({"batch_size": 4, "random_seed": 7, "etl": [)" + etl + R"(], "augmentation": [)" + aug + "]" + extra + "}";
}

struct Records {
    std::vector<uint8_t>          pixel{0};
    std::vector<aeon_record_elem> elems;
    Records(int n, int ne, unsigned seed, int bad = -1)
    {
        for (int i = 0; i < n; i++) {
            seed      = seed * 1103515245u + 12345u;
            const int w = 120 + (int)(seed >> 16) % 500, h = 100 + (int)(seed >> 8) % 500;
            for (int k = 0; k < ne; k++)
                elems.push_back(aeon_record_elem{pixel.data(), i == bad ? 0 : w, h, k == 0 ? 3 : 1, 0});
        }
    }
};

bool same_params(const std::vector<aeon_aug_params>& a, const std::vector<aeon_aug_params>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(aeon_aug_params)) == 0;
}

// draw windows on the pool (decoder a) and serially (decoder b) from the same slot engines
void draw_windows(const std::string& name, const std::string& cfg, int ne, int rounds)
{
    aeon_decoder *a = nullptr, *b = nullptr;
    if (aeon_decoder_create(cfg.c_str(), 0, &a) || aeon_decoder_create(cfg.c_str(), 0, &b)) {
        report(name, false, std::string("create: ") + aeon_decoder_last_error());
        return;
    }
    int  workers = 0;
    bool ok      = aeon_decoder_pool_size(a, &workers) == 0 && workers > 0;
    for (int w = 0; ok && w < workers; w++) {
        int map_cpu = -2, cpus[1024], count = 0;
        ok = aeon_decoder_pool_cpus(a, w, &map_cpu, cpus, 1024, &count) == 0 && count > 0;
    }
    const int windows[] = {5, 130, 33, 64, 1, 257};
    unsigned  seed      = 11;
    for (int r = 0; ok && r < rounds; r++)
        for (int n : windows) {
            Records                      recs(n, ne, seed++);
            std::vector<aeon_aug_params> pa(n), pb(n);
            ok = ok && aeon_decoder_draw_params(a, n, recs.elems.data(), pa.data(), 0) == 0 &&
                 aeon_decoder_draw_params(b, n, recs.elems.data(), pb.data(), 1) == 0 && same_params(pa, pb);
        }
    report(name, ok, "pool " + std::to_string(workers) + " workers, parallel draws == serial draws");
    aeon_decoder_destroy(a);
    aeon_decoder_destroy(b);
}

// a window whose draw throws on the pool leaves the decoder's engines and lighting cache untouched
void failed_window(const std::string& name, const std::string& cfg)
{
    aeon_decoder *a = nullptr, *b = nullptr;
    aeon_decoder_create(cfg.c_str(), 0, &a);
    aeon_decoder_create(cfg.c_str(), 0, &b);
    Records                      bad(40, 1, 3, 17), good(40, 1, 4);
    std::vector<aeon_aug_params> pa(40), pb(40);
    const int                    rc = aeon_decoder_draw_params(a, 40, bad.elems.data(), pa.data(), 0);
    const std::string            msg = aeon_decoder_last_error();
    bool ok = rc == AEON_HIP_ERUNTIME && msg.find("with size 0") != std::string::npos;
    ok      = ok && aeon_decoder_draw_params(a, 40, good.elems.data(), pa.data(), 0) == 0 &&
         aeon_decoder_draw_params(b, 40, good.elems.data(), pb.data(), 0) == 0 && same_params(pa, pb);
    report(name, ok, "rc " + std::to_string(rc) + " (" + msg + ")");
    aeon_decoder_destroy(a);
    aeon_decoder_destroy(b);
}

void invalid_config(const std::string& name, const std::string& cfg, int want)
{
    aeon_decoder* d  = nullptr;
    const int     rc = aeon_decoder_create(cfg.c_str(), 0, &d);
    report(name, rc == want && !d, "rc " + std::to_string(rc) + " (" + aeon_decoder_last_error() + ")");
    if (d) aeon_decoder_destroy(d);
}

// ---- batch_decoder::plan: the host half of a window (inspect, draw, arena layout) without a device ----
// The arena's rule, restated here and not read from the code under test: box tables in provider order, then
// label items, then the staged elements record-major and provider-minor -- `staged` ends here --, then the
// device-decoded slots in the same order, a clip's distinct non-empty frames at its element's position (an
// empty chunk repeats the previous slot); every claim 16-byte aligned; total at least 16.
using namespace aeon_hip;

size_t a16(size_t b) { return (b + 15) & ~(size_t)15; }

struct PlanProvider {
    enum { PIXEL, BOX, LABEL, VIDEO } kind;
    bool rcnn_ext;    // BOX: the table carries the rcnn extension
    int  item_bytes;  // LABEL: bytes of the output type
    int  max_frames;  // VIDEO
};

// one element of a plan case as the driver made it: its bytes and what it knows of them
struct PlanElem {
    std::vector<uint8_t>        bytes;
    int                         w = 0, h = 0, c = 0; // pixels, JPEG, PNG, a clip's frames
    bool                        jpeg = false, png = false;
    int                         boxes = 0;
    std::vector<aeon_avi_frame> frames; // every frame of the file (the driver's own demux)
};

struct Claim {
    size_t offset, bytes;
    int    region; // 0 box table, 1 label items, 2 staged element, 3 device-decoded slot
};

std::vector<uint8_t> be(uint32_t v, int n)
{
    std::vector<uint8_t> b;
    for (int i = n - 1; i >= 0; i--) b.push_back((uint8_t)(v >> (8 * i)));
    return b;
}

PlanElem pixels(int w, int h, int c)
{
    PlanElem e;
    e.bytes.assign((size_t)w * h * c, 5);
    e.w = w, e.h = h, e.c = c;
    return e;
}

// a baseline JPEG's SOI + SOF0 (three components, 4:2:0): all the header inspection reads
PlanElem jpeg_header(int w, int h)
{
    PlanElem e = pixels(0, 0, 0);
    e.bytes    = {0xFF, 0xD8, 0xFF, 0xC0, 0x00, 0x11, 0x08, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w,
                  0x03, 0x01, 0x22, 0x00, 0x02, 0x11, 0x01, 0x03, 0x11, 0x01, 0xFF, 0xD9};
    e.w = w, e.h = h, e.c = 3, e.jpeg = true;
    return e;
}

// a PNG's signature + IHDR (8-bit RGB) with its CRC: all the header inspection reads
PlanElem png_header(int w, int h)
{
    PlanElem e = pixels(0, 0, 0);
    e.bytes    = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    for (uint32_t v : {(uint32_t)w, (uint32_t)h})
        for (uint8_t b : be(v, 4)) e.bytes.push_back(b);
    for (uint8_t b : {8, 2, 0, 0, 0}) e.bytes.push_back(b);
    for (uint8_t b : be((uint32_t)crc32(0L, e.bytes.data() + 12, 17), 4)) e.bytes.push_back(b);
    e.w = w, e.h = h, e.c = 3, e.png = true;
    return e;
}

PlanElem datum(const std::string& text, int boxes = 0)
{
    PlanElem e;
    e.bytes.assign(text.begin(), text.end());
    e.boxes = boxes;
    return e;
}

PlanElem metadata(int boxes)
{
    std::string objs;
    for (int b = 0; b < boxes; b++)
        objs += std::string(b ? ", " : "") + R"({"bndbox": {"xmin": )" + std::to_string(10 + 20 * b) +
                R"(, "ymin": 12, "xmax": )" + std::to_string(25 + 20 * b) + R"(, "ymax": 40}, "name": "b"})";
    return datum(R"({"object": [)" + objs + R"(], "size": {"depth": 3, "height": 120, "width": 160}})", boxes);
}

// the golden clip, demuxed by the driver itself: every frame of the file and the first frame's size
PlanElem clip(const std::string& path)
{
    PlanElem e;
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        uint8_t buf[4096];
        for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;) e.bytes.insert(e.bytes.end(), buf, buf + got);
        std::fclose(f);
    }
    int         count = 0, aw = 0, ah = 0, comps = 0;
    std::string err;
    e.frames.resize(4096);
    if (avi_frames(e.bytes.data(), e.bytes.size(), e.frames.data(), 4096, &count, &aw, &ah, err) != 0) count = 0;
    e.frames.resize(std::min(count, 4096));
    if (count) aeon_jpeg_info(e.bytes.data() + e.frames[0].offset, e.frames[0].size, &e.w, &e.h, &comps);
    e.c = 3;
    return e;
}

// records[i * ne + k] through batch_decoder::plan, against the rule
void plan_case(const std::string& name, const std::string& cfg, const std::vector<PlanProvider>& prov,
               const std::vector<PlanElem>& records)
{
    const int                    ne = (int)prov.size(), n = (int)records.size() / ne;
    std::vector<decoded_element> in(records.size());
    for (size_t j = 0; j < in.size(); j++) {
        const PlanElem& r = records[j];
        in[j].data = r.bytes.data(), in[j].size = r.bytes.size();
        if (prov[j % ne].kind != PlanProvider::PIXEL) continue;
        if (r.jpeg || r.png) in[j].encoded = true;
        else in[j].width = r.w, in[j].height = r.h, in[j].channels = r.c, in[j].stride = r.w * r.c;
    }
    std::string why;
    auto        expect = [&](bool ok, const std::string& what) {
        if (!ok && why.empty()) why = what;
    };
    try {
        batch_decoder dec(Json::parse(cfg), 0);
        window_plan   p = dec.plan(n, in.data());
        // the expected offsets, and the claims the plan made
        std::vector<Claim> claims;
        size_t             off = 0;
        for (int k = 0; k < ne; k++) {
            if (prov[k].kind != PlanProvider::BOX) continue;
            size_t total = 0;
            for (int i = 0; i < n; i++) total += (size_t)records[(size_t)i * ne + k].boxes;
            const box_part& b = dynamic_cast<const box_part&>(*p.w.parts[k]);
            expect(b.offset == off && b.total == total, "box table of provider " + std::to_string(k));
            for (int i = 0; i < n; i++)
                expect((int)b.boxes[i].labels.size() == records[(size_t)i * ne + k].boxes, "boxes of record " + std::to_string(i));
            claims.push_back({b.offset, box_table_bytes(n, total, prov[k].rcnn_ext), 0});
            off += a16(claims.back().bytes);
        }
        for (int k = 0; k < ne; k++) {
            if (prov[k].kind != PlanProvider::LABEL) continue;
            const label_part& l = dynamic_cast<const label_part&>(*p.w.parts[k]);
            expect(l.offset == off, "label items of provider " + std::to_string(k));
            for (int i = 0; i < n; i++)
                expect(l.values[i] == std::stoi(std::string(records[(size_t)i * ne + k].bytes.begin(), records[(size_t)i * ne + k].bytes.end())),
                       "label value");
            claims.push_back({l.offset, (size_t)n * prov[k].item_bytes, 1});
            off += a16(claims.back().bytes);
        }
        auto pixel_desc = [&](int k, int i, const PlanElem& r, int region) {
            const aeon_img_desc& d = p.w.parts[k]->descs[i];
            expect(d.offset == off && d.width == r.w && d.height == r.h && d.channels == r.c && d.stride == r.w * r.c,
                   "descriptor of record " + std::to_string(i) + " provider " + std::to_string(k));
            claims.push_back({(size_t)d.offset, (size_t)d.stride * d.height, region});
            off += a16((size_t)r.w * r.h * r.c);
        };
        for (int i = 0; i < n; i++)
            for (int k = 0; k < ne; k++)
                if (prov[k].kind == PlanProvider::PIXEL && !records[(size_t)i * ne + k].jpeg)
                    pixel_desc(k, i, records[(size_t)i * ne + k], 2);
        expect(p.staged == off, "staged " + std::to_string(p.staged) + ", by the rule " + std::to_string(off));
        std::vector<jpeg_list> jpegs(ne);
        for (int i = 0; i < n; i++)
            for (int k = 0; k < ne; k++) {
                const PlanElem& r = records[(size_t)i * ne + k];
                if (prov[k].kind == PlanProvider::PIXEL && r.jpeg) {
                    jpegs[k].add(r.bytes.data(), r.bytes.size(), p.w.parts[k]->descs[i]);
                    pixel_desc(k, i, r, 3);
                }
                if (prov[k].kind != PlanProvider::VIDEO) continue;
                const video_part& v    = dynamic_cast<const video_part&>(*p.w.parts[k]);
                const int         D    = prov[k].max_frames, kept = std::min((int)r.frames.size(), D);
                expect(v.counts[i] == kept && (int)v.descs.size() == n * D, "clip_counts of record " + std::to_string(i));
                for (int d = 0; d < kept; d++) {
                    const aeon_img_desc& fd = v.descs[(size_t)i * D + d];
                    if (r.frames[d].size == 0) {
                        expect(d > 0 && fd.offset == v.descs[(size_t)i * D + d - 1].offset, "repeated frame " + std::to_string(d));
                        continue;
                    }
                    jpegs[k].add(r.bytes.data() + r.frames[d].offset, r.frames[d].size, fd);
                    pixel_desc(k, i * D + d, r, 3);
                }
            }
        expect(p.total == std::max<size_t>(off, 16), "total " + std::to_string(p.total) + ", by the rule " + std::to_string(off));
        // the JPEG stage's files: exactly the encoded elements and the non-empty kept frames, in record order
        expect((int)p.jpegs.size() == ne, "one JPEG list per provider");
        for (int k = 0; k < ne && why.empty(); k++) {
            const jpeg_list &got = p.jpegs[k], &want = jpegs[k];
            expect(got.files == want.files && got.sizes == want.sizes && got.descs.size() == want.descs.size(),
                   "JPEG files of provider " + std::to_string(k));
            for (size_t f = 0; f < want.descs.size() && why.empty(); f++)
                expect(std::memcmp(&got.descs[f], &want.descs[f], sizeof(aeon_img_desc)) == 0, "JPEG destination " + std::to_string(f));
        }
        // every claim aligned and inside [0, total); none overlaps; the regions in order, `staged` the boundary
        std::sort(claims.begin(), claims.end(), [](const Claim& a, const Claim& b) { return a.offset < b.offset; });
        for (size_t j = 0; j < claims.size(); j++) {
            const Claim& c = claims[j];
            expect(c.offset % 16 == 0 && c.offset + c.bytes <= p.total, "claim " + std::to_string(j) + " aligned, inside the arena");
            expect(c.region == 3 ? c.offset >= p.staged : c.offset + c.bytes <= p.staged, "claim " + std::to_string(j) + " on its side of staged");
            if (j) expect(claims[j - 1].offset + claims[j - 1].bytes <= c.offset && claims[j - 1].region <= c.region,
                          "claim " + std::to_string(j) + " after its predecessor, regions in order");
        }
        report(name, why.empty(), why.empty() ? std::to_string(claims.size()) + " claims, staged " + std::to_string(p.staged) +
                                                    ", total " + std::to_string(p.total) : why);
    } catch (const std::exception& e) {
        report(name, false, std::string("threw: ") + e.what());
    }
}

void plan_cases()
{
    const std::string img = R"({"type": "image", "height": 32, "width": 32, "channels": 3})";
    const std::string bb  = R"({"type": "boundingbox", "height": 32, "width": 32, "max_bbox_count": 4, "class_names": ["a", "b"]})";
    const std::string rcnn = R"({"type": "localization_rcnn", "height": 1000, "width": 1000, "class_names": ["a", "b"], "max_gt_boxes": 64})";
    const std::string rcnn_aug =
        R"({"type": "image", "flip_enable": false, "crop_enable": false, "fixed_aspect_ratio": true, "fixed_scaling_factor": 1.6})";
    const char* aug = R"({"type": "image", "scale": [0.5, 1.0], "flip_enable": true})";
    const PlanProvider pixel{PlanProvider::PIXEL, false, 0, 0}, box{PlanProvider::BOX, false, 0, 0},
        rbox{PlanProvider::BOX, true, 0, 0}, label{PlanProvider::LABEL, false, 4, 0};
    plan_case("plan_image_decoded_jpeg_png", loader(img, aug, ""), {pixel}, {pixels(37, 23, 3), jpeg_header(50, 41), png_header(19, 11)});
    plan_case("plan_label_image", loader(R"({"type": "label"}, )" + img, aug, ""), {label, pixel},
              {datum("7"), pixels(37, 23, 3), datum("-3"), jpeg_header(16, 16), datum("12"), pixels(5, 9, 3)});
    plan_case("plan_image_boxes", loader(img + ", " + bb, aug, ""), {pixel, box},
              {pixels(160, 120, 3), metadata(0), jpeg_header(160, 120), metadata(1), pixels(161, 119, 3), metadata(2)});
    plan_case("plan_rcnn_boxes", loader(rcnn + ", " + bb, rcnn_aug, ""), {rbox, box},
              {metadata(2), metadata(2), metadata(0), metadata(0), metadata(1), metadata(1)});
    // the golden clip lies next to this file's directory: tests/golden/video/bb8.avi
    const std::string here = __FILE__;
    const PlanElem    bb8  = clip(here.substr(0, here.rfind('/')) + "/../golden/video/bb8.avi");
    const int         F    = (int)bb8.frames.size();
    report("plan_video_clip_read", F > 1 && bb8.w > 0, std::to_string(F) + " frames");
    for (int D : {F - 1, F + 3}) {
        const std::string video = R"({"type": "video", "max_frame_count": )" + std::to_string(D) +
                                  R"(, "frame": {"type": "image", "height": 24, "width": 32}})";
        plan_case(D < F ? "plan_video_cut" : "plan_video_short", loader(video, R"({"type": "image"})", ""),
                  {{PlanProvider::VIDEO, false, 0, D}}, {bb8, bb8, bb8});
    }
}

// The host-only entries the layer calls are the library's own (aeon_amd/csrc/abi_host.cpp): calls that only
// the real wrappers refuse -- null pointers, an unknown decode mode, a stride shorter than a row -- each with
// AEON_HIP_EINVAL and a message.
void abi_refusals()
{
    // a valid 2x2 8-bit RGB PNG: IHDR, one IDAT (two rows, filter None), IEND
    std::vector<uint8_t> png = png_header(2, 2).bytes;
    auto                 chunk = [&](const char* type, const std::vector<uint8_t>& body) {
        std::vector<uint8_t> c(type, type + 4);
        c.insert(c.end(), body.begin(), body.end());
        for (uint8_t b : be((uint32_t)body.size(), 4)) png.push_back(b);
        png.insert(png.end(), c.begin(), c.end());
        for (uint8_t b : be((uint32_t)crc32(0L, c.data(), (uInt)c.size()), 4)) png.push_back(b);
    };
    const uint8_t        rows[14] = {0, 10, 20, 30, 40, 50, 60, 0, 70, 80, 90, 100, 110, 120};
    std::vector<uint8_t> z(compressBound(sizeof(rows)));
    uLongf               zn = (uLongf)z.size();
    compress(z.data(), &zn, rows, sizeof(rows));
    z.resize(zn);
    chunk("IDAT", z);
    chunk("IEND", {});
    const std::vector<uint8_t> jpg = jpeg_header(16, 16).bytes;

    std::string why;
    auto        refused = [&](const char* what, const char* text, int rc) { // (text: the wrapper's own message)
        const std::string msg = aeon_hip_last_error();
        if (why.empty() && (rc != AEON_HIP_EINVAL || msg.find(text) == std::string::npos)) why = std::string(what) + ": rc " + std::to_string(rc) + " (" + msg + ")";
    };
    int     w = 0, h = 0, depth = 0, ctype = 0, comps = 0, eb = 0;
    uint8_t dst[2 * 2 * 3 * 2] = {0};
    if (aeon_png_info(png.data(), png.size(), &w, &h, &depth, &ctype) != 0 || w != 2 || h != 2 ||
        aeon_decode_png(png.data(), png.size(), AEON_PNG_BGR8, dst, 6, &eb) != 0 || eb != 1 || dst[0] != 30 || dst[11] != 100)
        why = std::string("the 2x2 PNG does not decode: ") + aeon_hip_last_error();
    if (aeon_jpeg_info(jpg.data(), jpg.size(), &w, &h, &comps) != 0 || w != 16 || h != 16)
        why = std::string("the JPEG header does not parse: ") + aeon_hip_last_error();
    refused("png_info null data", "null argument", aeon_png_info(nullptr, png.size(), &w, &h, &depth, &ctype));
    refused("png_info null out", "null argument", aeon_png_info(png.data(), png.size(), &w, nullptr, &depth, &ctype));
    refused("jpeg_info null data", "null argument", aeon_jpeg_info(nullptr, jpg.size(), &w, &h, &comps));
    refused("jpeg_info null out", "null argument", aeon_jpeg_info(jpg.data(), jpg.size(), &w, &h, nullptr));
    refused("decode_png unknown mode", "unknown PNG decode mode", aeon_decode_png(png.data(), png.size(), AEON_PNG_ANYDEPTH + 1, dst, 6, &eb));
    refused("decode_png stride 1", "stride too small", aeon_decode_png(png.data(), png.size(), AEON_PNG_BGR8, dst, 1, &eb));
    report("abi_refusals", why.empty(), why.empty() ? "6 calls refused with AEON_HIP_EINVAL and a message" : why);
}

} // namespace

int main(int argc, char** argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 2;
    const std::string c2 = loader(kImage224, kC2Aug, ""), c3 = loader(kImage224, kC3Aug, "");
    draw_windows("draw_c2", c2, 1, rounds);
    draw_windows("draw_c3_lighting", c3, 1, rounds);
    draw_windows("draw_c5_image_mask", loader(std::string(kImage512) + ", " + kMask512, kC2Aug, ""), 2, rounds);
    draw_windows("draw_c3_cpu_list", loader(kImage224, kC3Aug, R"(, "cpu_list": "0")"), 1, rounds);
    draw_windows("draw_c3_thread_count", loader(kImage224, kC3Aug, R"(, "decode_thread_count": 5)"), 1, rounds);
    draw_windows("draw_c3_node", loader(kImage224, kC3Aug, R"(, "node_id": 3, "node_count": 8)"), 1, rounds);
    failed_window("failed_window_c3", c3);
    failed_window("failed_window_c2", c2);
    plan_cases();
    abi_refusals();

    // pools started and stopped back to back (thread start-up, pinning and shutdown races)
    bool ok = true;
    for (int i = 0; i < 20 * rounds; i++) {
        aeon_decoder* d = nullptr;
        ok = ok && aeon_decoder_create(c3.c_str(), 0, &d) == 0;
        int w = 0;
        if (d && i % 2) ok = ok && aeon_decoder_pool_size(d, &w) == 0;
        aeon_decoder_destroy(d);
    }
    report("pool_lifecycle", ok, std::to_string(20 * rounds) + " decoders");

    // a decode window needs the device: the stub refuses it and the decoder stays usable
    {
        aeon_decoder* d = nullptr;
        aeon_decoder_create(c2.c_str(), 0, &d);
        Records recs(4, 1, 9);
        std::vector<float> out(4 * 3 * 224 * 224);
        void*              outs[1] = {out.data()};
        const int          rc = aeon_decoder_decode(d, 4, recs.elems.data(), outs, 0, nullptr);
        std::vector<aeon_aug_params> p(4);
        const std::string msg = aeon_decoder_last_error();
        report("decode_without_device",
               rc == AEON_HIP_ERUNTIME && msg.find("no device") != std::string::npos &&
                   aeon_decoder_draw_params(d, 4, recs.elems.data(), p.data(), 0) == 0,
               "rc " + std::to_string(rc) + " (" + msg + ")");
        aeon_decoder_destroy(d);
    }

    // the aeon-side stager: 8 threads stage 4 batches concurrently (pinned chunk bump allocation,
    // per-batch slots); the window's flush fails without a device and drops the window whole; the
    // next window's stages work
    {
        aeon_out_desc o{};
        o.dtype = AEON_DTYPE_F32, o.channels = 3, o.channel_major = 1, o.item_stride = 3 * 224 * 224 * 4;
        aeon_hip_stager* st  = nullptr;
        const int        rc0 = aeon_hip_stager_create(reinterpret_cast<aeon_hip_ctx*>(0x10), AEON_STAGER_IMAGE, &o, 16, &st);
        std::vector<uint8_t>  px(300 * 200 * 3, 7);
        std::vector<std::vector<float>> outs(4, std::vector<float>(16 * 3 * 224 * 224));
        aeon_aug_params p{};
        p.crop_w = 200, p.crop_h = 150, p.out_w = 224, p.out_h = 224, p.contrast = p.brightness = p.saturation = 1.f;
        bool ok = rc0 == 0;
        for (int window = 0; ok && window < 2; window++) {
            std::vector<std::thread> th;
            std::vector<int>         rcs(64, -99);
            for (int t = 0; t < 8; t++)
                th.emplace_back([&, t] {
                    for (int i = t; i < 64; i += 8)
                        rcs[i] = aeon_hip_stager_stage(st, outs[i / 16].data(), i % 16, px.data(), 300, 200, 0, 3, 1, &p);
                });
            for (auto& x : th) x.join();
            for (int r : rcs)
                if (r != 0) ok = false, std::printf("stage rc %d: %s\n", r, aeon_hip_stager_last_error());
            const int rf = aeon_hip_stager_flush(st, outs[0].data()); // no device: the launch fails
            if (rf == 0) ok = false, std::printf("flush without a device succeeded\n");
        }
        report("stager_concurrent_stage", ok, "rc " + std::to_string(rc0) + " (" + aeon_hip_stager_last_error() + ")");
        aeon_hip_stager_destroy(st);
    }

    invalid_config("config_not_json", "{\"batch_size\": 4, ", AEON_HIP_EINVAL);
    invalid_config("config_unknown_key", loader(kImage224, kC2Aug, R"(, "shuffle_manifst": true)"), AEON_HIP_EINVAL);
    invalid_config("config_no_batch", R"({"etl": [{"type": "image", "height": 8, "width": 8}]})", AEON_HIP_EINVAL);
    invalid_config("config_bad_etl", loader(R"({"type": "image", "height": 8, "width": 8, "channels": 2})", kC2Aug, ""),
                   AEON_HIP_EINVAL);
    invalid_config("config_bad_cpu_list", loader(kImage224, kC2Aug, R"(, "cpu_list": "0-100000")"), AEON_HIP_EINVAL);
    invalid_config("config_cpu_list_text", loader(kImage224, kC2Aug, R"(, "cpu_list": "a-b")"), AEON_HIP_EINVAL);
    invalid_config("config_zero_threads", loader(kImage224, kC2Aug, R"(, "decode_thread_count": 0)"), AEON_HIP_EINVAL);
    invalid_config("config_node", loader(kImage224, kC2Aug, R"(, "node_id": 8, "node_count": 8)"), AEON_HIP_ERUNTIME);
    invalid_config("config_deep", std::string(300, '[') + std::string(300, ']'), AEON_HIP_EINVAL);

    {
        int cpus[64], n = 0;
        const bool a = aeon_thread_affinity_map("2,0-1,1", cpus, 64, &n) == 0 && n == 3 && cpus[0] == 0 && cpus[2] == 2;
        const bool b = aeon_thread_affinity_map("0-99999", cpus, 64, &n) == AEON_HIP_EINVAL;
        const bool c = aeon_thread_affinity_map("", cpus, 0, &n) == 0 && n > 0;
        report("cpu_lists", a && b && c, "");
    }
    {
        int64_t idx[4096], cnt = 0;
        bool    ok2 = aeon_manifest_node_slice(4096, 256, 3, 8, idx, &cnt) == 0 && cnt == 512 && idx[0] == 768;
        ok2 = ok2 && aeon_manifest_node_slice(257, 7, 2, 3, nullptr, &cnt) == 0 && cnt == 85;
        ok2 = ok2 && aeon_manifest_node_slice(10, 2, 5, 2, idx, &cnt) == AEON_HIP_EINVAL;
        report("node_slices", ok2, "");
    }
    return failures ? 1 : 0;
}
