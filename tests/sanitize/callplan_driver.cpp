// callplan_driver.cpp -- the image planner (aeon_amd/csrc/plan.cpp) on a CPU, under ASan + UBSan
// (make sanitize_plan; tests/test_plan.py).  Every case plans one call with fixed fake addresses, writes
// its job table into a zero-filled buffer and prints one `case` line: a hash of the table, the sizes the
// device half allocates by, and every launch's shape in launch order -- tests/golden/plan_tables.json holds
// these lines as the planner printed them when it had been moved out of stage.cpp verbatim, before it was
// restructured.  A `rule` line per case reports a layout check written here, independently of the
// planner: sections and scratch regions in bounds, aligned and disjoint, every scratch read produced by an
// earlier launch.  `refuse` lines give each refusal's code and text.  `--time` plans and writes two large
// calls repeatedly and prints the time per call.
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../aeon_amd/csrc/plan.hpp"

using namespace aeon_hip;

namespace {

constexpr uint64_t kSrc = 0x100000000ull, kOut = 0x200000000ull, kMaskSrc = 0x300000000ull, kMaskOut = 0x400000000ull,
                   kScratch = 0x500000000ull;

// the plan's tile groups in launch order: fn(pass name, position in the launch order, writes scratch, group)
enum Order { O_ROT, O_EXP, O_M16, O_GR_SHORT, O_PRE, O_GR_MAIN, O_PRE2, O_PASS1, O_MAIN };
template <typename F>
void each_group(CallPlan& c, F&& fn)
{
    for (int g = 0; g < CallPlan::kGroups; g++) {
        if (g < CallPlan::kPre2) fn("pre", O_PRE, true, c.tiles[g]);
        else if (g < CallPlan::kPass1) fn("pre2", O_PRE2, true, c.tiles[g]);
        else if (g < CallPlan::kMain) fn("pass1", O_PASS1, true, c.tiles[g]);
        else if (g < CallPlan::kWide) fn("main", O_MAIN, false, c.tiles[g]);
        else fn("pre", O_PRE, true, c.tiles[g]); // (the wide resize_short windows: launched with the pre-pass)
    }
}

struct Call {
    std::string                  name;
    std::vector<aeon_img_desc>   d, md;
    std::vector<aeon_aug_params> p;
    aeon_out_desc                o{}, mo{};
    bool                         is_mask = false, pair = false;
    std::vector<uint64_t>        items;
    int32_t                      plane = 0;
    uint64_t                     next  = 0;

    // a w x h x cn source of `eb`-byte elements, laid out behind the records before it
    void add(const aeon_aug_params& q, int w = 64, int h = 48, int cn = 3, int eb = 1)
    {
        aeon_img_desc s{};
        s.offset = next, s.width = w, s.height = h, s.stride = w * cn * eb, s.channels = cn, s.elem_bytes = eb;
        next += ((uint64_t)s.stride * h + 63) & ~(uint64_t)63;
        d.push_back(s), p.push_back(q);
    }
    void add(const Call& c, int i) { add(c.p[i], c.d[i].width, c.d[i].height, c.d[i].channels, c.d[i].elem_bytes); }
};

aeon_aug_params par(int x, int y, int w, int h, int ow = 16, int oh = 12, int interp = AEON_INTERP_LINEAR)
{
    aeon_aug_params q{};
    q.crop_x = x, q.crop_y = y, q.crop_w = w, q.crop_h = h, q.out_w = ow, q.out_h = oh, q.interp = interp;
    q.contrast = q.brightness = q.saturation = 1.0f;
    q.expand_ratio = 1.0f;
    return q;
}
aeon_aug_params expanded(aeon_aug_params q)
{
    q.expand_ratio = 2.0f, q.expand_w = 128, q.expand_h = 96, q.expand_x = 10, q.expand_y = 20;
    return q;
}
aeon_out_desc out(int dtype, int channels = 3, uint64_t stride = 4096)
{
    aeon_out_desc o{};
    o.dtype = dtype, o.channels = channels, o.channel_major = 1, o.item_stride = stride;
    for (int c = 0; c < 3; c++) o.stddev[c] = 1;
    return o;
}
Call call(const char* name, const aeon_out_desc& o, bool is_mask = false)
{
    Call c;
    c.name = name, c.o = o, c.is_mask = is_mask;
    return c;
}

uint64_t fnv(const uint8_t* p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

void plan_call(CallPlan& plan, const Call& c, std::vector<uint8_t>& table)
{
    const OutView ov = out_view(c.o);
    const MaskSet ms{c.md.data(), (const void*)kMaskSrc, c.mo, (void*)kMaskOut};
    const ItemMap im{c.items.data(), c.plane};
    plan.clear();
    plan.add_records((int)c.d.size(), c.d.data(), (const void*)kSrc, c.p.data(), ov.ko, (void*)kOut, c.is_mask,
                     c.pair ? &ms : nullptr, c.items.empty() ? nullptr : &im);
    plan.finalize(ov.ko);
    if (table.size() < plan.ring_need) table.resize(plan.ring_need);
    std::memset(table.data(), 0, plan.table_cap);
    plan.write(table.data(), kScratch, nullptr);
}

// ---- the layout rule ----------------------------------------------------------------------------
struct Span {
    std::string what;
    uint64_t    lo, hi;
    int         order; // (scratch regions) the launch that writes it
};
struct Rule {
    std::string bad;
    void        check(bool ok, const std::string& what)
    {
        if (!ok && bad.size() < 400) bad += (bad.empty() ? "" : "; ") + what;
    }
    void disjoint(std::vector<Span> v, const char* kind)
    {
        std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
        for (size_t i = 1; i < v.size(); i++)
            check(v[i - 1].hi <= v[i].lo, std::string(kind) + " " + v[i - 1].what + " overlaps " + v[i].what);
    }
};

std::string check_layout(CallPlan& c, const uint8_t* t)
{
    Rule              r;
    std::vector<Span> sec, scr;
    const auto        in_scratch = [&](uint64_t p) { return p >= kScratch && p < kScratch + (1ull << 32); };
    const auto section = [&](const std::string& what, size_t off, size_t bytes, size_t align) {
        if (bytes == 0) return;
        r.check(off % align == 0, what + " misaligned");
        r.check(off + bytes <= c.table_cap, what + " outside the table");
        sec.push_back({what, off, off + bytes, 0});
    };
    const auto writes = [&](const std::string& what, uint64_t ptr, uint64_t bytes, int order) {
        const uint64_t off = ptr - kScratch;
        r.check(in_scratch(ptr) && off % 16 == 0 && off + bytes <= c.scratch_bytes, what + " output outside scratch or misaligned");
        scr.push_back({what, off, off + bytes, order});
    };
    struct Read {
        std::string what;
        uint64_t    ptr;
        int         flag, order;
    };
    std::vector<Read> reads;
    section("rot", c.rot_off, c.rot.size() * sizeof(RotJob), 16);
    section("m16", c.m16_off, c.m16.size() * sizeof(Mask16Job), 16);
    section("exp", c.exp_off, c.exp.size() * sizeof(ExpandJob), 16);
    for (size_t i = 0; i < c.rot.size(); i++) {
        RotJob R;
        std::memcpy(&R, t + c.rot_off + i * sizeof R, sizeof R);
        writes("rot", R.out_ptr, (uint64_t)R.ow * R.oh * R.cn, O_ROT);
        reads.push_back({"rot", R.src_ptr, 0, O_ROT});
    }
    for (size_t i = 0; i < c.exp.size(); i++) {
        ExpandJob E;
        std::memcpy(&E, t + c.exp_off + i * sizeof E, sizeof E);
        writes("exp", E.out_ptr, (uint64_t)E.ew * E.eh * E.cn, O_EXP);
        reads.push_back({"exp", E.src_ptr, E.src_scratch, O_EXP});
    }
    for (size_t i = 0; i < c.m16.size(); i++) {
        Mask16Job M;
        std::memcpy(&M, t + c.m16_off + i * sizeof M, sizeof M);
        r.check(!in_scratch(M.out_ptr), "m16 output in scratch");
        reads.push_back({"m16", M.src_ptr, M.src_scratch, O_M16});
    }
    int gi = 0;
    for (GrPlan* g : {&c.gr_short, &c.gr_main}) {
        const std::string what  = gi ? "gr_main" : "gr_short";
        const int         order = gi++ ? O_GR_MAIN : O_GR_SHORT;
        section(what, g->off, g->jobs.size() * sizeof(ResizeJob), 16);
        section(what + ".lz", g->lz_off, g->jobs.empty() ? 0 : g->n_taps * sizeof(LzIn), 8);
        section(what + ".taps", g->taps_off, g->n_taps * sizeof(GrTap), 4);
        r.check(g->n_taps <= g->n_taps_max, what + " more taps than its jobs' axes");
        for (size_t i = 0; i < g->jobs.size(); i++) {
            ResizeJob R;
            std::memcpy(&R, t + g->off + i * sizeof R, sizeof R);
            if (R.final_out) r.check(!in_scratch(R.out_ptr) && !R.out_scratch, what + " final output in scratch");
            else writes(what, R.out_ptr, (uint64_t)R.win_w * R.win_h * R.cn, order);
            reads.push_back({what, R.src_ptr, R.src_scratch, order});
            const GrPlan::Sub* u = nullptr;
            for (const GrPlan::Sub& s : g->subs)
                if ((int)i >= s.first && (int)i < s.first + s.count) u = &s;
            r.check(u && R.tiles_x * u->CW >= R.win_w && R.tiles_x > 0 && (R.tiles / R.tiles_x) * u->TR >= R.win_h &&
                        R.tiles <= u->max_tiles,
                    what + " tiles do not cover the window");
            if (R.method == GR_LANCZOS4) {
                const size_t lo = g->taps_off, hi = g->taps_off + g->n_taps * sizeof(GrTap);
                r.check((size_t)R.coef_x >= lo && (size_t)R.coef_x + R.win_w * sizeof(GrTap) <= hi &&
                            (size_t)R.coef_y >= lo && (size_t)R.coef_y + R.win_h * sizeof(GrTap) <= hi,
                        what + " taps outside the tap region");
            }
        }
    }
    std::vector<int> slots, slot_tiles;
    each_group(c, [&](const char* pass, int order, bool to_scratch, LaunchPlan& P) {
        section(pass, P.blob_off, P.jobs.size() * sizeof(AugJob), 16);
        for (size_t i = 0; i < P.jobs.size(); i++) {
            AugJob J;
            std::memcpy(&J, t + P.blob_off + i * sizeof J, sizeof J);
            if (to_scratch) writes(pass, J.out_ptr, (uint64_t)J.win_w * J.win_h * J.cn, order);
            else r.check(!in_scratch(J.out_ptr), "main output in scratch");
            reads.push_back({pass, J.src_ptr, J.src_scratch, order});
            r.check((int64_t)J.tiles * P.tr >= J.win_h && J.tiles <= P.max_tiles, std::string(pass) + " tiles do not cover the window");
            if (order == O_PASS1) slots.push_back(J.stats_slot), slot_tiles.push_back(J.tiles);
        }
    });
    each_group(c, [&](const char*, int order, bool, LaunchPlan& P) {
        for (size_t i = 0; order == O_MAIN && i < P.jobs.size(); i++) {
            AugJob J;
            std::memcpy(&J, t + P.blob_off + i * sizeof J, sizeof J);
            if (J.stats_slot < 0) continue;
            const auto it = std::find(slots.begin(), slots.end(), J.stats_slot);
            r.check(it != slots.end() && slot_tiles[it - slots.begin()] == J.stats_tiles, "main job's stats slot has no pass-1 job");
        }
    });
    for (size_t i = 0; i < slots.size(); i++)
        r.check(slots[i] >= 0 && slots[i] < (int)slots.size() && std::count(slots.begin(), slots.end(), slots[i]) == 1,
                "stats slots not distinct below the pass-1 count");
    r.check(c.partial_words >= slots.size() * (size_t)c.partial_stride * 4, "partial sums too small");
    for (int tiles : slot_tiles) r.check(tiles * 8 <= c.partial_stride, "partial stride below a pass-1 job's tiles");
    r.check(c.blob <= c.table_cap && c.table_cap <= c.ring_need, "blob / table_cap / ring need out of order");
    for (const Span& s : sec)
        if (s.what.find(".taps") == std::string::npos) r.check(s.hi <= c.blob, s.what + " past the uploaded bytes");
    r.disjoint(sec, "section");
    r.disjoint(scr, "scratch");
    for (const Read& rd : reads) {
        r.check((rd.flag != 0) == in_scratch(rd.ptr), rd.what + " scratch flag disagrees with its source");
        if (!in_scratch(rd.ptr)) continue;
        bool found = false;
        for (const Span& s : scr) found = found || (s.lo == rd.ptr - kScratch && s.order < rd.order);
        r.check(found, rd.what + " reads scratch no earlier launch wrote");
    }
    return r.bad.empty() ? "ok" : "FAIL " + r.bad;
}

void print_case(CallPlan& plan, const Call& c, std::vector<uint8_t>& table)
{
    plan_call(plan, c, table);
    each_group(plan, [&](const char*, int, bool, LaunchPlan& P) { // AugJob's 8 bytes of tail padding: out of the hash
        for (size_t i = 0; i < P.jobs.size(); i++) std::memset(table.data() + P.blob_off + i * sizeof(AugJob) + 248, 0, 8);
    });
    static_assert(sizeof(AugJob) == 256 && __builtin_offsetof(AugJob, stats_tiles) == 244, "AugJob's padding");
    std::printf("case %s hash=%016" PRIx64 " blob=%zu table_cap=%zu ring=%zu scratch=%zu pstride=%d pwords=%zu mask_only=%d",
                c.name.c_str(), fnv(table.data(), plan.blob), plan.blob, plan.table_cap, plan.ring_need, plan.scratch_bytes,
                plan.partial_stride, plan.partial_words, (int)plan.mask_only);
    if (!plan.rot.empty()) std::printf(" | rot n=%zu max_tiles=%d cn=%d", plan.rot.size(), plan.rot_max_tiles, plan.rot_cn);
    if (!plan.exp.empty()) std::printf(" | exp n=%zu max_px=%d", plan.exp.size(), plan.exp_max_px);
    if (!plan.m16.empty())
        std::printf(" | m16 n=%zu max_h=%d max_w=%d max_seg=%d max_slots=%d", plan.m16.size(), plan.m16_max_h, plan.m16_max_w,
                    plan.m16_max_seg, plan.m16_max_slots);
    const auto generic = [&](const char* what, const GrPlan& g) {
        for (const GrPlan::Sub& u : g.subs)
            std::printf(" | %s n=%d sep=%d area=%d TR=%d CW=%d NR=%d SW=%d xs=%d amax=%d cn_max=%d max_tiles=%d any_final=%d", what,
                        u.count, u.sep, (int)u.area, u.TR, u.CW, u.NR, u.SW, u.xs, u.amax, u.cn_max, u.max_tiles, (int)u.any_final);
        if (!g.jobs.empty()) std::printf(" taps=%zu/%zu", g.n_taps, g.n_taps_max);
    };
    int at = O_GR_SHORT;
    each_group(plan, [&](const char* pass, int order, bool, LaunchPlan& P) {
        for (; at <= order; at++) {
            if (at == O_GR_SHORT) generic("gr_short", plan.gr_short);
            if (at == O_GR_MAIN) generic("gr_main", plan.gr_main);
        }
        if (P.jobs.empty()) return;
        std::printf(" | %s rm=%d tail=%d photo=%d n=%zu tr=%d threads=%d lds=%d stage=%d max_win_w=%d max_tiles=%d vec_ok=%d "
                    "rtab=%d hue=%d contrast=%d",
                    pass, P.rm, (int)P.tail, (int)P.photo, P.jobs.size(), P.tr, P.threads, P.lds, P.stage_bytes, P.max_win_w,
                    P.max_tiles, (int)P.vec_ok, (int)P.rtab, (int)P.has_hue, (int)P.has_contrast);
    });
    std::printf("\nrule %s %s\n", c.name.c_str(), check_layout(plan, table.data()).c_str());
}

// ---- the cases -----------------------------------------------------------------------------------
std::vector<Call> cases()
{
    std::vector<Call>   v;
    const aeon_out_desc f32 = out(AEON_DTYPE_F32), u8 = out(AEON_DTYPE_U8);
    const auto photo = [](aeon_aug_params q) { return q.brightness = 1.2f, q.saturation = 0.9f, q.hue = 10, q; };
    const auto light = [](aeon_aug_params q) {
        q.n_lighting = 3, q.lighting[0] = 0.1f, q.lighting[1] = -0.2f, q.lighting[2] = 0.05f, q.color_noise_std = 0.1f;
        return q;
    };
    {   // 1: INTER_LINEAR through the planner: widths 16 and 7 (scalar-tail columns), padding shift, photometric
        Call c = call("linear", f32);
        c.add(par(3, 5, 40, 30));
        c.add(par(0, 0, 64, 48, 7, 12));
        aeon_aug_params q = par(3, 5, 40, 30);
        q.padding = 4, q.pad_off_x = 2, q.pad_off_y = 6, q.flip = 1;
        c.add(q);
        c.add(photo(par(10, 8, 33, 29)));
        c.add(photo(par(1, 2, 50, 40, 7, 12)));
        v.push_back(c);
    }
    {   // 2: the mask gather (8-bit), a 16-bit mask rotated into scratch first, an 8-bit rotated mask (tile path)
        Call c = call("masks", out(AEON_DTYPE_U16, 1, 1024), true);
        c.add(par(3, 5, 40, 30), 64, 48, 1);
        aeon_aug_params q = par(4, 6, 41, 31);
        q.angle = 7, q.flip = 1;
        c.add(q, 64, 48, 1, 2);
        c.add(q, 64, 48, 1);
        c.add(par(0, 0, 64, 48, 16, 5), 64, 48, 1, 2);
        v.push_back(c);
    }
    {   // 3: image rotation: the cropbox window only; with expand the whole record; the same with resize_short
        Call c = call("rotate", f32);
        aeon_aug_params q = par(3, 5, 40, 30);
        q.angle = 7;
        c.add(q);
        q.angle = -90;
        c.add(expanded(q));
        q = expanded(q), q.resize_short_size = 80;
        c.add(q);
        v.push_back(c);
    }
    {   // 4: expand + resize_short as a tile pre-pass (LINEAR) and as a generic resize (CUBIC)
        Call c = call("expand_short", f32);
        aeon_aug_params q = expanded(par(3, 5, 40, 30));
        q.resize_short_size = 80;
        c.add(q);
        q.interp = AEON_INTERP_CUBIC;
        c.add(q);
        q.resize_short_size = 0, q.interp = AEON_INTERP_LINEAR;
        c.add(q);
        v.push_back(c);
    }
    // 5: CUBIC / LANCZOS4 / AREA at non-integer, 3x, 2x scales, an upscale and an identity; f32 (the resize writes
    // the output) and u8 (into scratch, then a copy pass); LANCZOS4 with two records sharing both axes
    const char* mname[] = {"cubic", "area", "lanczos4"};
    for (int m = 0; m < 3; m++)
        for (int k = 0; k < 2; k++) {
            const int interp = AEON_INTERP_CUBIC + m;
            Call      c      = call((std::string(mname[m]) + (k ? "_u8" : "_f32")).c_str(), k ? u8 : f32);
            c.add(par(3, 5, 40, 30, 16, 12, interp));
            c.add(par(8, 6, 48, 36, 16, 12, interp));
            c.add(par(16, 12, 32, 24, 16, 12, interp));
            c.add(par(20, 20, 8, 6, 16, 12, interp));
            c.add(par(7, 9, 16, 12, 16, 12, interp));
            if (interp == AEON_INTERP_LANCZOS4) c.add(par(11, 2, 40, 30, 16, 12, interp));
            v.push_back(c);
        }
    {   // 6: AREA2X + photometric (pre2); contrast alone; contrast + hue + lighting; contrast over a CUBIC resize
        Call c = call("contrast", f32);
        c.add(photo(par(16, 12, 32, 24)));
        aeon_aug_params q = par(3, 5, 40, 30);
        q.contrast = 0.8f;
        c.add(q);
        c.add(light(photo(q)));
        q.interp = AEON_INTERP_CUBIC;
        c.add(q);
        q = photo(par(16, 12, 32, 24)), q.contrast = 1.3f;
        c.add(q);
        v.push_back(c);
    }
    for (int k = 0; k < 2; k++) { // 7: the fixed_aspect_ratio canvas as u8, and as f32 + mean (u8_map)
        aeon_out_desc o = out(k ? AEON_DTYPE_F32 : AEON_DTYPE_U8, 3, 16 * 12 * 3 * 4);
        o.fixed_aspect_ratio = 1, o.canvas_w = 16, o.canvas_h = 12;
        if (k) o.has_mean = 1, o.mean[0] = 0.4, o.mean[1] = 0.5, o.mean[2] = 0.6, o.stddev[0] = 0.2;
        Call c = call(k ? "canvas_f32_mean" : "canvas_u8", o);
        c.add(par(3, 5, 40, 30, 16, 9));
        c.add(par(0, 0, 48, 48, 12, 12));
        c.add(par(3, 5, 40, 30, 16, 9, AEON_INTERP_AREA));
        v.push_back(c);
    }
    {
        Call c = call("gray", out(AEON_DTYPE_F32, 1));
        c.add(par(3, 5, 40, 30), 64, 48, 1);
        c.add(par(0, 0, 64, 48, 7, 12), 64, 48, 1);
        c.add(par(16, 12, 32, 24), 64, 48, 1);
        c.add(par(3, 5, 40, 30, 16, 12, AEON_INTERP_LANCZOS4), 64, 48, 1);
        v.push_back(c);
    }
    {   // 8: the video call's shape: 2 clips x 3 frames, planes D * H * W apart
        const int D = 3, H = 12, W = 16;
        Call      c = call("clips", out(AEON_DTYPE_U8, 3, 3 * D * H * W));
        for (int clip = 0; clip < 2; clip++)
            for (int f = 0; f < D; f++) {
                c.add(par(3 + clip, 5, 40, 30, W, H));
                c.items.push_back(kOut + (uint64_t)clip * c.o.item_stride + (uint64_t)f * H * W);
            }
        c.plane = D * H * W;
        v.push_back(c);
    }
    {   // 9: a pair call: the images and their masks' gather jobs in one plan
        Call c = call("pair", f32);
        for (int i = 0; i < 4; i++) {
            aeon_aug_params q = par(3 + i, 5, 40 - i, 30);
            q.flip = i & 1;
            c.add(q);
            aeon_img_desc m{};
            m.offset = (uint64_t)i * 64 * 48, m.width = 64, m.height = 48, m.stride = 64, m.channels = 1, m.elem_bytes = 1;
            c.md.push_back(m);
        }
        c.mo = out(AEON_DTYPE_U8, 1, 16 * 12), c.pair = true;
        v.push_back(c);
    }
    {   // 10: one call mixing the 3-channel float32 cases above
        Call c = call("mixed", f32);
        for (const Call& s : std::vector<Call>(v))
            for (size_t i = 0; i < s.d.size(); i++)
                if (s.name == "linear" || s.name == "rotate" || s.name == "expand_short" || s.name == "contrast" ||
                    (s.name.find("_f32") != std::string::npos && s.name.find("canvas") == std::string::npos && (i == 0 || i >= 4)))
                    c.add(s, (int)i);
        v.push_back(c);
    }
    return v;
}

// 11: every refusal of validate_record, the gather's checks and the planner
void refusals(CallPlan& plan, std::vector<uint8_t>& table)
{
    struct R {
        const char*     name;
        Call            c;
    };
    const aeon_out_desc f32 = out(AEON_DTYPE_F32), m16 = out(AEON_DTYPE_U16, 1, 1024);
    std::vector<R>      v;
    const auto one = [&](const char* name, const aeon_out_desc& o, bool is_mask, aeon_aug_params q, int w = 64, int h = 48, int cn = 3,
                         int eb = 1) -> Call& {
        Call c = call(name, o, is_mask);
        c.add(q, w, h, cn, eb);
        v.push_back({name, c});
        return v.back().c;
    };
    const aeon_aug_params ok = par(3, 5, 40, 30);
    aeon_aug_params       q;
    aeon_out_desc         o;
    one("channels", f32, false, ok, 64, 48, 2);
    one("channels_config", f32, false, ok, 64, 48, 1);
    one("descriptor", f32, false, ok).d[0].stride = 100;
    q = ok, q.interp = 9;
    one("interpolation", f32, false, q);
    q = ok, q.out_w = 0;
    one("output_size", f32, false, q);
    one("item_stride", out(AEON_DTYPE_F32, 3, 100), false, ok);
    o = f32, o.fixed_aspect_ratio = 1, o.canvas_w = 8, o.canvas_h = 12;
    one("canvas", o, false, ok);
    q = expanded(ok), q.expand_x = 100;
    one("expand", f32, false, q);
    one("cropbox", f32, false, par(30, 5, 40, 30));
    q = ok, q.resize_short_size = 20;
    one("cropbox_short", f32, false, q);
    one("cropbox_expand", f32, false, expanded(par(100, 5, 40, 30)));
    q = ok, q.brightness = 1.5f;
    one("photo_gray", out(AEON_DTYPE_F32, 1), false, q, 64, 48, 1);
    q = ok, q.n_lighting = 2;
    one("lighting", f32, false, q);
    one("m16_image", f32, false, ok, 64, 48, 3, 2);
    one("m16_channels", out(AEON_DTYPE_U16, 3, 4096), true, ok, 64, 48, 3, 2);
    one("m16_descriptor", m16, true, ok, 64, 48, 1, 2).d[0].stride = 129;
    one("gather_descriptor", m16, true, ok, 64, 48, 1, 1).d[0].stride = 10;
    q = ok, q.out_h = -1;
    one("m16_output_size", m16, true, q, 64, 48, 1, 2);
    one("m16_item_stride", out(AEON_DTYPE_U16, 1, 100), true, ok, 64, 48, 1, 2);
    o = m16, o.fixed_aspect_ratio = 1, o.canvas_w = 16, o.canvas_h = 8;
    one("m16_canvas", o, true, ok, 64, 48, 1, 2);
    one("m16_cropbox", m16, true, par(3, 20, 40, 30), 64, 48, 1, 2);
    one("elem_bytes", f32, false, ok, 64, 48, 3, 4);
    one("lds_rows", out(AEON_DTYPE_F32, 3, 1 << 20), false, par(0, 0, 60000, 4, 20000, 4), 60000, 4);
    one("generic_lds", f32, false, par(0, 0, 60001, 3001, 16, 12, AEON_INTERP_AREA), 60001, 3001);
    for (const R& r : v) {
        try {
            plan_call(plan, r.c, table);
            std::printf("refuse %s accepted\n", r.name);
        } catch (const aeon_error& e) {
            std::printf("refuse %s code=%d text=%s\n", r.name, e.code, e.what());
        }
    }
}

// ---- --time ---------------------------------------------------------------------------------------
void time_calls()
{
    uint32_t   seed = 12345;
    const auto rnd  = [&](int lo, int hi) { return seed = seed * 1664525u + 1013904223u, lo + (int)((seed >> 8) % (uint32_t)(hi - lo + 1)); };
    Call lz = call("lanczos4_c2_256", out(AEON_DTYPE_F32, 3, 224 * 224 * 3 * 4));
    for (int i = 0; i < 256; i++) {
        const int w = rnd(120, 256), h = rnd(120, 256);
        aeon_aug_params q = par(rnd(0, 256 - w), rnd(0, 256 - h), w, h, 224, 224, AEON_INTERP_LANCZOS4);
        q.flip = i & 1;
        lz.add(q, 256, 256);
    }
    Call c3 = call("contrast_c3_1024", out(AEON_DTYPE_F32, 3, 224 * 224 * 3 * 4));
    for (int i = 0; i < 1024; i++) {
        const int w = rnd(120, 256), h = rnd(120, 256);
        aeon_aug_params q = par(rnd(0, 256 - w), rnd(0, 256 - h), w, h, 224, 224);
        q.flip = i & 1, q.contrast = 0.8f + 0.001f * (i % 300), q.brightness = 1.1f, q.saturation = 0.9f, q.hue = i % 20 - 10;
        q.n_lighting = 3, q.lighting[0] = 0.1f, q.lighting[1] = -0.1f, q.lighting[2] = 0.05f, q.color_noise_std = 0.1f;
        c3.add(q, 256, 256);
    }
    std::vector<uint8_t> table;
    for (const Call* c : {&lz, &c3}) {
        std::vector<double> us;
        for (int rep = 0; rep < 5; rep++) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int k = 0; k < 200; k++) {
                static CallPlan plan; // (reused from call to call, as the context's)
                plan_call(plan, *c, table);
            }
            us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / 200);
        }
        std::printf("time %s us_per_call", c->name.c_str());
        for (double t : us) std::printf(" %.1f", t);
        std::sort(us.begin(), us.end());
        std::printf(" median %.1f slowest %.1f\n", us[2], us[4]);
    }
}

} // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "--time") return time_calls(), 0;
    CallPlan             plan;
    std::vector<uint8_t> table;
    for (const Call& c : cases()) print_case(plan, c, table);
    refusals(plan, table);
    return 0;
}
