// rcnn_host.cpp -- the host half of the localization_rcnn targets: localization::rcnn::config
// (src/etl_localization_rcnn.hpp:98-146, .cpp:23-78), anchor::generate (.cpp:430-554) and
// transformer::sample_anchors (.cpp:222-261).  Plain host C++ with no HIP dependency, so the sanitizer
// driver (tests/sanitize/rcnn_driver.cpp) links this file alone.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <random>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"
#include "rcnn_host.hpp"
#include "rcnn_job.hpp"

namespace aeon_hip {

namespace {

[[noreturn]] void invalid(const std::string& m) { throw std::invalid_argument(m); }

void fraction(const Json& js, const char* key, float& v)
{
    if (!js.has(key)) return;
    v = (float)js.at(key).number();
    if (!(v >= 0.0 && v <= 1.0)) invalid(std::string("value for '") + key + "' out of range");
}

void count(const Json& js, const char* key, int64_t& v)
{
    if (!js.has(key)) return;
    const double d = js.at(key).number();
    if (!(d >= 0 && d < 2147483648.0)) invalid(std::string("value for '") + key + "' out of range");
    v = (int64_t)d;
}

void floats(const Json& js, const char* key, std::vector<float>& v)
{
    if (!js.has(key)) return;
    v.clear();
    for (const Json& e : js.at(key).array()) v.push_back((float)e.number());
}

// nervana::box of the anchor code: four floats, width / height inclusive, centres through double
struct abox {
    float xmin, ymin, xmax, ymax;
    float width() const { return xmax - xmin + 1; }
    float height() const { return ymax - ymin + 1; }
    float xcenter() const { return xmin + (xmax - xmin) / 2.; }
    float ycenter() const { return ymin + (ymax - ymin) / 2.; }
};

std::vector<abox> mkanchors(const std::vector<float>& ws, const std::vector<float>& hs, float x_ctr, float y_ctr)
{
    std::vector<abox> rc;
    for (size_t i = 0; i < ws.size(); i++)
        rc.push_back(abox{(float)(x_ctr - 0.5 * (ws[i] - 1)), (float)(y_ctr - 0.5 * (hs[i] - 1)),
                          (float)(x_ctr + 0.5 * (ws[i] - 1)), (float)(y_ctr + 0.5 * (hs[i] - 1))});
    return rc;
}

std::vector<abox> ratio_enum(const abox& anchor, const std::vector<float>& ratios)
{
    const int          size = anchor.width() * anchor.height();
    std::vector<float> ws, hs;
    for (float ratio : ratios) ws.push_back(std::round(std::sqrt((float)(size / ratio))));
    for (size_t i = 0; i < ws.size(); i++) hs.push_back(std::round(ws[i] * ratios[i]));
    return mkanchors(ws, hs, anchor.xcenter(), anchor.ycenter());
}

std::vector<abox> scale_enum(const abox& anchor, const std::vector<float>& scales)
{
    std::vector<float> ws, hs;
    for (float scale : scales) {
        ws.push_back(anchor.width() * scale);
        hs.push_back(anchor.height() * scale);
    }
    return mkanchors(ws, hs, anchor.xcenter(), anchor.ycenter());
}

} // namespace

rcnn_config::rcnn_config(const Json& js)
{
    if (js.is_null()) throw std::runtime_error("missing localization_rcnn config in json config");
    for (const char* key : {"height", "width", "class_names"})
        if (!js.has(key)) invalid(std::string("Required Argument: '") + key + "' not set");
    static const std::set<std::string> known{"type", "height", "width", "class_names", "name", "rois_per_image",
                                             "base_size", "scaling_factor", "ratios", "scales", "negative_overlap",
                                             "positive_overlap", "foreground_fraction", "max_gt_boxes"};
    for (const auto& kv : js.object())
        if (!known.count(kv.first)) invalid("config element {" + kv.first + "} is not understood in localization_rcnn");
    count(js, "height", height);
    count(js, "width", width);
    count(js, "rois_per_image", rois_per_image);
    count(js, "base_size", base_size);
    count(js, "max_gt_boxes", max_gt_boxes);
    if (js.has("scaling_factor")) scaling_factor = (float)js.at("scaling_factor").number();
    floats(js, "ratios", ratios);
    floats(js, "scales", scales);
    fraction(js, "negative_overlap", negative_overlap);
    fraction(js, "positive_overlap", positive_overlap);
    fraction(js, "foreground_fraction", foreground_fraction);
    if (js.has("name")) name = js.at("name").str();
    for (const Json& n : js.at("class_names").array()) class_names.push_back(n.str());
    // aeon's validate() is empty; this stage needs sizes it can launch with (rcnn_host.hpp)
    if (height <= 0) invalid("invalid height");
    if (width <= 0) invalid("invalid width");
    if (max_gt_boxes <= 0) invalid("invalid max_gt_boxes");
    if (base_size <= 0) invalid("invalid base_size");
    if (!(scaling_factor > 0) || !std::isfinite(scaling_factor)) invalid("invalid scaling_factor");
    if (ratios.empty() || scales.empty()) invalid("invalid ratios / scales");
    for (float r : ratios)
        if (!(r > 0) || !std::isfinite(r)) invalid("invalid ratios");
    for (float s : scales)
        if (!(s > 0) || !std::isfinite(s)) invalid("invalid scales");
    if (width > (1 << 24) || height > (1 << 24) || max_gt_boxes > (1 << 24))
        throw unsupported_error("localization_rcnn: width, height or max_gt_boxes above 2^24");
    if (!(std::floor(width * scaling_factor) <= (1 << 24)) || !(std::floor(height * scaling_factor) <= (1 << 24)))
        throw unsupported_error("localization_rcnn: feature grid side above 2^24");
    if ((double)ratios.size() * (double)scales.size() * (double)conv_h() * (double)conv_w() > 1099511627776.0)
        throw unsupported_error("localization_rcnn: more than 2^40 anchors");
    if (total_anchors() <= 0) invalid("localization_rcnn config has no anchors");
}

int64_t rcnn_config::conv_w() const { return int(std::floor(width * scaling_factor)); }
int64_t rcnn_config::conv_h() const { return int(std::floor(height * scaling_factor)); }
int64_t rcnn_config::total_anchors() const { return (int64_t)(ratios.size() * scales.size()) * conv_h() * conv_w(); }

std::vector<float> rcnn_generate_anchors(const rcnn_config& cfg)
{
    const int conv_size_x = (int)cfg.conv_w(), conv_size_y = (int)cfg.conv_h();
    // generate_anchors: ratio anchors of the (0, 0, base - 1, base - 1) window, each enumerated over scales
    const abox        base{0.f, 0.f, (float)(cfg.base_size - 1), (float)(cfg.base_size - 1)};
    std::vector<abox> anchors;
    for (const abox& ra : ratio_enum(base, cfg.ratios))
        for (const abox& b : scale_enum(ra, cfg.scales)) anchors.push_back(b);
    // shifts: 1 / scaling_factor is the feature stride (a double quotient, narrowed)
    std::vector<float> shift_x, shift_y;
    for (float i = 0; i < conv_size_x; i++) shift_x.push_back(i * 1. / cfg.scaling_factor);
    for (float i = 0; i < conv_size_y; i++) shift_y.push_back(i * 1. / cfg.scaling_factor);
    std::vector<float> all;
    all.reserve(4 * anchors.size() * shift_x.size() * shift_y.size());
    for (const abox& a : anchors)
        for (float sy : shift_y)
            for (float sx : shift_x) {
                all.push_back(sx + a.xmin);
                all.push_back(sy + a.ymin);
                all.push_back(sx + a.xmax);
                all.push_back(sy + a.ymax);
            }
    return all;
}

std::vector<int32_t> rcnn_sample_anchors(const int32_t* labels, size_t n, int rois_per_image, int num_fg, bool shuffle,
                                         uint32_t* engine_state)
{
    std::vector<int32_t> fg_idx, bg_idx;
    for (size_t i = 0; i < n; i++) {
        if (labels[i] >= 1) fg_idx.push_back((int32_t)i);
        else if (labels[i] == 0) bg_idx.push_back((int32_t)i);
    }
    if (shuffle) {
        tracked_engine random(*engine_state);
        std::shuffle(fg_idx.begin(), fg_idx.end(), random);
        std::shuffle(bg_idx.begin(), bg_idx.end(), random);
        *engine_state = random.last;
    }
    if (num_fg < 0) num_fg = 0;
    if (fg_idx.size() > (size_t)num_fg) fg_idx.resize(num_fg);
    const long remainder = (long)rois_per_image - (long)fg_idx.size();
    if ((long)bg_idx.size() > remainder) bg_idx.resize(remainder > 0 ? remainder : 0);
    fg_idx.insert(fg_idx.end(), bg_idx.begin(), bg_idx.end());
    return fg_idx;
}

} // namespace aeon_hip

namespace {
thread_local std::string g_rcnn_err;

template <typename F>
int rcnn_guarded(F&& f)
{
    try {
        f();
        return AEON_HIP_OK;
    } catch (const std::invalid_argument& e) {
        g_rcnn_err = e.what();
        return AEON_HIP_EINVAL;
    } catch (const aeon_hip::unsupported_error& e) {
        g_rcnn_err = e.what();
        return AEON_HIP_EUNSUPPORTED;
    } catch (const std::exception& e) {
        g_rcnn_err = e.what();
        return AEON_HIP_ERUNTIME;
    }
}
} // namespace

extern "C" {

int aeon_rcnn_anchors(const char* config_json, float* out, int cap, int* n)
{
    using namespace aeon_hip;
    return rcnn_guarded([&] {
        if (!config_json || !n || cap < 0 || (cap > 0 && !out)) throw std::invalid_argument("null argument");
        const rcnn_config cfg(Json::parse(config_json));
        if (cfg.total_anchors() > (1 << 24)) throw unsupported_error("localization_rcnn: more than 2^24 anchors");
        *n = (int)cfg.total_anchors();
        if (cap == 0) return;
        const std::vector<float> a = rcnn_generate_anchors(cfg);
        std::memcpy(out, a.data(), sizeof(float) * 4 * (size_t)std::min<int64_t>(cap, *n));
    });
}

int aeon_rcnn_config_info(const char* config_json, aeon_rcnn_info* info)
{
    using namespace aeon_hip;
    return rcnn_guarded([&] {
        if (!config_json || !info) throw std::invalid_argument("null argument");
        const rcnn_config cfg(Json::parse(config_json));
        info->total_anchors       = cfg.total_anchors();
        info->rois_per_image      = (int32_t)cfg.rois_per_image;
        info->num_fg              = cfg.num_fg();
        info->max_gt_boxes        = (int32_t)cfg.max_gt_boxes;
        info->negative_overlap    = cfg.negative_overlap;
        info->positive_overlap    = cfg.positive_overlap;
        info->width               = (int32_t)cfg.width;
        info->height              = (int32_t)cfg.height;
        info->max_total_anchors   = kRcnnMaxAnchors;
        info->max_rois_per_image  = kRcnnMaxRois;
        info->max_boxes_per_record = kRcnnMaxBoxes;
    });
}

int aeon_rcnn_sample_anchors(const int32_t* labels, int n, int rois_per_image, int num_fg, int shuffle,
                             uint32_t* engine_state, int32_t* out, int* n_out)
{
    using namespace aeon_hip;
    return rcnn_guarded([&] {
        if (n < 0 || (n > 0 && !labels) || !n_out || rois_per_image < 0) throw std::invalid_argument("bad argument");
        if (shuffle && !engine_state) throw std::invalid_argument("null engine state");
        const std::vector<int32_t> v = rcnn_sample_anchors(labels, (size_t)n, rois_per_image, num_fg, shuffle != 0,
                                                           engine_state);
        if (!v.empty() && !out) throw std::invalid_argument("null output");
        if (!v.empty()) std::memcpy(out, v.data(), sizeof(int32_t) * v.size());
        *n_out = (int)v.size();
    });
}

const char* aeon_rcnn_last_error(void) { return g_rcnn_err.c_str(); }

} // extern "C"
