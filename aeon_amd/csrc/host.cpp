// host.cpp -- provider plugin surface + decode stage of the HIP image path (see host.hpp).
#include "host.hpp"
#include "box_job.hpp"
#include "pixmap.hpp"
#include "tiff.hpp"
#include "png.hpp"
#include "rcnn_job.hpp"

#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <set>
#include <sstream>
#include <stdexcept>
#include <unordered_map>

namespace aeon_hip {

namespace {

[[noreturn]] void invalid(const std::string& m) { throw std::invalid_argument(m); }

void hip_check(hipError_t e, const char* what)
{
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

void check(int rc)
{
    if (rc != 0) {
        int code = rc;
        std::string msg = aeon_hip_last_error();
        if (code == AEON_HIP_EINVAL) throw std::invalid_argument(msg);
        throw std::runtime_error(msg);
    }
}

size_t levenshtein(const std::string& a, const std::string& b)
{
    std::vector<size_t> v0(b.size() + 1), v1(b.size() + 1);
    std::iota(v0.begin(), v0.end(), 0);
    for (size_t i = 0; i < a.size(); i++) {
        v1[0] = i + 1;
        for (size_t j = 0; j < b.size(); j++)
            v1[j + 1] = std::min({v1[j] + 1, v0[j + 1] + 1, v0[j] + (a[i] == b[j] ? 0 : 1)});
        std::swap(v0, v1);
    }
    return v0[b.size()];
}

// interface.cpp verify_config: unknown keys are an error, with the closest known key suggested
void verify_config(const std::string& where, const std::set<std::string>& known, const Json& js)
{
    for (const auto& kv : js.object()) {
        if (known.count(kv.first)) continue;
        std::string best;
        size_t      best_d = (size_t)-1;
        for (const auto& k : known) {
            size_t d = levenshtein(kv.first, k);
            if (d < best_d) best_d = d, best = k;
        }
        invalid("config element {" + kv.first + "} is not understood in " + where +
                (best.empty() ? std::string() : ", did you mean {" + best + "}?"));
    }
}

template <typename T>
void get_num(const Json& js, const char* key, T& v)
{
    if (js.has(key)) v = (T)js.at(key).number();
}
void get_bool(const Json& js, const char* key, bool& v)
{
    if (js.has(key)) v = js.at(key).boolean();
}
void get_str(const Json& js, const char* key, std::string& v)
{
    if (js.has(key)) v = js.at(key).str();
}

Json without_type(const Json& j, std::string& type)
{
    if (!j.has("type")) invalid("missing required 'type' element in etl object");
    type = j.at("type").str();
    return j;
}

} // namespace

// ---- typemap -------------------------------------------------------------------------------
output_type::output_type(const std::string& n) : name(n)
{
    // typemap.hpp:43-52 (name -> cv type): the loader's convertTo target
    static const std::map<std::string, std::pair<size_t, int>> all{
        {"int8_t", {1, AEON_DTYPE_S8}},    {"uint8_t", {1, AEON_DTYPE_U8}},  {"int16_t", {2, AEON_DTYPE_S16}},
        {"uint16_t", {2, AEON_DTYPE_U16}}, {"int32_t", {4, AEON_DTYPE_S32}}, {"uint32_t", {4, AEON_DTYPE_S32}},
        {"float", {4, AEON_DTYPE_F32}},    {"double", {8, AEON_DTYPE_F64}},  {"char", {1, AEON_DTYPE_S8}}};
    auto it = all.find(n);
    if (it == all.end()) throw std::runtime_error("Unable to map output type " + n);
    size  = it->second.first;
    dtype = it->second.second;
}

bool output_type::is_valid_type(const std::string& n)
{
    try {
        output_type t(n);
        return true;
    } catch (...) {
        return false;
    }
}

size_t shape_type::byte_size() const
{
    size_t n = otype.size;
    for (size_t d : shape) n *= d;
    return n;
}

// ---- image::config (etl_image.cpp:25-65) ------------------------------------------------------
// half: the config of an "image" element, which also takes "float16" / "bfloat16" (AEON_DTYPE_F16 / BF16:
// the float output rounded once) when it says "extended_output_type": true -- without the key every config is
// valid or invalid exactly as aeon's typemap makes it; every other user of the struct keeps aeon's typemap
// and does not know the key.
image_config::image_config(const Json& js, bool half)
{
    if (js.is_null()) throw std::runtime_error("missing image config in json config");
    if (!js.has("height")) invalid("Required Argument: 'height' not set");
    if (!js.has("width")) invalid("Required Argument: 'width' not set");
    get_num(js, "height", height);
    get_num(js, "width", width);
    get_str(js, "name", name);
    get_bool(js, "bgr_to_rgb", bgr_to_rgb);
    get_bool(js, "channel_major", channel_major);
    get_num(js, "channels", channels);
    if (!(channels == 1 || channels == 3)) invalid("value for 'channels' out of range");
    get_str(js, "output_type", output_type_name);
    bool extended = false;
    if (half) get_bool(js, "extended_output_type", extended);
    const bool half_type = extended && (output_type_name == "float16" || output_type_name == "bfloat16");
    if (!half_type && !output_type::is_valid_type(output_type_name)) invalid("value for 'output_type' out of range");
    if (half)
        verify_config("image", {"type", "height", "width", "name", "bgr_to_rgb", "channel_major", "channels",
                                "output_type", "extended_output_type"},
                      js);
    else
        verify_config("image", {"type", "height", "width", "name", "bgr_to_rgb", "channel_major", "channels",
                                "output_type"},
                      js);
    if (js.at("height").number() <= 0) invalid("invalid height");
    if (js.at("width").number() <= 0) invalid("invalid width");
    if (bgr_to_rgb && channels != 3)
        invalid("invalid config: bgr_to_rgb can be 'true' only for channels set to '3'");
    if (half_type) {
        shape.otype.name  = output_type_name;
        shape.otype.size  = 2;
        shape.otype.dtype = output_type_name == "float16" ? AEON_DTYPE_F16 : AEON_DTYPE_BF16;
    } else {
        shape.otype = output_type(output_type_name);
    }
    if (channel_major) {
        shape.shape = {channels, height, width};
        shape.names = {"channels", "height", "width"};
    } else {
        shape.shape = {height, width, channels};
        shape.names = {"height", "width", "channels"};
    }
}

// ---- providers --------------------------------------------------------------------------------
const shape_type& provider_interface::get_output_shape(const std::string& name) const
{
    for (const auto& p : m_output_shapes)
        if (p.first == name) return p.second;
    throw std::runtime_error("key '" + name + "' not found");
}

const std::vector<std::string>& provider_interface::get_buffer_names()
{
    if (m_buffer_names.empty())
        for (const auto& p : m_output_shapes) m_buffer_names.push_back(p.first);
    return m_buffer_names;
}

namespace {

std::string create_name(const std::string& name, const std::string& base)
{
    return name.empty() ? base : name + "." + base;
}

std::string empty_element(const char* what, int idx)
{
    return std::string("received ") + what + " with size 0, at idx " + std::to_string(idx);
}

// provider::image (provider.cpp:145-184): make_params when the record has none yet, transform_single_image +
// image::loader::load on the GPU at post_process time; and provider::pixelmask (provider.cpp:353-393), which
// shares the record's image params, resamples with nearest neighbour and neither standardizes nor swaps channels.
class pixel_provider : public etl_provider {
public:
    pixel_provider(const Json& js, const Json& aug, bool mask)
        : m_cfg(js, !mask), m_factory(aug), m_mask(mask), m_name(create_name(m_cfg.name, mask ? "pixelmask" : "image"))
    {
        m_out.dtype         = m_cfg.shape.otype.dtype;
        m_out.channels      = (int)m_cfg.channels;
        m_out.channel_major = m_cfg.channel_major;
        m_out.item_stride   = m_cfg.shape.byte_size();
        m_out.fixed_aspect_ratio = m_factory.fixed_aspect_ratio;
        m_out.canvas_w = (int)m_cfg.width, m_out.canvas_h = (int)m_cfg.height;
        if (mask) return;
        // (aeon's fixed_aspect_ratio loader views the item as a uint8 canvas: no meaning for a 16-bit float)
        if (m_out.fixed_aspect_ratio && (m_out.dtype == AEON_DTYPE_F16 || m_out.dtype == AEON_DTYPE_BF16))
            throw unsupported_error("image: 'output_type' " + m_cfg.output_type_name + " with fixed_aspect_ratio");
        // image::loader ctor (etl_image.cpp:204-244)
        const auto& mean = m_factory.mean;
        const auto& std_ = m_factory.stddev;
        if (!mean.empty() || !std_.empty()) {
            if (!(m_cfg.output_type_name == "float" || m_cfg.output_type_name == "double" ||
                  m_cfg.output_type_name == "float16" || m_cfg.output_type_name == "bfloat16"))
                invalid("Standardization (mean, stddev) is supported only for float or double 'output_type'.");
            if (mean.size() != m_cfg.channels || std_.size() != m_cfg.channels)
                invalid("Size of 'mean' and 'stddev' must be equal to number of channels or empty.");
        }
        m_out.bgr_to_rgb = m_cfg.bgr_to_rgb;
        m_out.has_mean   = !mean.empty();
        for (size_t i = 0; i < mean.size() && i < 3; i++) m_out.mean[i] = mean[i], m_out.stddev[i] = std_[i];
    }
    std::vector<std::pair<std::string, shape_type>> output_shapes() const override { return {{m_name, m_cfg.shape}}; }
    const param_factory* factory() const override { return &m_factory; }
    const aeon_out_desc* pixel_out(bool mask) const override { return mask == m_mask ? &m_out : nullptr; }
    void from_abi(const aeon_encoded_elem& in, int idx, decoded_element& e) const override
    {
        if (in.width > 0) {
            e.width = in.width, e.height = in.height, e.channels = in.channels;
            e.stride = in.stride ? in.stride : in.width * in.channels;
        } else {
            if (!in.data || !in.size) throw std::runtime_error(empty_element("encoded image", idx));
            e.encoded = true, e.size = in.size;
        }
    }
    std::unique_ptr<window_part> new_part(int n) const override
    {
        std::unique_ptr<window_part> p(new window_part);
        p->descs.resize(n);
        return p;
    }
    // image::extractor::extract of an encoded element: the file's header gives the decoded size; it is decoded
    // with the provider's channel count (CV_LOAD_IMAGE_COLOR / GRAYSCALE for images, CV_LOAD_IMAGE_ANYDEPTH
    // for pixel masks).  JPEG files are decoded on the device, and so are the PNG files the PNG stage's routing
    // rule gives it (png.hpp); the others (Adam7, very wide rows) on the host pool while staging (png_host.cpp).
    // BMP and binary PNM files are converted on the device (the pixmap stage, pixmap.hpp), ASCII PNM files decoded
    // on the host pool while staging (pixmap_host.cpp).  TIFF files in strips are decoded on the device (the TIFF
    // stage, tiff.hpp), those with LZW / PackBits strips above 32 KiB on the host pool (tiff_host.cpp).  The sniff is strict: anything else is the JPEG parser's.
    void inspect(window_part&, int idx, decoded_element& e) const override
    {
        static const uint8_t kPngSig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
        const int            cn         = m_out.channels;
        if (e.encoded && e.size >= 8 && std::memcmp(e.data, kPngSig, 8) == 0) {
            int depth = 0, ctype = 0;
            check(aeon_png_info(e.data, e.size, &e.width, &e.height, &depth, &ctype));
            e.encoded    = false;
            e.png_device = png_routed(e.data, e.size);
            e.png_mode   = m_mask ? AEON_PNG_ANYDEPTH : (cn == 3 ? AEON_PNG_BGR8 : AEON_PNG_GRAY8);
            e.channels   = m_mask ? 1 : cn;
            e.elem_bytes = (m_mask && depth == 16 && ctype != 3) ? 2 : 1;
            e.stride     = e.width * e.channels * e.elem_bytes;
        } else if (e.encoded && pixmap_sniff(e.data, e.size)) {
            int depth = 0, fcn = 0, format = 0;
            check(aeon_pixmap_info(e.data, e.size, &e.width, &e.height, &depth, &fcn, &format));
            e.encoded       = false;
            e.pixmap_mode   = m_mask ? AEON_DECODE_ANYDEPTH : (cn == 3 ? AEON_DECODE_BGR8 : AEON_DECODE_GRAY8);
            e.pixmap_device = pixmap_routed(e.data, e.size);
            e.channels      = m_mask ? 1 : cn;
            e.elem_bytes    = (m_mask && depth == 16) ? 2 : 1;
            e.stride        = e.width * e.channels * e.elem_bytes;
        } else if (e.encoded && tiff_sniff(e.data, e.size)) {
            int fcn = 0, eb = 1;
            check(aeon_tiff_info(e.data, e.size, &e.width, &e.height, &fcn, &eb));
            e.encoded     = false;
            e.tiff_mode   = m_mask ? AEON_DECODE_ANYDEPTH : (cn == 3 ? AEON_DECODE_BGR8 : AEON_DECODE_GRAY8);
            e.tiff_device = tiff_routed(e.data, e.size);
            e.channels    = m_mask ? 1 : cn;
            e.elem_bytes  = m_mask ? eb : 1;
            e.stride      = e.width * e.channels * e.elem_bytes;
        } else if (e.encoded) {
            if (m_mask)
                throw std::runtime_error("encoded pixel masks are decoded from PNG files only (JPEG masks: pass the "
                                         "decoded mask)");
            int comps = 0;
            check(aeon_jpeg_info(e.data, e.size, &e.width, &e.height, &comps));
            e.channels = cn;
            e.stride   = e.width * e.channels;
        }
        if (!e.data || e.width <= 0 || e.height <= 0)
            throw std::runtime_error(empty_element(m_mask ? "pixelmask" : "encoded image", idx));
    }
    void layout_record(window_part& part, arena_region r, int idx, const decoded_element& e, size_t& offset,
                       jpeg_list& jpegs) const override
    {
        if (r != (e.on_device() ? arena_region::device_decoded : arena_region::staged)) return;
        const size_t b = (size_t)std::max(e.width, 0) * std::max(e.height, 0) * std::max(e.channels, 0) * e.elem_bytes;
        part.descs[idx] = aeon_img_desc{offset, e.width, e.height, e.width * e.channels * e.elem_bytes, e.channels,
                                        e.elem_bytes == 2 ? 2 : 0, 0};
        if (e.encoded) jpegs.add(e.data, e.size, part.descs[idx]);
        if (e.png_device) jpegs.png.add(e.data, e.size, e.png_mode, part.descs[idx]);
        if (e.pixmap_device) jpegs.pixmap.add(e.data, e.size, e.pixmap_mode, part.descs[idx]);
        if (e.tiff_device) jpegs.tiff.add(e.data, e.size, e.tiff_mode, part.descs[idx]);
        offset += arena_align(b);
    }
    void stage_record(const decode_window& w, size_t k, int idx, const decoded_element& e) const override
    {
        if (e.on_device()) return; // decoded on the device, straight into the source arena
        const size_t row = (size_t)e.width * e.channels * e.elem_bytes;
        uint8_t*     dst = w.arena + w.parts[k]->descs[idx].offset;
        if (e.png_mode >= 0) { // extract on this pool thread, straight into the pinned arena
            check(aeon_decode_png(e.data, e.size, e.png_mode, dst, row, nullptr));
        } else if (e.pixmap_mode >= 0) {
            check(aeon_decode_pixmap(e.data, e.size, e.pixmap_mode, dst, row, nullptr));
        } else if (e.tiff_mode >= 0) {
            check(aeon_decode_tiff(e.data, e.size, e.tiff_mode, dst, row, nullptr));
        } else if ((size_t)e.stride == row) {
            std::memcpy(dst, e.data, row * e.height);
        } else {
            for (int y = 0; y < e.height; y++) std::memcpy(dst + y * row, e.data + (size_t)y * e.stride, row);
        }
    }
    void launch(aeon_hip_ctx* ctx, const decode_window& w, size_t k, const uint8_t* dev_arena, void* const* out,
                void* stream) const override
    {
        const auto batch = m_mask ? aeon_hip_mask_batch : aeon_hip_augment_batch;
        check(batch(ctx, w.n, w.parts[k]->descs.data(), dev_arena, w.params[k].data(), &m_out, out[0], stream));
    }

protected:
    bool draw_over(const window_part&, int, const decoded_element& e, draw_source& s) const override
    {
        s = draw_source{e.width, e.height, (int)m_cfg.width, (int)m_cfg.height};
        return true;
    }

private:
    image_config  m_cfg;
    param_factory m_factory;
    bool          m_mask;
    std::string   m_name;
    aeon_out_desc m_out{};
};

// boundingbox::config (etl_boundingbox.cpp:27-49, etl_boundingbox.hpp) and localization::ssd::config
// (etl_localization_ssd.cpp:30-78, etl_localization_ssd.hpp) in one struct: the sizes, the class names
// and the output shapes, in aeon's order.
struct box_config {
    int                                  kind = AEON_BOX_BOUNDINGBOX;
    int64_t                              height = 0, width = 0, max_boxes = 64;
    std::vector<std::string>             class_names;
    std::string                          name, output_type_name = "float";
    std::vector<shape_type>              shapes;

    box_config(const Json& js, int kind_) : kind(kind_)
    {
        const bool ssd = kind == AEON_BOX_SSD;
        if (js.is_null()) throw std::runtime_error(ssd ? "missing ssd config in json config" : "missing bbox config in json config");
        const char* max_key = ssd ? "max_gt_boxes" : "max_bbox_count";
        for (const char* key : {"height", "width", "class_names"})
            if (!js.has(key)) invalid(std::string("Required Argument: '") + key + "' not set");
        if (!ssd && !js.has(max_key)) invalid(std::string("Required Argument: '") + max_key + "' not set");
        get_num(js, "height", height);
        get_num(js, "width", width);
        get_num(js, max_key, max_boxes);
        get_str(js, "name", name);
        for (const Json& n : js.at("class_names").array()) class_names.push_back(n.str());
        if (ssd) {
            verify_config("localization_ssd", {"type", "height", "width", "class_names", "name", "max_gt_boxes"}, js);
            // localization::ssd::config::validate
            if (width <= 0) invalid("invalid width");
            if (height <= 0) invalid("invalid height");
            if (max_boxes <= 0) invalid("invalid max_gt_boxes");
            if (class_names.empty()) invalid("class_names cannot be empty");
        } else {
            get_str(js, "output_type", output_type_name);
            if (!output_type::is_valid_type(output_type_name)) invalid("value for 'output_type' out of range");
            verify_config("bbox", {"type", "height", "width", "class_names", "name", "max_bbox_count", "output_type"}, js);
            // aeon's boundingbox::config::validate is empty; this stage needs sizes it can launch with
            if (width <= 0) invalid("invalid width");
            if (height <= 0) invalid("invalid height");
            if (max_boxes <= 0) invalid("invalid max_bbox_count");
        }
        if (max_boxes > (1 << 24) || width > (1 << 30) || height > (1 << 30)) invalid("box config out of range");
        auto add = [&](std::vector<size_t> s, const char* t) {
            shape_type st;
            st.shape = std::move(s);
            st.otype = output_type(t);
            shapes.push_back(st);
        };
        const size_t m = (size_t)max_boxes;
        if (ssd) {
            add({2, 1}, "int32_t");
            add({m, 4}, "float");
            add({1, 1}, "int32_t");
            add({m, 1}, "int32_t");
            add({m, 1}, "int32_t");
        } else {
            // aeon's quirk (etl_boundingbox.cpp:41): {max_bbox_count, 4 * sizeof(float)} elements of
            // output_type, of which the loader writes the first max_bbox_count * 4 floats
            add({m, 4 * sizeof(float)}, output_type_name.c_str());
        }
    }
};

// What the box providers share: their element is the record's JSON metadata (inspect extracts it), the draw is
// make_params over the metadata's image size unless a provider draws otherwise, and the transform + load run in
// the window's targets launch over the provider's box table, staged in the arena with the pixels.
class box_provider_base : public etl_provider {
public:
    std::vector<std::pair<std::string, shape_type>> output_shapes() const override { return m_shapes; }
    const param_factory* factory() const override { return &m_factory; }
    void from_abi(const aeon_encoded_elem& in, int, decoded_element& e) const override { e.size = in.size; }
    std::unique_ptr<window_part> new_part(int n) const override
    {
        std::unique_ptr<box_part> p(new box_part);
        p->boxes.resize(n);
        return p;
    }
    void inspect(window_part& part, int idx, decoded_element& e) const override
    {
        if (!e.data || e.size == 0) throw std::runtime_error(empty_element(m_what, idx));
        box_extract(m_label_map, e.data, e.size, static_cast<box_part&>(part).boxes[idx]);
    }
    void layout_window(window_part& part, arena_region r, int n, size_t& offset) const override
    {
        if (r != arena_region::box_tables) return;
        box_part& b = static_cast<box_part&>(part);
        b.total     = 0;
        for (const box_metadata& m : b.boxes) b.total += m.labels.size();
        if (b.total > ((size_t)1 << 26)) invalid("box table too large");
        b.offset = offset;
        offset += arena_align(box_table_bytes(n, b.total, m_ext));
    }
    // the table, and the host-side refusals (rotation, boundingbox::box::expand's precondition)
    void stage_window(const decode_window& w, size_t k) const override
    {
        const box_part&    b = static_cast<const box_part&>(*w.parts[k]);
        const BoxTableHost t(w.arena + b.offset, w.n, b.total, m_ext);
        size_t             first = 0;
        for (int i = 0; i < w.n; i++) {
            stage_box_record(t, i, first, b, w.params[k][i]);
            first += b.boxes[i].labels.size();
        }
    }

protected:
    box_provider_base(const Json& aug, size_t width, size_t height, const std::vector<std::string>& class_names, bool ext,
                      const char* what)
        : m_factory(aug), m_width((int)width), m_height((int)height), m_label_map(box_label_map(class_names)), m_ext(ext),
          m_what(what)
    {
    }
    void add_output(const std::string& name, const char* base, std::vector<size_t> shape, const std::string& type)
    {
        shape_type st;
        st.shape = std::move(shape);
        st.otype = output_type(type);
        m_shapes.emplace_back(create_name(name, base), st);
    }
    bool draw_over(const window_part& part, int idx, const decoded_element&, draw_source& s) const override
    {
        const box_metadata& m = static_cast<const box_part&>(part).boxes[idx];
        s = draw_source{m.width, m.height, m_width, m_height};
        return true;
    }
    // record i of the window, whose boxes start at `first` of the table's: refused, or written into t
    virtual void stage_box_record(const BoxTableHost& t, int i, size_t first, const box_part& b, const aeon_aug_params& p) const
    {
        const box_metadata& m   = b.boxes[i];
        const int           cnt = (int)m.labels.size();
        if (const char* why = box_refusal(p, m.boxes.data(), cnt)) invalid(std::string(why) + ", at idx " + std::to_string(i));
        t.recs[i] = box_rec((uint32_t)first, cnt, p);
        if (cnt) {
            std::memcpy(t.boxes + 4 * first, m.boxes.data(), sizeof(float) * 4 * (size_t)cnt);
            std::memcpy(t.labels + first, m.labels.data(), sizeof(int32_t) * (size_t)cnt);
            std::memcpy(t.difficult + first, m.difficult.data(), sizeof(int32_t) * (size_t)cnt);
        }
    }
    param_factory                                   m_factory;
    int                                             m_width, m_height; // the config's: what the params are drawn for
    std::unordered_map<std::string, int>            m_label_map;
    bool                                            m_ext;  // the table carries the rcnn extension
    const char*                                     m_what; // the element, as the empty-element refusal names it
    std::vector<std::pair<std::string, shape_type>> m_shapes;
};

// provider::boundingbox (provider.cpp:395-439) and provider::localization::ssd (provider.cpp:289-346);
// localization_ssd draws make_ssd_params over the extracted boxes.
class box_provider : public box_provider_base {
public:
    box_provider(const Json& js, const Json& aug, int kind) : box_provider(box_config(js, kind), aug) {}
    void launch(aeon_hip_ctx* ctx, const decode_window& w, size_t k, const uint8_t* dev_arena, void* const* out,
                void* stream) const override
    {
        const box_part& b = static_cast<const box_part&>(*w.parts[k]);
        aeon_box_out    o{};
        o.kind      = m_cfg.kind;
        o.max_boxes = (int)m_cfg.max_boxes;
        o.out_w = m_width, o.out_h = m_height;
        o.emit_type = m_factory.emit_type(), o.emit_min_overlap = m_factory.emit_constraint_min_overlap;
        for (size_t i = 0; i < m_shapes.size(); i++) o.item_stride[i] = m_shapes[i].second.byte_size(), o.buf[i] = out[i];
        check(box_targets_staged(ctx, w.n, dev_arena + b.offset, b.total, o, stream));
    }

protected:
    bool draw_over(const window_part& part, int idx, const decoded_element& e, draw_source& s) const override
    {
        box_provider_base::draw_over(part, idx, e, s);
        if (m_cfg.kind != AEON_BOX_SSD) return true;
        const box_metadata& m = static_cast<const box_part&>(part).boxes[idx];
        s.boxes = m.boxes.data(), s.nboxes = (int)m.labels.size();
        return true;
    }

private:
    box_provider(box_config cfg, const Json& aug)
        : box_provider_base(aug, cfg.width, cfg.height, cfg.class_names, false,
                            cfg.kind == AEON_BOX_SSD ? "localization_ssd data" : "boundingbox"),
          m_cfg(std::move(cfg))
    {
        static const char* const ssd_names[5] = {"image_shape", "gt_boxes", "gt_box_count", "gt_class_count",
                                                 "difficult_flag"};
        if (m_cfg.kind == AEON_BOX_SSD)
            for (size_t i = 0; i < 5; i++) m_shapes.emplace_back(create_name(m_cfg.name, ssd_names[i]), m_cfg.shapes[i]);
        else
            m_shapes.emplace_back(create_name(m_cfg.name, "boundingbox"), m_cfg.shapes[0]);
    }
    box_config m_cfg;
};

// provider::localization::rcnn (provider.cpp:222-287): make_params over the record's image size; transform,
// sample_anchors and load run in the window's targets launch.  aeon reads the input size from a member of
// its decoded type that nothing sets (etl_localization_rcnn.hpp:159); here it is the metadata's size, as
// for boundingbox.
class rcnn_provider : public box_provider_base {
public:
    rcnn_provider(const Json& js, const Json& aug) : rcnn_provider(rcnn_config(js), aug) {}
    void take_engines(window_part& part, std::vector<uint32_t>&& words, engine_states* end) const override
    {
        box_part& b = static_cast<box_part&>(part);
        b.engines = std::move(words), b.end = end;
    }
    void stage_box_record(const BoxTableHost& t, int i, size_t first, const box_part& b, const aeon_aug_params& p) const override
    {
        if (b.boxes[i].labels.size() > (size_t)kRcnnMaxBoxes)
            throw unsupported_error("localization_rcnn: more than 1024 boxes in a record, at idx " + std::to_string(i));
        t.ext[i] = rcnn_rec(p, m_factory.fixed_scaling_factor, m_width, m_height, b.engines[i]);
        box_provider_base::stage_box_record(t, i, first, b, p);
    }
    void launch(aeon_hip_ctx* ctx, const decode_window& w, size_t k, const uint8_t* dev_arena, void* const* out,
                void* stream) const override
    {
        const box_part& b = static_cast<const box_part&>(*w.parts[k]);
        aeon_rcnn_out   o{};
        o.total_anchors  = (int32_t)m_cfg.total_anchors();
        o.max_gt_boxes   = (int32_t)m_cfg.max_gt_boxes;
        o.rois_per_image = (int32_t)m_cfg.rois_per_image;
        o.num_fg         = m_cfg.num_fg();
        o.width = m_width, o.height = m_height;
        o.emit_type = m_factory.emit_type(), o.emit_min_overlap = m_factory.emit_constraint_min_overlap;
        o.negative_overlap = m_cfg.negative_overlap, o.positive_overlap = m_cfg.positive_overlap;
        o.fixed_scaling_factor = m_factory.fixed_scaling_factor;
        o.anchors              = m_anchors.data();
        o.anchors_key          = m_anchors_key;
        for (size_t i = 0; i < m_shapes.size(); i++) o.item_stride[i] = m_shapes[i].second.byte_size(), o.buf[i] = out[i];
        engine_states* end = b.end && b.end->dev ? b.end : nullptr;
        check(rcnn_targets_staged(ctx, w.n, dev_arena + b.offset, b.total, o, 1, end ? end->dev : nullptr, stream));
        if (end) { // the engines' end states, right behind the kernel
            hip_check(hipMemcpyAsync(end->host, end->dev, (size_t)w.n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                     (hipStream_t)stream),
                      "hipMemcpyAsync");
            hip_check(hipEventRecord(end->done, (hipStream_t)stream), "hipEventRecord");
            end->queued = true;
        }
    }

private:
    rcnn_provider(rcnn_config cfg, const Json& aug)
        : box_provider_base(aug, cfg.width, cfg.height, cfg.class_names, true, "localization_rcnn data"), m_cfg(std::move(cfg))
    {
        if (m_cfg.total_anchors() > kRcnnMaxAnchors)
            throw unsupported_error("localization_rcnn: total_anchors " + std::to_string(m_cfg.total_anchors()) +
                                    " above this build's 65536");
        if (m_cfg.rois_per_image > kRcnnMaxRois)
            throw unsupported_error("localization_rcnn: rois_per_image above this build's 1024");
        m_anchors = rcnn_generate_anchors(m_cfg);
        static std::atomic<uint64_t> next_key{1}; // one key per table of this process
        m_anchors_key = next_key.fetch_add(1);
        const size_t A = (size_t)m_cfg.total_anchors(), m = (size_t)m_cfg.max_gt_boxes;
        add_output(m_cfg.name, "bbtargets", {A * 4}, "float");
        add_output(m_cfg.name, "bbtargets_mask", {A * 4}, "float");
        add_output(m_cfg.name, "labels_flat", {1, A * 2}, "int32_t");
        add_output(m_cfg.name, "labels_mask", {A * 2, 1}, "int32_t");
        add_output(m_cfg.name, "image_shape", {2, 1}, "int32_t");
        add_output(m_cfg.name, "gt_boxes", {m, 4}, "float");
        add_output(m_cfg.name, "gt_box_count", {1, 1}, "int32_t");
        add_output(m_cfg.name, "gt_class_count", {m, 1}, "int32_t");
        add_output(m_cfg.name, "image_scale", {1, 1}, "float");
        add_output(m_cfg.name, "difficult_flag", {m, 1}, "int32_t");
    }
    rcnn_config        m_cfg;
    std::vector<float> m_anchors;
    uint64_t           m_anchors_key = 0;
};

// video::config (etl_video.hpp:33-66): max_frame_count REQUIRED, name optional, frame an image::config;
// one buffer {frame.channels, max_frame_count, frame.height, frame.width} of frame.output_type.
struct video_config {
    int64_t      max_frame_count = 0;
    std::string  name;
    image_config frame;
    shape_type   shape;
    // aeon builds image::config from js["frame"] first (etl_video.hpp:40-41): without one that is its "missing
    // image config" runtime_error.  A clip has no pixels without its frame config, so there is nothing of it
    // this stage could run.
    static const Json& frame_of(const Json& js)
    {
        if (js.is_null()) throw std::runtime_error("missing video config in json config");
        if (!js.has("frame") || js.at("frame").is_null())
            throw std::runtime_error("missing image config in json config: etl type 'video' without its 'frame' is "
                                     "outside the HIP image stage");
        return js.at("frame");
    }
    explicit video_config(const Json& js) : frame(frame_of(js))
    {
        if (!js.has("max_frame_count")) invalid("Required Argument: 'max_frame_count' not set");
        get_num(js, "max_frame_count", max_frame_count);
        get_str(js, "name", name);
        verify_config("video", {"type", "max_frame_count", "name", "frame"}, js);
        // aeon validates nothing more.  Its loader writes three uint8 planes per frame whatever the config says
        // (etl_video.cpp:76-107): into a one-plane item with channels 1, into a wider item with another
        // output_type.  This stage refuses both, and a frame count it cannot launch with.
        if (max_frame_count <= 0 || max_frame_count > 65535) invalid("invalid max_frame_count");
        if (frame.channels != 3) invalid("video: frame 'channels' must be 3 (the loader writes three planes per frame)");
        if (frame.shape.otype.dtype != AEON_DTYPE_U8)
            throw unsupported_error("video: frame 'output_type' must be uint8_t (the loader writes uint8 planes)");
        if ((uint64_t)max_frame_count * frame.height * frame.width * 3 > (uint64_t)INT32_MAX)
            throw unsupported_error("video: a clip item above 2^31 - 1 bytes");
        shape.shape = {frame.channels, (size_t)max_frame_count, frame.height, frame.width};
        shape.names = {"channels", "frames", "height", "width"};
        shape.otype = frame.shape.otype;
    }
};

// provider::video (provider.cpp:477-517).  The param factory is built from augmentation["frame"], not from
// the augmentation object itself (provider.cpp:483).  Per record: video::extractor's demux (avi_host.hpp) of
// the kept frames only -- aeon decodes every frame and its transformer drops those past max_frame_count
// (etl_video.cpp:23-41, 55-63): the same output --, params drawn from the first frame's size unless an
// earlier element of the record drew, the frames' JPEGs decoded by the JPEG stage and the clip written by
// aeon_hip_video_batch at post_process time.  The frame config's bgr_to_rgb, channel_major and the
// factory's fixed_aspect_ratio / mean / stddev are parsed and ignored, as aeon's loader ignores them.
class video_provider : public etl_provider {
public:
    video_provider(const Json& js, const Json& aug)
        : m_cfg(js), m_factory(aug.has("frame") ? aug.at("frame") : Json()), m_name(create_name(m_cfg.name, "video"))
    {
    }
    std::vector<std::pair<std::string, shape_type>> output_shapes() const override { return {{m_name, m_cfg.shape}}; }
    const param_factory* factory() const override { return &m_factory; }
    void from_abi(const aeon_encoded_elem& in, int, decoded_element& e) const override { e.size = in.size; }
    std::unique_ptr<window_part> new_part(int n) const override
    {
        std::unique_ptr<video_part> p(new video_part);
        p->clips.resize(n), p->counts.assign(n, 0);
        p->descs.assign((size_t)n * m_cfg.max_frame_count, aeon_img_desc{});
        return p;
    }
    // video::extractor: the demux, the kept frames' JPEG headers, the element's size set to the first frame's
    void inspect(window_part& part, int idx, decoded_element& e) const override
    {
        video_clip&       c  = static_cast<video_part&>(part).clips[idx];
        const std::string at = ", at idx " + std::to_string(idx);
        if (!e.data || e.size == 0) throw std::runtime_error("received encoded video with size 0" + at);
        const int   D = (int)m_cfg.max_frame_count;
        int         count = 0, aw = 0, ah = 0;
        std::string err;
        c.frames.assign((size_t)D, aeon_avi_frame{});
        if (avi_frames(e.data, e.size, c.frames.data(), D, &count, &aw, &ah, err) != 0) invalid(err + at);
        c.frames.resize((size_t)std::min(count, D));
        // every decoded frame goes through transform_single_image with the one params set, drawn for the first
        // frame's size: a frame of another size would be cropped with a cropbox that is not its own
        for (size_t d = 0; d < c.frames.size(); d++) {
            if (c.frames[d].size == 0) continue; // repeats the previous frame
            int fw = 0, fh = 0, comps = 0;
            check(aeon_jpeg_info(e.data + c.frames[d].offset, c.frames[d].size, &fw, &fh, &comps));
            if (d == 0) c.width = fw, c.height = fh;
            else if (fw != c.width || fh != c.height)
                invalid("video: frame " + std::to_string(d) + " is " + std::to_string(fw) + "x" + std::to_string(fh) +
                        ", the first frame " + std::to_string(c.width) + "x" + std::to_string(c.height) + at);
        }
        e.width = c.width, e.height = c.height, e.channels = 3, e.stride = c.width * 3;
        if (e.width <= 0 || e.height <= 0) throw std::runtime_error("received encoded video with size 0" + at);
    }
    // one source-arena slot per distinct non-empty frame of the clip, each a JPEG file of its own (imdecode COLOR:
    // 3 channels); an empty chunk's frame is the previous frame's slot again (cap_mjpeg_decoder.cpp:138-141)
    void layout_record(window_part& part, arena_region r, int idx, const decoded_element& e, size_t& offset,
                       jpeg_list& jpegs) const override
    {
        if (r != arena_region::device_decoded) return;
        video_part&       v   = static_cast<video_part&>(part);
        const video_clip& c   = v.clips[idx];
        aeon_img_desc*    row = &v.descs[(size_t)idx * m_cfg.max_frame_count];
        for (size_t d = 0; d < c.frames.size(); d++) {
            if (c.frames[d].size == 0) {
                row[d] = row[d - 1]; // (the demux refuses an empty first frame)
                continue;
            }
            row[d] = aeon_img_desc{offset, c.width, c.height, c.width * 3, 3, 0, 0};
            jpegs.add(e.data + c.frames[d].offset, c.frames[d].size, row[d]);
            offset += arena_align((size_t)c.width * c.height * 3);
        }
        v.counts[idx] = (int32_t)c.frames.size();
    }
    // video::transformer + loader over the clip's decoded frames
    void launch(aeon_hip_ctx* ctx, const decode_window& w, size_t k, const uint8_t* dev_arena, void* const* out,
                void* stream) const override
    {
        const video_part& v = static_cast<const video_part&>(*w.parts[k]);
        check(aeon_hip_video_batch(ctx, w.n, v.counts.data(), v.descs.data(), dev_arena, w.params[k].data(),
                                   (int)m_cfg.max_frame_count, (int)m_cfg.frame.width, (int)m_cfg.frame.height, out[0],
                                   m_cfg.shape.byte_size(), stream));
    }

protected:
    bool draw_over(const window_part&, int, const decoded_element& e, draw_source& s) const override
    {
        s = draw_source{e.width, e.height, (int)m_cfg.frame.width, (int)m_cfg.frame.height};
        return true;
    }

private:
    video_config  m_cfg;
    param_factory m_factory;
    std::string   m_name;
};

// label::config / extractor / loader (etl_label.hpp:36-150) and provider::label (provider.cpp:190-216): shape
// {1} of output_type (default uint32_t); the datum is 4 bytes read as a native int (binary) or text through
// std::stoi, and the loader copies the first sizeof(output_type) bytes of that int.  With an 8-byte
// output_type aeon copies 4 bytes past the int: refused here.  The provider draws no params.
class label_provider : public etl_provider {
public:
    explicit label_provider(const Json& js)
    {
        std::string otype = "uint32_t", name, type;
        get_str(js, "name", name);
        get_bool(js, "binary", m_binary);
        get_str(js, "type", type);
        get_str(js, "output_type", otype);
        if (!output_type::is_valid_type(otype)) invalid("value for 'output_type' out of range");
        verify_config("label", {"name", "binary", "type", "output_type"}, js);
        m_shape.shape = {1};
        m_shape.otype = output_type(otype);
        if (m_shape.otype.size > sizeof(int))
            throw unsupported_error("label: an 8-byte 'output_type' (aeon's loader copies past its int)");
        m_name = create_name(name, "label");
    }
    std::vector<std::pair<std::string, shape_type>> output_shapes() const override { return {{m_name, m_shape}}; }
    const param_factory* factory() const override { return nullptr; }
    void from_abi(const aeon_encoded_elem& in, int, decoded_element& e) const override { e.size = in.size; }
    std::unique_ptr<window_part> new_part(int n) const override
    {
        std::unique_ptr<label_part> p(new label_part);
        p->values.resize(n);
        return p;
    }
    // label::extractor
    void inspect(window_part& part, int idx, decoded_element& e) const override
    {
        int32_t&          v  = static_cast<label_part&>(part).values[idx];
        const std::string at = ", at idx " + std::to_string(idx);
        if (!e.data || e.size == 0) throw std::runtime_error("received encoded image with size 0" + at);
        if (m_binary) {
            if (e.size != 4)
                invalid("Only 4 byte buffers can be loaded as int32.  label_extractor::extract received " +
                        std::to_string(e.size) + " bytes" + at);
            std::memcpy(&v, e.data, 4);
            return;
        }
        try {
            v = (int32_t)std::stoi(std::string((const char*)e.data, e.size));
        } catch (const std::invalid_argument&) {
            invalid("Cannot convert label '" + std::string((const char*)e.data, std::min<size_t>(e.size, 32)) + "' to integer" + at);
        } catch (const std::out_of_range&) {
            invalid("String to int conversion out of range error" + at);
        }
    }
    void layout_window(window_part& part, arena_region r, int n, size_t& offset) const override
    {
        if (r != arena_region::label_items) return;
        static_cast<label_part&>(part).offset = offset;
        offset += arena_align((size_t)n * m_shape.otype.size);
    }
    void stage_window(const decode_window& w, size_t k) const override
    {
        const label_part& l = static_cast<const label_part&>(*w.parts[k]);
        host_output(l, w.n, w.arena + l.offset);
    }
    void launch(aeon_hip_ctx*, const decode_window& w, size_t k, const uint8_t*, void* const* out, void* stream) const override
    {
        if (!out[0]) return; // a host output: written by host_output
        const label_part& l = static_cast<const label_part&>(*w.parts[k]);
        hip_check(hipMemcpyAsync(out[0], w.arena + l.offset, (size_t)w.n * m_shape.otype.size, hipMemcpyHostToDevice,
                                 (hipStream_t)stream),
                  "hipMemcpyAsync");
    }
    // label::loader::load (etl_label.hpp:141-146): the first sizeof(output_type) bytes of the int
    bool host_output(const window_part& part, int n, void* out) const override
    {
        const size_t b = m_shape.otype.size;
        for (int i = 0; i < n; i++) std::memcpy((uint8_t*)out + (size_t)i * b, &static_cast<const label_part&>(part).values[i], b);
        return true;
    }

protected:
    bool draw_over(const window_part&, int, const decoded_element&, draw_source&) const override { return false; }

private:
    bool        m_binary = false;
    shape_type  m_shape;
    std::string m_name;
};

} // namespace

// The first element of a record that draws makes the record's params (localization_ssd: make_ssd_params over
// the extracted boxes, the others make_params); every later element copies them.
void etl_provider::draw(const window_part& part, int idx, const decoded_element& e, augmentation& aug,
                        std::minstd_rand0& random, aeon_aug_params& params, light_split* ls) const
{
    draw_source s;
    if (!draw_over(part, idx, e, s)) return;
    if (!aug.has) {
        const param_factory& f = *factory();
        aeon_aug_params*     p = &aug.image;
        if (s.nboxes >= 0 && ls)
            f.make_ssd_params_split(random, s.in_w, s.in_h, s.out_w, s.out_h, s.boxes, s.nboxes, ls->entry_avail, p, &ls->exit_saved);
        else if (s.nboxes >= 0) f.make_ssd_params(random, s.in_w, s.in_h, s.out_w, s.out_h, s.boxes, s.nboxes, p);
        else if (ls) f.make_params_split(random, s.in_w, s.in_h, s.out_w, s.out_h, ls->entry_avail, p, &ls->exit_saved);
        else f.make_params(random, s.in_w, s.in_h, s.out_w, s.out_h, p);
        aug.has = true;
    }
    params = aug.image;
}

provider_base::provider_base(const Json& js, const std::vector<Json>& etl, const Json& aug)
    : provider_interface(js, etl.size())
{
    bool device_work = false;
    for (const Json& j : etl) {
        std::string type;
        without_type(j, type);
        std::unique_ptr<etl_provider> p;
        if (type == "image") p.reset(new pixel_provider(j, aug, false));
        else if (type == "pixelmask") p.reset(new pixel_provider(j, aug, true));
        else if (type == "boundingbox") p.reset(new box_provider(j, aug, AEON_BOX_BOUNDINGBOX));
        else if (type == "localization_ssd") p.reset(new box_provider(j, aug, AEON_BOX_SSD));
        else if (type == "localization_rcnn") {
            if (m_shuffler >= 0) invalid("one localization_rcnn element per record");
            p.reset(new rcnn_provider(j, aug));
            m_shuffler = (int)m_providers.size();
        } else if (type == "video") p.reset(new video_provider(j, aug));
        else if (type == "label") p.reset(new label_provider(j));
        else if (type == "blob" || type == "char_map" || type == "label_map")
            throw std::runtime_error("etl type '" + type + "' is outside the HIP image stage");
        else
            invalid("unsupported etl type '" + type + "'");
        m_out_first.push_back((int)m_output_shapes.size());
        for (auto& s : p->output_shapes()) m_output_shapes.push_back(std::move(s));
        m_has_sized = m_has_sized || (type != "image" && type != "pixelmask");
        device_work = device_work || type != "label";
        m_providers.push_back(std::move(p));
    }
    m_out_first.push_back((int)m_output_shapes.size());
    // A record of labels alone has no pixels, boxes or clips: the decode stage would open a device to copy a few
    // ints.  aeon's CPU provider is the place for such a config; here label is the companion of a device element.
    if (!device_work && !m_providers.empty())
        throw std::runtime_error("etl type 'label' on its own is outside the HIP image stage: it accompanies an image, "
                                 "pixelmask, box or video element");
}

decode_window provider_base::new_window(int n) const
{
    decode_window w;
    w.n = n;
    w.params.assign(m_providers.size(), std::vector<aeon_aug_params>(n));
    for (const auto& p : m_providers) w.parts.push_back(p->new_part(n));
    return w;
}

void provider_base::inspect_window(int n, decoded_element* records, decode_window& w, thread_pool& pool) const
{
    const size_t ne = m_providers.size();
    // tasks of consecutive records, about eight per worker: a record's inspection may be a clip's demux or a
    // null check, and a task per record cost a 1,024-record window of decoded images 200 us of task hand-out
    const int chunk = std::max(1, n / (8 * pool.size()));
    pool.run((n + chunk - 1) / chunk, [&](int t) {
        for (int i = t * chunk; i < std::min(n, (t + 1) * chunk); i++)
            for (size_t k = 0; k < ne; k++) m_providers[k]->inspect(*w.parts[k], i, records[(size_t)i * ne + k]);
    });
}

void provider_base::draw(int idx, const decoded_element* elems, decode_window& w, std::minstd_rand0& random,
                         light_split* ls) const
{
    augmentation aug;
    for (size_t k = 0; k < m_providers.size(); k++)
        m_providers[k]->draw(*w.parts[k], idx, elems[k], aug, random, w.params[k][idx], ls);
}

// aeon runs provide() -- make_params included -- on its pool threads (batch_decoder.cpp:62-71); with
// one engine per record the draws are independent but for the lighting normal_distribution's cache
// inside the shared factory (augment_image.hpp:153-185), which passes one value from a record to the
// next.  Record i makes exactly three normal draws, each toggling the cache, so whether it starts
// with a cached value is known before any record is drawn: every record draws on the pool with that
// entry state (make_params_split), and one in-order pass hands each cached value to the next record.
// The params equal the in-order loop's bit for bit (tests/test_host.py draw-window tests).
void provider_base::draw_window(int n, const decoded_element* records, decode_window& w,
                                std::vector<std::minstd_rand0>& engines, thread_pool& pool) const
{
    const size_t ne = m_providers.size();
    size_t first = 0; // the first element that draws (aug.has after it): label providers draw nothing
    while (first + 1 < ne && !m_providers[first]->factory()) first++;
    const param_factory& F = *m_providers[first]->factory();
    const bool               lit = F.lighting_on();
    std::vector<light_split> ls(lit ? n : 0);
    const bool               a0 = F.light_avail();
    for (int i = 0; i < (int)ls.size(); i++) ls[i].entry_avail = a0 != ((i & 1) != 0);
    // tasks of 32 consecutive records, each engine drawn from a local copy: eight engines share a
    // cache line, and threads drawing neighbouring records through them made the pool slower than
    // one thread (C3 window of 1024: 399 vs 374 us)
    // The engines advance in a scratch copy committed (with the lighting state) only once every
    // record drew: a record that throws (an element of size 0) leaves the decoder as it was.
    constexpr int kChunk = 32;
    std::vector<std::minstd_rand0> next(engines.begin(), engines.begin() + n);
    pool.run((n + kChunk - 1) / kChunk, [&](int t) {
        for (int i = t * kChunk; i < std::min(n, (t + 1) * kChunk); i++)
            draw(i, records + (size_t)i * ne, w, next[i], lit ? &ls[i] : nullptr);
    });
    std::copy(next.begin(), next.end(), engines.begin());
    if (!lit) return;
    float cached = F.light_saved();
    for (int i = 0; i < n; i++) {
        if (ls[i].entry_avail)
            for (size_t k = 0; k < ne; k++) w.params[k][i].lighting[0] = cached;
        else
            cached = ls[i].exit_saved;
    }
    F.set_light_state(!ls[n - 1].entry_avail, cached);
}

void provider_base::layout(window_plan& p) const
{
    const size_t ne = m_providers.size();
    size_t       offset = 0;
    p.jpegs.assign(ne, jpeg_list{});
    for (arena_region r : {arena_region::box_tables, arena_region::label_items})
        for (size_t k = 0; k < ne; k++) m_providers[k]->layout_window(*p.w.parts[k], r, p.w.n, offset);
    for (arena_region r : {arena_region::staged, arena_region::device_decoded}) {
        for (int i = 0; i < p.w.n; i++)
            for (size_t k = 0; k < ne; k++)
                m_providers[k]->layout_record(*p.w.parts[k], r, i, p.records[(size_t)i * ne + k], offset, p.jpegs[k]);
        if (r == arena_region::staged) p.staged = offset;
    }
    p.total = std::max<size_t>(offset, 16);
}

void provider_base::stage(const window_plan& p, thread_pool& pool) const
{
    const size_t ne = m_providers.size();
    for (size_t k = 0; k < ne; k++) m_providers[k]->stage_window(p.w, k);
    pool.run(p.w.n, [&](int i) {
        for (size_t k = 0; k < ne; k++) m_providers[k]->stage_record(p.w, k, i, p.records[(size_t)i * ne + k]);
    });
}

void provider_base::post_process(aeon_hip_ctx* ctx, const decode_window& w, const uint8_t* dev_arena, void* const* outputs,
                                 void* stream) const
{
    // image + pixelmask with the same params per record (provider.cpp:365-393): one pair call, whose
    // masks run inside the image launch
    const aeon_out_desc *io = nullptr, *mo = nullptr;
    if (m_providers.size() == 2 && (io = m_providers[0]->pixel_out(false)) && (mo = m_providers[1]->pixel_out(true)) &&
        w.n > 0 && std::memcmp(w.params[0].data(), w.params[1].data(), (size_t)w.n * sizeof(aeon_aug_params)) == 0) {
        check(aeon_hip_augment_pair_batch(ctx, w.n, w.parts[0]->descs.data(), dev_arena, w.parts[1]->descs.data(), dev_arena,
                                          w.params[0].data(), io, outputs[0], mo, outputs[1], stream));
        return;
    }
    for (size_t k = 0; k < m_providers.size(); k++)
        m_providers[k]->launch(ctx, w, k, dev_arena, outputs + m_out_first[k], stream);
}

std::shared_ptr<provider_base> provider_factory::create(const Json& config)
{
    if (!config.has("etl")) invalid("required argument 'etl' not set");
    std::vector<Json> etl = config.at("etl").array();
    Json              aug;
    if (config.has("augmentation")) {
        const auto& a = config.at("augmentation").array();
        for (const Json& j : a)
            if (!j.has("type")) invalid("augmentation missing 'type'");
        if (!a.empty()) aug = a[0]; // provider_factory.cpp:39-43: only the first is used
    }
    return std::make_shared<provider_base>(config, etl, aug);
}

// ---- thread_pool ----------------------------------------------------------------------------------
thread_pool::thread_pool(std::vector<int> affinity_map) : m_map(std::move(affinity_map))
{
    // the worker count is fixed before any worker starts: a worker must not read m_threads while this
    // constructor is still growing it (ThreadSanitizer, tests/sanitize/host_driver.cpp)
    m_nthreads = std::max<int>(1, (int)m_map.size());
    m_worker_cpus.resize(m_nthreads);
    m_threads.reserve(m_nthreads);
    for (int i = 0; i < m_nthreads; i++) m_threads.emplace_back([this, i] { worker(i); });
}

thread_pool::~thread_pool()
{
    {
        std::lock_guard<std::mutex> l(m_mu);
        m_stop = true;
    }
    m_cv.notify_all();
    for (auto& t : m_threads) t.join();
}

std::vector<std::vector<int>> thread_pool::worker_cpus()
{
    std::unique_lock<std::mutex> l(m_mu);
    m_done_cv.wait(l, [&] { return m_started == m_nthreads; });
    return m_worker_cpus;
}

void thread_pool::worker(int index)
{
    // thread_pool.hpp:133-138: pin to thread_affinity_map[index] (the result is not checked there
    // either: a CPU outside the cpuset leaves the thread on the process mask)
    if (index < (int)m_map.size()) {
        cpu_set_t set;
        CPU_ZERO(&set);
        CPU_SET(m_map[index], &set);
        (void)pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
    }
    {
        std::vector<int> cpus;
        cpu_set_t        got;
        if (sched_getaffinity(0, sizeof(got), &got) == 0)
            for (int c = 0; c < CPU_SETSIZE; c++)
                if (CPU_ISSET(c, &got)) cpus.push_back(c);
        std::lock_guard<std::mutex> l(m_mu);
        m_worker_cpus[index] = std::move(cpus);
        if (++m_started == m_nthreads) m_done_cv.notify_all();
    }
    long seen = 0;
    for (;;) {
        const std::function<void(int, int)>* fn;
        int                            n;
        {
            std::unique_lock<std::mutex> l(m_mu);
            m_cv.wait(l, [&] { return m_stop || m_generation != seen; });
            if (m_stop) return;
            seen = m_generation;
            fn   = m_fn;
            n    = m_n;
        }
        // dynamic task distribution (thread_pool.hpp:155-162), the task counter tagged with the run's
        // generation: a worker that wakes after its run completed (the caller has returned, fn is
        // gone) takes nothing, whatever run the counter belongs to by then
        uint64_t st = m_state.load();
        for (;;) {
            if ((uint32_t)(st >> 32) != (uint32_t)seen || (int)(uint32_t)st >= n) break;
            if (!m_state.compare_exchange_weak(st, st + 1)) continue;
            try {
                (*fn)((int)(uint32_t)st, index);
            } catch (...) {
                std::lock_guard<std::mutex> l(m_mu);
                if (!m_error) m_error = std::current_exception();
            }
            if (m_done.fetch_add(1) + 1 == n) {
                std::lock_guard<std::mutex> l(m_mu);
                m_done_cv.notify_all();
            }
            st = m_state.load();
        }
    }
}

void thread_pool::run(int n, const std::function<void(int)>& fn)
{
    run_indexed(n, [&](int i, int) { fn(i); });
}

void thread_pool::run_indexed(int n, const std::function<void(int, int)>& fn)
{
    // aeon's run() waits for every worker to check in (thread_pool.hpp:103-116); this one waits for the
    // n tasks: a pinned worker whose CPU another process holds no longer stalls the run until it is
    // scheduled (milliseconds on a shared host) when the others have done its share
    {
        std::lock_guard<std::mutex> l(m_mu);
        m_fn    = &fn;
        m_n     = n;
        m_error = nullptr;
        m_done  = 0;
        m_generation++;
        m_state = (uint64_t)(uint32_t)m_generation << 32;
    }
    m_cv.notify_all();
    std::unique_lock<std::mutex> l(m_mu);
    m_done_cv.wait(l, [&] { return m_done.load() >= n; });
    if (m_error) std::rethrow_exception(m_error); // thread_pool.hpp:113-115
}

// ---- batch_decoder -------------------------------------------------------------------------------
std::vector<int> parse_cpu_list(const std::string& cpu_list)
{
    std::vector<int>  cpus;
    std::stringstream ss(cpu_list);
    std::string       tok;
    try {
        while (std::getline(ss, tok, ',')) {
            if (tok.empty()) continue;
            const auto dash = tok.find('-');
            if (dash == std::string::npos) {
                cpus.push_back(std::stoi(tok));
            } else {
                const int from = std::stoi(tok.substr(0, dash)), to = std::stoi(tok.substr(dash + 1));
                for (int i = from; i <= to; i++) cpus.push_back(i);
            }
        }
    } catch (const std::exception&) {
        invalid("Failed to parse cpu list '" + cpu_list + "'");
    }
    std::sort(cpus.begin(), cpus.end());
    cpus.erase(std::unique(cpus.begin(), cpus.end()), cpus.end());
    const int hc = (int)std::thread::hardware_concurrency();
    if (!cpus.empty() && (cpus.front() < 0 || cpus.back() >= hc))
        invalid("One or more indexes computed from cpu list '" + cpu_list +
                "' exceed number of logical cores. Use values in range [0, " + std::to_string(hc - 1) + "].");
    return cpus;
}

std::vector<int> thread_affinity_map(const std::string& cpu_list)
{
    // util.cpp:337-373: the environment has precedence over the config
    std::string list = cpu_list;
    if (const char* e = std::getenv("AEON_CPU_LIST"))
        if (*e) list = e;
    std::vector<int> map = list.empty() ? std::vector<int>() : parse_cpu_list(list);
    if (!map.empty()) return map;
    // hc - min(2, hc/8) over the CPUs this process may run on (its affinity mask: the GPU box gives
    // each job 16 of its 256 CPUs, and workers pinned outside it would stay unpinned), further
    // capped by OMP_NUM_THREADS when the launcher sets it
    std::vector<int> allowed;
    cpu_set_t        set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0)
        for (int c = 0; c < CPU_SETSIZE; c++)
            if (CPU_ISSET(c, &set)) allowed.push_back(c);
    if (allowed.empty()) {
        allowed.resize(std::max(1u, std::thread::hardware_concurrency()));
        std::iota(allowed.begin(), allowed.end(), 0);
    }
    int hc = (int)allowed.size();
    if (const char* e = std::getenv("OMP_NUM_THREADS"))
        if (std::atoi(e) > 0) hc = std::min(hc, std::atoi(e));
    allowed.resize(std::max(1, hc - std::min(2, hc / 8)));
    return allowed;
}

int aeon_thread_count(const std::string& cpu_list) { return (int)thread_affinity_map(cpu_list).size(); }

std::vector<int> affinity_for(const std::vector<int>& map, int n)
{
    std::vector<int> out(std::max(1, n));
    for (size_t i = 0; i < out.size(); i++) out[i] = map.empty() ? -1 : map[i % map.size()];
    if (map.empty()) out.clear();
    return out;
}

batch_decoder::batch_decoder(const Json& config, int device) : m_device(device)
{
    verify_config("loader", {"manifest_filename", "manifest_root", "batch_size", "cache_directory",
                             "block_size", "batch_major", "subset_fraction", "shuffle_enable",
                             "shuffle_manifest", "cpu_list", "pinned", "random_seed", "iteration_mode",
                             "iteration_mode_count", "etl", "augmentation", "node_id", "node_count",
                             "ssd_config", "decode_thread_count"},
                  config);
    if (!config.has("batch_size")) invalid("Required Argument: 'batch_size' not set");
    get_num(config, "batch_size", m_batch_size);
    if (m_batch_size <= 0) invalid("batch_size must be > 0");
    uint32_t seed = 0, node_id = 0, node_count = 0;
    get_num(config, "random_seed", seed);
    get_num(config, "node_id", node_id);
    get_num(config, "node_count", node_count);
    if (node_count > 1) {
        if (node_id >= node_count) throw std::runtime_error("node_id can't be greater than node_count");
        if (seed == 0) seed = 1; // loader.cpp:109-113
    }
    get_bool(config, "batch_major", m_batch_major);
    std::string cpu_list;
    get_str(config, "cpu_list", cpu_list);
    std::vector<int> map = thread_affinity_map(cpu_list); // loader.cpp:159-171
    if (config.has("decode_thread_count")) { // (this stage's own knob: the map cycled or cut to it)
        int threads = 0;
        get_num(config, "decode_thread_count", threads);
        if (threads <= 0) invalid("decode_thread_count must be > 0");
        map = affinity_for(map, threads);
    }
    m_provider = provider_factory::create(config);
    m_pool.reset(new thread_pool(map));
    m_local_random.seed(std::random_device{}());
    // decoder seed = random_seed + node_id (loader.cpp:174); deterministic when non-zero
    const uint32_t dseed = seed ? seed + node_id : 0;
    m_deterministic      = dseed != 0;
    if (m_deterministic) m_seed_gen.seed(dseed); // slot engines: see slot_engines()
    // the HIP context is created on the first window (configs validate without a GPU)
}

batch_decoder::~batch_decoder()
{
    if (!m_ctx) return; // no window ran: nothing was allocated on the device
    (void)hipSetDevice(m_device);
    for (auto& ws : m_slots)
        if (ws.pending) (void)hipEventSynchronize(ws.done);
    for (auto& ws : m_slots) {
        if (ws.states_done) (void)hipEventDestroy(ws.states_done);
        if (ws.states_dev) (void)hipFree(ws.states_dev);
        if (ws.states_host) (void)hipHostFree(ws.states_host);
    }
    aeon_hip_ctx_destroy(m_ctx);
    for (auto& ws : m_slots) {
        if (ws.done) (void)hipEventDestroy(ws.done);
        if (ws.stream) (void)hipStreamDestroy(ws.stream);
        if (ws.pinned) (void)hipHostFree(ws.pinned);
        if (ws.dev_src) (void)hipFree(ws.dev_src);
        for (auto* v : {&ws.dev_out, &ws.dev_tmp})
            for (auto* p : *v)
                if (p) (void)hipFree(p);
    }
}

// The slot engines take over the states an earlier localization_rcnn window's device shuffles left.
void batch_decoder::adopt_states()
{
    if (!m_states_from) return;
    hip_check(hipEventSynchronize(m_states_from->states_done), "hipEventSynchronize");
    for (int i = 0; i < m_states_n && i < (int)m_random.size(); i++) m_random[i].seed(m_states_from->states_host[i]);
    m_states_from = nullptr;
}

// Deterministic mode: engine i of the decode window is seeded with the i-th output of
// minstd_rand0(random_seed + node_id) (batch_decoder.cpp:47-54).  aeon seeds decode_size engines
// up front; here the table grows with the largest window seen, continuing the same generator, so
// the first N engines are aeon's for any N.
void batch_decoder::grow_slot_engines(int n)
{
    while ((int)m_random.size() < n) {
        m_random.emplace_back();
        m_random.back().seed(m_seed_gen());
    }
}

namespace {
// Device address through which the kernels can store straight into host buffer p (pinned and
// mapped: hipHostMalloc / hipHostRegister), or null for pageable memory.  Such host outputs are
// written over PCIe by the augmentation (or transpose) kernels themselves -- zero-copy --, which
// measured 81.6 K against 54 K records/s host->host for C2 with a D2H copy behind the kernels
// (tools/e2e_probe.py): the kernels' store stream uses both PCIe directions' worth of requests in
// flight where the copy engine does not.  AEON_HIP_ZERO_COPY=0 keeps the device staging + D2H (the
// kernels then occupy the CUs only for their HBM-speed run; zero-copy holds them for the PCIe time).
void* zero_copy_view(void* p)
{
    static const bool on = [] {
        const char* e = std::getenv("AEON_HIP_ZERO_COPY");
        return !(e && std::atoi(e) == 0);
    }();
    if (!on || !p) return nullptr;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); // pageable memory: not an error
        return nullptr;
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer || !a.hostPointer) return nullptr;
    return (uint8_t*)a.devicePointer + ((uint8_t*)p - (uint8_t*)a.hostPointer);
}

// A roctx range over one host phase of a decode window (rocprofv3 --marker-trace shows them
// next to the kernels: draw, stage, jpeg, augment, transpose, d2h).
struct phase_range {
    explicit phase_range(const char* name) { roctxRangePush(name); }
    ~phase_range() { roctxRangePop(); }
    phase_range(const phase_range&) = delete;
    phase_range& operator=(const phase_range&) = delete;
};

void grow_dev(uint8_t*& p, size_t& cap, size_t bytes)
{
    if (bytes <= cap) return;
    if (p) hip_check(hipFree(p), "hipFree");
    p = nullptr;
    hip_check(hipMalloc((void**)&p, bytes), "hipMalloc");
    cap = bytes;
}
} // namespace

// One decode window on `stream` using window slot ws (whose previous window has completed):
// batch_decoder::filler (batch_decoder.cpp:73-99) with the per-record body split into
//   plan:          inspect (headers, demux, metadata) -> make_params (aeon's deterministic draw order) ->
//                  the arena layout; host only
//   stage_sources: staged bytes into pinned memory on the pool -> one H2D -> JPEG entropy decode and
//                  IDCT/colour into the source arena
//   route_outputs: device outputs in place, pinned host outputs through zero_copy_view, others staged
//   launch:        the providers' kernels (post_process) -> [batch transpose] -> D2H of staged outputs
void batch_decoder::enqueue(window_slot& ws, int n, const decoded_element* in, void* const* outputs, bool on_device,
                            hipStream_t stream)
{
    // aeon's shuffles draw from the slot engine after make_params and leave it advanced
    // (batch_decoder.cpp:62-71): an earlier window's end states first, then this window's draws
    if (m_deterministic) adopt_states();
    window_plan   p = plan(n, in);
    engine_states end;
    // once post_process has queued the engine states' copy and its event, the next window adopts them,
    // whatever happens to the rest of this one
    struct adopt_later {
        batch_decoder& d;
        engine_states& end;
        window_slot&   ws;
        int            n;
        ~adopt_later()
        {
            if (end.queued) d.m_states_from = &ws, d.m_states_n = n;
        }
    } adopt_guard{*this, end, ws, n};
    if (m_provider->shuffles()) {
        if (m_deterministic) slot_states(ws, n, end);
        m_provider->take_engines(p.w, std::move(p.engines), &end);
    }
    stage_sources(ws, p, stream);
    const routed_outputs r = route_outputs(ws, p.w, outputs, on_device);
    launch(ws, p.w, r, outputs, stream);
}

// The draw phase of a window, host only.  Every element goes through its provider's inspect on the pool; then
// batch_decoder::process: the slot engine of record i draws its params (deterministic mode swaps the slot
// engine in and out, batch_decoder.cpp:62-71).  With slot engines the draws run on the pool (draw_window:
// aeon's in-order params exactly) unless serial asks for the in-order loop.  A record of a provider that
// shuffles gets its engine word: the slot engine's state after the draw, or -- with the one engine of
// non-deterministic mode, where aeon's result depends on its thread scheduling -- one further draw of it.
void batch_decoder::draw(window_plan& p, int n, const decoded_element* in, bool serial)
{
    const int ne = (int)m_provider->get_input_count();
    if (m_deterministic) grow_slot_engines(n);
    p.records.assign(in, in + (size_t)n * ne);
    p.w = m_provider->new_window(n);
    {
        phase_range r("aeon.inspect");
        m_provider->inspect_window(n, p.records.data(), p.w, *m_pool);
    }
    phase_range r("aeon.draw");
    const bool  words = m_provider->shuffles();
    if (words) p.engines.resize(n);
    if (m_deterministic && !serial) {
        m_provider->draw_window(n, p.records.data(), p.w, m_random, *m_pool);
        for (int i = 0; words && i < n; i++) p.engines[i] = minstd_state(m_random[i]);
        return;
    }
    for (int i = 0; i < n; i++) {
        std::minstd_rand0& random = m_deterministic ? m_random[i] : m_local_random;
        m_provider->draw(i, p.records.data() + (size_t)i * ne, p.w, random);
        if (words) p.engines[i] = m_deterministic ? minstd_state(random) : (uint32_t)random();
    }
}

window_plan batch_decoder::plan(int n, const decoded_element* records)
{
    window_plan p;
    draw(p, n, records, false);
    m_provider->layout(p);
    return p;
}

void batch_decoder::draw_params(int n, const decoded_element* records, aeon_aug_params* params, bool serial)
{
    if (n <= 0) return;
    window_plan p;
    draw(p, n, records, serial);
    std::copy(p.w.params[0].begin(), p.w.params[0].end(), params);
}

// localization_rcnn, deterministic mode: the slot's buffers for the window's engine end states
void batch_decoder::slot_states(window_slot& ws, int n, engine_states& end)
{
    if ((size_t)n > ws.states_cap) {
        if (ws.states_dev) hip_check(hipFree(ws.states_dev), "hipFree");
        if (ws.states_host) hip_check(hipHostFree(ws.states_host), "hipHostFree");
        ws.states_dev = ws.states_host = nullptr, ws.states_cap = 0;
        hip_check(hipMalloc((void**)&ws.states_dev, (size_t)n * sizeof(uint32_t)), "hipMalloc");
        hip_check(hipHostMalloc((void**)&ws.states_host, (size_t)n * sizeof(uint32_t), hipHostMallocDefault),
                  "hipHostMalloc");
        ws.states_cap = (size_t)n;
    }
    if (!ws.states_done) hip_check(hipEventCreateWithFlags(&ws.states_done, hipEventDisableTiming), "hipEventCreate");
    end.dev = ws.states_dev, end.host = ws.states_host, end.done = ws.states_done;
}

// The source arena: what the plan staged (box tables, label items, decoded elements) written into the slot's
// pinned memory and copied H2D in one piece, then the JPEG files decoded on the device behind it.
void batch_decoder::stage_sources(window_slot& ws, window_plan& p, hipStream_t stream)
{
    if (p.staged > ws.pinned_cap) {
        if (ws.pinned) hip_check(hipHostFree(ws.pinned), "hipHostFree");
        ws.pinned = nullptr;
        hip_check(hipHostMalloc((void**)&ws.pinned, p.staged, hipHostMallocDefault), "hipHostMalloc");
        ws.pinned_cap = p.staged;
    }
    grow_dev(ws.dev_src, ws.dev_src_cap, p.total);
    p.w.arena = ws.pinned;
    if (p.staged) {
        {
            phase_range r("aeon.stage");
            m_provider->stage(p, *m_pool);
        }
        phase_range r("aeon.h2d_enqueue");
        hip_check(hipMemcpyAsync(ws.dev_src, ws.pinned, p.staged, hipMemcpyHostToDevice, stream), "hipMemcpyAsync");
    }
    // (a window of clips holds many more files than a window of images: calls of a JPEG window's size, so the
    // stage's two staging sets stay at the size the image path sizes them to)
    constexpr size_t kJpegCallFiles = 512;
    for (const jpeg_list& j : p.jpegs) {
        phase_range r("aeon.jpeg");
        for (size_t f = 0; f < j.files.size(); f += kJpegCallFiles)
            check(aeon_hip_decode_jpeg_batch(m_ctx, (int)std::min(kJpegCallFiles, j.files.size() - f), j.files.data() + f,
                                             j.sizes.data() + f, j.descs.data() + f, ws.dev_src, stream));
        for (size_t f = 0; f < j.png.files.size(); f += kJpegCallFiles)
            check(aeon_hip_decode_png_batch(m_ctx, (int)std::min(kJpegCallFiles, j.png.files.size() - f), j.png.files.data() + f,
                                            j.png.sizes.data() + f, j.png.modes.data() + f, j.png.descs.data() + f, ws.dev_src,
                                            stream));
        for (size_t f = 0; f < j.pixmap.files.size(); f += kJpegCallFiles)
            check(aeon_hip_decode_pixmap_batch(m_ctx, (int)std::min(kJpegCallFiles, j.pixmap.files.size() - f),
                                               j.pixmap.files.data() + f, j.pixmap.sizes.data() + f, j.pixmap.modes.data() + f,
                                               j.pixmap.descs.data() + f, ws.dev_src, stream));
        for (size_t f = 0; f < j.tiff.files.size(); f += kJpegCallFiles)
            check(aeon_hip_decode_tiff_batch(m_ctx, (int)std::min(kJpegCallFiles, j.tiff.files.size() - f), j.tiff.files.data() + f,
                                             j.tiff.sizes.data() + f, j.tiff.modes.data() + f, j.tiff.descs.data() + f, ws.dev_src,
                                             stream));
    }
}

// outputs[] follow get_output_shapes() (a provider may own several buffers: localization_ssd five).  A device
// output is written in place; a pinned host output through its device view (zero_copy_view); any other host
// output is staged in the slot's device buffer and copied D2H; a provider that needs no device has written
// its host output here and now (a label: no device round trip), and its dev[] stays null.
batch_decoder::routed_outputs batch_decoder::route_outputs(window_slot& ws, const decode_window& w, void* const* outputs,
                                                           bool on_device)
{
    const auto&    oshapes = m_provider->get_output_shapes();
    const int      no      = (int)oshapes.size();
    routed_outputs r{std::vector<void*>(no), std::vector<bool>(no, false), std::vector<bool>(no, false)};
    ws.dev_out.resize(no, nullptr), ws.dev_out_cap.resize(no, 0);
    for (size_t k = 0; k < m_provider->providers().size() && !on_device; k++) {
        const int o  = m_provider->output_first(k);
        r.on_host[o] = m_provider->providers()[k]->host_output(*w.parts[k], w.n, outputs[o]);
    }
    for (int k = 0; k < no; k++) {
        if (r.on_host[k]) continue;
        if (on_device) r.dev[k] = outputs[k];
        else if (void* v = zero_copy_view(outputs[k])) r.dev[k] = v;
        else {
            grow_dev(ws.dev_out[k], ws.dev_out_cap[k], (size_t)w.n * oshapes[k].second.byte_size());
            r.dev[k]      = ws.dev_out[k];
            r.copy_out[k] = true;
        }
    }
    return r;
}

// The providers' device work into the routed outputs -- through dev_tmp and a transpose per batch for
// batch_major=false --, the D2H of the staged host outputs, and the window's completion event.
void batch_decoder::launch(window_slot& ws, const decode_window& w, const routed_outputs& r, void* const* outputs,
                           hipStream_t stream)
{
    const auto& oshapes = m_provider->get_output_shapes();
    const int   no = (int)oshapes.size(), n = w.n;
    phase_range range("aeon.launch");
    if (m_batch_major) {
        m_provider->post_process(m_ctx, w, ws.dev_src, r.dev.data(), stream);
    } else {
        ws.dev_tmp.resize(no, nullptr), ws.dev_tmp_cap.resize(no, 0);
        std::vector<void*> tmp(no);
        for (int k = 0; k < no; k++) {
            if (r.on_host[k]) continue; // (one element per item: its transpose is itself)
            grow_dev(ws.dev_tmp[k], ws.dev_tmp_cap[k], (size_t)n * oshapes[k].second.byte_size());
            tmp[k] = ws.dev_tmp[k];
        }
        m_provider->post_process(m_ctx, w, ws.dev_src, tmp.data(), stream);
        for (int k = 0; k < no; k++) {
            if (r.on_host[k]) continue;
            const shape_type& sh    = oshapes[k].second;
            const size_t      esize = sh.otype.size;
            const size_t      item  = sh.byte_size();
            for (int b = 0; b < n / m_batch_size; b++) {
                const size_t off = (size_t)b * m_batch_size * item;
                check(aeon_hip_transpose_batch(m_ctx, (uint8_t*)tmp[k] + off, (uint8_t*)r.dev[k] + off,
                                               m_batch_size, (int64_t)(item / esize), (int)esize, stream));
            }
        }
    }
    for (int k = 0; k < no; k++)
        if (r.copy_out[k]) {
            phase_range d2h("aeon.d2h_enqueue");
            hip_check(hipMemcpyAsync(outputs[k], r.dev[k], (size_t)n * oshapes[k].second.byte_size(),
                                     hipMemcpyDeviceToHost, stream),
                      "hipMemcpyAsync");
        }
    if (!ws.done) hip_check(hipEventCreateWithFlags(&ws.done, hipEventDisableTiming), "hipEventCreate");
    hip_check(hipEventRecord(ws.done, stream), "hipEventRecord");
    ws.pending = true;
}

void batch_decoder::decode(int n, const decoded_element* records, void* const* outputs, bool on_device, void* stream_)
{
    if (n <= 0) return;
    if (!m_batch_major && n % m_batch_size != 0) invalid("batch_major=false needs whole batches per decode window");
    while (!m_queue.empty()) wait(); // windows are completed in submission order
    if (m_deterministic) grow_slot_engines(n);
    if (!m_ctx) check(aeon_hip_ctx_create(m_device, &m_ctx)), ctx_share_pool(m_ctx, m_pool.get());
    hip_check(hipSetDevice(m_device), "hipSetDevice");
    window_slot& ws = m_slots[m_next];
    m_next ^= 1;
    if (ws.pending) hip_check(hipEventSynchronize(ws.done), "hipEventSynchronize");
    ws.pending = false;
    enqueue(ws, n, records, outputs, on_device, (hipStream_t)stream_);
    // the pinned arena and the window's params must outlive the copies: finish the window
    check(aeon_hip_synchronize(m_ctx, stream_));
    ws.pending = false;
}

void batch_decoder::submit(int n, const decoded_element* records, void* const* outputs, bool on_device)
{
    if (n <= 0) invalid("empty decode window");
    if (!m_batch_major && n % m_batch_size != 0) invalid("batch_major=false needs whole batches per decode window");
    if (m_queue.size() >= 2) invalid("two windows are in flight: wait() for the oldest before submitting another");
    if (m_deterministic) grow_slot_engines(n);
    if (!m_ctx) check(aeon_hip_ctx_create(m_device, &m_ctx)), ctx_share_pool(m_ctx, m_pool.get());
    hip_check(hipSetDevice(m_device), "hipSetDevice");
    const int    slot = m_next;
    window_slot& ws   = m_slots[slot];
    m_next ^= 1;
    if (!ws.stream) hip_check(hipStreamCreateWithFlags(&ws.stream, hipStreamNonBlocking), "hipStreamCreate");
    if (ws.pending) hip_check(hipEventSynchronize(ws.done), "hipEventSynchronize");
    ws.pending = false;
    enqueue(ws, n, records, outputs, on_device, ws.stream);
    m_queue.push_back(slot);
}

void batch_decoder::wait()
{
    if (m_queue.empty()) invalid("no decode window in flight");
    const int slot = m_queue.front();
    m_queue.erase(m_queue.begin());
    window_slot& ws = m_slots[slot];
    check(aeon_hip_synchronize(m_ctx, ws.stream));
    ws.pending = false;
}

// ---- manifest_file node slicing ------------------------------------------------------------------
std::vector<int64_t> manifest_node_slice(int64_t record_count, int batch_size, int node_id, int node_count)
{
    std::vector<int64_t> out;
    if (node_count <= 1) {
        out.resize(record_count);
        std::iota(out.begin(), out.end(), 0);
        return out;
    }
    if (node_id < 0 || node_id >= node_count) invalid("node_id can't be greater than node_count");
    if (batch_size <= 0) invalid("batch_size must be > 0");
    const int64_t count   = record_count / node_count;
    const int64_t batches = count / batch_size;
    out.resize(count);
    for (int64_t i = 0; i < batches * batch_size; i++) {
        const int64_t batch_num = i / batch_size, in_batch = i % batch_size;
        out[i] = batch_num * batch_size * node_count + (int64_t)batch_size * node_id + in_batch;
    }
    const int64_t tail_count = count - batches * batch_size;
    const int64_t tail_src   = batches * batch_size * node_count + tail_count * node_id;
    const int64_t tail_dst   = batches * batch_size;
    for (int64_t i = 0; i < tail_count; i++) out[i + tail_dst] = i + tail_src;
    return out;
}

} // namespace aeon_hip

// ---- C ABI of the host layer ---------------------------------------------------------------------
struct aeon_decoder {
    std::unique_ptr<aeon_hip::batch_decoder> d;
};

namespace {
thread_local std::string g_host_err;

template <typename F>
int host_guarded(F&& f)
{
    try {
        f();
        return 0;
    } catch (const std::invalid_argument& e) {
        g_host_err = e.what();
        return AEON_HIP_EINVAL;
    } catch (const aeon_hip::unsupported_error& e) {
        g_host_err = e.what();
        return AEON_HIP_EUNSUPPORTED;
    } catch (const std::exception& e) {
        g_host_err = e.what();
        return AEON_HIP_ERUNTIME;
    }
}

std::vector<aeon_hip::decoded_element> to_elements(aeon_decoder* d, int n, const aeon_encoded_elem* elems)
{
    const int ne = (int)d->d->provider().get_input_count();
    std::vector<aeon_hip::decoded_element> recs((size_t)n * ne);
    // (a datum -- JSON metadata, an AVI file, a label's bytes -- is data / size: an empty one is refused per
    // record by its provider's inspect, with aeon's message)
    for (size_t i = 0; i < recs.size(); i++) {
        recs[i].data = (const uint8_t*)elems[i].data;
        d->d->provider().providers()[i % ne]->from_abi(elems[i], (int)(i / ne), recs[i]);
    }
    return recs;
}

// decoded pixels as aeon_record_elem carries them
std::vector<aeon_hip::decoded_element> to_elements(aeon_decoder* d, int n, const aeon_record_elem* elems)
{
    std::vector<aeon_hip::decoded_element> recs((size_t)n * d->d->provider().get_input_count());
    for (size_t i = 0; i < recs.size(); i++)
        recs[i] = aeon_hip::decoded_element{(const uint8_t*)elems[i].data, elems[i].width, elems[i].height, elems[i].channels,
                                            elems[i].stride ? elems[i].stride : elems[i].width * elems[i].channels};
    return recs;
}
} // namespace

extern "C" {

int aeon_decoder_create(const char* config_json, int device, aeon_decoder** out)
{
    return host_guarded([&] {
        if (!out || !config_json) throw std::invalid_argument("null argument");
        auto* d = new aeon_decoder();
        try {
            d->d.reset(new aeon_hip::batch_decoder(aeon_hip::Json::parse(config_json), device));
        } catch (...) {
            delete d;
            throw;
        }
        *out = d;
    });
}

int aeon_decoder_destroy(aeon_decoder* d)
{
    delete d;
    return 0;
}

int aeon_decoder_output_count(aeon_decoder* d, int* count)
{
    return host_guarded([&] {
        if (!d || !count) throw std::invalid_argument("null argument");
        *count = (int)d->d->provider().get_output_shapes().size();
    });
}

int aeon_decoder_output_info(aeon_decoder* d, int index, char* name, size_t name_cap, int64_t* shape,
                             int* ndim, size_t* item_bytes, int* dtype)
{
    return host_guarded([&] {
        if (!d) throw std::invalid_argument("null decoder");
        const auto& shapes = d->d->provider().get_output_shapes();
        if (index < 0 || index >= (int)shapes.size()) throw std::invalid_argument("output index out of range");
        const auto& s = shapes[index];
        if (name && name_cap) {
            std::strncpy(name, s.first.c_str(), name_cap - 1);
            name[name_cap - 1] = 0;
        }
        if (ndim) *ndim = (int)s.second.shape.size();
        if (shape)
            for (size_t i = 0; i < s.second.shape.size(); i++) shape[i] = (int64_t)s.second.shape[i];
        if (item_bytes) *item_bytes = s.second.byte_size();
        if (dtype) *dtype = s.second.otype.dtype;
    });
}

int aeon_decoder_decode(aeon_decoder* d, int n, const aeon_record_elem* elems, void* const* outputs,
                        int outputs_on_device, void* stream)
{
    return host_guarded([&] {
        if (!d || (n > 0 && (!elems || !outputs))) throw std::invalid_argument("null argument");
        if (d->d->provider().has_sized())
            throw std::invalid_argument("aeon_record_elem carries no byte size for the metadata of a boundingbox / "
                                        "localization_ssd element, a video or a label datum: use aeon_decoder_decode_encoded");
        auto recs = to_elements(d, n, elems);
        d->d->decode(n, recs.data(), outputs, outputs_on_device != 0, stream);
    });
}

int aeon_decoder_draw_params(aeon_decoder* d, int n, const aeon_record_elem* elems, aeon_aug_params* params,
                             int serial)
{
    return host_guarded([&] {
        if (!d || (n > 0 && (!elems || !params))) throw std::invalid_argument("null argument");
        if (d->d->provider().has_sized())
            throw std::invalid_argument("aeon_record_elem carries no byte size for the metadata of a boundingbox / "
                                        "localization_ssd element, a video or a label datum: the draws of such a config need "
                                        "the records");
        auto recs = to_elements(d, n, elems);
        d->d->draw_params(n, recs.data(), params, serial != 0);
    });
}

int aeon_decoder_decode_encoded(aeon_decoder* d, int n, const aeon_encoded_elem* elems, void* const* outputs,
                                int outputs_on_device, void* stream)
{
    return host_guarded([&] {
        if (!d || (n > 0 && (!elems || !outputs))) throw std::invalid_argument("null argument");
        auto recs = to_elements(d, n, elems);
        d->d->decode(n, recs.data(), outputs, outputs_on_device != 0, stream);
    });
}

int aeon_decoder_submit(aeon_decoder* d, int n, const aeon_encoded_elem* elems, void* const* outputs,
                        int outputs_on_device)
{
    return host_guarded([&] {
        if (!d || n <= 0 || !elems || !outputs) throw std::invalid_argument("null argument");
        auto recs = to_elements(d, n, elems);
        d->d->submit(n, recs.data(), outputs, outputs_on_device != 0);
    });
}

int aeon_decoder_wait(aeon_decoder* d)
{
    return host_guarded([&] {
        if (!d) throw std::invalid_argument("null argument");
        d->d->wait();
    });
}

int aeon_manifest_node_slice(int64_t record_count, int batch_size, int node_id, int node_count,
                             int64_t* indices, int64_t* count)
{
    return host_guarded([&] {
        if (!count) throw std::invalid_argument("null count");
        auto v = aeon_hip::manifest_node_slice(record_count, batch_size, node_id, node_count);
        if (indices) std::copy(v.begin(), v.end(), indices);
        *count = (int64_t)v.size();
    });
}

int aeon_thread_affinity_map(const char* cpu_list, int* cpus, int cap, int* count)
{
    return host_guarded([&] {
        if (!count || (cap > 0 && !cpus)) throw std::invalid_argument("null argument");
        const auto map = aeon_hip::thread_affinity_map(cpu_list ? cpu_list : "");
        for (int i = 0; i < std::min(cap, (int)map.size()); i++) cpus[i] = map[i];
        *count = (int)map.size();
    });
}

int aeon_decoder_pool_cpus(aeon_decoder* d, int worker, int* map_cpu, int* cpus, int cap, int* count)
{
    return host_guarded([&] {
        if (!d || !count || (cap > 0 && !cpus)) throw std::invalid_argument("null argument");
        aeon_hip::thread_pool& p = d->d->pool();
        if (worker < 0 || worker >= p.size()) throw std::invalid_argument("worker out of range");
        const auto all = p.worker_cpus();
        const auto& w  = all[worker];
        if (map_cpu) *map_cpu = worker < (int)p.affinity_map().size() ? p.affinity_map()[worker] : -1;
        for (int i = 0; i < std::min(cap, (int)w.size()); i++) cpus[i] = w[i];
        *count = (int)w.size();
    });
}

int aeon_decoder_pool_size(aeon_decoder* d, int* workers)
{
    return host_guarded([&] {
        if (!d || !workers) throw std::invalid_argument("null argument");
        *workers = d->d->pool().size();
    });
}

const char* aeon_decoder_last_error(void) { return g_host_err.c_str(); }

} // extern "C"
