// box_host.cpp -- boundingbox::extractor::extract (src/etl_boundingbox.cpp:64-132, 263-275) over the
// in-tree Json reader: the host half of the boundingbox / localization_ssd targets.  The metadata of a
// record is untrusted JSON text ({"object": [{"bndbox": {...}, "name": ..., "difficult": ...,
// "truncated": ...}, ...], "size": {"width", "height", "depth"}}); everything here is plain host C++
// with no HIP dependency, so the sanitizer driver (tests/sanitize/box_driver.cpp) links this file alone.
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/aeon_hip.h"
#include "box_host.hpp"
#include "json.hpp"

namespace aeon_hip {

namespace {

// nlohmann's j["key"] on an object: the value, or null when the key is absent
const Json& member(const Json& j, const char* key)
{
    static const Json null_json;
    if (!j.is_object()) throw std::invalid_argument(std::string("json: expected object holding '") + key + "'");
    return j.has(key) ? j.at(key) : null_json;
}

const Json& required(const Json& j, const char* key)
{
    const Json& v = member(j, key);
    if (v.is_null()) throw std::invalid_argument(std::string("'") + key + "' missing from metadata");
    return v;
}

int to_int(const Json& v)
{
    const double d = v.number();
    if (!(d > -2147483648.0 && d < 2147483648.0)) throw std::invalid_argument("json: number out of int range");
    return (int)d;
}

void extract_object(const Json& object, const std::unordered_map<std::string, int>& label_map, box_metadata& out)
{
    const Json& bndbox = member(object, "bndbox");
    if (bndbox.is_null()) throw std::invalid_argument("'xmax' missing from metadata");
    // aeon's order of checks (etl_boundingbox.cpp:98-117)
    const Json& xmax = required(bndbox, "xmax");
    const Json& xmin = required(bndbox, "xmin");
    const Json& ymax = required(bndbox, "ymax");
    const Json& ymin = required(bndbox, "ymin");
    const Json& name = required(object, "name");
    const Json& dj   = member(object, "difficult");
    const Json& tj   = member(object, "truncated");
    const bool  difficult = dj.is_null() ? false : dj.boolean();
    const bool  truncated = tj.is_null() ? false : tj.boolean();
    const auto  found     = label_map.find(name.str());
    if (found == label_map.end())
        throw std::invalid_argument("label '" + name.str() + "' not found in metadata label list");
    out.boxes.push_back((float)xmin.number());
    out.boxes.push_back((float)ymin.number());
    out.boxes.push_back((float)xmax.number());
    out.boxes.push_back((float)ymax.number());
    out.labels.push_back(found->second);
    out.difficult.push_back(difficult ? 1 : 0);
    out.truncated.push_back(truncated ? 1 : 0);
}

} // namespace

std::unordered_map<std::string, int> box_label_map(const std::vector<std::string>& class_names)
{
    std::unordered_map<std::string, int> m;
    for (size_t i = 0; i < class_names.size(); i++) m.insert({class_names[i], (int)i}); // the first of equal names
    return m;
}

void box_extract(const std::unordered_map<std::string, int>& label_map, const void* data, size_t size, box_metadata& out)
{
    out = box_metadata{};
    const Json j = Json::parse(size ? std::string((const char*)data, size) : std::string());
    const Json& object_list = required(j, "object");
    const Json& image_size  = required(j, "size");
    const Json& width       = required(image_size, "width");
    const Json& height      = required(image_size, "height");
    const Json& depth       = required(image_size, "depth");
    out.height = to_int(height);
    out.width  = to_int(width);
    out.depth  = to_int(depth);
    if (object_list.is_array()) {
        for (const Json& o : object_list.array()) extract_object(o, label_map, out);
    } else if (object_list.is_object()) { // nlohmann iterates an object's values
        for (const auto& kv : object_list.object()) extract_object(kv.second, label_map, out);
    } else {
        throw std::invalid_argument("json: 'object' is not a list");
    }
}

} // namespace aeon_hip

namespace {
thread_local std::string g_box_err;
}

extern "C" {

int aeon_box_extract(const char* class_names_json, const void* data, size_t size, int* width, int* height, int* depth,
                     float* boxes, int32_t* labels, int32_t* difficult, int cap, int* n_boxes)
{
    using namespace aeon_hip;
    try {
        if (!class_names_json || (!data && size) || !n_boxes) throw std::invalid_argument("null argument");
        if (cap < 0 || (cap > 0 && (!boxes || !labels || !difficult))) throw std::invalid_argument("bad box buffers");
        std::vector<std::string> names;
        const Json class_names = Json::parse(class_names_json);
        for (const Json& n : class_names.array()) names.push_back(n.str());
        box_metadata m;
        box_extract(box_label_map(names), data, size, m);
        const int n = (int)m.labels.size(), k = n < cap ? n : cap;
        if (k > 0) {
            std::memcpy(boxes, m.boxes.data(), sizeof(float) * 4 * (size_t)k);
            std::memcpy(labels, m.labels.data(), sizeof(int32_t) * (size_t)k);
            std::memcpy(difficult, m.difficult.data(), sizeof(int32_t) * (size_t)k);
        }
        if (width) *width = m.width;
        if (height) *height = m.height;
        if (depth) *depth = m.depth;
        *n_boxes = n;
        return AEON_HIP_OK;
    } catch (const std::invalid_argument& e) {
        g_box_err = e.what();
        return AEON_HIP_EINVAL;
    } catch (const std::exception& e) {
        g_box_err = e.what();
        return AEON_HIP_ERUNTIME;
    }
}

const char* aeon_box_last_error(void) { return g_box_err.c_str(); }

} // extern "C"
