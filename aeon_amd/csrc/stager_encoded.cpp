// stager_encoded.cpp -- the encoded half of the aeon-side drop-in: aeon_hip_stager_stage_encoded
// (include/aeon_hip.h), so that provide() hands the stager the record's file and image::extractor::extract
// (cv::imdecode on aeon's pool threads) goes away with the pixels' trip over PCIe.
//
// The entry does what the decoder's pixel_provider does per element (host.cpp: inspect, stage_record,
// stage_sources), against the public C ABI alone:
//   aeon_encoded_info      -- the sniff, the header's size and the decoder's routing rule for the file
//   device_route == 0      -- decoded here, on the calling pool thread, into the window's pinned staging
//                             (aeon_decode_png / _pixmap / _tiff): an ordinary staged record from then on
//   device_route == 1      -- the file's bytes are copied and kept; the window's launch hands them to
//                             aeon_hip_decode_{jpeg,png,pixmap,tiff}_batch on the window's stream
// stager.cpp knows the decode stages only through the hook installed here (stager_encoded.hpp).
#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/aeon_hip.h"
#include "stager_encoded.hpp"

namespace {

using aeon_hip::stager_file;

// (a window of small files holds more of them than a JPEG window of the image path: calls of that size, so the
// stages' staging sets stay at the size the decoder sizes them to -- host.cpp, stage_sources)
constexpr size_t kCallFiles = 512;

// The window's files, format by format, at most kCallFiles a call.
int decode_files(aeon_hip_ctx* ctx, const stager_file* files, size_t n, void* dst_base, void* stream)
{
    std::vector<const void*>   data;
    std::vector<size_t>        sizes;
    std::vector<int>           modes;
    std::vector<aeon_img_desc> descs;
    for (int format = 0; format < AEON_FORMAT_COUNT; format++) {
        data.clear(), sizes.clear(), modes.clear(), descs.clear();
        for (size_t i = 0; i < n; i++) {
            if (files[i].format != format) continue;
            data.push_back(files[i].data), sizes.push_back(files[i].size), modes.push_back(files[i].mode);
            descs.push_back(files[i].desc);
        }
        for (size_t f = 0; f < data.size(); f += kCallFiles) {
            const int k  = (int)std::min(kCallFiles, data.size() - f);
            int       rc = 0;
            switch (format) {
            case AEON_FORMAT_JPEG:
                rc = aeon_hip_decode_jpeg_batch(ctx, k, data.data() + f, sizes.data() + f, descs.data() + f, dst_base, stream);
                break;
            case AEON_FORMAT_PNG:
                rc = aeon_hip_decode_png_batch(ctx, k, data.data() + f, sizes.data() + f, modes.data() + f, descs.data() + f,
                                               dst_base, stream);
                break;
            case AEON_FORMAT_PIXMAP:
                rc = aeon_hip_decode_pixmap_batch(ctx, k, data.data() + f, sizes.data() + f, modes.data() + f,
                                                  descs.data() + f, dst_base, stream);
                break;
            default:
                rc = aeon_hip_decode_tiff_batch(ctx, k, data.data() + f, sizes.data() + f, modes.data() + f, descs.data() + f,
                                                dst_base, stream);
            }
            if (rc != 0) return rc;
        }
    }
    return 0;
}

struct HostDecode {
    const void* data;
    size_t      size;
    int         format, mode, idx;
};

std::string at_idx(int idx) { return std::string(aeon_hip_last_error()) + ", at idx " + std::to_string(idx); }

// image::extractor::extract on the calling thread, into the record's pinned staging
int host_decode(void* arg, uint8_t* dst, size_t row)
{
    const HostDecode& h  = *static_cast<const HostDecode*>(arg);
    int               rc = 0;
    if (h.format == AEON_FORMAT_PNG) rc = aeon_decode_png(h.data, h.size, h.mode, dst, row, nullptr);
    else if (h.format == AEON_FORMAT_PIXMAP) rc = aeon_decode_pixmap(h.data, h.size, h.mode, dst, row, nullptr);
    else rc = aeon_decode_tiff(h.data, h.size, h.mode, dst, row, nullptr);
    if (rc != 0) aeon_hip::stager_set_error(at_idx(h.idx));
    return rc;
}

} // namespace

extern "C" int aeon_hip_stager_stage_encoded(aeon_hip_stager* s, void* batch_out, int idx, const void* data, size_t size,
                                             const aeon_aug_params* params)
try {
    if (!s || !batch_out || !params) {
        aeon_hip::stager_set_error("null argument");
        return AEON_HIP_EINVAL;
    }
    int kind = 0, out_channels = 0;
    aeon_hip::stager_describe(s, &kind, &out_channels);
    if (kind == AEON_STAGER_VIDEO) {
        aeon_hip::stager_set_error("aeon_hip_stager_stage_encoded on a video stager, which takes clips "
                                   "(aeon_hip_stager_stage_clip / _stage_frames), at idx " + std::to_string(idx));
        return AEON_HIP_EINVAL;
    }
    if (!data || size == 0) {
        aeon_hip::stager_set_error("received encoded image with size 0, at idx " + std::to_string(idx));
        return AEON_HIP_EINVAL;
    }
    aeon_hip::stager_set_decode(decode_files);
    const bool mask = kind == AEON_STAGER_MASK;
    int        format = 0, width = 0, height = 0, elem_bytes = 1, route = 0;
    if (const int rc = aeon_encoded_info(data, size, mask ? 1 : 0, &format, &width, &height, nullptr, &elem_bytes, &route)) {
        aeon_hip::stager_set_error(at_idx(idx));
        return rc;
    }
    const int mode     = mask ? AEON_DECODE_ANYDEPTH : (out_channels == 3 ? AEON_DECODE_BGR8 : AEON_DECODE_GRAY8);
    const int channels = mask ? 1 : (out_channels == 3 ? 3 : 1);
    if (!route) {
        HostDecode h{data, size, format, mode, idx};
        return aeon_hip::stager_stage_decoded(s, batch_out, idx, width, height, channels, elem_bytes, params, format,
                                              host_decode, &h);
    }
    // aeon's datum dies with provide(): the window's launch reads this copy
    std::unique_ptr<uint8_t[]> bytes(new uint8_t[size]);
    std::memcpy(bytes.get(), data, size);
    return aeon_hip::stager_stage_file(s, batch_out, idx, width, height, channels, elem_bytes, params, format, mode,
                                       std::move(bytes), size);
} catch (const std::exception& e) {
    aeon_hip::stager_set_error(e.what());
    return AEON_HIP_ERUNTIME;
}
