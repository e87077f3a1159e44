// video_job.hpp -- the table of the video call's zero-fill launch (video_kernels.hip), shared by the
// host planner (image_path.cpp) and the device.
#pragma once
#include <stdint.h>

namespace aeon_hip {

// One run of pad bytes: video::transformer appends all-zero frames up to max_frame_count
// (src/etl_video.cpp:66-71), and the loader lays a clip out channel x frame x height x width
// (etl_video.cpp:76-107), so the pad frames of one channel plane are contiguous: a short clip has three
// regions of (D - frames) * H * W bytes.  16 bytes: one load per region.
struct PadRegion {
    uint64_t dst;   // device address, any byte alignment
    uint64_t bytes; // > 0
};

} // namespace aeon_hip
