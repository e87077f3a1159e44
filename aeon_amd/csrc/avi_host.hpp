// avi_host.hpp -- the MJPEG AVI demux of aeon's video extractor, host C++ over a (data, size) span.
//
// Restates, over untrusted bytes (every read bounds-checked, positions in 64 bits, nothing read past
// `size`):
//   MotionJpegCapture::parseRiff / readFrame   src/cap_mjpeg_decoder.cpp:97-112, 190-227
//   AviMjpegStream::parseAviWithFrameList      src/avi.cpp:291-379
//   AviMjpegStream::parseHdrlList / parseStrl  src/avi.cpp:179-217, 238-289
//   AviMjpegStream::parseIndex                 src/avi.cpp:145-177
// The frames are the idx1 entries of the first vids/MJPG stream whose chunk lies inside movi; a frame's
// bytes are those of the chunk at that position (the chunk's own size, not the index's length).  Only
// the chunk headers of the frames the caller has room for are read: aeon's extractor reads every frame
// and its transformer drops those past max_frame_count (src/etl_video.cpp:23-41, 49-74) -- the same
// output, without looking at bytes nobody uses.
// Where aeon would dereference null or read past the datum this parser refuses: see aeon_avi_frames
// (include/aeon_hip.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/aeon_hip.h"

namespace aeon_hip {

// aeon_avi_frames with the message in `err`; returns 0 or AEON_HIP_EINVAL.  No exception leaves it.
int avi_frames(const uint8_t* data, size_t size, aeon_avi_frame* frames, int cap, int* count, int* width, int* height,
               std::string& err);

} // namespace aeon_hip
