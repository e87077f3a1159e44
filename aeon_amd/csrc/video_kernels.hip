// video_kernels.hip -- the device code provider::video adds to the image path: the all-zero frames
// video::transformer appends to a clip shorter than max_frame_count (src/etl_video.cpp:66-71), as
// video::loader lays them out (etl_video.cpp:76-107).  The frames themselves run through the image
// path's kernels unchanged (image_path.cpp run_video: one job per frame, with the clip's plane stride).
//
// Pure stores, nothing read but the region table: HBM-write-bound.  A region starts at any byte
// alignment (an item of 3*D*H*W bytes may be odd), so its 16-byte aligned middle goes out as 16-byte
// non-temporal stores (zeros nobody reads back on the device soon: no reason to keep the lines in L2
// ahead of the frames' own) and the at most 15 bytes before and after it as byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "video_job.hpp"
#include "launch.hpp"

namespace aeon_hip {

namespace {
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4   g_u32x4;
typedef __attribute__((address_space(1))) uint8_t g_u8;
constexpr int      kPadThreads = 256;
constexpr uint64_t kPadChunk   = (uint64_t)kPadThreads * 16; // bytes one pass of a workgroup stores
constexpr int      kPadMaxGrid = 2048;                       // then the workgroups stride over the work
} // namespace

// Work item w = (region w / bpr, part w % bpr): the region's aligned middle is stored in kPadChunk
// pieces part, part + bpr, ...; part 0 also stores the unaligned head and tail.  The table lies in
// device memory, written by an earlier launch or copy on the stream (image_path.cpp run_video).
__global__ __launch_bounds__(kPadThreads) void clip_pad(const PadRegion* regions, int n_regions, int bpr)
{
    const auto     rsrc  = __builtin_amdgcn_make_buffer_rsrc((void*)regions, (short)0, n_regions * (int)sizeof(PadRegion), 0x00020000);
    const int      tid   = threadIdx.x;
    const int64_t  total = (int64_t)n_regions * bpr;
    const u32x4    zero  = {0u, 0u, 0u, 0u};
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const int      r    = (int)(w / bpr), part = (int)(w - (int64_t)r * bpr);
        const auto     v    = __builtin_amdgcn_raw_buffer_load_b128(rsrc, r * (int)sizeof(PadRegion), 0, 0);
        const uint64_t dst  = (uint64_t)v[0] | ((uint64_t)v[1] << 32);
        const uint64_t len  = (uint64_t)v[2] | ((uint64_t)v[3] << 32);
        uint64_t       head = (16 - (dst & 15)) & 15;
        if (head > len) head = len;
        const uint64_t mid  = (len - head) & ~(uint64_t)15;
        const uint64_t tail = len - head - mid; // < 16
        const uint64_t base = dst + head;       // 16-byte aligned when mid > 0
        for (uint64_t off = (uint64_t)part * kPadChunk + (uint64_t)tid * 16; off < mid; off += (uint64_t)bpr * kPadChunk)
            __builtin_nontemporal_store(zero, (g_u32x4*)(base + off));
        if (part == 0) {
            if ((uint64_t)tid < head) *(g_u8*)(dst + (uint64_t)tid) = 0;
            if (tid >= 16 && (uint64_t)(tid - 16) < tail) *(g_u8*)(base + mid + (uint64_t)(tid - 16)) = 0;
        }
    }
}

// regions: device table of n_regions entries, max_bytes: the longest region.  Memory-bound grid:
// enough workgroups that each stores a few chunks, at most kPadMaxGrid of them (they stride over the rest).
hipError_t launch_clip_pad(const PadRegion* regions, int n_regions, uint64_t max_bytes, hipStream_t stream)
{
    if (n_regions <= 0) return hipSuccess;
    const uint64_t chunks = (max_bytes + kPadChunk - 1) / kPadChunk;
    int            bpr    = (int)std::min<uint64_t>(std::max<uint64_t>(chunks / 4, 1), (uint64_t)std::max(1, kPadMaxGrid / n_regions));
    const int64_t  total  = (int64_t)n_regions * bpr;
    const int      grid   = (int)std::min<int64_t>(total, kPadMaxGrid);
    hipLaunchKernelGGL(clip_pad, dim3(grid), dim3(kPadThreads), 0, stream, regions, n_regions, bpr);
    return hipGetLastError();
}

} // namespace aeon_hip
