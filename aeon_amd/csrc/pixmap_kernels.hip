// pixmap_kernels.hip -- the pixmap stage's kernel; its logic is pixmap_rows.hpp, shared with the
// host emulation.
//   pixmap_convert: one workgroup of 256 per (file, band of rows) through the call's band table.  The band's
//                   source bytes -- a BMP's or a binary PNM's rows as they lie in the file, at any alignment --
//                   are staged in LDS with aligned dword loads; every lane then makes four consecutive output
//                   bytes of a row per step (swizzle, replicate, 16-bit byte order, bit unpack and palette
//                   lookup through the job's table in LDS, colour -> gray) and stores them as one dword where
//                   the destination is aligned.  One read and one write per byte; no error word: everything a
//                   file can be refused for is refused on the host before the launch.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "pixmap.hpp"
#include "pixmap_rows.hpp"

namespace aeon_hip {
namespace {

__global__ __launch_bounds__(kPixmapLanes) void pixmap_convert(const PixmapJob* __restrict__ jobs,
                                                               const PixmapBand* __restrict__ bands)
{
    __shared__ uint32_t                                  tab[256];
    __shared__ __attribute__((aligned(16))) uint8_t      band[kPixmapBandBytes + 8];
    const PixmapBand B = bands[blockIdx.x];
    pmdev::convert_band(jobs[B.job], B, tab, band);
}

} // namespace

hipError_t launch_pixmap(const PixmapJob* jobs, const PixmapBand* bands, int n_bands, hipStream_t stream)
{
    if (n_bands <= 0) return hipSuccess;
    pixmap_convert<<<n_bands, kPixmapLanes, 0, stream>>>(jobs, bands);
    return hipGetLastError();
}

} // namespace aeon_hip
