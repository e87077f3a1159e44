// pixmap_kernels.hip -- the pixmap stage's kernels; their logic is pixmap_rows.hpp and pixmap_rle.hpp,
// shared with the host emulation.
//   pixmap_convert: one workgroup of 256 per (file, band of rows) through the call's band table.  The band's
//                   source bytes -- a BMP's or a binary PNM's rows as they lie in the file, at any alignment --
//                   are staged in LDS with aligned dword loads; every lane then makes four consecutive output
//                   bytes of a row per step (swizzle, replicate, 16-bit byte order, bit unpack and palette
//                   lookup through the job's table in LDS, colour -> gray) and stores them as one dword where
//                   the destination is aligned.  One read and one write per byte; no error word: everything a
//                   file can be refused for is refused on the host before the launch.
//   bmp_rle_expand: one wave (a workgroup of 64) per RLE8 / RLE4 file of the packed call.  The stream goes through
//                   LDS in blocks of 4 KiB and is walked in windows of 64 sixteen-bit words, a word per lane:
//                   pointer doubling marks the token starts, a ballot cuts the window at the stream's end, wave
//                   scans of the tokens' advances place each at its (x, y), a ballot finds a token past its row or
//                   its data (kPixmapCorruptBit), and all lanes write the window's palette indices into the file's
//                   index scratch, four per lane and store where aligned.  pixmap_convert_packed then takes the
//                   scratch as an 8-bit file's rows.
//   pixmap_convert_packed: pixmap_convert with the 16-bit kinds (5-5-5, 5-6-5) in out_byte.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "pixmap.hpp"
#include "pixmap_rle.hpp"
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

// pixmap_convert with the 16-bit kinds, for the packed call: a kernel of its own, so the plain call's stays as it was
__global__ __launch_bounds__(kPixmapLanes) void pixmap_convert_packed(const PixmapJob* __restrict__ jobs,
                                                                      const PixmapBand* __restrict__ bands)
{
    __shared__ uint32_t                             tab[256];
    __shared__ __attribute__((aligned(16))) uint8_t band[kPixmapBandBytes + 8];
    const PixmapBand B = bands[blockIdx.x];
    pmdev::convert_band<true>(jobs[B.job], B, tab, band);
}

__global__ __launch_bounds__(64) void bmp_rle_expand(const PixmapRleJob* __restrict__ files, int32_t* error)
{
    __shared__ pmdev::RleMem M;
    const PixmapRleJob J = files[blockIdx.x];
    if (!pmdev::rle_expand(J, M) && threadIdx.x == 0) atomicOr(error, kPixmapCorruptBit);
}

} // namespace

hipError_t launch_pixmap(const PixmapJob* jobs, const PixmapBand* bands, int n_bands, hipStream_t stream)
{
    if (n_bands <= 0) return hipSuccess;
    pixmap_convert<<<n_bands, kPixmapLanes, 0, stream>>>(jobs, bands);
    return hipGetLastError();
}

hipError_t launch_pixmap_packed(const PixmapRleJob* files, int n_files, const PixmapJob* jobs, const PixmapBand* bands, int n_bands,
                                int32_t* error, hipStream_t stream)
{
    if (n_files > 0) bmp_rle_expand<<<n_files, 64, 0, stream>>>(files, error);
    if (n_bands > 0) pixmap_convert_packed<<<n_bands, kPixmapLanes, 0, stream>>>(jobs, bands);
    return hipGetLastError();
}

} // namespace aeon_hip
