// tiff_kernels.hip -- the TIFF stage's four kernels; their logic is tiff_strips.hpp, shared with the
// host emulation.
//   tiff_expand:  one wave (a workgroup of 64) per compressed strip or tile, through the call's strip table (sorted by
//                 compressed size, largest first).  Deflate strips go through pngdev::inflate_file as they are;
//                 LZW strips through a wave-uniform MSB-first bit reader and a table of ranges of the strip's
//                 own output in LDS, every code emitted as a match copy by all lanes; PackBits strips through a
//                 wave-uniform walk of the control bytes.  The LZW / PackBits output lives in LDS and leaves for
//                 the scratch in 16-byte stores per lane.  A strip the wave refuses sets kTiffCorruptBit.
//   tiff_expand_large: one wave per LZW / PackBits strip or tile above kTiffStripCap, through the call's table of large
//                 strips (the opt-in call alone fills it).  The output goes through a 16 KiB window of LDS into the
//                 scratch, 16 bytes per lane and store; a string whose source has left the window is read back from
//                 the scratch.  LZW: up to 64 codes a step, a lane per code -- bit offsets known in advance, a ballot
//                 cuts the batch at a ClearCode / EOI / bad code, pointer doubling resolves the lengths of codes that
//                 name the batch's own entries, a wave scan places the codes, then the bytes in two passes.
//   tiff_convert: one workgroup of 256 per band of rows through the call's band table: the rows staged in LDS
//                 by aligned dword loads from the scratch (or from the file itself when it is uncompressed),
//                 16-bit samples made native, predictor 2 undone by a wave scan per row, then four output bytes
//                 per lane and step.
//   tiff_convert_tiled: one workgroup of 256 per band of a tiled file -- rows inside one row of tiles times a run
//                 of tiles across -- through the call's tiled band table: the waves stage whole tile-row segments
//                 side by side in LDS (16 bytes per lane from the scratch, realigned dwords from an uncompressed
//                 file), make each native and undo its predictor by a wave scan, then the workgroup writes the
//                 de-tiled rows as tiff_convert does, clipped at the image's edges.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "tiff.hpp"
#include "tiff_strips.hpp"

namespace aeon_hip {
namespace {

__global__ __launch_bounds__(64) void tiff_expand(const TiffJob* __restrict__ jobs, const TiffStrip* __restrict__ strips, int32_t* error)
{
    __shared__ tiffdev::ExpandMem M;
    const TiffStrip T = strips[blockIdx.x];
    if (!tiffdev::expand_strip(jobs[T.job], T, M) && threadIdx.x == 0) atomicOr(error, kTiffCorruptBit);
}

__global__ __launch_bounds__(64) void tiff_expand_large(const TiffJob* __restrict__ jobs, const TiffStrip* __restrict__ strips, int32_t* error)
{
    __shared__ tiffdev::LargeMem M;
    const TiffStrip T = strips[blockIdx.x];
    if (!tiffdev::expand_strip_large(jobs[T.job], T, M) && threadIdx.x == 0) atomicOr(error, kTiffCorruptBit);
}

__global__ __launch_bounds__(kTiffLanes) void tiff_convert(const TiffJob* __restrict__ jobs, const TiffBand* __restrict__ bands)
{
    __shared__ uint32_t                             tab[256];
    __shared__ __attribute__((aligned(16))) uint8_t band[kTiffBandBytes + 8];
    const TiffBand B = bands[blockIdx.x];
    tiffdev::convert_band(jobs[B.job], B, tab, band);
}

__global__ __launch_bounds__(kTiffLanes) void tiff_convert_tiled(const TiffJob* __restrict__ jobs, const TiffTileBand* __restrict__ bands,
                                                                 const uint32_t* __restrict__ tile_src)
{
    __shared__ uint32_t                             tab[256];
    __shared__ __attribute__((aligned(16))) uint8_t band[kTiffBandBytes];
    const TiffTileBand B = bands[blockIdx.x];
    tiffdev::convert_tiled_band(jobs[B.job], B, tile_src, tab, band);
}

} // namespace

hipError_t launch_tiff(const TiffJob* jobs, const TiffStrip* strips, int n_strips, const TiffStrip* large, int n_large,
                       const TiffBand* bands, int n_bands, const TiffTileBand* tbands, int n_tbands, const uint32_t* tile_src, int32_t* error, hipStream_t stream)
{
    if (n_strips > 0) tiff_expand<<<n_strips, 64, 0, stream>>>(jobs, strips, error);
    if (n_large > 0) tiff_expand_large<<<n_large, 64, 0, stream>>>(jobs, large, error);
    if (n_bands > 0) tiff_convert<<<n_bands, kTiffLanes, 0, stream>>>(jobs, bands);
    if (n_tbands > 0) tiff_convert_tiled<<<n_tbands, kTiffLanes, 0, stream>>>(jobs, tbands, tile_src);
    return hipGetLastError();
}

} // namespace aeon_hip
