// png_kernels.hip -- the PNG stage's two kernels; their logic is png_inflate.hpp, shared with the
// host emulation.
//   png_inflate:  one wave (a workgroup of 64) per file.  The bit reader and the Huffman decode are
//                 wave-uniform (scalar registers, scalar branches); the code tables are built by the lanes
//                 into LDS; the window is a 32 KiB ring in LDS that matches are copied in by all lanes and
//                 that leaves for the file's scratch in 16-byte stores per lane, each lane summing its
//                 share of the Adler-32.
//   png_unfilter: one workgroup (one wave) per file over that scratch: bands of up to 64 rows staged in
//                 LDS, lane r undoing row r one pixel behind row r - 1, then the rows converted into the
//                 record four output bytes per lane.
// Either sets kPngCorruptBit in the stream's error word for a file it refuses; png_unfilter skips nothing
// for such a file (its scratch is the call's own memory, whatever it holds).
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "png.hpp"
#include "png_inflate.hpp"

namespace aeon_hip {
namespace {

__global__ __launch_bounds__(64) void png_inflate(const PngJob* __restrict__ jobs, int32_t* error)
{
    __shared__ pngdev::InflateMem M;
    const PngJob&   J = jobs[blockIdx.x];
    pngdev::Inflate S;
    S.in   = (const PNG_GLOBAL uint32_t*)J.comp;
    S.raw  = (PNG_GLOBAL uint8_t*)J.raw;
    S.clen = PNG_UNI(J.clen), S.need = PNG_UNI(J.need);
    if (!pngdev::inflate_file(M, S) && threadIdx.x == 0) atomicOr(error, kPngCorruptBit);
}

__global__ __launch_bounds__(64) void png_unfilter(const PngJob* __restrict__ jobs, int lds, int32_t* error)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t png_lds[];
    if (!pngdev::unfilter_file(jobs[blockIdx.x], png_lds, lds)) atomicOr(error, kPngCorruptBit);
}

} // namespace

hipError_t launch_png(const PngJob* jobs, int n_jobs, int unfilter_lds, int32_t* error, hipStream_t stream)
{
    if (n_jobs <= 0) return hipSuccess;
    static bool       attr_done = false; // (the attribute is the kernel's, not a context's)
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)png_unfilter, hipFuncAttributeMaxDynamicSharedMemorySize, kPngUnfilterLds);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    png_inflate<<<n_jobs, 64, 0, stream>>>(jobs, error);
    png_unfilter<<<n_jobs, 64, unfilter_lds, stream>>>(jobs, unfilter_lds, error);
    return hipGetLastError();
}

} // namespace aeon_hip
