// png_kernels.hip -- the PNG stage's kernels; their logic is png_inflate.hpp, shared with the
// host emulation.
//   png_inflate:  one wave (a workgroup of 64) per file.  The bit reader and the Huffman decode are
//                 wave-uniform (scalar registers, scalar branches); the code tables are built by the lanes
//                 into LDS; the window is a 32 KiB ring in LDS that matches are copied in by all lanes and
//                 that leaves for the file's scratch in 16-byte stores per lane, each lane summing its
//                 share of the Adler-32.
//   png_unfilter: one workgroup (one wave) per file over that scratch: bands of up to 64 rows staged in
//                 LDS, lane r undoing row r one pixel behind row r - 1, then the rows converted into the
//                 record four output bytes per lane.
//   png_unfilter_adam7 (the opt-in call's interlaced files): one wave per file and Adam7 pass over the
//                 pass's sub-image in that scratch: the same bands in LDS at the pass's own row size, then
//                 the pass's pixels scattered into the record -- the last pass in whole rows as above, the
//                 others a pass pixel per lane and step (its 1, 2 or 3 output bytes; a 2-byte store for a
//                 16-bit element at an even address).
// Each sets kPngCorruptBit in the stream's error word for a file it refuses; png_unfilter skips nothing
// for such a file (its scratch is the call's own memory, whatever it holds).
#include <hip/hip_runtime.h>

#include <algorithm>

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

// Grid (7, files): the wave of pass blockIdx.x of interlaced file blockIdx.y.  A pass filters against nothing
// outside itself and owns its bytes of the record, so the seven waves of a file run unordered.
__global__ __launch_bounds__(64) void png_unfilter_adam7(const PngJob* __restrict__ jobs, int lds, int32_t* error)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t png_lds[];
    if (!pngdev::unfilter_file_adam7(jobs[blockIdx.y], (int)blockIdx.x, 7, png_lds, lds)) atomicOr(error, kPngCorruptBit);
}

} // namespace

hipError_t launch_png(const PngJob* jobs, int n_plain, int unfilter_lds, int n_adam7, int adam7_lds, int32_t* error,
                      hipStream_t stream)
{
    if (n_plain + n_adam7 <= 0) return hipSuccess;
    static bool       attr_done = false; // (the attribute is the kernel's, not a context's)
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)png_unfilter, hipFuncAttributeMaxDynamicSharedMemorySize, kPngUnfilterLds);
        if (e != hipSuccess) return e;
        e = hipFuncSetAttribute((const void*)png_unfilter_adam7, hipFuncAttributeMaxDynamicSharedMemorySize, kPngUnfilterLds);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    png_inflate<<<n_plain + n_adam7, 64, 0, stream>>>(jobs, error);
    if (n_plain > 0) png_unfilter<<<n_plain, 64, unfilter_lds, stream>>>(jobs, unfilter_lds, error);
    for (int f = 0; f < n_adam7; f += 65535) // (a grid's y is 16 bits)
        png_unfilter_adam7<<<dim3(7, std::min(n_adam7 - f, 65535)), 64, adam7_lds, stream>>>(jobs + n_plain + f, adam7_lds, error);
    return hipGetLastError();
}

} // namespace aeon_hip
