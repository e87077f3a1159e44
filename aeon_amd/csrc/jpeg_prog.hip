// jpeg_prog.hip -- the scans of progressive JPEG files (SOF2; ITU T.81 G.1.2, libjpeg's jdphuff.c as cv::imdecode runs
// it under aeon's image::extractor::extract, src/etl_image.cpp:83-99) decoded on the GPU, for the files
// jpeg_host.cpp's prepare_prog lays out (aeon_hip_decode_jpeg_progressive_batch).
//
// A refinement scan's bit consumption depends on which coefficients earlier scans made non-zero, so a progressive
// scan cannot be cut into subsequences that synchronise by themselves as jpeg_huff's are.  The work is split the
// other way: one wave walks one unit -- one scan of one file, or one restart interval of it -- serially, and the
// parallelism is across units.  A scan depends only on the earlier scans that share a component and a coefficient
// with it (its level, jpeg.hpp), so the host launches jpeg_prog_scan once per level over every unit of that level
// in the window: libjpeg's ten-scan script is three launches, and a window of 512 files keeps a few thousand waves
// busy.  Inside a wave the walk is the same on every lane, and the lanes carry what is per coefficient:
//   - first scans (DC, AC): a decoded coefficient and its address go to the next lane's buffer; all 64 lanes store
//     at once when the buffer is full (no store per symbol); an EOB run advances the block index alone;
//   - DC refinement has no codes: bit i of the data is block i's, the lanes stride over the blocks;
//   - AC refinement: lane z loads zigzag coefficient z of the block (one 128-byte row), a ballot gives the block's
//     history, bit arithmetic on it gives where a symbol's run ends and how many correction bits lie on the way, the
//     bits are read as one field and every history lane picks its own by its rank (mbcnt).
// The coefficients land in the dense slots jpeg_idct reads; jpeg_prog_mask then gives every block its mask from its
// row (load, ballot).  A closing pass rather than atomic ORs from the scans: a DC-first scan stores zeros too, a
// refinement never clears a coefficient, so the mask is a function of the final row alone, and the pass reads each
// row once where the scans would issue an atomic per block per scan.
// The wave's logic is in jpeg_prog.hpp (shared with the host emulation the CPU tests run).
#include <hip/hip_runtime.h>

#include "jpeg_prog.hpp"
#include "launch.hpp"

namespace aeon_hip {

// One unit per wave, kProgWaves waves per workgroup, each with its scan's tables in LDS; no barrier after the
// tables are built, so a wave that ends early waits for nobody.
__global__ __launch_bounds__(kProgWaves * 64) void jpeg_prog_scan(const JpegProgScan* __restrict__ scans,
                                                                    const JpegProgUnit* __restrict__ units, int n_units,
                                                                    int32_t* __restrict__ error)
{
    __shared__ huff::Tables T[kProgWaves];
    const int           wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int           u    = blockIdx.x * kProgWaves + wave;
    const JpegProgUnit  U    = units[min(u, n_units - 1)]; // (a wave past the last unit builds its tables and leaves)
    const JpegProgScan& S    = scans[U.scan];
    const JpegHuffFile  none{}; // (tables_long reads its tables from T alone)
    prog::tables_codes(T[wave], S, lane, 64);
    __syncthreads();
    prog::tables_fast(T[wave], S, lane, 64);
    huff::tables_long(T[wave], none, lane, 64);
    __syncthreads();
    if (u >= n_units) return;
    prog::Wave W;
    if (!prog::walk_unit(T[wave], S, U, huff::gmem<const uint32_t>(S.data), W) && lane == 0) atomicOr(error, kJpegCorruptBit);
}

// The closing pass: one workgroup per kProgMaskBlocks blocks of a component, one wave per 64 of them; lane i keeps
// block i's ballot and the wave writes its 64 records together.
__global__ __launch_bounds__(kProgMaskBlocks) void jpeg_prog_mask(const JpegProgMask* __restrict__ jobs)
{
    const JpegProgMask J    = jobs[blockIdx.x];
    const int          lane = threadIdx.x & 63, b0 = (threadIdx.x >> 6) * 64, nb = min(64, J.count - b0);
    prog::Wave         W;
    prog::wave_start(W);
    uint64_t mine = 0;
    for (int i = 0; i < nb; i++) {
        const uint64_t m = prog::block_mask(W, huff::gmem<int16_t>(J.dvals) + (size_t)(b0 + i) * 64);
        if (lane == i) mine = m;
    }
    if (lane < nb) huff::gmem<JpegBlock>(J.blocks)[b0 + lane] = JpegBlock{mine, 0, 0};
}

hipError_t launch_jpeg_prog_scan(const JpegProgScan* scans, const JpegProgUnit* units, int n_units, int32_t* error,
                                 hipStream_t stream)
{
    if (n_units <= 0) return hipSuccess;
    hipLaunchKernelGGL(jpeg_prog_scan, dim3((n_units + kProgWaves - 1) / kProgWaves), dim3(kProgWaves * 64), 0, stream, scans,
                       units, n_units, error);
    return hipGetLastError();
}

hipError_t launch_jpeg_prog_mask(const JpegProgMask* jobs, int n_jobs, hipStream_t stream)
{
    if (n_jobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(jpeg_prog_mask, dim3(n_jobs), dim3(kProgMaskBlocks), 0, stream, jobs);
    return hipGetLastError();
}

} // namespace aeon_hip
