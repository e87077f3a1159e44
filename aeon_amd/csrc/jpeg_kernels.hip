// jpeg_kernels.hip -- GPU half of the JPEG decode stage (see jpeg.hpp), bit-exact with libjpeg's
// defaults as cv::imdecode runs them under aeon's image::extractor::extract (etl_image.cpp:83-99).
//
// jpeg_idct: eight lanes per 8x8 block.  They gather the block's non-zero coefficients (the sparse
// stream of a host-decoded file, or the dense zigzag slots of a GPU-decoded one through an LDS
// scatter), dequantised, then run jidctint.c's jpeg_idct_islow (LL&M, CONST_BITS 13, PASS1_BITS 2;
// the post-IDCT range limit of jdmaster.c, x & 1023 wrap) -- integer multiply-adds only -- a column
// each, then a row each, and each lane writes its output row of the block into the component plane
// (one 8-byte store).
// jpeg_idct_reduced<4 / 2 / 1>: the blocks of a file decoded at 1/2, 1/4, 1/8 of its size, straight to 4x4, 2x2 or
// 1x1 samples (jidctred.c): four lanes per block, or a lane per block (see there).
// jpeg_color: a workgroup per band of up to kJpegRowsPerWg output rows.  4:2:0 files with BGR output
// take color_h2v2 (8 columns of a row pair per lane, packed 16-bit upsampling); the others one lane
// per 4 output pixels of the band: each component sampled
// through jdsample.c's upsampler (h2v1 / h1v2 / h2v2 fancy triangle filters, context rows
// replicated at the edges as jdmainct.c does; box replication for the other ratios and for
// components narrower than 3 samples), then jdcolor.c ycc_rgb_convert (16-bit fixed point) and the
// BGR store of the decoded record into the augmentation stage's source arena.
// jpeg_color4: the bands of CMYK, YCCK and RGB files (JpegImage.cs), which jpeg_color never sees: up
// to four staged planes, each through its own upsampler, then jdcolor.c ycck_cmyk_convert (YCCK),
// OpenCV's CMYK -> BGR / gray (grfmt_jpeg / utils.cpp icvCvt_CMYK2BGR_8u_C4C3R, icvCvt_CMYK2Gray_8u_C4C1R)
// or, for RGB files, the channel swap / libjpeg-turbo's rgb_gray_convert.
#include <hip/hip_runtime.h>

#include "jpeg.hpp"
#include "launch.hpp"

namespace aeon_hip {

// Device memory through address-space-1 pointers: generic (flat) loads and stores count on the LDS
// counter too, so the LDS transposes and upsampling reads would wait for them.
#if defined(__HIP_DEVICE_COMPILE__)
template <typename T>
using gp = __attribute__((address_space(1))) T*;
#else
template <typename T>
using gp = T*; // (the host pass only parses the kernels)
#endif
template <typename T>
__device__ __forceinline__ gp<T> gaddr(uint64_t a)
{
    return (gp<T>)a;
}

__constant__ uint8_t kZz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// range_limit[x & 1023] of jdmaster.c (prepare_range_limit_table, with the +CENTERJSAMPLE folded in):
// the low 10 bits as a signed value s, then clamp(s + 128, 0, 255) -- v_bfe_i32 + v_med3_i32
__device__ __forceinline__ uint32_t idct_limit(int x)
{
    const int s = __builtin_amdgcn_sbfe(x, 0, 10);
    return (uint32_t)min(max(s + 128, 0), 255);
}

// One 1-D LL&M pass on 8 values (in[0..7] at stride 1), results descaled by `shift`.
template <int SHIFT, bool FINAL>
__device__ __forceinline__ void llm8(const int* in, int* out)
{
    constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633,
                  F1501 = 12299, F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
    int z2 = in[2], z3 = in[6];
    int z1   = (z2 + z3) * F0541;
    int tmp2 = z1 + z3 * -F1847, tmp3 = z1 + z2 * F0765;
    int tmp0 = (in[0] + in[4]) * 8192, tmp1 = (in[0] - in[4]) * 8192;
    int t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
    tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3, z5 = (z3 + z4) * F1175;
    tmp0 *= F0298, tmp1 *= F2053, tmp2 *= F3072, tmp3 *= F1501;
    z1 *= -F0899, z2 *= -F2562, z3 *= -F1961, z4 *= -F0390;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    out[0] = (t10 + tmp3 + R) >> SHIFT, out[7] = (t10 - tmp3 + R) >> SHIFT;
    out[1] = (t11 + tmp2 + R) >> SHIFT, out[6] = (t11 - tmp2 + R) >> SHIFT;
    out[2] = (t12 + tmp1 + R) >> SHIFT, out[5] = (t12 - tmp1 + R) >> SHIFT;
    out[3] = (t13 + tmp0 + R) >> SHIFT, out[4] = (t13 - tmp0 + R) >> SHIFT;
}

// The record's and the rectangles' geometry as a kernel instantiation reads it.  REGION false -- the kernels of a
// call whose records are all whole images -- folds it to constants (the record is the image, a rectangle its
// component's whole grid), which leaves those kernels the code, registers and time they had before regions; REGION
// true reads what the host computed (JpegImage), whole images of a mixed call included.  GEO_SCALED -- the colour
// kernels of a call with reduced-size records (no regions there) -- differs from whole in the planes' pitch alone,
// which it reads (JpegImage.pitch); the image's sizes and upsamplers are the reduced image's already.
enum : int { GEO_WHOLE = 0, GEO_REGION = 1, GEO_SCALED = 2 };
template <int MODE>
struct Geo {
    static constexpr bool REGION = MODE == GEO_REGION;
    static __device__ __forceinline__ int ox(const JpegImage& I) { return REGION ? I.ox : 0; }
    static __device__ __forceinline__ int oy(const JpegImage& I) { return REGION ? I.oy : 0; }
    static __device__ __forceinline__ int ow(const JpegImage& I) { return REGION ? I.ow : I.W; }
    static __device__ __forceinline__ int rx(const JpegImage& I, int k) { return REGION ? I.rx[k] : 0; }
    static __device__ __forceinline__ int ry(const JpegImage& I, int k) { return REGION ? I.ry[k] : 0; }
    static __device__ __forceinline__ int rw(const JpegImage& I, int k) { return REGION ? I.rw[k] : I.bw[k]; }
    static __device__ __forceinline__ int pitch(const JpegImage& I, int k) { return MODE == GEO_SCALED ? I.pitch[k] : rw(I, k) * 8; }
};

// Natural index -> zigzag index (the inverse of kZz).
__constant__ uint8_t kZzInv[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                   3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                   10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                   21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// Eight lanes per block, the eight adjacent lanes of a wave, kJpegIdctUnroll blocks per lane group
// (group g takes blocks g, g + G, ... so concurrent lanes still write neighbouring blocks): first
// every block's descriptor, then every column gather, all loads in flight together.  A host-decoded
// file (sparse stream): lane j takes column j straight from the stream (coefficient at natural
// n = r*8 + j present iff its zigzag bit is set; its value index = the set bits below it).  A
// GPU-decoded file (dense zigzag slots): lane j takes zigzag slots 8j .. 8j + 7 of the block as one
// 16-byte load, dequantises them with the zigzag-ordered table (JpegImage.qz, one 16-byte load),
// zeroes those whose mask bit is clear (the slots are not cleared between calls) and scatters them
// to their natural positions in the group's LDS slot, from which it reads column j (block by
// block).  Then per block pass 1 in registers, a transpose through the same slot (wave barriers
// only) and pass 2 on row j.  Slot stride 66 dwords: lane (g, j) reads / writes column j of row r at
// bank (2g + 8r + j) % 64 -- conflict-free per wave.
constexpr int kSlot = 66;

template <bool REGION>
__global__ __launch_bounds__(kJpegIdctLanes) void jpeg_idct(const JpegImage* __restrict__ imgs,
                                                            const JpegChunk* __restrict__ chunks)
{
    constexpr int G = kJpegIdctLanes / 8; // lane groups per workgroup
    constexpr int U = kJpegIdctUnroll;
    __shared__ int slot[G * kSlot];
    const JpegChunk  C  = chunks[blockIdx.x];
    const JpegImage& I  = imgs[C.img];
    const int        k  = C.comp;
    const int        g = threadIdx.x >> 3, j = threadIdx.x & 7;
    const gp<const JpegBlock> blocks = gaddr<const JpegBlock>(I.blocks[k]);
    const gp<const int16_t>   vals   = gaddr<const int16_t>(I.values);
    const gp<const int16_t>   dense  = gaddr<const int16_t>(I.dvals[k]);
    // Block b of the component's rectangle (rw blocks a row) is row b / rw, column b % rw of it: its plane holds
    // the rectangle alone, its record and coefficients sit at sb0 + row * sbw + column (JpegImage).  b / rw
    // through a float reciprocal: exact while rw < 512 ((b + 0.5) / rw stays 0.5 / rw from an integer, far above
    // the float error at these sizes)
    const int   rw  = Geo<REGION>::rw(I, k), sbw = I.sbw[k], sb0 = I.sb0[k];
    const float rrw = 1.0f / (float)rw;
    auto locate = [&](int b, int& row, int& col) {
        row = rw < 512 ? (int)(((float)b + 0.5f) * rrw) : b / rw;
        col = b - row * rw;
    };
    JpegBlock        B[U];
    int              src[U]; // the blocks' records and coefficient slots
#pragma unroll
    for (int u = 0; u < U; u++) {
        int row, col;
        src[u] = C.first + min(g + u * G, C.count - 1);
        if constexpr (REGION) {
            locate(src[u], row, col);
            src[u] = sb0 + row * sbw + col;
        }
        B[u] = blocks[src[u]];
    }
    int* const s0 = slot + g * kSlot; // the group's block slot
    // pass 1 inputs: column j of every block, dequantised (jidctint.c DEQUANTIZE = coef * quantval)
    int col[U][8];
    if (dense) {
        uint4 c4[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            c4[u] = *(gp<const uint4>)(dense + (size_t)src[u] * 64 + 8 * j);
        const uint4 q4 = *(gp<const uint4>)gaddr<const uint16_t>((uint64_t)&I.qz[k][8 * j]);
        int nat[8];
#pragma unroll
        for (int e = 0; e < 8; e++) nat[e] = kZz[8 * j + e];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t m8 = (uint32_t)(B[u].mask >> (8 * j)) & 0xffu;
            const uint32_t cw[4] = {c4[u].x, c4[u].y, c4[u].z, c4[u].w}, qw[4] = {q4.x, q4.y, q4.z, q4.w};
            if (u) { // the previous block's column reads are done
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int c = (int)(int16_t)(cw[e >> 1] >> (16 * (e & 1)));
                const int q = (int)((qw[e >> 1] >> (16 * (e & 1))) & 0xffff);
                s0[nat[e]] = ((m8 >> e) & 1) ? c * q : 0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int r = 0; r < 8; r++) col[u][r] = s0[r * 8 + j];
        }
    } else {
        int qv[8];
#pragma unroll
        for (int r = 0; r < 8; r++) qv[r] = I.q[k][r * 8 + j];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int z = kZzInv[r * 8 + j];
                col[u][r]   = 0;
                if ((B[u].mask >> z) & 1)
                    col[u][r] = (int)vals[B[u].val_off + __builtin_popcountll(B[u].mask & ((1ull << z) - 1))] * qv[r];
            }
    }
    int* const  s   = s0;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int bi = g + u * G;
        int       out[8], in[8];
        // pass 1: columns, descaled by CONST_BITS - PASS1_BITS
        llm8<11, false>(col[u], out);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier(); // the previous block's pass-2 reads are done
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int r = 0; r < 8; r++) s[r * 8 + j] = out[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // pass 2: row j, descaled by CONST_BITS + PASS1_BITS + 3, range limited; 8 bytes to the plane
#pragma unroll
        for (int c = 0; c < 8; c++) in[c] = s[j * 8 + c];
        llm8<18, true>(in, out);
        if (bi < C.count) {
            int by, bx;
            locate(C.first + bi, by, bx);
            const gp<uint8_t> o = gaddr<uint8_t>(I.planes[k]) + (size_t)(by * 8 + j) * (rw * 8) + bx * 8;
            const uint32_t lo = idct_limit(out[0]) | idct_limit(out[1]) << 8 | idct_limit(out[2]) << 16 |
                                idct_limit(out[3]) << 24;
            const uint32_t hi = idct_limit(out[4]) | idct_limit(out[5]) << 8 | idct_limit(out[6]) << 16 |
                                idct_limit(out[7]) << 24;
            *(gp<uint2>)o = make_uint2(lo, hi);
        }
    }
}

// ---- reduced IDCTs: a block straight to 4x4, 2x2 or 1x1 samples (jidctred.c; a file decoded at 1/2, 1/4, 1/8) ----
// jpeg_idct_reduced<N> takes the chunks of the components whose IDCT size is N (JpegImage.nk) in a call with reduced
// records; components left at 8x8 (the chroma of 4:2:0 at scale 2) stay with jpeg_idct.  Whole images only: block b
// of a chunk is block b of the component's grid (bw a row), and the plane's pitch is JpegImage.pitch.  The lane split
// follows the live data of each size, not jpeg_idct's 8 lanes: a 4x4 block has 7 live columns of 7 coefficients and
// 4 output rows -- four lanes; of a 2x2 block 25 coefficients are live and of a 1x1 block one -- a lane each, with no
// LDS and no barrier.

template <int S>
__device__ __forceinline__ int descale(int x)
{
    return (x + (1 << (S - 1))) >> S;
}

// jidctred.c's 4-point pass over in[0..3], in[5..7] (in[4] is never read), descaled by S
template <int S>
__device__ __forceinline__ void red4(const int (&in)[8], int (&out)[4])
{
    const int t0 = in[0] * 16384, t2 = in[2] * 15137 - in[6] * 6270;
    const int t10 = t0 + t2, t12 = t0 - t2;
    const int z1 = in[7], z2 = in[5], z3 = in[3], z4 = in[1];
    const int a = -z1 * 1730 + z2 * 11893 - z3 * 17799 + z4 * 8697;
    const int b = -z1 * 4176 - z2 * 4926 + z3 * 7373 + z4 * 20995;
    out[0] = descale<S>(t10 + b), out[1] = descale<S>(t12 + a), out[2] = descale<S>(t12 - a), out[3] = descale<S>(t10 - b);
}

// its 2-point pass over the values at positions 0, 1, 3, 5, 7
template <int S>
__device__ __forceinline__ void red2(int c0, int c1, int c3, int c5, int c7, int& o0, int& o1)
{
    const int t10 = c0 * 32768, t0 = -c7 * 5906 + c5 * 6967 - c3 * 10426 + c1 * 29692;
    o0 = descale<S>(t10 + t0), o1 = descale<S>(t10 - t0);
}

// block b of a grid of rw blocks a row (jpeg_idct's locate)
__device__ __forceinline__ void locate_block(int b, int rw, int& row, int& col)
{
    row = rw < 512 ? (int)(((float)b + 0.5f) / (float)rw) : b / rw;
    row -= row * rw > b ? 1 : 0; // (the quotient is not the reciprocal's: settle the last ulp)
    row += (row + 1) * rw <= b ? 1 : 0;
    col = b - row * rw;
}

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int N>
__global__ void jpeg_idct_reduced(const JpegImage* __restrict__ imgs, const JpegChunk* __restrict__ chunks);

// 4x4: four adjacent lanes per block, sixteen blocks per wave, kJpegIdct4Unroll blocks per lane group.  Lane j takes
// columns j and j + 4 (lane 0's column 4 is dead: nothing is fetched for it) -- rows 0-3 and 5-7 of each: from the
// sparse stream by the mask / popcount walk, or, for the dense zigzag slots, slots 16j .. 16j + 15 as two 16-byte
// loads, dequantised, masked and scattered to their natural places in the group's LDS slot, from which the columns
// are read.  Pass 1 gives four values per column; they cross to rows through the same slot (rows 9 dwords apart),
// lane j runs pass 2 on row j and stores its four samples as one dword.  Slot stride 68 dwords: the lanes of a wave
// (g = 0..15, j) read natural column j of row r at bank (4g + 8r + j) % 64, write workspace (r, j) at (4g + 9r + j)
// and read workspace (j, c) at (4g + 9j + c) -- each conflict-free (9 dj = 4 dg mod 64 only for dj = dg = 0).
constexpr int kSlot4 = 68;

template <>
__global__ __launch_bounds__(kJpegIdctLanes) void jpeg_idct_reduced<4>(const JpegImage* __restrict__ imgs,
                                                                       const JpegChunk* __restrict__ chunks)
{
    constexpr int G = kJpegIdctLanes / 4, U = kJpegIdct4Unroll;
    __shared__ int slot[G * kSlot4];
    const JpegChunk  C = chunks[blockIdx.x];
    const JpegImage& I = imgs[C.img];
    const int        k = C.comp, g = threadIdx.x >> 2, j = threadIdx.x & 3;
    const gp<const JpegBlock> blocks = gaddr<const JpegBlock>(I.blocks[k]);
    const gp<const int16_t>   vals   = gaddr<const int16_t>(I.values);
    const gp<const int16_t>   dense  = gaddr<const int16_t>(I.dvals[k]);
    JpegBlock B[U];
    int       src[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        src[u] = C.first + min(g + u * G, C.count - 1);
        B[u]   = blocks[src[u]];
    }
    int* const s0 = slot + g * kSlot4;
    int        col[U][2][8]; // [block][column j, j + 4][row], dequantised
    if (dense) {
        uint4 c4[U][2], q4[2];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int h = 0; h < 2; h++) c4[u][h] = *(gp<const uint4>)(dense + (size_t)src[u] * 64 + 16 * j + 8 * h);
#pragma unroll
        for (int h = 0; h < 2; h++) q4[h] = *(gp<const uint4>)gaddr<const uint16_t>((uint64_t)&I.qz[k][16 * j + 8 * h]);
        int nat[16];
#pragma unroll
        for (int e = 0; e < 16; e++) nat[e] = kZz[16 * j + e];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t m16 = (uint32_t)(B[u].mask >> (16 * j)) & 0xffffu;
            if (u) wave_sync(); // the previous block's column reads are done
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t cw[4] = {c4[u][h].x, c4[u][h].y, c4[u][h].z, c4[u][h].w};
                const uint32_t qw[4] = {q4[h].x, q4[h].y, q4[h].z, q4[h].w};
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int c = (int)(int16_t)(cw[e >> 1] >> (16 * (e & 1)));
                    const int q = (int)((qw[e >> 1] >> (16 * (e & 1))) & 0xffff);
                    s0[nat[8 * h + e]] = ((m16 >> (8 * h + e)) & 1) ? c * q : 0;
                }
            }
            wave_sync();
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int r = 0; r < 8; r++)
                    if (r != 4) col[u][h][r] = s0[r * 8 + j + 4 * h];
        }
    } else {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const bool live = h == 0 || j != 0; // (column 4)
#pragma unroll
            for (int r = 0; r < 8; r++) {
                if (r == 4) continue;
                const int n = r * 8 + j + 4 * h, z = kZzInv[n], qv = I.q[k][n];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    col[u][h][r] = 0;
                    if (live && ((B[u].mask >> z) & 1))
                        col[u][h][r] = (int)vals[B[u].val_off + __builtin_popcountll(B[u].mask & ((1ull << z) - 1))] * qv;
                }
            }
        }
    }
    const int rw = I.bw[k], pitch = I.pitch[k];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int bi = g + u * G;
        int       ws[2][4], in[8], out[4];
        // pass 1: columns, descaled by CONST_BITS - PASS1_BITS + 1
        col[u][0][4] = col[u][1][4] = 0;
        red4<12>(col[u][0], ws[0]);
        red4<12>(col[u][1], ws[1]);
        wave_sync(); // the slot's earlier reads are done
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int r = 0; r < 4; r++) s0[r * 9 + j + 4 * h] = ws[h][r];
        wave_sync();
        // pass 2: row j over workspace columns 0-3, 5-7, descaled by CONST_BITS + PASS1_BITS + 3 + 1; 4 bytes to the plane
#pragma unroll
        for (int c = 0; c < 8; c++) in[c] = c != 4 ? s0[j * 9 + c] : 0;
        red4<19>(in, out);
        if (bi < C.count) {
            int by, bx;
            locate_block(C.first + bi, rw, by, bx);
            *(gp<uint32_t>)(gaddr<uint8_t>(I.planes[k]) + (size_t)(by * 4 + j) * pitch + bx * 4) =
                idct_limit(out[0]) | idct_limit(out[1]) << 8 | idct_limit(out[2]) << 16 | idct_limit(out[3]) << 24;
        }
    }
}

// 2x2: a lane per block.  The 25 coefficients at rows and columns 0, 1, 3, 5, 7 sit in registers -- from the sparse
// stream by the mask / popcount walk, or from the dense zigzag slots, all eight 16-byte groups of which hold some of
// them (Z: their zigzag places, kZzInv[8 * L[a] + L[b]], every index a constant once unrolled) -- then five column
// passes, two row passes and a 2-byte store per output row.
template <>
__global__ __launch_bounds__(kJpegIdctLanes) void jpeg_idct_reduced<2>(const JpegImage* __restrict__ imgs,
                                                                       const JpegChunk* __restrict__ chunks)
{
    constexpr uint8_t L[5]     = {0, 1, 3, 5, 7};
    constexpr uint8_t Z[5][5]  = {{0, 1, 6, 15, 28}, {2, 4, 13, 26, 42}, {9, 11, 24, 40, 53}, {20, 22, 38, 51, 60},
                                  {35, 36, 49, 58, 63}};
    const JpegChunk  C = chunks[blockIdx.x];
    const JpegImage& I = imgs[C.img];
    const int        k = C.comp, bi = threadIdx.x;
    if (bi >= C.count) return;
    const int       src = C.first + bi;
    const JpegBlock B   = gaddr<const JpegBlock>(I.blocks[k])[src];
    const gp<const int16_t> dense = gaddr<const int16_t>(I.dvals[k]);
    int c[5][5];
    if (dense) {
        uint4 d[8];
#pragma unroll
        for (int t = 0; t < 8; t++) d[t] = *(gp<const uint4>)(dense + (size_t)src * 64 + 8 * t);
#pragma unroll
        for (int a = 0; a < 5; a++)
#pragma unroll
            for (int b = 0; b < 5; b++) {
                const int      z = Z[a][b], e = z & 7;
                const uint4    v = d[z >> 3];
                const uint32_t w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
                c[a][b] = ((B.mask >> z) & 1) ? (int)(int16_t)(w >> (16 * (e & 1))) * (int)I.qz[k][z] : 0;
            }
    } else {
        const gp<const int16_t> vals = gaddr<const int16_t>(I.values);
#pragma unroll
        for (int a = 0; a < 5; a++)
#pragma unroll
            for (int b = 0; b < 5; b++) {
                const int z = Z[a][b];
                c[a][b]     = 0;
                if ((B.mask >> z) & 1)
                    c[a][b] = (int)vals[B.val_off + __builtin_popcountll(B.mask & ((1ull << z) - 1))] * (int)I.q[k][L[a] * 8 + L[b]];
            }
    }
    int ws[2][5], out[2][2];
#pragma unroll
    for (int b = 0; b < 5; b++) red2<13>(c[0][b], c[1][b], c[2][b], c[3][b], c[4][b], ws[0][b], ws[1][b]);
#pragma unroll
    for (int r = 0; r < 2; r++) red2<20>(ws[r][0], ws[r][1], ws[r][2], ws[r][3], ws[r][4], out[r][0], out[r][1]);
    int by, bx;
    locate_block(src, I.bw[k], by, bx);
    const gp<uint8_t> o = gaddr<uint8_t>(I.planes[k]) + (size_t)(by * 2) * I.pitch[k] + bx * 2;
#pragma unroll
    for (int r = 0; r < 2; r++)
        *(gp<uint16_t>)(o + (size_t)r * I.pitch[k]) = (uint16_t)(idct_limit(out[r][0]) | idct_limit(out[r][1]) << 8);
}

// 1x1: a lane per block reads the DC alone -- the first value of the sparse stream when mask bit 0 is set, or slot 0
// of the dense block -- and the four lanes that hold four aligned neighbours of a plane row (same wave, same chunk)
// hand their bytes to the first, which stores a dword; the others store their byte.
template <>
__global__ __launch_bounds__(kJpegIdctLanes) void jpeg_idct_reduced<1>(const JpegImage* __restrict__ imgs,
                                                                       const JpegChunk* __restrict__ chunks)
{
    const JpegChunk  C = chunks[blockIdx.x];
    const JpegImage& I = imgs[C.img];
    const int        k = C.comp, bi = threadIdx.x, lane = threadIdx.x & 63;
    const int        b = C.first + min(bi, C.count - 1);
    const JpegBlock  B = gaddr<const JpegBlock>(I.blocks[k])[b];
    const gp<const int16_t> dense = gaddr<const int16_t>(I.dvals[k]);
    int dc = 0;
    if (B.mask & 1) dc = dense ? (int)dense[(size_t)b * 64] : (int)gaddr<const int16_t>(I.values)[B.val_off];
    const uint32_t v = idct_limit(descale<3>(dc * (int)I.q[k][0]));
    const int rw = I.bw[k];
    int       by, bx;
    locate_block(b, rw, by, bx);
    const int      p  = bx & 3;
    const uint32_t v1 = __shfl_down(v, 1), v2 = __shfl_down(v, 2), v3 = __shfl_down(v, 3);
    const bool quad = lane - p >= 0 && lane - p + 3 < 64 && bx - p + 3 < rw && bi - p + 3 < C.count;
    if (bi >= C.count) return;
    const gp<uint8_t> o = gaddr<uint8_t>(I.planes[k]) + (size_t)by * I.pitch[k] + bx;
    if (!quad) *o = (uint8_t)v;
    else if (p == 0) *(gp<uint32_t>)o = v | v1 << 8 | v2 << 16 | v3 << 24;
}

// The geometry of one component as the colour pass uses it: its staged plane rows [lo, lo + n) in
// LDS (pitch pw: the component's block rectangle; P is set back by the rectangle's first sample column, so that
// samples are addressed by their column in the image's plane), upsampler and the whole image's sizes.
struct CompView {
    const uint8_t* P;
    int            lo, pw, dw, dh, up, hf, vf;
};

// The plane rows [lo, hi] of component k that output rows [y0, y1]'s upsampling reads (jdsample.c's
// context rows for the triangle filters, clamped at the image edges).
template <int MODE>
__device__ __forceinline__ void comp_rows(const JpegImage& I, int k, int y0, int y1, CompView& c, int& hi)
{
    c.pw = Geo<MODE>::pitch(I, k), c.dw = I.dw[k], c.dh = I.dh[k], c.up = I.up[k], c.hf = I.hf[k], c.vf = I.vf[k];
    if (c.up == UP_H1V2 || c.up == UP_H2V2) c.lo = max((y0 >> 1) - 1, 0), hi = min((y1 >> 1) + 1, c.dh - 1);
    else if (c.up == UP_BOX) c.lo = y0 / c.vf, hi = y1 / c.vf;
    else c.lo = y0, hi = y1;
}

// Sample (x, y) of the image from a component's plane through libjpeg's upsampler.
__device__ __forceinline__ int upsampled(const CompView& c, int x, int y)
{
    auto at = [&](int cx, int cy) { return (int)c.P[(cy - c.lo) * c.pw + cx]; };
    switch (c.up) {
    case UP_FULL: return at(x, y);
    case UP_H2V1: { // h2v1_fancy_upsample
        const int i = x >> 1;
        if ((x & 1) == 0) return i == 0 ? at(0, y) : (at(i, y) * 3 + at(i - 1, y) + 1) >> 2;
        return i == c.dw - 1 ? at(i, y) : (at(i, y) * 3 + at(i + 1, y) + 2) >> 2;
    }
    case UP_H1V2: { // h1v2_fancy_upsample (libjpeg-turbo)
        const int r = y >> 1, v = y & 1;
        const int nb = v == 0 ? max(r - 1, 0) : min(r + 1, c.dh - 1);
        return (at(x, r) * 3 + at(x, nb) + (v ? 2 : 1)) >> 2;
    }
    case UP_H2V2: { // h2v2_fancy_upsample
        const int r = y >> 1, v = y & 1;
        const int nb = v == 0 ? max(r - 1, 0) : min(r + 1, c.dh - 1);
        const int i  = x >> 1;
        auto cs = [&](int ci) { return at(ci, r) * 3 + at(ci, nb); };
        const int t = cs(i);
        if ((x & 1) == 0) return i == 0 ? (t * 4 + 8) >> 4 : (t * 3 + cs(i - 1) + 8) >> 4;
        return i == c.dw - 1 ? (t * 4 + 7) >> 4 : (t * 3 + cs(i + 1) + 7) >> 4;
    }
    default: return at(x / c.hf, y / c.vf); // h2v1_upsample / h2v2_upsample / int_upsample
    }
}

// Image rows [y0, y0 + rows) of the record of image I (its columns [ox, ox + ow)) from its staged component rows cv:
// one lane per 4 consecutive pixels of the record -- one dword (gray) or three dwords (BGR) when the group is whole
// and 4-byte aligned, bytewise otherwise.  A pixel is sampled at its place in the image, so the chroma phase
// and the filters' neighbours are the whole decode's wherever the record starts.
template <int MODE>
__device__ __forceinline__ void color_rows(const JpegImage& I, const CompView* cv, int y0, int nrows)
{
    const int W = Geo<MODE>::ow(I), ox = Geo<MODE>::ox(I), cn = I.out_cn, nc = cn == 1 ? 1 : I.ncomp;
    const gp<uint8_t> out = gaddr<uint8_t>(I.out) - (size_t)Geo<MODE>::oy(I) * I.out_stride; // (row y of the image)
    const int         stride = I.out_stride;
    const int groups = (W + 3) >> 2;
    for (int q = threadIdx.x; q < groups * nrows; q += blockDim.x) {
        const int y = y0 + q / groups, x0 = (q % groups) * 4;
        uint32_t  p[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int x = ox + min(x0 + e, W - 1);
            const int Y = upsampled(cv[0], x, y);
            if (nc == 1) {
                p[e] = cn == 1 ? (uint32_t)Y : (uint32_t)Y * 0x010101u;
            } else {
                const int cb = upsampled(cv[1], x, y) - 128, cr = upsampled(cv[2], x, y) - 128;
                const int r  = Y + ((91881 * cr + 32768) >> 16);
                const int g  = Y + ((-22554 * cb + 32768 + -46802 * cr) >> 16);
                const int bl = Y + ((116130 * cb + 32768) >> 16);
                p[e] = (uint32_t)min(max(bl, 0), 255) | (uint32_t)min(max(g, 0), 255) << 8 |
                       (uint32_t)min(max(r, 0), 255) << 16;
            }
        }
        const gp<uint8_t> o = out + (size_t)y * stride + (size_t)x0 * cn;
        if (x0 + 3 < W && ((uintptr_t)o & 3) == 0) {
            if (cn == 1) {
                *(gp<uint32_t>)o = p[0] | p[1] << 8 | p[2] << 16 | p[3] << 24;
            } else {
                const gp<uint32_t> d = (gp<uint32_t>)o;
                d[0] = p[0] | p[1] << 24;
                d[1] = p[1] >> 8 | p[2] << 16;
                d[2] = p[2] >> 16 | p[3] << 8;
            }
        } else {
            for (int e = 0; e < 4 && x0 + e < W; e++)
                for (int c = 0; c < cn; c++) o[e * cn + c] = (uint8_t)(p[e] >> (8 * c));
        }
    }
}

// ---- 4:2:0 BGR fast path (luma full, both chroma h2v2_fancy_upsample) --------------------------
// A lane owns 8 output columns x0 = 8q.. of an output row pair (2r, 2r + 1), which share chroma row
// r: per chroma it takes columns i0 - 1 .. i0 + 4 (i0 = 4q) of rows r - 1, r, r + 1 as three aligned
// dwords of the LDS-staged rows (each row staged with its edge columns replicated to columns -1 and
// dw, which turns jdsample.c's edge cases (i == 0, i == dw - 1) into the general formula), forms
// the column sums 3 * row r + neighbour row as packed 16-bit pairs, and the output pairs
// (3 * colsum(i) + colsum(i -+ 1) + 8 / 7) >> 4 of h2v2_fancy_upsample the same way.  Luma comes
// straight from the plane (8-byte loads).  Bit-exact with the general path: same integer formulas.
//
// A record that is a region of the image (columns [ox, ox + ow)): the lanes' 8-column groups stay aligned to the
// record, so its stores keep their 8-byte form.  The chroma rows are staged from the record's first chroma column
// c0 = ox >> 1 on (byte-shifted on the way into LDS), so group q still reads aligned dwords at i0 = 4q, with the
// real left neighbour c0 - 1 where column -1 stands -- the image's edge rule only where the region touches the edge.
// An odd ox flips the chroma phase of every record column: color_h2v2<true> takes pixel e of a group from output
// e + 1 of the even-aligned 8 columns that start one to the left, whose ninth output (the even phase of chroma
// column i0 + 4) the staged columns i0 + 3, i0 + 4 give.  Luma off an 8-byte boundary comes as three dwords,
// byte-aligned in registers.
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
constexpr int kH2v2Pad = 8; // staged chroma row: [8 bytes: col -1 at 7][pw bytes][8 bytes: col dw]

__device__ __forceinline__ u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }

// One staged chroma row's bytes i0 - 1 .. i0 + 4 as 16-bit pairs: P0 (i0-1, i0), P1 (i0+1, i0+2),
// P2 (i0+3, i0+4), Q0 (i0, i0+1), Q1 (i0+2, i0+3); `row` is 4-byte aligned at column i0 - 4.
struct ChromaCols {
    u16x2 p0, p1, p2, q0, q1;
};
__device__ __forceinline__ ChromaCols chroma_cols(const uint8_t* row)
{
    const uint32_t* w  = (const uint32_t*)row;
    const uint32_t  d0 = w[0], d1 = w[1], d2 = w[2];
    ChromaCols      c;
    c.p0 = as_u16x2(__builtin_amdgcn_perm(d1, d0, 0x0c040c03u));
    c.p1 = as_u16x2(__builtin_amdgcn_perm(d1, d1, 0x0c020c01u));
    c.p2 = as_u16x2(__builtin_amdgcn_perm(d2, d1, 0x0c040c03u));
    c.q0 = as_u16x2(__builtin_amdgcn_perm(d1, d1, 0x0c010c00u));
    c.q1 = as_u16x2(__builtin_amdgcn_perm(d1, d1, 0x0c030c02u));
    return c;
}

// h2v2_fancy_upsample of 8 output columns of one output row: e01 = (x0, x0 + 2), o01 = (x0 + 1,
// x0 + 3), e23 = (x0 + 4, x0 + 6), o23 = (x0 + 5, x0 + 7); `t3` = 3 * row r, `nb` the neighbour row.
struct ChromaOut {
    u16x2    e01, o01, e23, o23;
    uint32_t e4; // the even output of chroma column i0 + 4 (x0 + 8): only a record starting on an odd column reads it
};
__device__ __forceinline__ ChromaOut chroma_row(const ChromaCols& t3, const ChromaCols& nb)
{
    const u16x2 three = {3, 3}, r8 = {8, 8}, r7 = {7, 7}, four = {4, 4};
    const u16x2 sp0 = t3.p0 + nb.p0, sp1 = t3.p1 + nb.p1, sp2 = t3.p2 + nb.p2;
    const u16x2 sq0 = t3.q0 + nb.q0, sq1 = t3.q1 + nb.q1;
    ChromaOut o;
    o.e01 = (sq0 * three + sp0 + r8) >> four;
    o.o01 = (sq0 * three + sp1 + r7) >> four;
    o.e23 = (sq1 * three + sp1 + r8) >> four;
    o.o23 = (sq1 * three + sp2 + r7) >> four;
    o.e4  = ((uint32_t)sp2[1] * 3 + sp2[0] + 8) >> 4;
    return o;
}

// jdcolor.c ycc_rgb_convert of one pixel, packed B | G << 8 | R << 16
__device__ __forceinline__ uint32_t ycc_bgr(int Y, int cb, int cr)
{
    cb -= 128, cr -= 128;
    const int r  = Y + ((91881 * cr + 32768) >> 16);
    const int g  = Y + ((-22554 * cb + 32768 + -46802 * cr) >> 16);
    const int bl = Y + ((116130 * cb + 32768) >> 16);
    return (uint32_t)min(max(bl, 0), 255) | (uint32_t)min(max(g, 0), 255) << 8 | (uint32_t)min(max(r, 0), 255) << 16;
}

// 8 BGR pixels of one output row to `o`: three 8-byte stores (aligned), six dwords, or bytes
__device__ __forceinline__ void store_bgr8(gp<uint8_t> o, const uint32_t (&p)[8], int n)
{
    uint32_t d[6];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        d[3 * h + 0] = p[4 * h] | p[4 * h + 1] << 24;
        d[3 * h + 1] = p[4 * h + 1] >> 8 | p[4 * h + 2] << 16;
        d[3 * h + 2] = p[4 * h + 2] >> 16 | p[4 * h + 3] << 8;
    }
    const uintptr_t a = (uintptr_t)o;
    if (n == 8 && (a & 7) == 0) {
        const gp<uint2> d2 = (gp<uint2>)o;
        d2[0] = make_uint2(d[0], d[1]), d2[1] = make_uint2(d[2], d[3]), d2[2] = make_uint2(d[4], d[5]);
    } else if (n == 8 && (a & 3) == 0) {
        const gp<uint32_t> d4 = (gp<uint32_t>)o;
#pragma unroll
        for (int e = 0; e < 6; e++) d4[e] = d[e];
    } else {
        for (int e = 0; e < 3 * n; e++) o[e] = (uint8_t)(d[e >> 2] >> (8 * (e & 3)));
    }
}

template <bool ODD, bool REGION>
__device__ __forceinline__ void color_h2v2(const JpegImage& I, const JpegRows& R, uint8_t* lds)
{
    using G = Geo<REGION>;
    const int y0 = R.y0, y1 = R.y0 + R.rows - 1;
    const int W = G::ow(I), groups = (W + 7) >> 3, c0 = G::ox(I) >> 1; // c0: the chroma column of the record's first pixel
    // stage chroma rows [lo, hi] of both components from column c0 - 1 on, then replicate the image's edge columns
    int lo[2], n[2], lp[2], off[2];
    int o = 0;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int k = c + 1;
        lo[c] = max((y0 >> 1) - 1, 0);
        n[c]  = min((y1 >> 1) + 1, I.dh[k] - 1) - lo[c] + 1;
        const int pw = G::rw(I, k) * 8, s = c0 - G::rx(I, k) * 8; // the rectangle's row, column c0's place in it
        lp[c] = (REGION ? max(pw, 4 * groups) : pw) + 2 * kH2v2Pad, off[c] = o;
        const gp<const uint8_t> src = gaddr<const uint8_t>(I.planes[k]) + (size_t)(lo[c] - G::ry(I, k) * 8) * pw;
        if (s == 0) { // the rows start at the image's first column: whole, 8 bytes at a time
            const int per = pw >> 3; // 8-byte words per row
            for (int e = threadIdx.x; e < n[c] * per; e += blockDim.x) {
                const int rr = e / per, w = e - rr * per;
                *(uint2*)(lds + o + rr * lp[c] + kH2v2Pad + w * 8) = ((gp<const uint2>)src)[e];
            }
        } else { // dword w of the staged row = the row's bytes s + 4w .., w from -1 (byte s - 1: column c0 - 1)
            const int pwd = pw >> 2, per = ((pw - s + 3) >> 2) + 1, a0 = (s >> 2) - 1;
            for (int e = threadIdx.x; e < n[c] * per; e += blockDim.x) {
                const int rr = e / per, w = e - rr * per;
                const gp<const uint32_t> rw = (gp<const uint32_t>)src + rr * pwd;
                const uint32_t d0 = rw[min(max(a0 + w, 0), pwd - 1)], d1 = rw[min(a0 + w + 1, pwd - 1)];
                *(uint32_t*)(lds + o + rr * lp[c] + kH2v2Pad - 4 + w * 4) = __builtin_amdgcn_alignbyte(d1, d0, (uint32_t)(s & 3));
            }
        }
        o += n[c] * lp[c];
    }
    __syncthreads();
    if (threadIdx.x < n[0] + n[1]) {
        const bool c1 = threadIdx.x >= n[0]; // (selects, not an index: the arrays stay in registers)
        const int  rr = threadIdx.x - (c1 ? n[0] : 0);
        uint8_t*   row = lds + (c1 ? off[1] + rr * lp[1] : rr * lp[0]) + kH2v2Pad;
        const int  dw  = c1 ? I.dw[2] : I.dw[1];
        // (the staged rows reach the image's last column?)
        const int  end = REGION ? (c1 ? I.rx[2] + I.rw[2] : I.rx[1] + I.rw[1]) * 8 : dw;
        if (c0 == 0) row[-1] = row[0];
        if (end >= dw) row[dw - c0] = row[dw - 1 - c0];
    }
    __syncthreads();

    const int ye = REGION ? y0 & ~1 : y0, pairs = ((y1 - ye) >> 1) + 1; // (a region's first band may start on the odd row of a pair)
    const int pw0 = G::rw(I, 0) * 8, sx = G::ox(I) - G::rx(I, 0) * 8, dh1 = I.dh[1], dh2 = I.dh[2];
    const gp<const uint8_t> Yp  = gaddr<const uint8_t>(I.planes[0]) - (size_t)G::ry(I, 0) * 8 * pw0; // (row y of the image)
    const gp<uint8_t>       out = gaddr<uint8_t>(I.out) - (size_t)G::oy(I) * I.out_stride;
    const float rcp   = 1.0f / (float)groups;
    const int   total = groups * pairs;
    // 8 luma samples of row y from the rectangle's column c on: an 8-byte load, or three dwords aligned in registers
    auto luma8 = [&](int y, int c, uint2& v) {
        const gp<const uint8_t> row = Yp + (size_t)y * pw0;
        if ((sx & 7) == 0) {
            v = *(gp<const uint2>)(row + c);
            return;
        }
        const gp<const uint32_t> w = (gp<const uint32_t>)row;
        const int      a = c >> 2, last = (pw0 >> 2) - 1;
        const uint32_t d0 = w[a], d1 = w[min(a + 1, last)], d2 = w[min(a + 2, last)];
        v = make_uint2(__builtin_amdgcn_alignbyte(d1, d0, (uint32_t)(sx & 3)),
                       __builtin_amdgcn_alignbyte(d2, d1, (uint32_t)(sx & 3)));
    };
    // the luma of the lane's next item is loaded before this one is computed
    auto luma = [&](int it, uint2& a, uint2& b) {
        const int pr = (int)(((float)it + 0.5f) * rcp), q = it - pr * groups;
        const int y = ye + 2 * pr;
        luma8(y, sx + q * 8, a);
        luma8(min(y + 1, y1), sx + q * 8, b);
    };
    uint2 na = make_uint2(0, 0), nb = make_uint2(0, 0);
    if (threadIdx.x < total) luma(threadIdx.x, na, nb);
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const uint2 ya = na, yv = nb;
        if (it + (int)blockDim.x < total) luma(it + blockDim.x, na, nb);
        const int pr = (int)(((float)it + 0.5f) * rcp), q = it - pr * groups;
        const int y = ye + 2 * pr, x0 = q * 8, i0 = q * 4, r = y >> 1;
        ChromaOut ce[2], co[2]; // [chroma]: output row y (even), y + 1 (odd)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int      dh   = c ? dh2 : dh1;
            const uint8_t* base = lds + off[c] + kH2v2Pad - 4 + i0;
            const ChromaCols m  = chroma_cols(base + (max(r - 1, 0) - lo[c]) * lp[c]);
            const ChromaCols t  = chroma_cols(base + (r - lo[c]) * lp[c]);
            const ChromaCols p  = chroma_cols(base + (min(r + 1, dh - 1) - lo[c]) * lp[c]);
            const u16x2      three = {3, 3};
            const ChromaCols t3 = {t.p0 * three, t.p1 * three, t.p2 * three, t.q0 * three, t.q1 * three};
            ce[c] = chroma_row(t3, m);
            co[c] = chroma_row(t3, p);
        }
        const int nx = min(8, W - x0);
#pragma unroll
        for (int v = 0; v < 2; v++) {
            if (y + v < y0 || y + v > y1) continue; // (the pair's row outside the band, or the record)
            const uint2 yy = v ? yv : ya;
            const ChromaOut& cb = v ? co[0] : ce[0];
            const ChromaOut& cr = v ? co[1] : ce[1];
            const u16x2 bq[4] = {cb.e01, cb.o01, cb.e23, cb.o23}, rq[4] = {cr.e01, cr.o01, cr.e23, cr.o23};
            uint32_t px[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                // pixel e is output f of the aligned 8 (f = e + 1 from an odd column): even f -> e01/e23, odd ->
                // o01/o23; pair half = (f >> 1) & 1; f = 8: e4
                const int      f  = e + (ODD ? 1 : 0);
                const int      s  = ((f & 7) >> 2) * 2 + (f & 1), h = (f >> 1) & 1;
                const uint32_t yw = e < 4 ? yy.x : yy.y;
                const int      b8 = f < 8 ? (int)bq[s][h] : (int)cb.e4, r8 = f < 8 ? (int)rq[s][h] : (int)cr.e4;
                px[e] = ycc_bgr((int)((yw >> (8 * (e & 3))) & 0xff), b8, r8);
            }
            store_bgr8(out + (size_t)(y + v) * I.out_stride + (size_t)x0 * 3, px, nx);
        }
    }
}

// A workgroup per band of output rows: the plane rows the band's upsampling reads are copied into
// LDS with coalesced 8-byte loads (jpeg_stage_rows bounds them), then color_rows.  A scaled call's files all take
// color_rows: color_h2v2 is the full-size files' (a reduced 4:2:0 file has nothing left to upsample).
template <int MODE>
__global__ __launch_bounds__(256) void jpeg_color(const JpegImage* __restrict__ imgs, const JpegRows* __restrict__ rows)
{
    constexpr bool REGION = MODE == GEO_REGION;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
    const JpegRows   R  = rows[blockIdx.x];
    const JpegImage& I  = imgs[R.img];
    if constexpr (MODE != GEO_SCALED) {
        if (I.ncomp == 3 && I.out_cn == 3 && I.up[0] == UP_FULL && I.up[1] == UP_H2V2 && I.up[2] == UP_H2V2 &&
            ((R.y0 & 1) == 0 || (REGION && R.y0 == I.oy))) { // (a region's first band ends where the even bands start)
            if (REGION && (I.ox & 1)) color_h2v2<true, REGION>(I, R, lds_b);
            else color_h2v2<false, REGION>(I, R, lds_b);
            return;
        }
    }
    const int        nc = I.out_cn == 1 ? 1 : I.ncomp;
    const int        y1 = R.y0 + R.rows - 1;
    CompView         cv[3];
    int              off = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        CompView& c = cv[k];
        int       hi;
        comp_rows<MODE>(I, k, R.y0, y1, c, hi);
        c.P = lds_b + off - Geo<MODE>::rx(I, k) * 8;
        if (k >= nc) continue;
        // stage plane rows [lo, hi]: whole rows of pw bytes (a multiple of 8) are contiguous
        const gp<const uint2> src = (gp<const uint2>)(gaddr<const uint8_t>(I.planes[k]) + (size_t)(c.lo - Geo<MODE>::ry(I, k) * 8) * c.pw);
        uint2*       dst = (uint2*)(lds_b + off);
        const int    n8  = (hi - c.lo + 1) * c.pw / 8;
        for (int e = threadIdx.x; e < n8; e += blockDim.x) dst[e] = src[e];
        off += (hi - c.lo + 1) * c.pw;
    }
    __syncthreads();
    color_rows<MODE>(I, cv, R.y0, R.rows);
}

// ---- CMYK, YCCK and RGB sources ------------------------------------------------------------------
// One pixel from its upsampled samples s0..s3 (C M Y K, Y Cb Cr K or R G B -): packed B | G << 8 |
// R << 16, or the gray value when cn == 1.
__device__ __forceinline__ uint32_t convert4(int cs, int cn, int s0, int s1, int s2, int s3)
{
    if (cs == CS_RGB) {
        // jccolor.c rgb_gray_convert: FIX(0.299), FIX(0.587), FIX(0.114) at 16 bits
        if (cn == 1) return (uint32_t)((s0 * 19595 + s1 * 38470 + s2 * 7471 + 32768) >> 16);
        return (uint32_t)s2 | (uint32_t)s1 << 8 | (uint32_t)s0 << 16;
    }
    int c = s0, m = s1, y = s2;
    if (cs == CS_YCCK) { // jdcolor.c ycck_cmyk_convert: 255 - the YCbCr path's R, G, B; K unchanged
        const int cb = s1 - 128, cr = s2 - 128;
        c = min(max(255 - (s0 + ((91881 * cr + 32768) >> 16)), 0), 255);
        m = min(max(255 - (s0 + ((-22554 * cb + 32768 + -46802 * cr) >> 16)), 0), 255);
        y = min(max(255 - (s0 + ((116130 * cb + 32768) >> 16)), 0), 255);
    }
    const int k = s3;
    c = k - (((255 - c) * k) >> 8);
    m = k - (((255 - m) * k) >> 8);
    y = k - (((255 - y) * k) >> 8);
    if (cn == 1) return (uint32_t)((y * 1868 + m * 9617 + c * 4899 + 8192) >> 14);
    return (uint32_t)y | (uint32_t)m << 8 | (uint32_t)c << 16;
}

// A workgroup per band of output rows of a CMYK, YCCK or RGB file: every component's plane rows the
// band reads staged in LDS as jpeg_color stages them (jpeg_stage_rows bounds them), then one lane per
// 4 consecutive pixels of the record with color_rows' stores, each sampled at its place in the image.
template <int MODE>
__global__ __launch_bounds__(256) void jpeg_color4(const JpegImage* __restrict__ imgs, const JpegRows* __restrict__ rows)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
    const JpegRows   R  = rows[blockIdx.x];
    const JpegImage& I  = imgs[R.img];
    const int        nc = I.ncomp, y0 = R.y0, y1 = R.y0 + R.rows - 1;
    CompView         cv[kJpegMaxComp];
    int              off = 0;
#pragma unroll
    for (int k = 0; k < kJpegMaxComp; k++) {
        CompView& c = cv[k];
        if (k >= nc) { // (an RGB file has no fourth plane: never sampled)
            c = cv[0];
            continue;
        }
        int hi;
        comp_rows<MODE>(I, k, y0, y1, c, hi);
        c.P = lds_b + off - Geo<MODE>::rx(I, k) * 8;
        const gp<const uint2> src = (gp<const uint2>)(gaddr<const uint8_t>(I.planes[k]) + (size_t)(c.lo - Geo<MODE>::ry(I, k) * 8) * c.pw);
        uint2*       dst = (uint2*)(lds_b + off);
        const int    n8  = (hi - c.lo + 1) * c.pw / 8;
        for (int e = threadIdx.x; e < n8; e += blockDim.x) dst[e] = src[e];
        off += (hi - c.lo + 1) * c.pw;
    }
    __syncthreads();
    const int W = Geo<MODE>::ow(I), ox = Geo<MODE>::ox(I), cn = I.out_cn, cs = I.cs, stride = I.out_stride;
    const gp<uint8_t> out = gaddr<uint8_t>(I.out) - (size_t)Geo<MODE>::oy(I) * stride; // (row y of the image)
    const int groups = (W + 3) >> 2;
    for (int q = threadIdx.x; q < groups * R.rows; q += blockDim.x) {
        const int y = y0 + q / groups, x0 = (q % groups) * 4;
        uint32_t  p[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int x  = ox + min(x0 + e, W - 1);
            const int s0 = upsampled(cv[0], x, y), s1 = upsampled(cv[1], x, y), s2 = upsampled(cv[2], x, y);
            const int s3 = nc == 4 ? upsampled(cv[3], x, y) : 0;
            p[e] = convert4(cs, cn, s0, s1, s2, s3);
        }
        const gp<uint8_t> o = out + (size_t)y * stride + (size_t)x0 * cn;
        if (x0 + 3 < W && ((uintptr_t)o & 3) == 0) {
            if (cn == 1) {
                *(gp<uint32_t>)o = p[0] | p[1] << 8 | p[2] << 16 | p[3] << 24;
            } else {
                const gp<uint32_t> d = (gp<uint32_t>)o;
                d[0] = p[0] | p[1] << 24;
                d[1] = p[1] >> 8 | p[2] << 16;
                d[2] = p[2] >> 16 | p[3] << 8;
            }
        } else {
            for (int e = 0; e < 4 && x0 + e < W; e++)
                for (int c = 0; c < cn; c++) o[e * cn + c] = (uint8_t)(p[e] >> (8 * c));
        }
    }
}

// A colour kernel's launch: past 64 KB of dynamic LDS the kernel's limit is raised first.
template <typename K>
static hipError_t launch_color(K kernel, const JpegImage* imgs, const JpegRows* rows, int n_rows, int lds, hipStream_t stream)
{
    if (n_rows <= 0) return hipSuccess;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(n_rows), dim3(256), (size_t)lds, stream, imgs, rows);
    return hipSuccess;
}

template <int MODE>
static hipError_t launch_jpeg_as(const JpegImage* imgs, const JpegChunk* chunks, int n_chunks, const int* n_reduced,
                                 const JpegRows* rows, int n_rows, int color_lds, const JpegRows* rows4, int n_rows4,
                                 int color4_lds, hipStream_t stream)
{
    if (n_chunks > 0)
        hipLaunchKernelGGL(jpeg_idct<MODE == GEO_REGION>, dim3(n_chunks), dim3(kJpegIdctLanes), 0, stream, imgs, chunks);
    if constexpr (MODE == GEO_SCALED) { // one launch per IDCT size present; their chunks follow the 8x8 ones
        const JpegChunk* c = chunks + n_chunks;
        if (n_reduced[0] > 0) hipLaunchKernelGGL(jpeg_idct_reduced<4>, dim3(n_reduced[0]), dim3(kJpegIdctLanes), 0, stream, imgs, c);
        c += n_reduced[0];
        if (n_reduced[1] > 0) hipLaunchKernelGGL(jpeg_idct_reduced<2>, dim3(n_reduced[1]), dim3(kJpegIdctLanes), 0, stream, imgs, c);
        c += n_reduced[1];
        if (n_reduced[2] > 0) hipLaunchKernelGGL(jpeg_idct_reduced<1>, dim3(n_reduced[2]), dim3(kJpegIdctLanes), 0, stream, imgs, c);
    }
    hipError_t e = launch_color(jpeg_color<MODE>, imgs, rows, n_rows, color_lds, stream);
    if (e == hipSuccess) e = launch_color(jpeg_color4<MODE>, imgs, rows4, n_rows4, color4_lds, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_jpeg(const JpegImage* imgs, const JpegChunk* chunks, int n_chunks, const int* n_reduced, const JpegRows* rows,
                       int n_rows, int color_lds, const JpegRows* rows4, int n_rows4, int color4_lds, bool region,
                       hipStream_t stream)
{
    if (n_reduced)
        return launch_jpeg_as<GEO_SCALED>(imgs, chunks, n_chunks, n_reduced, rows, n_rows, color_lds, rows4, n_rows4, color4_lds, stream);
    return region ? launch_jpeg_as<GEO_REGION>(imgs, chunks, n_chunks, nullptr, rows, n_rows, color_lds, rows4, n_rows4, color4_lds, stream)
                  : launch_jpeg_as<GEO_WHOLE>(imgs, chunks, n_chunks, nullptr, rows, n_rows, color_lds, rows4, n_rows4, color4_lds, stream);
}

} // namespace aeon_hip
