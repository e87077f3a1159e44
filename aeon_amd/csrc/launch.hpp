// launch.hpp -- every host-callable launcher and helper that a .hip file defines and a .cpp file calls.
// The defining .hip file and each caller include it, so the compiler holds a definition against the one
// declaration its callers see.  The argument structs are only named here (aug_job.hpp, mask16.hpp, box_job.hpp,
// rcnn_job.hpp, video_job.hpp, jpeg.hpp, png.hpp, pixmap.hpp, tiff.hpp define them).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace aeon_hip {

struct LaunchArgs;
struct RecArgs;
struct RotJob;
struct ExpandJob;
struct ResizeJob;
struct GrTap;
struct LzIn;
struct Mask16Job;
struct BoxLaunch;
struct RcnnLaunch;
struct PadRegion;
struct JpegImage;
struct JpegChunk;
struct JpegRows;
struct JpegHuffFile;
struct JpegProgScan;
struct JpegProgUnit;
struct JpegProgMask;
struct PngJob;
struct PixmapJob;
struct PixmapBand;
struct PixmapRleJob;
struct TiffJob;
struct TiffStrip;
struct TiffBand;
struct TiffTileBand;

// augment_kernels.hip
hipError_t launch_tiles(int km, int rm, bool tail, bool photo, const LaunchArgs& a, int grid, hipStream_t stream,
                        hipEvent_t start, hipEvent_t stop);
hipError_t launch_contrast_reduce(const LaunchArgs& a, int n_jobs, hipStream_t stream);
hipError_t kernel_occupancy(int km, int rm, bool tail, bool photo, const LaunchArgs& a, int* blocks);
hipError_t set_kernel_lds_limit(int bytes);
// record_kernels.hip
hipError_t launch_contrast_records(bool fast, bool split, const LaunchArgs& a, const RecArgs& r, int grid, hipStream_t stream,
                                   hipEvent_t start, hipEvent_t stop);
hipError_t contrast_records_lds_limit(int bytes);
// batch_transpose.hip
hipError_t launch_transpose(const void* src, void* dst, int64_t rows, int64_t cols, int element_size,
                            hipStream_t stream);
hipError_t launch_upload_table(const void* host_dev, void* dst, size_t bytes, hipStream_t stream);
// rotate_kernels.hip
hipError_t launch_rotate(const RotJob* jobs, int n_jobs, int max_tiles, int words, int cn, int32_t* error,
                         hipStream_t stream);
int        rot_box_words(int angle);
hipError_t launch_expand(const ExpandJob* jobs, int n_jobs, int max_pixels, hipStream_t stream);
// mask16_kernels.hip
hipError_t launch_nearest(const Mask16Job* jobs, int n_jobs, int max_h, int max_w, int max_seg_bytes, int max_slots, hipStream_t stream,
                          hipEvent_t start, hipEvent_t stop);
// resize_kernels.hip
hipError_t launch_resize_generic(const ResizeJob* jobs, const uint8_t* table, int n_jobs, int max_tiles, int TR, int CW,
                                 int NR, int xs, int amax, int cn_max, int SW, const float* lut, int bgr, int chm,
                                 int32_t* error, hipStream_t stream);
hipError_t launch_lanczos4_taps(const LzIn* in, GrTap* out, int n, hipStream_t stream);
hipError_t launch_resize_sep(int K, bool area, const ResizeJob* jobs, const uint8_t* table, int n_jobs, int max_tiles, int TR, int CW,
                             int NR, int SW, int cn, const float* lut, int bgr, int chm, int32_t* error, hipStream_t stream);
// box_kernels.hip, rcnn_kernels.hip
hipError_t launch_box_targets(const BoxLaunch& L, hipStream_t stream);
hipError_t launch_rcnn_targets(const RcnnLaunch& L, hipStream_t stream);
// video_kernels.hip
hipError_t launch_clip_pad(const PadRegion* regions, int n_regions, uint64_t max_bytes, hipStream_t stream);
// jpeg_kernels.hip (region: some record of the call is a region of its image: the region instantiations).  n_reduced
// (null but for a call with reduced-size records: the scaled instantiations): the chunks of jpeg_idct_reduced<4>,
// <2> and <1>, which follow jpeg_idct's n_chunks in `chunks`
hipError_t launch_jpeg(const JpegImage* imgs, const JpegChunk* chunks, int n_chunks, const int* n_reduced, const JpegRows* rows,
                       int n_rows, int color_lds, const JpegRows* rows4, int n_rows4, int color4_lds, bool region,
                       hipStream_t stream);
// jpeg_huff.hip
int        jpeg_huff_stage_cap(int lanes);
// region: some file of the call stores only the blocks inside its components' rectangles (jpeg_huff<LANES, true>)
hipError_t launch_jpeg_huff(const JpegHuffFile* files, int n_files, int lanes, int stage_bytes, bool region, int32_t* error,
                            hipStream_t stream);
// jpeg_prog.hip: jpeg_prog_scan over the units of one level of a call's progressive files, one wave per unit (a launch
// per level, in order), then jpeg_prog_mask over their components, one workgroup per kProgMaskBlocks blocks
hipError_t launch_jpeg_prog_scan(const JpegProgScan* scans, const JpegProgUnit* units, int n_units, int32_t* error,
                                 hipStream_t stream);
hipError_t launch_jpeg_prog_mask(const JpegProgMask* jobs, int n_jobs, hipStream_t stream);
// png_kernels.hip: png_inflate over all the jobs, one wave per file; then png_unfilter over the first n_plain, one
// wave per file, and png_unfilter_adam7 over the n_adam7 interlaced ones behind them, one wave per file and pass
hipError_t launch_png(const PngJob* jobs, int n_plain, int unfilter_lds, int n_adam7, int adam7_lds, int32_t* error,
                      hipStream_t stream);
// pixmap_kernels.hip: pixmap_convert, one workgroup per band
hipError_t launch_pixmap(const PixmapJob* jobs, const PixmapBand* bands, int n_bands, hipStream_t stream);
// ... the packed call: bmp_rle_expand, one wave per RLE file, then pixmap_convert over all bands
hipError_t launch_pixmap_packed(const PixmapRleJob* files, int n_files, const PixmapJob* jobs, const PixmapBand* bands, int n_bands,
                                int32_t* error, hipStream_t stream);
// tiff_kernels.hip: tiff_expand, one wave per compressed strip or tile, tiff_expand_large, one wave per LZW / PackBits
// strip or tile above kTiffStripCap, then tiff_convert, one workgroup per band, and
// tiff_convert_tiled, one per band of the tiled files (each launched only where its table holds work)
hipError_t launch_tiff(const TiffJob* jobs, const TiffStrip* strips, int n_strips, const TiffStrip* large, int n_large,
                       const TiffBand* bands, int n_bands, const TiffTileBand* tbands, int n_tbands, const uint32_t* tile_src, int32_t* error, hipStream_t stream);

} // namespace aeon_hip
