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
struct PngJob;
struct PixmapJob;
struct PixmapBand;
struct TiffJob;
struct TiffStrip;
struct TiffBand;

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
// jpeg_kernels.hip
hipError_t launch_jpeg(const JpegImage* imgs, const JpegChunk* chunks, int n_chunks, const JpegRows* rows, int n_rows,
                       int color_lds, const JpegRows* rows4, int n_rows4, int color4_lds, hipStream_t stream);
// jpeg_huff.hip
int        jpeg_huff_stage_cap(int lanes);
hipError_t launch_jpeg_huff(const JpegHuffFile* files, int n_files, int lanes, int stage_bytes, int32_t* error,
                            hipStream_t stream);
// png_kernels.hip: png_inflate then png_unfilter over the jobs, one wave per file each
hipError_t launch_png(const PngJob* jobs, int n_jobs, int unfilter_lds, int32_t* error, hipStream_t stream);
// pixmap_kernels.hip: pixmap_convert, one workgroup per band
hipError_t launch_pixmap(const PixmapJob* jobs, const PixmapBand* bands, int n_bands, hipStream_t stream);
// tiff_kernels.hip: tiff_expand, one wave per compressed strip, then tiff_convert, one workgroup per band
hipError_t launch_tiff(const TiffJob* jobs, const TiffStrip* strips, int n_strips, const TiffBand* bands, int n_bands, int32_t* error,
                       hipStream_t stream);

} // namespace aeon_hip
