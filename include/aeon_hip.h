/* aeon_hip.h -- C ABI of the MI355X (gfx950) image-augmentation stage for aeon.
 *
 * Drop-in boundary for aeon's decode hot path
 *   batch_decoder::process (src/batch_decoder.cpp:62-71)
 *     -> provider::image::provide (src/provider.cpp:160-184)
 *        -> image::transformer::transform_single_image (src/etl_image.cpp:146-202)
 *        -> image::loader::load (src/etl_image.cpp:246-341)
 *     -> provider::pixelmask::provide (src/provider.cpp:365-393)
 *        -> pixel_mask::transformer::transform (src/etl_pixel_mask.cpp:65-92)
 * Host code keeps decode (image::extractor::extract) and seeded parameter sampling
 * (param_factory::make_params) and calls these entry points once per decode window.
 *
 * Conventions: plain C types and pointers only; every function returns 0 on success or a
 * negative AEON_HIP_E* code, with a thread-local message in aeon_hip_last_error().
 * No C++ exception crosses this boundary.  `stream` is a hipStream_t (NULL = default stream).
 * See INTEGRATION.md for the aeon-side call sites and a ctypes binding.
 */
#ifndef AEON_HIP_H
#define AEON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AEON_HIP_OK 0
#define AEON_HIP_EINVAL -1     /* invalid argument / configuration (aeon: std::invalid_argument) */
#define AEON_HIP_ERUNTIME -2   /* HIP runtime failure (aeon: std::runtime_error) */
#define AEON_HIP_EUNSUPPORTED -3 /* input this build refuses (e.g. arithmetic-coded / 12-bit / 2-component JPEG) */
#define AEON_HIP_EDEVICE -4    /* a kernel reported an inconsistency in its device error word */

/* output element types (aeon output_type -> cv type, src/typemap.hpp:43-52); the loader converts the
 * uint8 record with Mat::convertTo (saturating) and standardizes float / double outputs */
#define AEON_DTYPE_U8 0  /* uint8_t  (CV_8U) */
#define AEON_DTYPE_F32 1 /* float    (CV_32F) */
#define AEON_DTYPE_S8 2  /* int8_t, char (CV_8S) */
#define AEON_DTYPE_S16 3 /* int16_t  (CV_16S) */
#define AEON_DTYPE_U16 4 /* uint16_t (CV_16U) */
#define AEON_DTYPE_S32 5 /* int32_t, uint32_t (CV_32S) */
#define AEON_DTYPE_F64 6 /* double   (CV_64F) */
/* image outputs only, beyond aeon's output_type list: the float output rounded once (to nearest even,
 * IEEE: subnormals, +-inf past float16's 65504, signed zeros, no clamping) to a 16-bit type */
#define AEON_DTYPE_F16 7  /* float16:  IEEE binary16 */
#define AEON_DTYPE_BF16 8 /* bfloat16 */

/* resize interpolation (image::config "interpolation_method") */
#define AEON_INTERP_LINEAR 0
#define AEON_INTERP_NEAREST 1
#define AEON_INTERP_CUBIC 2    /* cv::INTER_CUBIC (a resize pre-pass, resize_kernels.hip) */
#define AEON_INTERP_AREA 3     /* cv::INTER_AREA (2x box in the tile kernel, else a pre-pass) */
#define AEON_INTERP_LANCZOS4 4 /* cv::INTER_LANCZOS4 (a resize pre-pass) */

typedef struct aeon_hip_ctx aeon_hip_ctx;
typedef struct aeon_param_factory aeon_param_factory;

/* One decoded source image, HWC uint8 (BGR for 3 channels, OpenCV imdecode layout), living in
 * device memory at src_base + offset. Replaces cv::Mat image::decoded::get_image(0). */
typedef struct aeon_img_desc {
    uint64_t offset;   /* byte offset from the src_base passed to the batch call */
    int32_t  width;    /* cols */
    int32_t  height;   /* rows */
    int32_t  stride;   /* bytes per row (>= width*channels*elem_bytes) */
    int32_t  channels; /* 1 or 3 */
    int32_t  elem_bytes; /* bytes per channel element: 1 (CV_8U; 0 means 1) or 2 (CV_16U, the
                          * ANYDEPTH pixel masks / depth maps of etl_pixel_mask.cpp:35 and
                          * etl_depthmap.cpp:35; one channel, masks only, no rotation) */
    int32_t  reserved;
} aeon_img_desc;

/* POD mirror of augment::image::params (src/augment_image.hpp:99-119): the fields the image
 * and pixel-mask transformers read.  Produced by aeon_make_params (or by aeon itself). */
typedef struct aeon_aug_params {
    int32_t crop_x, crop_y, crop_w, crop_h; /* cropbox (cv::Rect) */
    int32_t resize_short_size;              /* 0 = off */
    int32_t out_w, out_h;                   /* output_size */
    int32_t angle;                          /* rotation (degrees, image::rotate) */
    int32_t flip;                           /* horizontal flip after photometric */
    int32_t padding, pad_off_x, pad_off_y;  /* padding + padding_crop_offset */
    int32_t n_lighting;                     /* 0 or 3 */
    float   lighting[3];                    /* PCA lighting alphas */
    float   color_noise_std;                /* lighting stddev */
    float   contrast, brightness, saturation;
    int32_t hue;
    int32_t interp;                         /* AEON_INTERP_* */
    /* image::expand (src/image.cpp:276-303; make_ssd_params, src/augment_image.cpp:246-273): with
     * expand_ratio > 1 the (rotated) record is placed at (expand_x, expand_y) of a zeroed
     * expand_w x expand_h canvas before resize_short / crop; 0 or 1 = no expand */
    float   expand_ratio;
    int32_t expand_x, expand_y, expand_w, expand_h;
} aeon_aug_params;

/* image::loader configuration (src/etl_image.cpp:204-244) plus the batch-buffer geometry of
 * fixed_buffer_map (src/buffer_batch.hpp:154-188). */
typedef struct aeon_out_desc {
    int32_t  dtype;         /* AEON_DTYPE_*; F16 / BF16 for images only (no mask, depth map or
                             * fixed_aspect_ratio output: AEON_HIP_EUNSUPPORTED) */
    int32_t  channels;      /* 1 or 3 */
    int32_t  channel_major; /* 1: CHW planes, 0: HWC */
    int32_t  bgr_to_rgb;    /* swap channels 0 and 2 (3-channel only) */
    int32_t  has_mean;      /* standardize with mean/stddev (float / double / float16 / bfloat16 output only) */
    int32_t  fixed_aspect_ratio; /* image::loader m_fixed_aspect_ratio (etl_image.cpp:258-306):
                                  * each item (its whole dtype-sized byte size) is zeroed and the
                                  * record is written at the top-left of a canvas_w x canvas_h
                                  * canvas viewed as CV_8U planes, whatever the dtype, standardized
                                  * in place as uint8 when mean/stddev are set -- aeon's layout */
    double   mean[3];
    double   stddev[3];
    uint64_t item_stride;   /* bytes between consecutive items of the batch buffer */
    int32_t  canvas_w, canvas_h; /* image::config width/height (fixed_aspect_ratio only) */
} aeon_out_desc;

/* ---- context ------------------------------------------------------------------------------ */
/* Replaces the per-loader CPU decode state; one context per GPU (hipSetDevice(device)). */
int aeon_hip_ctx_create(int device, aeon_hip_ctx** out);
int aeon_hip_ctx_destroy(aeon_hip_ctx* ctx);

/* ---- hot path ----------------------------------------------------------------------------- */
/* The per-record body of provider::image::provide after extract + make_params, for n records
 * at once: transform_single_image + image::loader::load of record i into
 * out_dev + i*out->item_stride.  Asynchronous on `stream`; src/out must stay valid until the
 * stream reaches this work.  descs/params are host arrays, consumed before return.
 * src_base / out_dev are device addresses: HBM, or pinned device-mapped host memory
 * (aeon_hip_host_alloc), which the kernels then read / store over PCIe directly (zero-copy: the
 * fastest host->host path). */
int aeon_hip_augment_batch(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs,
                           const void* src_base, const aeon_aug_params* params,
                           const aeon_out_desc* out, void* out_dev, void* stream);

/* provider::pixelmask::provide after extract: crop -> NEAREST resize -> flip -> load, with the
 * SAME params as the image of the record (src/provider.cpp:378-391).  1-channel masks. */
int aeon_hip_mask_batch(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs,
                        const void* src_base, const aeon_aug_params* params,
                        const aeon_out_desc* out, void* out_dev, void* stream);

/* provider::image and provider::pixelmask of the same records in one call (provider_base::provide
 * runs both with one params set per record, src/provider.cpp:109-119, 365-393): equal to
 * aeon_hip_augment_batch(descs, src_base, params, out, out_dev) followed by
 * aeon_hip_mask_batch(mask_descs, mask_src_base, params, mask_out, mask_out_dev) on `stream`.
 * When every mask is an 8-bit 1-channel record without rotation into plain uint8 items, both share
 * ONE job table (one host write, no upload launch) and run as two launches on `stream`: the image
 * tile kernel, then the masks' nearest gather reading the same table.  (A single-launch form -- the
 * masks' gather blocks taken by the image launch's workgroups after their tiles -- exists behind
 * AEON_HIP_FUSE_MASKS=1; it measured slower)  Other masks go as the two calls. */
int aeon_hip_augment_pair_batch(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs,
                                const void* src_base, const aeon_img_desc* mask_descs,
                                const void* mask_src_base, const aeon_aug_params* params,
                                const aeon_out_desc* out, void* out_dev,
                                const aeon_out_desc* mask_out, void* mask_out_dev, void* stream);

/* depthmap::extractor -> transformer -> loader (src/etl_depthmap.cpp:30-134) after extract: the
 * pixel-mask transform (rotate nearest -> crop -> NEAREST resize -> flip) and a plain
 * convert_mix_channels load (no fixed_aspect_ratio canvas).  aeon's provider_factory does not
 * construct depth maps (src/provider.cpp:43-99); this is the entry a depthmap provider calls. */
int aeon_hip_depthmap_batch(aeon_hip_ctx* ctx, int n, const aeon_img_desc* descs,
                            const void* src_base, const aeon_aug_params* params,
                            const aeon_out_desc* out, void* out_dev, void* stream);

/* batch_major=false output layout: fixed_buffer_map::copy(..., transpose=true) ->
 * transpose_buf (src/buffer_batch.cpp:186-244, 251-280; called per batch by
 * batch_iterator_fbm::filler, src/batch_iterator.cpp:125-136):
 *   dst[c * rows + r] = src[r * cols + c]
 * for a rows x cols matrix of element_size-byte elements (rows = batch size, cols = elements
 * per item).  element_size 1, 2, 4 or 8; src and dst are device buffers that must not overlap.
 * Async on `stream`. */
int aeon_hip_transpose_batch(aeon_hip_ctx* ctx, const void* src_dev, void* dst_dev, int64_t rows,
                             int64_t cols, int element_size, void* stream);

/* ---- decode (image::extractor::extract, src/etl_image.cpp:83-99) ---------------------------- */
/* JPEG frame header: width, height, component count (1 or 3).  Host only, no context needed. */
int aeon_jpeg_info(const void* data, size_t size, int* width, int* height, int* components);
/* The host half of the JPEG stage alone (headers, Huffman tables, every scan's entropy decoding into
 * the sparse coefficient stream aeon_hip_decode_jpeg_batch uploads), on the calling thread, no device:
 * the stream's block / non-zero value counts and an FNV-1a hash of it.  For robustness tests of the
 * untrusted-input parser (sanitizer builds, malformed-file corpora).  Same error codes as the batch
 * decode. */
int aeon_jpeg_entropy_decode(const void* data, size_t size, int* width, int* height, int* components,
                             int64_t* n_blocks, int64_t* n_values, uint64_t* hash);
/* The host work aeon_hip_decode_jpeg_batch does for one file, on the calling thread, no device: a
 * sequential file with one scan of every component gets its headers parsed and its entropy-coded
 * bytes unstuffed for the GPU Huffman decoder (*gpu_entropy = 1); any other (progressive,
 * multi-scan) is entropy-decoded into the sparse stream (*gpu_entropy = 0).  *staged_bytes: what it
 * stages for the H2D.  For timing the host side of the stage per file. */
int aeon_jpeg_host_stage(const void* data, size_t size, int* gpu_entropy, int64_t* staged_bytes);
/* How the host lays one file out for the GPU Huffman decoder at a workgroup of `lanes` (256, 512 or 1024), on
 * the calling thread, no device, read-only; for tests that must know which of the kernel's paths a file takes.
 * out[0..9]: GPU entropy decoding (0: the host decodes the file, the rest of the file's entries are 0), restart
 * segments, subsequences, bits per subsequence, bytes of entropy-coded data as staged (what the kernel compares
 * with aeon_hip_jpeg_huff_stage_cap), the subsequences of the largest segment; then the decoder's limits, the
 * same for every file: least and most bits per subsequence, the default workgroup size, the most data bytes a
 * workgroup copies into LDS.  A file with more subsequences than lanes takes the strided path; any other the
 * lanes path, staged when its data fits the cap.  seg_nsub (may be null with seg_cap 0) receives the
 * subsequences of the first seg_cap segments, in file order. */
int aeon_jpeg_huff_layout(const void* data, size_t size, int lanes, int32_t* out, int32_t* seg_nsub, int seg_cap);
/* The most data bytes the GPU Huffman decoder copies into LDS per file at a workgroup of `lanes`, as the
 * kernel's static LDS on the current device leaves it.  Device half: with no device it reads 0. */
int aeon_hip_jpeg_huff_stage_cap(int lanes, int* bytes);
/* The workgroup size the context's GPU Huffman decoder runs: 512, or what AEON_HIP_JPEG_HUFF_LANES (256, 512 or
 * 1024) named when the context was created. */
int aeon_hip_jpeg_huff_lanes(aeon_hip_ctx* ctx, int* lanes);
/* cv::imdecode(CV_LOAD_IMAGE_COLOR / GRAYSCALE) of n JPEG files (baseline / extended sequential /
 * progressive Huffman, 8-bit, 1, 3 or 4 components) as libjpeg decodes them (ISLOW IDCT, fancy upsampling),
 * into device memory: record i as HWC uint8 (BGR if descs[i].channels == 3, gray if 1: the Y component of a YCbCr file)
 * at dst_base + descs[i].offset with descs[i].stride bytes per row; descs[i].width/height must be
 * the file's (aeon_jpeg_info).  Headers are parsed on the context's host pool; sequential files with
 * one scan of every component are Huffman-decoded on the GPU (their unstuffed entropy-coded bytes go
 * up), the others on the pool (their sparse coefficients go up), all in one H2D; the Huffman, IDCT /
 * upsampling / colour conversion kernels run on `stream`.  Corrupt entropy-coded data of a
 * GPU-decoded file is reported by aeon_hip_synchronize (AEON_HIP_EDEVICE).  The files may be released when the call returns; dst must stay valid until the stream
 * reaches the work.  Files of one, three or four components are taken: YCbCr and gray, and CMYK /
 * YCCK / Adobe-RGB files, which decode to what cv::imdecode gives for them (libjpeg's samples through
 * OpenCV's CMYK -> BGR / gray; aeon_jpeg_info reports 4 components, the record is still 3 channels or
 * 1).  Arithmetic-coded / lossless / 12-bit / 2-component files: AEON_HIP_EUNSUPPORTED. */
int aeon_hip_decode_jpeg_batch(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes,
                               const aeon_img_desc* descs, void* dst_base, void* stream);

/* ---- video: provider::video (src/provider.cpp:477-517, src/etl_video.{hpp,cpp}) ------------------
 * aeon_avi_frames: video::extractor's demux (MotionJpegCapture, src/cap_mjpeg_decoder.cpp:132-227 over
 * AviMjpegStream, src/avi.cpp:145-379) of one MJPEG AVI datum.  The frames are the idx1 entries of the
 * first vids/MJPG stream whose chunk lies inside movi, over every AVI / AVIX list of the datum; frame k
 * is the `size` bytes at data + `offset` (the chunk's own size; size 0: an empty chunk, for which aeon
 * repeats the previous frame).  *count receives the number of frames, of which the first min(*count, cap)
 * are written to frames and are the only ones whose chunk headers are read (cap 0: the count alone);
 * *width / *height (may be NULL): the main header's dwWidth / dwHeight.  Host only, no context.
 * AEON_HIP_EINVAL, message in aeon_avi_last_error(), where aeon would dereference null or read past the
 * datum: not a RIFF AVI file; no MJPG video stream; the index flag (0x10) clear, no idx1 after movi or no
 * frame in it ("Not a valid AVI file type", aeon's message); a kept frame's chunk that runs past the
 * datum; an empty first frame. */
typedef struct aeon_avi_frame {
    uint64_t offset; /* of the chunk's data from the start of the datum */
    uint32_t size;   /* the chunk's size as written (no RIFF even-padding) */
} aeon_avi_frame;
int aeon_avi_frames(const void* data, size_t size, aeon_avi_frame* frames, int cap, int* count, int* width,
                    int* height);
const char* aeon_avi_last_error(void);

/* video::transformer + video::loader (src/etl_video.cpp:49-107) for n clips of at most max_frames (D)
 * decoded frames each: clip i's first frame_counts[i] <= D frames are descs[i*D ..] (row-major by clip;
 * the rest of a row is not read; a repeated frame is a desc with the earlier frame's offset), every one
 * through transform_single_image with params[i], written as raw uint8 planes in source channel order
 * (B, G, R), channel x frame x height x width: frame d of channel c at
 * out_dev + i*item_stride + (c*D + d)*out_h*out_w.  Frames frame_counts[i] .. D-1 of every channel are
 * zero-filled (aeon appends all-zero frames).  No bgr_to_rgb, no standardization, no type conversion: the
 * loader does none.  Frames are 3-channel; params[i].out_w / out_h must equal out_w / out_h and
 * item_stride be at least 3*D*out_h*out_w, else AEON_HIP_EINVAL.  The frames run as n*D-at-most records
 * of one aeon_hip_augment_batch-like call (every pass of it: pre-passes, contrast, the resize methods)
 * followed by one zero-fill launch when some clip is short.  Asynchronous on `stream` like the other
 * batch calls. */
int aeon_hip_video_batch(aeon_hip_ctx* ctx, int n, const int32_t* frame_counts, const aeon_img_desc* descs,
                         const void* src_base, const aeon_aug_params* params, int max_frames, int out_w, int out_h,
                         void* out_dev, uint64_t item_stride, void* stream);

/* Wait for `stream` and check the device error word of the calls made on it (each stream has its own
 * word, so a window's check never reads or clears what another stream's kernels set):
 * AEON_HIP_EDEVICE (the word cleared) when a kernel flagged an inconsistency -- an LDS footprint the host sized too small, a dynamic-tail counter
 * not reset by an earlier launch, a rotation source box over its LDS.  None is expected. */
int aeon_hip_synchronize(aeon_hip_ctx* ctx, void* stream);

/* Streams: the context records one completion event per few calls on the stream of the calls (its ring
 * slots are reused after it), so a stream the calls ran on must stay valid until aeon_hip_synchronize or
 * aeon_hip_release_stream has been called on it (or the context is destroyed).  aeon_hip_release_stream:
 * the caller is about to destroy `stream` -- the pending completion event is recorded on it now and the
 * context keeps no reference to it: the stream's device error word goes back to the context's table
 * too (there are 63; streams beyond that share the null stream's word).  The calls made on the stream
 * must be complete by then, however the caller waited for them.  Bits they set that no
 * aeon_hip_synchronize has read are discarded: the word is cleared on its next owner's stream ahead of
 * that stream's first kernel, so it reaches no other stream with a bit set and loses none the new
 * owner's kernels set.  No wait. */
int aeon_hip_release_stream(aeon_hip_ctx* ctx, void* stream);

/* ---- measurement ---------------------------------------------------------------------------- */
/* every > 0: the kernel launches of one augment/mask call in `every` -- the every-th, 2*every-th,
 * ... call after this one, so never the first launch after an idle GPU -- are bracketed by HIP
 * events on their own stream (an event pair costs GPU time between launches, so benchmarks
 * sample); 0 disables timing. */
int aeon_hip_set_timing(aeon_hip_ctx* ctx, int every);
/* Drain the timers: per kernel kind [0]=augment (final), [1]=contrast statistics,
 * [2]=pre-passes (resize_short, CUBIC / AREA / LANCZOS4 resize, 2x-area ahead of photometric),
 * [3]=JPEG IDCT + colour kernels of aeon_hip_decode_jpeg_batch (bytes: decoded pixels),
 * [4]=PNG and pixmap decode kernels (png_inflate + png_unfilter of aeon_hip_decode_png_batch, bytes: inflated
 * scanlines; pixmap_convert of aeon_hip_decode_pixmap_batch, bytes: source rows plus records): total ms,
 * total algorithmic bytes, launches.  The arrays hold `kinds` entries (AEON_HIP_TIMER_KINDS = all;
 * fewer are filled, more are left alone).  Resets the totals of every kind. */
#define AEON_HIP_TIMER_KINDS 5
int aeon_hip_kernel_times(aeon_hip_ctx* ctx, int kinds, double* ms, double* bytes, long* count);

/* ---- augmentation parameters (host) ------------------------------------------------------- */
/* augment::image::param_factory(json) (src/augment_image.cpp:28-89) from the JSON text of the
 * "augmentation" object ({"type": "image", ...}).  Validators as aeon; like aeon (which skips
 * verify_config here, src/augment_image.cpp:50) unknown keys are ignored. */
int aeon_param_factory_create(const char* aug_json, aeon_param_factory** out);
int aeon_param_factory_destroy(aeon_param_factory* f);
/* param_factory::make_params (src/augment_image.cpp:107-230) drawing from the minstd_rand0
 * engine whose state word is *engine_state (updated in place).  Calls on one factory are
 * serialised internally, but the lighting normal_distribution caches its second draw inside the
 * factory (as aeon's shared, mutable one does), so reproducible lighting needs one calling thread
 * making the calls in record order -- aeon's own deterministic order. */
int aeon_make_params(aeon_param_factory* f, uint32_t* engine_state, int in_w, int in_h,
                     int out_w, int out_h, aeon_aug_params* out);
/* param_factory::make_ssd_params (src/augment_image.cpp:232-301): make_params, then expand
 * (expand_ratio / expand_probability) and -- crop_enable false -- a patch from the configured
 * batch_samplers (sampler scale / aspect_ratio, sample_constraint jaccard / coverage bounds, max_sample,
 * max_trials; src/augment_image.cpp:303-586) as the cropbox of the expanded image.  boxes: n_boxes
 * object boxes (xmin, ymin, xmax, ymax; boundingbox::box pixel coordinates, xmax inclusive), may be
 * NULL when n_boxes is 0.  Same engine and draw order as aeon, so the same state gives aeon's params. */
int aeon_make_ssd_params(aeon_param_factory* f, uint32_t* engine_state, int in_w, int in_h, int out_w, int out_h,
                         const float* boxes, int n_boxes, aeon_aug_params* out);

/* PNG decode -- image::extractor::extract / pixel_mask::extractor::extract on PNG files
 * (src/etl_image.cpp:83-99, src/etl_pixel_mask.cpp:30-53: cv::imdecode over libpng), on the host.
 * Modes: AEON_PNG_BGR8 = CV_LOAD_IMAGE_COLOR (8-bit BGR), AEON_PNG_GRAY8 = CV_LOAD_IMAGE_GRAYSCALE,
 * AEON_PNG_ANYDEPTH = CV_LOAD_IMAGE_ANYDEPTH (gray at the file's depth: 16-bit files give native
 * uint16 samples).  aeon_png_info: size, bit depth and PNG colour type from the header.
 * aeon_decode_png writes height rows of `stride` bytes to dst and the element size (1 or 2) to
 * *elem_bytes (may be NULL). */
#define AEON_PNG_BGR8     0
#define AEON_PNG_GRAY8    1
#define AEON_PNG_ANYDEPTH 2
int aeon_png_info(const void* data, size_t size, int* width, int* height, int* bit_depth, int* color_type);
int aeon_decode_png(const void* data, size_t size, int mode, void* dst, size_t stride, int* elem_bytes);
/* The PNG stage: n PNG files decoded into device memory as aeon_decode_png(data[i], sizes[i], modes[i], ...)
 * decodes them, byte for byte: record i at dst_base + descs[i].offset with descs[i].stride bytes per row --
 * BGR8 three channels, GRAY8 one, ANYDEPTH one channel of uint8 or, for a 16-bit non-palette file, native
 * uint16; descs[i].width / height must be the file's (aeon_png_info).  The host walks the chunks (signature,
 * CRCs, IHDR, PLTE), checks the zlib header and stages the IDAT payloads; the GPU inflates them (one wave per
 * file), undoes the row filters and converts.  Interlaced files, rows wider than 16 KiB and streams of 2^31
 * bytes decode on the host and go up as pixels with the same H2D.  What aeon_decode_png refuses at parse time
 * (signature, IHDR, CRC, truncated chunk, missing PLTE, no IDAT) is refused here before any launch, same code
 * and message.  Corrupt image data of a GPU-decoded file -- a stream zlib refuses (invalid or over-subscribed
 * codes, a distance too far back, a wrong Adler-32), one that does not inflate to exactly the image's
 * scanlines, a filter byte above 4, a palette index past PLTE -- is reported by aeon_hip_synchronize
 * (AEON_HIP_EDEVICE).  Asynchronous on `stream`; the files may be released when the call returns. */
int aeon_hip_decode_png_batch(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes, const int* modes,
                              const aeon_img_desc* descs, void* dst_base, void* stream);
/* The host half of the stage for one file, on the calling thread, no device.  *gpu_route: 1 when the device
 * takes the file's inflate, 0 when it decodes on the host.  *staged_bytes: what goes into the H2D. */
int aeon_png_host_stage(const void* data, size_t size, int mode, int* gpu_route, int64_t* staged_bytes);
/* What a decoder (aeon_decoder_*) does with an encoded PNG element: *device = 1, it goes through
 * aeon_hip_decode_png_batch; 0, it is decoded on the host pool while staging.  The stage's routing rule and,
 * on top, a measured one: only files whose zlib stream is at most an eighth of their inflated scanlines
 * (pixel masks, flat and smooth images), where the device is the faster decoder.  No error: a file the chunk
 * walk refuses gives 0 (the host decoder reports it). */
int aeon_png_decoder_route(const void* data, size_t size, int* device);
/* The stage's kernels run on the calling thread, lane after lane, no device (the code the kernels compile,
 * for CPU tests and sanitizer builds): decodes like aeon_decode_png.  AEON_HIP_EUNSUPPORTED: the file is not
 * routed to the device; AEON_HIP_EDEVICE: what the device reports as corrupt. */
int aeon_png_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride);

/* Pixmap decode -- the same extractors on BMP and PNM (PBM / PGM / PPM) files, the uncompressed containers
 * cv::imdecode reads.  Modes are the PNG entries' under container-neutral names.  aeon_pixmap_info (header
 * only): size, the decoded bits per sample (16 for a PNM with maxval > 255, else 8), the file's channels (3
 * for P3 / P6 and every BMP, else 1) and *format: AEON_PIXMAP_BMP or the PNM magic's digit (1..6).
 * aeon_decode_pixmap is the complete decoder on the host: height rows of `stride` bytes to dst, the element
 * size (2: ANYDEPTH of a 16-bit PNM, native uint16; else 1) to *elem_bytes (may be NULL).  Decoded: P1..P6
 * with maxval up to 65535, BI_RGB BMP files of 1, 4, 8, 24 and 32 bits per pixel with a core (12-byte) or
 * a 40-byte-or-longer info header, bottom-up or top-down.  Refused with AEON_HIP_EUNSUPPORTED: RLE4 / RLE8
 * and 16-bit (555 / 565 / bitfields) BMP files.  Messages start with "BMP:" / "PNM:".  The decode rules, and
 * which of them no reference output pins, are DESIGN.md section 20. */
#define AEON_DECODE_BGR8     AEON_PNG_BGR8
#define AEON_DECODE_GRAY8    AEON_PNG_GRAY8
#define AEON_DECODE_ANYDEPTH AEON_PNG_ANYDEPTH
#define AEON_PIXMAP_BMP      0
int aeon_pixmap_info(const void* data, size_t size, int* width, int* height, int* bit_depth, int* channels, int* format);
int aeon_decode_pixmap(const void* data, size_t size, int mode, void* dst, size_t stride, int* elem_bytes);
/* The pixmap stage: n BMP / PNM files decoded into device memory as aeon_decode_pixmap(data[i], sizes[i],
 * modes[i], ...) decodes them, byte for byte: record i at dst_base + descs[i].offset with descs[i].stride bytes
 * per row; descs[i].width / height must be the file's (aeon_pixmap_info).  The host parses the header, builds
 * the palette / gray table and copies the file as it is into pinned staging; the GPU converts it (pixmap_convert,
 * one workgroup per file and band of rows).  The device takes binary PNM (P4, P5, P6) and uncompressed BMP
 * files below 2^31 bytes; ASCII PNM (P1, P2, P3) decodes on the host and goes up as pixels with the same H2D.
 * Whatever aeon_decode_pixmap refuses is refused here before any launch, same code and message; the stage has
 * no device error.  Asynchronous on `stream`; the files may be released when the call returns. */
int aeon_hip_decode_pixmap_batch(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes, const int* modes,
                                 const aeon_img_desc* descs, void* dst_base, void* stream);
/* The host half of the stage for one file, on the calling thread, no device.  *gpu_route: 1 when the device
 * converts the file, 0 when it decodes on the host.  *staged_bytes: the file's or the pixels' bytes in the H2D. */
int aeon_pixmap_host_stage(const void* data, size_t size, int mode, int* gpu_route, int64_t* staged_bytes);
/* The stage's kernel code run on the calling thread, lane after lane, no device (for CPU tests and sanitizer
 * builds): decodes like aeon_decode_pixmap.  AEON_HIP_EUNSUPPORTED: the file is not routed to the device. */
int aeon_pixmap_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride);

/* TIFF decode -- the same extractors on classic TIFF files in strips (first IFD, both byte orders).  Modes are
 * AEON_DECODE_*.  aeon_tiff_info: size, the file's channels (3 for RGB and palette files, else 1) and the element
 * size ANYDEPTH gives (2 for a 16-bit gray file, else 1).  aeon_decode_tiff is the complete decoder on the host:
 * height rows of `stride` bytes to dst, the element size to *elem_bytes (may be NULL).  Decoded: Compression 1,
 * 5 (LZW), 8 / 32946 (Deflate) and 32773 (PackBits); 8 or 16 bits per sample; gray (WhiteIsZero, BlackIsZero),
 * RGB and 8-bit palette files, each with at most one associated or unspecified extra sample; Predictor 1 and 2.
 * Refused with AEON_HIP_EUNSUPPORTED and a message naming the variant: BigTIFF, tiles, planar-separate files,
 * 1 / 2 / 4 / 32-bit and float samples, Predictor 3, CCITT and JPEG compression, CMYK / YCbCr / CIELab,
 * FillOrder 2, unassociated alpha, old-style LZW, more than 2^28 pixels.  A malformed file is AEON_HIP_EINVAL.
 * Messages start with "TIFF:".  The decode rules, and which of them no reference output pins, are DESIGN.md
 * section 21. */
int aeon_tiff_info(const void* data, size_t size, int* width, int* height, int* channels, int* elem_bytes);
int aeon_decode_tiff(const void* data, size_t size, int mode, void* dst, size_t stride, int* elem_bytes);
/* The TIFF stage: n files decoded into device memory as aeon_decode_tiff(data[i], sizes[i], modes[i], ...) decodes
 * them, byte for byte: record i at dst_base + descs[i].offset with descs[i].stride bytes per row; descs[i].width /
 * height must be the file's (aeon_tiff_info).  The host parses the IFD and copies the file as it is into pinned
 * staging; the GPU decodes its strips (tiff_expand, one wave per compressed strip) and converts the rows
 * (tiff_convert, one workgroup per band of rows).  The device takes a file below 2^31 bytes whose LZW / PackBits
 * strips decode to at most 32 KiB each; the others decode on the host and go up as pixels with the same H2D.
 * Whatever aeon_decode_tiff refuses from the header is refused here before any launch, same code and message;
 * corrupt strip data of a device-routed file sets the stream's device error (aeon_hip_synchronize:
 * AEON_HIP_EDEVICE).  Asynchronous on `stream`; the files may be released when the call returns. */
int aeon_hip_decode_tiff_batch(aeon_hip_ctx* ctx, int n, const void* const* data, const size_t* sizes, const int* modes,
                               const aeon_img_desc* descs, void* dst_base, void* stream);
/* The host half of the stage for one file, on the calling thread, no device.  *gpu_route: 1 when the device
 * decodes the file, 0 when it decodes on the host.  *staged_bytes: the file's or the pixels' bytes in the H2D. */
int aeon_tiff_host_stage(const void* data, size_t size, int mode, int* gpu_route, int64_t* staged_bytes);
/* What the decoder's providers do with a TIFF file: *device 1 when it goes through the stage. */
int aeon_tiff_decoder_route(const void* data, size_t size, int* device);
/* The stage's kernel code run on the calling thread, lane after lane, no device (for CPU tests and sanitizer
 * builds): decodes like aeon_decode_tiff.  AEON_HIP_EUNSUPPORTED: the file is not routed to the device;
 * AEON_HIP_EDEVICE: what the device reports as corrupt. */
int aeon_tiff_gpu_emulate(const void* data, size_t size, int mode, void* dst, size_t stride);

/* batch_sampler::sample_patches (src/augment_image.cpp:567-586) of the factory's batch_samplers[sampler]
 * over n normalized object boxes (xmin, ymin, xmax, ymax in [0, 1]) -- what aeon's tests call as
 * factory.m_batch_samplers[i].sample_patches (test/test_augmentation.cpp:347-443).  Writes up to cap
 * boxes to out (4 floats each) and the number of samples found to *n_out. */
int aeon_batch_sample_patches(aeon_param_factory* f, int sampler, uint32_t* engine_state, const float* nboxes, int n,
                              float* out, int cap, int* n_out);

/* param_factory::emit_constraint_type / emit_constraint_min_overlap (src/augment_image.cpp:86-98): the
 * factory's emit constraint as an AEON_EMIT_* code.  The type compares lower-cased as in aeon
 * ("MIN_OVERLAP" is valid); anything but "center", "min_overlap" or "" fails the factory's creation. */
#define AEON_EMIT_NONE        0
#define AEON_EMIT_CENTER      1
#define AEON_EMIT_MIN_OVERLAP 2
int aeon_param_factory_emit(aeon_param_factory* f, int* type, float* min_overlap);

/* ---- object boxes: provider::boundingbox / provider::localization::ssd targets ----------------
 * boundingbox::extractor::extract (src/etl_boundingbox.cpp:64-132): the JSON metadata of one record
 * ({"object": [{"bndbox": {"xmin", "ymin", "xmax", "ymax"}, "name", "difficult", "truncated"}, ...],
 * "size": {"width", "height", "depth"}}) -> image size and up to cap boxes (4 floats each: xmin, ymin,
 * xmax, ymax; pixel coordinates, xmax / ymax inclusive), label indices into class_names_json (a JSON
 * array of names) and difficult flags.  *n_boxes receives the full count even above cap.  Host only,
 * no context; errors (aeon's texts, e.g. "'xmax' missing from metadata", "label 'x' not found in
 * metadata label list") in aeon_box_last_error(). */
int aeon_box_extract(const char* class_names_json, const void* data, size_t size, int* width, int* height,
                     int* depth, float* boxes, int32_t* labels, int32_t* difficult, int cap, int* n_boxes);
const char* aeon_box_last_error(void);

/* boundingbox::transformer::transform_box (src/etl_boundingbox.cpp:146-261) + the loaders
 * (etl_boundingbox.cpp:296-318, etl_localization_ssd.cpp:116-150) for n records in one launch: record
 * i's boxes boxes[recs[i].first .. + recs[i].count) are expanded, tested against the emit constraint,
 * cropped, flipped and rescaled with params[i] (the params of the record's image), the survivors
 * written in input order, at most max_boxes of them, and the rest of the item zero-filled.
 *   AEON_BOX_BOUNDINGBOX: buf[0] item i = max_boxes x (xmin, ymin, xmax, ymax) floats in output pixels;
 *     the whole item (item_stride[0] bytes: aeon's shape {max_bbox_count, 4*sizeof(float)} of
 *     output_type, of which its loader writes the first max_boxes*16 bytes) is written.
 *   AEON_BOX_SSD: buf[0] image_shape (out_w, out_h) int32; buf[1] gt_boxes max_boxes x 4 floats
 *     normalized by out_w / out_h (xmin/W, ymin/H, (xmax+1)/W, (ymax+1)/H); buf[2] gt_box_count int32;
 *     buf[3] gt_class_count, buf[4] difficult_flag: max_boxes int32 each.  aeon's range check on the
 *     normalized values (normalized_box.cpp:90-107) is not made.
 * out_w / out_h: the ETL config's width / height.  The rescale itself uses params[i].out_w / out_h over
 * params[i].crop_w / crop_h, as aeon's.  emit_type / emit_min_overlap: aeon_param_factory_emit.
 * Box buffers and strides must be multiples of 16 bytes, the int32 ones of 4.  params[i].angle != 0
 * (aeon's transformer returns null there) and a box failing boundingbox::box::expand's precondition
 * (src/boundingbox.cpp:88-105) are AEON_HIP_EINVAL.  Asynchronous on `stream`; recs, boxes, labels,
 * difficult and params are host arrays, consumed before return; buf[] are device addresses. */
#define AEON_BOX_BOUNDINGBOX 0
#define AEON_BOX_SSD         1
typedef struct aeon_box_record {
    uint32_t first; /* index of the record's first box in the box table */
    int32_t  count;
} aeon_box_record;
typedef struct aeon_box_out {
    int32_t  kind, max_boxes, out_w, out_h, emit_type;
    float    emit_min_overlap;
    void*    buf[5];
    uint64_t item_stride[5]; /* boundingbox uses buf[0] only */
} aeon_box_out;
int aeon_hip_box_targets_batch(aeon_hip_ctx* ctx, int n, const aeon_box_record* recs, const float* boxes,
                               const int32_t* labels, const int32_t* difficult, const aeon_aug_params* params,
                               const aeon_box_out* out, void* stream);

/* ---- localization_rcnn: provider::localization::rcnn anchor targets ---------------------------
 * (src/etl_localization_rcnn.{hpp,cpp}, provider.cpp:222-287.)  config_json is the ETL object
 * ({"type": "localization_rcnn", "height", "width", "class_names", and optionally "name",
 * "rois_per_image" 256, "base_size" 16, "scaling_factor" 1/16, "ratios" [0.5, 1, 2], "scales" [8, 16, 32],
 * "negative_overlap" 0.3, "positive_overlap" 0.7, "foreground_fraction" 0.5, "max_gt_boxes" 64}); unknown
 * keys and fractions outside [0, 1] are AEON_HIP_EINVAL.  aeon validates nothing else; here a config that
 * yields no launchable anchors is AEON_HIP_EINVAL too (height, width, base_size, max_gt_boxes, a ratio or
 * a scale that is not positive, empty ratios / scales, a scaling_factor that is not positive and finite, an
 * empty feature grid), and one that only this build cannot take is AEON_HIP_EUNSUPPORTED (height, width or
 * max_gt_boxes above 2^24, a feature grid side above 2^24; more than 2^24 anchors at aeon_rcnn_anchors;
 * the device limits below at the device entry and the decoder).  Host only; errors in aeon_rcnn_last_error().
 *
 * aeon_rcnn_anchors: anchor::generate's table, total_anchors x (xmin, ymin, xmax, ymax) -- base
 * anchors outermost, then shift rows, then shift columns.  *n receives total_anchors; at most cap
 * anchors are written (cap 0: the count alone).
 * aeon_rcnn_config_info: the derived numbers a caller of the device entry needs, and this build's limits
 * (a config or record beyond them is AEON_HIP_EUNSUPPORTED at the device entry and the decoder).
 * aeon_rcnn_sample_anchors: transformer::sample_anchors over labels[n] (>= 1 foreground, 0 background,
 * else ignored) with the real std::shuffle over std::minstd_rand0: the engine starts from *engine_state
 * and is left at the state after the two shuffles; shuffle == 0 is aeon's debug_deterministic (no
 * draws).  out receives at most rois_per_image anchor indices, foreground first.  This is the statement
 * of aeon (and of this machine's libstdc++) that the device shuffle is tested against. */
typedef struct aeon_rcnn_info {
    int64_t total_anchors;
    int32_t rois_per_image, num_fg, max_gt_boxes, width, height;
    float   negative_overlap, positive_overlap;
    int32_t max_total_anchors, max_rois_per_image, max_boxes_per_record;
} aeon_rcnn_info;
int aeon_rcnn_anchors(const char* config_json, float* out, int cap, int* n);
int aeon_rcnn_config_info(const char* config_json, aeon_rcnn_info* info);
int aeon_rcnn_sample_anchors(const int32_t* labels, int n, int rois_per_image, int num_fg, int shuffle,
                             uint32_t* engine_state, int32_t* out, int* n_out);
const char* aeon_rcnn_last_error(void);

/* transformer::transform + sample_anchors + loader::load for n records in one launch, one workgroup per
 * record.  recs / boxes / labels / difficult / params as in aeon_hip_box_targets_batch (the same
 * refusals).  Per record: im_scale = fixed_scaling_factor when > 0, else calculate_scale over the
 * cropbox and (width, height); im_size = unbiased_round(crop_w * im_scale) x (crop_h likewise); the
 * record's boxes through transform_box (all K survivors count, only buf[5], [7], [9] stop at
 * max_gt_boxes); anchors inside im_size labelled by bbox_overlaps against negative_overlap /
 * positive_overlap and the per-box maxima (ties included); at most rois_per_image of them sampled,
 * num_fg foreground at most.  engine_states (n words, may be NULL when shuffle == 0): record i's shuffles
 * start from engine_states[i], which receives the state after them -- the call then synchronizes
 * `stream`; without engine_states it is asynchronous.  shuffle == 0 is aeon's debug_deterministic.
 *   buf[0] bbtargets, buf[1] bbtargets_mask: 4 * total_anchors float     buf[5] gt_boxes: max_gt_boxes x 4 float
 *   buf[2] labels_flat, buf[3] labels_mask: 2 * total_anchors int32      buf[6] gt_box_count: int32
 *   buf[4] image_shape: (im_w, im_h) int32                               buf[7] gt_class_count, buf[9]
 *   buf[8] image_scale: float                                            difficult_flag: max_gt_boxes int32
 * Every element of every item is written.  anchors: the host table of aeon_rcnn_anchors, uploaded when
 * it differs from the context's resident one: with anchors_key 0 the tables' contents are compared on
 * every call; a caller that gives every distinct table it uses on this context its own non-zero
 * anchors_key is believed on the key (the decoder does).  engine_states words are taken as
 * minstd_rand0::seed takes them (mod 2^31 - 1, 0 becomes 1).  total_anchors above 65536, rois_per_image above 1024
 * or a record with more than 1024 boxes: AEON_HIP_EUNSUPPORTED. */
#define AEON_BOX_RCNN 2
typedef struct aeon_rcnn_out {
    int32_t      total_anchors, max_gt_boxes, rois_per_image, num_fg, width, height, emit_type;
    float        emit_min_overlap, negative_overlap, positive_overlap, fixed_scaling_factor;
    const float* anchors;
    uint64_t     anchors_key; /* 0, or the caller's name for this table: see above */
    void*        buf[10];
    uint64_t     item_stride[10];
} aeon_rcnn_out;
int aeon_hip_rcnn_targets_batch(aeon_hip_ctx* ctx, int n, const aeon_box_record* recs, const float* boxes,
                                const int32_t* labels, const int32_t* difficult, const aeon_aug_params* params,
                                uint32_t* engine_states, int shuffle, const aeon_rcnn_out* out, void* stream);

/* batch_decoder deterministic mode (src/batch_decoder.cpp:47-54): slot engine state words. */
int aeon_seed_slots(uint32_t seed, int n, uint32_t* states);

/* Host geometry helpers make_params is built on (exported for callers that derive their own
 * cropboxes, e.g. a localization provider, and for the reference's known-answer tests):
 *   nervana::unbiased_round (src/util.cpp:212-239)
 *   image::calculate_scale (src/image.cpp:214-224)
 *   image::cropbox_max_proportional (src/image.cpp:226-237) */
int aeon_unbiased_round(float x, int64_t* out);
int aeon_calculate_scale(int width, int height, int output_width, int output_height, float* scale);
int aeon_cropbox_max_proportional(float in_w, float in_h, float out_w, float out_h, float* res_w,
                                  float* res_h);

/* ---- decode stage: provider_factory + batch_decoder (host C++ above the kernels) --------------
 * aeon_decoder = batch_decoder (src/batch_decoder.cpp:24-99) over provider_factory::create
 * (src/provider_factory.cpp:24-51) with "image" / "pixelmask" / "boundingbox" / "localization_ssd" /
 * "localization_rcnn" / "video" / "label" ETL providers.  config_json is the
 * aeon loader configuration ({"batch_size", "random_seed", "node_id", "cpu_list", "etl": [...],
 * "augmentation": [...]}, src/loader.hpp:50-109; unknown keys are rejected like verify_config).
 * Records arrive decoded (image::extractor::extract stays with the caller).
 * A provider may own several output buffers (localization_ssd: image_shape, gt_boxes, gt_box_count,
 * gt_class_count, difficult_flag): outputs[] of the decoder calls and aeon_decoder_output_count / _info
 * follow get_output_shapes() order (aeon's fixed_buffer_map order), which for "image" / "pixelmask"
 * configs is the provider order.  The element of a box provider is the record's JSON metadata, an
 * aeon_encoded_elem with width == 0 (data / size = the text): aeon_decoder_decode and
 * aeon_decoder_draw_params, whose aeon_record_elem carries no byte size, return AEON_HIP_EINVAL for a
 * config that holds a box ETL.  The first element of a record draws its (shared) params
 * (src/provider.cpp:109-119): localization_ssd make_ssd_params over the extracted boxes, boundingbox and
 * image make_params.  A window fails with AEON_HIP_EINVAL when a box provider meets params.angle != 0
 * or a box that fails boundingbox::box::expand's precondition.
 * localization_rcnn (ten buffers: bbtargets, bbtargets_mask, labels_flat, labels_mask, image_shape,
 * gt_boxes, gt_box_count, gt_class_count, image_scale, difficult_flag) draws make_params over the
 * metadata's image size; its shuffles run on the device from the record's engine after the params draw.
 * With random_seed != 0 the engines' states after the shuffles come back with the window and are the
 * slot engines of the next one, as aeon's: a later window waits for that small copy alone before it
 * draws.  With random_seed 0 each record's shuffle engine is seeded by one further draw of the window's
 * engine.
 * video (provider::video, src/provider.cpp:477-517; one buffer {3, max_frame_count, height, width} uint8, B, G, R
 * planes, channel x frame x height x width): {"type": "video", "max_frame_count" (required), "name", "frame": an
 * image config}; frame.channels other than 3 is AEON_HIP_EINVAL and a frame.output_type other than uint8_t
 * AEON_HIP_EUNSUPPORTED (aeon's loader writes three uint8 planes per frame whatever they say); the frame config's
 * other members are parsed and ignored, as aeon's loader ignores them.  Its element is the whole MJPEG AVI datum,
 * an aeon_encoded_elem with width == 0.  The param factory is built from augmentation[0]["frame"], not from
 * augmentation[0] (provider.cpp:483).  Per record: the demux (aeon_avi_frames) of the first max_frame_count frames
 * -- aeon decodes every frame and drops the later ones: the same output --, params from the first frame's size
 * unless an earlier element drew, the kept non-empty frames through the JPEG stage (at most 512 files a call),
 * then aeon_hip_video_batch.  A kept frame of another size than the first, a datum the demux refuses: AEON_HIP_EINVAL
 * naming the record; an empty datum: "received encoded video with size 0, at idx N".
 * label (provider::label, src/provider.cpp:190-216; one buffer {1} of output_type, default uint32_t):
 * {"type": "label", "binary", "name", "output_type"}; the datum is 4 bytes read as a native int (binary) or text
 * through std::stoi; the first sizeof(output_type) bytes of the int are the item.  A text that is no integer or out
 * of int's range and a binary datum that is not 4 bytes are AEON_HIP_EINVAL naming the record; an 8-byte output_type
 * (aeon copies past the int) is AEON_HIP_EUNSUPPORTED.  Host outputs are written directly, device outputs staged in
 * the window's pinned arena and copied on its stream.  The provider draws no params.  A config of label
 * elements alone has nothing for the device and is refused ("outside the HIP image stage"), as is a video element
 * without its "frame" (aeon's "missing image config in json config").
 * aeon_decoder_decode and aeon_decoder_draw_params refuse a config with a video or a label element as they refuse
 * the box ones: aeon_record_elem carries no byte size. */
typedef struct aeon_decoder aeon_decoder;

/* One decoded element of a record: HWC uint8 (BGR) pixels in host memory. */
typedef struct aeon_record_elem {
    const void* data;
    int32_t     width, height, channels;
    int32_t     stride; /* bytes per row; 0 = width*channels */
} aeon_record_elem;

int aeon_decoder_create(const char* config_json, int device, aeon_decoder** out);
int aeon_decoder_destroy(aeon_decoder* d);
/* provider_interface::get_output_shapes (src/provider_interface.hpp:61-65) */
int aeon_decoder_output_count(aeon_decoder* d, int* count);
int aeon_decoder_output_info(aeon_decoder* d, int index, char* name, size_t name_cap, int64_t* shape,
                             int* ndim, size_t* item_bytes, int* dtype);
/* One decode window: n records x input_count elements (row-major in elems).  outputs[k] holds
 * n items of output k (host memory, or device memory when outputs_on_device).  Returns when
 * the window is complete (batch_decoder::filler, src/batch_decoder.cpp:73-99). */
int aeon_decoder_decode(aeon_decoder* d, int n, const aeon_record_elem* elems, void* const* outputs,
                        int outputs_on_device, void* stream);
/* The host half of a window alone (no GPU): batch_decoder::process's make_params for n records
 * (src/batch_decoder.cpp:62-71, augment_image.cpp:107-230) with the decoder's slot engines, which
 * advance as in a real window; params[i] = record i's params.  serial = 1 draws in record order on
 * the calling thread, 0 on the decoder's pool (identical params).  Only elems' sizes are read. */
int aeon_decoder_draw_params(aeon_decoder* d, int n, const aeon_record_elem* elems, aeon_aug_params* params,
                             int serial);
/* A record element as aeon's encoded_record holds it (src/buffer_batch.hpp:45-152): an encoded
 * JPEG file (width == 0: data/size, decoded by the JPEG stage with the provider's channel count;
 * for a boundingbox / localization_ssd provider the JSON metadata text, for a video provider the AVI file,
 * for a label provider the label's bytes),
 * or -- width > 0 -- decoded HWC uint8 pixels as in aeon_record_elem (pixel masks must be). */
typedef struct aeon_encoded_elem {
    const void* data;
    size_t      size;
    int32_t     width, height, channels;
    int32_t     stride; /* decoded pixels only; 0 = width*channels */
} aeon_encoded_elem;

/* As aeon_decoder_decode, from encoded records: extract (JPEG) + transform + load per record. */
int aeon_decoder_decode_encoded(aeon_decoder* d, int n, const aeon_encoded_elem* elems, void* const* outputs,
                                int outputs_on_device, void* stream);
/* Double-buffered decode windows (async_manager's two containers, src/async_manager.hpp:91-114,
 * 162-204): submit returns once the window's input bytes are consumed (params drawn, pixels staged,
 * JPEGs entropy-decoded) with its copies and kernels queued on the decoder's own stream; at most two
 * windows are in flight, and outputs[k] must stay valid until aeon_decoder_wait returns for that
 * window (windows complete in submission order).  Host outputs should be pinned
 * (aeon_hip_host_alloc) for the D2H to overlap the next window. */
int aeon_decoder_submit(aeon_decoder* d, int n, const aeon_encoded_elem* elems, void* const* outputs,
                        int outputs_on_device);
int aeon_decoder_wait(aeon_decoder* d);
/* The decode pool's CPU pinning (thread_pool.hpp:133-138 + util.cpp:337-373).
 * aeon_thread_affinity_map: nervana::get_thread_affinity_map -- AEON_CPU_LIST, else cpu_list ("0-3,8"),
 * else hc - min(2, hc/8) CPUs: the first ones of the process's affinity mask (aeon: iota from 0, which is
 * the same list on an unrestricted host).  Writes up to cap ids, the map's length to *count.
 * aeon_decoder_pool_size / aeon_decoder_pool_cpus: the decoder's workers; for worker i, the CPU of the map
 * it was pinned to (*map_cpu, -1 = none) and the CPUs its own sched_getaffinity reported after pinning
 * (a CPU outside the process's cpuset cannot be pinned to: that worker reports the process mask). */
int aeon_thread_affinity_map(const char* cpu_list, int* cpus, int cap, int* count);
int aeon_decoder_pool_size(aeon_decoder* d, int* workers);
int aeon_decoder_pool_cpus(aeon_decoder* d, int worker, int* map_cpu, int* cpus, int cap, int* count);
const char* aeon_decoder_last_error(void);

/* manifest_file node slicing (src/manifest_file.cpp:278-295): the record indices of node
 * node_id of node_count (indices may be NULL to query *count). */
int aeon_manifest_node_slice(int64_t record_count, int batch_size, int node_id, int node_count,
                             int64_t* indices, int64_t* count);

/* ---- the aeon-side drop-in: provide() stages, post_process() flushes ---------------------------
 * What provider::image / provider::pixelmask hold.  aeon's batch_decoder::filler runs
 * provide(idx, record, out_buf) for a decode window on its pool (src/batch_decoder.cpp:62-99) and, with
 * the one-line change, post_process(out_buf) once per batch of the window; provider_base forwards
 * post_process to each ETL provider (src/provider.hpp:64-76 gains the override).
 *   aeon_hip_stager_stage (from provide(), any pool thread, concurrently): record idx of the batch whose
 *     buffer is batch_out (out_buf[name]->get_item(0): the staging key) -- its decoded pixels (HWC,
 *     copied into pinned memory before the call returns) and its augment::image::params.
 *   aeon_hip_stager_launch (from post_process(), the filler thread): the first launch after a window's
 *     stages launches the WHOLE window on the window's own stream -- one H2D per pinned staging chunk,
 *     one augment (or pixel-mask) launch over every staged record of every batch, a D2H into each batch
 *     buffer (pinned, device-mapped batch buffers are stored into directly; AEON_STAGER_DEVICE_OUT:
 *     batch_out is device memory) -- and returns without waiting; later launches of the window's other
 *     batches only mark them.  A batch must hold idx 0..n-1.
 *   aeon_hip_stager_wait (from the consumer, batch_iterator_fbm::filler, src/batch_iterator.cpp:109-142,
 *     before it swaps or copies a batch out of the decoded container): returns once batch_out is
 *     complete.  stager may be NULL: the library finds the stager that launched batch_out (the consumer
 *     knows the buffers, not the providers); a buffer no stager launched (another ETL's, or one already
 *     waited for) returns 0 at once.  The window's last wait surfaces the device error word.
 *   aeon_hip_stager_flush: launch + wait for batch_out (a post_process that returns a finished batch).
 * Two windows are kept (aeon's async_manager, src/async_manager.hpp:162-204, has two containers): the
 * stages of window k+1 go to the other one while window k's copies and kernels run; staging a third
 * window while the first was never waited for completes and drops that first one.
 * Images: aeon_hip_augment_batch semantics; masks (AEON_STAGER_MASK): aeon_hip_mask_batch, staged with
 * the record's image params (provider.cpp:378-391).  Errors: AEON_HIP_E* codes,
 * aeon_hip_stager_last_error(); a window whose launch fails is dropped whole. */
typedef struct aeon_hip_stager aeon_hip_stager;
#define AEON_STAGER_IMAGE      0
#define AEON_STAGER_MASK       1
#define AEON_STAGER_DEVICE_OUT 0x100 /* or-ed into kind: batch buffers are device memory */
int aeon_hip_stager_create(aeon_hip_ctx* ctx, int kind, const aeon_out_desc* out, int batch_size,
                           aeon_hip_stager** stager);
int aeon_hip_stager_destroy(aeon_hip_stager* stager);
int aeon_hip_stager_stage(aeon_hip_stager* stager, void* batch_out, int idx, const void* pixels, int width,
                          int height, int stride, int channels, int elem_bytes, const aeon_aug_params* params);
int aeon_hip_stager_launch(aeon_hip_stager* stager, void* batch_out);
int aeon_hip_stager_wait(aeon_hip_stager* stager, void* batch_out);
int aeon_hip_stager_flush(aeon_hip_stager* stager, void* batch_out);
/* Read-only: the paths the stager's most recently launched window took (as aeon_png_host_stage's gpu_route:
 * a test can prove which path it compared).  launches == 0: nothing was launched yet, the rest is 0.  A
 * window whose launch failed and was dropped leaves the previous report in place. */
typedef struct aeon_stager_launch_info {
    uint64_t launches;      /* windows this stager has launched so far */
    int32_t  src_zero_copy; /* 1: the kernels read the sources from the window's pinned chunk over PCIe;
                             * 0: one H2D per chunk into device memory ahead of them */
    int32_t  out_direct;    /* 1: the kernels stored into the batch buffers (device, or pinned and mapped);
                             * 0: into device memory, each batch's D2H made by its wait */
    int32_t  chunks;        /* pinned staging chunks that held records of the window */
    int32_t  records;       /* records of the window */
} aeon_stager_launch_info;
int aeon_hip_stager_last_launch(aeon_hip_stager* stager, aeon_stager_launch_info* info);
const char* aeon_hip_stager_last_error(void);

/* ---- the drop-in, from encoded records: provide() hands over the file, not the pixels ------------
 * aeon_encoded_info: what a decoder (aeon_decoder_*) finds out about an encoded element before it decodes it, in
 * its order -- PNG signature, then the BMP / PNM sniff, then the TIFF sniff, then the JPEG parser -- on the
 * calling thread, host only, no context.  mask != 0: the file is a pixel mask (CV_LOAD_IMAGE_ANYDEPTH), else an
 * image.  *format: AEON_FORMAT_*; *width / *height: the decoded size (what aeon_make_params needs);
 * *file_channels: the file's own channels (JPEG: components; BMP / PNM and TIFF: as aeon_pixmap_info /
 * aeon_tiff_info; PNG: 1 gray, 2 gray + alpha, 3 RGB and palette, 4 RGBA); *elem_bytes: 2 where ANYDEPTH gives a
 * mask native uint16 samples (16-bit non-palette PNG, PNM with maxval > 255, 16-bit gray TIFF), else 1;
 * *device_route: 1 when the decoder's routing rule sends the file through its device stage
 * (aeon_png_decoder_route, the pixmap stage's rule, aeon_tiff_decoder_route; a JPEG file always), 0 when it
 * decodes on the host.  Any out pointer but format / width / height may be NULL.  Errors are the header
 * parser's own, code and message (aeon_hip_last_error); a JPEG file with mask != 0 is refused as the decoder
 * refuses it ("encoded pixel masks are decoded from PNG files only ..."). */
#define AEON_FORMAT_JPEG   0
#define AEON_FORMAT_PNG    1
#define AEON_FORMAT_PIXMAP 2
#define AEON_FORMAT_TIFF   3
#define AEON_FORMAT_COUNT  4
int aeon_encoded_info(const void* data, size_t size, int mask, int* format, int* width, int* height,
                      int* file_channels, int* elem_bytes, int* device_route);
/* aeon_hip_stager_stage_encoded: aeon_hip_stager_stage for a record still encoded (from provide(), any pool
 * thread, concurrently, mixed freely with aeon_hip_stager_stage in one window and one batch).  The decode mode
 * follows the stager as the decoder's provider picks it: an image stager decodes BGR8 when out->channels is 3,
 * else GRAY8; a mask stager ANYDEPTH, and refuses a JPEG file.  The file's bytes are copied, or decoded, before
 * the call returns.  A file with device_route 0 (aeon_encoded_info) is decoded here, on the calling thread,
 * straight into the window's pinned staging (aeon_decode_png / _pixmap / _tiff) and is an ordinary staged
 * record from then on.  Any other file keeps its bytes until the window's launch, which decodes it into a slot
 * of the window's device source arena with the stage of its format (aeon_hip_decode_{jpeg,png,pixmap,tiff}_batch,
 * at most 512 files a call) on the window's stream, ahead of the augment / mask launches: such a window's sources
 * are never read zero-copy (src_zero_copy 0).  A header the parser refuses returns here with the parser's code
 * and message plus ", at idx N"; the window stays usable and that idx may be staged again.  Corrupt entropy-coded
 * / compressed data of a device-decoded file is AEON_HIP_EDEVICE from the window's last wait; the next window is
 * unaffected. */
int aeon_hip_stager_stage_encoded(aeon_hip_stager* stager, void* batch_out, int idx, const void* data, size_t size,
                                  const aeon_aug_params* params);
/* Read-only: where the records of the most recently launched window were decoded, per AEON_FORMAT_*.
 * launches is aeon_stager_launch_info's; a dropped window leaves the previous report in place. */
typedef struct aeon_stager_decode_info {
    uint64_t launches;
    int32_t  device[AEON_FORMAT_COUNT]; /* decoded by the window's launch, on the device stage of the format */
    int32_t  host[AEON_FORMAT_COUNT];   /* decoded by aeon_hip_stager_stage_encoded on the calling thread */
    int32_t  pixels;                    /* staged decoded (aeon_hip_stager_stage) */
    int32_t  reserved;
} aeon_stager_decode_info;
int aeon_hip_stager_last_decode(aeon_hip_stager* stager, aeon_stager_decode_info* info);

/* ---- the drop-in for provider::video (src/provider.cpp:477-517): provide() stages a clip ---------------
 * A third stager kind.  Launch, wait, flush, destroy, the two windows, aeon_hip_stager_wait(NULL, ...), the error
 * word at a window's last wait and the three output kinds (pinned and mapped, pageable, AEON_STAGER_DEVICE_OUT)
 * are the image stager's; an item of the batch buffer is one clip as aeon_hip_video_batch writes it (uint8 B, G,
 * R planes, channel x frame x height x width, short clips zero-padded to max_frames).
 * aeon_hip_stager_create_video: flags 0 or AEON_STAGER_DEVICE_OUT; 1 <= max_frames <= 65535; item_stride at least
 *   3*max_frames*out_h*out_w, else AEON_HIP_EINVAL; an item above 2^31 - 1 bytes is AEON_HIP_EUNSUPPORTED with
 *   the video call's message.
 * aeon_clip_info (host only, no context): video::extractor's demux of the first max_frames frames
 *   (aeon_avi_frames with cap = max_frames) and aeon_jpeg_info of the first kept frame: *kept =
 *   min(frame count, max_frames), *width / *height the first frame's decoded size -- what provider::video calls
 *   make_params with (provider.cpp:503-513), not avih's dwWidth / dwHeight.  Errors are the demux's or the JPEG
 *   parser's own code and text, in aeon_hip_stager_last_error().
 * aeon_hip_stager_stage_clip (from provide(), any pool thread, concurrently): clip idx of batch_out from the AVI
 *   datum.  The first max_frames frames are kept; each non-empty one's JPEG header is parsed and must give the
 *   first one's size; an empty chunk repeats the frame before it and takes no slot.  The frames' bytes are copied
 *   before the call returns; each distinct frame gets a slot of the window's device source arena, which the
 *   window's launch fills through aeon_hip_decode_jpeg_batch (at most 512 files a call) ahead of the video call.
 *   An empty datum: "received encoded video with size 0, at idx N" (AEON_HIP_EINVAL); whatever the demux or a
 *   frame header refuses, and a frame of another size, return here with that code and text plus ", at idx N".
 *   The window stays usable and that idx may be staged again.
 * aeon_hip_stager_stage_frames: clip idx from n_frames (1 .. max_frames) decoded BGR frames of width x height,
 *   rows `stride` bytes apart (0: width*3), copied into the window's pinned staging before the call returns
 *   (aeon's video::extractor stays on the host).  pixels[d] == NULL, d > 0, repeats the frame before it.
 * The two forms may share a window and a batch.  params->out_w / out_h other than the stager's are
 * AEON_HIP_EINVAL.  aeon_hip_stager_stage / _stage_encoded on a video stager, and these two on an image or mask
 * stager, are AEON_HIP_EINVAL naming the kind.
 * The window's launch makes one aeon_hip_video_batch per batch (a batch of more than 65,535 frames: several),
 * into the batch buffers where they are device memory or pinned and mapped, else into the window's device output
 * with each batch's D2H made by its wait.  aeon_stager_launch_info.records counts clips, src_zero_copy follows the
 * image stager's rule (no device-decoded frame in the window); aeon_stager_decode_info.device[AEON_FORMAT_JPEG]
 * counts the frames the launch decoded and .pixels the frames staged decoded (repeats count with neither). */
#define AEON_STAGER_VIDEO 2
int aeon_hip_stager_create_video(aeon_hip_ctx* ctx, int flags, int max_frames, int out_w, int out_h, uint64_t item_stride,
                                 int batch_size, aeon_hip_stager** stager);
int aeon_clip_info(const void* data, size_t size, int max_frames, int* kept, int* width, int* height);
int aeon_hip_stager_stage_clip(aeon_hip_stager* stager, void* batch_out, int idx, const void* data, size_t size,
                               const aeon_aug_params* params);
int aeon_hip_stager_stage_frames(aeon_hip_stager* stager, void* batch_out, int idx, int n_frames,
                                 const void* const* pixels, int width, int height, int stride,
                                 const aeon_aug_params* params);

/* ---- host staging (replaces the dead cuMemAllocHost branch, src/buffer_batch.cpp:150-186) -- */
int aeon_hip_host_alloc(size_t bytes, void** out);
int aeon_hip_host_free(void* p);

/* Diagnostics: the device address ranges [lo, hi) of every uncached job-table block this process
 * allocated (stage.cpp grow_vram; they are pooled, never freed: DESIGN.md §8), up to cap pairs into
 * ranges; *n = how many there are.  Lets a test that finds lost writes say whether they lie inside one. */
int aeon_hip_debug_uncached_blocks(uint64_t* ranges, int cap, int* n);

const char* aeon_hip_last_error(void);
const char* aeon_hip_version(void);

#ifdef __cplusplus
}
#endif

#endif /* AEON_HIP_H */
