// host.hpp -- aeon's provider plugin surface and decode stage for the HIP image path (host C++).
//
// Mirrors, with the same names and argument meaning:
//   provider_interface       src/provider_interface.hpp:32-85  (post_process = the GPU flush)
//   provider_factory::create src/provider_factory.cpp:24-51
//   provider::image          src/provider.cpp:145-184          (etl type "image")
//   provider::pixelmask      src/provider.cpp:353-393          (etl type "pixelmask")
//   provider::boundingbox    src/provider.cpp:395-439          (etl type "boundingbox")
//   provider::localization::ssd src/provider.cpp:289-346       (etl type "localization_ssd")
//   provider::localization::rcnn src/provider.cpp:222-287      (etl type "localization_rcnn")
//   provider::video          src/provider.cpp:477-517          (etl type "video": an MJPEG AVI datum)
//   provider::label          src/provider.cpp:190-216          (etl type "label")
//   image::config            src/etl_image.hpp:56-96, etl_image.cpp:25-65
//   batch_decoder            src/batch_decoder.cpp:24-99        (thread pool + deterministic slots)
//   thread_pool              src/thread_pool.hpp:82-175         (dynamic atomic task counter)
//   manifest node slicing    src/manifest_file.cpp:278-295
// Records arrive as encoded JPEG files (image::extractor::extract's cv::imdecode runs in the
// JPEG stage: host Huffman + GPU IDCT/colour, jpeg_host.cpp) or as decoded HWC uint8 pixels (staged
// into pinned memory by the pool).  One flush per decode window runs the HIP kernels; windows are
// double-buffered like async_manager's two containers (submit / wait).
#pragma once
#include <atomic>
#include <condition_variable>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/aeon_hip.h"
#include "avi_host.hpp"
#include "box_host.hpp"
#include "json.hpp"
#include "param_factory.hpp"
#include "rcnn_host.hpp"

namespace aeon_hip {

// typemap.hpp output_type (the types this stage writes)
struct output_type {
    std::string name;
    size_t      size  = 1;
    int         dtype = AEON_DTYPE_U8;
    explicit output_type(const std::string& n = "uint8_t");
    static bool is_valid_type(const std::string& n);
};

struct shape_type {
    std::vector<size_t>      shape;
    std::vector<std::string> names;
    output_type              otype;
    size_t                   byte_size() const;
};

// image::config
struct image_config {
    uint32_t    height = 0, width = 0;
    std::string output_type_name = "uint8_t";
    bool        bgr_to_rgb = false, channel_major = true;
    uint32_t    channels = 3;
    std::string name;
    shape_type  shape;
    explicit image_config(const Json& js, bool half = false); // half: "float16" / "bfloat16" with "extended_output_type": true
};

// An element of a record: an encoded JPEG, PNG, BMP, PNM or TIFF file (size > 0; width/height/channels filled in from
// its header by its provider's inspect step), decoded HWC uint8 pixels (what image::extractor::extract
// returns), or the datum of a box, video or label provider (data / size: JSON metadata, an MJPEG AVI
// file whose width / height the demux fills in from its first frame, a label's bytes).
struct decoded_element {
    const uint8_t* data = nullptr;
    int            width = 0, height = 0, channels = 0, stride = 0;
    size_t         size    = 0;     // encoded bytes
    bool           encoded = false; // JPEG file: decoded on the device (jpeg_host.cpp)
    int            png_mode   = -1; // PNG file: its AEON_PNG_* decode mode
    bool           png_device = false; // ... decoded on the device (the PNG stage, png.hpp's routing rule), else on
                                       // the host pool while staging
    int            pixmap_mode   = -1; // BMP / PNM file: its AEON_DECODE_* mode
    bool           pixmap_device = false; // ... converted on the device (the pixmap stage, pixmap.hpp's routing
                                          // rule), else decoded on the host pool while staging (ASCII PNM)
    int            tiff_mode   = -1; // TIFF file: its AEON_DECODE_* mode
    bool           tiff_device = false; // ... decoded on the device (the TIFF stage, tiff.hpp's routing rule), else on
                                        // the host pool while staging
    int            elem_bytes = 1;  // bytes per sample (2: a 16-bit mask / depth map)
    // decoded on the device, straight into the device-decoded region of the source arena
    bool on_device() const { return encoded || png_device || pixmap_device || tiff_device; }
};

// What one provider keeps of a window's n records (etl_provider::new_part): the source descriptors into the
// arena -- one per record of a pixel provider, max_frame_count per record of a video provider -- and, in the
// provider's own subclass, its metadata, values, offsets and counts.
struct window_part {
    virtual ~window_part() = default;
    std::vector<aeon_img_desc> descs;
};

// Per-window staging shared by the providers (filled concurrently by the pool threads).
struct decode_window {
    int                                       n = 0;
    std::vector<std::vector<aeon_aug_params>> params; // [provider][record]
    std::vector<std::unique_ptr<window_part>> parts;  // [provider]
    uint8_t*                                  arena = nullptr;
};

// The source arena of a window, in this order, every claim 16-byte aligned: the box tables (provider order),
// the label items (provider order), the staged elements (record-major, provider-minor) -- up to here it is
// pinned host memory copied H2D in one piece --, then the device-decoded slots (record-major, provider-minor;
// a clip's frame slots at its element's position).
enum class arena_region { box_tables, label_items, staged, device_decoded };
inline size_t arena_align(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// The PNG files one provider wants decoded into the device-decoded region, with their modes and destinations
struct png_list {
    std::vector<const void*>   files;
    std::vector<size_t>        sizes;
    std::vector<int>           modes;
    std::vector<aeon_img_desc> descs;
    void add(const void* file, size_t size, int mode, const aeon_img_desc& d)
    {
        files.push_back(file), sizes.push_back(size), modes.push_back(mode), descs.push_back(d);
    }
};

using pixmap_list = png_list; // the BMP / PNM files likewise (AEON_DECODE_* modes)
using tiff_list   = png_list; // and the TIFF files

// The JPEG files one provider wants decoded into the device-decoded region, with their destinations; its PNG,
// pixmap and TIFF files travel beside them
struct jpeg_list {
    png_list                   png;
    pixmap_list                pixmap;
    tiff_list                  tiff;
    std::vector<const void*>   files;
    std::vector<size_t>        sizes;
    std::vector<aeon_img_desc> descs;
    void add(const void* file, size_t size, const aeon_img_desc& d) { files.push_back(file), sizes.push_back(size), descs.push_back(d); }
};

// Where the engines' states after a localization_rcnn window's device shuffles go (deterministic mode; dev
// null: not wanted): the device words, their pinned host copy, the event recorded behind the copy, and whether
// the copy and the event are on the stream.
struct engine_states {
    uint32_t*  dev = nullptr, *host = nullptr;
    hipEvent_t done   = nullptr;
    bool       queued = false;
};

// A box provider's part of a window: the records' extracted metadata, where the provider's box table (BoxRec
// per record, then boxes, labels, difficult flags; box_job.hpp) lies in the arena and how many boxes it
// holds.  localization_rcnn: the minstd_rand0 state record i's shuffles start from, and where the states after
// the shuffles go (copied back right behind the targets kernel).
struct box_part : window_part {
    std::vector<box_metadata> boxes;
    size_t                    offset = 0, total = 0;
    std::vector<uint32_t>     engines;
    engine_states*            end = nullptr;
};

// One record of a video provider after video::extractor's demux (avi_host.hpp): the kept frames (the first
// min(frames of the file, max_frame_count)) and the first frame's size, which every other non-empty kept
// frame must have.
struct video_clip {
    std::vector<aeon_avi_frame> frames;
    int                         width = 0, height = 0;
};

// A video provider's part of a window: the records' demuxed clips and the number of kept frames; descs holds
// max_frame_count frame descriptors per clip (one arena slot per distinct decoded frame).
struct video_part : window_part {
    std::vector<video_clip> clips;
    std::vector<int32_t>    counts;
};

// A label provider's part of a window: the records' values, and where the provider's output items (n values of
// its output type) are staged in the arena for a device output.
struct label_part : window_part {
    std::vector<int32_t> values;
    size_t               offset = 0;
};

// augmentation shared by the ETL providers of one record (provider.cpp:109-119)
struct augmentation {
    bool            has = false;
    aeon_aug_params image{};
};

class provider_interface {
public:
    provider_interface(Json js, size_t input_count) : m_js(std::move(js)), m_input_count(input_count) {}
    virtual ~provider_interface() = default;

    size_t                                                  get_input_count() const { return m_input_count; }
    const std::vector<std::pair<std::string, shape_type>>& get_output_shapes() const { return m_output_shapes; }
    const shape_type&                                       get_output_shape(const std::string& name) const;
    const std::vector<std::string>&                         get_buffer_names();
    const Json&                                             get_config() const { return m_js; }

protected:
    std::vector<std::pair<std::string, shape_type>> m_output_shapes;
    std::vector<std::string>                        m_buffer_names;
    Json                                            m_js;
    size_t                                          m_input_count = 0;
};

class thread_pool;

// One record's share of a parallel window draw (param_factory::make_params_split): the lighting
// cache state it starts from, and the value it leaves cached.
struct light_split {
    bool  entry_avail = false;
    float exit_saved  = 0.f;
};

// What a record's params are drawn over (etl_provider::draw): the source size and the target size;
// nboxes >= 0 asks for make_ssd_params over the record's boxes.
struct draw_source {
    int          in_w = 0, in_h = 0, out_w = 0, out_h = 0;
    const float* boxes  = nullptr;
    int          nboxes = -1;
};

// One ETL element provider of the HIP stage: image, pixelmask, boundingbox, localization_ssd,
// localization_rcnn, video or label.  Its virtuals are the steps of a decode window, in the order they run;
// part is the provider's own new_part() of that window, e its element of record idx.
class etl_provider {
public:
    virtual ~etl_provider() = default;
    // the provider's output buffers in aeon's get_output_shapes() order
    virtual std::vector<std::pair<std::string, shape_type>> output_shapes() const = 0;
    // the factory the provider's draws go through; null for a provider that draws nothing (label)
    virtual const param_factory* factory() const = 0;
    // the element as the C ABI hands it over (the byte size of a datum; decoded pixels or an encoded file)
    virtual void from_abi(const aeon_encoded_elem& in, int idx, decoded_element& e) const = 0;
    virtual std::unique_ptr<window_part> new_part(int n) const = 0;
    // inspect (on the pool): refuses an empty element and reads what the draw and the layout need -- the PNG /
    // JPEG header, the AVI demux and the kept frames' headers, the JSON metadata, the label's int
    virtual void inspect(window_part& part, int idx, decoded_element& e) const = 0;
    // draw: the record's params through the shared augmentation (the first element of a record draws, the
    // others copy); with ls, the record is drawn out of order (provider_base::draw_window)
    void draw(const window_part& part, int idx, const decoded_element& e, augmentation& aug, std::minstd_rand0& random,
              aeon_aug_params& params, light_split* ls) const;
    // layout: the provider claims its bytes of region r from the running offset and records its descriptors,
    // per window (box table, label items) or per record (pixels, device-decoded slots); the JPEG files it wants
    // decoded go into jpegs with their destinations
    virtual void layout_window(window_part&, arena_region, int /*n*/, size_t& /*offset*/) const {}
    virtual void layout_record(window_part&, arena_region, int /*idx*/, const decoded_element&, size_t& /*offset*/,
                               jpeg_list&) const
    {
    }
    // stage: the provider's staged bytes into the pinned arena, per window (the box table, with its host-side
    // refusals; the label items) or per record on the pool (pixels, the PNG decode)
    virtual void stage_window(const decode_window&, size_t /*k*/) const {}
    virtual void stage_record(const decode_window&, size_t /*k*/, int /*idx*/, const decoded_element&) const {}
    // launch: the provider's device work over the arena's device copy into out[] (its output buffers)
    virtual void launch(aeon_hip_ctx* ctx, const decode_window& w, size_t k, const uint8_t* dev_arena, void* const* out,
                        void* stream) const = 0;
    // host output: a provider that needs no device writes its n items into the host buffer and returns true
    virtual bool host_output(const window_part&, int /*n*/, void* /*out*/) const { return false; }
    // A provider whose device work shuffles (localization_rcnn) is handed the engine word each record's
    // shuffles start from and where the engines' end states go (the decoder's: they cross windows).
    virtual void take_engines(window_part&, std::vector<uint32_t>&&, engine_states*) const {}
    // the image + pixelmask pair call's one question: the output descriptor of a plain image (mask false) /
    // of a pixel mask (mask true), null for anything else
    virtual const aeon_out_desc* pixel_out(bool /*mask*/) const { return nullptr; }

protected:
    // what idx's draw is made over; false: the provider draws nothing
    virtual bool draw_over(const window_part& part, int idx, const decoded_element& e, draw_source& s) const = 0;
};

// What batch_decoder::plan makes of a window on the host alone: the inspected elements, the drawn window, its
// arena layout (staged bytes are copied H2D, total includes the device-decoded slots), the JPEG files per
// provider, and the records' shuffle engine words (empty unless a provider shuffles).
struct window_plan {
    std::vector<decoded_element> records;
    decode_window                w;
    size_t                       staged = 0, total = 0;
    std::vector<jpeg_list>       jpegs; // [provider]
    std::vector<uint32_t>        engines;
};

class provider_base : public provider_interface {
public:
    provider_base(const Json& js, const std::vector<Json>& etl, const Json& augmentation);
    // a window of n records: params and one part per provider
    decode_window new_window(int n) const;
    // every element of the window through its provider's inspect, on the pool
    void inspect_window(int n, decoded_element* records, decode_window& w, thread_pool& pool) const;
    // record idx of the window: params for every ETL element from one shared augmentation
    // (provider_base::provide, provider.cpp:109-119)
    void draw(int idx, const decoded_element* elems, decode_window& w, std::minstd_rand0& random,
              light_split* ls = nullptr) const;
    // draw() for every record of a window with its own engine (deterministic mode), on the pool:
    // the same params as the in-order loop (the lighting cache hand-off is fixed up afterwards)
    void draw_window(int n, const decoded_element* records, decode_window& w, std::vector<std::minstd_rand0>& engines,
                     thread_pool& pool) const;
    // the arena layout of an inspected, drawn window: p.staged, p.total, p.jpegs and the parts' descriptors
    void layout(window_plan& p) const;
    // the window's tables and items into the arena, then its records' pixels on the pool
    void stage(const window_plan& p, thread_pool& pool) const;
    // aeon's vestigial post_process hook, used as the per-window GPU flush: outputs[k] receives
    // n items of provider k (device pointers if on_device, else host memory)
    void post_process(aeon_hip_ctx* ctx, const decode_window& w, const uint8_t* dev_arena, void* const* outputs,
                      void* stream) const;
    const std::vector<std::unique_ptr<etl_provider>>& providers() const { return m_providers; }
    // outputs[] of the decoder calls follow get_output_shapes(): provider k's buffers are
    // output_first(k) .. output_first(k + 1) - 1
    int  output_first(size_t k) const { return m_out_first[k]; }
    // some element is a datum with a byte size (box metadata, an AVI file, a label): what aeon_record_elem
    // cannot carry
    bool has_sized() const { return m_has_sized; }
    // a provider's device work shuffles: every record needs an engine word (take_engines hands them over)
    bool shuffles() const { return m_shuffler >= 0; }
    void take_engines(decode_window& w, std::vector<uint32_t>&& words, engine_states* end) const
    {
        m_providers[m_shuffler]->take_engines(*w.parts[m_shuffler], std::move(words), end);
    }

private:
    std::vector<std::unique_ptr<etl_provider>> m_providers;
    std::vector<int>                           m_out_first; // size providers + 1
    bool                                       m_has_sized = false;
    int                                        m_shuffler  = -1; // the localization_rcnn provider
};

struct provider_factory {
    static std::shared_ptr<provider_base> create(const Json& config);
};

// thread_pool (src/thread_pool.hpp:82-175): persistent workers, worker i pinned to CPU
// affinity_map[i] (pthread_setaffinity_np, thread_pool.hpp:133-138); run(n, fn) hands out task ids
// from one atomic counter; the first exception is kept and rethrown after the barrier.
class thread_pool {
public:
    // one worker per entry of affinity_map (at least one; an empty map = one unpinned worker)
    explicit thread_pool(std::vector<int> affinity_map);
    ~thread_pool();
    void run(int n, const std::function<void(int)>& fn);
    // fn(task, worker): worker in [0, size()) identifies the calling pool thread
    void run_indexed(int n, const std::function<void(int, int)>& fn);
    int  size() const { return m_nthreads; }
    const std::vector<int>& affinity_map() const { return m_map; }
    // what worker i's own sched_getaffinity returned after it pinned itself (blocks until every
    // worker has started); a CPU outside the process's cpuset cannot be pinned to, and that worker
    // keeps the process mask -- aeon ignores pthread_setaffinity_np's result the same way
    std::vector<std::vector<int>> worker_cpus();

private:
    void                                 worker(int index);
    std::vector<int>                     m_map;
    std::vector<std::vector<int>>        m_worker_cpus;
    int                                  m_started = 0, m_nthreads = 0;
    std::vector<std::thread>             m_threads;
    std::mutex                           m_mu;
    std::condition_variable              m_cv, m_done_cv;
    const std::function<void(int, int)>* m_fn = nullptr;
    int                            m_n = 0;
    std::atomic<int>               m_done{0}; // tasks of the current run completed
    long                           m_generation = 0;
    std::atomic<uint64_t>          m_state{0}; // (generation << 32) | next task: a task is taken only in its own run
    std::exception_ptr             m_error;
    bool                           m_stop = false;
};

// batch_decoder: decode windows of records on the pool, flush each window to the GPU.
// Two window slots (async_manager's two containers, src/async_manager.hpp:203-204), each with its
// own pinned staging, device buffers, stream and completion event: submit() stages window k+1 and
// enqueues its copies and kernels while window k's are still running; wait() completes the oldest.
class batch_decoder {
public:
    batch_decoder(const Json& config, int device);
    ~batch_decoder();
    // n records x input_count elements (row-major); outputs[k] per provider buffer.  Synchronous,
    // on `stream` (batch_decoder::filler, src/batch_decoder.cpp:73-99).
    void decode(int n, const decoded_element* records, void* const* outputs, bool outputs_on_device,
                void* stream);
    // Asynchronous window on the decoder's own streams: returns once the records' bytes are
    // consumed (drawn, staged, entropy-decoded); outputs are complete after the matching wait().
    void submit(int n, const decoded_element* records, void* const* outputs, bool outputs_on_device);
    void wait(); // oldest submitted window
    // the draw phase of one window alone (host only): params[i] = record i's (first element's)
    // params; serial = the in-order loop instead of draw_window
    void draw_params(int n, const decoded_element* records, aeon_aug_params* params, bool serial);
    // the host half of one window alone -- inspect, draw and the arena layout --: no device call, no window
    // slot; what decode() and submit() go on to stage and launch
    window_plan plan(int n, const decoded_element* records);
    int  outstanding() const { return (int)m_queue.size(); }
    provider_base& provider() { return *m_provider; }
    thread_pool&   pool() { return *m_pool; }
    int            batch_size() const { return m_batch_size; }

private:
    struct window_slot {
        hipStream_t           stream  = nullptr;
        hipEvent_t            done    = nullptr;
        bool                  pending = false;
        uint8_t*              pinned = nullptr;
        size_t                pinned_cap = 0;
        uint8_t*              dev_src = nullptr;
        size_t                dev_src_cap = 0;
        std::vector<uint8_t*> dev_out, dev_tmp;
        std::vector<size_t>   dev_out_cap, dev_tmp_cap;
        // localization_rcnn, deterministic mode: the window's engine end states (device, pinned host)
        uint32_t*             states_dev = nullptr, *states_host = nullptr;
        size_t                states_cap = 0;
        hipEvent_t            states_done = nullptr;
    };
    // the slot engines take over the states an earlier rcnn window's shuffles left (waits for that
    // window's small copy alone)
    void adopt_states();
    window_slot*                   m_states_from = nullptr; // window whose end states are not adopted yet
    int                            m_states_n    = 0;
    // where each output buffer's device work writes (null: the provider wrote its host output itself, on_host),
    // and which are staged on the device and then copied D2H into outputs[k]
    struct routed_outputs {
        std::vector<void*> dev;
        std::vector<bool>  copy_out, on_host;
    };
    // one window through slot ws: plan -> stage_sources -> route_outputs -> launch
    void enqueue(window_slot& ws, int n, const decoded_element* records, void* const* outputs, bool on_device,
                 hipStream_t stream);
    void draw(window_plan& p, int n, const decoded_element* records, bool serial);
    void slot_states(window_slot& ws, int n, engine_states& end);
    void stage_sources(window_slot& ws, window_plan& p, hipStream_t stream);
    routed_outputs route_outputs(window_slot& ws, const decode_window& w, void* const* outputs, bool on_device);
    void launch(window_slot& ws, const decode_window& w, const routed_outputs& r, void* const* outputs, hipStream_t stream);
    void                           grow_slot_engines(int n);
    std::shared_ptr<provider_base> m_provider;
    int                            m_batch_size = 1;
    bool                           m_deterministic = false;
    std::vector<std::minstd_rand0> m_random; // one engine per decode slot (batch_decoder.cpp:47-54)
    std::minstd_rand0              m_seed_gen; // seeds m_random[i] (grow_slot_engines)
    std::minstd_rand0              m_local_random; // non-deterministic mode (util.cpp:266)
    std::unique_ptr<thread_pool>   m_pool;
    aeon_hip_ctx*                  m_ctx = nullptr;
    int                            m_device = 0;
    window_slot                    m_slots[2];
    int                            m_next = 0;
    std::vector<int>               m_queue; // submitted, not yet waited (slot indices, oldest first)
    // batch_major=false (loader.hpp:63): outputs are produced batch-major into dev_tmp and
    // transposed per batch into the caller's layout (batch_iterator.cpp:125-136)
    bool                           m_batch_major = true;
};

// manifest_file node slicing (generate_blocks, src/manifest_file.cpp:278-295)
std::vector<int64_t> manifest_node_slice(int64_t record_count, int batch_size, int node_id, int node_count);

// nervana::parse_cpu_list (src/util.cpp:283-330): "0-4,30,10" -> sorted, de-duplicated CPU ids;
// std::invalid_argument for an id >= hardware_concurrency
std::vector<int> parse_cpu_list(const std::string& cpu_list);
// nervana::get_thread_affinity_map (src/util.cpp:337-373): AEON_CPU_LIST over the config's cpu_list;
// else hc - min(2, hc/8) CPUs.  aeon's default is iota(0, ...); here it is the first CPUs of the
// process's own affinity mask (the same list on an unrestricted host; inside a container given 16
// of 256 CPUs, CPUs the workers can actually be pinned to), capped by OMP_NUM_THREADS.
std::vector<int> thread_affinity_map(const std::string& cpu_list);
int aeon_thread_count(const std::string& cpu_list); // thread_affinity_map(cpu_list).size()
// the decoder's pool runs its context's JPEG entropy decoding too (context.cpp)
void ctx_share_pool(aeon_hip_ctx* ctx, thread_pool* pool);
// aeon_hip_box_targets_batch over a box table that already lies in device memory (the decoder stages it
// in the window's arena with the pixels, so a window makes one H2D): table = n BoxRec, then `total`
// boxes, labels and difficult flags (box_job.hpp).  out and the result as in the C call; the records'
// refusals (box_refusal) are the caller's to make while it stages.
int box_targets_staged(aeon_hip_ctx* ctx, int n, const void* dev_table, size_t total, const aeon_box_out& out,
                        void* stream);
// aeon_hip_rcnn_targets_batch over a staged table with the rcnn extension (box_job.hpp: then RcnnRec[n]);
// states_dev (n words, or null) receives the engines' states after the shuffles
int rcnn_targets_staged(aeon_hip_ctx* ctx, int n, const void* dev_table, size_t total, const aeon_rcnn_out& out,
                        int shuffle, uint32_t* states_dev, void* stream);
// a map stretched or cut to n workers (decode_thread_count / AEON_HIP_JPEG_THREADS): worker i on map[i % size]
std::vector<int> affinity_for(const std::vector<int>& map, int n);

} // namespace aeon_hip
