// rcnn_kernels.hip -- localization_rcnn anchor targets of a decode window in one launch.
//
// aeon's provider::localization::rcnn (provider.cpp:222-287) transforms a record's object boxes with the
// params of its image, labels every anchor of the feature grid by its overlap with them, samples
// rois_per_image of the labelled anchors and loads ten buffers
// (localization::rcnn::transformer::transform / sample_anchors / loader::load,
// etl_localization_rcnn.cpp:97-261, 340-428).  Here: one 1024-thread workgroup per record, the record's
// state in LDS (rcnn_job.hpp states the limits that follow), these steps between workgroup barriers:
//   0  wave 0: transform_box of the record's boxes, compacted in input order into LDS (all K survivors)
//      and into gt_boxes / gt_class_count / difficult_flag (the first max_gt_boxes); small outputs
//   1  every inside anchor x gt box: bbox_overlaps, column maxima by LDS atomic max on the bit pattern
//      (overlaps are >= 0, so the unsigned order of the patterns is the float order)
//   2  overlaps again (same inputs, same order, same bits): row maximum, tie with a column maximum,
//      label; a wave's 64 labels become one word each of the foreground and background bitmaps
//   3  wave 0: running counts per 64 anchors, then std::shuffle of the two lists' ranks
//      (rcnn_shuffle.hpp; 64 draws at a time, wave_shuffle_prefix below), keeping the sampled prefixes
//   4  sampled ranks -> anchor indices (search of the running counts, then the rank-th set bit of the
//      word), marked in a third bitmap; the lane that found an anchor computes its regression target
//      (one argmax over the gt boxes) and stores its four words of bbtargets
//   5  every other element of the four big buffers is written, 16 bytes per lane and step, its value
//      picked from the bitmaps: each element has one writer
// The K x A overlap matrix is never stored.
//
// Arithmetic: float32, every operation rounded once and in aeon's order (-ffp-contract=off, correctly
// rounded divisions); dw / dh go through logf, which is within 1 ulp of the exact value as glibc's is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aeon_hip.h"
#include "box_device.hpp"
#include "rcnn_job.hpp"
#include "launch.hpp"
#include "rcnn_shuffle.hpp"

namespace aeon_hip {

namespace {

constexpr int kThreads = 1024; // 16 waves: the fills want many stores in flight per CU
constexpr int kWaves   = kThreads / 64;
constexpr int kChunks  = kRcnnMaxAnchors / 64; // 64 anchors: one wave step, two bitmap words
constexpr int kWords   = kRcnnMaxAnchors / 32;

// transformer::bbox_overlaps for one anchor and one gt box (garea = gt.width() * gt.height())
__device__ inline float overlap(const float4 a, const float4 g, const float garea)
{
    const float ix1 = g.z < a.z ? g.z : a.z; // std::min(b.xmax(), gt.xmax())
    const float ix0 = a.x < g.x ? g.x : a.x; // std::max(b.xmin(), gt.xmin())
    const float iw  = ix1 - ix0 + 1.0f;
    if (!(iw > 0)) return 0.0f;
    const float iy1 = g.w < a.w ? g.w : a.w;
    const float iy0 = a.y < g.y ? g.y : a.y;
    const float ih  = iy1 - iy0 + 1.0f;
    if (!(ih > 0)) return 0.0f;
    const float aw = a.z - a.x + 1.0f, ah = a.w - a.y + 1.0f;
    const float ua = aw * ah + garea - iw * ih;
    return iw * ih / ua;
}

// anchor::inside_image_bounds
__device__ inline bool inside(const float4 a, const float im_w, const float im_h)
{
    return a.x >= 0 && a.y >= 0 && a.z < im_w && a.w < im_h;
}

// box::xcenter (box.hpp:92): the float difference, halved and added in double, narrowed
__device__ inline float center(const float lo, const float hi) { return (float)((double)lo + (double)(hi - lo) / 2.); }

__device__ inline bool bit(const uint32_t* words, int i) { return (words[i >> 5] >> (i & 31)) & 1u; }

// a * b mod 2^31 - 1
__device__ inline uint32_t mulmod31(uint32_t a, uint32_t b)
{
    const uint64_t p = (uint64_t)a * b;
    uint64_t       r = (p & 0x7fffffffu) + (p >> 31);
    r                = (r & 0x7fffffffu) + (r >> 31);
    return r >= 0x7fffffffu ? (uint32_t)(r - 0x7fffffffu) : (uint32_t)r;
}

// rcnn_shuffle_prefix by one wave (all 64 lanes call it with the same arguments; out in LDS).  The swaps
// below the kept prefix run on lane 0 as the header states them.  From swap m on, a swap only ever stores
// its own index i into out[j] (j < m), and the last such store wins, which is the largest i: an atomic
// max, whatever the order.  So the wave takes 64 draws at once -- lane l the (l + 1)-th output of the
// engine, x * 16807^(l+1) mod 2^31 - 1 (apow = that power) -- and lets lane l serve the l-th pending
// swap (or pair of swaps) as long as no earlier lane's draw was rejected by the distribution's
// `while (ret >= past)`: the first rejected draw is consumed, and the swap it was for starts the next
// round.  The engine ends where the sequential shuffle leaves it.
__device__ inline void wave_shuffle_prefix(uint32_t n, uint32_t keep, minstd0& g, int32_t* out, int lane, uint32_t apow)
{
    const uint32_t m = n < keep ? n : keep;
    if (n < 2) {
        if (lane == 0 && m) out[0] = 0;
        return;
    }
    const bool pairs = rcnn_shuffle_pairs(n);
    uint32_t   i = 1, x = g.x;
    if (lane == 0) {
        for (uint32_t k = 0; k < m; k++) out[k] = (int32_t)k;
        minstd0 h{x};
        if (pairs && (n & 1u) == 0) rcnn_prefix_swap(out, m, i++, rcnn_uniform(h, 1));
        while (i < m && i != n) {
            if (pairs) {
                const uint32_t b1 = i + 2, v = rcnn_uniform(h, (i + 1) * b1 - 1);
                rcnn_prefix_swap(out, m, i, v / b1);
                rcnn_prefix_swap(out, m, i + 1, v % b1);
                i += 2;
            } else {
                rcnn_prefix_swap(out, m, i, rcnn_uniform(h, i));
                i += 1;
            }
        }
        x = h.x;
    }
    __builtin_amdgcn_wave_barrier(); // lane 0's stores stay ahead of the other lanes' atomics
    i = (uint32_t)__shfl((int)i, 0);
    x = (uint32_t)__shfl((int)x, 0);
    const uint32_t step  = pairs ? 2u : 1u;
    uint32_t       units = (n - i) / step; // pending swaps (pairs of swaps)
    while (units > 0) {
        const uint32_t mine    = i + step * (uint32_t)lane;
        const uint32_t uerange = pairs ? (mine + 1) * (mine + 2) : mine + 1;
        const bool     valid   = (uint32_t)lane < units;
        const uint32_t draw    = mulmod31(x, apow);
        uint32_t       scaling = 1, ret = draw - 1u;
        bool           reject  = false;
        if (valid) {
            scaling = kRcnnUrngRange / uerange;
            reject  = ret >= uerange * scaling;
        }
        const unsigned long long rej   = __ballot(reject);
        const uint32_t           live  = units < 64u ? units : 64u;
        const uint32_t           first = rej ? (uint32_t)(__ffsll((long long)rej) - 1) : 64u;
        const uint32_t           done  = first < live ? first : live; // swaps served this round
        if ((uint32_t)lane < done) {
            const uint32_t v = ret / scaling;
            if (pairs) {
                const uint32_t b1 = mine + 2, j0 = v / b1, j1 = v - j0 * b1;
                if (j0 < m) atomicMax(&out[j0], (int32_t)mine);
                if (j1 < m) atomicMax(&out[j1], (int32_t)(mine + 1));
            } else if (v < m) {
                atomicMax(&out[v], (int32_t)mine);
            }
        }
        const uint32_t consumed = first < live ? first + 1 : live;
        x = (uint32_t)__shfl((int)draw, (int)consumed - 1);
        i += step * done;
        units -= done;
    }
    g.x = x;
}

// len 32-bit words at p (4-byte aligned), element e = val(e): single words up to the first 16-byte
// boundary and after the last, 16 bytes per lane and step between them
// quick(e, v): when elements e .. e + 3 need no look at single anchors, their four values into v
// skip(e): element e is another writer's (step 4 stores the sampled anchors' targets) and is left alone
template <typename F, typename Q, typename S>
__device__ inline void fill_words(uint32_t* p, int len, int tid, F val, Q quick, S skip)
{
    int head = (int)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) >> 2);
    if (head > len) head = len;
    if (tid < head && !skip(tid)) p[tid] = val(tid);
    const int nvec = (len - head) >> 2;
    uint4*    v    = (uint4*)(p + head);
    for (int j = tid; j < nvec; j += kThreads) {
        const int e = head + 4 * j;
        uint4     q;
        if (!quick(e, q)) {
            if (skip(e) || skip(e + 1) || skip(e + 2) || skip(e + 3)) { // word by word around the other writer's
                for (int k = 0; k < 4; k++)
                    if (!skip(e + k)) p[e + k] = val(e + k);
                continue;
            }
            q = make_uint4(val(e), val(e + 1), val(e + 2), val(e + 3));
        }
        v[j] = q;
    }
    const int tail = head + 4 * nvec;
    if (tid < len - tail && !skip(tail + tid)) p[tail + tid] = val(tail + tid);
}

__global__ __launch_bounds__(kThreads) void rcnn_targets(RcnnLaunch L)
{
    __shared__ float4   s_gt[kRcnnMaxBoxes];
    __shared__ float    s_garea[kRcnnMaxBoxes];
    __shared__ uint32_t s_colmax[kRcnnMaxBoxes];
    __shared__ uint32_t s_fg[kWords], s_bg[kWords], s_sel[kWords + 1]; // (+1: clean4 reads a word pair)
    __shared__ int32_t  s_pfg[kChunks], s_pbg[kChunks]; // anchors of the kind before the chunk
    __shared__ int32_t  s_ranks[kRcnnMaxRois];
    __shared__ int32_t  s_K, s_take_fg, s_take_bg;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rec = blockIdx.x;
    const int A   = L.total_anchors;
    // the host refuses these; a launch that reaches here with them writes nothing
    if (A <= 0 || A > kRcnnMaxAnchors || L.rois_per_image < 0 || L.rois_per_image > kRcnnMaxRois || L.num_fg < 0 ||
        L.num_fg > L.rois_per_image)
        return;
    const BoxRec  r       = L.t.recs[rec];
    const RcnnRec x       = L.t.ext[rec];
    const int     nchunks = (A + 63) >> 6;
    const float4* anchors = (const float4*)L.anchors;
    const float   im_w = (float)x.im_w, im_h = (float)x.im_h;

    // ---- 0: gt boxes ----
    if (wave == 0) {
        const int32_t* lab     = L.t.labels + r.first;
        const int32_t* dif     = L.t.difficult + r.first;
        float4*        out_box = (float4*)(L.buf[5] + (uint64_t)rec * L.stride[5]);
        int32_t*       out_cls = (int32_t*)(L.buf[7] + (uint64_t)rec * L.stride[7]);
        int32_t*       out_dif = (int32_t*)(L.buf[9] + (uint64_t)rec * L.stride[9]);
        const int      kept    = compact_boxes(
            r, (const float4*)L.t.boxes + r.first, r.count < kRcnnMaxBoxes ? r.count : kRcnnMaxBoxes, L.emit_type,
            L.emit_min_overlap, L.max_gt_boxes, lane,
            [&](int slot, int i, float4 b) {
                s_gt[slot]     = b;
                s_garea[slot]  = (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f);
                s_colmax[slot] = 0u;
                if (slot < L.max_gt_boxes) {
                    out_box[slot] = b;
                    out_cls[slot] = lab[i];
                    out_dif[slot] = dif[i] != 0 ? 1 : 0;
                }
            },
            [&](int s) {
                out_box[s] = make_float4(0.f, 0.f, 0.f, 0.f);
                out_cls[s] = 0;
                out_dif[s] = 0;
            });
        if (lane == 0) {
            s_K            = kept;
            int32_t* shape = (int32_t*)(L.buf[4] + (uint64_t)rec * L.stride[4]);
            shape[0]       = x.im_w;
            shape[1]       = x.im_h;
            *(int32_t*)(L.buf[6] + (uint64_t)rec * L.stride[6]) = kept < L.max_gt_boxes ? kept : L.max_gt_boxes;
            *(float*)(L.buf[8] + (uint64_t)rec * L.stride[8])   = x.im_scale;
        }
    }
    __syncthreads();
    const int K = s_K;

    // ---- 1: column maxima over the inside anchors ----
    if (K > 0) {
        for (int a = tid; a < A; a += kThreads) {
            const float4 an = anchors[a];
            if (!inside(an, im_w, im_h)) continue;
            for (int k = 0; k < K; k++) {
                const uint32_t v = __float_as_uint(overlap(an, s_gt[k], s_garea[k]));
                if (v > *(volatile uint32_t*)&s_colmax[k]) atomicMax(&s_colmax[k], v);
            }
        }
    }
    __syncthreads();

    // ---- 2: labels -> bitmaps (with K == 0 aeon labels nothing) ----
    for (int c = wave; c < nchunks; c += kWaves) {
        const int a  = c * 64 + lane;
        bool      fg = false, bg = false;
        if (a < A && K > 0) {
            const float4 an = anchors[a];
            if (inside(an, im_w, im_h)) {
                float row_max = 0.0f;
                bool  tie     = false;
                for (int k = 0; k < K; k++) {
                    const float v = overlap(an, s_gt[k], s_garea[k]);
                    row_max       = row_max < v ? v : row_max;
                    tie           = tie || v == __uint_as_float(s_colmax[k]);
                }
                int label = -1;
                if (row_max < L.negative_overlap) label = 0;
                if (tie) label = 1;
                if (row_max >= L.positive_overlap) label = 1;
                fg = label == 1;
                bg = label == 0;
            }
        }
        const unsigned long long mfg = __ballot(fg), mbg = __ballot(bg);
        if (lane == 0) {
            s_fg[2 * c] = (uint32_t)mfg, s_fg[2 * c + 1] = (uint32_t)(mfg >> 32);
            s_bg[2 * c] = (uint32_t)mbg, s_bg[2 * c + 1] = (uint32_t)(mbg >> 32);
            s_sel[2 * c] = 0u, s_sel[2 * c + 1] = 0u;
            if (c == nchunks - 1) s_sel[2 * c + 2] = 0u;
            s_pfg[c] = __popcll(mfg);
            s_pbg[c] = __popcll(mbg);
        }
    }
    __syncthreads();

    // ---- 3: running counts, then sample_anchors' shuffles on wave 0 ----
    if (wave == 0) {
        int n_fg = 0, n_bg = 0; // wave-uniform
        for (int base = 0; base < nchunks; base += 64) {
            const int i  = base + lane;
            const int cf = i < nchunks ? s_pfg[i] : 0, cb = i < nchunks ? s_pbg[i] : 0;
            int       sf = cf, sb = cb; // inclusive scans
            for (int d = 1; d < 64; d <<= 1) {
                const int tf = __shfl_up(sf, d), tb = __shfl_up(sb, d);
                if (lane >= d) sf += tf, sb += tb;
            }
            if (i < nchunks) s_pfg[i] = n_fg + sf - cf, s_pbg[i] = n_bg + sb - cb;
            n_fg += __shfl(sf, 63);
            n_bg += __shfl(sb, 63);
        }
        // sample_anchors: the wave shuffles the two lists' ranks, keeping the sampled prefixes
        uint32_t apow = 16807u; // 16807^(lane + 1) mod 2^31 - 1
        for (int k = 0; k < lane; k++) apow = mulmod31(apow, 16807u);
        minstd0   g{rcnn_engine_word(x.engine)}; // (the host sends it so; the LCG never leaves 0)
        const int take_fg   = n_fg < L.num_fg ? n_fg : L.num_fg;
        const int remainder = L.rois_per_image - take_fg;
        const int take_bg   = n_bg < remainder ? n_bg : remainder;
        if (L.shuffle) {
            wave_shuffle_prefix((uint32_t)n_fg, (uint32_t)L.num_fg, g, s_ranks, lane, apow);
            wave_shuffle_prefix((uint32_t)n_bg, (uint32_t)remainder, g, s_ranks + take_fg, lane, apow);
        } else {
            for (int i = lane; i < take_fg; i += 64) s_ranks[i] = i;
            for (int i = lane; i < take_bg; i += 64) s_ranks[take_fg + i] = i;
        }
        if (lane == 0) {
            if (L.states_out) L.states_out[rec] = g.x;
            s_take_fg = take_fg;
            s_take_bg = take_bg;
        }
    }
    __syncthreads();

    // ---- 4: ranks -> anchors, marked in s_sel; their targets ----
    const int take_fg = s_take_fg, take = s_take_fg + s_take_bg;
    float*    bbt     = (float*)(L.buf[0] + (uint64_t)rec * L.stride[0]);
    for (int s = tid; s < take; s += kThreads) {
        const bool      is_fg = s < take_fg;
        const int       rank  = s_ranks[s];
        const int32_t*  pref  = is_fg ? s_pfg : s_pbg;
        const uint32_t* words = is_fg ? s_fg : s_bg;
        int lo = 0, hi = nchunks - 1; // the last chunk with at most `rank` anchors before it holds it
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pref[mid] <= rank) lo = mid;
            else hi = mid - 1;
        }
        unsigned long long w = (unsigned long long)words[2 * lo] | ((unsigned long long)words[2 * lo + 1] << 32);
        for (int j = rank - pref[lo]; j > 0; j--) w &= w - 1;
        if (w != 0) {
            const int a = lo * 64 + (__ffsll((long long)w) - 1);
            atomicOr(&s_sel[a >> 5], 1u << (a & 31));
            // compute_targets against the first gt box attaining the anchor's row maximum
            const float4 an  = anchors[a];
            int          idx = 0;
            float        mx  = 0.0f;
            for (int k = 0; k < K; k++) {
                const float v = overlap(an, s_gt[k], s_garea[k]);
                if (v > mx) idx = k, mx = v;
            }
            const float4 g  = s_gt[idx];
            const float  aw = an.z - an.x + 1.0f, ah = an.w - an.y + 1.0f;
            bbt[a]          = (center(g.x, g.z) - center(an.x, an.z)) / aw;
            bbt[a + A]      = (center(g.y, g.w) - center(an.y, an.w)) / ah;
            bbt[a + 2 * A]  = logf((g.z - g.x + 1.0f) / aw);
            bbt[a + 3 * A]  = logf((g.w - g.y + 1.0f) / ah);
        }
    }
    __syncthreads();

    // ---- 5: the four big buffers, every element but the sampled anchors' targets ----
    auto fg_sampled = [&](int i) { return bit(s_sel, i) && bit(s_fg, i); };
    // four consecutive elements of one plane with no sampled anchor among them: the fill value alone
    auto clean4 = [&](int e) {
        int i = e;
        while (i >= A) i -= A;
        if (i + 3 >= A) return false;
        const int                wd = i >> 5;
        const unsigned long long w  = (unsigned long long)s_sel[wd] | ((unsigned long long)s_sel[wd + 1] << 32);
        return ((w >> (i & 31)) & 0xFull) == 0;
    };
    auto zeros4 = [&](int e, uint4& q) {
        q = make_uint4(0u, 0u, 0u, 0u);
        return clean4(e);
    };
    auto sampled_at = [&](int e) {
        int i = e;
        while (i >= A) i -= A;
        return bit(s_sel, i);
    };
    auto never = [](int) { return false; };
    fill_words((uint32_t*)bbt, 4 * A, tid, [](int) -> uint32_t { return 0u; }, zeros4, sampled_at);
    fill_words((uint32_t*)(L.buf[1] + (uint64_t)rec * L.stride[1]), 4 * A, tid, [&](int e) -> uint32_t {
        int i = e;
        while (i >= A) i -= A;
        return fg_sampled(i) ? __float_as_uint(1.0f) : 0u;
    }, zeros4, never);
    fill_words((uint32_t*)(L.buf[2] + (uint64_t)rec * L.stride[2]), 2 * A, tid, [&](int e) -> uint32_t {
        return e < A ? (fg_sampled(e) ? 0u : 1u) : (fg_sampled(e - A) ? 1u : 0u);
    }, [&](int e, uint4& q) {
        const uint32_t f = e < A ? 1u : 0u; // (clean4 is false for four elements across the halves)
        q = make_uint4(f, f, f, f);
        return clean4(e);
    }, never);
    fill_words((uint32_t*)(L.buf[3] + (uint64_t)rec * L.stride[3]), 2 * A, tid,
               [&](int e) -> uint32_t { return sampled_at(e) ? 1u : 0u; }, zeros4, never);
}

} // namespace

hipError_t launch_rcnn_targets(const RcnnLaunch& L, hipStream_t stream)
{
    if (L.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rcnn_targets, dim3((unsigned)L.n), dim3(kThreads), 0, stream, L);
    return hipGetLastError();
}

} // namespace aeon_hip
