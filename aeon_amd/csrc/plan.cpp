// plan.cpp -- the image path's planner (plan.hpp): per-record planning, launch shapes, and the layout
// of a call's job table and scratch.  Host arithmetic only; built with -ffp-contract=off so every
// float/double expression rounds as aeon's x86 build does.
#include "plan.hpp"

#include <cfloat>
#include <string>

#include "param_factory.hpp"

namespace aeon_hip {

// launch-shape constants (compile-time overrides only for tuning builds, tools/build_variants.sh)
#ifndef AEON_HIP_STAGE_BUDGET_KB
#define AEON_HIP_STAGE_BUDGET_KB 48
#endif
constexpr int kStageBudget   = AEON_HIP_STAGE_BUDGET_KB * 1024; // preferred LDS bytes of the staging buffer
constexpr int kStageBudgetHi = 140 * 1024;  // fallback for very wide crops

template <typename J_>
void LaunchPlan::shape(const std::vector<J_>& jobs)
{
    int ww = 0;
    for (const J_& J : jobs) ww = std::max(ww, J.win_w);
    max_win_w = std::max(ww, 1);
    // workgroup = 256..512 lanes holding whole 4-pixel column groups (fewest idle lanes;
    // ties go to the larger group), row phases = lanes / column groups
    const int gpr = (max_win_w + 3) / 4;
    const int ncg = std::min(gpr, kBlockMax);
    threads       = kBlockMax;
    int best_idle = kBlockMax;
    for (int nt = kBlockMin; nt <= kBlockMax; nt += 64) {
        const int idle = nt - (nt / ncg) * ncg;
        // idle / nt <= best_idle / threads
        if ((long)idle * threads <= (long)best_idle * nt) threads = nt, best_idle = idle;
    }
    // contrast pass 2 (photometric over the u8 intermediate, no resize): full workgroups
    // beat the fewest-idle-lanes choice (C3: 140 vs 158 us at 512 vs 448 lanes)
    if (rm == RESIZE_COPY && photo) threads = kBlockMax;
    const int nph = threads / ncg;
    // one staging buffer and four rows per lane (a multiple of the row phases): the CU's other
    // workgroups cover a tile's staging latency.  Measured on C2/C3 against two buffers
    // (the next tile's loads in flight during the current tile's compute) at two rows per
    // lane: 42 vs 45 us (C2), 152/291 vs 186/370 us (C3 pass 2 / pass 1) -- the second
    // buffer costs occupancy and halves the rows per tile (rejected).
    const int tr_cap = std::min(64, std::max(1, 4 * nph));
    int       budget = kStageBudget;
    bool hue = false, contrast = false;
    for (const J_& J : jobs) {
        hue |= (J.photo & PHOTO_HUE) != 0;
        contrast |= (J.photo & PHOTO_CONTRAST) != 0 && J.stats_slot >= 0;
    }
    has_hue = hue, has_contrast = contrast;
    for (int pass = 0; pass < 2; pass++) {
        for (int t = tr_cap; t >= 1; t--) {
            // staged rows, each in whole DMA instructions (stage_bytes_for)
            long by = 0;
            for (const J_& J : jobs) by = std::max(by, stage_bytes_for(J.cn, stage_rows_for(J, t), stage_cols(J)));
            by = (by + 1023) / 1024 * 1024;
            if (by <= budget || (t == 1 && pass == 1)) {
                tr = t, stage_bytes = (int)by;
                goto chosen;
            }
        }
        budget = kStageBudgetHi;
    }
chosen:
    lds = lds_layout(max_win_w, tr, stage_bytes, photo && hue, rtab).total;
    if (lds > kMaxLds)
        fail(AEON_HIP_EUNSUPPORTED, "source crop too wide for LDS-staged row bands (" + std::to_string(lds) +
                                        " bytes)");
}
template void LaunchPlan::shape(const std::vector<AugJob>&);
template void LaunchPlan::shape(const std::vector<JobGeom>&);

// Geometry + constants of one image-provider record (transform_single_image).
// image::rotate (src/image.cpp:53-75): cv::getRotationMatrix2D(Point2i(cols/2, rows/2), angle, 1)
// inverted the way cv::warpAffine does without WARP_INVERSE_MAP (OpenCV 2.4 imgwarp.cpp); double
// arithmetic on the host, as aeon's.
static void rotation_inverse_map(int w, int h, int angle, double M[6])
{
    const float  cx = (float)(w / 2), cy = (float)(h / 2); // Point2i -> Point2f
    const double a  = (double)angle * (3.1415926535897932384626433832795 / 180);
    const double alpha = std::cos(a) * 1.0, beta = std::sin(a) * 1.0;
    M[0] = alpha, M[1] = beta, M[2] = (1 - alpha) * cx - beta * cy;
    M[3] = -beta, M[4] = alpha, M[5] = beta * cx + (1 - alpha) * cy;
    double D = M[0] * M[4] - M[1] * M[3];
    D        = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11;
    M[1] *= -D;
    M[3] *= -D;
    M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1, M[5] = b2;
}

// A single-channel pixel-mask / depth-map record, 16-bit (CV_16U, ANYDEPTH) or rotation-free
// 8-bit: crop -> INTER_NEAREST -> flip -> convertTo (etl_pixel_mask.cpp:65-92,
// etl_depthmap.cpp:65-96, image.cpp:176-212), one gather pass (mask16_kernels.hip).
void CallPlan::add_gather(const aeon_img_desc& d, const void* src_base, const aeon_aug_params& p, const aeon_out_desc& o,
                          uint64_t item, bool is_mask)
{
    const int eb = d.elem_bytes == 2 ? 2 : 1;
    if (!is_mask) fail(AEON_HIP_EUNSUPPORTED, "16-bit sources are implemented for pixel masks / depth maps only");
    if (d.channels != 1 || o.channels != 1) fail(AEON_HIP_EINVAL, "16-bit masks must have one channel");
    if (d.width <= 0 || d.height <= 0 || d.stride < d.width * eb || (eb == 2 && ((d.stride & 1) || (d.offset & 1))))
        fail(AEON_HIP_EINVAL, eb == 2 ? "invalid 16-bit source image descriptor" : "invalid source image descriptor");
    if (p.out_w <= 0 || p.out_h <= 0) fail(AEON_HIP_EINVAL, "invalid output size");
    const size_t elem = out_elem_bytes(o.dtype);
    if ((size_t)p.out_w * p.out_h * elem > o.item_stride) fail(AEON_HIP_EINVAL, "output item does not fit item_stride");
    if (o.fixed_aspect_ratio && (p.out_w > o.canvas_w || p.out_h > o.canvas_h))
        fail(AEON_HIP_EINVAL, "fixed_aspect_ratio: output_size larger than the image canvas");
    if (p.crop_x < 0 || p.crop_y < 0 || p.crop_w <= 0 || p.crop_h <= 0 || p.crop_x + p.crop_w > d.width ||
        p.crop_y + p.crop_h > d.height)
        fail(AEON_HIP_EINVAL, "cropbox outside image");
    Mask16Job M{};
    M.scale_x    = 1. / ((double)p.out_w / p.crop_w);
    M.scale_y    = 1. / ((double)p.out_h / p.crop_h);
    M.src_ptr    = (uint64_t)((const uint8_t*)src_base + d.offset);
    M.out_ptr    = item;
    M.src_stride = d.stride;
    M.crop_x = p.crop_x, M.crop_y = p.crop_y, M.crop_w = p.crop_w, M.crop_h = p.crop_h;
    M.out_w = p.out_w, M.out_h = p.out_h;
    M.out_pitch = o.fixed_aspect_ratio ? o.canvas_w : p.out_w;
    M.flip      = p.flip ? 1 : 0;
    M.dtype     = o.dtype;
    M.src_elem  = eb;
    if (p.angle != 0) {
        // image::rotate(..., interpolate = false, border 0) (etl_pixel_mask.cpp:72-74,
        // etl_depthmap.cpp:72-73): nearest moves whole elements, so a 16-bit record rotates as a
        // 2-byte-per-pixel one; the gather pass then reads the rotated copy in the slot scratch
        // only the cropbox window of the rotated record is produced (the gather reads nothing else)
        const RotJob& R = rotate(d, M.src_ptr, p, eb, AEON_INTERP_NEAREST, true);
        M.src_ptr       = R.out_ptr;
        M.src_scratch   = 1;
        M.src_stride    = R.ow * eb;
        M.crop_x = M.crop_y = 0;
    }
    m16.push_back(M);
}

// Checks of one 8-bit record aeon's transformer would throw on (or that this stage refuses).
void validate_record(const aeon_img_desc& d, const aeon_aug_params& p, const aeon_out_desc& o, bool is_mask)
{
    const int cn = d.channels;
    if (cn != 1 && cn != 3) fail(AEON_HIP_EINVAL, "channels must be 1 or 3");
    if (cn != o.channels) fail(AEON_HIP_EINVAL, "decoded channels do not match the output config");
    if (d.width <= 0 || d.height <= 0 || d.stride < d.width * cn)
        fail(AEON_HIP_EINVAL, "invalid source image descriptor");
    const int interp = is_mask ? AEON_INTERP_NEAREST : p.interp;
    if (interp < AEON_INTERP_LINEAR || interp > AEON_INTERP_LANCZOS4) fail(AEON_HIP_EINVAL, "unknown interpolation");
    if (p.out_w <= 0 || p.out_h <= 0) fail(AEON_HIP_EINVAL, "invalid output size");
    const size_t elem = out_elem_bytes(o.dtype);
    if ((size_t)p.out_w * p.out_h * cn * elem > o.item_stride)
        fail(AEON_HIP_EINVAL, "output item does not fit item_stride");
    if (o.fixed_aspect_ratio && (p.out_w > o.canvas_w || p.out_h > o.canvas_h))
        fail(AEON_HIP_EINVAL, "fixed_aspect_ratio: output_size larger than the image canvas");
    int base_w = d.width, base_h = d.height;
    if (!is_mask && expands(p)) { // image::expand throws on a record that does not fit the canvas
        if (p.expand_x < 0 || p.expand_y < 0 || p.expand_x + d.width > p.expand_w || p.expand_y + d.height > p.expand_h)
            fail(AEON_HIP_EINVAL, "Invalid parameters to expand image");
        base_w = p.expand_w, base_h = p.expand_h;
    }
    if (!is_mask && p.resize_short_size > 0) get_resized_short_size(base_w, base_h, p.resize_short_size, &base_w, &base_h);
    if (p.crop_x < 0 || p.crop_y < 0 || p.crop_w <= 0 || p.crop_h <= 0 || p.crop_x + p.crop_w > base_w ||
        p.crop_y + p.crop_h > base_h)
        fail(AEON_HIP_EINVAL, (is_mask || p.resize_short_size <= 0) && !(!is_mask && expands(p))
                                  ? "cropbox outside image"
                                  : "cropbox outside the expanded / resize_short image");
    if (!is_mask && photo_flags(p) && cn != 3) fail(AEON_HIP_EINVAL, "photometric augmentation needs a 3-channel image");
    if (!is_mask && (p.n_lighting != 0 && p.n_lighting != 3)) fail(AEON_HIP_EINVAL, "lighting needs 3 values");
}

OutView out_view(const aeon_out_desc& o)
{
    OutView v;
    v.ko = o;
    if (o.fixed_aspect_ratio && o.dtype != AEON_DTYPE_U8) {
        v.ko.dtype    = AEON_DTYPE_U8;
        v.ko.has_mean = 0;
        v.u8_map      = o.has_mean != 0;
    }
    return v;
}

// The cv::resize of a (sw x sh -> dw x dh) resize with interpolation `interp` when the tile kernel
// has no mode for it: a resize_generic method (CUBIC, LANCZOS4, INTER_AREA but its exact 2x box), or
// -1 -- LINEAR / NEAREST, any identity (every method reproduces the source at scale 1) and INTER_AREA's
// 2x fast path (RESIZE_AREA2X, the same (a+b+c+d+2)>>2).  OpenCV 2.4.9 cv::resize's dispatch.
static int generic_method(int sw, int sh, int dw, int dh, int interp, int cn, int* isx, int* isy)
{
    if (interp != AEON_INTERP_CUBIC && interp != AEON_INTERP_AREA && interp != AEON_INTERP_LANCZOS4) return -1;
    if (sw == dw && sh == dh) return -1;
    if (interp == AEON_INTERP_CUBIC) return GR_CUBIC;
    if (interp == AEON_INTERP_LANCZOS4) return GR_LANCZOS4;
    const double sx = 1. / ((double)dw / sw), sy = 1. / ((double)dh / sh);
    if (sx < 1 || sy < 1) return GR_LINEAR_AREA; // an upscaled axis: bilinear over area-mode coefficients
    const int ix = cv_round(sx), iy = cv_round(sy);
    if (std::fabs(sx - ix) < DBL_EPSILON && std::fabs(sy - iy) < DBL_EPSILON) {
        if (ix == 2 && iy == 2 && (cn == 1 || cn == 3)) return -1;
        *isx = ix, *isy = iy;
        return GR_AREA_FAST;
    }
    return GR_AREA;
}

// The host half of interpolateLanczos4 (OpenCV 2.4.9 imgwarp.cpp) for destinations [d0, d0 + n) of an
// ssize -> dsize axis (x: the anchor clamped as cv::resize does for columns; y: raw, the rows clipped
// per tap on use): the anchor, the fraction and the double sin / cos of the C library as OpenCV's --
// the one part a device could not reproduce bit for bit.  The coefficients are finished on the device
// (lanczos4_taps, resize_kernels.hip).
static void lanczos4_inputs(int ssize, double scale, int d0, int n, bool clamp, LzIn* out)
{
    const double kPi = 3.1415926535897932384626433832795;
    for (int d = d0; d < d0 + n; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int   s = (int)std::floor(f);
        f -= (float)s;
        if (clamp && s < 0) f = 0, s = 0;
        if (clamp && s >= ssize - 1) f = 0, s = ssize - 1;
        LzIn L{0.0, 0.0, f, s};
        if (!(f < FLT_EPSILON)) {
            // sin / cos of a function of the float f alone: memoised per thread.  A batch's fractions are
            // few (integer crop sizes over a common output size: multiples of 1 / (2 * size), rounded to
            // float), so a 256-record LANCZOS4 call computes a few thousand pairs instead of 115 K (the
            // host side was the C2:LANCZOS4 step's bound).  Same libm calls on the same doubles: the
            // same bits.
            struct Entry {
                uint32_t key; // float bits + 1 (0: empty)
                double   s, c;
            };
            static thread_local std::vector<Entry> memo(1 << 14);
            uint32_t bits;
            std::memcpy(&bits, &f, 4);
            Entry& e = memo[(bits * 2654435761u) >> 18];
            if (e.key != bits + 1) {
                const double y0 = -(f + 3) * kPi * 0.25;
                e               = Entry{bits + 1, std::sin(y0), std::cos(y0)};
            }
            L.s0 = e.s, L.c0 = e.c;
        }
        out[d - d0] = L;
    }
}

int32_t GrPlan::axis_taps(int ssize, double scale, int d0, int n, bool clamp)
{
    LzAxis a{ssize, d0, n, clamp ? 1 : 0, 0};
    std::memcpy(&a.scale_bits, &scale, 8);
    auto it = lz_index.find(a);
    if (it == lz_index.end()) {
        it = lz_index.emplace(a, n_taps).first;
        lz_axes.emplace_back(a, n_taps);
        n_taps += n;
    }
    return (int32_t)(it->second * sizeof(GrTap));
}

void GrPlan::add(ResizeJob R)
{
    if (R.method == GR_LANCZOS4) { // byte offsets, relative until the table is laid out
        n_taps_max += (size_t)R.win_w + R.win_h;
        R.coef_x = axis_taps(R.crop_w, R.scale_x, R.win_x, R.win_w, true);
        R.coef_y = axis_taps(R.crop_h, R.scale_y, R.win_y, R.win_h, false);
    }
    jobs.push_back(R);
}

void GrPlan::fill_taps(const ParallelFor& pool, LzIn* lz) const
{
    auto one = [&](int i) {
        const LzAxis& a = lz_axes[i].first;
        double        scale;
        std::memcpy(&scale, &a.scale_bits, 8);
        lanczos4_inputs(a.ssize, scale, a.d0, a.n, a.clamp != 0, lz + lz_axes[i].second);
    };
    if (pool && n_taps > 4096) pool((int)lz_axes.size(), one);
    else for (int i = 0; i < (int)lz_axes.size(); i++) one(i);
}

// rows of H a tile of `tr` output rows needs at most (jobs [f, f + n))
int GrPlan::rows_for(int f, int n, int tr) const
{
    int nr = 1;
    for (int i = f; i < f + n; i++) {
        const ResizeJob& R = jobs[i];
        if (R.method == GR_AREA) nr = std::max(nr, (int)std::ceil(tr * R.scale_y) + 3);
        else if (R.method != GR_AREA_FAST) nr = std::max(nr, (int)std::ceil((tr - 1) * R.scale_y) + ksize(R.method) + 2);
    }
    return nr;
}
// staged source bytes per row a tile of `cw` output columns needs at most (a multiple of 4)
int GrPlan::bytes_for(int f, int n, int cw) const
{
    int sw = 4;
    for (int i = f; i < f + n; i++) {
        const ResizeJob& R = jobs[i];
        int              cols = 1;
        if (R.method == GR_AREA) cols = (int)std::ceil(cw * R.scale_x) + 4;
        else if (R.method != GR_AREA_FAST) cols = (int)std::ceil((cw - 1) * R.scale_x) + ksize(R.method) + 2;
        sw = std::max(sw, (std::min(cols, R.crop_w) * R.cn + 3) / 4 * 4);
    }
    return sw;
}
// the launch shape of jobs [f, f + n): resize_sep when they are one fixed-K class of one channel
// count and a band fits, else resize_generic
GrPlan::Sub GrPlan::shape(int f, int n) const
{
    Sub u;
    u.first = f, u.count = n;
    for (int i = f; i < f + n; i++) u.any_final = u.any_final || jobs[i].final_out;
    const size_t lut_lds = u.any_final ? 768 * 4 : 0;
    int          K = 2, ww = 1;
    for (int i = f; i < f + n; i++) {
        const ResizeJob& R = jobs[i];
        K = std::max(K, ksize(R.method));
        if (R.method == GR_AREA) u.amax = std::max(u.amax, (int)std::ceil(std::max(R.scale_x, R.scale_y)) + 3);
        u.cn_max = std::max(u.cn_max, R.cn);
        ww       = std::max(ww, R.win_w);
    }
    // resize_sep: bands of up to 32 rows x the window's width (at most 256 lanes of 4 bytes); resizeArea_
    // jobs as its INTER_AREA form, K = their most taps per destination index (floor(scale) + 2)
    int ka = 0;
    if (jobs[f].method == GR_AREA) {
        double smax = 1;
        for (int i = f; i < f + n; i++) smax = std::max({smax, jobs[i].scale_x, jobs[i].scale_y});
        const int taps = (int)std::floor(smax) + 2;
        ka             = taps <= 4 ? 4 : taps <= 8 ? 8 : 0;
    }
    const int sk  = ka ? ka : sep_k(jobs[f].method);
    const int xs  = (ka ? 2 : 1) + sk;
    bool      one = sk != 0;
    for (int i = f; i < f + n; i++) one = one && jobs[i].method == jobs[f].method && jobs[i].cn == u.cn_max;
    if (one) {
        // a band's lanes (at most 256): 4 bytes of a u8 window row each, or 4 pixels of one channel of a
        // final_out job each -- cn * ceil(cw / 4) lanes, so 340 columns for 3 channels, not 341
        int cw = std::min({ww, 1024 / u.cn_max, 4 * (256 / u.cn_max)}), tr = 16;
        // staged rows: whole 16-byte blocks (resize_sep), hence up to 30 bytes more per row, and 32
        // bytes of room for the replicated borders (resize_kernels.hip kSepPadL)
        auto sw = [&] { return (bytes_for(f, n, cw) + 30 + 15) / 16 * 16 + 32; };
        auto l  = [&] {
            return ((size_t)(cw + tr) * xs * 4 + 15) / 16 * 16 + (size_t)rows_for(f, n, tr) * sw() + lut_lds;
        };
        while (l() > kSepLds && tr > 4) tr /= 2;
        if (l() <= kSepLds) {
            u.sep = sk, u.area = ka != 0, u.TR = tr, u.CW = cw, u.NR = rows_for(f, n, tr), u.SW = sw(), u.xs = xs;
            return u;
        }
    }
    u.xs = std::max(1 + K, 2 + u.amax);
    u.CW = std::min(128, ww);
    u.TR = 16;
    // with the source rows staged in LDS (SW > 0) when they fit at 16 x 128 tiles, else without
    bool staged = true;
    auto lds    = [&] {
        return ((size_t)u.CW * u.xs + (size_t)u.TR * u.xs + (size_t)rows_for(f, n, u.TR) * u.CW * u.cn_max) * 4 +
               (staged ? (size_t)rows_for(f, n, u.TR) * bytes_for(f, n, u.CW) : 0) + lut_lds;
    };
    staged = lds() <= kGenericLds;
    while (lds() > kGenericLds && u.TR > 1) u.TR--;
    while (lds() > kGenericLds && u.CW > 8) u.CW /= 2;
    if (lds() > kGenericLds) fail(AEON_HIP_EUNSUPPORTED, "resize scale too large for the generic resize's LDS tiles");
    u.NR = rows_for(f, n, u.TR);
    u.SW = staged ? bytes_for(f, n, u.CW) : 0;
    return u;
}
void GrPlan::finalize()
{
    subs.clear();
    bytes = 0;
    if (jobs.empty()) return;
    // the classes contiguous: resize_sep's by K, resizeArea_'s, then the other generic methods
    std::stable_sort(jobs.begin(), jobs.end(), [](const ResizeJob& a, const ResizeJob& b) { return cls(a.method) < cls(b.method); });
    for (int f = 0; f < (int)jobs.size();) {
        int e = f + 1;
        while (e < (int)jobs.size() && cls(jobs[e].method) == cls(jobs[f].method)) e++;
        subs.push_back(shape(f, e - f));
        f = e;
    }
    for (Sub& u : subs) {
        u.max_tiles = 0;
        for (int i = u.first; i < u.first + u.count; i++) {
            ResizeJob& R = jobs[i];
            R.tiles_x    = (R.win_w + u.CW - 1) / u.CW;
            R.tiles      = R.tiles_x * ((R.win_h + u.TR - 1) / u.TR);
            u.max_tiles  = std::max(u.max_tiles, R.tiles);
            bytes += (double)R.crop_w * R.crop_h * R.cn * ((double)R.win_w / R.dst_w) * ((double)R.win_h / R.dst_h) +
                     (double)R.win_w * R.win_h * R.cn * (R.final_out ? 4 : 1);
        }
    }
}

// A resize of the (cropped, padded) region of J's source to its window; the caller says where it writes.
static ResizeJob resize_job(const AugJob& J, int method, int isx, int isy)
{
    ResizeJob R{};
    R.scale_x = J.scale_x, R.scale_y = J.scale_y;
    R.inv_x = (double)J.dst_w / J.crop_w, R.inv_y = (double)J.dst_h / J.crop_h;
    R.src_ptr = J.src_ptr, R.src_scratch = J.src_scratch;
    R.src_stride = J.src_stride, R.cn = J.cn;
    R.crop_x = J.crop_x, R.crop_y = J.crop_y, R.crop_w = J.crop_w, R.crop_h = J.crop_h;
    R.shift_x = J.shift_x, R.shift_y = J.shift_y, R.padded = J.padded;
    R.dst_w = J.dst_w, R.dst_h = J.dst_h;
    R.win_x = J.win_x, R.win_y = J.win_y, R.win_w = J.win_w, R.win_h = J.win_h;
    R.method = method, R.isx = isx, R.isy = isy;
    return R;
}

size_t CallPlan::reserve(size_t bytes)
{
    const size_t off = (scratch_bytes + 15) & ~(size_t)15;
    scratch_bytes    = off + bytes + 16;
    return off;
}

// image::rotate of record d (cn bytes per pixel at src) into scratch: its cropbox window, or all of it
const RotJob& CallPlan::rotate(const aeon_img_desc& d, uint64_t src, const aeon_aug_params& p, int cn, int interp, bool window)
{
    RotJob R{};
    rotation_inverse_map(d.width, d.height, p.angle, R.M);
    R.src_ptr = src;
    R.w = d.width, R.h = d.height, R.stride = d.stride, R.cn = cn;
    R.interp = interp;
    R.ox = window ? p.crop_x : 0, R.oy = window ? p.crop_y : 0;
    R.ow = window ? p.crop_w : d.width, R.oh = window ? p.crop_h : d.height;
    R.out_ptr = reserve((size_t)R.ow * R.oh * cn);
    R.angle   = p.angle;
    rot.push_back(R);
    return rot.back();
}

// J's source is from here on the w x h x cn HWC copy an earlier launch leaves in scratch at `off` ...
static void reads_scratch(AugJob& J, size_t off, int w, int h, int cn)
{
    J.src_ptr     = off;
    J.src_scratch = 1;
    J.src_bytes   = (uint64_t)w * h * cn;
    J.src_w = w, J.src_h = h, J.src_stride = w * cn;
}
// ... and J a copy pass over its own window there: cropped, padded and resized already
static void copy_pass(AugJob& J, size_t off, int cn)
{
    reads_scratch(J, off, J.win_w, J.win_h, cn);
    J.crop_x = J.crop_y = 0, J.crop_w = J.win_w, J.crop_h = J.win_h;
    J.shift_x = J.shift_y = J.padded = 0;
    J.mode    = RESIZE_COPY;
    J.scale_x = J.scale_y = 1.0;
    J.xv      = simd_boundary(J.win_w * cn);
}

// J into its pass's group: by (resize mode, scalar tail), the final pass by photometric as well
void CallPlan::push(int pass, const AugJob& J)
{
    const int tail = J.mode == RESIZE_LINEAR && J.xv < J.dst_w * J.cn;
    const int g    = pass == kMain ? J.mode * 4 + tail * 2 + (J.photo ? 1 : 0) : J.mode * 2 + tail;
    tiles[pass + g].jobs.push_back(J);
}

void CallPlan::add(const aeon_img_desc& d, const void* src_base, const aeon_aug_params& p, const aeon_out_desc& o, uint64_t item,
                   bool is_mask, const ItemMap* im)
{
    // pixel masks without rotation (and every 16-bit record): the NEAREST gather pass
    const bool eight = d.elem_bytes == 0 || d.elem_bytes == 1;
    if (d.elem_bytes == 2 || (is_mask && d.channels == 1 && o.channels == 1 && p.angle == 0 && eight))
        return add_gather(d, src_base, p, o, item, is_mask);
    if (!eight) fail(AEON_HIP_EINVAL, "elem_bytes must be 1 (CV_8U) or 2 (CV_16U)");
    validate_record(d, p, o, is_mask);
    const int cn = d.channels;
    AugJob    J;
    plan_direct(d, (uint64_t)src_base, p, out_geom(o, im), item, is_mask, J);
    if (p.angle != 0) {
        // image::rotate into scratch (interpolated for images, nearest + border 0 for pixel
        // masks, etl_pixel_mask.cpp:72-74); everything after reads the rotated record
        // Only the cropbox window is produced when nothing before the crop needs the whole rotated
        // record (no expand canvas, no resize_short of it); the job then crops it at (0, 0).
        const bool    window = is_mask || (!expands(p) && p.resize_short_size <= 0);
        const RotJob& R = rotate(d, J.src_ptr, p, cn, is_mask ? AEON_INTERP_NEAREST : AEON_INTERP_LINEAR, window);
        reads_scratch(J, R.out_ptr, R.ow, R.oh, cn);
        J.crop_x -= R.ox, J.crop_y -= R.oy;
    }
    if (!is_mask && expands(p)) {
        // image::expand (image.cpp:276-303) into scratch: a zeroed expand_w x expand_h canvas with the
        // (rotated) record at (expand_x, expand_y); everything after reads the canvas
        ExpandJob E{};
        E.src_ptr     = J.src_ptr;
        E.src_scratch = J.src_scratch;
        E.w = J.src_w, E.h = J.src_h, E.stride = J.src_stride, E.cn = cn;
        E.ew = p.expand_w, E.eh = p.expand_h, E.ox = p.expand_x, E.oy = p.expand_y;
        E.out_ptr = reserve((size_t)E.ew * E.eh * cn);
        exp.push_back(E);
        reads_scratch(J, E.out_ptr, E.ew, E.eh, cn);
    }
    if (!is_mask && p.resize_short_size > 0) {
        // image::resize_short (image.cpp:118-127) into a device scratch, cropbox window only
        const int bw = J.src_w, bh = J.src_h; // the (rotated, expanded) record
        int       rw, rh;
        get_resized_short_size(bw, bh, p.resize_short_size, &rw, &rh);
        AugJob P = J;
        P.photo   = 0;
        P.flip    = 0;
        P.shift_x = P.shift_y = P.padded = 0;
        P.crop_x = 0, P.crop_y = 0, P.crop_w = bw, P.crop_h = bh;
        P.mode    = choose_mode(bw, bh, rw, rh, p.interp, cn);
        P.scale_x = 1. / ((double)rw / bw);
        P.scale_y = 1. / ((double)rh / bh);
        P.dst_w = rw, P.dst_h = rh;
        P.win_x = p.crop_x, P.win_y = p.crop_y, P.win_w = p.crop_w, P.win_h = p.crop_h;
        P.xv      = simd_boundary(rw * cn);
        P.out_ptr = reserve((size_t)p.crop_w * p.crop_h * cn);
        int       isx = 0, isy = 0;
        const int gm  = generic_method(bw, bh, rw, rh, p.interp, cn, &isx, &isy);
        if (gm >= 0) {
            ResizeJob R   = resize_job(P, gm, isx, isy);
            R.out_ptr     = P.out_ptr;
            R.out_scratch = 1;
            gr_short.add(R);
        } else {
            push(P.win_w > kWideCols ? kWide : kPre, P);
        }
        reads_scratch(J, P.out_ptr, p.crop_w, p.crop_h, cn);
        J.crop_x = 0, J.crop_y = 0;
    }
    int       isx = 0, isy = 0;
    int       gm  = is_mask ? -1 : generic_method(J.crop_w, J.crop_h, J.dst_w, J.dst_h, p.interp, cn, &isx, &isy);
    const bool final_ok = J.photo == 0 && o.dtype == AEON_DTYPE_F32 && !o.fixed_aspect_ratio && (cn == 1 || cn == 3) &&
                          o.channels == cn;
    // An identity resize (cv::resize copies) of a CUBIC / LANCZOS4 / INTER_AREA call with no photometric
    // stage and f32 output: through the call's resize class with identity taps -- (0, 2048, 0, 0), the
    // fraction-0 Lanczos row, the bilinear emulation's (2048, 0), each reproducing the byte exactly -- so
    // the call launches no tile kernel for its few uncropped records (an 8.5 us launch per C2:<method>
    // step: one tile's latency).
    if (gm < 0 && !is_mask && final_ok && J.crop_w == J.dst_w && J.crop_h == J.dst_h &&
        (p.interp == AEON_INTERP_CUBIC || p.interp == AEON_INTERP_LANCZOS4 || p.interp == AEON_INTERP_AREA))
        gm = p.interp == AEON_INTERP_CUBIC ? GR_CUBIC : p.interp == AEON_INTERP_LANCZOS4 ? GR_LANCZOS4 : GR_LINEAR_AREA;
    if (gm >= 0 && gm != GR_AREA_FAST && final_ok) {
        // no photometric stage and f32 output: the resize pass is the last one -- it flips,
        // standardizes through the LUT and stores the loader's layout itself (no u8 window in scratch,
        // no copy pass)
        ResizeJob R = resize_job(J, gm, isx, isy);
        R.out_ptr   = J.out_ptr;
        R.final_out = 1, R.flip = J.flip, R.out_pitch = J.out_pitch, R.out_plane = J.out_plane;
        gr_main.add(R);
        return;
    }
    if (gm >= 0) {
        // CUBIC / LANCZOS4 / INTER_AREA resize of the (padded) crop into scratch (resize_kernels.hip),
        // then the photometric stages, flip and the loader as a copy pass over it
        ResizeJob R   = resize_job(J, gm, isx, isy);
        R.out_ptr     = reserve((size_t)J.win_w * J.win_h * cn);
        R.out_scratch = 1;
        gr_main.add(R);
        copy_pass(J, R.out_ptr, cn);
    }
    const int photo = J.photo;
    if (photo && J.mode == RESIZE_AREA2X) {
        // 2x-area resize first (resize-only pre-pass into scratch, unflipped), then the
        // photometric stages as a copy pass over it
        AugJob P      = J;
        P.photo       = 0;
        P.flip        = 0;
        P.out_ptr     = reserve((size_t)J.win_w * J.win_h * 3);
        push(kPre2, P);
        copy_pass(J, P.out_ptr, 3);
    }
    if (photo & PHOTO_CONTRAST) {
        // contrast needs the mean of the post-hue image: pass 1 writes that image (HWC
        // uint8, unflipped) and its exact per-chunk sums; pass 2 (this job) reads it back
        AugJob P1     = J;
        P1.flip       = 0;
        P1.photo      = photo & (PHOTO_BS | PHOTO_HUE | PHOTO_CONTRAST);
        P1.stats_slot = n_stats++;
        P1.out_ptr    = reserve((size_t)J.win_w * J.win_h * 3);
        push(kPass1, P1);
        J.stats_slot  = P1.stats_slot;
        copy_pass(J, P1.out_ptr, 3);
        J.photo       = photo & (PHOTO_CONTRAST | PHOTO_LIGHTING);
    }
    if ((J.out_ptr & 15) != 0 || (J.win_w & 3) != 0 || o.fixed_aspect_ratio) vec_ok = false;
    push(kMain, J);
}

template <typename J_>
double launch_bytes(const std::vector<J_>& jobs, int mode, size_t out_elem)
{
    double b = 0;
    for (const J_& J : jobs) {
        double rd = (double)J.crop_w * J.crop_h * J.cn;
        if (J.mode == RESIZE_LINEAR || J.mode == RESIZE_NEAREST) {
            // a window of the resize target reads only its share of the source
            rd *= ((double)J.win_w / J.dst_w) * ((double)J.win_h / J.dst_h);
        }
        double wr = (double)J.win_w * J.win_h * J.cn * (mode == KM_FINAL ? out_elem : 1);
        b += rd + wr;
    }
    return b;
}
template double launch_bytes(const std::vector<AugJob>&, int, size_t);
template double launch_bytes(const std::vector<JobGeom>&, int, size_t);

CallPlan::CallPlan()
{
    for (int g = 0; g < kGroups; g++) {
        LaunchPlan& P = tiles[g];
        const bool pre = g < kMain || g >= kWide; // (a pass into scratch)
        P.rm = pre ? (g & 7) >> 1 : (g - kMain) >> 2;
        P.tail = pre ? (g & 1) != 0 : (g & 2) != 0;
        P.photo = pre ? g >= kPass1 && g < kMain : (g & 1) != 0;
        P.out_scratch = pre;
    }
}

void CallPlan::clear() // (what finalize() sets is read for launches with jobs only, and set again for those)
{
    rot.clear(), exp.clear(), m16.clear();
    for (GrPlan* g : {&gr_short, &gr_main})
        g->jobs.clear(), g->subs.clear(), g->lz_index.clear(), g->lz_axes.clear(), g->n_taps = g->n_taps_max = 0;
    for (LaunchPlan& P : tiles) P.jobs.clear();
    scratch_bytes = 0, n_stats = 0, vec_ok = true;
}

void CallPlan::add_records(int n, const aeon_img_desc* descs, const void* src_base, const aeon_aug_params* params,
                           const aeon_out_desc& o, void* out_dev, bool is_mask, const MaskSet* ms, const ItemMap* im)
{
    for (int i = 0; i < n; i++) add(descs[i], src_base, params[i], o, item_of(im, out_dev, o, i), is_mask, im);
    for (int i = 0; ms && i < n; i++) // the pair call's masks: the gather pass's jobs
        add_gather(ms->descs[i], ms->src_base, params[i], ms->out, (uint64_t)ms->out_dev + (uint64_t)i * ms->out.item_stride, true);
}

void CallPlan::finalize(const aeon_out_desc& o)
{
    size_t     end     = 0; // of the table so far
    const auto section = [&](size_t bytes) { // the next 16-aligned `bytes` of it
        const size_t at = (end + 15) & ~(size_t)15;
        end             = at + bytes;
        return at;
    };
    rot_off = section(rot.size() * sizeof(RotJob));
    m16_off = section(m16.size() * sizeof(Mask16Job));
    exp_off = section(exp.size() * sizeof(ExpandJob));
    for (GrPlan* g : {&gr_short, &gr_main}) { // jobs, then their Lanczos tap inputs
        if (g->jobs.empty()) continue;
        g->finalize();
        g->off    = section(g->jobs.size() * sizeof(ResizeJob));
        g->lz_off = section(g->n_taps * sizeof(LzIn));
    }
    slot_tiles.assign(n_stats, 0);
    partial_stride = 1;
    for (int g = 0; g < kGroups; g++) {
        LaunchPlan& P = tiles[g];
        if (P.jobs.empty()) continue;
        const bool last = g >= kMain && g < kWide;
        P.vec_ok = vec_ok;
        P.rtab   = last && P.photo && (o.dtype == AEON_DTYPE_F32 || out_is_half(o.dtype)); // (an f32 table either way)
        P.finalize();
        P.blob_off = section(P.jobs.size() * sizeof(AugJob));
        for (AugJob& J : P.jobs) {
            if (g >= kPass1 && g < kMain) {
                slot_tiles[J.stats_slot] = J.tiles;
                partial_stride           = std::max(partial_stride, J.tiles * 8); // (tile, wave) sums
            }
            if (last && J.stats_slot >= 0) J.stats_tiles = slot_tiles[J.stats_slot];
        }
    }
    partial_words = std::max<size_t>(4, (size_t)n_stats * partial_stride * 4);
    blob          = section(0);
    // the Lanczos4 taps the device builds: after everything the host writes (not uploaded); the ring sized
    // for them with no axis shared (the shared count varies from call to call, and a ring growth inside a
    // loader's steady state costs ~10-20 ms of allocations)
    for (GrPlan* g : {&gr_short, &gr_main}) {
        if (g->n_taps == 0) continue;
        g->taps_off = section(g->n_taps * sizeof(GrTap));
        for (ResizeJob& R : g->jobs)
            if (R.method == GR_LANCZOS4) R.coef_x += (int32_t)g->taps_off, R.coef_y += (int32_t)g->taps_off;
    }
    table_cap = ring_need = section(0);
    for (GrPlan* g : {&gr_short, &gr_main})
        ring_need += (g->n_taps_max - g->n_taps) * (sizeof(LzIn) + sizeof(GrTap)) + 32;

    exp_max_px = 0;
    for (const ExpandJob& E : exp) exp_max_px = std::max(exp_max_px, E.ew * E.eh);
    m16_max_h = m16_max_w = m16_max_seg = 0;
    m16_bytes = 0;
    for (const Mask16Job& M : m16) {
        m16_max_h = std::max(m16_max_h, M.out_h), m16_max_w = std::max(m16_max_w, M.out_w);
        m16_max_seg = std::max(m16_max_seg, M.crop_w * M.src_elem);
        m16_bytes += (double)M.crop_w * M.crop_h * M.src_elem + (double)M.out_w * M.out_h * out_elem_bytes(M.dtype);
    }
    // distinct source rows of any block of the gather pass: the kernel's own row map
    // (sy = min(floor(y * ify), crop_h - 1), monotonic in y), evaluated at each block's ends
    m16_max_slots = 1;
    if (!m16.empty()) {
        const int srows = mask16_rows(m16_max_w, m16_max_seg);
        for (const Mask16Job& M : m16)
            for (int y0 = 0; y0 < M.out_h; y0 += srows) {
                const auto sy = [&](int y) { return std::min((int)std::floor(y * M.scale_y), M.crop_h - 1); };
                const int  y1 = std::min(y0 + srows, M.out_h) - 1;
                m16_max_slots = std::max(m16_max_slots, std::min(y1 - y0 + 1, sy(y1) - sy(y0) + 1));
            }
    }
    rot_max_tiles = 0, rot_cn = rot.empty() ? 0 : rot[0].cn; // (rotate_tiles)
    for (const RotJob& R : rot) {
        if (R.cn != rot_cn) rot_cn = 0;
        rot_max_tiles = std::max(rot_max_tiles, ((R.ow + 63) / 64) * ((R.oh + 31) / 32));
    }
    mask_only = !m16.empty() && rot.empty() && exp.empty() && gr_short.jobs.empty() && gr_main.jobs.empty();
    for (const LaunchPlan& P : tiles) mask_only = mask_only && P.jobs.empty();
}

// Scratch offsets made addresses: which of a job's pointers are offsets is the job's own property
static void relocate(RotJob& R, uint64_t s) { R.out_ptr += s; }
static void relocate(Mask16Job& M, uint64_t s) { M.src_ptr += M.src_scratch ? s : 0; }
static void relocate(ExpandJob& E, uint64_t s) { E.out_ptr += s, E.src_ptr += E.src_scratch ? s : 0; }
static void relocate(ResizeJob& R, uint64_t s) { R.src_ptr += R.src_scratch ? s : 0, R.out_ptr += R.out_scratch ? s : 0; }
template <typename J_>
static void put(uint8_t* table, size_t off, std::vector<J_>& jobs, uint64_t scratch)
{
    for (J_& J : jobs) relocate(J, scratch);
    if (!jobs.empty()) std::memcpy(table + off, jobs.data(), jobs.size() * sizeof(J_));
}

void CallPlan::write(uint8_t* table, uint64_t scratch, const ParallelFor& pool)
{
    put(table, rot_off, rot, scratch);
    put(table, m16_off, m16, scratch);
    put(table, exp_off, exp, scratch);
    for (GrPlan* g : {&gr_short, &gr_main}) {
        put(table, g->off, g->jobs, scratch);
        if (g->n_taps) g->fill_taps(pool, (LzIn*)(table + g->lz_off));
    }
    for (LaunchPlan& P : tiles) {
        for (AugJob& J : P.jobs) J.src_ptr += J.src_scratch ? scratch : 0, J.out_ptr += P.out_scratch ? scratch : 0;
        if (!P.jobs.empty()) std::memcpy(table + P.blob_off, P.jobs.data(), P.jobs.size() * sizeof(AugJob));
    }
}

} // namespace aeon_hip
