"""The record geometries of the size sweep (tests/test_hip_size_sweep.py) and the planner rules they are chosen
against, restated in Python (tests/test_size_cases.py pins that the lists reach what they claim).

What a record's geometry decides on the device:

  * the tile kernel's workgroup: LaunchPlan::shape (plan.cpp) picks 320..512 lanes by the 4-pixel column
    groups of the widest window and lanes / groups row phases (lanes_and_phases), then up to 4 x phases rows
    per tile (at most 64), fewer when the staged source rows pass 48 KiB of LDS (tile_rows);
  * the store form: float4 / half4 planes need out_w % 4 == 0 and 16-byte aligned items, uint8 planes go
    out as dwords on aligned 4-byte groups, everything else element by element;
  * OpenCV's scalar row tail: simd_boundary(out_w * cn) (plan_record.hpp) is the first element of a row whose
    vertical pass uses the scalar formula; it depends on 3 * out_w mod 16;
  * the staging: 12-byte loads at the crop's byte offset in its row (crop_x * 3 mod 16 for a 16-aligned
    image), re-read byte by byte where a load would cross the end of the source buffer;
  * the resize mode: an identity record (crop = output: planned as RESIZE_LINEAR with identity taps; the
    copy passes behind a pre-pass are RESIZE_COPY), the exact 2x record (RESIZE_AREA2X), else RESIZE_LINEAR;
  * resize_sep / resize_generic (CUBIC, LANCZOS4, INTER_AREA; GrPlan::shape, plan.cpp): column bands of
    sep_band_columns(cn) = 340 / 1024 columns, simd_end(ksize, W) as the vertical pass's own SIMD boundary
    (resize_kernels.hip), and for INTER_AREA the class of a call (area_class): the bilinear emulation on an
    upscaled axis, the integer-box fast path, K = floor(max scale) + 2 taps as resize_sep's K = 4 or K = 8
    form, resize_generic above that.

The restatements follow the C++ line by line (integer division where it divides integers, doubles where it
uses doubles); none of them is used to compute an expected pixel.
"""
import math
from collections import namedtuple

import numpy as np

# ---- the planner rules, restated ------------------------------------------------------------------------------
BLOCK_MIN, BLOCK_MAX = 256, 512  # aug_job.hpp kBlockMin / kBlockMax
STAGE_BUDGET, STAGE_BUDGET_HI = 48 * 1024, 140 * 1024  # plan.cpp kStageBudget / kStageBudgetHi
JOB_BYTES = 256  # sizeof(AugJob)

LINEAR, NEAREST, AREA2X = "linear", "nearest", "area2x"


def lanes_and_phases(max_win_w, copy_photo=False):
    """LaunchPlan::shape: (lanes of the workgroup, row phases) for a launch whose widest window is max_win_w
    (copy_photo: a RESIZE_COPY + photometric launch takes full workgroups)."""
    gpr = (max(max_win_w, 1) + 3) // 4
    ncg = min(gpr, BLOCK_MAX)
    threads, best_idle = BLOCK_MAX, BLOCK_MAX
    for nt in range(BLOCK_MIN, BLOCK_MAX + 1, 64):
        idle = nt - (nt // ncg) * ncg
        if idle * threads <= best_idle * nt:
            threads, best_idle = nt, idle
    if copy_photo:
        threads = BLOCK_MAX
    return threads, threads // ncg


def simd_boundary(W):
    """plan_record.hpp: first element of a W-element row on OpenCV's scalar tail (VResizeLinearVec_32s8u)."""
    x = (W // 16) * 16 if W >= 16 else 0
    while x < W - 4:
        x += 4
    return x


def simd_end(ksize, W):
    """resize_kernels.hip: first element of a W-element row on the scalar tail of the generic vertical pass."""
    x = 0
    if ksize == 2:
        x = simd_boundary(W)
    elif ksize == 4:
        x = (W // 8) * 8 if W >= 8 else 0
    return x


def scale_of(out, crop):
    return 1. / (out / crop)  # as plan_direct: 1. / ((double)out / crop)


def resize_mode(crop_w, crop_h, out_w, out_h, cn=3, nearest=False):
    """choose_mode (plan_record.hpp)."""
    if nearest:
        return NEAREST
    if (crop_w, crop_h) == (out_w, out_h):
        return LINEAR
    sx, sy = scale_of(out_w, crop_w), scale_of(out_h, crop_h)
    ix, iy = round(sx), round(sy)  # round half to even, as cvRound
    eps = np.finfo(np.float64).eps
    if abs(sx - ix) < eps and abs(sy - iy) < eps and ix == 2 and iy == 2 and cn in (1, 3):
        return AREA2X
    return LINEAR


def stage_cols(mode, crop_w, win_w, sx):
    if mode == LINEAR:
        return min(crop_w + 1, math.ceil((win_w - 1) * sx) + 4)
    if mode == NEAREST:
        return min(crop_w, math.ceil((win_w - 1) * sx) + 3)
    return 2 * win_w if mode == AREA2X else win_w


def stage_rows(mode, crop_h, win_h, sy, tr):
    rows = min(tr, win_h)
    if mode == LINEAR:
        return min(crop_h, math.ceil((rows - 1) * sy) + 3)
    if mode == NEAREST:
        return min(crop_h, math.ceil((rows - 1) * sy) + 2)
    return 2 * rows if mode == AREA2X else rows


def stage_bytes(cn, rows, cols):
    groups = rows * ((cols + 3) // 4)
    return (groups + 63) // 64 * 1024 if cn == 3 else (groups * 4 + 63) // 64 * 256


def tile_rows(recs, nearest=False):
    """LaunchPlan::shape for one launch group of records: (rows per tile, their cap 4 x phases <= 64, staged
    bytes).  rows < cap when the staged rows of some record passed the budget."""
    _, nph = lanes_and_phases(max(r.out_w for r in recs))
    cap = min(64, max(1, 4 * nph))
    for last, budget in ((False, STAGE_BUDGET), (True, STAGE_BUDGET_HI)):
        for t in range(cap, 0, -1):
            by = 0
            for r in recs:
                m = resize_mode(r.crop_w, r.crop_h, r.out_w, r.out_h, r.cn, nearest)
                by = max(by, stage_bytes(r.cn, stage_rows(m, r.crop_h, r.out_h, scale_of(r.out_h, r.crop_h), t),
                                         stage_cols(m, r.crop_w, r.out_w, scale_of(r.out_w, r.crop_w))))
            by = (by + 1023) // 1024 * 1024
            if by <= budget or (t == 1 and last):
                return t, cap, by
    raise AssertionError("unreachable")


def has_scalar_tail(out_w, cn=3):
    return simd_boundary(out_w * cn) < out_w * cn


def sep_band_columns(cn):
    """GrPlan::shape's CW for a window at least that wide: 4 * (256 / cn) lanes' pixels, at most 1024 / cn."""
    return min(1024 // cn, 4 * (256 // cn))


def column_bands(win_w, cn):
    cw = min(win_w, sep_band_columns(cn))
    return (win_w + cw - 1) // cw


IDENTITY, LINEAR_AREA, AREA_FAST, AREA_2X, AREA_K4, AREA_K8, AREA_GENERIC = (
    "identity", "linear_area", "fast", "area2x", "k4", "k8", "generic")
AREA_CLASSES = (LINEAR_AREA, AREA_FAST, AREA_K4, AREA_K8, AREA_GENERIC)


def area_class(crop_w, crop_h, out_w, out_h):
    """generic_method + GrPlan::shape (plan.cpp) for one INTER_AREA record: the bilinear emulation (an
    upscaled axis), the integer-box fast path (2x2: the tile kernel's RESIZE_AREA2X), or resizeArea_ with
    floor(max scale) + 2 taps: resize_sep's K = 4 form up to 4 taps, K = 8 up to 8, resize_generic above.  A
    launch takes the class of its most taps, so the sweep sends each class as a call of its own."""
    if (crop_w, crop_h) == (out_w, out_h):
        return IDENTITY
    sx, sy = scale_of(out_w, crop_w), scale_of(out_h, crop_h)
    if sx < 1 or sy < 1:
        return LINEAR_AREA
    ix, iy = round(sx), round(sy)
    eps = np.finfo(np.float64).eps
    if abs(sx - ix) < eps and abs(sy - iy) < eps:
        return AREA_2X if ix == 2 and iy == 2 else AREA_FAST
    taps = math.floor(max(1.0, sx, sy)) + 2
    return AREA_K4 if taps <= 4 else AREA_K8 if taps <= 8 else AREA_GENERIC


# the records kernel (image_path.cpp run_records, aug_job.hpp rec_phases / rec_lds_layout)
MAX_LDS = 160 * 1024


def rec_phases(win_w, win_h):
    gpr = win_w // 4
    if gpr <= 0:
        return 0
    most = min(1024 // gpr, 32)
    nph = 16 if most >= 16 and (win_h + 15) // 16 <= 14 else most
    return nph if nph > 0 and (win_h + nph - 1) // nph <= 14 else 0


def records_kernel_takes(recs):
    """run_records for a call of contrast records with float32 CHW output on 16-aligned items: every record
    of one output size, width a multiple of 4 and at most 1024, no scalar row tail (so 3 * out_w % 16 == 0:
    out_w a multiple of 16), every record RESIZE_LINEAR, the two staging buffers within the LDS."""
    W, H = recs[0].out_w, recs[0].out_h
    nph = rec_phases(W, H)
    if W % 4 or W > 1024 or nph <= 0 or has_scalar_tail(W):
        return False
    stage = 0
    for r in recs:
        if (r.out_w, r.out_h) != (W, H) or r.cn != 3 or resize_mode(r.crop_w, r.crop_h, W, H) != LINEAR:
            return False
        stage = max(stage, stage_bytes(3, stage_rows(LINEAR, r.crop_h, H, scale_of(H, r.crop_h), nph * 2),
                                       stage_cols(LINEAR, r.crop_w, W, scale_of(W, r.crop_w))))
    stage = (stage + 1023) // 1024 * 1024
    fixed = 3072 + 3072 + 4096 + 3072 + 184 * 16 + 2 * 64 * 16 + 3 * JOB_BYTES + 256 + 16
    return fixed + 2 * ((W * 8 + 15) // 16 * 16) + 2 * stage <= MAX_LDS


# ---- the records ------------------------------------------------------------------------------------------------
# image: A.synthetic_image's index; the source is src_w x src_h x cn (sources shared by several records have one
# image index and one size)
Rec = namedtuple("Rec", "out_w out_h crop_x crop_y crop_w crop_h src_w src_h flip image cn")

SOURCE_CAP = 64 * 1024     # bytes of a record's own source, where the geometry allows
CALL_SOURCE_CAP = 4 << 20  # ... and of all the sources of one width


def source(rec):
    """The record's source image (tests share them through their own caches)."""
    import aeon_amd as A
    return A.synthetic_image(rec.image, rec.src_w, rec.src_h, rec.cn)


def source_bytes(recs):
    return sum(w * h * cn for w, h, cn in {(r.image, r.src_w, r.src_h, r.cn): (r.src_w, r.src_h, r.cn)
                                           for r in recs}.values())


# -- widths
WIDTH_CENTRES = (597, 641, 681, 769, 897, 1025, 1281, 1537, 1793, 2049)
WIDTHS = list(range(1, 529)) + [w + d for w in WIDTH_CENTRES for d in range(-3, 5)]
CONTIGUOUS_MAX = 528
# (crop_h, out_h) by record index; widths above 528 keep out_h <= 3 (the same ratios: identity, 2x, a
# fractional downscale, an upscale, a single source row, a steep downscale)
ROW_CYCLE = ((5, 5), (10, 5), (7, 5), (3, 9), (1, 4), (23, 3))
ROW_CYCLE_WIDE = ((3, 3), (6, 3), (4, 3), (2, 3), (1, 2), (23, 3))


def crop_widths(w):
    """The crop widths of output width w, in the issue's order (so the widest crop, ceil(7.3 w), meets the
    one-row entry of the row cycle), deduplicated, at least 1."""
    vals = [1, 2, 3, w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1, 3 * w, math.ceil(7.3 * w), math.ceil(w / 3),
            math.ceil(w / 7.3)]
    seen, res = set(), []
    for v in vals:
        if v >= 1 and v not in seen:
            seen.add(v)
            res.append(v)
    return res


def width_records(w, cn=3):
    """The records of output width w: one per crop width, then the exact identity and the exact 2x record.
    crop_x = index mod 16 (every byte alignment of the first staged group, 3 being coprime to 16); the crop
    touches the source's last column on even records and its last row on all but every fourth."""
    cycle = ROW_CYCLE if w <= CONTIGUOUS_MAX else ROW_CYCLE_WIDE
    ident_h, twice_h = (5, 5) if w <= CONTIGUOUS_MAX else (3, 2)
    geo = [(cw,) + cycle[i % len(cycle)] for i, cw in enumerate(crop_widths(w))]
    geo += [(w, ident_h, ident_h), (2 * w, 2 * twice_h, twice_h)]
    recs = []
    for i, (cw, ch, oh) in enumerate(geo):
        exact = i >= len(geo) - 2
        cx, cy = i % 16, i % 3
        sw = cx + cw + (i & 1)
        below = 1 if i % 4 == 1 else 0
        if sw * cn * (cy + ch + below) > SOURCE_CAP:  # a wide crop: fewer source rows (the exact ones keep theirs)
            cy = 0
            if not exact:
                ch = max(1, min(ch, SOURCE_CAP // (sw * cn) - below))
        recs.append(Rec(w, oh, cx, cy, cw, ch, sw, cy + ch + below, i & 1, w * 32 + i, cn))
    return recs


def at_end(r):
    """The crop's last row is the source's last row: its 12-byte loads may cross the end of the buffer."""
    return r.crop_y + r.crop_h == r.src_h


def alignment(r):
    """Byte offset mod 16 of the crop's first staged byte in a 16-aligned, densely packed source."""
    return ((r.crop_y * r.src_w + r.crop_x) * r.cn) % 16


def kind(r):
    if (r.crop_w, r.crop_h) == (r.out_w, r.out_h):
        return IDENTITY
    return resize_mode(r.crop_w, r.crop_h, r.out_w, r.out_h, r.cn)


# -- heights
HEIGHT_WIDTHS = (4, 60, 224, 340)
HEIGHTS = list(range(1, 137))
HEIGHT_MAX = HEIGHTS[-1]
# (vertical crop / output, horizontal crop width of output width w): a vertical identity one column wider than
# the output, the exact 2x record, an upscale, and the steep vertical downscale on a 3x horizontal one (at 340
# columns its staged rows pass the 48 KiB budget at every band height above 2 rows)
HEIGHT_FORMS = ((1.0, lambda w: w + 1), (2.0, lambda w: 2 * w), (0.37, lambda w: math.ceil(0.37 * w)),
                (7.3, lambda w: 3 * w))


def height_records(w, oh, cn=3):
    """The four records of output size w x oh.  The records of one (w, form) over all heights crop one shared
    source, sized for the tallest (the sources of the four 7.3x forms alone are 6 MB)."""
    recs = []
    for k, (fy, fw) in enumerate(HEIGHT_FORMS):
        cw = fw(w)
        ch = oh if k == 0 else 2 * oh if k == 1 else math.ceil(fy * oh)
        ch_max = HEIGHT_MAX if k == 0 else 2 * HEIGHT_MAX if k == 1 else math.ceil(fy * HEIGHT_MAX)
        cx, cy = oh % 5, 3 if k & 1 else 0
        recs.append(Rec(w, oh, cx, cy, cw, ch, cw + 5, ch_max + 3, (oh + k) & 1, 100000 + w * 8 + k, cn))
    return recs


# -- the resize methods
METHOD_WIDTHS = list(range(1, 361)) + list(range(677, 685))
METHOD_WIDTHS_GRAY = list(range(1021, 1029))
METHOD_SCALES = (1 / 3, 1 / 1.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.01, 6.9, 7.1)  # crop / output, crops rounded up
METHOD_HEIGHTS = (1, 5, 17, 33)
# the vertical scale of record k is METHOD_SCALES[k + 3]: that never pairs two integer scales, so two records
# with integer scales on both axes (INTER_AREA's integer-box path, other than the tile kernel's 2x2) follow
METHOD_INTEGER_PAIRS = ((2.0, 3.0), (3.0, 3.0))


def method_records(w, cn=3):
    pairs = [(sx, METHOD_SCALES[(k + 3) % len(METHOD_SCALES)]) for k, sx in enumerate(METHOD_SCALES)]
    pairs += list(METHOD_INTEGER_PAIRS)
    recs = []
    for k, (sx, sy) in enumerate(pairs):
        cw = max(1, math.ceil(w * sx - 1e-9))
        hs = [h for h in METHOD_HEIGHTS[:(k + w) % 4 + 1][::-1]]  # the chosen height first, then shorter ones
        cx, cy = (k + w) % 16, k % 3
        sw = cx + cw + (k & 1)
        for oh in hs:
            ch = max(1, math.ceil(oh * sy - 1e-9))
            sh = cy + ch + (1 if k % 4 == 1 else 0)
            if sw * sh * cn <= SOURCE_CAP or oh == hs[-1]:
                break
        recs.append(Rec(w, oh, cx, cy, cw, ch, sw, sh, k & 1, 200000 + w * 16 + k, cn))
    return recs
