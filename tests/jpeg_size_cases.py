"""The files of the JPEG size sweep (tests/test_hip_jpeg_sizes.py) and the rules of the JPEG stage they are chosen
against, restated in Python (tests/test_jpeg_size_cases.py pins that the lists reach what they claim and that the
oracle's decode of every file is Pillow's).

What a file's geometry decides on the device (aeon_amd/csrc/jpeg.hpp, jpeg_host.cpp, jpeg_kernels.hip):

  * the upsampler of each component: jpeg_upsample_mode picks full resolution, one of the three fancy triangle
    filters, or box replication -- the latter also for an h2v1 / h2v2 component of fewer than 3 samples a row;
  * the colour bands: jpeg_decode_batch gives a workgroup kJpegRowsPerWg = 32 output rows (AEON_HIP_JPEG_BAND in
    tests), halved while the rows jpeg_stage_rows bounds, at a pitch of bw * 8 + 16 bytes, pass kJpegColorLds =
    160 KiB; past 64 KiB launch_color raises the kernel's dynamic LDS limit first;
  * the colour kernel: four-component files go to jpeg_color4; a three-component file with full-resolution luma
    and h2v2 chroma decoded to BGR takes color_h2v2 in every band that starts on an even row (8 columns of a row
    pair per lane), everything else color_rows (4 pixels per lane);
  * the store form: store_bgr8 writes 8 whole pixels as three 8-byte stores at an address that is 0 mod 8, as six
    dwords at 4 mod 8, else bytes; color_rows and jpeg_color4 write 4 whole pixels as three dwords (BGR) or one
    (gray) at an address that is 0 mod 4, else bytes; a group cut by the row's end goes out as bytes;
  * the IDCT chunks: kJpegIdctBlocks = 128 blocks of one component per workgroup, 32 lane groups x 4 blocks, the
    last chunk of a component short; the block row of block b is b / bw, through a float reciprocal while
    bw < 512.

The restatements follow the C++ line by line; none of them is used to compute an expected pixel.

Every file is written by tests/jpeg_writer.py from the seeded sparse blocks of tests/jpeg_blocks.py (seeded by the
file's name; the drawer keeps every sample inside [-256, 511] and asserts it), when it is first asked for.
"""
import functools
from collections import namedtuple

from tests import jpeg_blocks as JB

# ---- the rules, restated ----------------------------------------------------------------------------------------
UP_FULL, UP_H2V1, UP_H1V2, UP_H2V2, UP_BOX = range(5)  # jpeg.hpp JpegUpsample
ROWS_PER_WG, COLOR_LDS = 32, 160 * 1024  # kJpegRowsPerWg, kJpegColorLds
IDCT_BLOCKS = 128                        # kJpegIdctBlocks
RAISE_LDS_ABOVE = 64 * 1024              # launch_color: hipFuncSetAttribute first


def upsample_mode(hf, vf, dw):
    """jpeg_upsample_mode."""
    fancy = dw > 2
    if hf == 1 and vf == 1:
        return UP_FULL
    if hf == 2 and vf == 1 and fancy:
        return UP_H2V1
    if hf == 1 and vf == 2:
        return UP_H1V2
    if hf == 2 and vf == 2 and fancy:
        return UP_H2V2
    return UP_BOX


def stage_rows(up, vf, rows):
    """jpeg_stage_rows."""
    if up in (UP_H1V2, UP_H2V2):
        return rows // 2 + 3
    if up == UP_BOX:
        return rows // vf + 2
    return rows


Comp = namedtuple("Comp", "bw bh dw dh hf vf up")


def components(w, h, samp):
    """parse_frame's component geometry (blocks with padding, samples, expansion factors) and the upsampler."""
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    mcux, mcuy = (w + 8 * hmax - 1) // (8 * hmax), (h + 8 * vmax - 1) // (8 * vmax)
    out = []
    for ch, cv in samp:
        dw, dh = (w * ch + hmax - 1) // hmax, (h * cv + vmax - 1) // vmax
        hf, vf = hmax // ch, vmax // cv
        out.append(Comp(mcux * ch, mcuy * cv, dw, dh, hf, vf, upsample_mode(hf, vf, dw)))
    return out


def planes_needed(ncomp, cn):
    """jpeg_planes_needed: a gray record of a YCbCr (or gray) file is its first plane alone."""
    return 1 if cn == 1 and ncomp <= 3 else ncomp


def band_rows(comps, cn, band_max=ROWS_PER_WG):
    """The band loop of jpeg_decode_batch: (rows per colour workgroup, the LDS bytes it asks for)."""
    nc, band = planes_needed(len(comps), cn), band_max
    while True:
        lds = 0
        for c in comps[:nc]:
            lds += stage_rows(c.up, c.vf, band) * (c.bw * 8 + 16)
        if lds <= COLOR_LDS or band == 1:
            break
        band //= 2
    assert lds <= COLOR_LDS  # (else the stage refuses the file)
    return band, lds


def bands(h, band):
    return [(y, min(band, h - y)) for y in range(0, h, band)]


def chunks(comps, cn):
    """The chunk split of jpeg_decode_batch: (component, first block, blocks) per jpeg_idct workgroup."""
    out = []
    for k, c in enumerate(comps[:planes_needed(len(comps), cn)]):
        nb = c.bw * c.bh
        for b in range(0, nb, IDCT_BLOCKS):
            out.append((k, b, min(IDCT_BLOCKS, nb - b)))
    return out


def idct_division(bw):
    """jpeg_idct's block-row division of a component bw blocks wide."""
    return "reciprocal" if bw < 512 else "integer"


def takes_h2v2(comps, cn, y0):
    """jpeg_color's dispatch of one band (of a file that is not jpeg_color4's)."""
    return (len(comps) == 3 and cn == 3 and [c.up for c in comps] == [UP_FULL, UP_H2V2, UP_H2V2] and y0 % 2 == 0)


# the three store predicates: the form a group of n pixels leaves in at address a
def store_bgr8(a, n):
    if n == 8 and a % 8 == 0:
        return "3 x 8 bytes"
    if n == 8 and a % 4 == 0:
        return "6 dwords"
    return "bytes"


def store_bgr4(a, x0, w):
    return "3 dwords" if x0 + 3 < w and a % 4 == 0 else "bytes"


def store_gray4(a, x0, w):
    return "dword" if x0 + 3 < w and a % 4 == 0 else "bytes"


# ---- the record layout of a decode call ------------------------------------------------------------------------
GUARD = 0x5A


def record_layout(sizes, cn):
    """[(offset, stride)] of the records of one decode call and the buffer's size: record i has `i % 8` bytes of
    padding after each row (so the starts of BGR rows reach every residue mod 8) and starts on a multiple of 16,
    16 or 32 guard bytes after the end of the record before it (the first after 16 guard bytes)."""
    out, off = [], 16
    for i, (w, h) in enumerate(sizes):
        stride = w * cn + i % 8
        out.append((off, stride))
        off = (off + h * stride + 15) // 16 * 16 + (16 if i % 2 == 0 else 32)
    return out, off


def decode_guarded(ctx, files, channels, names=None):
    """The records of `files` through ctx.decode_jpeg_batch into a buffer laid out by record_layout and filled
    with GUARD: asserts that no byte of the row padding, of the gaps or of the buffer's two ends was written, and
    returns the records (HWC, or HW for one channel)."""
    import torch

    import aeon_amd as A
    sizes = [A.jpeg_info(b)[:2] for b in files]
    lay, total = record_layout(sizes, channels)
    descs = [A.ImgDesc(offset=off, width=w, height=h, stride=stride, channels=channels)
             for (off, stride), (w, h) in zip(lay, sizes)]
    dst = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    ctx.decode_jpeg_batch(files, descs, dst.data_ptr(), stream)
    ctx.synchronize(stream)
    return guarded_records(dst.cpu().numpy(), sizes, channels, names)


def guarded_records(host, sizes, channels, names=None):
    """The records of a buffer laid out by record_layout(sizes, channels) (copies), after asserting that every
    byte outside their pixels still holds GUARD: the failure names the record of the first three such bytes and
    where they lie."""
    import numpy as np
    lay, total = record_layout(sizes, channels)
    assert host.shape == (total,)
    guard, out = np.ones(total, bool), []
    for (off, stride), (w, h) in zip(lay, sizes):
        rows = host[off:off + h * stride].reshape(h, stride)[:, :w * channels]
        guard[off:off + h * stride].reshape(h, stride)[:, :w * channels] = False
        out.append(rows.reshape(h, w, channels).copy() if channels == 3 else rows.copy())
    bad = np.flatnonzero(guard & (host != GUARD))
    if len(bad):
        offs, where = [off for off, _ in lay], []
        for p in bad[:3].tolist():
            i = max(int(np.searchsorted(offs, p, side="right")) - 1, 0)
            (off, stride), (w, h) = lay[i], sizes[i]
            row, col = divmod(p - off, stride)
            where.append((names[i] if names else i, f"{w}x{h}", "stride", stride,
                          "before the first record" if p < off else ("row", row, "byte", col) if row < h else
                          ("bytes past the record's end", p - off - h * stride), "value", int(host[p])))
        raise AssertionError(f"{len(bad)} guard bytes written ({channels} channels): {where}")
    return out


def stores(case, cn, stride, band_max=ROWS_PER_WG):
    """Every (kernel path, store form, alignment class, "whole" / "tail", pixels) that the rows of `case` leave in
    when its record starts on a multiple of 16 with `stride` bytes a row."""
    comps = components(case.w, case.h, case.samp)
    band, _ = band_rows(comps, cn, band_max)
    four, w, out = len(comps) == 4, case.w, set()
    for y0, rows in bands(case.h, band):
        fast = not four and takes_h2v2(comps, cn, y0)
        for y in range(y0, y0 + rows):
            a = y * stride  # every group of a row starts a multiple of 8 (h2v2: 24 q) or of 4 (12 q, 4 q) further
            if fast:
                cls = {0: "0 mod 8", 4: "4 mod 8"}.get(a % 8, "other")
                if w >= 8:
                    out.add(("h2v2", store_bgr8(a, 8), cls, "whole", 8))
                if w % 8:
                    out.add(("h2v2", store_bgr8(a + w // 8 * 24, w % 8), cls, "tail", w % 8))
                continue
            path = ("color4" if four else "rows") + (" bgr" if cn == 3 else " gray")
            form = store_bgr4 if cn == 3 else store_gray4
            cls = "0 mod 4" if a % 4 == 0 else "other"
            if w >= 4:
                out.add((path, form(a, 0, w), cls, "whole", 4))
            if w % 4:
                x0 = w // 4 * 4
                out.add((path, form(a + x0 * cn, x0, w), cls, "tail", w % 4))
    return out


# ---- the files --------------------------------------------------------------------------------------------------
# Y / Cb / Cr as (h, v)
YCC = {
    "s444": ((1, 1), (1, 1), (1, 1)),
    "s420": ((2, 2), (1, 1), (1, 1)),
    "s422": ((2, 1), (1, 1), (1, 1)),
    "s440": ((1, 2), (1, 1), (1, 1)),
    "s411": ((4, 1), (1, 1), (1, 1)),  # box replication by 4
    "mixed_c": ((2, 2), (2, 1), (1, 2)),
    "luma_sub": ((1, 1), (2, 2), (2, 2)),
}
GRAY = {"gray": ((1, 1),)}
# four components through jpeg_color4: (C / M / Y / K as (h, v), the Adobe transform: 0 CMYK, 2 YCCK)
FOUR = {
    "cmyk_11": (((1, 1),) * 4, 0),
    "cmyk_22": (((2, 2), (1, 1), (1, 1), (1, 1)), 0),
    "cmyk_12": (((1, 2), (1, 1), (1, 1), (1, 1)), 0),
    "cmyk_21": (((2, 1), (1, 1), (1, 1), (1, 1)), 0),
    "ycck_420": (((2, 2), (1, 1), (1, 1), (2, 2)), 2),  # 10 blocks per MCU
}
LAYOUTS = list(YCC) + list(GRAY) + list(FOUR)
SAMP = dict(YCC, **GRAY, **{k: v[0] for k, v in FOUR.items()})

SWEEP_WIDTHS, SWEEP_WIDTHS_FOUR, SWEEP_HEIGHTS = range(1, 73), range(1, 41), range(1, 71)
HEIGHT_CYCLE = (1, 2, 3, 5, 8, 9, 15, 16, 17, 31, 33)  # of the width sweep
WIDTH_CYCLE = (1, 2, 3, 7, 8, 9, 16, 17, 24, 25, 33)   # of the height sweep

Case = namedtuple("Case", "name layout sweep w h samp")  # sweep: "w", "h" or "s" (structural)


def sweep_cases(layout):
    """The width sweep, then the height sweep of a layout; the cycles start one entry later per layout."""
    k = LAYOUTS.index(layout)
    widths = SWEEP_WIDTHS_FOUR if layout in FOUR else SWEEP_WIDTHS
    wh = [("w", w, HEIGHT_CYCLE[(w + k) % 11]) for w in widths] + [("h", WIDTH_CYCLE[(h + k) % 11], h) for h in SWEEP_HEIGHTS]
    return [Case(f"{layout}_{s}_{w}x{h}", layout, s, w, h, SAMP[layout]) for s, w, h in wh]


def _block_file(n):
    """A gray file of n blocks: as many block rows (at most 8) as divide n, the last block column and row cut."""
    rows = max(r for r in range(1, 9) if n % r == 0)
    return ("gray", n // rows * 8 - n % 7, rows * 8 - n % 5)


# the widths on each side of the first band halving of a layout class (derived from the band loop: tests pin it),
# heights 33..35 so that a halved band has a short tail
HALVING = (("s444", 1688, 34), ("s444", 1689, 34), ("s420", 3184, 34), ("s420", 3185, 35),
           ("gray", 5104, 34), ("gray", 5105, 33), ("cmyk_11", 1264, 33), ("cmyk_11", 1265, 35))
# a component of 511 and of 512 blocks a row, two block rows each: both forms of jpeg_idct's division
DIVISION = (("gray", 4088, 9), ("gray", 4089, 9))
BLOCK_COUNTS = (127, 128, 129, 255, 256, 257)
CHUNK_TAILS = (1, 31, 32, 33, 64, 65, 96, 97)  # blocks of a component's last chunk
SHORT_CHUNKS = tuple(range(1, 34))             # components of fewer blocks than a chunk: the lane groups' clamps
BLOCK_FILES = tuple(_block_file(n) for n in BLOCK_COUNTS + tuple(IDCT_BLOCKS + t for t in CHUNK_TAILS if t != 1) + SHORT_CHUNKS)
STRUCTURAL_KW = dict(nac=2, amp=60, zmax=10)  # sparser blocks: the wide files stay under 16 KB


def structural_cases():
    return [Case(f"{layout}_s_{w}x{h}", layout, "s", w, h, SAMP[layout]) for layout, w, h in HALVING + DIVISION + BLOCK_FILES]


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(c for layout in LAYOUTS for c in sweep_cases(layout)) + tuple(structural_cases())


@functools.lru_cache(maxsize=None)
def jpg(case):
    """The file's bytes."""
    kw = STRUCTURAL_KW if case.sweep == "s" else None
    if case.layout in YCC:
        return JB.ycc(case.name, case.w, case.h, case.samp, draw_kw=kw)
    if case.layout in GRAY:
        return JB.gray(case.name, case.w, case.h, draw_kw=kw)
    return JB.four(case.name, case.w, case.h, case.samp, FOUR[case.layout][1], draw_kw=kw)
