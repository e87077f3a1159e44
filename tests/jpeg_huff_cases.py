"""Files that put jpeg_huff (aeon_amd/csrc/jpeg_huff.hip) on each of its three paths -- staged lanes, unstaged
lanes, strided -- with Jacobi rounds in the tens to a thousand, written with tests/jpeg_writer.py and shared by
tests/test_jpeg_huff_cases.py (CPU: the host emulation, and the conditions that keep the files what they are meant
to be) and tests/test_hip_jpeg_huff_paths.py (GPU).  Helper, no test of its own.

Sizes come from the decoder's limits (aeon_jpeg_huff_layout reports them): a file is strided at L lanes when its
scan data is more than L subsequences of sub_max bits, i.e. more than L * sub_max / 8 bytes; below that it runs on
the lanes path, staged in LDS when the data fits the stage cap (a device query, at most stage_max).

The families:
  never_sync  gray; the DC table is {0} and the AC table {0x08}, each one 1-bit code, and every AC is -255: the scan
              is all zero bits, 568 per block from any phase, so no guessed start ever re-synchronises and a start is
              exact only once its predecessor's is -- one subsequence settles per round.
  dense       every coefficient uniform in +-1000 with the Annex K tables: no EOB, blocks of ~1,400 bits, so the
              block phase of a guessed start is lost for many subsequences (what a quality-100 photo looks like).
  four        dense CMYK and YCCK files, strided at 256 lanes and one at 512: the only carriers of a fourth
              component's DC sums across scan chunks.
  sparse      dense in the upper half, DC + EOB blocks in the lower: blocks per subsequence 1 .. ~100.
  long        category-10 coefficients at the least subsequence length: a block spans six subsequences and more,
              and most subsequences start no block.
Each case names the path it is meant to take per lane count (`meant`); a lane count it does not name is still run.
"""
import functools
import math

import numpy as np

import aeon_amd as A
from tests import jpeg_writer as JW

LANES = (256, 512, 1024)
STAGED, UNSTAGED, STRIDED = "staged", "unstaged", "strided"
NS_BLOCK_BITS = 1 + 63 * 9  # a never_sync block: the DC code, then 63 times the AC code and eight value bits


class Case:
    def __init__(self, name, family, data, meant, blocks):
        self.name, self.family, self.data, self.meant, self.blocks = name, family, data, meant, blocks

    def __repr__(self):
        return f"Case({self.name}, {len(self.data)} bytes)"


def _gray():
    return [JW.Component(1)]


def _c444():
    return [JW.Component(1, 1, 1, 0, 0, 0), JW.Component(2, 1, 1, 0, 1, 1), JW.Component(3, 1, 1, 0, 1, 1)]


def _c420():
    return [JW.Component(1, 2, 2, 0, 0, 0), JW.Component(2, 1, 1, 0, 1, 1), JW.Component(3, 1, 1, 0, 1, 1)]


def _c4():
    return [JW.Component(1, 1, 1, 0, 0, 0), JW.Component(2, 1, 1, 0, 1, 1), JW.Component(3, 1, 1, 0, 1, 1),
            JW.Component(4, 1, 1, 0, 0, 0)]


ONES = np.ones(64, np.int64)


@functools.lru_cache(None)
def limits():
    """The decoder's limits: sub_min, sub_max (bits per subsequence), default_lanes, stage_max (bytes)."""
    tiny = JW.write_jpeg(8, 8, _gray(), [np.zeros((1, 1, 64), np.int16)], {0: ONES}, {0: JW.K3_DC_LUMA}, {0: JW.K3_AC_LUMA})
    lay = A.jpeg_huff_layout(tiny, LANES[0])
    return {k: lay[k] for k in ("sub_min", "sub_max", "default_lanes", "stage_max")}


def strided_above(lanes):
    """Scan data of more than this many bytes has more than `lanes` subsequences."""
    return lanes * limits()["sub_max"] // 8


def path_of(data, lanes, stage_cap):
    """The path jpeg_huff<lanes> takes for a file, as the kernel decides it, given the queried stage cap."""
    lay = A.jpeg_huff_layout(data, lanes)
    assert lay["gpu_entropy"], "the file goes to the host entropy decoder"
    if lay["nsub"] > lanes:
        return STRIDED
    return STAGED if lay["data_bytes"] <= stage_cap else UNSTAGED


def _never_sync(side, restart=0):
    """side x side blocks, gray."""
    cf = np.full((side, side, 64), -255, np.int16)
    cf[:, :, 0] = 0
    one = [1] + [0] * 15
    return JW.write_jpeg(8 * side, 8 * side, _gray(), [cf], {0: ONES}, {0: (one, [0])}, {0: (one, [0x08])}, restart=restart)


def _side(blocks):
    return math.isqrt(blocks - 1) + 1  # the least square of at least `blocks`


def _dense_coefs(rng, comps, w, h, lo=0, amp=1000, sparse_from=None):
    _, _, blocks = JW.grid(w, h, comps)
    out = []
    for bx, by in blocks:
        cf = rng.integers(-amp, amp + 1, (by, bx, 64))
        if lo:  # magnitudes in [lo, amp] only
            cf = rng.integers(lo, amp + 1, (by, bx, 64)) * rng.choice((-1, 1), (by, bx, 64))
        cf = cf.astype(np.int16)
        cf[:, :, 0] = rng.integers(-1000, 1001, (by, bx))
        if sparse_from is not None:
            cf[int(by * sparse_from):, :, 1:] = 0
        out.append(cf)
    return out


def _dense(seed, comps, w, h, restart=0, adobe=None, **kw):
    rng = np.random.default_rng(seed)
    return JW.write_jpeg(w, h, comps, _dense_coefs(rng, comps, w, h, **kw), {0: ONES},
                         {0: JW.K3_DC_LUMA, 1: JW.K3_DC_CHROMA}, {0: JW.K3_AC_LUMA, 1: JW.K3_AC_CHROMA},
                         restart=restart, adobe=adobe, jfif=adobe is None)


# bytes of a dense block under the Annex K tables (63 coefficients, half of them category 10: 16 + 10 bits in the
# luminance table, 11 + 10 in the chrominance one), rounded down so that a size meant to exceed a bound does
LUMA_BLOCK, CHROMA_BLOCK = 175, 148


def _mcus(target_bytes, mcu_bytes):
    """(mcus_x, mcus_y), near square, of at least target_bytes."""
    n = -(-int(target_bytes) // mcu_bytes)
    mx = _side(n)
    return mx, -(-n // mx)


@functools.lru_cache(None)
def sparse_parts():
    """The sparse-among-dense file (4:4:4; the upper half alone is past the strided bound at 512 lanes) and what
    it was written from: (bytes, components, coefficients, first sparse block row)."""
    mx, my = _mcus(2 * 1.06 * strided_above(512), LUMA_BLOCK + 2 * CHROMA_BLOCK)
    comps, w, h = _c444(), 8 * mx - 1, 8 * my - 5
    coefs = _dense_coefs(np.random.default_rng(20), comps, w, h, sparse_from=0.5)
    data = JW.write_jpeg(w, h, comps, coefs, {0: ONES}, {0: JW.K3_DC_LUMA, 1: JW.K3_DC_CHROMA},
                         {0: JW.K3_AC_LUMA, 1: JW.K3_AC_CHROMA})
    return data, comps, coefs, int(my * 0.5)


def _blocks(data):
    return A.jpeg_entropy_decode(data)[3]


@functools.lru_cache(None)
def cases():
    """Every case, in an order that is not by size."""
    lim = limits()
    s256, s512, s1024 = (strided_above(n) for n in LANES)
    out = []

    def add(name, family, data, meant):
        out.append(Case(name, family, data, meant, _blocks(data)))

    # never_sync.  (a) staged with nsub close to the lanes: nearly two least-length subsequences per lane at 256
    # and at 512 lanes (at sub_min itself the guessed walk's lead-in covers two subsequences, and the first three
    # starts are exact before any round); (b) 3 % past the strided bound at 256 and at 512 lanes; (c) segments of
    # 0.54 x 512 subsequences, two of them and a short one: the first runs past subsequence 256, the second past 512
    ns = lambda frac, lanes: int(frac * lanes * lim["sub_max"] / NS_BLOCK_BITS)
    for n in LANES[:2]:
        add(f"ns_staged{n}", "never_sync", _never_sync(math.isqrt(n * (2 * lim["sub_min"] - 32) // NS_BLOCK_BITS)), {n: STAGED})
    add("ns_strided256", "never_sync", _never_sync(_side(ns(1.03, 256))), {256: STRIDED, 512: UNSTAGED, 1024: STAGED})
    add("ns_strided512", "never_sync", _never_sync(_side(ns(1.03, 512))), {256: STRIDED, 512: STRIDED, 1024: UNSTAGED})
    seg = ns(0.54, 512)
    add("ns_restart", "never_sync", _never_sync(_side(int(2.2 * seg)), restart=seg),
        {256: STRIDED, 512: STRIDED, 1024: UNSTAGED})

    # dense: 6 % past a strided bound, or at 85 % of it for the unstaged lanes path; odd frame sizes.  The rounds
    # of a dense file grow with its subsequences (about an eighth of them with one block per MCU, more with six),
    # so the 4:4:4 and gray files for 256 lanes are 1.8 times the bound: 50 rounds and more, and still on the lanes
    # path at 512
    m444, m420, m4 = LUMA_BLOCK + 2 * CHROMA_BLOCK, 4 * LUMA_BLOCK + 2 * CHROMA_BLOCK, 2 * LUMA_BLOCK + 2 * CHROMA_BLOCK
    mx, my = _mcus(1.8 * s256, m444)
    add("dense_444_s256", "dense", _dense(11, _c444(), 8 * mx - 3, 8 * my - 1), {256: STRIDED, 512: UNSTAGED})
    mx, my = _mcus(1.8 * s256, LUMA_BLOCK)
    add("dense_gray_s256", "dense", _dense(12, _gray(), 8 * mx - 5, 8 * my), {256: STRIDED, 512: UNSTAGED})
    mx, my = _mcus(1.06 * s512, m420)
    add("dense_420_s512", "dense", _dense(13, _c420(), 16 * mx - 6, 16 * my - 2), {256: STRIDED, 512: STRIDED, 1024: UNSTAGED})
    # restart intervals that do not divide the MCU row: one with segments of more than 256 subsequences, one
    # with segments between 128 and 256
    r512 = -(-int(1.04 * s512 / 2) // m420) | 1
    assert r512 % mx, "the restart interval divides the MCU row"
    add("dense_420_rst_long", "dense", _dense(14, _c420(), 16 * mx - 6, 16 * my - 2, restart=r512), {256: STRIDED, 512: STRIDED})
    r256 = -(-int(1.1 * s256 / 2) // m420) | 1
    assert r256 % mx and r256 < r512
    add("dense_420_rst_short", "dense", _dense(15, _c420(), 16 * mx - 6, 16 * my - 2, restart=r256), {256: STRIDED, 1024: UNSTAGED})
    mx, my = _mcus(1.06 * s1024, m444)
    add("dense_444_s1024", "dense", _dense(16, _c444(), 8 * mx - 3, 8 * my - 1), {256: STRIDED, 512: STRIDED, 1024: STRIDED})
    mx, my = _mcus(0.85 * s256, m420)
    add("dense_420_u256", "dense", _dense(17, _c420(), 16 * mx - 9, 16 * my - 1), {256: UNSTAGED, 512: UNSTAGED, 1024: STAGED})

    # four components, strided at 256 lanes with a third of the subsequences in the second chunk of the prefix
    # scan: CMYK (Adobe transform 0) and YCCK (transform 2)
    mx, my = _mcus(1.5 * s256, m4)
    add("dense_cmyk_s256", "four", _dense(18, _c4(), 8 * mx - 3, 8 * my - 3, adobe=0), {256: STRIDED})
    add("dense_ycck_s256", "four", _dense(19, _c4(), 8 * mx - 3, 8 * my - 3, adobe=2), {256: STRIDED})
    # and one past the bound of the default workgroup, where no other file carries a fourth sum across chunks
    mx, my = _mcus(1.06 * s512, m4)
    add("dense_cmyk_s512", "four", _dense(22, _c4(), 8 * mx - 5, 8 * my - 1, adobe=0), {256: STRIDED, 512: STRIDED, 1024: UNSTAGED})

    add("sparse_444", "sparse", sparse_parts()[0], {256: STRIDED, 512: STRIDED})

    # long blocks at the least subsequence length: little enough data for sub_min at every lane count
    nblk = LANES[0] * lim["sub_min"] // 8 // 2 // LUMA_BLOCK
    side = math.isqrt(nblk)
    add("long_blocks", "long", _dense(21, _gray(), 8 * side + 3, 8 * side - 2, lo=512), {256: STAGED, 512: STAGED, 1024: STAGED})
    return out


def by_name():
    return {c.name: c for c in cases()}


@functools.lru_cache(None)
def reference(name, channels):
    """oracle.jpeg_decode of a case, computed once and read-only."""
    import oracle
    a = oracle.jpeg_decode(by_name()[name].data, channels)
    a.setflags(write=False)
    return a
