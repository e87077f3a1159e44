"""CPU: the JPEG size sweep's lists (tests/jpeg_size_cases.py) are what they claim -- every branch of the JPEG
stage they are chosen against is reached, on the rules restated there -- the oracle's decode of every file is
Pillow's (committed digests, recomputed where Pillow is installed), and the two float-reciprocal divisions of
jpeg_kernels.hip are exact over their whole domains."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import aeon_amd as A
import oracle
from tests import jpeg_size_cases as J

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = np.load(os.path.join(HERE, "golden", "jpeg_size_digests.npz"))
CASES = J.all_cases()
COMPS = {c: J.components(c.w, c.h, c.samp) for c in CASES}


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def test_lists_are_the_sweep():
    assert len({c.name for c in CASES}) == len(CASES) == 8 * (72 + 70) + 5 * (40 + 70) + len(J.structural_cases())
    assert DIGESTS["names"].tolist() == [c.name for c in CASES]
    for layout in J.LAYOUTS:
        cs = J.sweep_cases(layout)
        widths = [c for c in cs if c.sweep == "w"]
        assert [c.w for c in widths] == list(range(1, 41 if layout in J.FOUR else 73))
        assert {c.h for c in widths} == set(J.HEIGHT_CYCLE)
        heights = [c for c in cs if c.sweep == "h"]
        assert [c.h for c in heights] == list(range(1, 71)) and {c.w for c in heights} == set(J.WIDTH_CYCLE)
    assert all(33 <= h <= 35 for _, _, h in J.HALVING)
    assert max(c.w * c.h * 3 for c in CASES) < 600 * 1024  # small records only (the widest: 5105 x 33)


@pytest.mark.parametrize("layout", J.LAYOUTS + ["structural"])
def test_generator_and_oracle_match_the_committed_digests(layout):
    """The generator still writes the committed bytes, the product's parser reads each file's size and sends it to
    the GPU entropy decoder, and the oracle decodes it to Pillow's record at both channel counts."""
    for i, c in enumerate(CASES):
        if (c.layout if c.sweep != "s" else "structural") != layout:
            continue
        b = J.jpg(c)
        assert np.array_equal(_sha(np.frombuffer(b, np.uint8))[:8], DIGESTS["jpg"][i]), c.name
        assert A.jpeg_info(b) == (c.w, c.h, len(c.samp)), c.name
        assert A.jpeg_host_stage(b)[0], (c.name, "routed to the host entropy decoder")
        bgr, gray = oracle.jpeg_decode(b, 3), oracle.jpeg_decode(b, 1)
        assert bgr.shape == (c.h, c.w, 3) and gray.shape == (c.h, c.w), c.name
        assert np.array_equal(_sha(bgr), DIGESTS["bgr"][i]), c.name
        assert np.array_equal(_sha(gray), DIGESTS["gray"][i]), c.name


def test_pillow_gives_the_committed_digests():
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("make_jpeg_size_digests",
                                                  os.path.join(HERE, "golden", "make_jpeg_size_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = mod.digests()
    for k in ("names", "jpg", "bgr", "gray"):
        bad = np.flatnonzero((fresh[k] != DIGESTS[k]).reshape(len(CASES), -1).any(axis=1))
        assert len(bad) == 0, (k, [CASES[i].name for i in bad[:5]])


def test_samples_clamp_at_both_ends():
    """The drawer asserts every sample inside [-256, 511] (nothing is skipped: a block outside is drawn again);
    samples below 0 and above 255 occur, so the IDCT's clamp is exercised."""
    for c in CASES:
        J.jpg(c)
    lo, hi = zip(*(J.JB.RANGE[c.name] for c in CASES))
    assert J.JB.LO <= min(lo) < -1 and 256 < max(hi) <= J.JB.HI
    assert sum(a < 0 and b > 255 for a, b in zip(lo, hi)) > len(CASES) // 2


# ---- coverage, on the restated rules ---------------------------------------------------------------------------

def test_restated_rules_at_hand_computed_points():
    assert [J.upsample_mode(*a) for a in ((1, 1, 1), (2, 1, 3), (2, 1, 2), (1, 2, 1), (2, 2, 3), (2, 2, 2), (4, 1, 9),
                                          (1, 4, 9))] == [J.UP_FULL, J.UP_H2V1, J.UP_BOX, J.UP_H1V2, J.UP_H2V2, J.UP_BOX,
                                                          J.UP_BOX, J.UP_BOX]
    assert J.stage_rows(J.UP_FULL, 1, 32) == 32 and J.stage_rows(J.UP_H2V2, 2, 32) == 19 and J.stage_rows(J.UP_BOX, 4, 32) == 10
    c = J.components(37, 29, J.YCC["s420"])
    assert [(k.bw, k.bh, k.dw, k.dh) for k in c] == [(6, 4, 37, 29), (3, 2, 19, 15), (3, 2, 19, 15)]
    assert J.band_rows(c, 3) == (32, 32 * (48 + 16) + 2 * 19 * (24 + 16)) and J.band_rows(c, 1) == (32, 32 * 64)
    assert J.chunks(J.components(1015, 6, J.GRAY["gray"]), 3) == [(0, 0, 127)]
    assert J.chunks(c, 1) == [(0, 0, 24)] and J.chunks(c, 3) == [(0, 0, 24), (1, 0, 6), (2, 0, 6)]
    assert J.store_bgr8(16, 8) == "3 x 8 bytes" and J.store_bgr8(20, 8) == "6 dwords" and J.store_bgr8(18, 8) == "bytes"
    assert J.store_bgr8(16, 7) == "bytes" and J.store_bgr4(8, 4, 8) == "3 dwords" and J.store_bgr4(8, 4, 7) == "bytes"
    assert J.store_gray4(6, 0, 8) == "bytes" and J.store_gray4(4, 0, 4) == "dword"
    assert J.record_layout([(3, 2), (5, 1), (1, 1)], 3) == ([(16, 9), (64, 16), (112, 5)], 144)


def test_every_upsampler_occurs():
    seen = {}
    for c in CASES:
        for k in COMPS[c]:
            seen.setdefault(k.up, set()).add((k.hf, k.vf, k.dw <= 2))
    assert set(seen) == {J.UP_FULL, J.UP_H2V1, J.UP_H1V2, J.UP_H2V2, J.UP_BOX}
    # box replication: by 4, and the h2v1 and h2v2 components of one and two samples a row
    assert {(4, 1, False), (4, 1, True), (2, 1, True), (2, 2, True)} <= seen[J.UP_BOX]
    for hf, vf in ((2, 1), (2, 2)):
        assert {k.dw for c in CASES for k in COMPS[c] if (k.hf, k.vf) == (hf, vf)} >= {1, 2, 3, 4}
    # h1v2 stays fancy at one sample a row and at one row
    h1v2 = {(k.dw, k.dh) for c in CASES for k in COMPS[c] if k.up == J.UP_H1V2}
    assert {dw for dw, _ in h1v2} >= {1, 2, 3} and {dh for _, dh in h1v2} >= {1, 2, 3} and (1, 1) in h1v2
    # the fast path's width threshold: 4:2:0 BGR files on both sides of it
    s420 = [c for c in CASES if c.layout == "s420"]
    assert {J.takes_h2v2(COMPS[c], 3, 0) for c in s420 if c.w <= 4} == {False}
    assert {J.takes_h2v2(COMPS[c], 3, 0) for c in s420 if c.w >= 5} == {True}
    assert not any(J.takes_h2v2(COMPS[c], 1, 0) for c in s420)
    assert not any(J.takes_h2v2(COMPS[c], 3, 0) for c in CASES if c.layout not in ("s420",))
    # MCU widths 8, 16 and 32
    assert {8 * max(s[0] for s in c.samp) for c in CASES} == {8, 16, 32}


def test_band_counts_and_halved_bands():
    classes = {"s444": 1689, "s420": 3185, "gray": 5105, "cmyk_11": 1265}  # the first halved width of each class
    for layout, first in classes.items():
        for w in (first - 1, first):
            (c,) = [c for c in CASES if c.sweep == "s" and c.layout == layout and c.w == w]
            band, lds = J.band_rows(COMPS[c], 3)
            assert (band, lds > J.RAISE_LDS_ABOVE) == (32 if w < first else 16, True), c.name
            assert len(J.bands(c.h, band)) == (2 if w < first else 3)
            assert J.bands(c.h, band)[-1][1] in (1, 2, 3)  # a short tail
        # ... and it is the first: one MCU narrower fits
        hmax = 8 * max(s[0] for s in J.SAMP[layout])
        assert (first - 1) % hmax == 0
        assert J.band_rows(J.components(first - 1, 34, J.SAMP[layout]), 3)[0] == 32
    assert {len(J.bands(c.h, J.band_rows(COMPS[c], 3)[0])) for c in CASES if c.sweep == "h"} == {1, 2, 3}
    # LDS on both sides of the kernel's 64 KiB default
    assert any(J.band_rows(COMPS[c], cn)[1] <= J.RAISE_LDS_ABOVE for c in CASES for cn in (3, 1))
    # band edges (rows 32 and 64) at every height, against every vertical upsampler
    for layout in J.LAYOUTS:
        hs = {c.h for c in CASES if c.layout == layout and c.sweep == "h"}
        assert hs == set(range(1, 71)), layout


def test_both_idct_divisions_and_every_chunk_tail():
    by_form = {}
    for c in CASES:
        for k in COMPS[c]:
            by_form.setdefault(J.idct_division(k.bw), set()).add((k.bw, k.bh))
    assert {(511, 2), (1, 1)} <= by_form["reciprocal"] and {(512, 2), (639, 5)} <= by_form["integer"]
    blocks = {k.bw * k.bh for c in CASES if c.sweep == "s" for k in COMPS[c]}
    assert set(J.BLOCK_COUNTS) <= blocks
    tails, counts = set(), set()
    for c in CASES:
        ch = J.chunks(COMPS[c], 3)
        counts |= {n for _, _, n in ch}
        last = {}
        for k, first, n in ch:
            last[k] = (first, n)
        tails |= {n for first, n in last.values() if first > 0}  # the short last chunk of a component of several
    assert set(J.CHUNK_TAILS) <= tails
    assert set(J.SHORT_CHUNKS) | {127, 128} <= counts  # chunks of 1..33 blocks, and the whole one
    # block rows of several chunks, and chunks that span block rows
    assert any(k.bw > 128 and k.bh > 1 for c in CASES for k in COMPS[c])
    assert any(k.bw < 128 and k.bw * k.bh > 128 for c in CASES for k in COMPS[c])


def _stores(layout_cases, cn, band_max=J.ROWS_PER_WG):
    lay, _ = J.record_layout([(c.w, c.h) for c in layout_cases], cn)
    out = set()
    for c, (off, stride) in zip(layout_cases, lay):
        assert off % 16 == 0 and stride == c.w * cn + lay.index((off, stride)) % 8
        out |= J.stores(c, cn, stride, band_max)
    return out


def test_every_store_form_at_every_alignment():
    """With the strides of the decode helper (record_layout), per call of the GPU test (one layout's sweep)."""
    for layout in J.LAYOUTS:
        cs = J.sweep_cases(layout)
        for cn in (3, 1):
            got = _stores(cs, cn)
            path = ("color4" if layout in J.FOUR else "rows") + (" bgr" if cn == 3 else " gray")
            word = "3 dwords" if cn == 3 else "dword"
            want = {(path, word, "0 mod 4", "whole", 4), (path, "bytes", "other", "whole", 4)}
            want |= {(path, "bytes", cls, "tail", n) for cls in ("0 mod 4", "other") for n in (1, 2, 3)}
            assert want <= got, (layout, cn, sorted(want - got))
            if layout == "s420" and cn == 3:
                want = {("h2v2", "3 x 8 bytes", "0 mod 8", "whole", 8), ("h2v2", "6 dwords", "4 mod 8", "whole", 8),
                        ("h2v2", "bytes", "other", "whole", 8)}
                want |= {("h2v2", "bytes", cls, "tail", n) for cls in ("0 mod 8", "4 mod 8", "other") for n in range(1, 8)}
                assert want <= got, sorted(want - got)
                # a band of 3 rows: odd band starts take color_rows inside files of the fast path
                assert {p for p, *_ in _stores(cs, 3, 3)} == {"h2v2", "rows bgr"}
            else:
                assert not any(p == "h2v2" for p, *_ in got)
    # no form is ever chosen for a cut group or a misaligned one
    for p, form, cls, part, n in _stores(list(CASES), 3) | _stores(list(CASES), 1):
        assert (form != "bytes") == (part == "whole" and cls in ("0 mod 4", "0 mod 8", "4 mod 8")), (p, form, cls, part, n)


def test_guard_check_sees_one_byte_anywhere_outside_the_pixels():
    """guarded_records on a buffer filled from the oracle: the records come back; one changed byte in a row's
    padding, in a gap, before the first record or at the buffer's end fails and names the record."""
    cases = J.sweep_cases("s420")[:12]
    sizes = [(c.w, c.h) for c in cases]
    for cn in (3, 1):
        lay, total = J.record_layout(sizes, cn)
        host = np.full(total, J.GUARD, np.uint8)
        want = [oracle.jpeg_decode(J.jpg(c), cn).reshape(c.h, c.w * cn) for c in cases]
        for (off, stride), (w, h), a in zip(lay, sizes, want):
            host[off:off + h * stride].reshape(h, stride)[:, :w * cn] = a
        got = J.guarded_records(host, sizes, cn)
        assert all(np.array_equal(g.reshape(a.shape), a) for g, a in zip(got, want))
        (off5, stride5), (w5, h5) = lay[5], sizes[5]
        spots = {"pad": (off5 + w5 * cn, "('row', 0, 'byte', %d)" % (w5 * cn)),       # first byte past row 0
                 "last pad": (off5 + h5 * stride5 - 1, "'row', %d" % (h5 - 1)),        # the last row's padding
                 "gap": (lay[6][0] - 1, "past the record's end"), "front": (15, "before the first record"),
                 "end": (total - 1, "past the record's end")}
        for what, (p, text) in spots.items():
            dirty = host.copy()
            dirty[p] ^= 0xFF
            with pytest.raises(AssertionError, match="1 guard bytes written") as e:
                J.guarded_records(dirty, sizes, cn, [c.name for c in cases])
            assert text in str(e.value) and (cases[5].name in str(e.value)) == (what in ("pad", "last pad", "gap")), (what, str(e.value))


# ---- the reciprocal divisions -----------------------------------------------------------------------------------

def _idct_rows(bw, rows):
    """jpeg_idct's (int)(((float)b + 0.5f) * (1.0f / (float)bw)) at the first and last block of each block row."""
    by = np.arange(rows, dtype=np.int64)
    b = np.stack([by * bw, by * bw + bw - 1], axis=1)
    rbw = np.float32(1.0) / np.float32(bw)
    got = ((b.astype(np.float32) + np.float32(0.5)) * rbw).astype(np.int32)
    return got, b // bw


def test_idct_reciprocal_division_is_exact_below_512():
    """Every block-row boundary of every component width the reciprocal form serves (a 65,535-row file has 8,192
    block rows), and the first width at which the unguarded form would fail lies at or above the guard."""
    for bw in range(1, 512):
        got, want = _idct_rows(bw, 8193)
        assert np.array_equal(got, want), bw
    first = next(bw for bw in range(1, 8192) if not np.array_equal(*_idct_rows(bw, 8193)))
    assert first >= 512
    for bw in (1000, 2047, 4096, 8191):  # the guard matters
        assert not np.array_equal(*_idct_rows(bw, 8193)), bw


def test_h2v2_reciprocal_division_is_exact():
    """color_h2v2's pr = (int)(((float)it + 0.5f) * (1.0f / (float)groups)) for item it = pr * groups + q: groups
    1..8192 (a 65,535-column file), row pairs 0..31 (a band of at most 64 rows), at both ends of every pair."""
    groups = np.arange(1, 8193, dtype=np.int64)[:, None, None]
    pr = np.arange(32, dtype=np.int64)[None, :, None]
    it = pr * groups + np.stack([np.zeros_like(groups), groups - 1], axis=2).reshape(-1, 1, 2)
    rcp = np.float32(1.0) / groups.astype(np.float32)
    got = ((it.astype(np.float32) + np.float32(0.5)) * rcp).astype(np.int32)
    assert np.array_equal(got, np.broadcast_to(pr, got.shape))
