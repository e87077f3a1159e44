"""The size sweep's lists (tests/size_cases.py) are what they claim -- every planner threshold they are chosen
against is reached -- and four oracle invariants of the width records that do not depend on the restated
planner rules being right (crop offsets never leak, flips mirror, identity records copy, 2x records average
2x2 blocks)."""
import numpy as np

import oracle as O
from tests import size_cases as S

WIDTH_RECS = {w: S.width_records(w) for w in S.WIDTHS}


def test_restated_boundaries():
    """simd_boundary / simd_end at hand-computed points (VResizeLinearVec_32s8u: 16 elements while
    x <= W - 16, then 4 while x < W - 4; VResizeCubicVec_32s8u: 8 while x <= W - 8; no SIMD for LANCZOS4)."""
    assert [S.simd_boundary(W) for W in (1, 4, 5, 8, 9, 12, 16, 20, 21, 36, 672)] == [0, 0, 4, 4, 8, 8, 16, 16, 20, 32, 672]
    assert [S.simd_end(4, W) for W in (7, 8, 15, 16, 23)] == [0, 8, 8, 16, 16]
    assert S.simd_end(8, 100) == 0 and S.simd_end(2, 21) == 20
    assert S.lanes_and_phases(224) == (448, 8) and S.lanes_and_phases(2500) == (512, 1)
    assert S.sep_band_columns(3) == 340 and S.sep_band_columns(1) == 1024


def test_widths_reach_every_workgroup_shape():
    want = {S.lanes_and_phases(w) for w in range(1, 2101)}
    assert len(want) == 70 and {lanes for lanes, _ in want} == {320, 384, 448, 512}
    assert {S.lanes_and_phases(w) for w in S.WIDTHS} == want
    assert max((w + 3) // 4 for w in S.WIDTHS) > 512  # past 512 column groups
    assert S.WIDTHS[:528] == list(range(1, 529)) and len(S.WIDTHS) == 528 + 80 == len(set(S.WIDTHS))
    for w in S.WIDTHS:
        if w > S.CONTIGUOUS_MAX:
            assert all(r.out_h <= 3 for r in WIDTH_RECS[w]), w


def test_widths_reach_every_store_form_and_row_tail():
    tails = {((3 * w) % 16, S.has_scalar_tail(w)) for w in S.WIDTHS}
    assert {t[0] for t in tails} == set(range(16))
    # the 4-wide loop stops at x < W - 4, so a row is free of the scalar tail only where its elements are a
    # multiple of 16: out_w % 16 == 0 for one and for three channels.  out_w % 4 == 0 therefore occurs with and
    # without a tail (the vector store forms on both vertical formulas), the other three residues only with one
    for cn in (1, 3):
        for w in S.WIDTHS:
            assert S.has_scalar_tail(w, cn) == (w % 16 != 0), (w, cn)
    for q in range(4):
        assert {S.has_scalar_tail(w) for w in S.WIDTHS if w % 4 == q} == ({False, True} if q == 0 else {True}), q
    # ... and a tail is one to four elements long
    assert {3 * w - S.simd_boundary(3 * w) for w in S.WIDTHS if w > 5} == {0, 1, 2, 3, 4}


def test_every_width_has_the_three_resize_modes_and_the_crop_list():
    for w, recs in WIDTH_RECS.items():
        kinds = {S.kind(r) for r in recs}
        assert kinds == {S.IDENTITY, S.AREA2X, S.LINEAR}, w
        ident, twice = recs[-2], recs[-1]
        assert (ident.crop_w, ident.crop_h) == (w, ident.out_h) and (twice.crop_w, twice.crop_h) == (2 * w, 2 * twice.out_h)
        assert [r.crop_w for r in recs[:-2]] == S.crop_widths(w)
        assert {r.flip for r in recs} == {0, 1}
        for i, r in enumerate(recs):
            assert r.crop_x == i % 16 and r.out_w == w and r.crop_w >= 1 and r.crop_h >= 1
            assert r.src_w == r.crop_x + r.crop_w + (i & 1) and r.crop_y + r.crop_h <= r.src_h
    assert S.crop_widths(100) == [1, 2, 3, 99, 100, 101, 199, 200, 201, 300, 730, 34, 14]


def test_width_records_reach_every_alignment_and_the_end_of_the_buffer():
    """crop_x = index mod 16 gives as many byte offsets of the crop in its row as a width has records (3 is
    coprime to 16) -- 15 at most, the list holding 13 crop widths and the two exact records, so offset 13
    (index 15) is reached only through crop_y: the first staged byte lies (crop_y * src_w + crop_x) * 3 bytes
    into a 16-aligned image (S.alignment), and over the rows every alignment occurs hundreds of times."""
    seen = {}
    for w, recs in WIDTH_RECS.items():
        in_row = {(r.crop_x * 3) % 16 for r in recs}
        assert len(in_row) == min(16, len(recs)), w
        if len(recs) >= 16:
            assert in_row == set(range(16)), w
        align = {S.alignment(r) for r in recs}
        assert len(recs) < 15 or len(align) >= 6, w
        for a in align:
            seen[a] = seen.get(a, 0) + 1
        ends = [S.at_end(r) for r in recs]
        assert all(a or b for a, b in zip(ends, ends[1:])), w  # the last row: at least every other record
        assert any(S.at_end(r) and r.src_w == r.crop_x + r.crop_w for r in recs), w  # ... and the last column with it
        assert any(not S.at_end(r) for r in recs) or len(recs) < 2, w
    assert set(seen) == set(range(16)) and min(seen.values()) >= 100
    assert sum(len(recs) == 15 for recs in WIDTH_RECS.values()) > 500  # 13 crop widths + the two exact records


def test_source_sizes():
    over = 0
    for w, recs in WIDTH_RECS.items():
        assert S.source_bytes(recs) < S.CALL_SOURCE_CAP, w
        over += sum(r.src_w * r.src_h * r.cn > S.SOURCE_CAP for r in recs)
    assert over == 0
    for w in S.HEIGHT_WIDTHS:
        for oh in S.HEIGHTS:
            assert S.source_bytes(S.height_records(w, oh)) < S.CALL_SOURCE_CAP, (w, oh)
    for cn, widths in ((3, S.METHOD_WIDTHS), (1, S.METHOD_WIDTHS_GRAY)):
        for w in widths:
            recs = S.method_records(w, cn)
            assert S.source_bytes(recs) < S.CALL_SOURCE_CAP, w
            # over 64 KiB only where a single output row already needs that much
            assert all(r.src_w * r.src_h * cn <= S.SOURCE_CAP or r.out_h == 1 for r in recs), w


def test_heights_cross_the_band_cap_and_cut_the_band():
    assert S.HEIGHTS == list(range(1, 137)) and S.HEIGHT_WIDTHS == (4, 60, 224, 340)
    caps, cut = set(), {}
    for w in S.HEIGHT_WIDTHS:
        for oh in S.HEIGHTS:
            recs = S.height_records(w, oh)
            assert [r.crop_h for r in recs] == [oh, 2 * oh, int(np.ceil(0.37 * oh)), int(np.ceil(7.3 * oh))]
            assert [S.kind(r) for r in recs] == [S.LINEAR, S.AREA2X, S.LINEAR, S.LINEAR]
            assert [r.crop_y for r in recs] == [0, 3, 0, 3] and all(r.crop_y + r.crop_h <= r.src_h for r in recs)
            assert all(r.crop_x + r.crop_w <= r.src_w for r in recs)
            tr, cap, _ = S.tile_rows([r for r in recs if S.kind(r) == S.LINEAR])
            caps.add(cap)
            if tr < min(cap, oh):
                cut.setdefault(w, []).append(oh)
    assert 64 in caps and min(caps) < 32  # the 64-row cap (4 columns: 512 phases) and bands well below it
    # 340 columns, 7.3x down on a 3x horizontal downscale: 256 column groups a row, 12 rows within 48 KiB
    assert cut[340] == list(range(3, 137))
    tr, cap, by = S.tile_rows([S.height_records(340, 136)[3]])
    assert (tr, cap) == (2, 24) and by <= S.STAGE_BUDGET
    assert 4 not in cut  # (1 column group: every band fits)


def test_method_lists():
    assert S.METHOD_WIDTHS == list(range(1, 361)) + list(range(677, 685)) and S.METHOD_WIDTHS_GRAY == list(range(1021, 1029))
    assert {S.column_bands(w, 3) for w in S.METHOD_WIDTHS} == {1, 2, 3}
    assert {S.column_bands(w, 1) for w in S.METHOD_WIDTHS_GRAY} == {1, 2}
    assert S.column_bands(340, 3) == 1 and S.column_bands(341, 3) == 2 and S.column_bands(681, 3) == 3
    for ksize, period in ((2, 16), (4, 8)):
        for cn, widths in ((3, S.METHOD_WIDTHS), (1, S.METHOD_WIDTHS_GRAY)):
            res = {(w * cn) % period for w in widths}
            # (one channel: the eight widths around 1024 are eight residues, 13 .. 4 mod 16)
            assert res == (set(range(period)) if cn == 3 or period == 8 else {13, 14, 15, 0, 1, 2, 3, 4}), (ksize, cn)
            tails = {w * cn - S.simd_end(ksize, w * cn) for w in widths if w * cn >= period}
            assert tails == (set(range(5)) if ksize == 2 else set(range(8))), (ksize, cn)
    classes = {}
    for w in S.METHOD_WIDTHS:
        recs = S.method_records(w)
        assert len(recs) == len(S.METHOD_SCALES) + len(S.METHOD_INTEGER_PAIRS)
        assert all(r.out_h in S.METHOD_HEIGHTS and r.out_w == w for r in recs)
        for r in recs:
            classes.setdefault(S.area_class(r.crop_w, r.crop_h, r.out_w, r.out_h), set()).add(w)
    assert set(classes) >= set(S.AREA_CLASSES)
    for c in S.AREA_CLASSES:  # every class on both sides of the band edge
        assert min(classes[c]) <= 8 and any(340 < w <= 360 for w in classes[c]) and max(classes[c]) >= 677, c
    assert {r.out_h for w in S.METHOD_WIDTHS for r in S.method_records(w)} == set(S.METHOD_HEIGHTS)
    # where the scale pairs of a 100-column record land (vertical = the scale three places on; the crops are
    # rounded up, so at a short output 3.01 becomes the integer 4 and 6.9 becomes 7):
    #   1/3 x 1.5, 1/1.5 x 2, 3.01 x 1/3       an upscaled axis: the bilinear emulation
    #   1 x 2.5 (43 / 17)                      floor(2.53) + 2 = 4 taps: K = 4
    #   1.5 x 3 (99 / 33), 6.9 x 1/1.5 -> 1    5 and 8 taps: K = 8
    #   2 x 3.01 -> 4 / 1, 2 x 3, 3 x 3        integer boxes
    #   2.5 x 6.9 -> 35 / 5, 3 x 7.1, 7.1 x 1  9 taps: resize_generic
    r100 = S.method_records(100)
    assert [S.area_class(r.crop_w, r.crop_h, r.out_w, r.out_h) for r in r100] == [
        S.LINEAR_AREA, S.LINEAR_AREA, S.AREA_K4, S.AREA_K8, S.AREA_FAST, S.AREA_GENERIC, S.AREA_GENERIC, S.LINEAR_AREA,
        S.AREA_K8, S.AREA_GENERIC, S.AREA_FAST, S.AREA_FAST], [(r.crop_w, r.crop_h, r.out_h) for r in r100]
    assert S.area_class(299, 298, 100, 100) == S.AREA_K4 and S.area_class(690, 483, 100, 70) == S.AREA_K8
    assert S.area_class(710, 500, 100, 70) == S.AREA_GENERIC and S.area_class(448, 448, 224, 224) == S.AREA_2X


def test_records_kernel_rule():
    """The restated run_records: only widths that are a multiple of 16 (no scalar row tail), one output size,
    no 2x record."""
    for w in (4, 60, 100, 228):
        assert not S.records_kernel_takes([r for r in WIDTH_RECS[w] if S.kind(r) != S.AREA2X and r.out_h == 5])
    for w in (16, 224, 256):
        five = [r for r in WIDTH_RECS[w] if S.kind(r) != S.AREA2X and r.out_h == 5]
        assert len(five) >= 4 and S.records_kernel_takes(five), w
        assert not S.records_kernel_takes([WIDTH_RECS[w][0], WIDTH_RECS[w][3]])  # two output heights
        assert not S.records_kernel_takes([WIDTH_RECS[w][-1]])  # the exact 2x record


# ---- oracle invariants over one width case in eight -------------------------------------------------------------
SAMPLE = [r for w in S.WIDTHS[::8] for r in WIDTH_RECS[w]]


def _params(r, **kw):
    kw = dict(dict(crop_x=r.crop_x, crop_y=r.crop_y, crop_w=r.crop_w, crop_h=r.crop_h, out_w=r.out_w, out_h=r.out_h,
                   flip=r.flip), **kw)
    return O.params(**kw)


def test_oracle_invariants_of_the_width_records():
    assert len(SAMPLE) > 1000
    n_ident = n_twice = 0
    for r in SAMPLE:
        src = S.source(r)
        got = O.transform_image(src, _params(r))
        assert got.shape == (r.out_h, r.out_w, 3)
        crop = np.ascontiguousarray(src[r.crop_y:r.crop_y + r.crop_h, r.crop_x:r.crop_x + r.crop_w])
        # the crop cut out as its own image: the offset and the pixels around the crop never leak
        alone = O.transform_image(crop, _params(r, crop_x=0, crop_y=0))
        assert np.array_equal(got, alone), r
        # the flip mirrors
        other = O.transform_image(src, _params(r, flip=1 - r.flip))
        assert np.array_equal(got, other[:, ::-1]), r
        plain = other if r.flip else got
        if S.kind(r) == S.IDENTITY:
            n_ident += 1
            assert np.array_equal(plain, crop), r
        elif S.kind(r) == S.AREA2X:
            n_twice += 1
            c = crop.astype(np.uint32)
            box = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
            assert np.array_equal(plain, box.astype(np.uint8)), r
    assert n_ident >= len(S.WIDTHS[::8]) and n_twice >= len(S.WIDTHS[::8])
