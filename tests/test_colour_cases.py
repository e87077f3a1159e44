"""tests/colour_cases.py pinned on the CPU: the records of every shape tests/test_hip_colour_cube.py cuts the
colour cube into hold each of the 2^24 BGR triples, in cube order, with the documented padding; the lattice
holds what it says; and the geometry those tests use hands the photometric stages exactly these pixels (the
oracle's identity resize, and its 2x INTER_AREA of a pixel-doubled record, return the record)."""
import numpy as np
import pytest

import aeon_amd as A
from tests import colour_cases as K
from tests import helpers as H

SHAPES = [(1024, 1024), (256, 224)]  # (w, h): the tile kernel's slabs, the records kernel's records


@pytest.mark.parametrize("w,h", SHAPES)
def test_cube_records_hold_every_triple(w, h):
    n = K.cube_record_count(w, h)
    assert n == {(1024, 1024): 16, (256, 224): 293}[(w, h)]
    recs = K.cube_records(w, h)
    assert len(recs) == n and all(r.shape == (h, w, 3) and r.dtype == np.uint8 for r in recs)
    idx = np.concatenate([K.triple_index(r).reshape(-1) for r in recs])
    assert idx.size == n * w * h
    assert np.array_equal(idx[:K.CUBE], np.arange(K.CUBE, dtype=np.uint32))  # each triple, in cube order
    pad = idx.size - K.CUBE
    assert 0 <= pad < w * h
    assert np.array_equal(idx[K.CUBE:], np.arange(pad, dtype=np.uint32))  # the padding repeats the cube's start
    seen = np.zeros(K.CUBE, bool)
    seen[idx] = True
    assert seen.all()


def test_cube_record_slices():
    a = K.cube_records(256, 224, first=290)
    assert len(a) == 3 and np.array_equal(a[0], K.cube_record(290, 256, 224))
    assert len(K.cube_records(1024, 1024, first=4, count=2)) == 2
    assert tuple(K.cube_record(5, 1024, 1024)[3, 7]) == (5 * 16, 12, 7)  # pixel 5 * 2^20 + 3 * 1024 + 7
    with pytest.raises(IndexError):
        K.cube_record(16, 1024, 1024)


def test_lattice():
    lv = K.LATTICE_LEVELS
    assert len(lv) >= 32 and len(set(lv)) == len(lv) and {0, 1, 127, 128, 254, 255} <= set(lv)
    rec = K.lattice_record()
    assert rec.shape == (K.LATTICE_H, K.LATTICE_W, 3) and rec.dtype == np.uint8
    idx = K.triple_index(rec).reshape(-1)
    assert idx.size == len(lv) ** 3 == np.unique(idx).size
    assert set(np.unique(rec)) == set(lv)
    assert np.all(np.diff(idx.astype(np.int64)) > 0)  # cube order


def test_identity_geometry_hands_the_cube_to_the_photometric_stages(oracle):
    """An identity record (crop = record = output, no flip) leaves the oracle's resize as a copy, and so does a
    2x INTER_AREA (cv::resize's dispatch of a 2x INTER_LINEAR) of the record with every pixel doubled both ways:
    (4 v + 2) >> 2 = v.  One slab from the saturated end of the cube, and the lattice."""
    out = A.out_desc(channels=3, channel_major=False, dtype="uint8", item_stride=1024 * 1024 * 3)
    for rec in (K.cube_record(15, 1024, 1024), K.lattice_record()):
        h, w = rec.shape[:2]
        p = A.aug_params(crop_x=0, crop_y=0, crop_w=w, crop_h=h, out_w=w, out_h=h)
        (same,) = H.oracle_records([rec], [p], out)
        assert np.array_equal(same, rec)
        twice = np.repeat(np.repeat(rec, 2, axis=0), 2, axis=1)
        p2 = A.aug_params(crop_x=0, crop_y=0, crop_w=2 * w, crop_h=2 * h, out_w=w, out_h=h)
        (half,) = H.oracle_records([twice], [p2], out)
        assert np.array_equal(half, rec)
