"""GPU: every image size through the JPEG stage's IDCT and colour kernels (jpeg_idct, jpeg_color with its 4:2:0
fast path color_h2v2, jpeg_color4).

The files of tests/jpeg_size_cases.py -- per sampling layout every width 1..72 (1..40 for four components) and
every height 1..70, and the structural files: the widths on each side of the first colour band halving, a
component of 511 and of 512 blocks a row, components of 127..257 blocks and every listed chunk tail -- decode to
the oracle's record of each, bit for bit, at both channel counts (tests/test_jpeg_size_cases.py pins the oracle's
decode to Pillow's, and that the lists reach the branches they are chosen against).

Every call goes through jpeg_size_cases.decode_guarded: rows padded by 0..7 bytes (the BGR row starts reach
every residue mod 8, so every store form meets every alignment on whole and on cut pixel groups), records 16 or
32 bytes apart in a buffer filled with 0x5A, and no byte outside a record's pixels may change.  Through the
default context, with colour bands of 1, 2 and 3 rows (band 3 puts odd band starts into 4:2:0 files: color_rows
inside files of the fast path), through the host entropy decoder's sparse stream, and -- the structural files --
at the other two Huffman workgroup sizes and mixed with sweep files in one call.
"""
import functools
import os

import numpy as np
import pytest

import aeon_amd as A
import oracle
from tests import jpeg_size_cases as J

pytestmark = pytest.mark.gpu

GROUPS = {layout: J.sweep_cases(layout) for layout in J.LAYOUTS}
GROUPS["structural"] = J.structural_cases()


@functools.lru_cache(maxsize=None)
def _want(case, channels):
    """The oracle's record, computed once and shared (never written to)."""
    a = oracle.jpeg_decode(J.jpg(case), channels)
    a.setflags(write=False)
    return a


def _context(**env):
    """A context created with `env` set (the JPEG stage's flags are read when the context is created)."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    os.environ.update(env)
    try:
        return A.Context(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_ctx():
    c = _context(AEON_HIP_JPEG_HUFF="host")
    yield c
    c.close()


def _check(ctx, cases, channels, what=""):
    """One guarded decode call of `cases`; every record against the oracle's: the file, the mismatch count and the
    first three coordinates with both values."""
    res = J.decode_guarded(ctx, [J.jpg(c) for c in cases], channels, [c.name for c in cases])
    assert len(res) == len(cases)
    for c, r in zip(cases, res):
        want = _want(c, channels)
        assert r.shape == want.shape, (what, c.name, r.shape, want.shape)
        bad = np.argwhere(r != want)
        assert len(bad) == 0, (what, c.name, channels, len(bad),
                               [(xy, int(r[tuple(xy)]), int(want[tuple(xy)])) for xy in bad[:3].tolist()])
    return res


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("layout", J.LAYOUTS)
def test_sweep_matches_oracle(ctx, layout, channels):
    _check(ctx, GROUPS[layout], channels)


@pytest.mark.parametrize("band", [1, 2, 3])
@pytest.mark.parametrize("group", list(GROUPS))
def test_short_colour_bands(ctx, group, band, monkeypatch):
    """AEON_HIP_JPEG_BAND rows per colour workgroup: band starts on every row, on every even row, and on odd rows
    inside the row pairs of the vertical upsamplers."""
    monkeypatch.setenv("AEON_HIP_JPEG_BAND", str(band))
    for cn in (3, 1):
        _check(ctx, GROUPS[group], cn, f"band {band}")


@pytest.mark.parametrize("group", list(GROUPS))
def test_host_entropy_decoder(host_ctx, group):
    """AEON_HIP_JPEG_HUFF=host: jpeg_idct gathers its columns from the sparse stream."""
    for cn in (3, 1):
        _check(host_ctx, GROUPS[group], cn, "host entropy decoder")


def test_structural_files(ctx):
    """The band-halving widths (launches of more than 64 KiB of LDS), both forms of jpeg_idct's block-row division
    and the chunk edges, on the GPU entropy decoder -- a file the host stage routes to the host decoder fails here
    -- then once more in a call mixed with sweep files, with the same records."""
    cases = GROUPS["structural"]
    for c in cases:
        assert A.jpeg_host_stage(J.jpg(c))[0], (c.name, "routed to the host entropy decoder")
    first = {cn: _check(ctx, cases, cn) for cn in (3, 1)}
    mixed = []
    for i, c in enumerate(cases):
        mixed += [c, GROUPS[J.LAYOUTS[i % len(J.LAYOUTS)]][5 * i % 110]]
    for cn in (3, 1):
        for c, a, b in zip(cases, first[cn], _check(ctx, mixed, cn, "mixed")[::2]):
            assert np.array_equal(a, b), (c.name, cn)


@pytest.mark.parametrize("lanes", [256, 1024])
def test_structural_files_at_other_huffman_workgroup_sizes(lanes):
    c = _context(AEON_HIP_JPEG_HUFF_LANES=str(lanes))
    try:
        assert c.jpeg_huff_lanes() == lanes
        for cn in (3, 1):
            _check(c, GROUPS["structural"], cn, f"lanes {lanes}")
    finally:
        c.close()
