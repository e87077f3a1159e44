"""GPU: the JPEG sampling layouts, tables and stream structures of tests/golden/jpeg_layout_fixtures.npz
through aeon_hip_decode_jpeg_batch and a decode window.

Every file (written by tests/jpeg_writer.py, see make_jpeg_layout_fixtures.py for what each one
exercises) decodes to Pillow's record of it, bit for bit, at both channel counts: 4:4:0 (h1v2 fancy
upsampling, down to one sample a row), box replication by 3 and 4, a subsampled luma plane, chroma
planes of different shapes, a 2x2 grayscale header, 16-bit quantisation tables, Huffman tables past
Annex K and past table ids 0 and 1, zigzag 63 without EOB, more restart segments than jpeg_huff has
lanes, stuffed and fill bytes -- alone, with short colour bands, at each Huffman workgroup size,
through the host entropy decoder, mixed with the fixtures of jpeg_fixtures.npz (which keep their
golden digests), and inside a Decoder window.
"""
import os

import numpy as np
import pytest

import aeon_amd as A
from aeon_amd import configs as C
from tests.jpeg_size_cases import decode_guarded
from tests.test_jpeg_layouts import FX, NAMES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OLD = np.load(os.path.join(HERE, "golden", "jpeg_fixtures.npz"))
OLD_NAMES = sorted({k.rsplit(".", 1)[0] for k in OLD.files})
FILES = [FX[n + ".jpg"].tobytes() for n in NAMES]


def _sha(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def _decode(ctx, files, channels):
    """Padded rows, guarded gaps (tests/jpeg_size_cases.py decode_guarded): a store outside a record fails here."""
    return decode_guarded(ctx, files, channels)


def _context(**env):
    """A context created with `env` set (the JPEG stage's flags are read when the context is created, not at its
    first decode call: Context.jpeg_huff_lanes() tells the workgroup size in effect)."""
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


def _want(name, channels):
    return FX[name + (".bgr" if channels == 3 else ".gray")]


def _check(res, channels, what=""):
    """Every record against the committed one: the fixture, the mismatch count and the first three
    coordinates with both values."""
    assert len(res) == len(NAMES)
    for n, r in zip(NAMES, res):
        want = _want(n, channels)
        assert r.shape == want.shape, (what, n)
        bad = np.argwhere(r != want)
        assert len(bad) == 0, (what, n, channels, len(bad),
                               [(c, int(r[tuple(c)]), int(want[tuple(c)])) for c in bad[:3].tolist()])


@pytest.fixture(scope="module")
def default_records(ctx):
    """The default context's records of every fixture, decoded once."""
    return {cn: _decode(ctx, FILES, cn) for cn in (3, 1)}


@pytest.mark.parametrize("channels", [3, 1])
def test_fixtures_match_reference(default_records, channels):
    _check(default_records[channels], channels)


@pytest.mark.parametrize("band", [1, 2, 3])
def test_short_colour_bands(ctx, band, monkeypatch):
    """AEON_HIP_JPEG_BAND rows per colour workgroup: odd band starts fall inside h1v2 row pairs and
    inside the 4-row groups of box replication."""
    monkeypatch.setenv("AEON_HIP_JPEG_BAND", str(band))
    for cn in (3, 1):
        _check(_decode(ctx, FILES, cn), cn, f"band {band}")


@pytest.mark.parametrize("lanes", [256, 1024])
def test_other_huffman_workgroup_sizes(lanes):
    """jpeg_huff at 256 and 1,024 lanes (512 is the default): rst1_gray_529 has more subsequences than
    512 lanes, rst1_444_289 more than 256 -- one tiny restart segment per subsequence.  Then the encoder-made
    fixtures of jpeg_fixtures.npz against their committed digests: flowers.jpg has more than 256 subsequences
    (the strided phases with Jacobi rounds) and more data than 512 or 1,024 lanes stage."""
    c = _context(AEON_HIP_JPEG_HUFF_LANES=str(lanes))
    try:
        assert c.jpeg_huff_lanes() == lanes
        for cn in (3, 1):
            _check(_decode(c, FILES, cn), cn, f"lanes {lanes}")
        flowers = A.jpeg_huff_layout(OLD["flowers.jpg"].tobytes(), lanes)
        assert flowers["gpu_entropy"] and (flowers["nsub"] > lanes) == (lanes == 256), flowers
        old = [OLD[n + ".jpg"].tobytes() for n in OLD_NAMES]
        for cn, key in ((3, ".bgr"), (1, ".gray")):
            for n, r in zip(OLD_NAMES, _decode(c, old, cn)):
                assert np.array_equal(_sha(r), OLD[n + key]), (f"lanes {lanes}", n, cn)
    finally:
        c.close()


def test_host_entropy_decoder_gives_the_same_records(default_records):
    """AEON_HIP_JPEG_HUFF=host: every file through the host entropy decoder's sparse stream."""
    c = _context(AEON_HIP_JPEG_HUFF="host")
    try:
        for cn in (3, 1):
            for n, a, b in zip(NAMES, default_records[cn], _decode(c, FILES, cn)):
                assert np.array_equal(a, b), (n, cn)
    finally:
        c.close()


# the mixed call: every new fixture with the YCbCr / gray fixtures of jpeg_fixtures.npz in between
MIXED = [(FX, n) for n in NAMES]
for _i, _n in enumerate(OLD_NAMES):
    MIXED.insert(min(2 * _i + 1, len(MIXED)), (OLD, _n))
MIXED_FILES = [fx[n + ".jpg"].tobytes() for fx, n in MIXED]


def test_mixed_call_with_the_encoder_made_fixtures(ctx):
    first = {cn: _decode(ctx, MIXED_FILES, cn) for cn in (3, 1)}
    for cn in (3, 1):
        for (fx, n), r in zip(MIXED, first[cn]):
            if fx is FX:
                want = _want(n, cn)
                bad = np.argwhere(r != want)
                assert len(bad) == 0, (n, cn, len(bad), [(c, int(r[tuple(c)]), int(want[tuple(c)])) for c in bad[:3].tolist()])
            else:
                assert np.array_equal(_sha(r), OLD[n + (".bgr" if cn == 3 else ".gray")]), (n, cn)
    for (fx, n), a, b in zip(MIXED, first[3], _decode(ctx, MIXED_FILES, 3)):
        assert np.array_equal(a, b), ("rerun", n)


def test_decoder_window_with_layout_records():
    """A C1 window of 8 records, two of them the 4:4:0 file and the file with a subsampled luma plane:
    the same outputs as the window with those two records supplied decoded (their committed BGR)."""
    cfg = dict(batch_size=8, random_seed=7, etl=[C.IMAGE_224], augmentation=[C.C1_AUG])
    recs = [(A.synthetic_image(300 + i, 200 + 17 * i, 260 - 11 * i, 3),) for i in range(8)]
    enc, dec = list(recs), list(recs)
    for slot, name in ((2, "y1x2_37x29"), (5, "luma_sub")):
        enc[slot] = (FX[name + ".jpg"].tobytes(),)
        dec[slot] = (np.ascontiguousarray(FX[name + ".bgr"]),)
    (got,) = A.Decoder(cfg).decode(enc)
    (want,) = A.Decoder(cfg).decode(dec)
    assert got.shape == want.shape and got.shape[0] == 8
    assert np.array_equal(got, want)
    assert not np.array_equal(got[2], got[5])
