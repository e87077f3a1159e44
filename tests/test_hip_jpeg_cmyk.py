"""GPU: CMYK, YCCK and Adobe-RGB JPEG files through aeon_hip_decode_jpeg_batch and a decode window.

Every fixture of tests/golden/jpeg_cmyk_fixtures.npz (made by make_jpeg_cmyk_fixtures.py) decodes to
the records tests/jpeg_cmyk_ref.py gives from Pillow's decode, bit for bit: four components through
the GPU Huffman decoder (jpeg_huff) or the host one, the IDCT, each component's upsampler and
jpeg_color4 -- alone, mixed with the YCbCr and gray fixtures of jpeg_fixtures.npz (which keep their
golden digests), with short colour bands, and inside a Decoder window.
"""
import hashlib
import os

import numpy as np
import pytest

import aeon_amd as A
from aeon_amd import configs as C

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, "golden", "jpeg_cmyk_fixtures.npz"))
NAMES = sorted(k[:-4] for k in FX.files if k.endswith(".jpg"))
OLD = np.load(os.path.join(HERE, "golden", "jpeg_fixtures.npz"))
OLD_NAMES = sorted({k.rsplit(".", 1)[0] for k in OLD.files})


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def _decode(ctx, files, channels):
    import torch
    descs, off = [], 0
    for b in files:
        w, h, _ = A.jpeg_info(b)
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=w * channels, channels=channels))
        off += (w * h * channels + 15) // 16 * 16
    dst = torch.full((max(off, 16),), 0x5A, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.decode_jpeg_batch(files, descs, dst.data_ptr(), stream)
    ctx.synchronize(stream)
    host = dst.cpu().numpy()
    out = []
    for d in descs:
        a = host[d.offset:d.offset + d.width * d.height * channels]
        out.append(a.reshape(d.height, d.width, channels) if channels == 3 else a.reshape(d.height, d.width))
    return out


def _context(**env):
    """A context created with `env` set (the JPEG stage reads its flags when the context is created)."""
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


# the mixed window: every new fixture with the YCbCr / gray fixtures in between
MIXED = [(FX, n) for n in NAMES]
for _i, _n in enumerate(OLD_NAMES):
    MIXED.insert(min(2 * _i + 1, len(MIXED)), (OLD, _n))
MIXED_FILES = [fx[n + ".jpg"].tobytes() for fx, n in MIXED]


def _check_mixed(res, channels, what=""):
    for (fx, n), r in zip(MIXED, res):
        if fx is FX:
            bad = np.argwhere(r != _want(n, channels))
            assert len(bad) == 0, (what, n, channels, len(bad), bad[:3].tolist())
        else:
            assert np.array_equal(_sha(r), OLD[n + (".bgr" if channels == 3 else ".gray")]), (what, n, channels)


@pytest.mark.parametrize("channels", [3, 1])
def test_fixtures_match_reference(ctx, channels):
    res = _decode(ctx, [FX[n + ".jpg"].tobytes() for n in NAMES], channels)
    for n, r in zip(NAMES, res):
        want = _want(n, channels)
        assert r.shape == want.shape, n
        bad = np.argwhere(r != want)
        assert len(bad) == 0, (n, len(bad), bad[:3].tolist(), r[tuple(bad[0])], want[tuple(bad[0])])


@pytest.fixture(scope="module")
def mixed(ctx):
    """The mixed call's records at the default band height, decoded once."""
    return {cn: _decode(ctx, MIXED_FILES, cn) for cn in (3, 1)}


@pytest.mark.parametrize("channels", [3, 1])
def test_mixed_call_with_ycbcr_and_gray_files(mixed, channels):
    _check_mixed(mixed[channels], channels)


def test_mixed_call_rerun_identical(ctx, mixed):
    for a, b in zip(mixed[3], _decode(ctx, MIXED_FILES, 3)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("band", [1, 2, 3])
def test_mixed_call_short_colour_bands(ctx, band, monkeypatch):
    """AEON_HIP_JPEG_BAND rows per colour workgroup: odd band starts on four planes, bands that start
    and end inside an h2v2 row pair."""
    monkeypatch.setenv("AEON_HIP_JPEG_BAND", str(band))
    for cn in (3, 1):
        _check_mixed(_decode(ctx, MIXED_FILES, cn), cn, f"band {band}")


def test_mixed_call_host_entropy_decoder(mixed):
    """AEON_HIP_JPEG_HUFF=host: every file through the host entropy decoder's sparse stream, the same
    records."""
    c = _context(AEON_HIP_JPEG_HUFF="host")
    try:
        for cn in (3, 1):
            for (fx, n), a, b in zip(MIXED, mixed[cn], _decode(c, MIXED_FILES, cn)):
                assert np.array_equal(a, b), (n, cn)
    finally:
        c.close()


@pytest.mark.parametrize("lanes", [256, 1024])
def test_other_huffman_workgroup_sizes(lanes):
    """jpeg_huff at 256 and 1,024 lanes (512 is the default): at 256 the cmyk_strided fixture has more
    subsequences than lanes and takes the strided phases."""
    c = _context(AEON_HIP_JPEG_HUFF_LANES=str(lanes))
    try:
        assert c.jpeg_huff_lanes() == lanes
        for n, r in zip(NAMES, _decode(c, [FX[n + ".jpg"].tobytes() for n in NAMES], 3)):
            assert np.array_equal(r, FX[n + ".bgr"]), (n, lanes)
    finally:
        c.close()


def test_decoder_window_with_cmyk_records():
    """A C1 window of 8 records, two of them a CMYK and a YCCK file: the same outputs as the window
    with those two records supplied decoded (the reference BGR)."""
    cfg = dict(batch_size=8, random_seed=7, etl=[C.IMAGE_224], augmentation=[C.C1_AUG])
    recs = [(A.synthetic_image(300 + i, 200 + 17 * i, 260 - 11 * i, 3),) for i in range(8)]
    enc, dec = list(recs), list(recs)
    for slot, name in ((2, "cmyk_strided"), (5, "ycck_37x53")):
        enc[slot] = (FX[name + ".jpg"].tobytes(),)
        dec[slot] = (np.ascontiguousarray(FX[name + ".bgr"]),)
    (got,) = A.Decoder(cfg).decode(enc)
    (want,) = A.Decoder(cfg).decode(dec)
    assert got.shape == want.shape and got.shape[0] == 8
    assert np.array_equal(got, want)
    assert not np.array_equal(got[2], got[5])
