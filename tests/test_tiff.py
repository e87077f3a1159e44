"""The TIFF host decoder (aeon_decode_tiff, tiff_host.cpp) against the numpy restatement of its rules
(tests/tiff_ref.py) and, where a rule is pinned, against Pillow's decode of the same bytes
(tests/golden/tiff_fixtures.npz, written by libtiff through Pillow; the writer's files, which
tests/test_tiff_writer.py holds against Pillow).  Then every refusal with its code and message.
"""
import os
import struct

import numpy as np
import pytest

import aeon_amd as A
from tests import tiff_cases as TC
from tests import tiff_ref as R
from tests import tiff_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, "golden", "tiff_fixtures.npz"))
NAMES = sorted(k[:-5] for k in FX.files if k.endswith(".file"))
MODES = [A.DECODE_BGR8, A.DECODE_GRAY8, A.DECODE_ANYDEPTH]
EINVAL, EUNSUPPORTED = -1, -3


def test_fixtures_decoder_equals_reference_equals_pillow():
    """No fixture left out: the RGBA ones, which Pillow writes with unassociated alpha, are refused as such."""
    assert len(NAMES) == 50
    pinned = 0
    for n in NAMES:
        f, px, mode = FX[n + ".file"].tobytes(), FX[n + ".pil"], str(FX[n + ".mode"])
        if mode == "RGBA":
            with pytest.raises(A.AeonHipError) as e:
                A.decode_tiff(f)
            assert e.value.code == EUNSUPPORTED and "TIFF: unassociated alpha" in str(e.value), n
            continue
        got = [A.decode_tiff(f, m) for m in MODES]
        for m in MODES:
            want = R.decode(f, m)
            assert got[m].dtype == want.dtype and np.array_equal(got[m], want), (n, m)
        w, h, cn, eb = A.tiff_info(f)
        assert (h, w) == px.shape[:2] and cn == (1 if mode in ("L", "I;16") else 3) and eb == (2 if mode == "I;16" else 1), n
        # the pinned rules
        if mode == "L":
            assert np.array_equal(got[1], px) and np.array_equal(got[2], px) and np.array_equal(got[0], np.dstack([px] * 3)), n
        elif mode == "RGB":
            assert np.array_equal(got[0], px[:, :, ::-1]), n
        elif mode == "I;16":
            assert got[2].dtype == np.uint16 and np.array_equal(got[2], px), n
        else:  # P: Pillow's palette is the file's ColorMap >> 8 too (this build; the rule stays "parity unpinned")
            assert mode == "P" and np.array_equal(got[0], px[:, :, ::-1]), n
        pinned += 1
    assert pinned == 40


def test_writer_files_decoder_equals_reference():
    files = TC.device_files() + TC.host_files()
    assert len(files) > 150
    for name, f in files:
        for m in MODES:
            want, got = R.decode(f, m), A.decode_tiff(f, m)
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, m, np.argwhere(got != want)[:3].tolist())


def test_modes_and_strides():
    a = np.arange(5 * 7, dtype=np.uint16).reshape(5, 7) * 900
    f = W.write(a, 1, "lzw", pred=2, big=True)
    assert A.tiff_info(f) == (7, 5, 1, 2)
    assert np.array_equal(A.decode_tiff(f, A.DECODE_ANYDEPTH), a)
    assert np.array_equal(A.decode_tiff(f, A.DECODE_GRAY8), a >> 8)
    buf = np.full((5, 40), 0x5A, np.uint8)
    assert A.lib().aeon_decode_tiff(f, len(f), A.DECODE_BGR8, buf.ctypes.data, 40, None) == 0
    assert np.all(buf[:, 21:] == 0x5A) and np.array_equal(buf[:, :21].reshape(5, 7, 3)[:, :, 1], a >> 8)
    assert A.lib().aeon_decode_tiff(f, len(f), A.DECODE_BGR8, buf.ctypes.data, 20, None) == EINVAL
    assert A.lib().aeon_decode_tiff(f, len(f), 3, buf.ctypes.data, 40, None) == EINVAL


G = np.arange(12, dtype=np.uint8).reshape(3, 4)
RGB = np.arange(36, dtype=np.uint8).reshape(3, 4, 3)


def _retag(f, tag, value):
    """The file with a SHORT / LONG tag's inline value replaced (little-endian writer files)."""
    (ifd,) = struct.unpack_from("<I", f, 4)
    (n,) = struct.unpack_from("<H", f, ifd)
    for k in range(n):
        at = ifd + 2 + 12 * k
        t, ty = struct.unpack_from("<HH", f, at)
        if t == tag:
            return f[:at + 8] + struct.pack("<HH" if ty == 3 else "<I", *((value, 0) if ty == 3 else (value,))) + f[at + 12:]
    raise KeyError(tag)


UNSUPPORTED = {
    "BigTIFF": lambda: W.write(G, 1, version=43),
    "tiled files": lambda: W.write(G, 1, more_tags=[(322, 3, [16])]),
    "planar-separate": lambda: W.write(RGB, 2, planar=2),
    "1-bit samples": lambda: _retag(W.write(G, 1), 258, 1),
    "2-bit samples": lambda: _retag(W.write(G, 1), 258, 2),
    "4-bit samples": lambda: _retag(W.write(G, 1), 258, 4),
    "32-bit samples": lambda: _retag(W.write(G, 1), 258, 32),
    "float samples": lambda: W.write(G.astype(np.uint16), 1, sampleformat=3),
    "Predictor 3": lambda: W.write(G, 1, "lzw", more_tags=[(317, 3, [3])]),
    "CCITT compression": lambda: W.write(G, 1, 3),
    "JPEG compression": lambda: W.write(G, 1, 7),
    "old-style JPEG": lambda: W.write(G, 1, 6),
    "CMYK": lambda: W.write(np.dstack([RGB, G]), 5),
    "YCbCr": lambda: W.write(RGB, 6),
    "CIELab": lambda: W.write(RGB, 8),
    "FillOrder 2": lambda: W.write(G, 1, fillorder=2),
    "unassociated alpha": lambda: W.write(np.dstack([RGB, G]), 2, extra=2),
    "old-style LZW": lambda: W.write(G, 1, "lzw", codec=lambda d: b"\x00\x01" + W.lzw(d)[0][2:]),
    "above 2^28 pixels": lambda: _retag(_retag(W.write(G, 1), 256, 1 << 15), 257, (1 << 13) + 1),
}


# what each refusal's message names
NAMED = {w: w for w in UNSUPPORTED}
NAMED.update({"above 2^28 pixels": "2^28 pixels", "tiled files": "TileWidth", "planar-separate": "PlanarConfiguration 2",
              "old-style JPEG": "old-style JPEG", "old-style LZW": "old-style LZW", "CCITT compression": "CCITT"})


@pytest.mark.parametrize("what", sorted(UNSUPPORTED))
def test_refused_variants_are_named(what):
    f = UNSUPPORTED[what]()
    for call in (lambda: A.decode_tiff(f), lambda: A.tiff_info(f), lambda: A.tiff_host_stage(f)):
        with pytest.raises(A.AeonHipError) as e:
            call()
        msg = str(e.value).split(": ", 1)[1]
        assert e.value.code == EUNSUPPORTED and msg.startswith("TIFF: ") and msg.endswith("not supported"), (what, msg)
        assert NAMED[what].lower() in msg.lower(), (what, msg)


MALFORMED = {
    "IFD past the end": lambda: W.write(G, 1)[:4] + struct.pack("<I", 4000) + W.write(G, 1)[8:],
    "IFD entries past the end": lambda: W.write(G, 1)[:-30],
    "tag values past the end": lambda: _cut_values(),
    "strip past the end": lambda: _retag(W.write(G, 1), 279, 1 << 20),
    "zero width": lambda: _retag(W.write(G, 1), 256, 0),
    "zero height": lambda: _retag(W.write(G, 1), 257, 0),
    "too few strips": lambda: _retag(W.write(G, 1, rps=3), 278, 1),
    "counts disagree": lambda: _retag(W.write(G, 1), 279, 5),
    "BitsPerSample count": lambda: W.write(RGB, 2, more_tags=[(258, 3, [8, 8])]),
    "no StripByteCounts, compressed": lambda: W.write(G, 1, "lzw", bytecounts=False),
    "palette without ColorMap": lambda: W.write(G, 3),
    "bad version": lambda: W.write(G, 1, version=41),
    "bad zlib header": lambda: W.write(G, 1, "deflate", codec=lambda d: b"\x78\x02" + W.deflate_stored(d)[2:]),
}


def _cut_values():
    """The StripOffsets array (three LONGs, out of line) moved past the end of the file."""
    f = W.write(RGB, 2, rps=1)
    (ifd,) = struct.unpack_from("<I", f, 4)
    (n,) = struct.unpack_from("<H", f, ifd)
    for k in range(n):
        at = ifd + 2 + 12 * k
        if struct.unpack_from("<H", f, at)[0] == 273:
            return f[:at + 8] + struct.pack("<I", len(f) - 8) + f[at + 12:]
    raise KeyError(273)


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_files_are_invalid(what):
    f = MALFORMED[what]()
    with pytest.raises(A.AeonHipError) as e:
        A.decode_tiff(f)
    assert e.value.code == EINVAL and str(e.value).split(": ", 1)[1].startswith("TIFF: "), (what, str(e.value))
    with pytest.raises(A.AeonHipError) as e2:
        A.tiff_host_stage(f)
    assert (e2.value.code, str(e2.value)) == (e.value.code, str(e.value)), what


def test_corrupt_strip_data_is_invalid_on_the_host():
    for name, f in TC.corrupt_files():
        with pytest.raises(A.AeonHipError) as e:
            A.decode_tiff(f)
        assert e.value.code == EINVAL and "TIFF: strip 0" in str(e.value), (name, str(e.value))


def test_sniff_is_strict():
    f = W.write(G, 1)
    assert A.tiff_decoder_route(f) is True
    for g in [b"II" + struct.pack("<HI", 41, 8) + f[8:], f[:4] + struct.pack("<I", len(f)) + f[8:], b"II*", f[:7]]:
        assert A.tiff_decoder_route(g) is False
