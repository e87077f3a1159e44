"""The pixmap decoder on the CPU (aeon_pixmap_info, aeon_decode_pixmap: BMP and PNM files) against the numpy
restatement of the decode rules (tests/pixmap_ref.py) and, for the rules the formats pin, against Pillow's decode of
the same bytes (tests/golden/pixmap_fixtures.npz), and each refusal with its code and message prefix.  (What a
Decoder does with files that are neither BMP nor PNM needs a device: tests/test_hip_pixmap.py.)
"""
import os
import struct

import numpy as np
import pytest

import aeon_amd as A
from tests import pixmap_cases as PC
from tests import pixmap_ref as R
from tests import pixmap_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, "golden", "pixmap_fixtures.npz"))
NAMES = sorted({k.rsplit(".", 1)[0] for k in FX.files})
MODES = [(A.DECODE_BGR8, "bgr8"), (A.DECODE_GRAY8, "gray8"), (A.DECODE_ANYDEPTH, "any")]


def test_constants_are_the_png_modes():
    assert (A.DECODE_BGR8, A.DECODE_GRAY8, A.DECODE_ANYDEPTH) == (A.PNG_BGR8, A.PNG_GRAY8, A.PNG_ANYDEPTH) == (0, 1, 2)


def test_fixtures_pillow_pins():
    n = 0
    for name in NAMES:
        f = FX[name + ".file"].tobytes()
        for mode, key in MODES:
            got, ref = A.decode_pixmap(f, mode), R.decode(f, mode)
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (name, key)
            if name + "." + key in FX.files:
                want = FX[name + "." + key]
                assert got.dtype == want.dtype and np.array_equal(got, want), (name, key, "Pillow")
                n += 1
    assert len(NAMES) >= 30 and n >= 45


@pytest.mark.parametrize("group", ["device_files", "ascii_files"])
def test_decoder_matches_reference(group):
    files = getattr(PC, group)()
    assert len(files) > 90
    for name, f in files:
        for mode, _ in MODES:
            got, want = A.decode_pixmap(f, mode), R.decode(f, mode)
            assert got.dtype == want.dtype and got.shape == want.shape, (name, mode)
            assert np.array_equal(got, want), (name, mode, np.argwhere(got != want)[:3].tolist())


def test_info():
    assert A.pixmap_info(W.pnm(6, np.zeros((2, 5, 3), int), 255)) == (5, 2, 8, 3, 6)
    assert A.pixmap_info(W.pnm(5, np.zeros((3, 4), int), 256)) == (4, 3, 16, 1, 5)
    assert A.pixmap_info(W.pnm(1, np.zeros((3, 4), int))) == (4, 3, 8, 1, 1)
    assert A.pixmap_info(W.bmp(np.zeros((3, 4), int), 8, np.zeros((256, 3), int), top_down=True)) == (4, 3, 8, 3, A.PIXMAP_BMP)


def test_unpinned_rules_by_hand():
    """The rules no reference output pins, spelled out on single pixels."""
    g = lambda b, g_, r: (b * 1868 + g_ * 9617 + r * 4899 + 8192) >> 14
    px = W.pnm(6, np.array([[[200, 100, 50]]]), 255)  # R, G, B
    assert A.decode_pixmap(px, A.DECODE_BGR8).tolist() == [[[50, 100, 200]]]
    assert A.decode_pixmap(px, A.DECODE_GRAY8).tolist() == [[g(50, 100, 200)]]
    # binary samples are not scaled by maxval; ASCII samples are clamped, then v * 255 / maxval
    assert A.decode_pixmap(W.pnm(5, np.array([[9]]), 15), A.DECODE_GRAY8).tolist() == [[9]]
    assert A.decode_pixmap(W.pnm(2, np.array([[9, 15, 99]]), 15), A.DECODE_GRAY8).tolist() == [[9 * 255 // 15, 255, 255]]
    # 16-bit: native under ANYDEPTH, the high byte of each sample otherwise; the gray formula on 16-bit samples
    wide = W.pnm(6, np.array([[[0x1234, 0xABCD, 0xFF01]]]), 65535)
    assert A.decode_pixmap(wide, A.DECODE_BGR8).tolist() == [[[0xFF, 0xAB, 0x12]]]
    assert A.decode_pixmap(wide, A.DECODE_GRAY8).tolist() == [[g(0xFF, 0xAB, 0x12)]]
    any_ = A.decode_pixmap(wide, A.DECODE_ANYDEPTH)
    assert any_.dtype == np.uint16 and any_.tolist() == [[g(0xFF01, 0xABCD, 0x1234)]]
    # P1 / P4: bit 1 is black
    assert A.decode_pixmap(W.pnm(1, np.array([[0, 1]]), digits_tight=True), A.DECODE_GRAY8).tolist() == [[255, 0]]
    # an index past a short palette is black; gray from a palette file is the gray of the entry
    f = W.bmp(np.array([[0, 1, 2, 3]]), 4, np.array([[10, 20, 30], [200, 0, 0]]))
    assert A.decode_pixmap(f, A.DECODE_BGR8).tolist() == [[[10, 20, 30], [200, 0, 0], [0, 0, 0], [0, 0, 0]]]
    assert A.decode_pixmap(f, A.DECODE_ANYDEPTH).tolist() == [[g(10, 20, 30), g(200, 0, 0), 0, 0]]


def _patch(f, at, fmt, v):
    return f[:at] + struct.pack(fmt, v) + f[at + struct.calcsize(fmt):]


def _refusals():
    p6 = W.pnm(6, np.zeros((2, 3, 3), int), 255)
    p2 = W.pnm(2, np.ones((2, 3), int), 255)
    b24 = W.bmp(np.zeros((2, 3, 3), int), 24)
    b8 = W.bmp(np.zeros((2, 3), int), 8, np.zeros((256, 3), int))
    return [
        ("pnm short data", p6[:-1], -1, "PNM:"),
        ("pnm no maxval", b"P6\n3 2\n", -1, "PNM:"),
        ("pnm maxval 0", b"P5\n1 1\n0\n\x00", -1, "PNM:"),
        ("pnm maxval 65536", b"P5\n1 1\n65536\n\x00\x00", -1, "PNM:"),
        ("pnm width 0", b"P5\n0 1\n255\n\x00", -1, "PNM:"),
        ("pnm height 0", b"P5\n1 0\n255\n\x00", -1, "PNM:"),
        ("pnm too many pixels", b"P4\n32768 8193\n" + b"\x00" * 64, -1, "PNM:"),
        ("pnm no whitespace before the data", b"P5\n1 1\n255", -1, "PNM:"),
        ("pnm letters", b"P5\nab 1\n255\n\x00", -1, "PNM:"),
        ("pnm ascii runs out", p2[:-4], -1, "PNM:"),
        ("pnm P1 runs out", b"P1\n3 2\n01101", -1, "PNM:"),
        ("bmp header size 20", _patch(b24, 14, "<I", 20), -1, "BMP:"),
        ("bmp header size 39", _patch(b24, 14, "<I", 39), -1, "BMP:"),
        ("bmp width 0", _patch(b24, 18, "<i", 0), -1, "BMP:"),
        ("bmp height 0", _patch(b24, 22, "<i", 0), -1, "BMP:"),
        ("bmp too many pixels", _patch(_patch(b24, 18, "<i", 1 << 15), 22, "<i", (1 << 13) + 1), -1, "BMP:"),
        ("bmp short data", b24[:-1], -1, "BMP:"),
        ("bmp bfOffBits past the end", _patch(b24, 10, "<I", len(b24)), -1, "BMP:"),
        ("bmp 257 palette entries", _patch(b8, 46, "<I", 257), -1, "BMP:"),
        ("bmp bit count 2", _patch(b24, 28, "<H", 2), -1, "BMP:"),
        ("bmp RLE8", W.bmp(np.zeros((2, 3), int), 8, np.zeros((256, 3), int), compression=1), -3, "BMP: RLE8"),
        ("bmp RLE4", W.bmp(np.zeros((2, 3), int), 4, np.zeros((16, 3), int), compression=2), -3, "BMP: RLE4"),
        ("bmp 16-bit", W.bmp(np.zeros((2, 3), int), 16), -3, "BMP: 16-bit"),
        ("bmp bitfields", W.bmp(np.zeros((2, 3, 4), int), 32, compression=3), -3, "BMP: 16-bit"),
    ]


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0])
def test_refusals(case):
    name, f, code, prefix = case
    with pytest.raises(R.Refused) as r:
        R.decode(f, R.BGR8)
    assert r.value.code == code and prefix.startswith(r.value.prefix.rstrip(":")), name
    with pytest.raises(A.AeonHipError) as e0:
        A.decode_pixmap(f)
    assert e0.value.code == code and str(e0.value).split(": ", 1)[1].startswith(prefix), (name, str(e0.value))
    # the stage's host half refuses the same file with the same code and message, before any launch
    for mode in (A.DECODE_BGR8, A.DECODE_GRAY8, A.DECODE_ANYDEPTH):
        with pytest.raises(A.AeonHipError) as e1:
            A.pixmap_host_stage(f, mode)
        assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value)), name


def test_bad_mode_and_stride():
    f = W.pnm(5, np.zeros((2, 3), int), 255)
    with pytest.raises(A.AeonHipError):
        A.decode_pixmap(f, 3)
    with pytest.raises(A.AeonHipError):
        A.pixmap_host_stage(f, -1)
