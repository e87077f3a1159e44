"""CPU: the opt-in PNG path for Adam7-interlaced files (aeon_png_interlaced_route, aeon_png_gpu_emulate_interlaced:
png_unfilter_adam7's code, png_inflate.hpp, run lane after lane) against the Pillow-pinned fixtures, the oracle and
the host decoder, bit for bit.  The case lists below are tests/test_hip_png_adam7.py's too.
"""
import os

import numpy as np
import pytest

import aeon_amd as A
from oracle import png_oracle as PO
from tests import png_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, "golden", "png_fixtures.npz"))
INTER = sorted({k.rsplit(".", 1)[0] for k in FX.files if k.endswith("_i.png")})
MODES = [(A.PNG_BGR8, "bgr8"), (A.PNG_GRAY8, "gray8"), (A.PNG_ANYDEPTH, "any")]
EDEVICE = -4
X0, Y0, DX, DY = (0, 4, 0, 2, 0, 1, 0), (0, 0, 4, 0, 2, 0, 1), (8, 8, 4, 4, 2, 2, 1), (8, 8, 8, 4, 4, 2, 2)
PAL = bytes(range(48))  # 16 entries


def passes(arr, ctype, depth, filters=(0,)):
    """The seven sub-images' scanlines (b"" for an absent pass), pass k's filters starting at filters[k]."""
    arr = np.asarray(arr)
    subs = [arr[Y0[k]::DY[k], X0[k]::DX[k]] for k in range(7)]
    return [W.scanlines(s, ctype, depth, [filters[(k + y) % len(filters)] for y in range(len(filters))]) if s.size else b""
            for k, s in enumerate(subs)]


def adam7(arr, ctype, depth, filters=(0,), palette=None, raw=None):
    h, w = np.asarray(arr).shape[:2]
    raw = b"".join(passes(arr, ctype, depth, filters)) if raw is None else raw
    return W.png_from_stream(w, h, ctype, depth, W.deflate(raw), palette, interlace=1)


def size_files():
    """Gray 8-bit at every size 1..9 x 1..9: every pattern of absent passes, the five filters cycling."""
    rng = np.random.default_rng(71)
    return [("g8_%dx%d" % (w, h), adam7(rng.integers(0, 256, (h, w)), 0, 8, (0, 1, 2, 3, 4)))
            for w in range(1, 10) for h in range(1, 10)]


def depth_files():
    """Depths 1, 2, 4, gray and palette, widths 1..17 at height 9: the padding bits of every pass row."""
    rng = np.random.default_rng(72)
    return [("%s%d_w%d" % ("gp"[ct == 3], d, w), adam7(rng.integers(0, 1 << d, (9, w)), ct, d, (4, 3, 1, 2, 0), PAL if ct else None))
            for ct in (0, 3) for d in (1, 2, 4) for w in range(1, 18)]


def band_files():
    """5 x 131: pass 7 has 65 rows, two bands with the previous row carried; 5 x 1041: so has pass 1."""
    rng = np.random.default_rng(73)
    out = [("%s_%s" % (name, "paeth" if f == 4 else "avg"), adam7(rng.integers(0, 1 << d, (131, 5, s)), ct, d, (f,)))
           for name, ct, d, s in (("rgb8", 2, 8, 3), ("rgba16", 6, 16, 4), ("ga8", 4, 8, 2)) for f in (4, 3)]
    return out + [("rgb8_h1041", adam7(rng.integers(0, 256, (130 * 8 + 1, 5, 3)), 2, 8, (4, 3)))]


def corrupt_files():
    rng = np.random.default_rng(74)
    g = rng.integers(0, 256, (12, 12))
    p = passes(g, 0, 8, (1, 2))
    filter5 = b"".join(p[:2]) + b"\x05" + p[2][1:] + b"".join(p[3:])  # pass 3's first filter byte
    idx = rng.integers(0, 16, (12, 12))
    idx[2, 5] = 200  # x odd, y even: a pixel of pass 6 alone
    return [("filter5_pass3", adam7(g, 0, 8, raw=filter5)),
            ("palette_index_pass6", adam7(idx, 3, 8, (0, 1), PAL)),
            ("truncated_pass7", adam7(g, 0, 8, raw=b"".join(p)[:-20]))]


def _check(named):
    for name, png in named:
        assert A.png_interlaced_route(png) and A.png_info(png)[0] > 0, name
        for m, _ in MODES:
            want = PO.decode(png, m)
            got = A.png_gpu_emulate(png, m, interlaced=True)
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, m)
            assert np.array_equal(A.decode_png(png, m), want), (name, m)


@pytest.mark.parametrize("name", INTER)
def test_fixtures(name):
    png = FX[name + ".png"].tobytes()
    assert png[28] == 1 and A.png_interlaced_route(png) and not A.png_host_stage(png)[0]
    for m, key in MODES:
        got = A.png_gpu_emulate(png, m, interlaced=True)
        assert got.dtype == FX[name + "." + key].dtype and np.array_equal(got, FX[name + "." + key]), key
        assert np.array_equal(got, A.decode_png(png, m)), key


@pytest.mark.parametrize("files", [size_files, depth_files, band_files])
def test_lists(files):
    _check(files())


def test_routing_edge_at_the_widest_pass_row():
    rng = np.random.default_rng(75)
    for w, routed in ((16383, True), (16384, False)):
        png = adam7(rng.integers(0, 256, (3, w)), 0, 8, (1, 4, 3))
        assert A.png_interlaced_route(png) == routed, w
        if routed:
            assert np.array_equal(A.png_gpu_emulate(png, A.PNG_ANYDEPTH, interlaced=True), A.decode_png(png, A.PNG_ANYDEPTH))
        else:
            with pytest.raises(A.AeonHipError) as e:
                A.png_gpu_emulate(png, A.PNG_ANYDEPTH, interlaced=True)
            assert e.value.code == -3


@pytest.mark.parametrize("case", range(3))
def test_refusals(case):
    name, png = corrupt_files()[case]
    assert A.png_interlaced_route(png), name
    with pytest.raises(A.AeonHipError) as e:
        A.png_gpu_emulate(png, A.PNG_ANYDEPTH, interlaced=True)
    assert e.value.code == EDEVICE, (name, str(e.value))
    with pytest.raises(A.AeonHipError):
        A.decode_png(png, A.PNG_ANYDEPTH)


def test_defaults_are_unchanged():
    png = FX["pal4_i.png"].tobytes()
    with pytest.raises(A.AeonHipError) as e:
        A.png_gpu_emulate(png)
    assert e.value.code == -3
    assert A.png_host_stage(png) == (False, 23 * 10 * 3)
