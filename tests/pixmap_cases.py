"""The BMP / PNM files of the pixmap tests (tests/test_pixmap.py, test_pixmap_stage.py, test_hip_pixmap.py), from
tests/pixmap_writer.py: the smallest shapes at which the conversion can go wrong.  Widths 1-9, 15-17, 31-33, 63-65,
255-257 (dword groups, 1-bit widths that are no multiple of 8, odd 4-bit widths), heights 1, 2, 3, 65 (more than one
band at the wider rows), every source alignment 0..15 (a PNM header padded with a comment, a moved bfOffBits),
bottom-up and top-down BMP, core and 40 / 108 / 124-byte info headers, palettes shorter than 1 << bpp with indices
past them, maxval 1, 15, 255, 256, 65535, and rows wider than one band of the kernel's LDS (16 KiB of source).
"""
import functools

import numpy as np

from tests import pixmap_writer as W

WIDTHS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257]
HEIGHTS = [1, 2, 3, 65]


def _aligned_pnm(magic, a, maxval, align):
    """The file with its pixel data at offset `align` mod 16: the header padded with a comment."""
    base = len(W.pnm(magic, a, maxval)) - _body_len(magic, a, maxval)
    c = (align - base) % 16
    c = c if c >= 2 else (c + 16 if c else None)
    f = W.pnm(magic, a, maxval, comment=c)
    assert (len(f) - _body_len(magic, a, maxval)) % 16 == align
    return f


def _body_len(magic, a, maxval):
    h, w = a.shape[:2]
    if magic == 4:
        return (w + 7) // 8 * h
    return a.size * (2 if maxval > 255 else 1)


@functools.lru_cache(None)
def device_files():
    """(name, file) of files the device converts: binary PNM and BI_RGB BMP."""
    rng = np.random.default_rng(20)
    out = []
    for i, w in enumerate(WIDTHS):
        h = HEIGHTS[i % 4]
        for k, (magic, maxval) in enumerate([(4, 1), (5, 255), (5, 65535), (6, 255), (6, 65535)]):
            shape = (h, w, 3) if magic == 6 else (h, w)
            a = rng.integers(0, 2 if magic == 4 else (65536 if maxval > 255 else 256), shape)
            out.append((f"P{magic}_{maxval}_{w}x{h}", _aligned_pnm(magic, a, maxval, (i + 5 * k) % 16)))
        for k, bpp in enumerate([1, 4, 8, 24, 32]):
            header = [40, 12, 108, 124][(i + k) % 4]
            top = bool((i + k) % 2)
            pal = None
            if bpp <= 8:
                n = 1 << bpp
                if (i + k) % 3 == 0 and header != 12 and bpp > 1:
                    n = n - n // 4  # shorter than 1 << bpp: the indices past it decode as black
                pal = rng.integers(0, 256, (n, 3))
                a = rng.integers(0, 1 << bpp, (h, w))
            else:
                a = rng.integers(0, 256, (h, w, bpp // 8))
            f0 = W.bmp(a, bpp, pal, header, top)
            off = int.from_bytes(f0[10:14], "little")
            gap = ((i + 3 * k) % 16 - off) % 16
            f = W.bmp(a, bpp, pal, header, top, gap=gap, trailer=b"tail" if i % 5 == 0 else b"")
            assert int.from_bytes(f[10:14], "little") % 16 == (i + 3 * k) % 16
            out.append((f"bmp{bpp}_{header}_{'td' if top else 'bu'}_{w}x{h}", f))
    # maxval 1, 15, 255, 256, 65535: binary samples are taken as they are
    for magic in (5, 6):
        for maxval in (1, 15, 255, 256, 65535):
            shape = (3, 7, 3) if magic == 6 else (3, 7)
            a = rng.integers(0, 65536 if maxval > 255 else 256, shape)
            out.append((f"P{magic}_maxval{maxval}", W.pnm(magic, a, maxval) + b"trailing bytes"))
    # rows wider than one band: the band table splits them into pieces of pixels
    out.append(("P6_wide", _aligned_pnm(6, rng.integers(0, 256, (2, 5500, 3)), 255, 7)))
    out.append(("P6_16_wide", _aligned_pnm(6, rng.integers(0, 65536, (2, 2800, 3)), 65535, 3)))
    out.append(("P4_wide", _aligned_pnm(4, rng.integers(0, 2, (2, 131085)), 1, 5)))
    out.append(("bmp24_wide_bu", W.bmp(rng.integers(0, 256, (3, 5470, 3)), 24, gap=3)))
    out.append(("bmp4_wide_td", W.bmp(rng.integers(0, 16, (2, 32771)), 4, rng.integers(0, 256, (16, 3)), top_down=True, gap=1)))
    return out


@functools.lru_cache(None)
def ascii_files():
    """(name, file) of ASCII PNM files (the host route): comments, and P1 digits with no space between them."""
    rng = np.random.default_rng(21)
    out = []
    for i, w in enumerate([1, 2, 3, 5, 8, 9, 17]):
        h = [1, 2, 3][i % 3]
        bits = rng.integers(0, 2, (h, w))
        out.append((f"P1_{w}x{h}", W.pnm(1, bits, comment=5 + i)))
        out.append((f"P1_tight_{w}x{h}", W.pnm(1, bits, digits_tight=True)))
        for maxval in (1, 15, 100, 255, 256, 65535):
            # values past maxval among them: clamped
            a = rng.integers(0, min(65536, maxval + 1 + maxval // 4 + 1), (h, w))
            out.append((f"P2_{maxval}_{w}x{h}", W.pnm(2, a, maxval, comment=3 if i % 2 else None, ascii_sep=b"\t" if i % 2 else b" ")))
            a = rng.integers(0, min(65536, maxval + 1 + maxval // 4 + 1), (h, w, 3))
            out.append((f"P3_{maxval}_{w}x{h}", W.pnm(3, a, maxval)))
    return out
