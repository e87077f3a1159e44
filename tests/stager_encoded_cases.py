"""The encoded records of the stager's encoded-path tests (tests/test_stager_encoded.py, tests/test_hip_stager_encoded.py):
one small file per format and per route of the decoder's routing rule, at the record sizes of
tests/test_hip_stager_reuse.py.  Test infrastructure only: Pillow and the tests' own writers encode what the arrays
say; which route a file takes is asked of the library (encoded_info) by the tests, never assumed here.
"""
import functools
import io

import numpy as np

import aeon_amd as A
from tests import pixmap_writer as XW
from tests import tiff_writer as TW

SIZES = [(96, 64), (101, 67), (107, 70), (113, 71), (118, 73), (123, 75), (128, 76), (131, 77)]  # (w, h) of record i


def _smooth(seed, w, h, cn=3):
    """A photo-like image: smooth gradients plus a little noise (JPEG blocks with few coefficients)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [127 + 100 * np.sin((x * (3 + c + seed % 5) + y * (2 + seed % 3)) / 37.0 + seed + c) for c in range(cn)]
    a = np.stack(planes, -1) + (A.synthetic_image(seed, w, h, cn).reshape(h, w, cn) & 7)
    a = np.clip(a, 0, 255).astype(np.uint8)
    return a if cn > 1 else a[:, :, 0]


def _classes(seed, w, h, n=5):
    """A pixel-mask-like image: blocks of n class indices."""
    y, x = np.mgrid[0:h, 0:w]
    return (((x + seed) // 16 + (y + 2 * seed) // 8) % n).astype(np.uint8)


def _pil(arr, fmt, mode=None, palette=None, **kw):
    from PIL import Image
    im = Image.fromarray(arr, mode) if mode else Image.fromarray(arr)
    if palette is not None:
        im.putpalette([int(v) for v in np.asarray(palette).reshape(-1)])
    buf = io.BytesIO()
    im.save(buf, fmt, **kw)
    return buf.getvalue()


PALETTE = [(c * 30, c * 50, 255 - c * 40) for c in range(5)]  # R, G, B

# name -> (format, device route the file is meant for)
IMAGE_KINDS = [("jpeg420", A.FORMAT_JPEG, True), ("jpeg_gray", A.FORMAT_JPEG, True), ("jpeg_prog", A.FORMAT_JPEG, True),
               ("png_palette", A.FORMAT_PNG, True), ("png_noise", A.FORMAT_PNG, False), ("ppm_p6", A.FORMAT_PIXMAP, True),
               ("bmp_pal8", A.FORMAT_PIXMAP, True), ("tiff_lzw", A.FORMAT_TIFF, True)]


def image_file(kind, seed, w, h):
    """One encoded image of `kind`, w x h, its pixels a function of seed."""
    if kind == "jpeg420":
        return _pil(_smooth(seed, w, h), "JPEG", quality=85, subsampling=2)
    if kind == "jpeg_gray":
        return _pil(_smooth(seed, w, h, 1), "JPEG", quality=80)
    if kind == "jpeg_prog":
        return _pil(_smooth(seed, w, h), "JPEG", quality=75, subsampling=1, progressive=True)
    if kind == "png_palette":
        return _pil(_classes(seed, w, h), "PNG", "P", PALETTE)
    if kind == "png_noise":
        return _pil(A.synthetic_image(seed, w, h, 3), "PNG")
    if kind == "ppm_p6":
        return XW.pnm(6, A.synthetic_image(seed, w, h, 3))
    if kind == "ppm_p3":
        return XW.pnm(3, A.synthetic_image(seed, w, h, 3))
    if kind == "bmp_pal8":
        pal = A.synthetic_image(seed + 7, 256, 1, 3).reshape(256, 3)
        return XW.bmp(A.synthetic_image(seed, w, h, 1), 8, palette=pal)
    if kind == "tiff_lzw":  # strips of about 8 KB
        return TW.write(_smooth(seed, w, h), 2, comp="lzw", rps=max(1, 8192 // (3 * w)))
    if kind == "tiff_lzw_big":  # one LZW strip above 32 KiB: the host decodes it
        return TW.write(_smooth(seed, w, h), 2, comp="lzw")
    if kind == "tiff_deflate_noise":
        return TW.write(A.synthetic_image(seed, w, h, 3), 2, comp="deflate", rps=16)
    raise KeyError(kind)


def decode_image(data, channels=3):
    """The record's pixels as the reference decodes them: oracle.jpeg_decode for a JPEG file, else the library's host
    decoder of the format (BGR8 for 3 channels, GRAY8 for 1)."""
    import oracle as O
    mode = A.DECODE_BGR8 if channels == 3 else A.DECODE_GRAY8
    fmt = A.encoded_info(data)["format"]
    if fmt == A.FORMAT_JPEG:
        return O.jpeg_decode(data, channels)
    return {A.FORMAT_PNG: A.decode_png, A.FORMAT_PIXMAP: A.decode_pixmap, A.FORMAT_TIFF: A.decode_tiff}[fmt](data, mode)


MASK_KINDS = ["png_gray16", "tiff_gray16", "png_palette"]


def mask_file(kind, seed, w, h):
    cls = _classes(seed, w, h)
    if kind == "png_gray16":
        return _pil((cls.astype(np.uint16) * 97 + seed % 50).astype(np.uint16), "PNG")
    if kind == "tiff_gray16":
        return TW.write((cls.astype(np.uint16) * 61 + seed % 40).astype(np.uint16), 1, comp="lzw", rps=16)
    if kind == "png_palette":
        return _pil(cls, "PNG", "P", PALETTE)
    raise KeyError(kind)


def decode_mask(data):
    fmt = A.encoded_info(data, mask=True)["format"]
    return {A.FORMAT_PNG: A.decode_png, A.FORMAT_PIXMAP: A.decode_pixmap, A.FORMAT_TIFF: A.decode_tiff}[fmt](
        data, A.DECODE_ANYDEPTH)


@functools.lru_cache(maxsize=None)
def window(win):
    """The 8 image files of window `win` (one of every IMAGE_KINDS, record i at SIZES[i]): the same sizes in every
    window, other pixels.  Computed once; read-only."""
    return tuple(image_file(kind, 1000 * win + i, *SIZES[i]) for i, (kind, _, _) in enumerate(IMAGE_KINDS))


@functools.lru_cache(maxsize=None)
def window_decoded(win):
    out = tuple(decode_image(f) for f in window(win))
    for a in out:
        a.setflags(write=False)
    return out
