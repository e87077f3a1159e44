"""Writes tests/golden/pixmap_fixtures.npz: a few dozen tiny BMP / PNM files (tests/pixmap_writer.py) with Pillow's
decode of each, for the decode rules the formats pin and only for those:

  P4 bit polarity and padding        -> <name>.gray8, <name>.bgr8 (replicated)
  P5 at maxval 255                   -> <name>.gray8, <name>.any, <name>.bgr8 (replicated)
  P5 at maxval 65535 (byte order)    -> <name>.any (native uint16)
  P6 at maxval 255 (RGB -> BGR swap) -> <name>.bgr8
  BI_RGB BMP at 1, 4, 8, 24, 32 bpp  -> <name>.bgr8

The unpinned rules (gray constants, maxval handling, indices past a palette) have no entry: Pillow decides them
differently or not at all.  Run from the repository root with Pillow installed: python tests/golden/make_pixmap_fixtures.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import pixmap_writer as W  # noqa: E402


def pil(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def main():
    rng = np.random.default_rng(7)
    out = {}

    def add(name, data, **arrays):
        out[name + ".file"] = np.frombuffer(data, np.uint8)
        for k, v in arrays.items():
            out[name + "." + k] = v

    for w, h in [(1, 1), (7, 2), (8, 3), (9, 2), (17, 3)]:
        bits = rng.integers(0, 2, (h, w))
        f = W.pnm(4, bits, comment=3 + w)
        g = np.asarray(pil(f).convert("L"))
        add(f"p4_{w}x{h}", f, gray8=g, bgr8=np.repeat(g[:, :, None], 3, 2))
        a = rng.integers(0, 256, (h, w))
        f = W.pnm(5, a, 255)
        g = np.asarray(pil(f).convert("L"))
        add(f"p5_{w}x{h}", f, gray8=g, any=g, bgr8=np.repeat(g[:, :, None], 3, 2))
        a = rng.integers(0, 65536, (h, w))
        f = W.pnm(5, a, 65535, comment=2 + h)
        im = pil(f)
        assert im.mode.startswith("I;16") or im.mode == "I", im.mode
        add(f"p5w_{w}x{h}", f, any=np.asarray(im).astype(np.uint16))
        a = rng.integers(0, 256, (h, w, 3))
        f = W.pnm(6, a, 255, comment=4)
        add(f"p6_{w}x{h}", f, bgr8=np.ascontiguousarray(np.asarray(pil(f).convert("RGB"))[:, :, ::-1]))
    k = 0
    for bpp in (1, 4, 8, 24, 32):
        for w, h in [(1, 1), (5, 2), (9, 3)]:
            header, top = [40, 12, 108, 124][k % 4], bool(k % 2)
            k += 1
            if bpp <= 8:
                pal = rng.integers(0, 256, (1 << bpp, 3))
                a = rng.integers(0, 1 << bpp, (h, w))
            else:
                pal, a = None, rng.integers(0, 256, (h, w, bpp // 8))
            if header == 12 and top:
                top = False  # a core header has no sign to carry
            f = W.bmp(a, bpp, pal, header, top, gap=k % 4)
            add(f"bmp{bpp}_{w}x{h}_{header}{'t' if top else 'b'}", f,
                bgr8=np.ascontiguousarray(np.asarray(pil(f).convert("RGB"))[:, :, ::-1]))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pixmap_fixtures.npz")
    np.savez_compressed(path, **out)
    print(len([k for k in out if k.endswith(".file")]), "files ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
