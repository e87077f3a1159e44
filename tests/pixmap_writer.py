"""Writes PNM (P1..P6) and BMP files from arrays, in every variant the pixmap tests need: header comments of a
chosen length (so the pixel data starts at any alignment), bfOffBits gaps, the OS/2 core header and the 40 / 108 /
124-byte info headers, top-down rows, palettes shorter than 1 << bpp.  Test infrastructure only: it encodes what
the arrays say and knows nothing of how the product decodes.
"""
import struct

import numpy as np


def pnm(magic, a, maxval=255, comment=None, sep=b"\n", ascii_sep=b" ", digits_tight=False):
    """A PNM file.  magic 1..6; a: HxW (P1/P2/P4/P5) or HxWx3 (P3/P6) array of sample values (P1/P4: bits, 1 =
    black).  comment: None or a number of bytes a `#` comment line in the header takes in all (>= 2).
    digits_tight: P1 samples with no separator between them."""
    a = np.asarray(a)
    h, w = a.shape[:2]
    head = b"P%d\n" % magic
    if comment is not None:
        assert comment >= 2
        head += b"#" + b"c" * (comment - 2) + b"\n"
    head += b"%d %d" % (w, h)
    if magic not in (1, 4):
        head += b"\n%d" % maxval
    head += sep[:1]
    if magic == 4:
        body = np.packbits(a.astype(bool), axis=1).tobytes()
    elif magic in (5, 6):
        body = (a.astype(">u2") if maxval > 255 else a.astype(np.uint8)).tobytes()
    elif magic == 1:
        rows = [(b"" if digits_tight else ascii_sep).join(b"%d" % v for v in r) for r in a.reshape(h, -1)]
        body = b"\n".join(rows) + b"\n"
    else:
        rows = [ascii_sep.join(b"%d" % v for v in r) for r in a.reshape(h, -1)]
        body = b"\n# a comment between rows\n".join(rows) + b"\n"
    return head + body


def bmp(a, bpp, palette=None, header=40, top_down=False, gap=0, clr_used=None, compression=0, trailer=b""):
    """A BMP file.  a: HxW indices (bpp 1, 4, 8) or HxWx3 / HxWx4 B,G,R(,x) samples (bpp 24 / 32); bpp 16: HxW
    uint16 words.  palette: Nx3 B,G,R entries (stored as N entries; clr_used defaults to N when N != 1 << bpp).
    header: 12 (core) or >= 40.  gap: bytes between the palette and the pixel data (bfOffBits moves)."""
    a = np.asarray(a)
    h, w = a.shape[:2]
    if header == 12:
        top_down = False  # a core header's height is unsigned: bottom-up only
    pitch = ((w * bpp + 7) // 8 + 3) & ~3
    rows = np.zeros((h, pitch), np.uint8)
    if bpp == 1:
        packed = np.packbits(a.astype(bool), axis=1)
        rows[:, :packed.shape[1]] = packed
    elif bpp == 4:
        p = np.zeros((h, (w + 1) // 2 * 2), np.uint8)
        p[:, :w] = a
        rows[:, :p.shape[1] // 2] = (p[:, 0::2] << 4) | p[:, 1::2]
    elif bpp == 8:
        rows[:, :w] = a
    elif bpp == 16:
        rows[:, :2 * w] = a.astype("<u2").view(np.uint8).reshape(h, 2 * w)
    else:
        rows[:, :w * bpp // 8] = a.astype(np.uint8).reshape(h, -1)
    if not top_down:
        rows = rows[::-1]
    pal = b""
    if palette is not None:
        palette = np.asarray(palette, np.uint8).reshape(-1, 3)
        if header == 12:
            pal = palette.tobytes()
        else:
            pal = np.concatenate([palette, np.zeros((len(palette), 1), np.uint8)], 1).tobytes()
        if clr_used is None:
            clr_used = 0 if len(palette) == (1 << bpp) else len(palette)
    clr_used = clr_used or 0
    off = 14 + header + len(pal) + gap
    if header == 12:
        info = struct.pack("<IHHHH", 12, w, h, 1, bpp)
    else:
        info = struct.pack("<IiiHHIIiiII", header, w, -h if top_down else h, 1, bpp, compression, pitch * h, 2835, 2835,
                           clr_used, 0)
        info += b"\x00" * (header - 40)
    body = rows.tobytes()
    size = off + len(body) + len(trailer)
    return b"BM" + struct.pack("<IHHI", size, 0, 0, off) + info + pal + b"\xEE" * gap + body + trailer
