"""The files of the packed pixmap calls' tests (RLE8 / RLE4 and 16-bit BMP) with their
references.  An RLE case is a size, a depth and an explicit token list: rle_file writes the list out as a file,
rle_paint paints the same list onto a numpy canvas and never sees the bytes.  Tokens: ("run", n, v), ("lit", [indices]),
("eol",), ("end",), ("delta", dx, dy), ("raw", bytes).  Test infrastructure only.
"""
import functools
import struct

import numpy as np

from tests import pixmap_ref as R
from tests import pixmap_writer as W


def palette(n):
    i = np.arange(n)
    return np.stack([i * 7 + 1, i * 13 + 2, i * 29 + 3], 1).astype(np.uint8)


def rle_file(w, h, depth, tokens, pal_n=None, gap=0, cut=0):
    """gap: bytes between the palette and the stream (its alignment); cut: bytes dropped from the stream's end."""
    s = bytearray()
    for t in tokens:
        if t[0] == "run":
            s += bytes([t[1], t[2]])
        elif t[0] == "lit":
            idx = list(t[1])
            pay = bytes(idx) if depth == 8 else bytes(a << 4 | b for a, b in zip(idx[0::2], (idx + [0])[1::2]))
            s += bytes([0, len(idx)]) + pay + b"\0" * (len(pay) & 1)
        elif t[0] == "raw":
            s += t[1]
        else:
            s += {"eol": b"\0\0", "end": b"\0\1", "delta": b"\0\2"}[t[0]] + bytes(t[1:])
    s = s[:len(s) - cut]
    n = pal_n or 1 << depth
    pal = np.concatenate([palette(n), np.zeros((n, 1), np.uint8)], 1).tobytes()
    off = 54 + len(pal) + gap
    info = struct.pack("<IiiHHIIiiII", 40, w, h, 1, depth, 1 if depth == 8 else 2, len(s), 2835, 2835, pal_n or 0, 0)
    return b"BM" + struct.pack("<IHHI", off + len(s), 0, 0, off) + info + pal + b"\xEE" * gap + bytes(s)


def rle_paint(w, h, depth, tokens):
    """The palette indices the tokens paint, top row first; None where a run or literal leaves the image."""
    c, x, y = np.zeros((h, w), np.uint8), 0, 0
    for t in tokens:
        if t[0] == "eol":
            x, y = 0, y + 1
        elif t[0] == "delta":
            x, y = x + t[1], y + t[2]
        elif t[0] in ("end", "raw"):
            break
        else:
            px = t[1] if t[0] == "lit" else [t[2] if depth == 8 else (t[2] >> 4, t[2] & 15)[i & 1] for i in range(t[1])]
            if x + len(px) > w or y >= h:
                return None
            c[h - 1 - y, x:x + len(px)] = px
            x += len(px)
    return c


def expected(idx, mode, pal_n):
    pal = np.zeros((256, 3), np.uint8)
    pal[:pal_n] = palette(pal_n)
    return pal[idx] if mode == R.BGR8 else R.gray(pal[:, 0], pal[:, 1], pal[:, 2]).astype(np.uint8)[idx]


RUN, LIT, EOL, END = (lambda n, v: ("run", n, v)), (lambda *i: ("lit", list(i))), ("eol",), ("end",)
ROW = [RUN(5, 9), EOL]  # two words

# name: (w, h, depth, tokens, palette entries or None, gap, cut)
RLE = {
    "width_1": (1, 3, 8, [RUN(1, 4), EOL, RUN(1, 5), EOL, RUN(1, 6), END], None, 0, 0),
    "run_255_eol_at_width": (255, 2, 8, [RUN(255, 7), EOL, RUN(3, 1), EOL, END], None, 1, 0),
    "literals_odd_even": (9, 2, 8, [LIT(1, 2, 3), LIT(4, 5, 6, 7), RUN(2, 8), EOL, LIT(9, 8, 7, 6, 5), RUN(4, 1), END], None, 2, 0),
    "rle4_runs": (12, 2, 4, [RUN(5, 0x12), RUN(4, 0x34), RUN(3, 0x5F), EOL, RUN(1, 0xA0), RUN(2, 0xBC), END], None, 3, 0),
    "rle4_literals": (12, 2, 4, [LIT(1, 2, 3), LIT(4, 5, 6, 7), LIT(8, 9, 10, 11, 12), EOL, RUN(1, 0x10), LIT(15, 14, 13), END],
                      None, 0, 0),
    "delta_rows_skipped": (10, 5, 8, [RUN(2, 3), ("delta", 3, 2), RUN(2, 4), EOL, ("delta", 1, 1), LIT(5, 6, 7), RUN(6, 2), END], None, 0, 0),
    "delta_across_window": (80, 3, 8, [RUN(1, 2)] * 63 + [("delta", 2, 1), RUN(3, 5), EOL, RUN(80, 6), END], None, 1, 0),
    "literal_across_window": (80, 2, 8, [RUN(1, 3)] * 60 + [LIT(*range(10, 19)), RUN(2, 4), EOL, RUN(7, 1)], None, 0, 0),
    "literal_over_a_window": (300, 2, 8, [RUN(1, 1)] * 10 + [LIT(*range(1, 256)), RUN(9, 2), EOL, LIT(3, 2, 1), RUN(255, 4), RUN(42, 5), END],
                              None, 2, 0),
    "rle4_literal_over_windows": (300, 1, 4, [RUN(3, 0x21)] * 50 + [LIT(*[i % 16 for i in range(149)]), END], None, 1, 0),
    "two_blocks": (8, 1064, 8, ROW * 1023 + [LIT(1, 2, 3, 4, 5, 6, 7), EOL] + ROW * 40 + [END], None, 0, 0),
    "rle4_two_blocks": (7, 1300, 4, [RUN(7, 0x1E), EOL] * 1290 + [("delta", 2, 3), LIT(1, 2, 3), END], None, 3, 0),
    "no_eol_no_end": (6, 2, 8, [RUN(6, 1), EOL, RUN(4, 2)], None, 0, 0),
    "bytes_after_end": (6, 2, 8, [RUN(6, 1), END, ("raw", b"\x09\x09\x00\x05\x01")], None, 0, 0),
    "short_palette": (6, 1, 8, [LIT(0, 2, 3, 200), RUN(2, 255), END], 3, 0, 0),
}
# Pillow decodes these: RLE8, a whole palette, painted through the top row's last pixel, (0,1) at the end
PILLOW = ("width_1", "run_255_eol_at_width", "literals_odd_even", "delta_rows_skipped", "delta_across_window",
          "literal_over_a_window", "two_blocks")
CORRUPT = {
    "run_past_width": (6, 2, 8, [RUN(4, 1), RUN(3, 2), END], None, 0, 0),
    "literal_past_width": (6, 2, 8, [EOL, RUN(4, 1), LIT(1, 2, 3), END], None, 0, 0),
    "pixels_at_height": (6, 2, 8, [RUN(6, 1), EOL, RUN(6, 2), EOL, RUN(1, 3), END], None, 0, 0),
    "literal_cut_off": (9, 70, 8, [RUN(2, 1), EOL] * 31 + [LIT(1, 2, 3, 4, 5, 6, 7)], None, 1, 4),  # in the next window
    "delta_cut_off": (9, 2, 8, [RUN(2, 1), ("delta", 1, 1)], None, 0, 1),
}

# 16-bit and bitfields files: the values 0, 0x7FFF, 0xFFFF and a mid pattern among others, odd and even widths
M555, M565, M888 = (0x7C00, 0x03E0, 0x001F), (0xF800, 0x07E0, 0x001F), (0xFF0000, 0xFF00, 0xFF)


def words(w, h):
    a = (np.arange(w * h, dtype=np.uint32) * 0x2F1B + 0x1234).astype(np.uint16).reshape(h, w)
    a.flat[:4] = [0, 0x7FFF, 0xFFFF, 0x5A3C]
    return a


def bitfields(a, bpp, masks, top_down):
    f = bytearray(W.bmp(a, bpp, header=52, compression=3, top_down=top_down))
    f[54:66] = struct.pack("<III", *masks)
    return bytes(f)


def expected16(a, is565, mode):
    """The issue's shifts: no bit replication."""
    a = a.astype(np.uint32)
    bgr = np.stack([(a << 3) & 0xF8, (a >> 3) & 0xFC if is565 else (a >> 2) & 0xF8, (a >> 8) & 0xF8 if is565 else (a >> 7) & 0xF8], 2)
    return bgr.astype(np.uint8) if mode == R.BGR8 else R.gray(bgr[:, :, 0], bgr[:, :, 1], bgr[:, :, 2]).astype(np.uint8)


def wide_files():
    """[(name, file, mode -> reference)]"""
    out = []
    for w, td in ((3, False), (4, True)):
        a = words(w, 3)
        out.append((f"rgb555_{w}", W.bmp(a, 16, top_down=td), lambda m, a=a: expected16(a, False, m)))
        out.append((f"bf555_{w}", bitfields(a, 16, M555, not td), lambda m, a=a: expected16(a, False, m)))
        out.append((f"bf565_{w}", bitfields(a, 16, M565, td), lambda m, a=a: expected16(a, True, m)))
        px = np.stack([a & 0xFF, a >> 8, (a * 3) & 0xFF, a & 0x55], 2).astype(np.uint8)
        f = bitfields(px, 32, M888, td)
        plain = bytearray(f)
        plain[30:34] = struct.pack("<I", 0)  # the BI_RGB file it equals
        out.append((f"bf888_{w}", f, lambda m, p=bytes(plain): R.decode(p, m)))
    return out


@functools.lru_cache(None)
def good():
    """[(name, file, mode, reference)]: every good file in the three modes, computed once."""
    out = []
    for name, (w, h, d, toks, pn, gap, cut) in RLE.items():
        idx = rle_paint(w, h, d, toks)
        out += [(name, rle_file(w, h, d, toks, pn, gap, cut), m, expected(idx, m, pn or 1 << d)) for m in (R.BGR8, R.GRAY8, R.ANYDEPTH)]
    for name, f, ref in wide_files():
        out += [(name, f, m, ref(m)) for m in (R.BGR8, R.GRAY8, R.ANYDEPTH)]
    return out


def corrupt():
    """[(name, file)]: the painter leaves the image, or the stream is cut inside a token."""
    assert all(rle_paint(*c[:4]) is None for n, c in CORRUPT.items() if "cut_off" not in n)
    return [(n, rle_file(*c)) for n, c in CORRUPT.items()]
