"""A PNG writer on the standard library (and numpy for the filters), for files no encoder produces on request:
a chosen filter type per row, a chosen deflate form (stored blocks, Z_FIXED, dynamic, several blocks through
Z_FULL_FLUSH), deflate streams assembled bit by bit (fixed-Huffman blocks from literals and (length, distance)
pairs -- zlib's own matcher never emits a distance above 32,506 -- and dynamic blocks from explicit code
lengths), and IDAT chunks split at given byte counts.  Helper of tests/test_png_stage.py and
tests/test_hip_png.py; no test of its own.
"""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def row_bytes(w, ctype, depth):
    return (w * SAMPLES[ctype] * depth + 7) // 8


def pack_rows(arr, ctype, depth):
    """arr: (h, w) or (h, w, samples) integer samples -> (h, rowbytes) uint8 as PNG lays them out."""
    a = np.asarray(arr)
    h, w = a.shape[:2]
    a = a.reshape(h, w * SAMPLES[ctype]).astype(np.uint32)
    if depth == 16:
        out = np.empty((h, a.shape[1] * 2), np.uint8)
        out[:, 0::2], out[:, 1::2] = a >> 8, a & 255
        return out
    if depth == 8:
        return a.astype(np.uint8)
    per = 8 // depth
    pad = (-a.shape[1]) % per
    a = np.pad(a, ((0, 0), (0, pad)))
    out = np.zeros((h, a.shape[1] // per), np.uint32)
    for k in range(per):
        out |= a[:, k::per] << (8 - depth * (k + 1))
    return out.astype(np.uint8)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(rows, bpp, filters):
    """The scanlines of a (h, rowbytes) uint8 picture, row y filtered with type filters[y % len(filters)]."""
    h, n = rows.shape
    out = np.zeros((h, n + 1), np.uint8)
    zero = np.zeros(n, np.int32)
    for y in range(h):
        ft = filters[y % len(filters)]
        cur = rows[y].astype(np.int32)
        up = rows[y - 1].astype(np.int32) if y else zero
        left = np.concatenate([np.zeros(min(bpp, n), np.int32), cur[:-bpp] if n > bpp else cur[:0]])[:n]
        upleft = np.concatenate([np.zeros(min(bpp, n), np.int32), up[:-bpp] if n > bpp else up[:0]])[:n]
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - left
        elif ft == 2:
            f = cur - up
        elif ft == 3:
            f = cur - ((left + up) >> 1)
        elif ft == 4:
            pred = np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, up, upleft)], np.int32)
            f = cur - pred
        else:  # an invalid type: the bytes as they are
            f = cur
        out[y, 0] = ft
        out[y, 1:] = f & 255
    return out.tobytes()


class BitWriter:
    """Deflate's bit order: values LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.bits(int(format(c & ((1 << n) - 1), "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths."""
    codes, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


def _len_sym(length):
    if length == 258:
        return 28
    return max(i for i in range(28) if LEN_BASE[i] <= length)


def _dist_sym(dist):
    return max(i for i in range(30) if DIST_BASE[i] <= dist)


def put_symbols(bw, ops, lit, dist, end=True):
    """ops: ints (literals) and (length, distance) pairs, written with the code maps lit / dist.  A pair given
    as ("sym", litlen symbol[, distance symbol]) writes those symbols raw (for invalid ones)."""
    for op in ops:
        if isinstance(op, int):
            bw.code(*lit[op])
        elif op[0] == "sym":
            bw.code(*lit[op[1]])
            if len(op) > 2:
                bw.code(*dist[op[2]])
        else:
            length, d = op
            ls, ds = _len_sym(length), _dist_sym(d)
            bw.code(*lit[257 + ls])
            bw.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
            bw.code(*dist[ds])
            bw.bits(d - DIST_BASE[ds], DIST_EXTRA[ds])
    if end:
        bw.code(*lit[256])


def fixed_block(bw, ops, final, end=True):
    bw.bits(1 if final else 0, 1)
    bw.bits(1, 2)
    put_symbols(bw, ops, canonical(FIXED_LIT), canonical(FIXED_DIST), end)


def stored_block(bw, data, final):
    bw.bits(1 if final else 0, 1)
    bw.bits(0, 2)
    bw.align()
    bw.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + bytes(data)


def dynamic_block(bw, ops, final, lit_lens, dist_lens, cl_ops, cl_lens, end=True):
    """A dynamic block with explicit code lengths: lit_lens (257..286 entries), dist_lens (1..30), sent as
    cl_ops -- a list of code-length symbols, a repeat symbol as (16 | 17 | 18, extra bits value) -- through the
    code-length code cl_lens (19 lengths by symbol)."""
    bw.bits(1 if final else 0, 1)
    bw.bits(2, 2)
    ncode = max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]) + 1
    ncode = max(ncode, 4)
    bw.bits(len(lit_lens) - 257, 5)
    bw.bits(len(dist_lens) - 1, 5)
    bw.bits(ncode - 4, 4)
    for s in CL_ORDER[:ncode]:
        bw.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for op in cl_ops:
        if isinstance(op, int):
            bw.code(*cl[op])
        else:
            bw.code(*cl[op[0]])
            bw.bits(op[1], {16: 2, 17: 3, 18: 7}[op[0]])
    put_symbols(bw, ops, canonical(lit_lens), canonical(dist_lens), end)


def expand(ops):
    """What a list of literals and (length, distance) pairs inflates to."""
    out = bytearray()
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        else:
            length, d = op
            for _ in range(length):
                out.append(out[-d])
    return bytes(out)


def zwrap(deflate, raw, adler=None):
    """A zlib stream around raw deflate data (32 KiB window, no dictionary) with raw's Adler-32."""
    a = zlib.adler32(raw) & 0xFFFFFFFF if adler is None else adler
    return b"\x78\x01" + deflate + struct.pack(">I", a)


def deflate(raw, form="dynamic", level=6):
    """raw as a zlib stream in the given form: "stored", "fixed" (Z_FIXED), "dynamic", or "blocks" (stored,
    fixed and dynamic blocks in one stream, cut with Z_FULL_FLUSH)."""
    if form == "stored":
        return zlib.compress(raw, 0)
    if form == "fixed":
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        return c.compress(raw) + c.flush()
    if form == "dynamic":
        return zlib.compress(raw, level)
    if form == "blocks":
        cut = [len(raw) // 3, 2 * len(raw) // 3]
        bw = BitWriter()
        stored_block(bw, raw[:cut[0]], False)
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        mid = c.compress(raw[cut[0]:cut[1]]) + c.flush(zlib.Z_FULL_FLUSH)  # ends in an empty stored block, not final
        c = zlib.compressobj(9, zlib.DEFLATED, -15)
        return zwrap(bw.bytes() + mid + c.compress(raw[cut[1]:]) + c.flush(), raw)
    raise ValueError(form)


def png_from_stream(w, h, ctype, depth, stream, palette=None, splits=None, interlace=0):
    """The file around a ready zlib stream.  splits: byte counts of the first IDAT chunks (the rest in a last one)."""
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    if palette is not None:
        out += chunk(b"PLTE", bytes(palette))
    at = 0
    for n in splits or []:
        out += chunk(b"IDAT", stream[at:at + n])
        at += n
    if at < len(stream) or not splits:
        out += chunk(b"IDAT", stream[at:])
    return out + chunk(b"IEND", b"")


def scanlines(arr, ctype, depth, filters=(0,)):
    rows = pack_rows(arr, ctype, depth)
    return filter_rows(rows, max(1, SAMPLES[ctype] * depth // 8), list(filters))


def write(arr, ctype, depth, filters=(0,), form="dynamic", palette=None, splits=None, level=6):
    h, w = np.asarray(arr).shape[:2]
    return png_from_stream(w, h, ctype, depth, deflate(scanlines(arr, ctype, depth, filters), form, level), palette, splits)
