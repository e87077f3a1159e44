"""The PNG stage's test files, made once with tests/png_writer.py and shared by tests/test_png_stage.py (CPU: the
kernels' code run on the host, and the routing of every file the GPU tests use) and tests/test_hip_png.py (GPU).
Each list holds (name, png bytes); helper, no test of its own.
"""
import functools
import struct
import zlib

import numpy as np

from tests import png_writer as W

# (name, colour type, depth): the filters' byte distance 1, 2, 3, 4, 6 and 8, and the sub-byte depths
FORMATS = [("gray8", 0, 8), ("gray16", 0, 16), ("la8", 4, 8), ("rgb8", 2, 8), ("rgba8", 6, 8), ("la16", 4, 16),
           ("rgb16", 2, 16), ("rgba16", 6, 16), ("gray1", 0, 1), ("gray2", 0, 2), ("gray4", 0, 4), ("pal1", 3, 1),
           ("pal2", 3, 2), ("pal4", 3, 4), ("pal8", 3, 8)]
FILTERS = [("f0", (0,)), ("f1", (1,)), ("f2", (2,)), ("f3", (3,)), ("f4", (4,)), ("cycle", (0, 1, 2, 3, 4))]


def _samples(rng, w, h, ctype, depth):
    n = W.SAMPLES[ctype]
    a = rng.integers(0, 1 << depth, (h, w, n) if n > 1 else (h, w))
    # smooth in places, so that the filters see equal neighbours as well as noise
    a[h // 2:, : max(1, w // 2)] = a[h // 2, 0]
    return a


def _palette(rng, depth):
    return rng.integers(0, 256, 3 << depth).astype(np.uint8).tobytes()


def _one(rng, ctype, depth, w, h, filters, form="dynamic", **kw):
    pal = _palette(rng, depth) if ctype == 3 else None
    return W.write(_samples(rng, w, h, ctype, depth), ctype, depth, filters, form, pal, **kw)


@functools.lru_cache(None)
def filter_files():
    """Every format x every filter type alone and all five cycling, 13 x 9; a 1-pixel-wide and a 1-pixel-high
    image per format."""
    rng = np.random.default_rng(31)
    out = []
    for fname, ctype, depth in FORMATS:
        for gname, filters in FILTERS:
            out.append((f"{fname}_{gname}", _one(rng, ctype, depth, 13, 9, filters)))
        out.append((f"{fname}_w1", _one(rng, ctype, depth, 1, 7, (0, 1, 2, 3, 4))))
        out.append((f"{fname}_h1", _one(rng, ctype, depth, 11, 1, (4,))))
    return out


@functools.lru_cache(None)
def band_files():
    """130 rows (two full bands of the unfilter kernel and a 2-row tail), all Paeth and all Average, at widths
    around the wave's 64 lanes."""
    rng = np.random.default_rng(32)
    out = []
    for w in (1, 2, 63, 64, 65):
        out.append((f"paeth130_w{w}", _one(rng, 2, 8, w, 130, (4,))))
        out.append((f"avg130_w{w}", _one(rng, 2, 8, w, 130, (3,))))
    return out


def _lits(rng, n):
    return [int(v) for v in rng.integers(0, 5, n)]  # every byte a valid filter type, wherever a row starts


def _gray(w, h, stream, **kw):
    return W.png_from_stream(w, h, 0, 8, stream, **kw)


LIT8 = [3] * 5 + [0] * 251 + [3, 3, 3]  # literals 0..4, end of block, lengths 3 and 4: eight codes of 3 bits
CL = {0: 2, 3: 2, 16: 2, 17: 3, 18: 3}


def _cl_lens(d):
    return [d.get(s, 0) for s in range(19)]


def _repeat_blocks(rng):
    """Three dynamic blocks whose code lengths run across the literal/distance boundary with repeat codes 16
    (a run of 3s), 17 and 18 (runs of zeros)."""
    head = [3, (16, 1), (18, 127), (18, 102)]  # 5 threes, 251 zeros
    bw, ops_all = W.BitWriter(), []
    # A: 256..258 = 3 and eight distance codes of 3 bits: 11 threes as 3, 16 x6, 16 x4
    ops = _lits(rng, 29) + [(3, 1), (4, 2), (3, 4)] + _lits(rng, 9)
    W.dynamic_block(bw, ops, False, LIT8, [3] * 8, head + [3, (16, 3), (16, 1)], _cl_lens(CL))
    ops_all += ops
    # B: three zeros behind 258 and three ahead of the distance codes 3..10: 17 x6
    ops = _lits(rng, 12) + [(3, 4), (4, 5), (3, 8)] + _lits(rng, 5)
    W.dynamic_block(bw, ops, False, LIT8 + [0] * 3, [0] * 3 + [3] * 8, head + [3, 3, 3, (17, 3), 3, (16, 3), 3],
                    _cl_lens(CL))
    ops_all += ops
    # C: eleven zeros behind 258 and five ahead of the distance codes 5..12: 18 x16
    ops = _lits(rng, 7) + [(4, 7), (3, 9), (4, 12)] + _lits(rng, 3)
    W.dynamic_block(bw, ops, True, LIT8 + [0] * 11, [0] * 5 + [3] * 8, head + [3, 3, 3, (18, 5), 3, (16, 3), 3],
                    _cl_lens(CL))
    ops_all += ops
    return bw.bytes(), ops_all


@functools.lru_cache(None)
def inflate_files():
    """(name, png, zlib stream, expected inflated bytes): the deflate forms and hand-built edges."""
    rng = np.random.default_rng(33)
    out = []

    def add(name, w, h, ctype, stream, raw):
        assert len(raw) == (W.row_bytes(w, ctype, 8) + 1) * h, (name, len(raw))
        out.append((name, W.png_from_stream(w, h, ctype, 8, stream), stream, raw))

    big = bytes(_lits(rng, 901 * 80))  # 300 x 80 RGB: 72,080 bytes, the ring wraps twice
    bw = W.BitWriter()
    W.stored_block(bw, b"", False)
    W.stored_block(bw, big[:65535], False)
    W.stored_block(bw, big[65535:], True)
    add("stored", 300, 80, 2, W.zwrap(bw.bytes(), big), big)
    small = W.scanlines(_samples(rng, 40, 30, 0, 8), 0, 8, (0, 1, 2, 3, 4))
    add("fixed", 40, 30, 0, W.deflate(small, "fixed"), small)
    smooth = W.scanlines((np.add.outer(np.arange(80), np.arange(96)) // 7 % 256), 0, 8, (1, 4))
    add("dynamic", 96, 80, 0, W.deflate(smooth, "dynamic"), smooth)
    add("blocks", 96, 80, 0, W.deflate(smooth, "blocks"), smooth)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(smooth) + c.flush(zlib.Z_FULL_FLUSH)
    bw = W.BitWriter()
    W.fixed_block(bw, [], True)
    add("empty_final", 96, 80, 0, W.zwrap(body + bw.bytes(), smooth), smooth)
    # matches by hand: 41 x 20 gray = 840 bytes
    ops = _lits(rng, 2) + [(3, 1)] + _lits(rng, 1) + [(258, 1)] + _lits(rng, 2) + [(7, 2)] + _lits(rng, 70)
    ops += [(80, 63), (80, 64), (80, 65), (5, 63), (5, 64), (5, 65)]
    ops += _lits(rng, 840 - len(W.expand(ops)))
    bw = W.BitWriter()
    W.fixed_block(bw, ops, True)
    raw = W.expand(ops)
    add("matches", 41, 20, 0, W.zwrap(bw.bytes(), raw), raw)
    # distance 32,768: the window's first byte, then again after the ring has wrapped twice
    ops = _lits(rng, 32768) + [(258, 32768)] + _lits(rng, 33000) + [(200, 32768), (258, 32767), (3, 32768)]
    ops += _lits(rng, 901 * 80 - len(W.expand(ops)))
    bw = W.BitWriter()
    W.fixed_block(bw, ops, True)
    raw = W.expand(ops)
    add("far", 300, 80, 2, W.zwrap(bw.bytes(), raw), raw)
    body, ops = _repeat_blocks(rng)
    raw = W.expand(ops)
    add("repeats", len(raw) - 1, 1, 0, W.zwrap(body, raw), raw)
    # one distance code of one bit (an incomplete set zlib accepts)
    ops = _lits(rng, 30) + [(3, 1), (4, 1)] + _lits(rng, 8)
    bw = W.BitWriter()
    W.dynamic_block(bw, ops, True, LIT8, [1], [3, (16, 1), (18, 127), (18, 102), 3, 3, 3, 1],
                    _cl_lens({0: 2, 1: 2, 3: 2, 16: 3, 18: 3}))
    raw = W.expand(ops)
    add("one_dist", 8, 5, 0, W.zwrap(bw.bytes(), raw), raw)
    return out


@functools.lru_cache(None)
def corrupt_files():
    """Files whose chunks are in order and whose image data the device must refuse."""
    rng = np.random.default_rng(34)
    out = []
    img = _samples(rng, 24, 16, 0, 8)
    raw = W.scanlines(img, 0, 8, (0, 1, 2, 3, 4))
    good = W.deflate(raw, "dynamic")
    out.append(("adler", _gray(24, 16, good[:-1] + bytes([good[-1] ^ 0xFF]))))
    bw = W.BitWriter()
    W.fixed_block(bw, [0, 1, (3, 5)] + _lits(rng, 20), True)
    out.append(("distance", _gray(24, 1, W.zwrap(bw.bytes(), b"", 1))))
    bw = W.BitWriter()
    W.fixed_block(bw, [0, 1, 2, ("sym", 286)] + _lits(rng, 22), True)
    out.append(("length_symbol", _gray(24, 1, W.zwrap(bw.bytes(), b"", 1))))
    bw = W.BitWriter()
    W.dynamic_block(bw, _lits(rng, 25), True, LIT8 + [3], [3] * 8, [3, (16, 1), (18, 127), (18, 102), 3, (16, 3), (16, 2)],
                    _cl_lens(CL))
    out.append(("oversubscribed", _gray(24, 1, W.zwrap(bw.bytes(), b"", 1))))
    noisy = W.deflate(W.scanlines(rng.integers(0, 256, (16, 24)), 0, 8), "dynamic")
    out.append(("truncated", _gray(24, 16, noisy[: len(noisy) * 3 // 5])))
    out.append(("too_long", _gray(24, 16, W.deflate(raw + bytes(10), "dynamic"))))
    out.append(("filter5", _gray(24, 16, W.deflate(W.scanlines(img, 0, 8, (0, 5)), "dynamic"))))
    idx = rng.integers(0, 4, (16, 24))
    idx[9, 7] = 9
    out.append(("palette_index", W.write(idx, 3, 8, (0,), "dynamic", bytes(range(12)))))
    return out


@functools.lru_cache(None)
def split_files():
    """IDAT split at 1-byte chunks, inside the zlib header and inside the Adler trailer."""
    rng = np.random.default_rng(35)
    img = _samples(rng, 20, 12, 2, 8)
    stream = W.deflate(W.scanlines(img, 2, 8, (4,)), "dynamic")
    n = len(stream)
    return [("split_header", W.png_from_stream(20, 12, 2, 8, stream, splits=[1])),
            ("split_ones", W.png_from_stream(20, 12, 2, 8, stream, splits=[1, 1, 1, 1, 1, 0, 3])),
            ("split_adler", W.png_from_stream(20, 12, 2, 8, stream, splits=[n - 2])),
            ("split_adler_ones", W.png_from_stream(20, 12, 2, 8, stream, splits=[n - 4, 1, 1, 1]))]
