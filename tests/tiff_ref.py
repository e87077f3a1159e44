"""The TIFF decode rules restated in numpy: decode(file, mode) is what aeon_decode_tiff must give
for a file it accepts.  A reader of its own: the first IFD, strips, the four compressions (LZW and PackBits in plain
Python, Deflate by zlib), byte order, predictor 2, then the conversions.  It refuses nothing gracefully: it is for
files the library accepts.
"""
import struct
import zlib

import numpy as np

BGR8, GRAY8, ANYDEPTH = 0, 1, 2


def gray_of(b, g, r):
    """The project's colour -> gray formula."""
    return ((b.astype(np.uint32) * 1868 + g.astype(np.uint32) * 9617 + r.astype(np.uint32) * 4899 + 8192) >> 14).astype(np.uint8)


def _lzw(data, need):
    out, bit, width, table, prev = bytearray(), 0, 9, None, None
    total = 8 * len(data)
    val = int.from_bytes(data, "big")
    while len(out) < need:
        assert bit + width <= total, "LZW data ends early"
        code = (val >> (total - bit - width)) & ((1 << width) - 1)
        bit += width
        if code == 256:
            table, width, prev = [bytes([i]) for i in range(256)] + [b"", b""], 9, None
            continue
        if code == 257:
            break
        if prev is None:
            s = table[code]
        else:
            s = table[code] if code < len(table) else prev + prev[:1]
            assert code <= len(table)
            if len(table) < 4096:
                table.append(prev + s[:1])
                if len(table) + 1 >= (1 << width) and width < 12:
                    width += 1
        out += s
        prev = s
    assert len(out) >= need
    return bytes(out[:need])


def _packbits(data, need):
    out, i = bytearray(), 0
    while len(out) < need:
        c = data[i]
        i += 1
        if c == 128:
            continue
        if c < 128:
            out += data[i:i + c + 1]
            i += c + 1
        else:
            out += data[i:i + 1] * (257 - c)
            i += 1
    assert len(out) == need
    return bytes(out)


def parse(f):
    E = "<" if f[:2] == b"II" else ">"
    (ifd,) = struct.unpack_from(E + "I", f, 4)
    (n,) = struct.unpack_from(E + "H", f, ifd)
    tags = {}
    for k in range(n):
        t, ty, cnt = struct.unpack_from(E + "HHI", f, ifd + 2 + 12 * k)
        sz, ch = {1: (1, "B"), 3: (2, "H"), 4: (4, "I")}.get(ty, (0, None))
        if ch is None:
            continue
        at = ifd + 2 + 12 * k + 8
        if sz * cnt > 4:
            (at,) = struct.unpack_from(E + "I", f, at)
        tags[t] = list(struct.unpack_from(E + ch * cnt, f, at))
    return E, tags


def samples(f):
    """The file's samples as stored values, native, predictor undone: HxWxS."""
    E, T = parse(f)
    w, h, bps = T[256][0], T[257][0], T[258][0]
    spp, comp, pred = T.get(277, [1])[0], T.get(259, [1])[0], T.get(317, [1])[0]
    rps = min(T.get(278, [h])[0], h)
    rowb = w * spp * bps // 8
    rows = []
    for s, y0 in enumerate(range(0, h, rps)):
        need = min(rps, h - y0) * rowb
        off = T[273][s]
        d = f[off:off + (T[279][s] if 279 in T else need)]
        if comp == 5:
            d = _lzw(d, need)
        elif comp == 32773:
            d = _packbits(d, need)
        elif comp in (8, 32946):
            d = zlib.decompressobj().decompress(d, need)
        rows.append(d[:need])
    a = np.frombuffer(b"".join(rows), np.uint8 if bps == 8 else np.dtype(E + "u2")).reshape(h, w, spp)
    a = a.astype(np.uint16 if bps == 16 else np.uint8)
    if pred == 2 and comp in (5, 8, 32946):  # (libtiff knows Predictor under LZW and Deflate only)
        a = np.cumsum(a.astype(np.uint64), axis=1).astype(a.dtype)  # mod 2^8 / 2^16 per sample, stride SamplesPerPixel
    return a, T


def decode(f, mode):
    a, T = samples(f)
    photo, wide = T[262][0], a.dtype == np.uint16
    if photo == 3:
        cm = (np.array(T[320], np.uint32).reshape(3, 256) >> 8).astype(np.uint8)  # entry >> 8
        r, g, b = (cm[c][a[:, :, 0]] for c in range(3))
        return np.dstack([b, g, r]) if mode == BGR8 else gray_of(b, g, r)
    if photo <= 1:
        v = a[:, :, 0]  # an extra sample is dropped
        if photo == 0:
            v = (65535 if wide else 255) - v
        if mode == ANYDEPTH and wide:
            return v.astype(np.uint16)
        v8 = (v >> 8).astype(np.uint8) if wide else v
        return np.dstack([v8, v8, v8]) if mode == BGR8 else v8
    c = (a[:, :, :3] >> 8).astype(np.uint8) if wide else a[:, :, :3]
    r, g, b = c[:, :, 0], c[:, :, 1], c[:, :, 2]
    return np.dstack([b, g, r]) if mode == BGR8 else gray_of(b, g, r)
