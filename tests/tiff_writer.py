"""A numpy-only TIFF writer for the files Pillow will not produce on request: both byte orders, chosen strip heights,
WhiteIsZero, predictor 2 on 16-bit big-endian samples, LZW streams with a ClearCode in mid-strip, a table filled
past 4,094 entries before a clear, no EOI; PackBits with every control-byte class; hand-assembled stored and
fixed-Huffman Deflate blocks; tag values inline and by offset; the IFD ahead of the data or at the end of the file;
the first strip at any byte alignment.  tests/test_tiff_writer.py holds every file against Pillow's decode of it.

write(samples, ...) takes the samples as the file stores them (before the predictor): HxW or HxWxS, uint8 / uint16.
"""
import struct
import zlib

import numpy as np

COMP = dict(raw=1, lzw=5, deflate=8, adobe=32946, packbits=32773)


# ---- LZW (TIFF flavour: MSB-first codes, the width grows one entry early) ----------------------------------------
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, w):
        self.acc = (self.acc << w) | v
        self.n += w
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 0xFF)
        return bytes(self.out)


def lzw(data, clear_at=(), fill=False, eoi=True, full_codes=60):
    """clear_at: input positions ahead of which a ClearCode goes (mid-strip clears).  fill: no ClearCode at 4,094
    entries; the table fills to 4,096, `full_codes` more codes follow at 12 bits defining nothing, then a clear.
    The writer tracks the reader's width: every code goes out as wide as the reader then expects it."""
    data = bytes(data)
    b = _Bits()
    clear_at = set(clear_at)
    stats = dict(max_entries=258, widths=set(), clears=0, after_full=0)
    table, nxt = {}, 258          # the writer's strings
    dnext, dwidth, dfresh = 258, 9, True  # the reader's state

    def emit(code):
        nonlocal dnext, dwidth, dfresh
        b.put(code, dwidth)
        stats["widths"].add(dwidth)
        if code == 256:
            dnext, dwidth, dfresh = 258, 9, True
            stats["clears"] += 1
            return
        if code == 257:
            return
        if not dfresh and dnext < 4096:
            dnext += 1
            stats["max_entries"] = max(stats["max_entries"], dnext)
            if dnext + 1 >= (1 << dwidth) and dwidth < 12:
                dwidth += 1
        dfresh = False

    emit(256)
    i, n, since_full = 0, len(data), 0
    while i < n:
        if i in clear_at:
            emit(256)
            table, nxt, since_full = {}, 258, 0
        w, j = data[i:i + 1], i + 1
        code = w[0]
        while j < n and j not in clear_at:
            c = table.get(data[i:j + 1])
            if c is None:
                break
            code, j = c, j + 1
        emit(code)
        if j < n:
            if nxt < 4096:
                table[data[i:j + 1]] = nxt
                nxt += 1
            else:
                since_full += 1
                stats["after_full"] += 1
            if (not fill and nxt >= 4094) or (fill and since_full >= full_codes):
                emit(256)
                table, nxt, since_full = {}, 258, 0
        i = j
    if eoi:
        emit(257)
    return b.done(), stats


# ---- PackBits ---------------------------------------------------------------------------------------------------
def packbits(rows, noop_every=0):
    """Each row packed on its own (TIFF 6.0 section 9): repeats of 2..128, literals of 1..128, and a no-op byte
    (0x80) after every noop_every-th packet."""
    out, packets = bytearray(), 0

    def packet(p):
        nonlocal packets
        out.extend(p)
        packets += 1
        if noop_every and packets % noop_every == 0:
            out.append(0x80)

    for row in rows:
        row, i, n = bytes(row), 0, len(row)
        while i < n:
            r = 1
            while i + r < n and r < 128 and row[i + r] == row[i]:
                r += 1
            if r >= 2:
                packet(bytes([257 - r, row[i]]))
                i += r
                continue
            j = i + 1
            while j < n and j - i < 128 and not (j + 1 < n and row[j] == row[j + 1]):
                j += 1
            packet(bytes([j - i - 1]) + row[i:j])
            i = j
    return bytes(out)


# ---- Deflate by hand --------------------------------------------------------------------------------------------
def deflate_stored(data, block=1000, header=b"\x78\x01"):
    data, out = bytes(data), bytearray(header)
    blocks = [data[i:i + block] for i in range(0, len(data), block)] or [b""]
    for k, blk in enumerate(blocks):
        out += bytes([1 if k == len(blocks) - 1 else 0]) + struct.pack("<HH", len(blk), len(blk) ^ 0xFFFF) + blk
    return bytes(out) + struct.pack(">I", zlib.adler32(data))


class _LsbBits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, w):  # w bits of v, least significant first
        self.acc |= v << self.n
        self.n += w
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, w):  # a Huffman code: most significant bit first
        self.put(int(format(code, "0%db" % w)[::-1], 2), w)

    def done(self):
        if self.n:
            self.out.append(self.acc & 0xFF)
        return bytes(self.out)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]


def deflate_fixed(data):
    """One fixed-Huffman block: literals, and a run of a byte as a match at distance 1 (lengths 3..258)."""
    data, b = bytes(data), _LsbBits()
    b.put(1, 1), b.put(1, 2)

    def sym(v):
        if v < 144:
            b.huff(0x30 + v, 8)
        elif v < 256:
            b.huff(0x190 + v - 144, 9)
        elif v < 280:
            b.huff(v - 256, 7)
        else:
            b.huff(0xC0 + v - 280, 8)

    i, n = 0, len(data)
    while i < n:
        sym(data[i])
        r = 0
        while i + 1 + r < n and r < 258 and data[i + 1 + r] == data[i]:
            r += 1
        if r >= 3:
            k = max(s for s in range(29) if _LEN_BASE[s] <= r)
            r = min(r, _LEN_BASE[k] + (1 << _LEN_EXTRA[k]) - 1)
            sym(257 + k)
            b.put(r - _LEN_BASE[k], _LEN_EXTRA[k])
            b.huff(0, 5)  # distance code 0: distance 1
            i += r
        i += 1
    sym(256)
    return b"\x78\x01" + b.done() + struct.pack(">I", zlib.adler32(data))


# ---- the file ---------------------------------------------------------------------------------------------------
def write(samples, photo, comp="raw", big=False, pred=1, rps=None, extra=None, colormap=None, pad=0, ifd_first=False,
          bytecounts=True, codec=None, tail=b"", more_tags=(), planar=None, fillorder=None, sampleformat=None, version=42):
    """samples: HxW or HxWxS uint8 / uint16 as stored; photo: PhotometricInterpretation; comp: a COMP key or a number;
    rps: RowsPerStrip (None: the tag is absent, one strip); extra: the ExtraSamples value (None: absent);
    colormap: 256x3 uint16; pad: bytes between the header and the first strip (its alignment); codec: a function
    strip bytes -> compressed bytes that replaces comp's own; tail: bytes appended to every strip's decoded data
    before it is compressed (a strip that decodes to more than its rows); more_tags: (tag, type, values) to add."""
    a = np.asarray(samples)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, spp = a.shape
    bps = 16 if a.dtype == np.uint16 else 8
    a = a.astype(np.uint16 if bps == 16 else np.uint8)
    if pred == 2:
        d = a.astype(np.int64)
        d[:, 1:] -= a[:, :-1].astype(np.int64)
        a = (d % (1 << bps)).astype(a.dtype)
    if bps == 16:
        a = a.astype(">u2" if big else "<u2")
    E = ">" if big else "<"
    n_rps = h if rps is None else rps
    strips = []
    for y0 in range(0, h, n_rps):
        rows = a[y0:y0 + n_rps]
        raw = rows.tobytes() + tail
        if codec is not None:
            strips.append(codec(raw))
        elif comp == "raw":
            strips.append(raw)
        elif comp == "lzw":
            strips.append(lzw(raw)[0])
        elif comp == "packbits":
            strips.append(packbits([r.tobytes() for r in rows] + ([tail] if tail else [])))
        else:
            strips.append(zlib.compress(raw, 6))
    offs = []
    tags = {256: (4, [w]), 257: (4, [h]), 258: (3, [bps] * spp), 259: (3, [COMP.get(comp, comp)]), 262: (3, [photo]),
            277: (3, [spp])}
    if rps is not None:
        tags[278] = (4 if rps > 65535 else 3, [rps])
    if pred != 1:
        tags[317] = (3, [pred])
    if extra is not None:
        tags[338] = (3, [extra])
    if colormap is not None:
        tags[320] = (3, [int(v) for v in np.asarray(colormap).T.reshape(-1)])
    if planar is not None:
        tags[284] = (3, [planar])
    if fillorder is not None:
        tags[266] = (3, [fillorder])
    if sampleformat is not None:
        tags[339] = (3, [sampleformat] * spp)
    tags[273] = (4, [0] * len(strips))
    if bytecounts:
        tags[279] = (4, [len(s) for s in strips])
    for t, ty, v in more_tags:
        tags[t] = (ty, list(v))
    size = {1: 1, 3: 2, 4: 4}
    fmt = {1: "B", 3: "H", 4: "I"}
    ifd_len = 2 + 12 * len(tags) + 4
    ool = {t: len(v) * size[ty] for t, (ty, v) in tags.items() if len(v) * size[ty] > 4}
    # layout: header, [IFD, out-of-line values,] pad, strips, [out-of-line values, IFD]
    pos = 8
    if ifd_first:
        ifd_at, pos = pos, pos + ifd_len
        ool_at = {}
        for t, nb in ool.items():
            ool_at[t], pos = pos, pos + nb + (nb & 1)
    pos += pad
    for s in strips:
        offs.append(pos)
        pos += len(s)
    if not ifd_first:
        pos += pos & 1
        ool_at = {}
        for t, nb in ool.items():
            ool_at[t], pos = pos, pos + nb + (nb & 1)
        ifd_at = pos
    tags[273] = (4, offs)
    ifd = struct.pack(E + "H", len(tags))
    blobs = {}
    for t in sorted(tags):
        ty, v = tags[t]
        data = struct.pack(E + fmt[ty] * len(v), *v)
        if len(data) > 4:
            blobs[t] = data
            ifd += struct.pack(E + "HHII", t, ty, len(v), ool_at[t])
        else:
            ifd += struct.pack(E + "HHI", t, ty, len(v)) + data.ljust(4, b"\0")
    ifd += struct.pack(E + "I", 0)
    ool_bytes = b"".join(blobs[t] + b"\0" * (len(blobs[t]) & 1) for t in ool)
    head = (b"MM" if big else b"II") + struct.pack(E + "HI", version, ifd_at)
    sdata = b"".join(strips)
    if ifd_first:
        return head + ifd + ool_bytes + b"\0" * pad + sdata
    return head + b"\0" * pad + sdata + b"\0" * ((8 + pad + len(sdata)) & 1) + ool_bytes + ifd  # the IFD ends the file
