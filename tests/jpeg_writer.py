"""A small sequential-JPEG writer for tests, written from ITU T.81 with numpy only.

It writes a Huffman-coded sequential file (SOF0 baseline or SOF1 extended, 8-bit samples, one scan)
from already-quantised coefficients, so a test controls everything an encoder normally decides: the
frame size, each component's id, sampling factors and table selectors, the quantisation tables (8- or
16-bit entries), the Huffman tables (Annex K, explicit counts / symbols, or built from symbol
statistics by the procedure of T.81 K.2, limited to 16-bit codes), the restart interval, fill bytes
before markers, extra APPn / COM segments and the order of the table segments around the frame header.

Coefficients are per component int16[blocks_y][blocks_x][64] in natural (row-major 8x8) order, padding
blocks included: blocks_x = mcus_x * h and blocks_y = mcus_y * v, with the MCU grid of the frame
(T.81 A.2.4).  A single-component scan is non-interleaved (A.2.2): it codes only the
ceil(width / 8) x ceil(height / 8) blocks of the component, whatever its sampling factors say.

The writer is deterministic, and it asserts what would make the file invalid: a coefficient too large
for its category, more than 10 blocks per MCU, a Huffman table without the symbol a block needs, a
table whose codes do not fit 16 bits, baseline files using what only extended files may.
"""
import numpy as np

# zigzag position -> natural index (T.81 figure A.6)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                   38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# T.81 Annex K.1: the example quantisation tables (natural order)
K1_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
K1_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                      47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def _hex(s):
    return [int(x, 16) for x in s.split()]


# T.81 Annex K.3: the example Huffman tables as (counts of the code lengths 1..16, symbols)
_AC_LUMA = _hex(
    "01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72 "
    "82 09 0a 16 17 18 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 "
    "5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 "
    "a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 "
    "e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 f8 f9 fa")
_AC_CHROMA = _hex(
    "00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 62 72 d1 "
    "0a 16 24 34 e1 25 f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 "
    "59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a "
    "a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da "
    "e2 e3 e4 e5 e6 e7 e8 e9 ea f2 f3 f4 f5 f6 f7 f8 f9 fa")
K3_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
K3_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
K3_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], _AC_LUMA)
K3_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], _AC_CHROMA)


def scaled_qtable(base, quality):
    """An Annex K.1 table scaled the way encoders commonly map a 1..100 quality to it."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.asarray(base, np.int64) * s + 50) // 100, 1, 255)


def huffman_codes(counts, symbols):
    """{symbol: (code, length)} of a table (T.81 C.2); asserts the table is one a decoder accepts."""
    counts, symbols = list(counts), list(symbols)
    assert len(counts) == 16 and sum(counts) == len(symbols) and 1 <= len(symbols) <= 256
    assert len(set(symbols)) == len(symbols) and all(0 <= s <= 255 for s in symbols)
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[symbols[k]] = (code, length)
            code, k = code + 1, k + 1
        # the all-ones code of a length stays free (T.81 C.2: the codes are a prefix of it)
        assert code < (1 << length), "Huffman table overflows its code space"
        code <<= 1
    return codes


def huffman_from_lengths(lengths):
    """(counts, symbols) from {symbol: code length}: symbols of a length in ascending order."""
    counts = [0] * 16
    for n in lengths.values():
        assert 1 <= n <= 16
        counts[n - 1] += 1
    symbols = [s for n in range(1, 17) for s in sorted(k for k, v in lengths.items() if v == n)]
    huffman_codes(counts, symbols)
    return counts, symbols


def huffman_from_stats(freq):
    """(counts, symbols) from {symbol: frequency > 0} by T.81 K.2 (figures K.1 - K.4): code sizes from
    pairwise merging with a reserved 257th symbol (so no code is all ones), lengths above 16 folded
    back by Adjust_BITS, symbols sorted by code length then value."""
    f = [0] * 257
    for s, n in freq.items():
        assert 0 <= s <= 255 and n > 0
        f[s] = int(n)
    f[256] = 1
    size, other = [0] * 257, [-1] * 257
    while True:
        live = [i for i in range(257) if f[i] > 0]
        if len(live) < 2:
            break
        v1 = min(live, key=lambda i: (f[i], -i))          # least frequency, the larger index on ties
        v2 = min((i for i in live if i != v1), key=lambda i: (f[i], -i))
        f[v1] += f[v2]
        f[v2] = 0
        size[v1] += 1
        while other[v1] >= 0:
            v1 = other[v1]
            size[v1] += 1
        other[v1] = v2                                     # v2's chain goes behind v1's
        size[v2] += 1
        while other[v2] >= 0:
            v2 = other[v2]
            size[v2] += 1
    bits = [0] * 64
    for i in range(257):
        if size[i]:
            assert size[i] < 64
            bits[size[i]] += 1
    i = 63
    while i > 16:                                          # figure K.3: Adjust_BITS
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                           # the reserved symbol's code
    counts = bits[1:17]
    symbols = [s for n in range(1, 64) for s in range(256) if size[s] == n]
    assert sum(counts) == len(symbols)
    huffman_codes(counts, symbols)
    return counts, symbols


class Component:
    def __init__(self, id, h=1, v=1, tq=0, td=0, ta=0):
        self.id, self.h, self.v, self.tq, self.td, self.ta = id, h, v, tq, td, ta


def grid(width, height, comps):
    """(mcus_x, mcus_y) of the frame and per component (blocks_x, blocks_y) with padding."""
    hmax, vmax = max(c.h for c in comps), max(c.v for c in comps)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    return mx, my, [(mx * c.h, my * c.v) for c in comps]


def category(v):
    """SSSS of a value (T.81 tables F.1 / F.2): the bits of its magnitude."""
    return int(abs(int(v))).bit_length()


def block_symbols(zz, pred):
    """The (class, symbol, value bits, size) sequence of one block (T.81 F.1.2): zz its 64 coefficients
    in zigzag order, pred the DC prediction."""
    out = []
    d = int(zz[0]) - pred
    s = category(d)
    assert s <= 11, f"DC difference {d} is too large for category 11"
    out.append((0, s, d if d >= 0 else d + (1 << s) - 1, s))
    run = 0
    nz = np.flatnonzero(zz[1:]) + 1
    last = int(nz[-1]) if len(nz) else 0
    for k in range(1, last + 1):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        s = category(v)
        assert s <= 10, f"AC coefficient {v} is too large for category 10"
        out.append((1, run << 4 | s, v if v >= 0 else v + (1 << s) - 1, s))
        run = 0
    if last < 63:
        out.append((1, 0x00, 0, 0))
    return out


def scan_units(width, height, comps):
    """The scan's coding units, each a list of (component, block row, block column): the MCUs of an
    interleaved scan, single blocks of a one-component scan (T.81 A.2)."""
    mx, my, _ = grid(width, height, comps)
    if len(comps) > 1:
        return [[(k, ymcu * c.v + y, xmcu * c.h + x) for k, c in enumerate(comps) for y in range(c.v) for x in range(c.h)]
                for ymcu in range(my) for xmcu in range(mx)]
    return [[(0, y, x)] for y in range(-(-height // 8)) for x in range(-(-width // 8))]


def scan_statistics(width, height, comps, coefs, restart=0):
    """({DC table id: {symbol: count}}, {AC table id: {symbol: count}}) of the scan write_jpeg would
    code: the input of huffman_from_stats."""
    dc, ac = {}, {}
    pred = [0] * len(comps)
    for u, unit in enumerate(scan_units(width, height, comps)):
        if restart and u and u % restart == 0:
            pred = [0] * len(comps)
        for k, y, x in unit:
            zz = coefs[k][y, x][ZIGZAG]
            for cls, sym, _, _ in block_symbols(zz, pred[k]):
                t = (ac if cls else dc).setdefault(comps[k].ta if cls else comps[k].td, {})
                t[sym] = t.get(sym, 0) + 1
            pred[k] = int(zz[0])
    return dc, ac



class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.stuffed = bytearray(), 0, 0, 0

    def put(self, value, nbits):
        self.acc = self.acc << nbits | value
        self.n += nbits
        while self.n >= 8:
            self.n -= 8
            b = self.acc >> self.n & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
                self.stuffed += 1
        self.acc &= (1 << self.n) - 1

    def flush(self):
        """Pad the last byte with 1-bits (T.81 F.1.2.3)."""
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _segment(marker, payload, fill=0):
    assert len(payload) + 2 <= 0xFFFF
    return b"\xff" * (fill + 1) + bytes([marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def write_jpeg(width, height, comps, coefs, qtables, dc_tables, ac_tables, *, sof=0xC0, restart=0,
               layout=("DQT", "SOF", "DHT", "DRI"), dht_split=False, jfif=True, adobe=None,
               fill_header=0, fill_rst=0, fill_eoi=0, trace=None):
    """The file's bytes.

    comps       list of Component (1, 3 or 4 of them), in frame and scan order
    coefs       per component int16[blocks_y][blocks_x][64], natural order (see grid())
    qtables     {id: 64 entries in natural order}; a table with an entry above 255 is written 16-bit
    dc_tables   {id: (counts, symbols)}, ac_tables likewise
    sof         0xC0 (baseline) or 0xC1 (extended sequential)
    restart     the restart interval in MCUs (0: none)
    layout      the segments between the APP0 / APP14 markers and SOS, in order: "DQT", "SOF", "DHT", "DRI"
                (each once; "DRI" is skipped when restart is 0) and any (marker, payload) extras
    dht_split   each Huffman table in a DHT segment of its own
    jfif        write a JFIF APP0 segment; adobe: the transform byte of an Adobe APP14 segment, or None
    fill_*      extra FF bytes before the header markers, each RSTn and EOI
    trace       a list that receives (class, symbol, code length, size) of every coded symbol, and
                ("rst", bytes so far) at each restart marker
    """
    assert sof in (0xC0, 0xC1) and 1 <= width <= 0xFFFF and 1 <= height <= 0xFFFF and 0 <= restart <= 0xFFFF
    assert len(comps) in (1, 3, 4) and len(coefs) == len(comps)
    assert sorted(x for x in layout if isinstance(x, str)) == ["DHT", "DQT", "DRI", "SOF"]
    mx, my, blocks = grid(width, height, comps)
    inter = len(comps) > 1
    for c, cf, (bx, by) in zip(comps, coefs, blocks):
        assert 1 <= c.h <= 4 and 1 <= c.v <= 4 and 0 <= c.id <= 255
        assert cf.shape == (by, bx, 64) and cf.dtype == np.int16, (cf.shape, (by, bx, 64))
        assert c.tq in qtables and c.td in dc_tables and c.ta in ac_tables
        if sof == 0xC0:
            assert c.td < 2 and c.ta < 2 and max(qtables[c.tq]) <= 255, "baseline: tables 0-1, 8-bit entries"
    if inter:
        assert sum(c.h * c.v for c in comps) <= 10, "more than 10 blocks per MCU"
    dcc = {i: huffman_codes(*t) for i, t in dc_tables.items()}
    acc = {i: huffman_codes(*t) for i, t in ac_tables.items()}

    def seg_dqt():
        p = bytearray()
        for i in sorted(qtables):
            q = np.asarray(qtables[i]).reshape(64)
            assert 0 <= i <= 3 and q.min() >= 1 and q.max() <= 0xFFFF
            wide = int(q.max() > 255)
            p.append(wide << 4 | i)
            for z in range(64):
                p += int(q[ZIGZAG[z]]).to_bytes(2 if wide else 1, "big")
        return _segment(0xDB, p, fill_header)

    def seg_sof():
        p = bytearray([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([len(comps)])
        for c in comps:
            p += bytes([c.id, c.h << 4 | c.v, c.tq])
        return _segment(sof, p, fill_header)

    def seg_dht():
        tabs = [(0 << 4 | i, dc_tables[i]) for i in sorted(dc_tables)] + [(1 << 4 | i, ac_tables[i]) for i in sorted(ac_tables)]
        parts = []
        for tc_th, (counts, symbols) in tabs:
            assert 0 <= (tc_th & 15) <= 3
            parts.append(bytes([tc_th]) + bytes(counts) + bytes(symbols))
        if dht_split:
            return b"".join(_segment(0xC4, p, fill_header) for p in parts)
        return _segment(0xC4, b"".join(parts), fill_header)

    out = bytearray(b"\xff\xd8")
    if jfif:
        out += _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00", fill_header)
    if adobe is not None:
        out += _segment(0xEE, b"Adobe\0\x64\x00\x00\x00\x00" + bytes([adobe]), fill_header)
    for item in layout:
        if item == "DQT":
            out += seg_dqt()
        elif item == "SOF":
            out += seg_sof()
        elif item == "DHT":
            out += seg_dht()
        elif item == "DRI":
            if restart:
                out += _segment(0xDD, restart.to_bytes(2, "big"), fill_header)
        else:
            marker, payload = item
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE
            out += _segment(marker, payload, fill_header)
    p = bytearray([len(comps)])
    for c in comps:
        p += bytes([c.id, c.td << 4 | c.ta])
    out += _segment(0xDA, p + bytes([0, 63, 0]), fill_header)

    units = scan_units(width, height, comps)
    bits, pred, nrst = _Bits(), [0] * len(comps), 0
    for u, unit in enumerate(units):
        if restart and u and u % restart == 0:
            bits.flush()
            out += bits.out
            if trace is not None:
                trace.append(("rst", bytes(bits.out)))
            out += b"\xff" * (fill_rst + 1) + bytes([0xD0 + (nrst & 7)])
            bits, pred, nrst = _Bits(), [0] * len(comps), nrst + 1
        for k, y, x in unit:
            zz = coefs[k][y, x][ZIGZAG]
            for cls, sym, val, size in block_symbols(zz, pred[k]):
                table = acc[comps[k].ta] if cls else dcc[comps[k].td]
                assert sym in table, f"{'AC' if cls else 'DC'} table {comps[k].ta if cls else comps[k].td} has no symbol {sym:#04x}"
                code, length = table[sym]
                bits.put(code, length)
                if size:
                    bits.put(val, size)
                if trace is not None:
                    trace.append((cls, sym, length, size))
            pred[k] = int(zz[0])
    bits.flush()
    out += bits.out
    if trace is not None:
        trace.append(("end", bytes(bits.out)))
    out += b"\xff" * (fill_eoi + 1) + b"\xd9"
    return bytes(out)
