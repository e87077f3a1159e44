"""Generate the committed fixtures of the JPEG layouts and streams Pillow's encoder cannot produce.

Run by hand where Pillow is installed (Pillow 12.2 / libjpeg-turbo); the output is committed.  Every
file is built by tests/jpeg_writer.py from seeded coefficients -- files() needs numpy only, and the CPU
tests call it to pin the writer -- and decoded by Pillow exactly as make_jpeg_fixtures.py decodes:
convert("RGB") reversed to BGR, draft("L") for gray; the four-component file through
tests/jpeg_cmyk_ref.py as make_jpeg_cmyk_fixtures.py does.

jpeg_layout_fixtures.npz, per fixture <name>:
  <name>.jpg    the file's bytes (uint8)
  <name>.bgr    the whole HWC BGR record
  <name>.gray   the whole grayscale record
and `refused`, the names (their .jpg only) of the files Pillow refuses to decode: the product and the
oracle must refuse them too.

Coefficients are sparse random blocks.  Each block is checked with a float64 inverse DCT: every sample
(level shift included) lies in [-256, 511], where libjpeg's range-limit table clamps; outside it the
table wraps and the C and SIMD IDCTs disagree.  A block outside the range is drawn again (blocks with
fixed content assert the range instead).  Samples below 0 and above 255 both occur (asserted), so the
clamp itself is exercised.

Sampling layouts (YCbCr, Annex K tables, 37x29 unless sizes are named; Y / Cb / Cr as h x v):
  y1x2_WxH     Y 1x2 (4:4:0): h1v2 fancy upsampling.  Heights 1, 2, 3, 17 (chroma height 1 and 2) and
               widths 1, 2, 3 (h1v2 stays fancy below 3 samples a row, unlike h2v1 and h2v2)
  y4x1         Y 4x1 (the real 4:1:1), y1x4, y4x2 (exactly 10 blocks per MCU), y3x1: box replication
               by factors other than 2
  mixed_c      Y 2x2, Cb 2x1, Cr 1x2: three differently shaped planes, h1v2 and h2v1 side by side
  one_c_sub    Y 2x2, Cb 1x1, Cr 2x2: one chroma plane at full resolution
  luma_sub     Y 1x1, Cb 2x2, Cr 2x2: the luma plane is the upsampled one, in colour and in gray records
  gray_22      one component whose frame header says 2x2, 45x23 (a non-interleaved scan: 8x8 units);
               gray_22_33x9: the scan's rows of 5 blocks are shorter than the padded plane's 6
  w_thresh_h2v1_W / w_thresh_h2v2_W   widths 3..6: chroma rows of 2 and 3 samples, box against fancy
  cmyk_440     four components, C 1x2 and M, Y, K 1x1: jpeg_color4 with h1v2
Tables:
  q16              SOF1, 16-bit quantisation tables with entries above 255
  tab_ids_23       SOF1, Huffman tables 2 and 3, luma on 3
  tab_swapped      luma on tables 1, chroma on tables 0
  tab_three        a Huffman table pair per component: the host entropy decoder
  huff_long        explicit tables whose used codes are 9, 10, 11 and 16 bits long; code + value bits of
                   exactly 10 and 11 (asserted on the writer's trace)
  huff_one_symbol  a flat image whose DC table holds a single 1-bit code
Coefficients:
  coef_extremes    DC differences of category 11 in both directions, AC values of category 10
  zz63             every block ends at zigzag 63 (no EOB), some through three ZRLs; tables from statistics
  all_ac           blocks with all 63 AC terms next to blocks with none; tables from statistics
Streams:
  rst1_gray_529    184x184 gray, restart interval 1: 529 segments, more than a 512-lane workgroup
  rst1_444_289     136x136 4:4:4, restart interval 1: 289 segments, more than a 256-lane workgroup
  rst_odd          restart interval 5 over rows of 7 MCUs
  rst_single       a restart interval larger than the scan: no marker appears
  stuffed          at least 50 stuffed FF 00 pairs, one of them the last bytes before an RSTn (asserted)
  fill_bytes       FF FF fill before every RSTn and before EOI
  segments_shuffled  SOF first, then DQT, an APP1, DRI, one DHT segment per table, a COM before SOS
Refused:
  frac_y3x1_c2x1   Y 3x1 over chroma 2x1: a fractional ratio, which libjpeg does not implement

main() also asserts the path each file takes on the host half (aeon_amd.jpeg_host_stage): tab_three
goes to the host entropy decoder, every other file to the GPU one.  jpeg_host_stage does not report
the subsequence count; prepare_gpu gives every restart segment at least one subsequence, so the
two restart-interval-1 files are asserted by their segment counts (RSTn markers + 1) instead.
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
try:  # loaded by the tests (the repository root is on the path), or run as a script
    from tests import jpeg_writer as JW
    from tests.jpeg_blocks import (AC_K, DC_K, HI, LO, RANGE, S420, S444, _note, _q, _rng, _ycc, draw, gray, samples,
                                   sparse_block, ycc)
except ImportError:
    sys.path.insert(0, os.path.dirname(HERE))
    import jpeg_writer as JW
    from jpeg_blocks import (AC_K, DC_K, HI, LO, RANGE, S420, S444, _note, _q, _rng, _ycc, draw, gray, samples,
                             sparse_block, ycc)
# (the block drawer and the YCbCr / gray files live in tests/jpeg_blocks.py, shared with tests/jpeg_size_cases.py)


# ---- blocks of the table / coefficient / stream cases ------------------------------------------------

# huff_long: the AC symbols (run << 4 | size) and DC categories in use and their code lengths
LONG_AC = {0x31: 3, 0x00: 2, 0x01: 9, 0x02: 9, 0x11: 10, 0xF0: 10, 0x03: 11, 0x21: 11, 0x04: 16, 0x12: 16}
LONG_DC = {0: 2, 5: 3, 1: 9, 2: 10, 3: 11, 4: 16}


def long_block(rng, q):
    """A block coded with LONG_AC's symbols only: runs and sizes drawn from the table, a ZRL now and
    then (zeros of 16 + the next symbol's run)."""
    syms = [s for s in LONG_AC if s not in (0x00, 0xF0)]
    while True:
        b, k = np.zeros(64, np.int16), 1
        for _ in range(int(rng.integers(0, 6))):
            s = syms[int(rng.integers(len(syms)))]
            k += (s >> 4) + (16 if rng.integers(4) == 0 else 0)
            if k > 63:
                break
            mag = int(rng.integers(1 << ((s & 15) - 1), 1 << (s & 15)))
            b[JW.ZIGZAG[k]] = mag if rng.integers(2) else -mag
            k += 1
        s = samples(b, q)
        if LO <= s.min() and s.max() <= HI:
            return b


def zz63_block(rng, q):
    """Ends at zigzag 63; one block in three reaches it through three ZRLs (its last term before 63 is
    among the first 15)."""
    while True:
        b = sparse_block(rng, q, dc_span=60, nac=3, amp=40, zmax=15 if rng.integers(3) == 0 else 60).copy()
        b[63] = int(rng.choice([-3, -2, -1, 1, 2, 3]))
        s = samples(b, q)
        if LO <= s.min() and s.max() <= HI:
            return b


def all_ac_block(rng, q):
    b = np.zeros(64, np.int16)
    b[0] = int(rng.integers(-40, 40))
    if rng.integers(2):
        b[1:] = rng.choice([-2, -1, 1, 2], 63)
    return b


def ones_block(rng, q):
    """Values 2^s - 1 (all-ones value bits) at a few places, and 255 at zigzag 63 in half of the blocks:
    a segment that ends with such a block ends with a byte of ones, whatever its alignment."""
    while True:
        b = np.zeros(64, np.int16)
        b[0] = int(rng.integers(-60, 60))
        for _ in range(int(rng.integers(1, 5))):
            b[JW.ZIGZAG[int(rng.integers(1, 63))]] = (1 << int(rng.integers(1, 9))) - 1
        if rng.integers(2):
            b[63] = 255
        s = samples(b, q)
        if LO <= s.min() and s.max() <= HI:
            return b


def _ones(n=1):
    return {0: np.full(64, n), 1: np.full(64, n)}


def _segments(b):
    """Restart segments of the file's scan: its RSTn markers + 1 (FF in entropy-coded data is stuffed)."""
    scan = b[b.index(b"\xff\xda"):]
    return sum(scan.count(bytes([0xFF, 0xD0 + i])) for i in range(8)) + 1


def files():
    """{name: file bytes} of every fixture, and the set of names Pillow must refuse."""
    out = {}
    for w, h in ((37, 29), (5, 1), (5, 2), (5, 3), (5, 17), (1, 9), (2, 9), (3, 9)):
        out[f"y1x2_{w}x{h}"] = ycc(f"y1x2_{w}x{h}", w, h, ((1, 2), (1, 1), (1, 1)))
    for n, hv in (("y4x1", (4, 1)), ("y1x4", (1, 4)), ("y4x2", (4, 2)), ("y3x1", (3, 1))):
        out[n] = ycc(n, 37, 29, (hv, (1, 1), (1, 1)))
    out["mixed_c"] = ycc("mixed_c", 37, 29, ((2, 2), (2, 1), (1, 2)))
    out["one_c_sub"] = ycc("one_c_sub", 37, 29, ((2, 2), (1, 1), (2, 2)))
    out["luma_sub"] = ycc("luma_sub", 37, 29, ((1, 1), (2, 2), (2, 2)))
    out["gray_22"] = gray("gray_22", 45, 23, (2, 2))
    out["gray_22_33x9"] = gray("gray_22_33x9", 33, 9, (2, 2))
    for w in (3, 4, 5, 6):
        out[f"w_thresh_h2v1_{w}"] = ycc(f"w_thresh_h2v1_{w}", w, 9, ((2, 1), (1, 1), (1, 1)))
        out[f"w_thresh_h2v2_{w}"] = ycc(f"w_thresh_h2v2_{w}", w, 9, S420)
    comps = [JW.Component(ord(c), 1, 2 if c == "C" else 1, 0, 0, 0) for c in "CMYK"]
    out["cmyk_440"] = JW.write_jpeg(37, 29, comps, draw("cmyk_440", _rng("cmyk_440"), 37, 29, comps, _q(85)), {0: _q(85)[0]},
                                    {0: JW.K3_DC_LUMA}, {0: JW.K3_AC_LUMA}, jfif=False, adobe=0)

    # tables
    q = {0: np.minimum(JW.K1_LUMA * 6, 1500), 1: np.minimum(JW.K1_CHROMA * 6, 1500)}
    comps = _ycc(S420)
    out["q16"] = JW.write_jpeg(40, 24, comps, draw("q16", _rng("q16"), 40, 24, comps, q), q, DC_K, AC_K, sof=0xC1)
    comps = [JW.Component(1, 2, 1, 0, 3, 3), JW.Component(2, 1, 1, 1, 2, 2), JW.Component(3, 1, 1, 1, 2, 2)]
    out["tab_ids_23"] = JW.write_jpeg(37, 29, comps, draw("tab_ids_23", _rng("tab_ids_23"), 37, 29, comps, _q(80)), _q(80),
                                      {3: JW.K3_DC_LUMA, 2: JW.K3_DC_CHROMA}, {3: JW.K3_AC_LUMA, 2: JW.K3_AC_CHROMA}, sof=0xC1)
    comps = [JW.Component(1, 2, 2, 0, 1, 1), JW.Component(2, 1, 1, 1, 0, 0), JW.Component(3, 1, 1, 1, 0, 0)]
    out["tab_swapped"] = JW.write_jpeg(37, 29, comps, draw("tab_swapped", _rng("tab_swapped"), 37, 29, comps, _q(80)), _q(80),
                                       {1: JW.K3_DC_LUMA, 0: JW.K3_DC_CHROMA}, {1: JW.K3_AC_LUMA, 0: JW.K3_AC_CHROMA})
    comps = [JW.Component(1, 2, 1, 0, 0, 0), JW.Component(2, 1, 1, 1, 1, 1), JW.Component(3, 1, 1, 1, 2, 2)]
    out["tab_three"] = JW.write_jpeg(37, 29, comps, draw("tab_three", _rng("tab_three"), 37, 29, comps, _q(80)), _q(80),
                                     {0: JW.K3_DC_LUMA, 1: JW.K3_DC_CHROMA, 2: JW.K3_DC_LUMA},
                                     {0: JW.K3_AC_LUMA, 1: JW.K3_AC_CHROMA, 2: JW.K3_AC_LUMA}, sof=0xC1)

    comps, rng = _ycc(S420), _rng("huff_long")
    coefs = draw("huff_long", rng, 40, 24, comps, _ones(2), block=long_block)
    for a in coefs:  # DC levels whose differences stay within LONG_DC's categories (scan order is not
        a[..., 0] = rng.integers(-15, 16, a.shape[:2])  # raster order, so any two levels: |d| <= 30)
        for b in a.reshape(-1, 64):
            _note("huff_long", samples(b, _ones(2)[0]))
    tab_dc, tab_ac, trace = JW.huffman_from_lengths(LONG_DC), JW.huffman_from_lengths(LONG_AC), []
    out["huff_long"] = JW.write_jpeg(40, 24, comps, coefs, _ones(2), {0: tab_dc, 1: tab_dc}, {0: tab_ac, 1: tab_ac}, trace=trace)
    coded = [t for t in trace if isinstance(t[0], int)]
    assert {9, 10, 11, 16} <= {t[2] for t in coded if t[0] == 1} and {9, 10, 11, 16} <= {t[2] for t in coded if t[0] == 0}
    assert {10, 11} <= {t[2] + t[3] for t in coded}
    assert any(t[1] == 0xF0 for t in coded)

    comps = _ycc(S444)
    coefs = [np.zeros((3, 4, 64), np.int16) for _ in comps]
    _note("huff_one_symbol", samples(coefs[0][0, 0], _ones()[0]))
    one = ([1] + [0] * 15, [0])
    out["huff_one_symbol"] = JW.write_jpeg(27, 19, comps, coefs, _q(75), {0: one, 1: one}, AC_K)

    # coefficients
    comps = [JW.Component(1, 1, 1, 0, 0, 0)]
    a = np.zeros((4, 5, 64), np.int16)
    a[..., 0] = np.where(np.arange(20).reshape(4, 5) % 2 == 0, -1023, 1024)
    a[1, 1] = a[2, 3] = 0
    a[1, 1, 1], a[2, 3, 8], a[2, 3, 9] = 700, -1000, 512
    trace = []
    out["coef_extremes"] = JW.write_jpeg(37, 29, comps, [a], {0: np.ones(64, np.int64)}, {0: JW.K3_DC_LUMA},
                                         {0: JW.K3_AC_LUMA}, trace=trace)
    for b in a.reshape(-1, 64):
        _note("coef_extremes", samples(b, np.ones(64)))
    assert sum(t[0] == 0 and t[1] == 11 for t in trace) >= 10 and sum(t[0] == 1 and t[1] & 15 == 10 for t in trace) == 3

    for name, block, size in (("zz63", zz63_block, (40, 24)), ("all_ac", all_ac_block, (37, 29))):
        comps, q, trace = _ycc(S420), _q(90) if name == "zz63" else _ones(), []
        coefs = draw(name, _rng(name), *size, comps, q, block=block)
        dcs, acs = JW.scan_statistics(*size, comps, coefs)
        out[name] = JW.write_jpeg(*size, comps, coefs, q, {i: JW.huffman_from_stats(f) for i, f in dcs.items()},
                                  {i: JW.huffman_from_stats(f) for i, f in acs.items()}, trace=trace)
        coded = [t for t in trace if isinstance(t[0], int)]
        if name == "zz63":
            assert not any(t[0] == 1 and t[1] == 0 for t in coded)  # no EOB at all
            assert any(coded[i][1] == coded[i + 1][1] == coded[i + 2][1] == 0xF0 and coded[i][0] == 1 for i in range(len(coded) - 2))
        else:
            assert any(t[0] == 1 and t[1] == 0 for t in coded)

    # streams
    out["rst1_gray_529"] = gray("rst1_gray_529", 184, 184, draw_kw=dict(nac=1, amp=30, dc_span=120, zmax=4), restart=1)
    out["rst1_444_289"] = ycc("rst1_444_289", 136, 136, S444, draw_kw=dict(nac=1, amp=30, dc_span=120, zmax=4), restart=1)
    assert _segments(out["rst1_gray_529"]) == 529 and _segments(out["rst1_444_289"]) == 289
    out["rst_odd"] = ycc("rst_odd", 56, 24, S444, restart=5)
    out["rst_single"] = ycc("rst_single", 20, 20, S420, restart=100)
    assert not any(bytes([0xFF, 0xD0 + i]) in out["rst_single"] for i in range(8))
    comps = _ycc(S444)
    out["stuffed"] = JW.write_jpeg(48, 40, comps, draw("stuffed", _rng("stuffed"), 48, 40, comps, _ones(), block=ones_block),
                                   _ones(), DC_K, AC_K, restart=2)
    scan = out["stuffed"][out["stuffed"].index(b"\xff\xda"):]
    assert scan.count(b"\xff\x00") >= 50, scan.count(b"\xff\x00")
    assert any(b"\xff\x00" + bytes([0xFF, 0xD0 + i]) in scan for i in range(8))
    out["fill_bytes"] = ycc("fill_bytes", 37, 29, S420, restart=2, fill_rst=1, fill_eoi=1)
    assert b"\xff\xff\xd0" in out["fill_bytes"] and out["fill_bytes"].endswith(b"\xff\xff\xd9")
    out["segments_shuffled"] = ycc("segments_shuffled", 37, 29, S420, restart=3, dht_split=True,
                                   layout=("SOF", "DQT", (0xE1, b"Exif\0\0not really"), "DRI", "DHT", (0xFE, b"a comment")))

    refused = {"frac_y3x1_c2x1"}
    out["frac_y3x1_c2x1"] = ycc("frac_y3x1_c2x1", 37, 29, ((3, 1), (2, 1), (2, 1)))
    assert any(r[0] < -1 and r[1] > 256 for r in RANGE.values())  # one file clamps at both ends
    return out, refused


def _decode(b):
    from PIL import Image
    sys.path.insert(0, os.path.dirname(HERE))
    import jpeg_cmyk_ref as R
    im = Image.open(io.BytesIO(b))
    if im.mode == "CMYK":
        return R.decode(R.raw_from_pillow(im))
    bgr = np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])
    im = Image.open(io.BytesIO(b))
    im.draft("L", im.size)  # libjpeg JCS_GRAYSCALE output: the (upsampled) Y component
    gray_px = np.asarray(im if im.mode == "L" else im.convert("L"))
    return bgr, gray_px


def main():
    import warnings
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import aeon_amd as A
    warnings.simplefilter("error")  # a libjpeg warning (corrupt data, extraneous bytes) is a writer bug
    fs, refused = files()
    fx, got_refused = {}, set()
    for name, b in fs.items():
        fx[name + ".jpg"] = np.frombuffer(b, np.uint8)
        try:
            bgr, gray_px = _decode(b)
        except Exception as e:  # Pillow refuses the file
            print("refused by Pillow:", name, "--", e)
            got_refused.add(name)
            continue
        assert bgr.shape[:2] == gray_px.shape == A.jpeg_info(b)[1::-1], name
        fx[name + ".bgr"], fx[name + ".gray"] = bgr, gray_px
        assert A.jpeg_host_stage(b)[0] == (name != "tab_three"), name
    assert got_refused == refused, (got_refused, refused)
    assert _segments(fs["rst1_gray_529"]) > 512 and _segments(fs["rst1_444_289"]) > 256
    fx["refused"] = np.array(sorted(refused))
    path = os.path.join(HERE, "jpeg_layout_fixtures.npz")
    np.savez_compressed(path, **fx)
    print(len(fs), "fixtures,", os.path.getsize(path), "bytes; sample range",
          min(r[0] for r in RANGE.values()), max(r[1] for r in RANGE.values()))


if __name__ == "__main__":
    sys.exit(main())
