"""tests/tiff_writer.py against Pillow (libtiff): Pillow reads each writer file back to the pixels it was made from, so
a writer bug cannot pass as a decoder rule.  What Pillow does not read at all (gray + extra sample at 16 bits, palette
+ extra sample, big-endian 16-bit WhiteIsZero) or reads by another rule (16-bit WhiteIsZero: Pillow hands the samples
on as stored; the decoder inverts) is listed here by kind, and nothing else is let off.
"""
import io

import numpy as np
from PIL import Image

from tests import tiff_cases as TC
from tests import tiff_ref as R
from tests import tiff_writer as W

UNREAD = ("ga16_", "pala8_")  # kinds Pillow cannot identify


def _pillow(f):
    im = Image.open(io.BytesIO(f))
    im.load()
    return im


def test_pillow_reads_every_case_file_back():
    seen = set()
    for name, f in TC.device_files() + TC.host_files():
        a, T = R.samples(f)  # the samples the file was made from, by the tests' own reader of strips
        photo = T[262][0]
        if name.startswith(UNREAD) or (name.startswith("align") and T[277][0] == 2):
            continue
        try:
            im = _pillow(f)
        except Exception:
            assert photo == 0 and a.dtype == np.uint16 and f[:2] == b"MM", name  # the one more form Pillow has no mode for
            continue
        px = np.array(im)
        seen.add(im.mode)
        if name == "orientation":
            px = px[:, ::-1]  # (Pillow applies Orientation 2, a mirror; cv::imdecode of OpenCV 2.4 does not)
        if im.mode == "P":
            assert np.array_equal(px, a[:, :, 0]), name
            pal = np.array(im.getpalette()).reshape(-1, 3)
            assert np.array_equal(pal[:256], (np.array(T[320]).reshape(3, 256).T >> 8)[:len(pal)]), name
        elif im.mode == "L":
            assert np.array_equal(px, 255 - a[:, :, 0] if photo == 0 else a[:, :, 0]), name
        elif im.mode in ("I;16", "I;16B"):
            assert np.array_equal(px, a[:, :, 0]), name  # as stored, WhiteIsZero too
        elif im.mode == "RGB":
            assert np.array_equal(px, a[:, :, :3] if a.dtype == np.uint8 else (a[:, :, :3] >> 8)), name
        else:
            assert im.mode in ("RGBA", "RGBX", "RGBa", "LA"), (name, im.mode)
            if T.get(338) == [1]:  # associated alpha: Pillow divides the colour by it on the way to RGBA;
                assert px.shape == a.shape, name  # the decoder drops the sample (parity unpinned)
                continue
            want = a if a.dtype == np.uint8 else (a >> 8)
            assert np.array_equal(px[:, :, :want.shape[2] - 1], want[:, :, :-1]), name
    assert {"L", "RGB", "P", "I;16"} <= seen


def test_lzw_streams_hold_what_their_names_say():
    rng = np.random.default_rng(5)
    noise = bytes(rng.integers(0, 256, 5600).astype(np.uint8))
    s, st = W.lzw(noise)
    assert st["widths"] == {9, 10, 11, 12} and st["clears"] >= 2 and st["max_entries"] <= 4094 + 1
    s, st = W.lzw(noise, fill=True)
    assert st["max_entries"] == 4096 and st["after_full"] >= 60 and st["clears"] == 2
    s, st = W.lzw(noise[:400], clear_at=(100, 101))
    assert st["clears"] == 3
    assert W.lzw(b"abc", eoi=False)[0] != W.lzw(b"abc")[0]
    # aaaa...: the second code of the run is the entry being defined
    s, _ = W.lzw(b"a" * 7)
    codes = [int(format(int.from_bytes(s, "big"), "0%db" % (8 * len(s)))[9 * i:9 * i + 9], 2) for i in range(5)]
    assert codes[:4] == [256, 97, 258, 259]


def test_packbits_stream_has_every_control_class():
    name, f = [c for c in TC.device_files() if c[0] == "packbits_classes"][0]
    _, T = R.parse(f)
    d = f[T[273][0]:T[273][0] + T[279][0]]
    seen, i = set(), 0
    while i < len(d):
        c = d[i]
        seen.add("noop" if c == 128 else "lit1" if c == 0 else "lit128" if c == 127 else "lit" if c < 128 else
                 "rep128" if c == 129 else "rep2" if c == 255 else "rep")
        i += 1 if c == 128 else c + 2 if c < 128 else 2
    assert seen == {"noop", "lit1", "lit128", "lit", "rep128", "rep2", "rep"}, seen


def test_hand_deflate_is_zlib_readable():
    import zlib
    data = bytes(range(256)) * 3 + b"\x07" * 700 + b"xyz"
    assert zlib.decompress(W.deflate_stored(data, 300)) == data
    assert zlib.decompress(W.deflate_fixed(data)) == data
    assert len(W.deflate_fixed(data)) < len(data)
