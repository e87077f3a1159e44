"""Generate the committed fixtures of the CMYK / YCCK / Adobe-RGB JPEG decode.

Run by hand where Pillow is installed; the output is committed.  Every file is written by Pillow
(libjpeg-turbo); the expected records are Pillow's decode taken back to libjpeg's raw samples and
through tests/jpeg_cmyk_ref.py's formulas.

jpeg_cmyk_fixtures.npz, per fixture <name>:
  <name>.jpg    the file's bytes (uint8)
  <name>.bgr    the HWC BGR record (cv::imdecode(..., CV_LOAD_IMAGE_COLOR))
  <name>.gray   the grayscale record (CV_LOAD_IMAGE_GRAYSCALE)
and for the YCCK fixture its libjpeg samples before and after jdcolor.c's ycck_cmyk_convert:
  ycck_37x53.ycck   the Y, Cb, Cr, K samples (the same file decoded as CMYK, Adobe transform 0)
  ycck_37x53.cmyk   the C, M, Y, K samples (Pillow's decode of the YCCK file, inverted back)

Fixtures (content: a random grid upscaled 3x, so blocks hold edges and the values cover the range):
  cmyk_444_*     4:4:4, Adobe transform 0, 37x53 / 1x1 / 2x5 / 8x8 (widths below 3: the box upsampler)
  cmyk_sub2_*    subsampling=2: C at 2x2, M, Y, K at 1x1 (h2v2 fancy upsampling of M, Y and K)
  prog_cmyk      progressive: the host entropy decoder
  cmyk_rst       restart intervals
  ycck_37x53     byte 11 of the Adobe segment patched 0 -> 2: libjpeg's YCCK path
  cmyk_noadobe   the APP14 segment cut out: still CMYK
  rgb_adobe      3 components, keep_rgb: Adobe transform 0, ids R, G, B
  cmyk_long      160x120 noise, q95, subsampling=2: several Huffman subsequences per lane
  cmyk_strided   240x180 noise, q95, subsampling=2: above 64 KB of entropy-coded data, so a 256-lane
                 Huffman workgroup takes more than one subsequence per lane (the strided phases)
  cmyk_k255 / cmyk_k0   flat K at both ends of the range (the CMYK formulas' corner cases)
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cmyk_ref as R  # noqa: E402


def _blocky(rng, w, h, ch):
    g = rng.integers(0, 256, ((h + 2) // 3, (w + 2) // 3, ch)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(g, 3, axis=0), 3, axis=1)[:h, :w])


def _save(arr, mode, **kw):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(arr, mode).save(bio, "JPEG", **kw)
    return bio.getvalue()


def _adobe(b):
    """Offset of the Adobe APP14 marker and its segment length."""
    i = b.index(b"\xff\xee")
    assert b[i + 4:i + 9] == b"Adobe"
    return i, (b[i + 2] << 8) | b[i + 3]


def files():
    rng = np.random.default_rng(4141)
    out = {}
    for w, h in ((37, 53), (1, 1), (2, 5), (8, 8)):
        out[f"cmyk_444_{w}x{h}"] = _save(_blocky(rng, w, h, 4), "CMYK", quality=90, subsampling=0)
    for w, h in ((37, 53), (16, 16)):
        out[f"cmyk_sub2_{w}x{h}"] = _save(_blocky(rng, w, h, 4), "CMYK", quality=85, subsampling=2)
    out["prog_cmyk"] = _save(_blocky(rng, 37, 53, 4), "CMYK", quality=90, subsampling=2, progressive=True)
    out["cmyk_rst"] = _save(_blocky(rng, 45, 29, 4), "CMYK", quality=90, subsampling=0, restart_marker_blocks=3)
    src = _save(_blocky(rng, 37, 53, 4), "CMYK", quality=92, subsampling=0)
    i, _ = _adobe(src)
    assert src[i + 4 + 11] == 0
    out["ycck_37x53"] = src[:i + 15] + b"\x02" + src[i + 16:]
    out["_ycck_source"] = src
    src = _save(_blocky(rng, 40, 24, 4), "CMYK", quality=90, subsampling=2)
    i, n = _adobe(src)
    out["cmyk_noadobe"] = src[:i] + src[i + 2 + n:]
    out["rgb_adobe"] = _save(_blocky(rng, 37, 53, 3), "RGB", quality=90, subsampling=0, keep_rgb=True)
    out["cmyk_long"] = _save(rng.integers(0, 256, (120, 160, 4)).astype(np.uint8), "CMYK", quality=95, subsampling=2)
    out["cmyk_strided"] = _save(rng.integers(0, 256, (180, 240, 4)).astype(np.uint8), "CMYK", quality=95, subsampling=2)
    assert len(out["cmyk_strided"]) > 66 * 1024
    for name, k in (("cmyk_k255", 0), ("cmyk_k0", 255)):  # (Pillow's K is 255 - libjpeg's)
        a = _blocky(rng, 21, 19, 4)
        a[..., 3] = k
        out[name] = _save(a, "CMYK", quality=100, subsampling=0)
    return out


def main():
    from PIL import Image
    fx = {}
    fs = files()
    ycck_src = fs.pop("_ycck_source")
    for name, b in fs.items():
        im = Image.open(io.BytesIO(b))
        assert im.mode == ("RGB" if name == "rgb_adobe" else "CMYK"), (name, im.mode)
        raw = R.raw_from_pillow(im)
        bgr, gray = R.decode(raw)
        fx[name + ".jpg"] = np.frombuffer(b, np.uint8)
        fx[name + ".bgr"] = bgr
        fx[name + ".gray"] = gray
    fx["ycck_37x53.ycck"] = R.raw_from_pillow(Image.open(io.BytesIO(ycck_src)))
    fx["ycck_37x53.cmyk"] = R.raw_from_pillow(Image.open(io.BytesIO(fs["ycck_37x53"])))
    np.savez_compressed(os.path.join(HERE, "jpeg_cmyk_fixtures.npz"), **fx)
    print(len(fs), "fixtures,", os.path.getsize(os.path.join(HERE, "jpeg_cmyk_fixtures.npz")), "bytes")


if __name__ == "__main__":
    sys.exit(main())
