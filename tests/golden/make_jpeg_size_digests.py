"""Generate tests/golden/jpeg_size_digests.npz: the reference of the JPEG size sweep (tests/jpeg_size_cases.py).

Run by hand where Pillow is installed (Pillow 12.2 / libjpeg-turbo); the output is committed.  Every file of the
sweep is decoded by Pillow exactly as make_jpeg_layout_fixtures.py decodes: convert("RGB") reversed to BGR,
draft("L") for gray, the four-component files through tests/jpeg_cmyk_ref.py.  Digests only, no pixels:

  names   the files, in the order of jpeg_size_cases.all_cases()
  jpg     per file, the first 8 bytes of the SHA-256 of its bytes (pins the generator)
  bgr     per file, the SHA-256 of Pillow's HWC BGR record
  gray    per file, the SHA-256 of Pillow's grayscale record
"""
import hashlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import jpeg_cmyk_ref as R  # noqa: E402
from tests import jpeg_size_cases as J  # noqa: E402


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def pillow_decode(b):
    """(BGR, gray) of a file as cv::imdecode gives them, from Pillow's decode."""
    from PIL import Image
    im = Image.open(io.BytesIO(b))
    if im.mode == "CMYK":
        return R.decode(R.raw_from_pillow(im))
    bgr = np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])
    im = Image.open(io.BytesIO(b))
    im.draft("L", im.size)  # libjpeg JCS_GRAYSCALE output: the (upsampled) Y component
    return bgr, np.asarray(im if im.mode == "L" else im.convert("L"))


def digests():
    """{key: array} as committed."""
    import warnings
    warnings.simplefilter("error")  # a libjpeg warning (corrupt data, extraneous bytes) is a writer bug
    cases = J.all_cases()
    out = {"names": np.array([c.name for c in cases]), "jpg": np.zeros((len(cases), 8), np.uint8),
           "bgr": np.zeros((len(cases), 32), np.uint8), "gray": np.zeros((len(cases), 32), np.uint8)}
    for i, c in enumerate(cases):
        b = J.jpg(c)
        bgr, gray = pillow_decode(b)
        assert bgr.shape == (c.h, c.w, 3) and gray.shape == (c.h, c.w), c.name
        out["jpg"][i], out["bgr"][i], out["gray"][i] = sha(np.frombuffer(b, np.uint8))[:8], sha(bgr), sha(gray)
    return out


def main():
    path = os.path.join(HERE, "jpeg_size_digests.npz")
    d = digests()
    np.savez_compressed(path, **d)
    print(len(d["names"]), "files,", sum(len(J.jpg(c)) for c in J.all_cases()), "bytes of JPEG,", os.path.getsize(path),
          "bytes of digests")


if __name__ == "__main__":
    sys.exit(main())
