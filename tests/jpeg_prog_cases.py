"""The progressive JPEG files of tests/test_jpeg_prog.py (CPU) and tests/test_hip_jpeg_prog.py (GPU): data only, a
name -> file bytes table.  The drawn files are written by Pillow (progressive=True, so libjpeg's scan scripts: ten
scans for three components, six for gray), each the smallest shape at which a piece of jpeg_prog.hip can go wrong; the
rest are the progressive entries of the committed fixtures (aeon's two images re-encoded among them)."""
import functools
import io
import os

import numpy as np
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _save(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", progressive=True, **kw)
    return b.getvalue()


def _noise(seed, h, w, cn):
    return np.random.RandomState(seed).randint(0, 256, (h, w, cn) if cn > 1 else (h, w)).astype(np.uint8)


def _specks():
    a = np.full((40, 264, 3), 128, np.uint8)
    for y, x in ((3, 5), (20, 130), (21, 131), (38, 260)):
        a[y, x] = (250, 20, 90)
    return a


@functools.lru_cache(maxsize=None)
def files():
    t = {
        "gray_1x1": _save(_noise(1, 1, 1, 1)),                                       # one block; scans of one block
        "s420_1x1": _save(_noise(2, 1, 1, 3), subsampling=2),                        # one block per component
        "s444_8x8_q90": _save(_noise(3, 8, 8, 3), quality=90, subsampling=0),        # interleaved DC, one block per MCU
        "s420_17x9_q95": _save(_noise(4, 9, 17, 3), quality=95, subsampling=2),      # 3x2 grid in a 4x2 plane, partial MCUs
        "s444_64x64_q100": _save(_noise(5, 64, 64, 3), quality=100, subsampling=0),  # long codes, ZRL in refinement, fields > 32 bits
        "s420_264x40_specks_q50": _save(_specks(), quality=50, subsampling=2),       # EOB runs across block rows, refinement inside runs
        "gray_1480_flat": _save(np.full((1480, 1480), 77, np.uint8)),                # 34,225 blocks: an EOB run at 0x7FFF
        "gray_33x70_q75": _save(_noise(6, 70, 33, 1), quality=75),                   # gray script; 45 blocks, units beyond one workgroup
        "s420_40x24_rst": _save(_noise(7, 24, 40, 3), quality=85, subsampling=2, restart_marker_blocks=2),  # restart intervals
    }
    for npz, keep in (("jpeg_fixtures.npz", lambda k: k.startswith("prog_") and k.endswith(".jpg")), ("jpeg_cmyk_fixtures.npz", lambda k: k == "prog_cmyk.jpg")):
        z = np.load(os.path.join(GOLDEN, npz))
        t.update({k[:-4]: z[k].tobytes() for k in z.files if keep(k)})
    return t


def _scan_bodies(f):
    """(first, end) of every scan's entropy-coded bytes: from behind the SOS header to the next marker that is
    neither a stuffed 0xFF nor RSTn."""
    out, p = [], 2
    while p + 4 <= len(f):
        assert f[p] == 0xFF
        m, n = f[p + 1], int.from_bytes(f[p + 2:p + 4], "big")
        p += 2 + n
        if m == 0xDA:
            e = p
            while not (f[e] == 0xFF and f[e + 1] != 0 and not 0xD0 <= f[e + 1] <= 0xD7):
                e += 1
            out.append((p, e))
            p = e
        if f[p + 1] == 0xD9:
            break
    return out


def corrupt(name="s420_17x9_q95"):
    """`name` with its first AC scan's bytes overwritten by FF 00 pairs: all ones once unstuffed, which no Huffman
    table codes."""
    f = files()[name]
    a, e = _scan_bodies(f)[1]
    return f[:a] + (b"\xff\x00" * (e - a))[:e - a - (e - a) % 2] + b"\x00" * ((e - a) % 2) + f[e:]


def cut(name="s444_64x64_q100"):
    """`name` cut off inside a scan -- the last but one of those that hold a stuffed pair, behind that pair's 0xFF: the
    decoders read that as a marker, what the scan still wants as zeros, and the later scans are missing."""
    f = files()[name]
    at = [f.rfind(b"\xff\x00", a, e) for a, e in _scan_bodies(f)]
    return f[:sorted(p for p in at if p >= 0)[-2] + 1]
