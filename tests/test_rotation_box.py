"""The LDS source box of rotate_tiles (aeon_amd/csrc/rotate_kernels.hip) against the capacity the host gives
it, without a GPU: a numpy restatement of the kernel's corner-box rule -- warpAffine's X0 / Y0 / adelta /
bdelta terms, each rounded with rint, the >> 10 (nearest) and >> 5 >> 5 (bilinear) taps saturated to short,
+ 1 for the bilinear second tap, the pitch rounded up to 4 -- over every tile of whole-record windows of
sources from 1 x 1 to 700 x 500, every integer angle in [-360, 360], both interpolations, against a Python
restatement of rot_box_words.  The kernel flags error bit 64 and writes nothing where the box exceeds the
launch's words; this pins the margin against a change of the tile size or of the + 4.

The tile size, the capacity and the margin are read from the kernel's source, so the restatement follows them.

Measured: the fullest bilinear box is 0.961 of rot_box_words (a 700 x 500 source at 120 degrees, which is
also -240), the fullest nearest one 0.894 (318 degrees).  The margin is wider than the rule needs: a tile's
extent is at most ceil(TX |cos| + TY |sin|) - (|cos| + |sin|) + 1 + the second tap, so with + 1 the fullest
box is exactly rot_box_words (ratio 1.000 over the same sweep) and only + 0 overflows (at most bilinear angles)."""
import math
import os
import re

import numpy as np
import pytest

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aeon_amd", "csrc", "rotate_kernels.hip")


def kernel_constants():
    """(kRotTX, kRotTY, kRotMaxWords, rot_box_words' margin) as rotate_kernels.hip spells them: the restatement
    below follows a change of the tile size or of the margin, and fails if the box then no longer fits."""
    text = open(SOURCE).read()
    tile = re.search(r"constexpr int kRotTX = (\d+), kRotTY = (\d+);", text)
    most = re.search(r"constexpr int kRotMaxWords = (\d+) \* (\d+);", text)
    size = re.search(r"const int\s+w = \(int\)std::ceil\(kRotTX \* c \+ kRotTY \* s\) \+ (\d+), "
                     r"h = \(int\)std::ceil\(kRotTX \* s \+ kRotTY \* c\) \+ (\d+);\s+"
                     r"return \(\(w \+ 3\) & ~3\) \* h;", text)
    assert tile and most and size, "rotate_kernels.hip no longer spells its box rule as this test restates it"
    assert size.group(1) == size.group(2)
    return int(tile.group(1)), int(tile.group(2)), int(most.group(1)) * int(most.group(2)), int(size.group(1))


TX, TY, MAX_WORDS, MARGIN = kernel_constants()
ANGLES = list(range(-360, 361))
SIZES = [(1, 1), (2, 1), (1, 2), (3, 3), (5, 4), (31, 17), (63, 31), (64, 32), (65, 33), (129, 65), (150, 100),
         (97, 203), (333, 217), (500, 700), (640, 480), (700, 500)]


def rot_box_words(angle):
    a = angle * (3.14159265358979323846 / 180)
    c, s = abs(math.cos(a)), abs(math.sin(a))
    w, h = math.ceil(TX * c + TY * s) + MARGIN, math.ceil(TX * s + TY * c) + MARGIN
    return ((w + 3) & ~3) * h


def inverse_map(w, h, angle):
    """rotation_inverse_map (plan.cpp): getRotationMatrix2D about (w / 2, h / 2), inverted as warpAffine does."""
    cx, cy = float(w // 2), float(h // 2)
    a = angle * (3.1415926535897932384626433832795 / 180)
    alpha, beta = math.cos(a), math.sin(a)
    m = [alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy]
    d = m[0] * m[4] - m[1] * m[3]
    d = 1. / d if d != 0 else 0.
    a11, a22 = m[4] * d, m[0] * d
    m[0] = a11
    m[1] *= -d
    m[3] *= -d
    m[4] = a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def taps(M, x, y, linear):
    """First source tap (sx, sy) of output pixels (x, y) (int64 arrays that broadcast): RotMap::tap."""
    rdelta = 1024 // 32 // 2 if linear else 1024 // 2
    X = np.rint((M[1] * y + M[2]) * 1024).astype(np.int64) + rdelta + np.rint(M[0] * x * 1024).astype(np.int64)
    Y = np.rint((M[4] * y + M[5]) * 1024).astype(np.int64) + rdelta + np.rint(M[3] * x * 1024).astype(np.int64)
    sh = (lambda v: v >> 5 >> 5) if linear else (lambda v: v >> 10)
    return np.clip(sh(X), -32768, 32767), np.clip(sh(Y), -32768, 32767)


def tile_boxes(w, h, M, linear):
    """(bx0, by0, bw, bh, words) per tile of the whole-record window, from the tiles' four corners."""
    tx0 = np.arange(0, w, TX, dtype=np.int64)[None, :]
    ty0 = np.arange(0, h, TY, dtype=np.int64)[:, None]
    tx1, ty1 = np.minimum(tx0 + TX, w) - 1, np.minimum(ty0 + TY, h) - 1
    sx, sy = zip(*[taps(M, x + 0 * y, y + 0 * x, linear) for x in (tx0, tx1) for y in (ty0, ty1)])
    sx, sy = np.stack(sx), np.stack(sy)
    bx0, by0 = sx.min(0), sy.min(0)
    bw, bh = sx.max(0) + linear - bx0 + 1, sy.max(0) + linear - by0 + 1
    return bx0, by0, bw, bh, ((bw + 3) & ~3) * bh


def test_rot_box_words_fits_the_kernel_capacity():
    assert max(rot_box_words(a) for a in ANGLES) <= MAX_WORDS


@pytest.mark.parametrize("linear", [1, 0], ids=["bilinear", "nearest"])
def test_corner_box_never_exceeds_rot_box_words(linear):
    worst = (0.0, None)
    for w, h in SIZES:
        for angle in ANGLES:
            words = tile_boxes(w, h, inverse_map(w, h, angle), linear)[4]
            cap = rot_box_words(angle)
            assert words.max() <= cap, (w, h, angle, int(words.max()), cap)
            worst = max(worst, (words.max() / cap, (w, h, angle)))
    print(f"fullest box: {worst[0]:.3f} of rot_box_words at {worst[1]}")
    # (a restatement that found no nearly full box would be checking nothing; nearest has no second tap)
    assert (0.9 if linear else 0.85) < worst[0] <= 1.0


@pytest.mark.parametrize("linear", [1, 0], ids=["bilinear", "nearest"])
def test_every_tap_of_a_tile_lies_in_its_corner_box(linear):
    """The kernel's own premise: the taps are monotone in x and in y, so the corners bound them."""
    w, h = 150, 100
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    for angle in ANGLES:
        M = inverse_map(w, h, angle)
        sx, sy = taps(M, x + 0 * y, y + 0 * x, linear)
        bx0, by0, bw, bh, _ = tile_boxes(w, h, M, linear)
        for ty in range(bx0.shape[0]):
            for tx in range(bx0.shape[1]):
                qx = sx[ty * TY:(ty + 1) * TY, tx * TX:(tx + 1) * TX] - bx0[ty, tx]
                qy = sy[ty * TY:(ty + 1) * TY, tx * TX:(tx + 1) * TX] - by0[ty, tx]
                assert qx.min() >= 0 and qy.min() >= 0 and qx.max() + linear < bw[ty, tx] and \
                    qy.max() + linear < bh[ty, tx], (angle, tx, ty)
