"""Inputs that exhaust the photometric stages' domain: the cube of all 2^24 BGR triples cut into records,
and a coarse lattice of it as one record.  Pixel i of the cube is (B, G, R) = (i >> 16, i >> 8 & 255,
i & 255); a record of w x h pixels holds w * h consecutive cube pixels, row-major, and the last record is
padded by repeating the cube's start.  tests/test_colour_cases.py pins both."""
import numpy as np

CUBE = 1 << 24

# the levels per channel of the lattice record: 36 evenly spaced over [0, 255] and the neighbours of both
# ends and of the middle (0, 1, 127, 128, 254, 255 among them), 40 in all -- 64,000 triples, a 256 x 250 record
LATTICE_LEVELS = tuple(sorted({(k * 255 + 17) // 35 for k in range(36)} | {1, 127, 128, 254}))
LATTICE_W, LATTICE_H = 256, 250


def cube_pixels(first, count):
    """(count, 3) uint8: cube pixels first .. first + count - 1, indices taken modulo 2^24."""
    i = (np.arange(first, first + count, dtype=np.int64) % CUBE).astype(np.uint32)
    px = np.empty((count, 3), np.uint8)
    px[:, 0] = i >> 16
    px[:, 1] = (i >> 8) & 255
    px[:, 2] = i & 255
    return px


def cube_record_count(w, h):
    return -(-CUBE // (w * h))


def cube_record(k, w, h):
    """Record k of the cube cut into w x h records: (h, w, 3) uint8."""
    if not 0 <= k < cube_record_count(w, h):
        raise IndexError(k)
    return cube_pixels(k * w * h, w * h).reshape(h, w, 3)


def cube_records(w, h, first=0, count=None):
    """Records first .. first + count - 1 (default: to the last) of the cube cut into w x h records."""
    n = cube_record_count(w, h)
    last = n if count is None else min(n, first + count)
    return [cube_record(k, w, h) for k in range(first, last)]


def lattice_record():
    """(LATTICE_H, LATTICE_W, 3) uint8: every triple over LATTICE_LEVELS, B slowest."""
    lv = np.array(LATTICE_LEVELS, np.uint8)
    b, g, r = np.meshgrid(lv, lv, lv, indexing="ij")
    px = np.stack([b, g, r], axis=-1).reshape(-1, 3)
    assert px.shape[0] == LATTICE_W * LATTICE_H
    return np.ascontiguousarray(px.reshape(LATTICE_H, LATTICE_W, 3))


def triple_index(img):
    """Cube index of every pixel of an (..., 3) uint8 array."""
    a = np.asarray(img).astype(np.uint32)
    return (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]
