"""Seeded coefficient blocks for files written by tests/jpeg_writer.py, and the YCbCr / gray files made of them
(shared by tests/golden/make_jpeg_layout_fixtures.py and tests/jpeg_size_cases.py; numpy only).

Coefficients are sparse random blocks.  Each block is checked with a float64 inverse DCT: every sample
(level shift included) lies in [-256, 511], where libjpeg's range-limit table clamps; outside it the
table wraps and the C and SIMD IDCTs disagree.  A block outside the range is drawn again (blocks with
fixed content assert the range instead).
"""
import zlib

import numpy as np

try:  # loaded by the tests (the repository root is on the path), or next to a script's own import
    from tests import jpeg_writer as JW
except ImportError:
    import jpeg_writer as JW

LO, HI = -256.0, 511.0  # the samples libjpeg's range-limit table clamps (beyond: it wraps)

_u = np.arange(8)
_C = np.cos((2 * _u[None, :] + 1) * _u[:, None] * np.pi / 16) / 2
_C[0] /= np.sqrt(2)

RANGE = {}  # fixture -> [lowest, highest] sample before the clamp


def samples(block, q):
    """The float64 inverse DCT of a quantised block (natural order), level shift included."""
    f = (block.astype(np.float64) * np.asarray(q, np.float64)).reshape(8, 8)
    return _C.T @ f @ _C + 128.0


def _note(name, s):
    assert LO <= s.min() and s.max() <= HI, (name, s.min(), s.max())
    r = RANGE.setdefault(name, [s.min(), s.max()])
    r[0], r[1] = min(r[0], s.min()), max(r[1], s.max())


def _rng(name):
    return np.random.default_rng([5150, zlib.crc32(name.encode())])


def sparse_block(rng, q, dc_span=150, nac=4, amp=70, zmax=24):
    """A random sparse block inside the clamped range: a DC level of 128 +- dc_span and up to nac AC
    terms of roughly +- amp samples each among the first zmax zigzag positions."""
    while True:
        b = np.zeros(64, np.int16)
        b[0] = int(round(rng.uniform(-dc_span, dc_span) * 8 / q[0]))
        for _ in range(int(rng.integers(0, nac + 1))):
            n = JW.ZIGZAG[int(rng.integers(1, zmax))]
            b[n] = int(np.clip(round(rng.uniform(-amp, amp) * 4 / q[n]), -1023, 1023))
        s = samples(b, q)
        if LO <= s.min() and s.max() <= HI:
            return b


def draw(name, rng, w, h, comps, qtables, block=sparse_block, **kw):
    """Coefficients of every component: block(rng, q, **kw) per block, padding blocks included."""
    _, _, blocks = JW.grid(w, h, comps)
    out = []
    for c, (bx, by) in zip(comps, blocks):
        a = np.zeros((by, bx, 64), np.int16)
        for y in range(by):
            for x in range(bx):
                a[y, x] = block(rng, qtables[c.tq], **kw)
                _note(name, samples(a[y, x], qtables[c.tq]))
        out.append(a)
    return out


DC_K, AC_K = {0: JW.K3_DC_LUMA, 1: JW.K3_DC_CHROMA}, {0: JW.K3_AC_LUMA, 1: JW.K3_AC_CHROMA}


def _q(quality):
    return {0: JW.scaled_qtable(JW.K1_LUMA, quality), 1: JW.scaled_qtable(JW.K1_CHROMA, quality)}


def _ycc(samp):
    return [JW.Component(1, *samp[0], 0, 0, 0), JW.Component(2, *samp[1], 1, 1, 1), JW.Component(3, *samp[2], 1, 1, 1)]


S444, S420 = ((1, 1), (1, 1), (1, 1)), ((2, 2), (1, 1), (1, 1))


def ycc(name, w, h, samp, quality=75, draw_kw=None, **kw):
    comps, q = _ycc(samp), _q(quality)
    return JW.write_jpeg(w, h, comps, draw(name, _rng(name), w, h, comps, q, **(draw_kw or {})), q, DC_K, AC_K, **kw)


def gray(name, w, h, hv=(1, 1), quality=75, draw_kw=None, **kw):
    comps, q = [JW.Component(1, *hv, 0, 0, 0)], _q(quality)
    return JW.write_jpeg(w, h, comps, draw(name, _rng(name), w, h, comps, q, **(draw_kw or {})), {0: q[0]},
                         {0: JW.K3_DC_LUMA}, {0: JW.K3_AC_LUMA}, **kw)


def four(name, w, h, samp, adobe, quality=85, draw_kw=None):
    """A four-component file (ids C, M, Y, K; one table set; an Adobe APP14 segment with transform `adobe`:
    0 = CMYK, 2 = YCCK) with components sampled samp[k] = (h, v)."""
    comps, q = [JW.Component(ord(c), *hv, 0, 0, 0) for c, hv in zip("CMYK", samp)], _q(quality)
    return JW.write_jpeg(w, h, comps, draw(name, _rng(name), w, h, comps, q, **(draw_kw or {})), {0: q[0]},
                         {0: JW.K3_DC_LUMA}, {0: JW.K3_AC_LUMA}, jfif=False, adobe=adobe)
